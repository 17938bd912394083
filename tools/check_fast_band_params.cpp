// check_fast_band_params.cpp -- the streaming encode kernels read BandParams as bytes: fastBandParams() and raiseCandidates()
// (codec_encode.cpp, on top of makeBandParams) must give, bit for bit, what the encoder's host filled in by hand before they existed.
// `before()` below is a transcription of that filling.  Host code only: linked against the emulator build's objects
// (make -C lerc_amd/csrc bandparams), run by tests/test_sim_encode_forms.py.
#include "codec.h"
#include "tile_fast.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

using namespace lerc;

static BandParams before(int dt, int nRows, int nCols, double maxZErr)
{
  const bool isFlt = dt >= DT_Float;
  BandParams bp;
  memset(&bp, 0, sizeof(bp));
  bp.nRows = nRows; bp.nCols = nCols; bp.nDepth = 1; bp.dt = dt; bp.version = kCodecVersion;
  bp.mb = 8; bp.nTV = (nRows + 7) / 8; bp.nTH = (nCols + 7) / 8;
  bp.allValid = 1;
  bp.maxQ = maxValToQuantize(dt);
  bp.maxZErr = isFlt ? maxZErr : std::max(0.5, floor(maxZErr));
  bp.scale = 1 / (2 * bp.maxZErr);
  bp.invScale = 2 * bp.maxZErr;
  bp.intLossless = (!isFlt && bp.maxZErr == 0.5) ? 1 : 0;
  return bp;
}

static u32 candidatesBefore(int dt, double maxZErr)
{
  u32 cand = 0;
  if (dt >= DT_Float)
  {
    static const double errCand[9] = { 1, 0.5, 0.1, 0.05, 0.01, 0.005, 0.001, 0.0005, 0.0001 };
    for (int c = 0; c < 9; c++) if (errCand[c] / 2 > maxZErr) cand |= 1u << c;
  }
  return cand;
}

int main()
{
  static const double bounds[7] = { 0, 0.5, 0.7, 1, 3.9, 0.01, 1e-6 };
  static const int shapes[3][2] = { { 64, 64 }, { 136, 200 }, { 257, 257 } };
  int nCompared = 0, nBad = 0;
  for (int dt = DT_Char; dt <= DT_Double; dt++)
    for (double e : bounds)
      for (const auto& s : shapes)
      {
        if (candidatesBefore(dt, e) != raiseCandidates(dt, e)) { printf("candidates differ: dt %d, maxZErr %g\n", dt, e); nBad++; }
        if (dt >= DT_Float && e == 0)
        {
          // (1 / (2 * 0) by hand, 0 from makeBandParams: the streaming path never fills parameters for such a request)
          if (fastEncodeEligible(dt, s[0], s[1], 1, false, e, true)) { printf("lossless float is eligible: dt %d\n", dt); nBad++; }
          continue;
        }
        const BandParams a = before(dt, s[0], s[1], e), b = fastBandParams(dt, s[0], s[1], e);
        nCompared++;
        if (memcmp(&a, &b, sizeof(BandParams)) != 0) { printf("BandParams differ: dt %d, %d x %d, maxZErr %g\n", dt, s[0], s[1], e); nBad++; }
      }
  printf("band params: %d compared, %d bad\n", nCompared, nBad);
  return nBad ? 1 : 0;
}
