// codec_encode_band.cpp -- the general band path of lerc_encode(): one band, stage by stage, on device-resident pixels.
//
// Host logic mirrors Lerc::EncodeInternal (Lerc.cpp:628-789: band loop, mask reuse, flags) and
// Lerc2::ComputeNumBytesNeededToWrite / Lerc2::Encode (Lerc2.cpp:179-480: mode decision, section
// order).  Every sweep over pixels is a HIP kernel; the host only sees a few scalars per band.
#include "codec.h"
#include "huffman.h"
#include "fpl.h"
#include "tile_fast.h"
#include <cfloat>
#include <functional>
#include <future>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>

namespace lerc {

namespace {

struct MaskState    // what the reference keeps inside its Lerc2 object between bands
{
  u32 fplStale = 0;    // bytes of lossless float planes that were coded but not written (see BandEncoder::price)
  bool allValid = true;
  int numValid = 0;
  u8* dBits = nullptr;          // device bit mask (valid when !allValid)
  std::vector<u8> hBits;        // host copy, for RLE and band-to-band comparison
};

}    // namespace

// ------------------------------------------------------------------------------------------------
// noData values: what Lerc::FilterNoDataAndNaN (float, Lerc.cpp:1378-1552) and its integer sibling (:1241-1374)
// decide once the sweep over the band (k_nodata_scan) is done.  In: the requested error bound and noData value;
// out: the bound to encode with, whether the blob has to carry a noData value, and the value it is remapped to.
// ------------------------------------------------------------------------------------------------
struct NoDataDecision
{
  bool active = false;       // this band came with a noData value
  bool needNoData = false;   // some valid pixels keep noData in some depths: the header carries the value
  bool allInt = false;       // float types: header flag bIsInt
  bool remap = false;
  double maxZErr = 0, noDataOrig = 0, noDataNew = 0, remapFrom = 0, remapTo = 0;
  const u8* dData = nullptr; // the filtered copy of the band
  const u8* dMask = nullptr; // ... and of its byte mask
  bool modifiedMask = false;
  bool empty = false;        // no value left at all
};

template<class T> static bool isIntValT(T z) { return z == (T)floor((double)z + 0.5); }    // Lerc.h:271

// Lerc.cpp:1558-1618
template<class T>
static bool findNoDataBelowMin(double minVal, double maxZErr, bool allInt, double lowIntLimit, T& out)
{
  std::vector<T> cand;
  if (allInt)
  {
    const double dist[] = { 4 * maxZErr, 1, 10, 100, 1000, 10000 };
    for (double d : dist) cand.push_back((T)(minVal - d));
    cand.push_back((T)(minVal > 0 ? floor(minVal / 2) : minVal * 2));
    std::sort(cand.begin(), cand.end(), std::greater<double>());
    for (T v : cand)
      if ((v > (T)lowIntLimit) && (v < (T)(minVal - 2 * maxZErr)) && isIntValT(v)) { out = v; return true; }
  }
  else
  {
    const double dist[] = { 4 * maxZErr, 0.0001, 0.001, 0.01, 0.1, 1, 10, 100, 1000, 10000 };
    for (double d : dist) cand.push_back((T)(minVal - d));
    cand.push_back((T)(minVal > 0 ? minVal / 2 : minVal * 2));
    std::sort(cand.begin(), cand.end(), std::greater<double>());
    const T lowest = (T)(std::is_same<T, float>::value ? -FLT_MAX : -DBL_MAX);
    for (T v : cand)
      if ((v > lowest) && (v < (T)(minVal - 2 * maxZErr))) { out = v; return true; }
  }
  return false;
}

template<class T>
static u32 decideNoDataFloat(const NoDataScan& sc, bool any, double minVal, double maxVal, int nDepth, double maxZErr, double noDataValue,
                             NoDataDecision& d)
{
  const bool isF32 = std::is_same<T, float>::value;
  const T origNoData = (T)noDataValue;
  const bool noDataLeft = (sc.flags & 2u) != 0;
  bool allInt = !(sc.flags & 8u);
  const double lowInt = isF32 ? -(double)(1L << 23) : -(double)((i64)1 << 53), highInt = -lowInt;
  d.maxZErr = maxZErr; d.noDataNew = noDataValue;
  if (!any) { d.empty = true; d.maxZErr = 0; return kOk; }
  d.needNoData = noDataLeft;
  (void)nDepth;
  double e = maxZErr;
  if (allInt)
  {
    allInt = allInt && (minVal >= lowInt) && (minVal <= highInt) && (maxVal >= lowInt) && (maxVal <= highInt);
    if (noDataLeft) allInt = allInt && isIntValT(origNoData) && (origNoData >= lowInt) && (origNoData <= highInt);
    if (allInt) e = std::max(0.5, floor(maxZErr));
  }
  d.allInt = allInt;
  if (e == 0) { d.maxZErr = maxZErr; return kOk; }
  {
    const double dist = allInt ? floor(e) : 2 * e;
    if ((origNoData >= minVal - dist) && (origNoData <= maxVal + dist)) { d.maxZErr = allInt ? 0.5 : 0; return kOk; }
  }
  if (noDataLeft)
  {
    T remap = origNoData;
    if (findNoDataBelowMin<T>(minVal, e, allInt, lowInt, remap))
    {
      if (remap != origNoData) { d.remap = true; d.remapFrom = (double)origNoData; d.remapTo = (double)remap; d.noDataNew = (double)remap; }
    }
    else if ((double)origNoData >= minVal) e = allInt ? 0.5 : 0;
  }
  d.maxZErr = e;
  return kOk;
}

template<class T>
static u32 decideNoDataInt(const NoDataScan& sc, bool any, double minVal, double maxVal, double lo, double hi, double maxZErr,
                           double noDataValue, NoDataDecision& d)
{
  const T orig = (T)noDataValue;
  d.needNoData = (sc.flags & 2u) != 0;
  d.noDataNew = noDataValue;
  double e = std::max(0.5, floor(maxZErr));
  const double dist = floor(e);
  if (!any) { d.empty = true; d.maxZErr = 0.5; return kOk; }
  if (((double)orig >= minVal - dist) && ((double)orig <= maxVal + dist)) { d.maxZErr = 0.5; return kOk; }
  if (d.needNoData)
  {
    const double minDist = floor(e) + 1;
    double remap = minVal - minDist;
    T nd = orig;
    if (remap >= lo) nd = (T)remap;
    else
    {
      e = 0.5;
      remap = minVal - 1;
      if (remap >= lo) nd = (T)remap;
      else
      {
        remap = maxVal + 1;
        if ((remap <= hi) && (remap < (double)orig)) nd = (T)remap;
      }
    }
    if (nd != orig) { d.remap = true; d.remapFrom = (double)orig; d.remapTo = (double)nd; d.noDataNew = (double)nd; }
  }
  d.maxZErr = e;
  return kOk;
}

// sweeps a private copy of band iBand and fills `d`; workspace comes from ctx (behind whatever is allocated so far)
static u32 filterNoData(Context& ctx, const EncodeRequest& rq, int iBand, NoDataDecision& d)
{
  hipStream_t st = ctx.activeStream();
  const int dt = rq.dt, nD = rq.nDepth;
  const int tb = dtSize(dt);
  const i64 nPix = (i64)rq.nRows * rq.nCols, nElem = nPix * nD;
  const double noData = rq.hNoDataValues[iBand];
  static const double tlo[6] = { -128, 0, -32768, 0, -2147483648.0, 0 }, thi[6] = { 127, 255, 32767, 65535, 2147483647.0, 4294967295.0 };
  if (dt == DT_Float && (noData < -FLT_MAX || noData > FLT_MAX)) return kWrongParam;
  if (dt < DT_Float && (noData < tlo[dt] || noData > thi[dt])) return kWrongParam;
  if (noData != noData) return kWrongParam;
  u8* dCopy = ctx.allocT<u8>((size_t)nElem * tb + 256);
  u8* dMask = ctx.allocT<u8>((size_t)nPix + 256);
  NoDataScan* dScan = ctx.allocT<NoDataScan>(1);
  if (!dCopy || !dMask || !dScan) return kFailed;
  const u8* src = (const u8*)rq.dData + (size_t)iBand * nElem * tb;
  hipMemcpyAsync(dCopy, src, (size_t)nElem * tb, hipMemcpyDeviceToDevice, st);
  if (rq.nMasks > 0) hipMemcpyAsync(dMask, rq.dValidBytes + ((rq.nMasks > 1) ? (size_t)iBand * nPix : 0), (size_t)nPix, hipMemcpyDeviceToDevice, st);
  else hipMemsetAsync(dMask, 1, (size_t)nPix, st);
  launchNoDataScan(dt, dCopy, dMask, nPix, nD, noData, dScan, st);
  NoDataScan sc;
  hipMemcpyAsync(&sc, dScan, sizeof(sc), hipMemcpyDeviceToHost, st);
  if (hipStreamSynchronize(st) != hipSuccess) return kFailed;
  const bool any = sc.minKey != statKeyInitMin() || sc.maxKey != statKeyInitMax();
  const double minVal = any ? statKeyToDouble(dt, sc.minKey) : 0, maxVal = any ? statKeyToDouble(dt, sc.maxKey) : 0;
  d = NoDataDecision();
  d.active = true; d.noDataOrig = noData; d.dData = dCopy; d.dMask = dMask; d.modifiedMask = (sc.flags & 4u) != 0;
  u32 rc = kOk;
  switch (dt)
  {
    case DT_Float:  rc = decideNoDataFloat<float>(sc, any, minVal, maxVal, nD, rq.maxZErr, noData, d); break;
    case DT_Double: rc = decideNoDataFloat<double>(sc, any, minVal, maxVal, nD, rq.maxZErr, noData, d); break;
    case DT_Char:   rc = decideNoDataInt<signed char>(sc, any, minVal, maxVal, tlo[dt], thi[dt], rq.maxZErr, noData, d); break;
    case DT_Byte:   rc = decideNoDataInt<unsigned char>(sc, any, minVal, maxVal, tlo[dt], thi[dt], rq.maxZErr, noData, d); break;
    case DT_Short:  rc = decideNoDataInt<short>(sc, any, minVal, maxVal, tlo[dt], thi[dt], rq.maxZErr, noData, d); break;
    case DT_UShort: rc = decideNoDataInt<unsigned short>(sc, any, minVal, maxVal, tlo[dt], thi[dt], rq.maxZErr, noData, d); break;
    case DT_Int:    rc = decideNoDataInt<int>(sc, any, minVal, maxVal, tlo[dt], thi[dt], rq.maxZErr, noData, d); break;
    default:        rc = decideNoDataInt<unsigned int>(sc, any, minVal, maxVal, tlo[dt], thi[dt], rq.maxZErr, noData, d); break;
  }
  if (rc != kOk) return rc;
  if (d.remap) launchNoDataRemap(dt, dCopy, dMask, nullptr, nPix, nD, d.remapFrom, d.remapTo, st);
  return kOk;
}

namespace {

// LERC_AMD_MASKED_STREAMING=0: masked bands keep the general kernels for their block stream (a test / tuning knob)
bool maskedStreamingOn()
{
  static const bool on = []() { const char* e = getenv("LERC_AMD_MASKED_STREAMING"); return !(e && atoi(e) == 0); }();
  return on;
}

// ------------------------------------------------------------------------------------------------
// the decisions that are arithmetic over what the statistics kernels brought home
// ------------------------------------------------------------------------------------------------
// TryRaiseMaxZError's candidates (Lerc2.cpp:1244-1253): error bounds that beat the request ...
const double errCand[9] = { 1, 0.5, 0.1, 0.05, 0.01, 0.005, 0.001, 0.0005, 0.0001 };
const int facCand[9] = { 1, 2, 10, 20, 100, 200, 1000, 2000, 10000 };

u32 raiseCandidates(double maxZErr)
{
  u32 cand = 0;
  for (int c = 0; c < 9; c++) if (errCand[c] / 2 > maxZErr) cand |= 1u << c;
  return cand;
}
// ... those of `cand` whose rounding errors `raiseErr` (over the first row, or the band) stay within the request
u32 raiseSurvivors(u32 cand, const double* raiseErr, double maxZErr)
{
  for (int c = 0; c < 9; c++)
    if (((cand >> c) & 1u) && raiseErr[c] / facCand[c] > maxZErr / 2) cand &= ~(1u << c);
  return cand;
}
// ... and the bound the band is coded with: that of the first survivor
double raisedMaxZErr(u32 cand, const double* raiseErr, double maxZErr)
{
  for (int c = 0; c < 9; c++)
    if (((cand >> c) & 1u) && raiseErr[c] / facCand[c] <= maxZErr / 2) return errCand[c] / 2;
  return maxZErr;
}

// bit plane mode (Lerc2::TryBitPlaneCompression, Lerc2.cpp:1071-1229): drop the low bit planes whose XOR with
// the neighbours looks like coin flips (|1 - 2 p| < eps); lossless (0) whenever the statistics are inconclusive.
// counts: [nD][32] set bits per plane, then the number of pixel pairs looked at
double bitPlaneMaxZErr(const std::vector<u32>& counts, int nD, int nBits, double eps)
{
  const int minCnt = 5000;
  const double cnt = (double)counts[(size_t)nD * 32];
  if (cnt < minCnt) return 0;
  int nCut = 0, lastKept = 0;
  for (int s2 = nBits - 1; s2 >= 0; s2--)
  {
    bool crit = true;
    for (int m = 0; m < nD; m++)
      if (fabs(1 - 2 * ((double)counts[(size_t)m * 32 + s2] / cnt)) >= eps) crit = false;
    if (crit && nCut < 2)
    {
      if (nCut == 0) lastKept = s2;
      if (nCut == 1 && s2 < lastKept - 1) { lastKept = s2; nCut = 0; }
      nCut++;
    }
  }
  lastKept = std::max(0, lastKept);
  return (double)((1 << lastKept) >> 1);
}

// ------------------------------------------------------------------------------------------------
// The mask on its way home.  A single band's bits travel to pinned host memory as soon as they are final, and a helper thread
// codes their RLE (a millisecond for the 8 MB of an 8192 x 8192 mask) while the calling thread goes on launching and waiting for
// kernels -- or, a large mask (deviceRleFrom()): it is coded on the device (rle_kernels.hip), the bits never leave it, the stream's
// size and its first kRleFirst bytes travel home beside the statistics kernels, and code() picks them up.
// ------------------------------------------------------------------------------------------------
struct MaskTransit
{
  static const u32 kRleCap = 4u << 20, kRleFirst = 64u << 10;
  const u8* bitsOnTheWay = nullptr;    // pinned
  size_t nBitsOnTheWay = 0;
  std::future<std::vector<u8> > rleFuture;
  bool deviceRle = false;
  u8* dRle = nullptr;
  u32* pinRle = nullptr;        // [0]: the stream's size (~0: it did not fit kRleCap), from byte 16 on: its first kRleFirst bytes
  size_t nBitsOnDevice = 0;
  bool coded = false;
  std::vector<u8> rle;          // what code() made: the band's mask section (empty: the band writes none)

  bool away() const { return bitsOnTheWay || deviceRle; }
  size_t nBytes() const { return bitsOnTheWay ? nBitsOnTheWay : nBitsOnDevice; }
  bool send(Context& ctx, hipStream_t st, const u8* dNewBits, size_t nb);
  // wanted: the band writes a mask.  (Called with kernels in flight where there are any: the RLE of 8 MB of bits takes the host a millisecond)
  bool code(Context& ctx, bool wanted, const u8* dNewBits, std::vector<u8>& hBits);
};

bool MaskTransit::send(Context& ctx, hipStream_t st, const u8* dNewBits, size_t nb)
{
  if (nb >= deviceRleFrom() && nb < 0xFFFFFFF0ull)
  {
    u8* scratch = ctx.allocT<u8>(maskRleScratchBytes(nb));
    dRle = ctx.allocT<u8>((size_t)kRleCap + 64);
    u32* dSize = ctx.allocT<u32>(4);
    pinRle = (u32*)ctx.pinnedAux((size_t)kRleCap + 64);
    if (scratch && dRle && dSize && pinRle)
    {
      hipStream_t side = ctx.forkSide();
      hipStream_t sr = side ? side : st;
      ProfScope ps(ctx, "mask_rle");
      launchMaskRle(dNewBits, (u32)nb, dRle, kRleCap, dSize, scratch, sr);
      hipMemcpyAsync(pinRle, dSize, 4, hipMemcpyDeviceToHost, sr);
      hipMemcpyAsync((u8*)pinRle + 16, dRle, kRleFirst, hipMemcpyDeviceToHost, sr);
      hipEventRecord(ctx.auxEvent(), sr);
      deviceRle = true; nBitsOnDevice = nb;
      return true;
    }
  }
  u8* pin = (u8*)ctx.pinnedAux(nb);
  if (!pin) return false;
  // (beside the stream, so that the statistics kernels do not wait behind 8 MB on their way over PCIe: a third of a millisecond)
  hipStream_t side = nb >= (256u << 10) ? ctx.forkSide() : nullptr;
  hipEvent_t ev = ctx.auxEvent();
  hipMemcpyAsync(pin, dNewBits, nb, hipMemcpyDeviceToHost, side ? side : st);
  hipEventRecord(ev, side ? side : st);
  bitsOnTheWay = pin; nBitsOnTheWay = nb;
  if (nb < (256u << 10)) return true;    // small masks: code() does it in line (starting a thread costs ~30 us)
  try
  {
    rleFuture = std::async(std::launch::async, [pin, nb, ev]()
    {
      std::vector<u8> out;
      const auto t0 = std::chrono::steady_clock::now();
      // (the workers are started now, while the bits travel, and wait for them one by one)
      if (!rleEncodeWhenReady(pin, nb, [ev]() { return hipEventSynchronize(ev) == hipSuccess; }, out)) out.clear();
      if (getenv("LERC_AMD_HOST_TIMES")) fprintf(stderr, "  [tl] helper: %zu -> %zu bytes, %.1f us after its start\n", nb, out.size(), std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
      return out;    // (empty: the copy failed; an RLE stream is never empty)
    });
  }
  catch (...) { rleFuture = std::future<std::vector<u8> >(); }    // no thread to be had: code() codes the mask in line
  return true;
}

bool MaskTransit::code(Context& ctx, bool wanted, const u8* dNewBits, std::vector<u8>& hBits)
{
  if (coded) return true;
  coded = true;
  // (the helper must be through in any case: the pinned area takes the blob's prefix next)
  bool helped = rleFuture.valid();
  if (helped) { rle = rleFuture.get(); if (rle.empty()) return false; }
  else if (away() && hipEventSynchronize(ctx.auxEvent()) != hipSuccess) return false;
  if (!wanted) { rle.clear(); return true; }
  if (deviceRle)
  {
    const u32 size = pinRle[0];
    if (size != 0xFFFFFFFFu && size >= 2u && size <= kRleCap)
    {
      if (size > kRleFirst)    // (a mask with many short runs: the rest of its stream)
      {
        if (hipMemcpy((u8*)pinRle + 16 + kRleFirst, dRle + kRleFirst, size - kRleFirst, hipMemcpyDeviceToHost) != hipSuccess) return false;
      }
      rle.assign((const u8*)pinRle + 16, (const u8*)pinRle + 16 + size);
      helped = true;
    }
    else
    {
      // (a mask that hardly compresses: its bits come home after all, and the host codes them)
      hBits.resize(nBitsOnDevice);
      if (hipMemcpy(hBits.data(), dNewBits, nBitsOnDevice, hipMemcpyDeviceToHost) != hipSuccess) return false;
    }
  }
  if (!helped)
  {
    if (bitsOnTheWay) rleEncode(bitsOnTheWay, nBitsOnTheWay, rle);
    else rleEncode(hBits.data(), hBits.size(), rle);
  }
  return true;
}

// ------------------------------------------------------------------------------------------------
// One band of the general path.  The members are what the stages hand to each other; encodeBand() below is their order.
// ------------------------------------------------------------------------------------------------
const u32 kStatsWords = (u32)(sizeof(BandStats) / 4);
static_assert(sizeof(BandStats) % 4 == 0, "words");

struct WordSrc { const void* d; u32 n; };    // n words of device memory (n == 0: left out)
struct WordCursor    // over what a statistics round gathered in pinned memory, in the order of its sources
{
  const u32* p = nullptr;
  template<class T> void take(T* dst, u32 nWords) { memcpy(dst, p, (size_t)nWords * 4); p += nWords; }
};

struct BandEncoder
{
  // ---- the call
  Context& ctx;
  const EncodeRequest& rq;
  const int iBand;
  MaskState& ms;
  u8* const dBandOut;         // nullptr: a size query
  const u32 capacityLeft;
  const hipStream_t st;
  const std::chrono::steady_clock::time_point tl0 = std::chrono::steady_clock::now();
  // ---- geometry
  const int dt, tb, nD, nRows, nCols;
  const i64 nPix, nElem;
  const bool isFlt;
  const int nPos8;
  const u8* dData;
  const u8* dByteMask;
  NoDataDecision nd;          // a noData value: the band is filtered into a private copy first, and the decisions come from that filter
  // ---- device scratch of this band
  DeviceStatus* dStatus = nullptr;
  BandStats* dStats = nullptr;
  BandStats* dStatsRow0 = nullptr;    // (the first row's TryRaiseMaxZError errors, measured beside the mask's statistics)
  u64* dMins = nullptr;
  u64* dMaxs = nullptr;
  u8* dNewBits = nullptr;
  // ---- the statistics' host copy
  struct HostRes { BandStats stats; BandStats row0; } hr = {};
  std::vector<u64> hMins, hMaxs;
  u32* statsPin = nullptr;    // where the round in flight gathers
  bool bandAllValid = true;
  int bandNumValid;
  bool haveBits = false;      // dNewBits holds this band's bit mask
  bool maskStats = false;     // the mask's kernel has made the band's statistics as well (launchMaskStats)
  bool row0Measured = false;
  bool nanSeen = false, mixedNaN = false;
  const u32 candAll;          // TryRaiseMaxZError's candidates, before the first row prunes them
  // ---- the mask on its way home
  MaskTransit transit;
  // ---- the speculated 8-bit pricing.  8-bit values without a mask, lossless: what the choice between tiling and Huffman coding is
  // made from -- the sizes of the 8 x 8 blocks and the two histograms -- depends on nothing the statistics decide, so both are enqueued
  // right behind the statistics kernel and arrive with the same wait (every wait costs the stream ~50 us of idling)
  struct Speculated
  {
    bool on = false, sizesFresh = false;
    u32* dSizes = nullptr; u32* dOffsets = nullptr; u32* dScratch = nullptr;
    u32* dHisto = nullptr; const u32* dTotal = nullptr;
    u32 total = 0;
    u32 histo[512];
    BandParams bp;
  } spec;
  const bool specWanted;
  // ---- the decisions
  Header hd;
  BandParams bp;
  double maxZErr;
  u32 raiseMask = 0;
  bool allInt = false;
  bool encMask = false;       // this band writes its mask
  const u8* dBits = nullptr;  // the mask in force (ms.dBits), nullptr: every pixel valid
  int numValid = 0;           // ... and its count
  std::vector<double> zMinVec, zMaxVec;
  // ---- the sizing result
  enum Payload { P_NONE, P_TILING, P_ONESWEEP, P_HUFFMAN, P_FLOAT } payload = P_NONE;
  int imageMode = IEM_Tiling;
  u32 nBytesData = 0, blobSize = 0;
  HuffmanPlan huff;
  FplPlan fpl;
  u32 fplPlanes = 0;          // bytes of this band's coded planes, if they were made
  bool writeRanges = false;
  u32* dSizes = nullptr;
  u32* dOffsets = nullptr;
  u32* dScratch = nullptr;
  // A band with a validity mask, one value per pixel, a type of 16 bits or more: its block stream is made by
  // the one-launch encoder's masked form (tile_fast.hip) -- straight into the band's place behind mask and ranges, with the band's
  // FINAL parameters, all decisions about the band having been made -- instead of tile_sizes + scan + tile_write.  If the band
  // ends up coded another way (16 x 16 blocks, one sweep) that writer comes later in the stream and overwrites it.
  // dStreamed: that stream is in place; a launch that gave up waiting (never seen) leaves the band to the three kernels.
  u8* dStreamed = nullptr;
  u32 nBytesStreamed = 0, streamSums = 0;    // (streamSums: the stream's Fletcher terms, which the kernel collects as it writes)
  bool streamedTried = false;
  // ---- emit
  u8* dPayload = nullptr;

  BandEncoder(Context& c, const EncodeRequest& r, int band, MaskState& m, u8* dOut, u32 capLeft)
    : ctx(c), rq(r), iBand(band), ms(m), dBandOut(dOut), capacityLeft(capLeft), st(c.activeStream()),
      dt(r.dt), tb(dtSize(r.dt)), nD(r.nDepth), nRows(r.nRows), nCols(r.nCols), nPix((i64)r.nRows * r.nCols), nElem(nPix * r.nDepth),
      isFlt(r.dt >= DT_Float), nPos8(((r.nRows + 7) / 8) * ((r.nCols + 7) / 8)),
      dData((const u8*)r.dData + (size_t)band * nElem * tb),
      dByteMask((r.nMasks > 0) ? r.dValidBytes + ((r.nMasks > 1) ? (size_t)band * nPix : 0) : nullptr),
      hMins(r.nDepth), hMaxs(r.nDepth), bandNumValid((int)nPix),
      candAll((isFlt && r.maxZErr > 0) ? raiseCandidates(r.maxZErr) : 0u),
      specWanted(!isFlt && tb == 1 && !dByteMask && !(r.hUsesNoData && r.hUsesNoData[band]) && r.maxZErr >= 0 && r.maxZErr < 1 && r.version >= 4
                 && (r.nRows > 8 || r.nCols > 8)),
      maxZErr(r.maxZErr) {}

  bool wait() const { return hipStreamSynchronize(st) == hipSuccess; }
  // (LERC_AMD_HOST_TIMES: where the host is, microseconds into the band -- a tuning aid)
  void TL(const char* what) const
  {
    static const bool kTL = getenv("LERC_AMD_HOST_TIMES") != nullptr;
    if (kTL) fprintf(stderr, "  [tl] %8.1f us  %s\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tl0).count(), what);
  }
  const u8* bandBits() const { return (haveBits && !bandAllValid) ? dNewBits : nullptr; }
  void blocksOf(int mb) { bp.mb = mb; bp.nTV = (nRows + mb - 1) / mb; bp.nTH = (nCols + mb - 1) / mb; }

  // the stages, in their order
  u32 begin();
  u32 validity();
  u32 statistics();
  u32 maskAcrossBands(std::vector<u8>& prevByteValid, bool& anyMaskModified);
  u32 decide();
  u32 price(u32& bandBytes);
  u32 emit();
  u32 seal();

  // what they are made of
  bool statsBegin(u32 pinWords, u32* dZeroToo, u32 nZeroToo);
  bool statsEnd(const WordSrc (&src)[5], WordCursor& w);
  bool makeBits();
  bool runStats(int rows, u32 mask);
  void speculate();
  bool codeMask();
  bool streamMasked();
  bool tilingBytes(int mb, u32& total);
  u32 priceModes();
};

// One kernel sets the statistics kernels' inputs, one gathers their results -- and what was enqueued ahead of the decisions: the
// two histograms, the blocks' total size -- in pinned memory the host reads after its wait: between the kernels of a band no
// copy command of a few bytes, and none into pageable memory (each keeps this thread until the stream has reached it).
bool BandEncoder::statsBegin(u32 pinWords, u32* dZeroToo, u32 nZeroToo)
{
  statsPin = (u32*)ctx.pinned((size_t)(pinWords + 16u) * 4u);
  if (!statsPin) return false;
  launchStatsInit(dMins, dMaxs, nD, reinterpret_cast<u32*>(dStats), kStatsWords, dZeroToo, nZeroToo, st);
  return true;
}

bool BandEncoder::statsEnd(const WordSrc (&src)[5], WordCursor& w)
{
  const u32* from[5];
  u32 nw[5];
  for (int i = 0; i < 5; i++) { nw[i] = src[i].n; from[i] = src[i].n ? reinterpret_cast<const u32*>(src[i].d) : nullptr; }
  launchWordsGather(from, nw, statsPin, st);
  if (!wait()) return false;
  w.p = statsPin;
  return true;
}

// the band's validity bits and their count; where the band qualifies, its statistics in the same read (they stand if no
// TryRaiseMaxZError candidate survives the first row), and that row measured in the same wait (every wait costs the stream ~50 us of idling)
bool BandEncoder::makeBits()
{
  if (!statsBegin(2u * kStatsWords + 4u, candAll ? reinterpret_cast<u32*>(dStatsRow0) : nullptr, candAll ? kStatsWords : 0u)) return false;
  maskStats = false;
  if (dByteMask && !nd.active) { ProfScope ps(ctx, "mask_stats"); maskStats = launchMaskStats(dt, dData, dByteMask, nRows, nCols, nD, dNewBits, dMins, dMaxs, dStats, st); }
  if (!maskStats) { ProfScope ps(ctx, "build_mask"); launchBuildMask(dt, dData, dByteMask, nRows, nCols, nD, dNewBits, dStats, st); }
  row0Measured = false;
  if (candAll)
  {
    { ProfScope ps(ctx, "band_stats_row0"); launchBandStats(dt, dData, dNewBits, 1, nCols, nD, candAll, dMins, dMaxs, dStatsRow0, st); }    // (with the bits just made: all ones if nothing is invalid)
    row0Measured = true;
  }
  const WordSrc src[5] = { { dStats, kStatsWords }, { dStatsRow0, candAll ? kStatsWords : 0u }, { dMins, maskStats ? 2u : 0u }, { dMaxs, maskStats ? 2u : 0u }, { nullptr, 0u } };
  WordCursor w;
  if (!statsEnd(src, w)) return false;
  w.take(&hr.stats, kStatsWords);
  if (candAll) w.take(&hr.row0, kStatsWords);
  if (maskStats) { w.take(hMins.data(), 2); w.take(hMaxs.data(), 2); }
  bandNumValid = (int)hr.stats.numValid;
  bandAllValid = (bandNumValid == (int)nPix);
  haveBits = true;
  if (rq.nBands == 1 && !bandAllValid && bandNumValid > 0 && ctx.auxEvent() && !transit.send(ctx, st, dNewBits, (size_t)((nPix + 7) >> 3))) return false;
  return true;
}

void BandEncoder::speculate()
{
  spec.dSizes = ctx.allocT<u32>((size_t)nPos8 + 4);
  spec.dOffsets = ctx.allocT<u32>((size_t)nPos8 + 4);
  spec.dScratch = ctx.allocT<u32>((size_t)nPos8 / 1024 + 8);
  if (!spec.dSizes || !spec.dOffsets || !spec.dScratch) return;
  BandParams& b = spec.bp;
  b = makeBandParams(dt, nRows, nCols, nD, rq.version, 8, 0.5, true);
  b.intLossless = 1;
  b.tryDiff = (rq.version >= 5 && nD > 1) ? 1 : 0;
  { ProfScope ps(ctx, "tile_sizes"); launchTileSizes(dt, 8, dData, nullptr, b, spec.dSizes, dStatus, st); }
  { ProfScope ps(ctx, "scan_block_sizes"); launchExclusiveScan(spec.dSizes, spec.dOffsets, (u32)nPos8, spec.dScratch, st); }
  enqueueHuffmanHistoDevice(ctx, dt, dData, nullptr, nRows, nCols, nD, spec.dHisto);    // (zeroed by runStats; the counts and the total come home with the statistics)
  spec.dTotal = spec.dOffsets + nPos8;
  spec.on = spec.sizesFresh = true;
}

bool BandEncoder::runStats(int rows, u32 mask)
{
  const bool specNow = specWanted && rows == nRows && !spec.on && !haveBits;
  if (specNow && !spec.dHisto) spec.dHisto = ctx.allocT<u32>(512);
  const u32 wKeys = 2u * (u32)nD;
  if (!statsBegin(kStatsWords + 2u * wKeys + 512u, (specNow && spec.dHisto) ? spec.dHisto : nullptr, (specNow && spec.dHisto) ? 512u : 0u)) return false;
  { ProfScope ps(ctx, rows == nRows ? "band_stats" : "band_stats_row0"); launchBandStats(dt, dData, bandBits(), rows, nCols, nD, mask, dMins, dMaxs, dStats, st); }
  if (specNow && spec.dHisto) speculate();
  const bool specHome = spec.on && specNow;
  const WordSrc src[5] = { { dStats, kStatsWords }, { dMins, wKeys }, { dMaxs, wKeys }, { spec.dHisto, specHome ? 512u : 0u }, { spec.dTotal, specHome ? 1u : 0u } };
  WordCursor w;
  if (!statsEnd(src, w)) return false;
  w.take(&hr.stats, kStatsWords);
  w.take(hMins.data(), wKeys);
  w.take(hMaxs.data(), wKeys);
  if (specHome) { w.take(spec.histo, 512); w.take(&spec.total, 1); }
  return true;
}

// the noData filter and the band's scratch
u32 BandEncoder::begin()
{
  if (rq.hUsesNoData && rq.hUsesNoData[iBand])
  {
    const u32 rc = filterNoData(ctx, rq, iBand, nd);
    if (rc != kOk) return rc;
    dData = nd.dData;
    dByteMask = nd.dMask;
  }
  dStatus = ctx.allocT<DeviceStatus>(1);
  dStats = ctx.allocT<BandStats>(1);
  dStatsRow0 = ctx.allocT<BandStats>(1);
  dMins = ctx.allocT<u64>(nD);
  dMaxs = ctx.allocT<u64>(nD);
  dNewBits = ctx.allocT<u8>((size_t)((nPix + 7) >> 3) + 16);
  if (!dStatus || !dStats || !dStatsRow0 || !dMins || !dMaxs || !dNewBits) return kFailed;
  hipMemsetAsync(dStatus, 0, sizeof(DeviceStatus), st);
  hipMemsetAsync(dStats, 0, sizeof(BandStats), st);
  return kOk;
}

// ---- 1. validity: caller's byte mask, minus pixels that are NaN in every depth (Lerc.cpp:1440-1476)
u32 BandEncoder::validity()
{
  if (!dByteMask) return kOk;
  if (!makeBits()) return kFailed;
  nanSeen = hr.stats.hasNaN != 0;
  mixedNaN = hr.stats.mixedNaN != 0;
  return kOk;
}

// ---- 2. statistics: per-depth min / max; float: NaN, all-integer, TryRaiseMaxZError candidates
u32 BandEncoder::statistics()
{
  // candidates whose error bound beats the request (Lerc2.cpp:1244-1253), pruned on the first row the
  // way the reference prunes after every row (:1277); survivors are then measured over the whole band
  if (candAll)
  {
    if (!row0Measured)
    {
      if (!runStats(1, candAll)) return kFailed;
      hr.row0 = hr.stats;
    }
    raiseMask = raiseSurvivors(candAll, hr.row0.raiseErr, maxZErr);
  }
  // (statistics that came with the mask stand: range, "not all integers", NaN -- if no candidate asks for more)
  if (bandNumValid > 0 && !(maskStats && raiseMask == 0u && haveBits))
  {
    if (!runStats(nRows, raiseMask)) return kFailed;
    if (isFlt && hr.stats.hasNaN && !haveBits)
    {
      // NaNs present and no mask yet: derive the mask (NaN in every depth -> invalid) and redo the stats
      if (!makeBits()) return kFailed;
      nanSeen = true;
      mixedNaN = hr.stats.mixedNaN != 0;
      if (bandNumValid > 0 && !runStats(nRows, raiseMask)) return kFailed;
    }
  }
  if (isFlt && nanSeen && mixedNaN && nD > 1)
  {
    if (rq.version >= 6) return kNaN;    // Lerc.cpp:1498-1501 (no noData value to stand in)
    ctx.lastError = "codec < 6 with NaN in some depths of a pixel only (-FLT_MAX stand-ins) is not built";
    return kFailed;
  }
  return kOk;
}

// ---- 3. mask bookkeeping across bands (Lerc.cpp:717-741)
u32 BandEncoder::maskAcrossBands(std::vector<u8>& prevByteValid, bool& anyMaskModified)
{
  std::vector<u8> hBandBits;
  if (haveBits && !bandAllValid && !transit.away())
  {
    const size_t nb = (size_t)((nPix + 7) >> 3);
    hBandBits.resize(nb);
    u8* pin = (u8*)ctx.pinned(nb);    // (a pageable target costs a staging copy at ~1 GB/s)
    if (!pin) return kFailed;
    hipMemcpyAsync(pin, dNewBits, nb, hipMemcpyDeviceToHost, st);
    if (!wait()) return kFailed;
    memcpy(hBandBits.data(), pin, nb);
  }
  if (nanSeen || nd.modifiedMask) anyMaskModified = true;    // (NaN: conservative, the reference only flags bands whose mask really changed)
  encMask = (iBand == 0);
  {
    // the reference compares the (filtered) byte masks of consecutive bands; validity bits are equivalent
    const bool compare = (rq.nMasks > 1) || anyMaskModified;    // (an empty vector == all valid)
    if (compare && iBand > 0 && hBandBits != prevByteValid) encMask = true;
    if (rq.nBands > 1 && iBand < rq.nBands - 1) prevByteValid = hBandBits;
  }
  if (encMask)
  {
    ms.allValid = bandAllValid;
    ms.numValid = bandNumValid;
    const size_t nMaskBytes = transit.away() ? transit.nBytes() : hBandBits.size();
    ms.hBits = std::move(hBandBits);    // (megabytes for a large raster: moved, not copied)
    if (!bandAllValid)
    {
      if (!ms.dBits) return kFailed;
      hipMemcpyAsync(ms.dBits, dNewBits, nMaskBytes, hipMemcpyDeviceToDevice, st);
    }
  }
  dBits = ms.allValid ? nullptr : ms.dBits;
  numValid = ms.numValid;
  return kOk;
}

// ---- 4. what Lerc::FilterNoDataAndNaN + Lerc2::ComputeNumBytesNeededToWrite decide from the stats: header fields, the final maxZErr
u32 BandEncoder::decide()
{
  hd.version = rq.version;
  const bool oldCodec = rq.version < 6;    // Lerc::EncodeInternal_v5 (Lerc.cpp:526-624): no all-integer promotion, no noData
  hd.nRows = nRows; hd.nCols = nCols; hd.nDepth = nD; hd.numValid = numValid; hd.dt = dt;
  hd.nBlobsMore = rq.nBands - 1 - iBand;
  zMinVec.assign(nD, 0); zMaxVec.assign(nD, 0);
  if (bandNumValid > 0)
    for (int m = 0; m < nD; m++) { zMinVec[m] = statKeyToDouble(dt, hMins[m]); zMaxVec[m] = statKeyToDouble(dt, hMaxs[m]); }
  if (isFlt && !oldCodec)
  {
    if (bandNumValid == 0) maxZErr = 0;    // "tile has no valid data" (Lerc.cpp:1479-1484)
    else
    {
      const double lo = *std::min_element(zMinVec.begin(), zMinVec.end());
      const double hi = *std::max_element(zMaxVec.begin(), zMaxVec.end());
      const double lim = (dt == DT_Float) ? (double)(1L << 23) : (double)((i64)1 << 53);
      allInt = !hr.stats.notAllInt && lo >= -lim && lo <= lim && hi >= -lim && hi <= lim;
      if (allInt) maxZErr = std::max(0.5, floor(maxZErr));
    }
    if (nd.active) { allInt = nd.allInt; maxZErr = nd.maxZErr; }    // decided by the noData filter (it knows the original values)
    hd.isInt = allInt ? 1 : 0;
  }
  else if (nd.active) maxZErr = nd.maxZErr;
  hd.passNoData = nd.needNoData ? 1 : 0;
  hd.noDataVal = nd.needNoData ? nd.noDataNew : 0;
  hd.noDataValOrig = nd.needNoData ? nd.noDataOrig : 0;
  if (maxZErr == 777) maxZErr = -0.01;    // Lerc2.cpp:210-211
  if (!isFlt)
  {
    if (maxZErr < 0)
    {
      const double eps = -maxZErr;
      maxZErr = 0;
      if (bandNumValid >= 5000)
      {
        u32* dCounts = ctx.allocT<u32>((size_t)nD * 32 + 1);
        if (!dCounts) return kFailed;
        std::vector<u32> hCounts((size_t)nD * 32 + 1);
        { ProfScope ps(ctx, "bitplane_counts"); launchBitPlaneCounts(dt, dData, bandBits(), nRows, nCols, nD, dCounts, st); }
        hipMemcpyAsync(hCounts.data(), dCounts, hCounts.size() * 4, hipMemcpyDeviceToHost, st);
        if (!wait()) return kFailed;
        maxZErr = bitPlaneMaxZErr(hCounts, nD, 8 * tb, eps);
      }
    }
    maxZErr = std::max(0.5, floor(maxZErr));
  }
  else
  {
    if (maxZErr < 0) return kFailed;
    if (maxZErr > 0 && raiseMask && !allInt && numValid > 0)    // (numValid: Lerc2.cpp:1236)
      maxZErr = raisedMaxZErr(raiseMask, hr.stats.raiseErr, maxZErr);
  }
  TL("statistics read, decisions made");
  hd.maxZErr = maxZErr;
  hd.zMin = hd.zMax = 0;
  hd.mbSize = 8;
  bp = makeBandParams(dt, nRows, nCols, nD, hd.version, 8, maxZErr, ms.allValid);
  bp.intLossless = (!isFlt && maxZErr == 0.5) ? 1 : 0;
  bp.tryDiff = (hd.version >= 5 && nD > 1 && bp.intLossless) ? 1 : 0;
  return kOk;
}

bool BandEncoder::codeMask()
{
  if (transit.coded) return true;
  const bool needMask = numValid > 0 && numValid < (int)nPix;
  if (!transit.code(ctx, needMask && encMask, dNewBits, ms.hBits)) return false;
  blobSize += (u32)transit.rle.size();
  return true;
}

bool BandEncoder::streamMasked()    // false: an error (not: "not applicable")
{
  if (streamedTried) return true;
  streamedTried = true;
  const bool eligible = maskedStreamingOn() && dBits && !bp.allValid && nD == 1 && hd.version == kCodecVersion
    && dt != DT_Char && dt != DT_Byte && !hd.tryHuffmanInt() && !hd.tryHuffmanFlt() && !nd.active && !bp.tryDiff && fastEncodeOneLaunch() && fastDimsOkRagged(nRows, nCols)
    && ((uintptr_t)dData & 15) == 0 && (!dBandOut || ((uintptr_t)dBandOut & 15) == 0) && (u64)nPix * tb + (u64)nPos8 + 8192 < 0xFFFFFFFFull;
  if (!eligible) return true;
  TL("streamMasked: before codeMask");
  if (!codeMask()) return false;
  TL("streamMasked: mask coded");    // (the mask's length says where the block stream begins; the statistics kernels have covered its coding)
  const u32 nWGt = fastFusedNumWG(dt, nRows, nCols);
  const size_t cellWords = fastFusedCellWords(nWGt), counterWords = fastFusedCounterWords(nWGt);
  const u64 cap = capacityLeft;
  const u32 payloadAt = (u32)(headerBytes(hd.version) + 4 + transit.rle.size() + 2 * (size_t)tb + 1);    // header, mask, ranges, "not one sweep"
  u8* cells = ctx.persistentState(1, cellWords * 8 + 256);
  u8* counters = ctx.persistentState(0, counterWords * 8 + 256);
  u8* dWs = dBandOut;    // (a size query: no payloads, no stores)
  FastEncodeResult* dRes = ctx.allocT<FastEncodeResult>(1);
  FastEncodeResult* hRes = (FastEncodeResult*)ctx.pinned(sizeof(FastEncodeResult));
  if (!cells || !counters || !dRes || !hRes) return false;
  FastEncodeBuffers fb;
  memset(&fb, 0, sizeof(fb));
  const u32 nG = fastFusedGroups(nWGt), nPG = fastPackGroups(nWGt);
  FastFused& f = fb.fused;
  f.sizeCell = (u64*)cells; f.baseCell = f.sizeCell + nWGt; f.totalCell = f.baseCell + nG; f.raise = f.totalCell + nG;
  f.packPart = (u64*)counters; f.keyPart = f.packPart + nPG + 1;
  f.nWG = nWGt; f.nTiles = 1; f.cellStride = (u32)cellWords; f.counterStride = (u32)counterWords;
  f.tileElems = (u64)nPix; f.outStride = cap;
  f.maskBits = dBits; f.payloadAt = payloadAt;
  f.epoch = ctx.nextEpoch();
  f.publishEpoch = (fastTestGiveUp() & 1u) ? f.epoch ^ 0x5A5A5A5Au : f.epoch;
  f.spinLimit = (fastTestGiveUp() & 1u) ? 8u : (1u << 22);
  fb.result = dRes;
  FastBatch batch;
  memset(&batch, 0, sizeof(batch));
  batch.nTiles = 1; batch.nWG = nWGt; batch.tileElems = (u64)nPix; batch.nBlobsMore = 0;
  BandParams sp = bp;
  sp.mb = 8; sp.nTV = (nRows + 7) / 8; sp.nTH = (nCols + 7) / 8;
  (void)hipGetLastError();
  hipMemsetAsync(dRes, 0, sizeof(FastEncodeResult), st);
  { ProfScope ps(ctx, "masked_encode1"); launchFastEncode(0, sp, maxZErr, 0, dData, dWs, cap, 0, fb, batch, st); }
  if (hipGetLastError() != hipSuccess) { ctx.lastError = "lerc_amd: a streaming encode kernel could not be launched"; return false; }
  hipMemcpyAsync(hRes, dRes, sizeof(FastEncodeResult), hipMemcpyDeviceToHost, st);
  if (!wait()) return false;
  TL("streamMasked: kernel done");
  if (hRes->stuck) { ctx.wipePersistentState(); return true; }    // (the three kernels take the band)
  streamSums = hRes->streamSums;
  nBytesStreamed = hRes->nBytesTiling;    // (a stream that does not fit the buffer was cut off inside it; the size check in emit() says BufferTooSmall)
  dStreamed = dWs ? dWs + payloadAt : reinterpret_cast<u8*>(dRes);    // (size query: only != nullptr counts)
  ctx.lastNote = "masked band: block stream by the one-launch encoder";
  return true;
}

// the size of the band's block stream with blocks of mb x mb (dOffsets: where each block goes)
bool BandEncoder::tilingBytes(int mb, u32& total)
{
  blocksOf(mb);
  const u32 nPos = (u32)bp.nTV * (u32)bp.nTH;
  if (mb == 8)
  {
    if (!streamMasked()) return false;
    if (dStreamed) { total = nBytesStreamed; return codeMask(); }
  }
  if (mb == 8 && spec.sizesFresh)    // priced behind the statistics already (see Speculated): dSizes / dOffsets hold the result
  {
    spec.sizesFresh = false;
    total = spec.total;
    return codeMask();
  }
  { ProfScope ps(ctx, "tile_sizes"); launchTileSizes(dt, mb, dData, dBits, bp, dSizes, dStatus, st); }
  { ProfScope ps(ctx, "scan_block_sizes"); launchExclusiveScan(dSizes, dOffsets, nPos, dScratch, st); }
  hipMemcpyAsync(&total, dOffsets + nPos, 4, hipMemcpyDeviceToHost, st);
  if (!codeMask()) return false;
  return wait();
}

// a band whose depths are not constant: 8 x 8 blocks against Huffman / lossless float coding, 16 x 16 blocks, one sweep
u32 BandEncoder::priceModes()
{
  // (what was enqueued ahead of the decisions only counts if they came out as assumed)
  if (spec.on && !(bp.allValid && bp.intLossless && bp.maxZErr == 0.5 && bp.tryDiff == spec.bp.tryDiff && bp.version == spec.bp.version && !dBits))
    spec.on = spec.sizesFresh = false;
  if (spec.on) { dSizes = spec.dSizes; dOffsets = spec.dOffsets; dScratch = spec.dScratch; }
  else
  {
    dSizes = ctx.allocT<u32>((size_t)nPos8 + 4);
    dOffsets = ctx.allocT<u32>((size_t)nPos8 + 4);
    dScratch = ctx.allocT<u32>((size_t)nPos8 / 1024 + 8);
  }
  if (!dSizes || !dOffsets || !dScratch) return kFailed;

  u32 nBytesTiling = 0;
  if (!tilingBytes(8, nBytesTiling)) return kFailed;
  payload = P_TILING;
  nBytesData = nBytesTiling;
  u32 nBytesHuffman = 0;

  if (hd.tryHuffmanInt())
  {
    TL("before the Huffman plan");
    if (!planHuffman(ctx, dt, dData, dBits, nRows, nCols, nD, hd.version, huff, spec.on ? spec.histo : nullptr)) return kFailed;
    TL("Huffman plan made");
    nBytesHuffman = huff.ok ? huff.nBytes : 0;
    if (huff.ok && nBytesHuffman < nBytesTiling) { payload = P_HUFFMAN; imageMode = huff.imageMode; nBytesData = nBytesHuffman; }
    else huff.ok = false;
  }
  else if (hd.tryHuffmanFlt())
  {
    // lossless float / double: predictor + byte planes + entropy coding, kept if it beats the (raw) blocks by 10 % (Lerc2.cpp:305-328)
    if (!planLosslessFloat(ctx, dt, dData, dByteMask, nd.active, nRows, nCols, nD, fpl)) return kFailed;
    // The reference keeps the coded planes inside its Lerc2 object until a band writes them, and only the
    // nDepth == 1 entry drops planes left over from a band that did not (fpl_Lerc2Ext.cpp:432-452): with
    // nDepth > 1 they count into the next band's length (every later band of a size query, :391-403).
    if (nD == 1) ms.fplStale = 0;
    fplPlanes = fpl.nBytes - 1;
    nBytesHuffman = 1 + ms.fplStale + fplPlanes;
    if ((double)nBytesHuffman < (double)nBytesTiling * 0.9) { payload = P_FLOAT; imageMode = IEM_DeltaDeltaHuffman; nBytesData = nBytesHuffman; }
  }

  const size_t nBytesOneSweep = (size_t)tb * nD * (size_t)numValid;
  // retry with 16 x 16 blocks at low bit rates (Lerc2.cpp:333-357)
  if (((size_t)nBytesTiling * 8 < (size_t)nPix * nD * 1.5)
    && ((size_t)nBytesTiling < 4 * nBytesOneSweep)
    && (nBytesHuffman == 0 || (size_t)nBytesTiling < (size_t)2 * nBytesHuffman)
    && (nRows > 8 || nCols > 8))
  {
    u32 nBytes16 = 0;
    if (!tilingBytes(16, nBytes16)) return kFailed;
    if (nBytes16 <= nBytesData) { nBytesData = nBytes16; payload = P_TILING; imageMode = IEM_Tiling; huff.ok = false; hd.mbSize = 16; }
    else if (payload == P_TILING && !tilingBytes(8, nBytesTiling)) return kFailed;    // restore the 8x8 offsets
    if (hd.mbSize == 8) blocksOf(8);
  }
  if (hd.tryHuffmanInt() || hd.tryHuffmanFlt()) nBytesData += 1;
  if (nBytesOneSweep <= (size_t)nBytesData) { payload = P_ONESWEEP; blobSize += 1 + (u32)nBytesOneSweep; }
  else blobSize += 1 + nBytesData;
  return kOk;
}

// ---- 5. the band's sections and their sizes; ends where a size query ends
u32 BandEncoder::price(u32& bandBytes)
{
  blobSize = headerBytes(hd.version) + 4;
  if (numValid > 0)
  {
    hd.zMin = *std::min_element(zMinVec.begin(), zMinVec.end());
    hd.zMax = *std::max_element(zMaxVec.begin(), zMaxVec.end());
    bp.zMaxHdr = hd.zMax;
    bp.checkOverflow = ((dt == DT_Int || dt == DT_UInt) && (hd.zMax - hd.zMin >= 0x7FFFFFFF)) ? 1 : 0;
    if (hd.zMin != hd.zMax)
    {
      writeRanges = hd.version >= 4;    // Lerc2.cpp:260
      if (writeRanges) blobSize += 2u * (u32)nD * (u32)tb;
      const bool constDepths = writeRanges && (0 == memcmp(zMinVec.data(), zMaxVec.data(), nD * sizeof(double)));
      if (!constDepths)
      {
        const u32 rc = priceModes();
        if (rc != kOk) return rc;
      }
    }
  }
  if (!codeMask()) return kFailed;
  if ((size_t)blobSize > (size_t)INT_MAX) return kFailed;
  hd.blobSize = (int)blobSize;
  bandBytes = blobSize;
  if (fplPlanes)
  {
    if (dBandOut && payload == P_FLOAT)
    {
      if (ms.fplStale) { ctx.lastError = "lossless float: planes of an earlier band would be written again (reference quirk, not reproduced)"; return kFailed; }
    }
    else ms.fplStale += fplPlanes;
  }
  return kOk;
}

// ---- 6. emit: small sections from the host, pixel payload by kernels
u32 BandEncoder::emit()
{
  if (blobSize > capacityLeft) return kBufferTooSmall;
  // (put together in pinned memory -- the mask's RLE can be megabytes, and a pageable source is staged at ~1 GB/s with the
  // stream waiting; the area held the mask bits, which codeMask() has consumed by now)
  const std::vector<u8>& rle = transit.rle;
  const size_t prefixLen = headerBytes(hd.version) + 4 + rle.size() + (writeRanges ? 2 * (size_t)nD * tb : 0) + 2;
  const size_t huffPinAt = (prefixLen + 63) & ~(size_t)63;    // (the Huffman mode's code words and table: emitHuffman)
  const size_t prefixCap = huffPinAt + (payload == P_HUFFMAN ? 2048 + huff.table.size() + 64 : 0);
  u8* prefix = (u8*)ctx.pinnedAux(prefixCap);
  if (!prefix) return kFailed;
  writeHeader(prefix, hd);
  size_t at = headerBytes(hd.version);
  const int nm = (int)rle.size();
  memcpy(&prefix[at], &nm, 4); at += 4;
  if (nm) { memcpy(&prefix[at], rle.data(), rle.size()); at += rle.size(); }
  if (writeRanges)
  {
    for (int m = 0; m < nD; m++) { const u64 raw = statKeyToRawBits(dt, hMins[m]); putBytes(&prefix[at], raw, tb); at += tb; }
    for (int m = 0; m < nD; m++) { const u64 raw = statKeyToRawBits(dt, hMaxs[m]); putBytes(&prefix[at], raw, tb); at += tb; }
  }
  if (payload != P_NONE)
  {
    prefix[at++] = (payload == P_ONESWEEP) ? 1 : 0;
    if (payload != P_ONESWEEP && (hd.tryHuffmanInt() || hd.tryHuffmanFlt())) prefix[at++] = (u8)imageMode;
  }
  TL("prefix assembled");
  const bool prefixByKernel = payload == P_HUFFMAN && at <= 4096;    // (the Huffman mode's kernel takes a short prefix along: emitHuffman)
  if (!prefixByKernel) hipMemcpyAsync(dBandOut, prefix, at, hipMemcpyHostToDevice, st);
  dPayload = dBandOut + at;

  if (payload == P_TILING && dStreamed && hd.mbSize == 8)    // (in place since streamMasked)
  {
    if (dStreamed != dPayload) { ctx.lastError = "lerc_amd: the masked band's block stream is not where the band's sections end"; return kFailed; }
  }
  else if (payload == P_TILING)
  {
    ProfScope ps(ctx, "tile_write");
    launchTileWrite(dt, hd.mbSize, dData, dBits, bp, dOffsets, dPayload, dStatus, st);
  }
  else if (payload == P_ONESWEEP)
  {
    if (ms.allValid) hipMemcpyAsync(dPayload, dData, (size_t)nElem * tb, hipMemcpyDeviceToDevice, st);
    else if (!enqueueMaskedOneSweep(ctx, true, dData, dPayload, dBits, nPix, nD * tb, st)) return kFailed;
  }
  else if (payload == P_FLOAT)
  {
    if (!emitLosslessFloat(ctx, fpl, dPayload)) return kFailed;
  }
  else if (payload == P_HUFFMAN)
  {
    if (!emitHuffman(ctx, dt, dData, dBits, nRows, nCols, nD, huff, dPayload, dStatus, prefix + huffPinAt, prefixByKernel ? dBandOut : nullptr, prefix, (u32)at)) return kFailed;
    TL("Huffman stream enqueued");
  }
  return kOk;
}

// ---- 7. checksum over blob[14 ..) (Lerc2.cpp:1012-1030), patched into the header (codec 2 has none); the kernels' status
u32 BandEncoder::seal()
{
  if (hd.version >= 3)
  {
    u64* dFl = ctx.allocT<u64>(kFletcherPartials);
    if (!dFl) return kFailed;
    // (the sums are folded and the header field is written on the device: one wait at the end of the band instead of two)
    ProfScope ps(ctx, "fletcher_enc");
    if (payload == P_TILING && dStreamed && hd.mbSize == 8 && dStreamed == dPayload && (size_t)(dPayload - dBandOut) + nBytesStreamed == blobSize)
    {
      // the masked band's block stream came with its terms (tile_fast.hip: fusedFlush); what is left to read is what lies in front of it
      launchFletcher(dBandOut + 14, (u32)(dPayload - dBandOut) - 14, dFl, st);
      launchFletcherPatchWith(dFl, streamSums, blobSize - 14, dBandOut + 10, st);
    }
    else { launchFletcher(dBandOut + 14, blobSize - 14, dFl, st); launchFletcherPatch(dFl, blobSize - 14, dBandOut + 10, st); }
  }
  DeviceStatus status;
  hipMemcpyAsync(&status, dStatus, sizeof(DeviceStatus), hipMemcpyDeviceToHost, st);
  if (!wait()) return kFailed;
  if (hd.version >= 3) TL("band done");
  if (status.error) { ctx.lastError = "device kernel reported an error"; return status.error; }
  if (ctx.profOn()) ctx.profCollect();
  return kOk;
}

u32 encodeBand(Context& ctx, const EncodeRequest& rq, int iBand, MaskState& ms, std::vector<u8>& prevByteValid,
                      bool& anyMaskModified, u8* dBandOut, u32 capacityLeft, u32& bandBytes)
{
  bandBytes = 0;
  BandEncoder e(ctx, rq, iBand, ms, dBandOut, capacityLeft);
  u32 rc = e.begin();
  if (rc == kOk) rc = e.validity();
  if (rc == kOk) rc = e.statistics();
  if (rc == kOk) rc = e.maskAcrossBands(prevByteValid, anyMaskModified);
  if (rc == kOk) rc = e.decide();
  if (rc == kOk) rc = e.price(bandBytes);
  if (rc != kOk || !dBandOut) return rc;    // (a size query ends here)
  rc = e.emit();
  return rc == kOk ? e.seal() : rc;
}

}    // namespace

u32 encodeBands(Context& ctx, const EncodeRequest& rq, u32& numBytesNeeded, u32& numBytesWritten)
{
  const i64 nPix = (i64)rq.nRows * rq.nCols;
  const size_t maskBytes = (size_t)((nPix + 7) >> 3) + 64;
  ctx.pathCount[1]++;
  MaskState ms;
  ms.dBits = ctx.allocT<u8>(maskBytes);
  std::vector<u8> prevValid;
  bool anyMaskModified = false;
  u32 total = 0;
  const size_t persistent = maskBytes + 512;    // keep ms.dBits across bands
  for (int iBand = 0; iBand < rq.nBands; iBand++)
  {
    // band scratch is re-used: rewind the bump pointer to just behind the persistent mask
    ctx.reset();
    ctx.alloc(persistent);
    u32 bandBytes = 0;
    u8* dst = rq.dOut ? rq.dOut + total : nullptr;
    const u32 left = rq.dOut ? (rq.outCapacity > total ? rq.outCapacity - total : 0) : 0;
    const u32 rc = encodeBand(ctx, rq, iBand, ms, prevValid, anyMaskModified, dst, left, bandBytes);
    if (rc != kOk) return rc;
    if ((size_t)total + bandBytes > (size_t)UINT_MAX) return kDimsTooLarge;
    total += bandBytes;
  }
  numBytesNeeded = total;
  if (rq.dOut) numBytesWritten = total;
  return kOk;
}

}    // namespace lerc
