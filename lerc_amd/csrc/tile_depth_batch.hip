// tile_depth_batch.hip -- batches of DEPTH tiles: nTiles rasters [nRows][nCols][nDepth] of one shape, each with a validity mask of its
// own, encoded into (decoded from) nTiles independent Lerc2 blobs with the header's nDepth by ONE set of launches, a tile per blockIdx.y
// (or per workgroup).  This is Lerc's own pixel-interleaved form: what a tiled writer makes of an [H, W, C] raster.  The launch set is the
// masked family's (tile_mask_batch.hip), the block bodies are the general kernels' over all slices (tile_encode.hip, tile_decode.hip),
// composed from the same stages (tile_encode_dev.h, tile_decode_dev.h, tile_batch_dev.h).
//
// What differs from a tile of one value a pixel:
//   k_tdb_prelude   the range is taken per slice (nDepth <= kTdbMaxDepth minima and maxima in registers), the header's range is over all
//                   slices; NaN, all-integer and TryRaiseMaxZError findings run over every value of the valid pixels.  One more kind:
//                   every slice constant, the slices different (Lerc2.cpp:273-278) -- the blob ends behind the ranges.
//   k_tdb_blocks    a wave writes a position's nDepth sub-blocks back to back (Lerc2.cpp:1521-1662): k_encode_tiles' loop with the tile's
//                   own mask, error bound and place in the arena.  The difference to the slice in front is tried for integer types at
//                   maxZErr 0.5, taken where strictly shorter, and left alone where it overflows int.  A position's table entry is the
//                   sum over its slices.
//   k_tdb_decide*   the low-bit-rate rule and one sweep count nDepth values a pixel (Lerc2.cpp:331-338)
//   the front       ranges are 2 * nDepth values, all minima first (WriteMinMaxRanges); one sweep is the valid pixels in row order, all
//                   slices of a pixel together
//   k_tdbd_parse    the header's nDepth, nDepth ranges, both constant kinds, one sweep of nDepth values, the walk over nDepth sub-blocks
//                   a position; a difference bit on slice 0 is damage
//   k_tdbd_blocks   slice after slice: adds the slice in front where the bit says so, clamps to the slice's own maximum
// Tiles that leave the batch (TdbTile::head.flags) are left alone; the host does them one by one behind it.  No workgroup waits for
// another one inside a launch, so the emulator build runs the same path.
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include "kernels.h"
#include "wave_utils.h"
#include "tile_depth_batch.h"
#include "tile_batch_dev.h"

namespace lerc {

template<class T> struct TdbAcc { typedef i64 type; static __device__ __forceinline__ i64 hi() { return 0x7FFFFFFFFFFFFFFFll; } static __device__ __forceinline__ i64 lo() { return -0x7FFFFFFFFFFFFFFFll - 1; } };
template<> struct TdbAcc<float> { typedef double type; static __device__ __forceinline__ double hi() { return __builtin_huge_val(); } static __device__ __forceinline__ double lo() { return -__builtin_huge_val(); } };
template<> struct TdbAcc<double> { typedef double type; static __device__ __forceinline__ double hi() { return __builtin_huge_val(); } static __device__ __forceinline__ double lo() { return -__builtin_huge_val(); } };

// ================================================================================================
// encode
// ================================================================================================
template<class T, bool LARGE>
__global__ void __launch_bounds__(256)
k_tdb_prelude(TmbGeom g, int nD, double maxZErr, u32 cand, const T* __restrict__ data, const u8* __restrict__ valid, u64 validStride, TdbEncodeBuffers b)
{
  typedef typename TdbAcc<T>::type Acc;
  constexpr bool isFlt = DtOf<T>::v >= DT_Float;
  constexpr int MD = kTdbMaxDepth;
  __shared__ __align__(16) u8 s_bits[TbForm<LARGE>::kMaskBytes + 16];
  __shared__ u64 s_red[4];
  __shared__ Acc s_mn[4][MD], s_mx[4][MD];
  __shared__ u64 s_raise[4][9];
  const u32 t = blockIdx.x;
  const u32 nPix = (u32)g.tileElems, nBytes = (nPix + 7u) >> 3;
  const T* __restrict__ px = data + (u64)t * g.tileElems * (u64)nD;
  const u8* __restrict__ vb = valid + (u64)t * validStride;
  u8* __restrict__ bitsOut = b.bits + (u64)t * g.bitStride;
  const int facCand[9] = { 1, 2, 10, 20, 100, 200, 1000, 2000, 10000 };

  u32 flags = 0;
  Acc mn[MD], mx[MD];
#pragma unroll
  for (int d = 0; d < MD; d++) { mn[d] = TdbAcc<T>::hi(); mx[d] = TdbAcc<T>::lo(); }
  bool frac = false;
  double rerr[9];
#pragma unroll
  for (int c = 0; c < 9; c++) rerr[c] = 0;
  const u32 cnt = tbMaskToBits(vb, nPix, s_bits, bitsOut, [&](u32 k)
  {
    const T* __restrict__ pv = px + (u64)k * (u64)nD;
#pragma unroll
    for (int d = 0; d < MD; d++)
    {
      if (d >= nD) continue;
      const T v = pv[d];
      if (isFlt && v != v) { flags |= kTmbNaN; continue; }
      const Acc a = (Acc)v;
      mn[d] = a < mn[d] ? a : mn[d]; mx[d] = a > mx[d] ? a : mx[d];
      if (isFlt)
      {
        const double x = (double)v;
        if (!(v == (T)floor(x + 0.5))) frac = true;    // Lerc.h:271 IsInt
        // TryRaiseMaxZError (Lerc2.cpp:1233-1318) over every slice's value: the largest rounding error per candidate factor
#pragma unroll
        for (int c = 0; c < 9; c++)
          if ((cand >> c) & 1u)
          {
            const double z = x * facCand[c];
            const double dlt = fabs(floor(z + 0.5) - z);
            rerr[c] = dlt > rerr[c] ? dlt : rerr[c];
          }
      }
    }
  });
  const u32 numValid = (u32)blockSum((u64)cnt, s_red);
  const u32 anyFlags = (u32)blockSum((u64)flags, s_red) ? kTmbNaN : 0u;    // (the only flag raised so far)
  const u32 anyFrac = (u32)blockSum(frac ? 1ull : 0ull, s_red);
#pragma unroll
  for (int d = 0; d < MD; d++)
    if (d < nD)    // (the same for every lane)
    {
      const Acc lo = waveMin(mn[d]), hi = waveMax(mx[d]);
      if (laneId() == 0) { s_mn[waveId()][d] = lo; s_mx[waveId()][d] = hi; }
    }
  if (isFlt && cand)
  {
#pragma unroll
    for (int c = 0; c < 9; c++)
    {
      u64 bb; double r = rerr[c]; memcpy(&bb, &r, 8);    // non-negative doubles order like their bit patterns
      bb = waveMax(bb);
      if (laneId() == 0) s_raise[waveId()][c] = bb;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;

  TdbTile ti;
  memset(&ti, 0, sizeof(ti));
  ti.numValid = numValid;
  Acc all0 = TdbAcc<T>::hi(), all1 = TdbAcc<T>::lo();
  bool slicesConst = true;
  for (int d = 0; d < nD; d++)
  {
    Acc lo = s_mn[0][d], hi = s_mx[0][d];
    for (int w = 1; w < 4; w++) { lo = s_mn[w][d] < lo ? s_mn[w][d] : lo; hi = s_mx[w][d] > hi ? s_mx[w][d] : hi; }
    all0 = lo < all0 ? lo : all0; all1 = hi > all1 ? hi : all1;
    if (numValid)
    {
      // (CheckMinMaxRanges compares the vectors of doubles byte for byte, Lerc2.cpp:2640-2653)
      const double dl = (double)lo, dh = (double)hi;
      u64 bl, bh; memcpy(&bl, &dl, 8); memcpy(&bh, &dh, 8);
      if (bl != bh) slicesConst = false;
      ti.minBits[d] = typedBits(dl, g.dt); ti.maxBits[d] = typedBits(dh, g.dt);
    }
  }
  u32 fl = anyFlags;
  ti.kind = (numValid == 0) ? kTmbKindEmpty : (!(all0 < all1) ? kTmbKindConst : (slicesConst ? kTdbKindConstSlices : kTmbKindBlocks8));
  if (numValid) { ti.zMin = (double)all0; ti.zMax = (double)all1; }
  ti.checkOverflow = ((g.dt == DT_Int || g.dt == DT_UInt) && numValid && (ti.zMax - ti.zMin >= (double)0x7FFFFFFF)) ? 1u : 0u;
  // ---- the tile's own error bound, as k_tmb_prelude decides it (tile_mask_batch.hip), from the statistics over all slices
  ti.maxZErr = maxZErr;
  if (isFlt && !numValid) ti.maxZErr = 0;    // "tile has no valid data" (Lerc.cpp:1479-1484)
  if (isFlt && numValid)
  {
    const double lim = (g.dt == DT_Float) ? (double)(1 << 23) : (double)(1ll << 53);
    if (!anyFrac && ti.zMin >= -lim && ti.zMin <= lim && ti.zMax >= -lim && ti.zMax <= lim)
    {
      ti.isInt = 1u;
      const double fl0 = floor(maxZErr);
      ti.maxZErr = fl0 > 0.5 ? fl0 : 0.5;
    }
    else if (cand)
    {
      const double errCand[9] = { 1, 0.5, 0.1, 0.05, 0.01, 0.005, 0.001, 0.0005, 0.0001 };
      for (int c = 0; c < 9; c++)
        if ((cand >> c) & 1u)
        {
          u64 bb = 0;
          for (int w = 0; w < 4; w++) bb = s_raise[w][c] > bb ? s_raise[w][c] : bb;
          double r; memcpy(&r, &bb, 8);
          if (r / facCand[c] <= maxZErr / 2) { ti.maxZErr = errCand[c] / 2; break; }
        }
    }
  }

  // ---- the mask's run-length stream (tbMaskRle): one a tile
  u32 rleLen = 0;
  if (fl == 0 && numValid > 0 && numValid < nPix)
  {
    rleLen = tbMaskRle(s_bits, nBytes, b.rle + (u64)t * g.rleStride, g.rleStride);
    if (!rleLen) fl |= kTmbRle;
  }
  ti.head.flags = fl;
  ti.rleLen = rleLen;
  // header and mask section; where values differ: the ranges, and unless every slice is constant the "one sweep" byte
  const u32 ranges = 2u * (u32)nD * (u32)sizeof(T);
  ti.dataBegin = kHdr6 + 4u + rleLen + (ti.kind == kTmbKindBlocks8 ? ranges + 1u : ti.kind == kTdbKindConstSlices ? ranges : 0u);
  ti.mbSize = 8u;
  ti.head.blobSize = ti.dataBegin;    // (all there is of an empty or a constant tile; the others: k_tdb_decide2)
  b.tiles[t] = ti;
}

// What lies in front of a tile's block stream, by one workgroup: header, mask section; where values differ: the ranges (all minima,
// then all maxima: WriteMinMaxRanges, Lerc2.cpp:2611) and the "one sweep" byte, and behind a 1 the valid pixels raw in row order, all
// slices of a pixel together (Lerc2::WriteDataOneSweep).  s_hdr: 96 bytes of LDS, s_w: 4 words.
template<class T>
__device__ __forceinline__ void tdbWriteFront(const TmbGeom& g, int nD, u32 t, const TdbTile& ti, const T* __restrict__ px, u8* __restrict__ blob,
                                              const TdbEncodeBuffers& b, u8* s_hdr, u32* s_w)
{
  const TbHeader6 h = { kCodecVersion, 0u, g.nRows, g.nCols, nD, (int)ti.numValid, (int)ti.mbSize, (int)ti.head.blobSize, g.dt, 0,
                        ti.isInt ? 0x100u : 0u, ti.maxZErr, ti.zMin, ti.zMax };
  tbWriteHeaderMask(blob, h, b.rle + (u64)t * g.rleStride, ti.rleLen, s_hdr);
  if (ti.kind == kTmbKindEmpty || ti.kind == kTmbKindConst) return;    // (Lerc2.cpp:240, :255: nothing behind the mask)
  u8* r = blob + kHdr6 + 4u + ti.rleLen;
  if ((int)threadIdx.x < nD)
  {
    putBytes(r + (u64)threadIdx.x * sizeof(T), ti.minBits[threadIdx.x], (int)sizeof(T));
    putBytes(r + (u64)((u32)nD + threadIdx.x) * sizeof(T), ti.maxBits[threadIdx.x], (int)sizeof(T));
  }
  if (ti.kind == kTdbKindConstSlices) return;
  if (threadIdx.x == 0) r[2u * (u32)nD * (u32)sizeof(T)] = ti.kind == kTmbKindOneSweep ? 1 : 0;
  if (ti.kind != kTmbKindOneSweep) return;
  u8* __restrict__ dst = blob + ti.dataBegin;    // (any alignment: bytes)
  auto put = [&](u32 k, bool valid, u32 rank)
  {
    if (!valid) return;
    for (int d = 0; d < nD; d++)
    {
      u64 bits = 0;
      const T v = px[(u64)k * (u64)nD + d];
      memcpy(&bits, &v, sizeof(T));
      putBytes(dst + ((u64)rank * (u64)nD + d) * sizeof(T), bits, (int)sizeof(T));
    }
  };
  const u32 nPix = (u32)g.tileElems;
  if (ti.numValid == nPix) { for (u32 k = threadIdx.x; k < nPix; k += 256u) put(k, true, k); }
  else tbRankedSweep(b.bits + (u64)t * g.bitStride, nPix, s_w, put);
}

// A wave per MB x MB position of a tile (blockIdx.y), all slices in turn: k_encode_tiles' body (tile_encode.hip) with the tile's own
// mask, error bound and place in the arena.  Not WRITE: the position's size over all slices goes to its table entry; WRITE: its
// sub-blocks go back to back to where the scanned table says.  In the 8 x 8 WRITE launch one more workgroup behind a tile's last block
// writes what lies in front of the block stream -- for a tile of any kind.
template<class T, int MB, bool WRITE>
__global__ void __launch_bounds__(256)
k_tdb_blocks(TmbGeom g, int nD, BandParams p, const T* __restrict__ data, u8* __restrict__ arena, TdbEncodeBuffers b)
{
  constexpr int E = MB * MB / 64, NMAX = MB * MB;
  constexpr int OBW = (1 + NMAX * (int)sizeof(T) + 3) / 4 + 4;
  constexpr bool kInt = std::is_integral<T>::value;
  __shared__ T s_val[2][4][NMAX];
  __shared__ int s_diff[4][kInt ? NMAX : 1];
  __shared__ u32 s_obuf[4][WRITE ? OBW : 1];
  __shared__ u32 s_lut[4][WRITE ? NMAX : 1];
  const u32 t = blockIdx.y;
  const TdbTile& rec = b.tiles[t];
  if (rec.head.flags) return;
  const u32 kind = rec.kind;
  const int nTV = (g.nRows + MB - 1) / MB, nTH = (g.nCols + MB - 1) / MB;
  const T* __restrict__ px = data + (u64)t * g.tileElems * (u64)nD;

  if constexpr (WRITE && MB == 8)
  {
    __shared__ u8 s_hdr[96];
    __shared__ u32 s_w[4];
    if (blockIdx.x == gridDim.x - 1) { tdbWriteFront<T>(g, nD, t, rec, px, arena + rec.head.offset, b, s_hdr, s_w); return; }
  }
  if (WRITE ? kind != (MB == 8 ? kTmbKindBlocks8 : kTmbKindBlocks16) : (kind != kTmbKindBlocks8 || (MB == 16 && !rec.retry))) return;

  const int w = waveId(), lane = laneId();
  const int pos = (int)blockIdx.x * 4 + w;
  if (pos >= nTV * nTH) return;    // whole wave leaves together
  p.mb = MB; p.nTV = nTV; p.nTH = nTH; p.nDepth = nD;
  p.allValid = (rec.numValid == (u32)g.tileElems) ? 1 : 0;
  const double tileErr = rec.maxZErr;    // (the tile's own bound: k_tdb_prelude)
  p.maxZErr = tileErr; p.scale = 1 / (2 * tileErr); p.invScale = 2 * tileErr;
  p.tryDiff = (kInt && p.intLossless) ? 1 : 0;    // (Lerc2.cpp:1493-1495; codec 6)
  p.checkOverflow = (int)rec.checkOverflow;
  u32* __restrict__ table = (MB == 8 ? b.blockOff + (u64)t * g.posStride : b.blockOff16 + (u64)t * g.pos16Stride);
  u8* __restrict__ out = WRITE ? arena + rec.head.offset + rec.dataBegin : nullptr;

  const BlockLanes<E> L = blockLanes<E, true>(p, pos, b.bits + (u64)t * g.bitStride);
  const int n = L.n;
  u32 total = 0, outOff = WRITE ? table[pos] : 0u;
  u32* obuf = s_obuf[w];

  for (int iD = 0; iD < nD; iD++)
  {
    const int cur = iD & 1;
    T* valBuf = s_val[cur][w];
    const T* prevBuf = s_val[cur ^ 1][w];

    if (n == 0)    // empty position: one "all zero" byte per slice
    {
      if (WRITE && lane == 0) out[outOff] = emptyBlockByte(p, L.j0);
      outOff += 1; total += 1;
      continue;
    }

    T v[E];
    gatherSlice<T, E>(L, px, nD, iD, valBuf, v);
    const SliceCode<T, E> sv = analyseSlice<T, E>(p, n, v, L.rank, valBuf, p.dt, p.allValid != 0, p.maxZErr > 0, p.intLossless != 0);

    // the difference to the slice in front (integer lossless only; the kernels of the float types carry none of it)
    bool useDiff = false;
    int d[E];
    SliceCode<int, E> sd = {};
#pragma unroll
    for (int k = 0; k < E; k++) d[k] = 0;
    if (kInt && p.tryDiff && iD > 0)
    {
      bool ovf = false;
#pragma unroll
      for (int k = 0; k < E; k++)
        if (L.rank[k] >= 0)
        {
          const T pv = prevBuf[L.rank[k]];
          if (!p.checkOverflow) d[k] = (int)((i64)(int)v[k] - (i64)(int)pv);
          else
          {
            const double z = (double)v[k] - (double)pv;
            if (z < -2147483648.0 || z > 2147483647.0) ovf = true; else d[k] = (int)z;
          }
          s_diff[w][kInt ? L.rank[k] : 0] = d[k];
        }
      waveSync();
      if (!__any(ovf))
      {
        sd = analyseSlice<int, E>(p, n, d, L.rank, s_diff[w], DT_Int, true, true, true);
        useDiff = sv.plan.nBytes > sd.plan.nBytes;
      }
      waveSync();
    }

    const int nBytes = useDiff ? sd.plan.nBytes : sv.plan.nBytes;
    if (WRITE)
    {
      if (!useDiff) composeBlock<T, E>(obuf, s_lut[w], p, sv.plan, n, L.j0, false, sv.zMin, v, sv.q, L.rank, sv.qMax);
      else composeBlock<int, E>(obuf, s_lut[w], p, sd.plan, n, L.j0, true, sd.zMin, d, sd.q, L.rank, sd.qMax);
      const u8* ob8 = reinterpret_cast<const u8*>(obuf);
      for (int i = lane; i < nBytes; i += 64) out[outOff + i] = ob8[i];
      waveSync();
    }
    outOff += (u32)nBytes;
    total += (u32)nBytes;
  }
  if (!WRITE && lane == 0) table[pos] = total;
}

// the 8 x 8 positions' sizes scanned, and whether the low-bit-rate rule asks for the sizes of 16 x 16 blocks too (Lerc2.cpp:331-338:
// the bit rate counts nDepth values a pixel, invalid pixels too; vb: sizeof(T) * nDepth)
__global__ void __launch_bounds__(256) k_tdb_decide(TmbGeom g, u32 nD, u32 vb, TdbEncodeBuffers b)
{
  __shared__ u32 s_scan[257];
  const u32 t = blockIdx.x;
  if (b.tiles[t].head.flags || b.tiles[t].kind != kTmbKindBlocks8) return;    // (neither is written in this kernel)
  const u32 nPos = (u32)(g.nTV * g.nTH);
  const u32 nBytesTiling = blockScanInPlace(b.blockOff + (u64)t * g.posStride, nPos, s_scan);
  if (threadIdx.x != 0) return;
  TdbTile& ti = b.tiles[t];
  const u64 oneSweep = (u64)vb * ti.numValid;
  ti.retry = ((double)((u64)nBytesTiling * 8u) < (double)(g.tileElems * (u64)nD) * 1.5 && (u64)nBytesTiling < 4u * oneSweep && (g.nRows > 8 || g.nCols > 8)) ? 1u : 0u;
  ti.nBytesTiling = nBytesTiling;
}

// Lerc2.cpp:340-381: 16 x 16 blocks if they are no longer than the 8 x 8 ones, one sweep if it is no longer than the blocks that are
// left, the blob's size, the slot check
__global__ void __launch_bounds__(256) k_tdb_decide2(TmbGeom g, u32 vb, u64 slotBytes, u64 firstTile, TdbEncodeBuffers b)
{
  __shared__ u32 s_scan[257];
  __shared__ u32 s_rec[3];
  const u32 t = blockIdx.x;
  // (the record is read once, in front of a barrier: thread 0 rewrites it further down)
  if (threadIdx.x == 0) { s_rec[0] = b.tiles[t].head.flags; s_rec[1] = b.tiles[t].kind; s_rec[2] = b.tiles[t].retry; }
  __syncthreads();
  if (s_rec[0]) return;
  const bool blocks = s_rec[1] == kTmbKindBlocks8, retry = blocks && s_rec[2];
  u32 nBytes16 = 0;
  if (retry) nBytes16 = blockScanInPlace(b.blockOff16 + (u64)t * g.pos16Stride, (u32)(((g.nRows + 15) / 16) * ((g.nCols + 15) / 16)), s_scan);
  if (threadIdx.x != 0) return;
  TdbTile& ti = b.tiles[t];
  if (blocks)
  {
    if (retry && nBytes16 <= ti.nBytesTiling) { ti.kind = kTmbKindBlocks16; ti.mbSize = 16u; ti.nBytesTiling = nBytes16; }
    const u64 oneSweep = (u64)vb * ti.numValid;
    const u64 size = (u64)ti.dataBegin + (oneSweep <= (u64)ti.nBytesTiling ? oneSweep : (u64)ti.nBytesTiling);
    if (oneSweep <= (u64)ti.nBytesTiling) ti.kind = kTmbKindOneSweep;
    if (size > 0x7FFFFFFFull) { ti.head.flags = kTbCapacity; return; }    // (a blob is at most 2 GB, Lerc2.cpp:375)
    ti.head.blobSize = (u32)size;
  }
  if (slotBytes)
  {
    ti.head.offset = (firstTile + t) * slotBytes;
    if ((u64)ti.head.blobSize > slotBytes) ti.head.flags = kTbCapacity;
  }
}

__global__ void __launch_bounds__(256) k_tdb_arena(u32 nTiles, u64 arenaBase, u64 arenaCapacity, TdbEncodeBuffers b)
{
  __shared__ u64 s_part[257];
  tbArenaPlace(b.tiles, nTiles, arenaBase, arenaCapacity, s_part);
}

__global__ void __launch_bounds__(256) k_tdb_checksum(u8* __restrict__ arena, TdbEncodeBuffers b)
{
  __shared__ u64 s_red[4];
  tbWriteChecksum(arena, b.tiles[blockIdx.x].head, s_red);
}

template<class T>
static void tdbEncodeT(const TmbGeom& g, int nD, const BandParams& bp, double maxZErr, u32 cand, const void* dTiles, const u8* dValidBytes, u64 validStride,
                       u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile, const TdbEncodeBuffers& b, hipStream_t st)
{
  const int nPos = g.nTV * g.nTH, nPos16 = ((g.nRows + 15) / 16) * ((g.nCols + 15) / 16);
  const dim3 perTile(g.nTiles), blk(256);
  const u32 vb = (u32)sizeof(T) * (u32)nD;
  if (tbLargeForm(g)) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tdb_prelude<T, true>), perTile, blk, 0, st, g, nD, maxZErr, cand, (const T*)dTiles, dValidBytes, validStride, b); }
  else { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tdb_prelude<T, false>), perTile, blk, 0, st, g, nD, maxZErr, cand, (const T*)dTiles, dValidBytes, validStride, b); }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tdb_blocks<T, 8, false>), dim3((nPos + 3) / 4, g.nTiles), blk, 0, st, g, nD, bp, (const T*)dTiles, (u8*)nullptr, b);
  hipLaunchKernelGGL(k_tdb_decide, perTile, blk, 0, st, g, (u32)nD, vb, b);
  // (over the whole batch, whether a tile is marked or not: the host knows nothing yet, and does not wait to learn it)
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tdb_blocks<T, 16, false>), dim3((nPos16 + 3) / 4, g.nTiles), blk, 0, st, g, nD, bp, (const T*)dTiles, (u8*)nullptr, b);
  hipLaunchKernelGGL(k_tdb_decide2, perTile, blk, 0, st, g, vb, slotBytes, firstTile, b);
  if (!slotBytes) hipLaunchKernelGGL(k_tdb_arena, dim3(1), blk, 0, st, g.nTiles, arenaBase, arenaCapacity, b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tdb_blocks<T, 8, true>), dim3((nPos + 3) / 4 + 1, g.nTiles), blk, 0, st, g, nD, bp, (const T*)dTiles, dArena, b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tdb_blocks<T, 16, true>), dim3((nPos16 + 3) / 4, g.nTiles), blk, 0, st, g, nD, bp, (const T*)dTiles, dArena, b);
  hipLaunchKernelGGL(k_tdb_checksum, perTile, blk, 0, st, dArena, b);
}

void launchTdbEncode(const TmbGeom& g, int nDepth, const BandParams& bp, double maxZErr, u32 cand, const void* dTiles, const u8* dValidBytes,
                     u64 validStride, u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile, const TdbEncodeBuffers& b,
                     hipStream_t st)
{
  if (nDepth < 1 || nDepth > kTdbMaxDepth) return;    // (the host's check: codec_tiles_batch.cpp)
  switch (g.dt)
  {
    case DT_Short:  tdbEncodeT<short>(g, nDepth, bp, maxZErr, cand, dTiles, dValidBytes, validStride, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_UShort: tdbEncodeT<unsigned short>(g, nDepth, bp, maxZErr, cand, dTiles, dValidBytes, validStride, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_Int:    tdbEncodeT<int>(g, nDepth, bp, maxZErr, cand, dTiles, dValidBytes, validStride, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_UInt:   tdbEncodeT<unsigned int>(g, nDepth, bp, maxZErr, cand, dTiles, dValidBytes, validStride, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_Float:  tdbEncodeT<float>(g, nDepth, bp, maxZErr, cand, dTiles, dValidBytes, validStride, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_Double: tdbEncodeT<double>(g, nDepth, bp, maxZErr, cand, dTiles, dValidBytes, validStride, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    default: break;
  }
}

// ================================================================================================
// decode
// ================================================================================================
// is z a value of type T (so that (T)z means the same everywhere)?
template<class T> __device__ __forceinline__ bool tdbIsValueOf(double z)
{
  if (DtOf<T>::v == DT_Double) return z == z;
  if (DtOf<T>::v == DT_Float) return (double)(float)z == z;
  const double lo = (DtOf<T>::v == DT_Short) ? -32768.0 : (DtOf<T>::v == DT_Int) ? -2147483648.0 : 0.0;
  const double hi = (DtOf<T>::v == DT_Short) ? 32767.0 : (DtOf<T>::v == DT_UShort) ? 65535.0 : (DtOf<T>::v == DT_Int) ? 2147483647.0 : 4294967295.0;
  return z >= lo && z <= hi && z == floor(z);
}

// The walk over a depth tile's block stream by ONE thread: a position is nDepth sub-blocks back to back, each with the position's
// count of valid pixels (tbWalkBlocks, tile_batch_dev.h, takes one).  A difference block's reduced type comes from DT_Int (parseWindow);
// a difference bit on slice 0, or on a float type, is damage (Lerc2.cpp:2048).  table[k]: where position k begins.  p.nDepth: the tile's.
template<int TBYTES, u32 MB>
__device__ __forceinline__ u32 tdbWalkBlocks(const u8* __restrict__ blob, u32 begin, u32 blobEnd, const BandParams& p, u32* __restrict__ table, const u16* nv16)
{
  const u32 nTH = (u32)p.nTH, nPos = (u32)(p.nTV * p.nTH);
  const u32 pattern = 14u;    // codec >= 5: bit 2 of the flag is the difference flag
  u32 pos = begin, fl = 0;
  for (u32 k = 0; k < nPos && !fl; k++)
  {
    table[k] = pos;
    const u32 it = k / nTH, jt = k - it * nTH;
    const u32 nElem = min(MB, (u32)p.nRows - it * MB) * min(MB, (u32)p.nCols - jt * MB);
    const int nv = (int)nv16[k];
    for (int iD = 0; iD < p.nDepth; iD++)
    {
      BlkInfo bi;
      const int rc = parseBlock<TBYTES>(blob, pos, blobEnd, p, nv, nElem, bi);
      if (rc != 0 || bi.len == 0 || (((u32)bi.flag >> 2) & pattern) != (((jt * MB) >> 3) & pattern) || (bi.diff && (iD == 0 || p.dt >= DT_Float))
        || (nv == 0 && (bi.mode != 2 || bi.diff)))
      { fl = kTbBlocks; break; }
      pos += bi.len;
    }
  }
  if (!fl && pos != blobEnd) fl = kTbBlocks;
  table[nPos] = pos;
  return fl;
}

template<class T, bool LARGE>
__global__ void __launch_bounds__(256)
k_tdbd_parse(TmbGeom g, int nD, const u8* __restrict__ arena, const u64* __restrict__ offsets, const u32* __restrict__ sizes, T* __restrict__ outAll,
             u8* __restrict__ validOut, TdbDecodeBuffers b)
{
  constexpr u32 TB = (u32)sizeof(T);
  __shared__ __align__(16) u8 s_bits[TbForm<LARGE>::kMaskBytes + 16];
  __shared__ u16 s_nv[TbForm<LARGE>::kBlocks];
  __shared__ u64 s_red[4];
  __shared__ u32 s_w[4];
  __shared__ TdbTile s_ti;
  __shared__ u32 s_flags, s_nm;
  const u32 t = blockIdx.x;
  const u8* __restrict__ blob = arena + offsets[t];
  const u32 sizeGiven = sizes[t];
  const u32 nPix = (u32)g.tileElems, nBytes = (nPix + 7u) >> 3;
  const u32 ranges = 2u * (u32)nD * TB;

  if (threadIdx.x == 0)
  {
    TdbTile ti;
    memset(&ti, 0, sizeof(ti));
    u32 fl = 0, nm = 0;
    if (sizeGiven < kHdr6 + 4u) fl = kTbHeader;
    else
    {
      TbHeader6 h;
      if (!tbReadHeader6(blob, h)) fl = kTbHeader;
      ti.checksum = h.checksum;
      ti.numValid = (u32)h.numValid;
      ti.head.blobSize = (u32)h.blobSize;
      ti.maxZErr = h.maxZErr; ti.zMin = h.zMin; ti.zMax = h.zMax;
      // (codec 6 only; a blob of another depth, shape or type; noData values or a Huffman mode behind flagBytes / the type: the single-blob decoder's)
      if (h.version != kCodecVersion || h.nRows != g.nRows || h.nCols != g.nCols || h.nDepth != nD || h.numValid < 0 || (u32)h.numValid > nPix
        || (h.microBlockSize != 8 && h.microBlockSize != 16) || h.blobSize < (int)(kHdr6 + 4u) || (u32)h.blobSize > sizeGiven || h.dt != g.dt || h.nBlobsMore != 0
        || (h.flagBytes & 0xFFu) != 0u || (!validOut && (u32)h.numValid != nPix))
        fl = kTbHeader;
      const int mbSize = h.microBlockSize;
      if (!fl)
      {
        nm = (u32)getBytes(blob + kHdr6, 4);
        const bool noStream = ti.numValid == nPix || ti.numValid == 0u;
        if (noStream ? nm != 0u : (nm < 2u || nm > ti.head.blobSize)) fl = kTbHeader;
        else if (ti.numValid == 0u)
        {
          ti.kind = kTmbKindEmpty;    // nothing may follow the mask section's length
          if (ti.head.blobSize != kHdr6 + 4u) fl = kTbHeader;
        }
        else if (ti.zMin == ti.zMax)
        {
          ti.kind = kTmbKindConst;    // every value of a valid pixel is (T)zMin: nothing may follow the mask section
          if ((u64)ti.head.blobSize != (u64)kHdr6 + 4u + nm || !tdbIsValueOf<T>(ti.zMin)) fl = kTbHeader;
          for (int d = 0; d < nD; d++) ti.minBits[d] = typedBits(ti.zMin, g.dt);
        }
        else if (!(ti.zMin < ti.zMax) || (u64)kHdr6 + 4u + nm + ranges > (u64)ti.head.blobSize) fl = kTbHeader;    // (NaN fails every comparison)
        else
        {
          const u8* r = blob + kHdr6 + 4u + nm;
          bool slicesConst = true;
          for (int d = 0; d < nD; d++)
          {
            ti.minBits[d] = getBytes(r + (u64)d * TB, (int)TB); ti.maxBits[d] = getBytes(r + (u64)(nD + d) * TB, (int)TB);
            const double lo = typedFromBits(ti.minBits[d], g.dt), hi = typedFromBits(ti.maxBits[d], g.dt);
            if (lo != lo || hi != hi) fl = kTbHeader;    // (a NaN among the ranges: not this decoder's)
            u64 bl, bh; memcpy(&bl, &lo, 8); memcpy(&bh, &hi, 8);
            if (bl != bh) slicesConst = false;    // (the vectors of doubles byte for byte: CheckMinMaxRanges)
          }
          ti.dataBegin = kHdr6 + 4u + nm + ranges + 1u;
          if (fl) {}
          else if (slicesConst)
          {
            ti.kind = kTdbKindConstSlices;    // the blob ends behind the ranges
            ti.dataBegin -= 1u;
            if (ti.head.blobSize != ti.dataBegin) fl = kTbHeader;
          }
          else if (ti.dataBegin >= ti.head.blobSize) fl = kTbHeader;
          else if (r[ranges] == 1)
          {
            // one sweep: the blob ends behind numValid * nDepth raw values; the mask's own count is compared below
            ti.kind = kTmbKindOneSweep;
            if ((u64)ti.dataBegin + (u64)ti.numValid * nD * TB != (u64)ti.head.blobSize) fl = kTbHeader;
          }
          else if (r[ranges] != 0) fl = kTbHeader;
          else
          {
            ti.kind = mbSize == 16 ? kTmbKindBlocks16 : kTmbKindBlocks8;
            // (an error bound of 0 is the lossless float mode or a stream this decoder has not been pinned on)
            if (!(ti.maxZErr > 0) || !(ti.maxZErr < 1e300)) fl = kTbHeader;
          }
        }
        ti.rleLen = nm;
      }
    }
    ti.head.flags = fl;
    s_ti = ti; s_flags = fl; s_nm = nm;
  }
  __syncthreads();
  if (s_flags) { if (threadIdx.x == 0) b.tiles[t] = s_ti; return; }
  const u32 blobEnd = s_ti.head.blobSize, nm = s_nm, kind = s_ti.kind;

  // ---- Fletcher32 over blob[14 .. blobSize)
  if (!tbChecksumOk(blob, blobEnd, s_ti.checksum, s_red))
  {
    if (threadIdx.x == 0) { s_ti.head.flags = kTbChecksum; b.tiles[t] = s_ti; }
    return;
  }

  // ---- the mask: all ones, all zeros, or the run-length stream expanded (what it does not fill stays zero)
  const bool allValid = s_ti.numValid == nPix;
  for (u32 i = threadIdx.x; i < nBytes + 16u; i += 256u) s_bits[i] = (allValid && i < nBytes) ? (u8)0xFF : (u8)0;
  __syncthreads();
  if (!allValid && kind != kTmbKindEmpty && threadIdx.x == 0)
    if (!tbMaskUnrle(blob + kHdr6 + 4u, nm, s_bits, nBytes)) s_flags = kTmbMaskStream;
  __syncthreads();
  if (s_flags) { if (threadIdx.x == 0) { s_ti.head.flags = s_flags; b.tiles[t] = s_ti; } return; }

  T* __restrict__ out = outAll + (u64)t * g.tileElems * (u64)nD;
  if (kind == kTmbKindConst || kind == kTdbKindConstSlices || kind == kTmbKindOneSweep)
  {
    // ---- pixels by the mask alone.  A mask that names another number of valid pixels than the header does is the single-blob
    // decoder's business: nothing has been written yet.
    const u8* __restrict__ raw = blob + s_ti.dataBegin;
    const bool sweep = kind == kTmbKindOneSweep;
    if (tbMaskCount(s_bits, nPix, s_red) != s_ti.numValid)
    {
      if (threadIdx.x == 0) { s_ti.head.flags = kTbHeader; b.tiles[t] = s_ti; }
      return;
    }
    tbRankedSweep(s_bits, nPix, s_w, [&](u32 k, bool valid, u32 rank)
    {
      for (int d = 0; d < nD; d++)
      {
        const u64 bits = !valid ? 0ull : sweep ? getBytes(raw + ((u64)rank * (u64)nD + d) * TB, (int)TB) : s_ti.minBits[d];    // (0 where nothing is valid)
        T v; memcpy(&v, &bits, sizeof(T));
        out[(u64)k * (u64)nD + d] = v;
      }
    });
  }
  else if (kind == kTmbKindEmpty)
    for (u64 k = threadIdx.x; k < (u64)nPix * (u64)nD; k += 256u) out[k] = T(0);

  // ---- the bit mask for the block kernel, the caller's valid bytes
  u8* __restrict__ bitsOut = b.bits + (u64)t * g.bitStride;
  for (u32 i = threadIdx.x; i < nBytes; i += 256u) bitsOut[i] = s_bits[i];
  if (validOut)
  {
    u8* __restrict__ vOut = validOut + (u64)t * g.tileElems;
    for (u32 k = threadIdx.x; k < nPix; k += 256u) vOut[k] = (u8)((s_bits[k >> 3] >> (7u - (k & 7u))) & 1u);
  }
  if (kind != kTmbKindBlocks8 && kind != kTmbKindBlocks16)
  {
    if (threadIdx.x == 0) b.tiles[t] = s_ti;
    return;
  }

  // ---- valid pixels per block, then the walk: a sub-block's length follows from its header and the position's valid count
  const u32 MB = kind == kTmbKindBlocks16 ? 16u : 8u;
  tbBlockValidCounts(s_bits, (u32)g.nRows, (u32)g.nCols, MB, s_nv);
  __syncthreads();
  if (threadIdx.x == 0)
  {
    u32* __restrict__ table = b.blockOff + (u64)t * g.posStride;
    BandParams p = tbFillBandParams(g, (int)MB);
    p.nDepth = nD;
    s_ti.head.flags = MB == 16u ? tdbWalkBlocks<(int)TB, 16u>(blob, s_ti.dataBegin, blobEnd, p, table, s_nv)
                                : tdbWalkBlocks<(int)TB, 8u>(blob, s_ti.dataBegin, blobEnd, p, table, s_nv);
    b.tiles[t] = s_ti;
  }
}

// a wave per position, slice after slice: k_decode_tiles (tile_decode.hip) with the tile's own blob, mask and header values; lane l
// holds elements l, l + 64, ... of the block.  A difference block adds the value of the slice in front, which this lane wrote itself;
// lossy values are clamped to the slice's own maximum, read from the blob's ranges.  Pixels of the block that are not valid are
// written as 0.  One launch per block size over the whole batch; a tile of another kind is left alone.
template<class T, int MB>
__global__ void __launch_bounds__(256)
k_tdbd_blocks(TmbGeom g, int nD, const u8* __restrict__ arena, const u64* __restrict__ offsets, T* __restrict__ outAll, TdbDecodeBuffers b)
{
  constexpr int E = MB * MB / 64;
  constexpr u32 TB = (u32)sizeof(T);
  __shared__ u32 s_lut[4][256];
  __shared__ __align__(16) u8 s_head[4][64];
  const u32 t = blockIdx.y;
  const TdbTile& rec = b.tiles[t];
  if (rec.head.flags & ~kTbSibling) return;    // (whatever the parse kernel raised; a sibling wave's kTbSibling: nothing to gain from leaving)
  if (rec.kind != (MB == 8 ? kTmbKindBlocks8 : kTmbKindBlocks16)) return;
  const int w = waveId(), lane = laneId();
  const int pos = (int)blockIdx.x * 4 + w;
  if (pos >= ((g.nRows + MB - 1) / MB) * ((g.nCols + MB - 1) / MB)) return;
  BandParams p = tbFillBandParams(g, MB);
  p.nDepth = nD;
  p.allValid = (rec.numValid == (u32)g.tileElems) ? 1 : 0;
  p.invScale = 2 * rec.maxZErr;
  const u8* __restrict__ blob = arena + offsets[t];
  const u32 blobEnd = rec.head.blobSize;
  const u8* __restrict__ zMaxBytes = blob + kHdr6 + 4u + rec.rleLen + (u32)nD * TB;    // (inside the blob: the parse has checked it)
  const u8* __restrict__ maskBits = b.bits + (u64)t * g.bitStride;
  T* __restrict__ out = outAll + (u64)t * g.tileElems * (u64)nD;
  u32* lut = s_lut[w];
  u8* head = s_head[w];

  const int it = pos / p.nTH, jt = pos - it * p.nTH;
  const int i0 = it * MB, j0 = jt * MB;
  const int tileH = min(MB, p.nRows - i0), tileW = min(MB, p.nCols - j0);
  const int nElem = tileH * tileW;
  int rank[E];
  i64 px[E];
  int nValid = 0;
#pragma unroll
  for (int k = 0; k < E; k++)
  {
    const int e = k * 64 + lane;
    const bool inb = e < nElem;
    const int r = inb ? e / tileW : 0, c = inb ? e - r * tileW : 0;
    px[k] = inb ? (i64)(i0 + r) * p.nCols + (j0 + c) : -1;
    const bool valid = inb && (p.allValid || maskBit(maskBits, px[k]));
    const u64 bal = __ballot(valid);
    rank[k] = valid ? nValid + __popcll(bal & laneMaskLt()) : -1;
    nValid += __popcll(bal);
  }

  u32 off = b.blockOff[(u64)t * g.posStride + pos];
  bool failed = false;
  for (int iD = 0; iD < nD && !failed; iD++)
  {
    head[lane] = ((u64)off + (u64)lane < (u64)blobEnd) ? blob[(u64)off + lane] : (u8)0;
    waveSync();
    BlkInfo bi;
    const int rc = (off < blobEnd) ? parseBlockWords<(int)TB>(reinterpret_cast<const u32*>(head), 0u, blobEnd - off, p, nValid, (u32)nElem, bi) : 1;
    if (rc != 0 || bi.len == 0 || (((u32)bi.flag >> 2) & 14u) != (((u32)j0 >> 3) & 14u) || (bi.diff && (iD == 0 || p.dt >= DT_Float))) { failed = true; break; }
    double offset = 0;
    if (bi.mode == 1 || bi.mode == 3) offset = typedFromBits(getBytes(head + 1, bi.offBytes), bi.dtUsed);
    const double zMax = typedFromBits(getBytes(zMaxBytes + (u64)iD * TB, (int)TB), p.dt);    // zMaxVec[iDepth]
    const u64 payloadBit = 8ull * ((u64)off + bi.payload);
    const int nbIdx = bi.lut ? bitLen(bi.nLut) : 0;
    u64 idxBit = 0;
    if (bi.mode == 1 && bi.lut)
    {
      lut[0] = 0;
      for (u32 i = (u32)lane; i < bi.nLut; i += 64) lut[i + 1] = unstuffElement(blob, payloadBit, i, bi.nb, bi.nLut, blobEnd, p.version);
      idxBit = payloadBit + 8ull * (((u64)bi.nLut * bi.nb + 7) >> 3);
      waveSync();
    }
    bool badIdx = false;
#pragma unroll
    for (int k = 0; k < E; k++)
    {
      if (px[k] < 0) continue;
      const i64 m = px[k] * nD + iD;
      T val = T(0);
      if (rank[k] >= 0)
      {
        if (bi.mode == 2) val = bi.diff ? out[m - 1] : T(0);
        else if (bi.mode == 0)
        {
          const u64 bits = getBytes(blob + off + 1 + (u64)rank[k] * TB, (int)TB);
          memcpy(&val, &bits, sizeof(T));
        }
        else if (bi.mode == 3)
        {
          if (!bi.diff) val = (T)offset;
          else { const double z = offset + (double)out[m - 1]; val = (T)(z < zMax ? z : zMax); }
        }
        else
        {
          u32 q;
          if (!bi.lut) q = unstuffElement(blob, payloadBit, (u32)rank[k], bi.nb, bi.cnt, blobEnd, p.version);
          else
          {
            const u32 ix = unstuffElement(blob, idxBit, (u32)rank[k], nbIdx, bi.cnt, blobEnd, p.version);
            if (ix > bi.nLut) { badIdx = true; q = 0; } else q = lut[ix];
          }
          double z = offset + (double)q * p.invScale;
          if (bi.diff) z = z + (double)out[m - 1];
          val = (T)(z < zMax ? z : zMax);    // std::min(z, zMax)
        }
      }
      out[m] = val;
    }
    if (__any(badIdx)) failed = true;
    off += bi.len;
    waveSync();
  }
  if (failed && lane == 0) atomicOr(&b.tiles[t].head.flags, kTbSibling);
}

template<class T>
static void tdbDecodeT(const TmbGeom& g, int nD, const u8* dArena, const u64* dOffsets, const u32* dSizes, void* dTiles, u8* dValidBytes,
                       const TdbDecodeBuffers& b, hipStream_t st)
{
  const int nPos = g.nTV * g.nTH, nPos16 = ((g.nRows + 15) / 16) * ((g.nCols + 15) / 16);
  if (tbLargeForm(g)) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tdbd_parse<T, true>), dim3(g.nTiles), dim3(256), 0, st, g, nD, dArena, dOffsets, dSizes, (T*)dTiles, dValidBytes, b); }
  else { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tdbd_parse<T, false>), dim3(g.nTiles), dim3(256), 0, st, g, nD, dArena, dOffsets, dSizes, (T*)dTiles, dValidBytes, b); }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tdbd_blocks<T, 8>), dim3((nPos + 3) / 4, g.nTiles), dim3(256), 0, st, g, nD, dArena, dOffsets, (T*)dTiles, b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tdbd_blocks<T, 16>), dim3((nPos16 + 3) / 4, g.nTiles), dim3(256), 0, st, g, nD, dArena, dOffsets, (T*)dTiles, b);
}

void launchTdbDecode(const TmbGeom& g, int nDepth, const u8* dArena, const u64* dOffsets, const u32* dSizes, void* dTiles, u8* dValidBytes,
                     const TdbDecodeBuffers& b, hipStream_t st)
{
  if (nDepth < 1 || nDepth > kTdbMaxDepth) return;    // (the host's check: codec_tiles_batch.cpp)
  switch (g.dt)
  {
    case DT_Short:  tdbDecodeT<short>(g, nDepth, dArena, dOffsets, dSizes, dTiles, dValidBytes, b, st); break;
    case DT_UShort: tdbDecodeT<unsigned short>(g, nDepth, dArena, dOffsets, dSizes, dTiles, dValidBytes, b, st); break;
    case DT_Int:    tdbDecodeT<int>(g, nDepth, dArena, dOffsets, dSizes, dTiles, dValidBytes, b, st); break;
    case DT_UInt:   tdbDecodeT<unsigned int>(g, nDepth, dArena, dOffsets, dSizes, dTiles, dValidBytes, b, st); break;
    case DT_Float:  tdbDecodeT<float>(g, nDepth, dArena, dOffsets, dSizes, dTiles, dValidBytes, b, st); break;
    case DT_Double: tdbDecodeT<double>(g, nDepth, dArena, dOffsets, dSizes, dTiles, dValidBytes, b, st); break;
    default: break;
  }
}

}    // namespace lerc
