// tile_mask_batch.hip -- batches of MASKED tiles: nTiles rasters of one shape, each with a validity mask of its own, encoded into
// (decoded from) nTiles independent Lerc2 blobs by ONE set of launches, a tile per blockIdx.y (or per workgroup) -- no launch, no
// copy and no host wait per tile.
//
// Encode (launchTmbEncode), every section of a masked band's blob made on the device:
//   1. k_tmb_prelude   a workgroup per tile: byte mask -> bit mask (BitMask's layout: most significant bit first) in LDS and in
//                      global memory, the count of valid pixels, the range over them, NaN findings, the tile's own error bound (all-integer
//                      float values, TryRaiseMaxZError; 0 for a float tile without a valid pixel), the tile's kind where the statistics
//                      settle it (empty, constant), and the mask's run-length stream (RLE.cpp:123-254, the same bytes as rleEncode,
//                      codec_common.cpp)
//   2. k_tmb_blocks<8, false>    a wave per 8 x 8 block: the block's size (the general encoder's decisions, tile_encode.hip)
//   3. k_tmb_decide    a workgroup per tile: the sizes' exclusive scan; marks the tiles the low-bit-rate rule (Lerc2.cpp:333-357) sends
//                      to the retry;  k_tmb_blocks<16, false>: the sizes of 16 x 16 blocks of the marked tiles (launched over the whole
//                      batch: the host does not wait to learn which tiles are marked);  k_tmb_decide2: 16 x 16 if no longer (:346),
//                      then one sweep against what is left, the blob's size, the slot check;  k_tmb_arena: one workgroup places the blobs
//                      of every kind in a packed arena (16-byte aligned)
//   4. k_tmb_blocks<8, true>, <16, true>    the blocks' bytes of the tiles of that block size; in the 8 x 8 launch one more workgroup
//                      per tile writes header and mask section, and where the valid pixels differ ranges and the "one sweep" byte --
//                      behind a 1 the valid pixels raw in row order, by their rank among the valid pixels (a workgroup scan over the
//                      popcounts of the bit mask)
//   5. k_tmb_checksum  a workgroup per tile: Fletcher32 over blob[14 ..) (Lerc2.cpp:1037-1064), stored into the header.  It reads
//                      the finished blob, whatever the parity of the mask section's length.
// Tiles that leave the batch (TmbTile::flags: NaN at a valid pixel, no room) are left alone; the host encodes them one by one behind it.
// No workgroup waits for another one inside a launch, so the emulator build runs the same path.
//
// Decode (launchTmbDecode):
//   1. k_tmbd_parse    a workgroup per tile: header (which names the blob's kind: no valid pixel, zMin == zMax, the one-sweep byte,
//                      blocks of 8 x 8 or 16 x 16), Fletcher32, the mask's run-length stream expanded into LDS (bounded by the section's
//                      length and the mask's size), the caller's valid bytes; the pixels of empty, constant and one-sweep blobs; for
//                      blocks the valid counts per block by popcount and the walk over the block headers -- a block's length follows
//                      from its header and its valid count, which is known here -- into a table of block offsets
//   2. k_tmbd_blocks<8>, <16>   a wave per block: the general decoder's block (tile_decode.hip), checked against the table
// Every walk is bounded by the blob's size; whatever does not fit, or is not certain, raises a flag and the host repeats that tile with
// the single-blob decoder, which also yields the exact status of a damaged blob.
#include <cstdio>
#include <cstdlib>
#include "kernels.h"
#include "wave_utils.h"
#include "tile_mask_batch.h"
#include "tile_batch_dev.h"

namespace lerc {

template<class T> struct TmbAcc { typedef i64 type; static __device__ __forceinline__ i64 hi() { return 0x7FFFFFFFFFFFFFFFll; } static __device__ __forceinline__ i64 lo() { return -0x7FFFFFFFFFFFFFFFll - 1; } };
template<> struct TmbAcc<float> { typedef double type; static __device__ __forceinline__ double hi() { return __builtin_huge_val(); } static __device__ __forceinline__ double lo() { return -__builtin_huge_val(); } };
template<> struct TmbAcc<double> { typedef double type; static __device__ __forceinline__ double hi() { return __builtin_huge_val(); } static __device__ __forceinline__ double lo() { return -__builtin_huge_val(); } };

// ================================================================================================
// encode
// ================================================================================================
// BANDS: t is a plane, tile * nBands + band (tile_mask_batch.h); the tile's mask lies at valid + tile * validStride, and only band 0
// makes the mask's run-length stream -- the bands behind it write the count 0, "the mask of the band in front stays in force"
// LARGE: the form for tiles beyond the small form's mask bytes or blocks (tile_batch.h: TbForm), picked by the host from the shape
template<class T, bool BANDS = false, bool LARGE = false>
__global__ void __launch_bounds__(256)
k_tmb_prelude(TmbGeom g, double maxZErr, u32 cand, const T* __restrict__ data, const u8* __restrict__ valid, TmbEncodeBuffers b, u32 nBands,
              u64 validStride)
{
  typedef typename TmbAcc<T>::type Acc;
  constexpr bool isFlt = DtOf<T>::v >= DT_Float;
  __shared__ __align__(16) u8 s_bits[TbForm<LARGE>::kMaskBytes + 16];
  __shared__ u64 s_red[4];
  __shared__ Acc s_mn[4], s_mx[4];
  __shared__ u64 s_raise[4][9];
  const u32 t = blockIdx.x;
  const u32 nPix = (u32)g.tileElems, nBytes = (nPix + 7u) >> 3;
  const T* __restrict__ px = data + (u64)t * g.tileElems;
  const u32 band = BANDS ? t % nBands : 0u;
  const u8* __restrict__ vb = BANDS ? valid + (u64)(t / nBands) * validStride : valid + (u64)t * g.tileElems;
  u8* __restrict__ bitsOut = b.bits + (u64)t * g.bitStride;
  const int facCand[9] = { 1, 2, 10, 20, 100, 200, 1000, 2000, 10000 };

  u32 flags = 0;
  Acc mn = TmbAcc<T>::hi(), mx = TmbAcc<T>::lo();
  bool frac = false;
  double rerr[9];
#pragma unroll
  for (int c = 0; c < 9; c++) rerr[c] = 0;
  const u32 cnt = tbMaskToBits(vb, nPix, s_bits, bitsOut, [&](u32 k)
  {
    const T v = px[k];
    if (isFlt && v != v) { flags |= kTmbNaN; return; }
    const Acc a = (Acc)v;
    mn = a < mn ? a : mn; mx = a > mx ? a : mx;
    if (isFlt)
    {
      const double x = (double)v;
      if (!(v == (T)floor(x + 0.5))) frac = true;    // Lerc.h:271 IsInt
      // TryRaiseMaxZError (Lerc2.cpp:1233-1318): the largest rounding error per candidate factor.  Every factor is a multiple of
      // the ones in front of it, so a value that one factor makes an integer adds nothing to the later ones either way.
#pragma unroll
      for (int c = 0; c < 9; c++)
        if ((cand >> c) & 1u)
        {
          const double z = x * facCand[c];
          const double dlt = fabs(floor(z + 0.5) - z);
          rerr[c] = dlt > rerr[c] ? dlt : rerr[c];
        }
    }
  });
  const u32 numValid = (u32)blockSum((u64)cnt, s_red);
  const u32 anyFlags = (u32)blockSum((u64)flags, s_red) ? kTmbNaN : 0u;    // (the only flag raised so far)
  const u32 anyFrac = (u32)blockSum(frac ? 1ull : 0ull, s_red);
  mn = waveMin(mn); mx = waveMax(mx);
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
  if (laneId() == 0) { s_mn[waveId()] = mn; s_mx[waveId()] = mx; }
  __syncthreads();
  if (threadIdx.x != 0) return;

  for (int w = 1; w < 4; w++) { mn = s_mn[w] < mn ? s_mn[w] : mn; mx = s_mx[w] > mx ? s_mx[w] : mx; }
  TmbTile ti;
  memset(&ti, 0, sizeof(ti));
  ti.numValid = numValid;
  u32 fl = anyFlags;
  ti.kind = (numValid == 0) ? kTmbKindEmpty : (!(mn < mx) ? kTmbKindConst : kTmbKindBlocks8);
  if (numValid)
  {
    ti.zMin = (double)mn; ti.zMax = (double)mx;
    ti.minBits = typedBits(ti.zMin, g.dt); ti.maxBits = typedBits(ti.zMax, g.dt);
  }
  // ---- the tile's own error bound, as Lerc::FilterNoDataAndNaN and Lerc2::TryRaiseMaxZError decide it from the statistics
  // (encodeBand, codec_encode.cpp, restated per tile): float values that are all integers inside the type's exact range make the
  // tile an integer one (isInt in the header, bound max(0.5, floor)); else the first candidate bound every valid value agrees with
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

  // ---- the mask's run-length stream (tbMaskRle)
  u32 rleLen = 0;
  if (fl == 0 && numValid > 0 && numValid < nPix && band == 0)
  {
    rleLen = tbMaskRle(s_bits, nBytes, b.rle + (u64)t * g.rleStride, g.rleStride);
    if (!rleLen) fl |= kTmbRle;
  }
  ti.head.flags = fl;
  ti.rleLen = rleLen;
  // header and mask section; where pixels differ: ranges and the "one sweep" byte
  ti.dataBegin = kHdr6 + 4u + rleLen + (ti.kind == kTmbKindBlocks8 ? 2u * (u32)sizeof(T) + 1u : 0u);
  ti.mbSize = 8u;
  if (BANDS) ti.nBlobsMore = nBands - 1u - band;
  ti.head.blobSize = ti.dataBegin;    // (all there is of an empty or a constant tile; the others: k_tmb_decide2)
  b.tiles[t] = ti;
}

// What lies in front of a tile's block stream, by one workgroup: header (Lerc2.cpp:724-786; checksum patched by k_tmb_checksum),
// mask section; where the valid pixels differ: ranges and the "one sweep" byte, and behind a 1 the valid pixels raw in row
// order (Lerc2::WriteDataOneSweep).  s_hdr: 96 bytes of LDS, s_w: 4 words.
template<class T>
__device__ __forceinline__ void tmbWriteFront(const TmbGeom& g, u32 t, const TmbTile& ti, const T* __restrict__ px, u8* __restrict__ blob, const TmbEncodeBuffers& b,
                                              u8* s_hdr, u32* s_w)
{
  const TbHeader6 h = { kCodecVersion, 0u, g.nRows, g.nCols, 1, (int)ti.numValid, (int)ti.mbSize, (int)ti.head.blobSize, g.dt, (int)ti.nBlobsMore,
                        ti.isInt ? 0x100u : 0u, ti.maxZErr, ti.zMin, ti.zMax };
  tbWriteHeaderMask(blob, h, b.rle + (u64)t * g.rleStride, ti.rleLen, s_hdr);
  if (ti.kind == kTmbKindEmpty || ti.kind == kTmbKindConst) return;    // (Lerc2.cpp:235-241, :255: nothing behind the mask)
  if (threadIdx.x == 0)
  {
    u8* r = blob + kHdr6 + 4u + ti.rleLen;
    putBytes(r, ti.minBits, (int)sizeof(T));
    putBytes(r + sizeof(T), ti.maxBits, (int)sizeof(T));
    r[2 * sizeof(T)] = ti.kind == kTmbKindOneSweep ? 1 : 0;
  }
  if (ti.kind != kTmbKindOneSweep) return;
  u8* __restrict__ dst = blob + ti.dataBegin;    // (any alignment: bytes)
  auto put = [&](u32 k, bool valid, u32 rank)
  {
    if (!valid) return;
    u64 bits = 0;
    const T v = px[k];
    memcpy(&bits, &v, sizeof(T));
    putBytes(dst + (u64)rank * sizeof(T), bits, (int)sizeof(T));
  };
  const u32 nPix = (u32)g.tileElems;
  if (ti.numValid == nPix) { for (u32 k = threadIdx.x; k < nPix; k += 256u) put(k, true, k); }
  else tbRankedSweep(b.bits + (u64)t * g.bitStride, nPix, s_w, put);
}

// A wave per MB x MB block of a tile (blockIdx.y): k_encode_tiles (tile_encode.hip) for one value a pixel, with the tile's own mask,
// "all valid" and place in the arena; lane l holds elements l, l + 64, ... of the block.  Sizes: 8 x 8 for every tile with blocks,
// 16 x 16 for the tiles k_tmb_decide marked.  WRITE: the tiles of that block size, and in the 8 x 8 launch one more workgroup behind
// a tile's last block that writes what lies in front of the block stream -- for a tile of any kind.
template<class T, int MB, bool WRITE>
__global__ void __launch_bounds__(256)
k_tmb_blocks(TmbGeom g, BandParams p, const T* __restrict__ data, u8* __restrict__ arena, TmbEncodeBuffers b)
{
  constexpr int E = MB * MB / 64, NMAX = MB * MB;
  constexpr int OBW = (1 + NMAX * (int)sizeof(T) + 3) / 4 + 4;
  __shared__ T s_val[4][NMAX];
  __shared__ u32 s_obuf[4][WRITE ? OBW : 1];
  __shared__ u32 s_lut[4][WRITE ? NMAX : 1];
  const u32 t = blockIdx.y;
  const TmbTile ti = b.tiles[t];
  if (ti.head.flags) return;
  const int nTV = (g.nRows + MB - 1) / MB, nTH = (g.nCols + MB - 1) / MB;
  u8* __restrict__ blob = WRITE ? arena + ti.head.offset : nullptr;
  const T* __restrict__ px = data + (u64)t * g.tileElems;

  if constexpr (WRITE && MB == 8)
  {
    __shared__ u8 s_hdr[96];
    __shared__ u32 s_w[4];
    if (blockIdx.x == gridDim.x - 1) { tmbWriteFront<T>(g, t, ti, px, blob, b, s_hdr, s_w); return; }
  }
  if (WRITE ? ti.kind != (MB == 8 ? kTmbKindBlocks8 : kTmbKindBlocks16) : (ti.kind != kTmbKindBlocks8 || (MB == 16 && !ti.retry))) return;

  const int w = waveId();
  const int pos = (int)blockIdx.x * 4 + w;
  if (pos >= nTV * nTH) return;    // whole wave leaves together
  p.mb = MB; p.nTV = nTV; p.nTH = nTH;
  p.allValid = (ti.numValid == (u32)g.tileElems) ? 1 : 0;
  p.maxZErr = ti.maxZErr; p.scale = 1 / (2 * ti.maxZErr); p.invScale = 2 * ti.maxZErr;    // (the tile's own bound: k_tmb_prelude)
  tbEncodeBlock<T, E, true, WRITE>(p, pos, px, b.bits + (u64)t * g.bitStride, MB == 8 ? b.blockOff + (u64)t * g.posStride : b.blockOff16 + (u64)t * g.pos16Stride,
                                   WRITE ? blob + ti.dataBegin : nullptr, s_val[w], s_obuf[w], s_lut[w]);
}

// the 8 x 8 blocks' sizes scanned, and whether the low-bit-rate rule asks for the sizes of 16 x 16 blocks too
__global__ void __launch_bounds__(256) k_tmb_decide(TmbGeom g, u32 tb, TmbEncodeBuffers b)
{
  __shared__ u32 s_scan[257];
  const u32 t = blockIdx.x;
  if (b.tiles[t].head.flags || b.tiles[t].kind != kTmbKindBlocks8) return;    // (neither is written in this kernel)
  const u32 nPos = (u32)(g.nTV * g.nTH);
  const u32 nBytesTiling = blockScanInPlace(b.blockOff + (u64)t * g.posStride, nPos, s_scan);
  if (threadIdx.x != 0) return;
  TmbTile& ti = b.tiles[t];
  const u64 nPix = g.tileElems, oneSweep = (u64)tb * ti.numValid;
  // 16 x 16 blocks at low bit rates (Lerc2.cpp:333-357; nPix counts invalid pixels too)
  ti.retry = ((double)((u64)nBytesTiling * 8u) < (double)nPix * 1.5 && (u64)nBytesTiling < 4u * oneSweep && (g.nRows > 8 || g.nCols > 8)) ? 1u : 0u;
  ti.nBytesTiling = nBytesTiling;
}

// Lerc2.cpp:330-381 from the retry on: 16 x 16 blocks if they are no longer than the 8 x 8 ones (:346), one sweep if it is no
// longer than the blocks that are left, the blob's size, the slot check
__global__ void __launch_bounds__(256) k_tmb_decide2(TmbGeom g, u32 tb, u64 slotBytes, u64 firstTile, TmbEncodeBuffers b)
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
  TmbTile& ti = b.tiles[t];
  if (blocks)
  {
    if (retry && nBytes16 <= ti.nBytesTiling) { ti.kind = kTmbKindBlocks16; ti.mbSize = 16u; ti.nBytesTiling = nBytes16; }
    const u64 oneSweep = (u64)tb * ti.numValid;
    if (oneSweep <= (u64)ti.nBytesTiling) { ti.kind = kTmbKindOneSweep; ti.head.blobSize = ti.dataBegin + (u32)oneSweep; }
    else ti.head.blobSize = ti.dataBegin + ti.nBytesTiling;
  }
  if (slotBytes)
  {
    ti.head.offset = (firstTile + t) * slotBytes;
    if ((u64)ti.head.blobSize > slotBytes) ti.head.flags = kTbCapacity;
  }
}

__global__ void __launch_bounds__(256) k_tmb_arena(u32 nTiles, u64 arenaBase, u64 arenaCapacity, TmbEncodeBuffers b)
{
  __shared__ u64 s_part[257];
  tbArenaPlace(b.tiles, nTiles, arenaBase, arenaCapacity, s_part);
}

__global__ void __launch_bounds__(256) k_tmb_checksum(u8* __restrict__ arena, TmbEncodeBuffers b)
{
  __shared__ u64 s_red[4];
  tbWriteChecksum(arena, b.tiles[blockIdx.x].head, s_red);
}

// band stacks: ONE workgroup folds the planes into tiles and places the tiles (tbPlaceBands, tile_batch_dev.h)
__global__ void __launch_bounds__(256) k_tmb_place_bands(u32 nTiles, u32 nBands, u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile,
                                                         TmbEncodeBuffers b)
{
  __shared__ u64 s[257];
  tbPlaceBands(b.tiles, nTiles, nBands, arenaBase, arenaCapacity, slotBytes, firstTile, s);
}

template<class T>
static void tmbEncodeBandsT(const TmbGeom& g, u32 nBands, const BandParams& bp, double maxZErr, u32 cand, const void* dTiles, const u8* dValidBytes,
                            u64 validStride, u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile, const TmbEncodeBuffers& b,
                            hipStream_t st)
{
  // (the single-band launch set over the planes; the slot check and the placement are k_tmb_place_bands' for whole tiles)
  const int nPos = g.nTV * g.nTH, nPos16 = ((g.nRows + 15) / 16) * ((g.nCols + 15) / 16);
  const dim3 perPlane(g.nTiles), blk(256);
  if (tbLargeForm(g)) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmb_prelude<T, true, true>), perPlane, blk, 0, st, g, maxZErr, cand, (const T*)dTiles, dValidBytes, b, nBands, validStride); }
  else { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmb_prelude<T, true, false>), perPlane, blk, 0, st, g, maxZErr, cand, (const T*)dTiles, dValidBytes, b, nBands, validStride); }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmb_blocks<T, 8, false>), dim3((nPos + 3) / 4, g.nTiles), blk, 0, st, g, bp, (const T*)dTiles, (u8*)nullptr, b);
  hipLaunchKernelGGL(k_tmb_decide, perPlane, blk, 0, st, g, (u32)sizeof(T), b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmb_blocks<T, 16, false>), dim3((nPos16 + 3) / 4, g.nTiles), blk, 0, st, g, bp, (const T*)dTiles, (u8*)nullptr, b);
  hipLaunchKernelGGL(k_tmb_decide2, perPlane, blk, 0, st, g, (u32)sizeof(T), (u64)0, (u64)0, b);
  hipLaunchKernelGGL(k_tmb_place_bands, dim3(1), blk, 0, st, g.nTiles / nBands, nBands, arenaBase, arenaCapacity, slotBytes, firstTile, b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmb_blocks<T, 8, true>), dim3((nPos + 3) / 4 + 1, g.nTiles), blk, 0, st, g, bp, (const T*)dTiles, dArena, b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmb_blocks<T, 16, true>), dim3((nPos16 + 3) / 4, g.nTiles), blk, 0, st, g, bp, (const T*)dTiles, dArena, b);
  hipLaunchKernelGGL(k_tmb_checksum, perPlane, blk, 0, st, dArena, b);
}

void launchTmbEncodeBands(const TmbGeom& g, u32 nBands, const BandParams& bp, double maxZErr, u32 cand, const void* dTiles, const u8* dValidBytes,
                          u64 validStride, u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile, const TmbEncodeBuffers& b, hipStream_t st)
{
  switch (g.dt)
  {
    case DT_Short:  tmbEncodeBandsT<short>(g, nBands, bp, maxZErr, cand, dTiles, dValidBytes, validStride, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_UShort: tmbEncodeBandsT<unsigned short>(g, nBands, bp, maxZErr, cand, dTiles, dValidBytes, validStride, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_Int:    tmbEncodeBandsT<int>(g, nBands, bp, maxZErr, cand, dTiles, dValidBytes, validStride, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_UInt:   tmbEncodeBandsT<unsigned int>(g, nBands, bp, maxZErr, cand, dTiles, dValidBytes, validStride, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_Float:  tmbEncodeBandsT<float>(g, nBands, bp, maxZErr, cand, dTiles, dValidBytes, validStride, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_Double: tmbEncodeBandsT<double>(g, nBands, bp, maxZErr, cand, dTiles, dValidBytes, validStride, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    default: break;
  }
}

template<class T>
static void tmbEncodeT(const TmbGeom& g, const BandParams& bp, double maxZErr, u32 cand, const void* dTiles, const u8* dValidBytes, u8* dArena,
                       u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile, const TmbEncodeBuffers& b, hipStream_t st)
{
  const int nPos = g.nTV * g.nTH, nPos16 = ((g.nRows + 15) / 16) * ((g.nCols + 15) / 16);
  const dim3 perTile(g.nTiles), blk(256);
  if (tbLargeForm(g)) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmb_prelude<T, false, true>), perTile, blk, 0, st, g, maxZErr, cand, (const T*)dTiles, dValidBytes, b, 1u, (u64)0); }
  else { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmb_prelude<T, false, false>), perTile, blk, 0, st, g, maxZErr, cand, (const T*)dTiles, dValidBytes, b, 1u, (u64)0); }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmb_blocks<T, 8, false>), dim3((nPos + 3) / 4, g.nTiles), blk, 0, st, g, bp, (const T*)dTiles, (u8*)nullptr, b);
  hipLaunchKernelGGL(k_tmb_decide, perTile, blk, 0, st, g, (u32)sizeof(T), b);
  // (over the whole batch, whether a tile is marked or not: the host knows nothing yet, and does not wait to learn it)
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmb_blocks<T, 16, false>), dim3((nPos16 + 3) / 4, g.nTiles), blk, 0, st, g, bp, (const T*)dTiles, (u8*)nullptr, b);
  hipLaunchKernelGGL(k_tmb_decide2, perTile, blk, 0, st, g, (u32)sizeof(T), slotBytes, firstTile, b);
  if (!slotBytes) hipLaunchKernelGGL(k_tmb_arena, dim3(1), blk, 0, st, g.nTiles, arenaBase, arenaCapacity, b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmb_blocks<T, 8, true>), dim3((nPos + 3) / 4 + 1, g.nTiles), blk, 0, st, g, bp, (const T*)dTiles, dArena, b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmb_blocks<T, 16, true>), dim3((nPos16 + 3) / 4, g.nTiles), blk, 0, st, g, bp, (const T*)dTiles, dArena, b);
  hipLaunchKernelGGL(k_tmb_checksum, perTile, blk, 0, st, dArena, b);
}

void launchTmbEncode(const TmbGeom& g, const BandParams& bp, double maxZErr, u32 cand, const void* dTiles, const u8* dValidBytes, u8* dArena,
                     u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile, const TmbEncodeBuffers& b, hipStream_t st)
{
  switch (g.dt)
  {
    case DT_Short:  tmbEncodeT<short>(g, bp, maxZErr, cand, dTiles, dValidBytes, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_UShort: tmbEncodeT<unsigned short>(g, bp, maxZErr, cand, dTiles, dValidBytes, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_Int:    tmbEncodeT<int>(g, bp, maxZErr, cand, dTiles, dValidBytes, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_UInt:   tmbEncodeT<unsigned int>(g, bp, maxZErr, cand, dTiles, dValidBytes, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_Float:  tmbEncodeT<float>(g, bp, maxZErr, cand, dTiles, dValidBytes, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    case DT_Double: tmbEncodeT<double>(g, bp, maxZErr, cand, dTiles, dValidBytes, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st); break;
    default: break;
  }
}

// ================================================================================================
// decode
// ================================================================================================
// is z a value of type T (so that (T)z means the same everywhere)?
template<class T> __device__ __forceinline__ bool tmbIsValueOf(double z)
{
  if (DtOf<T>::v == DT_Double) return z == z;
  if (DtOf<T>::v == DT_Float) return (double)(float)z == z;
  const double lo = (DtOf<T>::v == DT_Short) ? -32768.0 : (DtOf<T>::v == DT_Int) ? -2147483648.0 : 0.0;
  const double hi = (DtOf<T>::v == DT_Short) ? 32767.0 : (DtOf<T>::v == DT_UShort) ? 65535.0 : (DtOf<T>::v == DT_Int) ? 2147483647.0 : 4294967295.0;
  return z >= lo && z <= hi && z == floor(z);
}

// band stacks: a thread per tile walks the chain of band blobs (tbBandChain, tile_batch_dev.h)
__global__ void __launch_bounds__(256)
k_tmbd_chain(TmbGeom g, u32 nTiles, u32 nBands, const u8* __restrict__ arena, const u64* __restrict__ offsets, const u32* __restrict__ sizes,
             u64* __restrict__ planeOff, u32* __restrict__ planeSize)
{
  tbBandChain(g, nTiles, nBands, arena, offsets, sizes, planeOff, planeSize);
}

// BANDS: t is a plane, tile * nBands + band, offsets / sizes are the planes' (k_tmbd_chain).  A band behind band 0 carries no mask
// section of its own: its count of valid pixels is band 0's, and between none and all it takes band 0's run-length stream ("the mask
// stays in force").  A band with a mask section of its own, or a count that is not band 0's, is refused: the single-blob decoder
// takes the whole stack.  The caller's valid bytes are written by band 0; without them a blob with an invalid pixel is refused.
template<class T, bool BANDS = false, bool LARGE = false>
__global__ void __launch_bounds__(256)
k_tmbd_parse(TmbGeom g, const u8* __restrict__ arena, const u64* __restrict__ offsets, const u32* __restrict__ sizes, T* __restrict__ outAll,
             u8* __restrict__ validOut, TmbDecodeBuffers b, u32 nBands)
{
  constexpr u32 TB = (u32)sizeof(T);
  __shared__ __align__(16) u8 s_bits[TbForm<LARGE>::kMaskBytes + 16];
  __shared__ u16 s_nv[TbForm<LARGE>::kBlocks];
  __shared__ u64 s_red[4];
  __shared__ u32 s_w[4];
  __shared__ TmbTile s_ti;
  __shared__ u32 s_flags, s_nm;
  const u32 t = blockIdx.x;
  const u8* __restrict__ blob = arena + offsets[t];
  const u32 sizeGiven = sizes[t];
  const u32 nPix = (u32)g.tileElems, nBytes = (nPix + 7u) >> 3;
  const u32 band = BANDS ? t % nBands : 0u, plane0 = t - band;
  // (band 0's blob: read by the bands behind it only where their own header, and so the chain, has held)
  const u8* __restrict__ blob0 = BANDS ? arena + offsets[plane0] : blob;
  const u32 size0 = BANDS ? sizes[plane0] : sizeGiven;

  if (threadIdx.x == 0)
  {
    TmbTile ti;
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
      if (h.version != kCodecVersion || h.nRows != g.nRows || h.nCols != g.nCols || h.nDepth != 1 || h.numValid < 0 || (u32)h.numValid > nPix
        || (h.microBlockSize != 8 && h.microBlockSize != 16) || h.blobSize < (int)(kHdr6 + 4u) || (u32)h.blobSize > sizeGiven || h.dt != g.dt || h.nBlobsMore != (BANDS ? (int)(nBands - 1u - band) : 0)
        || (h.flagBytes & 0xFFu) != 0u)
        fl = kTbHeader;
      if (BANDS && !fl)
      {
        if (!validOut && (u32)h.numValid != nPix) fl = kTbHeader;
        if (band > 0 && (size0 < kHdr6 + 4u || (u32)getBytes(blob0 + 26, 4) != (u32)h.numValid)) fl = kTbHeader;
      }
      const int mbSize = h.microBlockSize;
      if (!fl)
      {
        nm = (u32)getBytes(blob + kHdr6, 4);
        const bool noStream = ti.numValid == nPix || ti.numValid == 0u;
        if ((noStream || band > 0u) ? nm != 0u : (nm < 2u || nm > ti.head.blobSize)) fl = kTbHeader;
        else if (ti.numValid == 0u)
        {
          // no valid pixel: nothing may follow the mask section's length (Lerc2.cpp:235-241); range and error bound are not asked
          ti.kind = kTmbKindEmpty;
          if (ti.head.blobSize != kHdr6 + 4u) fl = kTbHeader;
        }
        else if (ti.zMin == ti.zMax)
        {
          // every valid pixel is (T)zMin (Lerc2.cpp:255, FillConstImage): nothing may follow the mask section
          ti.kind = kTmbKindConst;
          if ((u64)ti.head.blobSize != (u64)kHdr6 + 4u + nm || !tmbIsValueOf<T>(ti.zMin)) fl = kTbHeader;
          ti.minBits = typedBits(ti.zMin, g.dt);
        }
        else if (!(ti.zMin < ti.zMax) || (u64)kHdr6 + 4u + nm + 2u * TB + 1u >= (u64)ti.head.blobSize) fl = kTbHeader;    // (NaN fails every comparison)
        else
        {
          const u8* r = blob + kHdr6 + 4u + nm;
          ti.minBits = getBytes(r, (int)TB); ti.maxBits = getBytes(r + TB, (int)TB);
          ti.dataBegin = kHdr6 + 4u + nm + 2u * TB + 1u;
          if (ti.minBits == ti.maxBits) fl = kTbHeader;    // (constant by its ranges)
          else if (r[2 * TB] == 1)
          {
            // one sweep: the blob ends behind numValid raw values (Lerc2::ReadDataOneSweep); the mask's own count is compared below
            ti.kind = kTmbKindOneSweep;
            if ((u64)ti.dataBegin + (u64)ti.numValid * TB != (u64)ti.head.blobSize) fl = kTbHeader;
          }
          else if (r[2 * TB] != 0) fl = kTbHeader;
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

  // ---- the mask: all ones, all zeros, or the run-length stream expanded (rleDecode, codec_common.cpp: what it does not fill stays zero)
  const bool allValid = s_ti.numValid == nPix;
  for (u32 i = threadIdx.x; i < nBytes + 16u; i += 256u) s_bits[i] = (allValid && i < nBytes) ? (u8)0xFF : (u8)0;
  __syncthreads();
  if (!allValid && kind != kTmbKindEmpty && threadIdx.x == 0)
  {
    if (band > 0u)
    {
      const u32 nm0 = (u32)getBytes(blob0 + kHdr6, 4);
      if (nm0 < 2u || (u64)kHdr6 + 4u + nm0 > (u64)size0 || !tbMaskUnrle(blob0 + kHdr6 + 4u, nm0, s_bits, nBytes)) s_flags = kTmbMaskStream;
    }
    else if (!tbMaskUnrle(blob + kHdr6 + 4u, nm, s_bits, nBytes)) s_flags = kTmbMaskStream;
  }
  __syncthreads();
  if (s_flags) { if (threadIdx.x == 0) { s_ti.head.flags = s_flags; b.tiles[t] = s_ti; } return; }
  // (a mask taken over from band 0 must hold this band's count, whatever the band's kind)
  if (band > 0u && !allValid && kind != kTmbKindEmpty && tbMaskCount(s_bits, nPix, s_red) != s_ti.numValid)
  {
    if (threadIdx.x == 0) { s_ti.head.flags = kTbHeader; b.tiles[t] = s_ti; }
    return;
  }

  T* __restrict__ out = outAll + (u64)t * g.tileElems;
  if (kind == kTmbKindConst || kind == kTmbKindOneSweep)
  {
    // ---- pixels by the mask alone.  A mask that names another number of valid pixels than the header does is the single-blob
    // decoder's business (it asks the mask, codec_decode.cpp): nothing has been written yet.
    const u8* __restrict__ raw = blob + s_ti.dataBegin;
    const u64 constBits = s_ti.minBits;
    const bool sweep = kind == kTmbKindOneSweep;
    if (tbMaskCount(s_bits, nPix, s_red) != s_ti.numValid)
    {
      if (threadIdx.x == 0) { s_ti.head.flags = kTbHeader; b.tiles[t] = s_ti; }
      return;
    }
    tbRankedSweep(s_bits, nPix, s_w, [&](u32 k, bool valid, u32 rank)
    {
      const u64 bits = !valid ? 0ull : sweep ? getBytes(raw + (u64)rank * TB, (int)TB) : constBits;    // (0 where nothing is valid, like FillConstImage)
      T v; memcpy(&v, &bits, sizeof(T));
      out[k] = v;
    });
  }
  else if (kind == kTmbKindEmpty)
    for (u32 k = threadIdx.x; k < nPix; k += 256u) out[k] = T(0);

  // ---- the bit mask for the block kernel, the caller's valid bytes
  u8* __restrict__ bitsOut = b.bits + (u64)t * g.bitStride;
  for (u32 i = threadIdx.x; i < nBytes; i += 256u) bitsOut[i] = s_bits[i];
  if (!BANDS || (band == 0u && validOut))
  {
    u8* __restrict__ vOut = validOut + (u64)(BANDS ? t / nBands : t) * g.tileElems;
    for (u32 k = threadIdx.x; k < nPix; k += 256u) vOut[k] = (u8)((s_bits[k >> 3] >> (7u - (k & 7u))) & 1u);
  }
  if (kind != kTmbKindBlocks8 && kind != kTmbKindBlocks16)
  {
    if (threadIdx.x == 0) b.tiles[t] = s_ti;
    return;
  }

  // ---- valid pixels per block
  const u32 MB = kind == kTmbKindBlocks16 ? 16u : 8u;
  tbBlockValidCounts(s_bits, (u32)g.nRows, (u32)g.nCols, MB, s_nv);
  __syncthreads();

  // ---- the walk: a block's length follows from its header and its valid count
  if (threadIdx.x == 0)
  {
    u32* __restrict__ table = b.blockOff + (u64)t * g.posStride;
    auto nValidOf = [&](u32 k, u32) { return (int)s_nv[k]; };
    s_ti.head.flags = MB == 16u ? tbWalkBlocks<(int)TB, 16u>(blob, s_ti.dataBegin, blobEnd, tbFillBandParams(g, 16), table, nValidOf)
                                : tbWalkBlocks<(int)TB, 8u>(blob, s_ti.dataBegin, blobEnd, tbFillBandParams(g, 8), table, nValidOf);
    b.tiles[t] = s_ti;
  }
}

// a wave per block: k_decode_tiles (tile_decode.hip) for one value a pixel, with the tile's own blob, mask and header values; lane l
// holds elements l, l + 64, ... of the block.  One launch per block size over the whole batch; a tile of another kind is left alone.
template<class T, int MB>
__global__ void __launch_bounds__(256)
k_tmbd_blocks(TmbGeom g, const u8* __restrict__ arena, const u64* __restrict__ offsets, T* __restrict__ outAll, TmbDecodeBuffers b)
{
  constexpr int E = MB * MB / 64;
  __shared__ u32 s_lut[4][256];
  __shared__ __align__(16) u8 s_head[4][64];
  const u32 t = blockIdx.y;
  if (b.tiles[t].head.flags & ~kTbSibling) return;    // (whatever the parse kernel raised; a sibling wave's kTbSibling: nothing to gain from leaving)
  if (b.tiles[t].kind != (MB == 8 ? kTmbKindBlocks8 : kTmbKindBlocks16)) return;
  const int w = waveId();
  const int pos = (int)blockIdx.x * 4 + w;
  if (pos >= ((g.nRows + MB - 1) / MB) * ((g.nCols + MB - 1) / MB)) return;
  BandParams p = tbFillBandParams(g, MB);
  p.allValid = (b.tiles[t].numValid == (u32)g.tileElems) ? 1 : 0;
  p.invScale = 2 * b.tiles[t].maxZErr;
  const bool failed = tbDecodeBlock<T, E, true>(p, b.tiles[t].zMax, pos, arena + offsets[t], b.tiles[t].head.blobSize, b.blockOff[(u64)t * g.posStride + pos],
                                                b.bits + (u64)t * g.bitStride, outAll + (u64)t * g.tileElems, s_lut[w], s_head[w]);
  if (failed && laneId() == 0) atomicOr(&b.tiles[t].head.flags, kTbSibling);
}

template<class T>
static void tmbDecodeT(const TmbGeom& g, const u8* dArena, const u64* dOffsets, const u32* dSizes, void* dTiles, u8* dValidBytes,
                       const TmbDecodeBuffers& b, hipStream_t st)
{
  const int nPos = g.nTV * g.nTH, nPos16 = ((g.nRows + 15) / 16) * ((g.nCols + 15) / 16);
  if (tbLargeForm(g)) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmbd_parse<T, false, true>), dim3(g.nTiles), dim3(256), 0, st, g, dArena, dOffsets, dSizes, (T*)dTiles, dValidBytes, b, 1u); }
  else { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmbd_parse<T, false, false>), dim3(g.nTiles), dim3(256), 0, st, g, dArena, dOffsets, dSizes, (T*)dTiles, dValidBytes, b, 1u); }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmbd_blocks<T, 8>), dim3((nPos + 3) / 4, g.nTiles), dim3(256), 0, st, g, dArena, dOffsets, (T*)dTiles, b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmbd_blocks<T, 16>), dim3((nPos16 + 3) / 4, g.nTiles), dim3(256), 0, st, g, dArena, dOffsets, (T*)dTiles, b);
}

template<class T>
static void tmbDecodeBandsT(const TmbGeom& g, u32 nBands, const u8* dArena, const u64* dOffsets, const u32* dSizes, u64* planeOff, u32* planeSize,
                            void* dTiles, u8* dValidBytes, const TmbDecodeBuffers& b, hipStream_t st)
{
  const int nPos = g.nTV * g.nTH, nPos16 = ((g.nRows + 15) / 16) * ((g.nCols + 15) / 16);
  const u32 nTiles = g.nTiles / nBands;
  hipLaunchKernelGGL(k_tmbd_chain, dim3((nTiles + 255u) / 256u), dim3(256), 0, st, g, nTiles, nBands, dArena, dOffsets, dSizes, planeOff, planeSize);
  if (tbLargeForm(g)) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmbd_parse<T, true, true>), dim3(g.nTiles), dim3(256), 0, st, g, dArena, (const u64*)planeOff, (const u32*)planeSize, (T*)dTiles,
                                         dValidBytes, b, nBands); }
  else { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmbd_parse<T, true, false>), dim3(g.nTiles), dim3(256), 0, st, g, dArena, (const u64*)planeOff, (const u32*)planeSize, (T*)dTiles,
                          dValidBytes, b, nBands); }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmbd_blocks<T, 8>), dim3((nPos + 3) / 4, g.nTiles), dim3(256), 0, st, g, dArena, (const u64*)planeOff, (T*)dTiles, b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tmbd_blocks<T, 16>), dim3((nPos16 + 3) / 4, g.nTiles), dim3(256), 0, st, g, dArena, (const u64*)planeOff, (T*)dTiles, b);
}

void launchTmbDecodeBands(const TmbGeom& g, u32 nBands, const u8* dArena, const u64* dOffsets, const u32* dSizes, u64* planeOff, u32* planeSize,
                          void* dTiles, u8* dValidBytes, const TmbDecodeBuffers& b, hipStream_t st)
{
  switch (g.dt)
  {
    case DT_Short:  tmbDecodeBandsT<short>(g, nBands, dArena, dOffsets, dSizes, planeOff, planeSize, dTiles, dValidBytes, b, st); break;
    case DT_UShort: tmbDecodeBandsT<unsigned short>(g, nBands, dArena, dOffsets, dSizes, planeOff, planeSize, dTiles, dValidBytes, b, st); break;
    case DT_Int:    tmbDecodeBandsT<int>(g, nBands, dArena, dOffsets, dSizes, planeOff, planeSize, dTiles, dValidBytes, b, st); break;
    case DT_UInt:   tmbDecodeBandsT<unsigned int>(g, nBands, dArena, dOffsets, dSizes, planeOff, planeSize, dTiles, dValidBytes, b, st); break;
    case DT_Float:  tmbDecodeBandsT<float>(g, nBands, dArena, dOffsets, dSizes, planeOff, planeSize, dTiles, dValidBytes, b, st); break;
    case DT_Double: tmbDecodeBandsT<double>(g, nBands, dArena, dOffsets, dSizes, planeOff, planeSize, dTiles, dValidBytes, b, st); break;
    default: break;
  }
}

void launchTmbDecode(const TmbGeom& g, const u8* dArena, const u64* dOffsets, const u32* dSizes, void* dTiles, u8* dValidBytes,
                     const TmbDecodeBuffers& b, hipStream_t st)
{
  switch (g.dt)
  {
    case DT_Short:  tmbDecodeT<short>(g, dArena, dOffsets, dSizes, dTiles, dValidBytes, b, st); break;
    case DT_UShort: tmbDecodeT<unsigned short>(g, dArena, dOffsets, dSizes, dTiles, dValidBytes, b, st); break;
    case DT_Int:    tmbDecodeT<int>(g, dArena, dOffsets, dSizes, dTiles, dValidBytes, b, st); break;
    case DT_UInt:   tmbDecodeT<unsigned int>(g, dArena, dOffsets, dSizes, dTiles, dValidBytes, b, st); break;
    case DT_Float:  tmbDecodeT<float>(g, dArena, dOffsets, dSizes, dTiles, dValidBytes, b, st); break;
    case DT_Double: tmbDecodeT<double>(g, dArena, dOffsets, dSizes, dTiles, dValidBytes, b, st); break;
    default: break;
  }
}

}    // namespace lerc
