// raster_tiles_depth.hip -- the staging pass of the DEPTH raster calls (lerc_amd_depth.h, codec_raster_tiles.cpp) for every layout
// but packed pixels: element (row i, column j, depth d) of the raster lies at i * rowPitch + j * pixelPitch + d * depthPitch, and the
// staged form the depth tile batches take is [n][r][c][nDepth], pixels packed.  k_rtd_cut gathers the rectangles of a chunk of tiles
// into it, k_rtd_paste scatters them back -- clipped to a window of the raster, so that the whole-raster decode (the window that covers
// everything) and lerc_amd_decode_raster_window_device_depth are one kernel.  The mirror of raster_tiles_px.hip: there the raster is
// interleaved and the staged form planes, here the staged form is interleaved and the raster is
//   planes, lines  (pixelPitch 1: the nDepth rows of a raster row lie depthPitch apart -- [C, H, W], GDAL's INTERLEAVE=LINE), or
//   gapped pixels  (depthPitch 1, pixelPitch > nDepth: RGB out of RGBA).
// Packed pixels (pixelPitch == nDepth) are runs of elements and go through k_rt_cut / k_rt_paste / k_rw_paste; the kernels here take
// them too (as gapped pixels without a gap), which the host uses only where a row's element count leaves 32 bits.
//
// A bandwidth kernel with a transposition in the middle.  A unit is a strip of kRtPxRows rows of one tile, a half-wave of 32 lanes has
// a row, a row goes in segments of kRtPxSegBytes / sizeof(T) pixels through the LDS slot of raster_tiles_px.hip (kRtPxSlotDwords a
// row: 37376 bytes a workgroup, whatever the tile's width), in its layout: one padding dword after every 16 * pitch bytes of the
// interleaved run, which sits in LDS as far behind a 16-byte boundary as it does in memory (raster_tiles_dev.h).
//
// Planes and lines.  Cut: (1) each of the nDepth source rows of the segment is read in 16-byte vectors from its first 16-byte aligned
// address on, head and tail by the element, and a lane spreads the V = 16 / sizeof(T) pixels of a vector to where the staged run has
// them, nDepth elements apart; (2) the staged run of np * nDepth elements goes out as it lies, whole 16-byte vectors from the first
// aligned staged address on.  Paste: (1) the staged run is copied to LDS as it lies, (2) per depth a lane collects V pixels and stores
// them as one vector at a 16-byte aligned address of the destination row, the pixels in front of the first such address and behind
// the last whole vector by the element.  The pitch of the layout is nDepth, and the conflict degrees are those raster_tiles_px.hip
// names, counted by tools/lds_conflicts_px.py (its rows P = nDepth): the TRANSPOSING side -- (1) of the cut, (2) of the paste -- has
// a lane stride of 4 * nDepth + 1 dwords, odd: degree 1 for nDepth 2 .. 8 and every element size.  The COPYING side -- (2) of the cut,
// (1) of the paste -- moves a 16-byte vector as four dwords: 2-way within a 32-lane group for nDepth 2 .. 7, 1 for 8; the paste's
// ds_write_b32 hides that behind its own four cycles, the cut's ds_read_b32 pays it as a second cycle.
//
// Gapped pixels.  The pitch of the layout is pixelPitch.  Cut: (1) the raster's run -- element 0 of the first pixel to the last
// element of the last one, gaps with it -- is copied to LDS as it lies (the copying side above: 2-way, hidden by the write); (2) a
// lane collects V consecutive elements of the staged run, the nDepth elements of each pixel compacted, and stores one aligned vector.
// Lane l's q-th element is element (l * V + q) of the compacted run: a lane stride of 16 * pixelPitch / nDepth bytes of the raster's
// run, no whole number of dwords in general.  tools/lds_conflicts_px.py counts this COMPACTING side too (its second table): at most
// 3-way for every nDepth < pixelPitch <= 8 and element size, and for RGB out of RGBA (4 / 3) 2-way for 1-, 2- and 4-byte elements,
// 3-way for 8-byte ones (laid out as in memory: 6) -- a read side, paid in cycles, on a kernel the gaps make fetch more than it
// stores.  Paste: (1) the staged run is read in vectors and spread to where the raster's run has the elements (the compacting side,
// written); (2) a lane a pixel, its nDepth elements in the widest pieces the address of each admits (pxStoreRun), never an element
// of a gap -- those are neither written nor read.
//
// nDepth or pixelPitch above kRtPxMaxPitch -- a pixel that does not fit the segment buffer -- goes the plain way: a lane an element
// through the three pitches, no LDS.  Same results.  Nothing in front of a row's first element or behind its last is read or written.
// All addresses are 64-bit.  The kernels wait for nobody (__syncthreads only, its loops uniform in a workgroup: the clip is a tile's,
// not a row's), so tools/hipsim runs them as they are.
#include "raster_tiles_dev.h"

#include <algorithm>

namespace lerc {

namespace {

// the part of the chunk's tile kk inside the window, in pixels: rows [i0, i1) and columns [x0, x1) of the tile (empty: the tile misses
// the window), and the raster row / column of the tile's first pixel
struct RtdClip { u32 i0, i1, x0, x1, row0, col0; };

__device__ __forceinline__ RtdClip rtdClip(const RtdChunk& cd, u32 kk)
{
  const RtChunk& ch = cd.ch;
  const u32 k = ch.k0 + kk;
  RtdClip q;
  q.row0 = (ch.ty0 + k / ch.classW) * ch.tileRows; q.col0 = (ch.tx0 + k % ch.classW) * ch.tileCols;    // (inside the raster: no overflow)
  const u32 rowEnd = cd.winRow0 + cd.winRows, colEnd = cd.winCol0 + cd.winCols;
  q.i0 = cd.winRow0 > q.row0 ? cd.winRow0 - q.row0 : 0u;
  q.i1 = rowEnd > q.row0 ? min(ch.r, rowEnd - q.row0) : 0u;
  q.x0 = cd.winCol0 > q.col0 ? cd.winCol0 - q.col0 : 0u;
  q.x1 = colEnd > q.col0 ? min(ch.c, colEnd - q.col0) : 0u;
  if (q.x0 >= q.x1 || q.i0 >= q.i1) q.i0 = q.i1 = q.x0 = q.x1 = 0u;
  return q;
}

// where pixel (row i, column x) of the clipped tile lies in the raster (the window's buffer), depth 0, and in the staging buffer
__device__ __forceinline__ u64 rtdRasterAt(const RtdChunk& cd, const RtdClip& q, u32 i, u32 x)
{
  return (u64)(q.row0 + i - cd.winRow0) * cd.ch.rowPitch + (u64)(q.col0 + x - cd.winCol0) * cd.pixelPitch;
}
__device__ __forceinline__ u64 rtdStageAt(const RtChunk& ch, u32 kk, u32 i, u32 x)
{
  return (((u64)kk * ch.r + i) * ch.c + x) * ch.nBands;
}

// the plain form: a lane an element of the staged run
template<class T, bool CUT>
__device__ __forceinline__ void rtdPlain(const T* __restrict__ from, T* __restrict__ to, const RtdChunk& cd, u32 stripsPerTile, u64 nUnits)
{
  const RtChunk& ch = cd.ch;
  const u32 li = threadIdx.x & 31u, slot = threadIdx.x >> 5, D = ch.nBands;
  for (u64 unit = blockIdx.x; unit < nUnits; unit += gridDim.x)
  {
    const u32 s = (u32)(unit % stripsPerTile), kk = (u32)(unit / stripsPerTile);
    const RtdClip clip = rtdClip(cd, kk);
    const u32 i = s * kRtPxRows + slot;
    if (i < clip.i0 || i >= clip.i1) continue;
    const u64 ra = rtdRasterAt(cd, clip, i, clip.x0), sa = rtdStageAt(ch, kk, i, clip.x0);
    const u64 n = (u64)(clip.x1 - clip.x0) * D;
    for (u64 j = li; j < n; j += 32u)
    {
      const u64 p = j / D, d = j - p * D, r = ra + p * cd.pixelPitch + d * cd.depthPitch;
      if (CUT) to[sa + j] = from[r];
      else to[r] = from[sa + j];
    }
  }
}

// ---- the pieces of a segment; su / sd: the row's LDS slot, e: LDS elements counted from the 16-byte boundary in front of the run

// a run of len elements at g copied to LDS as it lies (mis: g's elements behind a 16-byte boundary): the copying side, written
template<class T>
__device__ __forceinline__ void rtdRunIn(const T* g, u32 len, u32 mis, u32* sd, u32 inv, u32 li)
{
  using U = typename PxLds<T>::U;
  constexpr u32 V = PxLds<T>::V;
  U* su = reinterpret_cast<U*>(sd);
  const u32 head = pxHead<T>(g, len), nVec = (len - head) / V, k0 = (mis + head) / V;
  const uint4* sv = reinterpret_cast<const uint4*>(g + head);
  for (u32 v0 = li; v0 < nVec; v0 += 128u)
  {
    uint4 x[4];
#pragma unroll
    for (u32 q = 0; q < 4u; q++)
    {
      x[q] = make_uint4(0u, 0u, 0u, 0u);
      if (v0 + 32u * q < nVec) x[q] = loadStreaming(sv + v0 + 32u * q);
    }
#pragma unroll
    for (u32 q = 0; q < 4u; q++)
    {
      if (v0 + 32u * q >= nVec) continue;
      const u32 d = pxVecAt<T>(k0 + v0 + 32u * q, inv);
      sd[d] = x[q].x; sd[d + 1] = x[q].y; sd[d + 2] = x[q].z; sd[d + 3] = x[q].w;
    }
  }
  for (u32 e = li; e < head; e += 32u) pxWrite<T>(su, mis + e, inv, g[e]);
  for (u32 e = head + nVec * V + li; e < len; e += 32u) pxWrite<T>(su, mis + e, inv, g[e]);
}

// the reverse: whole vectors from the first aligned address of g on: the copying side, read
template<class T>
__device__ __forceinline__ void rtdRunOut(T* g, u32 len, u32 mis, const u32* sd, u32 inv, u32 li)
{
  using U = typename PxLds<T>::U;
  constexpr u32 V = PxLds<T>::V;
  const U* su = reinterpret_cast<const U*>(sd);
  const u32 head = pxHead<T>(g, len), nVec = (len - head) / V, k0 = (mis + head) / V;
  for (u32 v = li; v < nVec; v += 32u)
  {
    const u32 d = pxVecAt<T>(k0 + v, inv);
    *reinterpret_cast<uint4*>(g + head + v * V) = make_uint4(sd[d], sd[d + 1], sd[d + 2], sd[d + 3]);
  }
  for (u32 e = li; e < head; e += 32u) g[e] = pxRead<T>(su, mis + e, inv);
  for (u32 e = head + nVec * V + li; e < len; e += 32u) g[e] = pxRead<T>(su, mis + e, inv);
}

// a row of np elements at g (one depth of a planes / lines raster) spread to LDS elements e0, e0 + P, ..: the transposing side, written
template<class T>
__device__ __forceinline__ void rtdRowIn(const T* g, u32 np, u32 e0, u32 P, typename PxLds<T>::U* su, u32 inv, u32 li)
{
  constexpr u32 V = PxLds<T>::V;
  const u32 hd = pxHead<T>(g, np), nv = (np - hd) / V;
  const uint4* sv = reinterpret_cast<const uint4*>(g + hd);
  for (u32 v = li; v < nv; v += 32u)
  {
    T t[V];
    pxUnpack<T>(loadStreaming(sv + v), t);
    const u32 e = e0 + (hd + v * V) * P;
#pragma unroll
    for (u32 q = 0; q < V; q++) pxWrite<T>(su, e + q * P, inv, t[q]);
  }
  for (u32 p = li; p < hd; p += 32u) pxWrite<T>(su, e0 + p * P, inv, g[p]);
  for (u32 p = hd + nv * V + li; p < np; p += 32u) pxWrite<T>(su, e0 + p * P, inv, g[p]);
}

// the reverse: V pixels a lane, one aligned vector out: the transposing side, read
template<class T>
__device__ __forceinline__ void rtdRowOut(T* g, u32 np, u32 e0, u32 P, const typename PxLds<T>::U* su, u32 inv, u32 li)
{
  constexpr u32 V = PxLds<T>::V;
  const u32 hd = pxHead<T>(g, np), nv = (np - hd) / V;
  for (u32 v = li; v < nv; v += 32u)
  {
    const u32 e = e0 + (hd + v * V) * P;
    T t[V];
#pragma unroll
    for (u32 q = 0; q < V; q++) t[q] = pxRead<T>(su, e + q * P, inv);
    *reinterpret_cast<uint4*>(g + hd + v * V) = pxPack<T>(t);
  }
  for (u32 p = li; p < hd; p += 32u) g[p] = pxRead<T>(su, e0 + p * P, inv);
  for (u32 p = hd + nv * V + li; p < np; p += 32u) g[p] = pxRead<T>(su, e0 + p * P, inv);
}

// element j of a compacted run (D elements a pixel) in a run of pitch P that begins at LDS element e0; invD = ceil(2^20 / D) is exact
// for j < 2^20 / D, and j < 512 * 8
__device__ __forceinline__ u32 rtdGappedAt(u32 j, u32 e0, u32 D, u32 P, u32 invD)
{
  const u32 p = (j * invD) >> 20;
  return e0 + p * P + (j - p * D);
}

// the compacted run of n = np * D elements at g out of (CUT) / into LDS, whole vectors from the first aligned address of g on: the
// compacting side
template<class T, bool CUT>
__device__ __forceinline__ void rtdCompact(typename std::conditional<CUT, T*, const T*>::type g, u32 n, u32 e0, u32 D, u32 P, typename PxLds<T>::U* su, u32 inv, u32 li)
{
  constexpr u32 V = PxLds<T>::V;
  const u32 invD = ((1u << 20) + D - 1u) / D;
  const u32 hd = pxHead<T>(g, n), nv = (n - hd) / V;
  for (u32 v = li; v < nv; v += 32u)
  {
    const u32 j0 = hd + v * V;
    u32 p = (j0 * invD) >> 20, d = j0 - p * D;
    T t[V];
    if (!CUT) pxUnpack<T>(loadStreaming(reinterpret_cast<const uint4*>(g + j0)), t);
#pragma unroll
    for (u32 q = 0; q < V; q++)
    {
      if (CUT) t[q] = pxRead<T>(su, e0 + p * P + d, inv);
      else pxWrite<T>(su, e0 + p * P + d, inv, t[q]);
      if (++d == D) { d = 0u; p++; }
    }
    if constexpr (CUT) *reinterpret_cast<uint4*>(g + j0) = pxPack<T>(t);
  }
  auto one = [&](u32 j)
  {
    if constexpr (CUT) g[j] = pxRead<T>(su, rtdGappedAt(j, e0, D, P, invD), inv);
    else pxWrite<T>(su, rtdGappedAt(j, e0, D, P, invD), inv, g[j]);
  };
  for (u32 j = li; j < hd; j += 32u) one(j);
  for (u32 j = hd + nv * V + li; j < n; j += 32u) one(j);
}

}    // namespace

template<class T>
__global__ void __launch_bounds__(256) k_rtd_cut(const T* __restrict__ raster, T* __restrict__ stage, RtdChunk cd, u32 stripsPerTile, u64 nUnits)
{
  using U = typename PxLds<T>::U;
  constexpr u32 V = PxLds<T>::V, SP = kRtPxSegBytes / (u32)sizeof(T);
  __shared__ u32 lds[kRtPxRows * kRtPxSlotDwords];
  const RtChunk& ch = cd.ch;
  const u32 D = ch.nBands;
  const bool planes = cd.pixelPitch == 1;
  if (D > kRtPxMaxPitch || cd.pixelPitch > kRtPxMaxPitch) { rtdPlain<T, true>(raster, stage, cd, stripsPerTile, nUnits); return; }

  const u32 P = planes ? D : (u32)cd.pixelPitch, inv = ((1u << 20) + V * P - 1u) / (V * P);    // (the pitch of the run in LDS)
  const u32 li = threadIdx.x & 31u, slot = threadIdx.x >> 5;
  u32* sd = lds + slot * kRtPxSlotDwords;
  U* su = reinterpret_cast<U*>(sd);
  for (u64 unit = blockIdx.x; unit < nUnits; unit += gridDim.x)
  {
    const u32 s = (u32)(unit % stripsPerTile), kk = (u32)(unit / stripsPerTile);
    const RtdClip clip = rtdClip(cd, kk);
    const u32 i = s * kRtPxRows + slot;
    const bool live = i >= clip.i0 && i < clip.i1;
    for (u32 x0 = clip.x0; x0 < clip.x1; x0 += SP)
    {
      const u32 np = min(SP, clip.x1 - x0);
      const T* src = raster + (live ? rtdRasterAt(cd, clip, i, x0) : 0);
      T* dst = stage + (live ? rtdStageAt(ch, kk, i, x0) : 0);
      // (the run in LDS sits as the interleaved side does in memory: the staged run, or the raster's with its gaps)
      const u32 mis = ((u32)(uintptr_t)(planes ? (const T*)dst : src) & 15u) / (u32)sizeof(T);
      if (live)
      {
        if (planes) for (u32 d = 0; d < D; d++) rtdRowIn<T>(src + (u64)d * cd.depthPitch, np, mis + d, D, su, inv, li);
        else rtdRunIn<T>(src, (np - 1u) * P + D, mis, sd, inv, li);
      }
      __syncthreads();
      if (live)
      {
        if (planes) rtdRunOut<T>(dst, np * D, mis, sd, inv, li);
        else rtdCompact<T, true>(dst, np * D, mis, D, P, su, inv, li);
      }
      __syncthreads();    // (the next segment overwrites the buffer)
    }
  }
}

template<class T>
__global__ void __launch_bounds__(256) k_rtd_paste(const T* __restrict__ stage, T* __restrict__ raster, RtdChunk cd, u32 stripsPerTile, u64 nUnits)
{
  using U = typename PxLds<T>::U;
  constexpr u32 V = PxLds<T>::V, SP = kRtPxSegBytes / (u32)sizeof(T);
  __shared__ u32 lds[kRtPxRows * kRtPxSlotDwords];
  const RtChunk& ch = cd.ch;
  const u32 D = ch.nBands;
  const bool planes = cd.pixelPitch == 1;
  if (D > kRtPxMaxPitch || cd.pixelPitch > kRtPxMaxPitch) { rtdPlain<T, false>(stage, raster, cd, stripsPerTile, nUnits); return; }

  const u32 P = planes ? D : (u32)cd.pixelPitch, inv = ((1u << 20) + V * P - 1u) / (V * P);
  const u32 li = threadIdx.x & 31u, slot = threadIdx.x >> 5;
  u32* sd = lds + slot * kRtPxSlotDwords;
  U* su = reinterpret_cast<U*>(sd);
  for (u64 unit = blockIdx.x; unit < nUnits; unit += gridDim.x)
  {
    const u32 s = (u32)(unit % stripsPerTile), kk = (u32)(unit / stripsPerTile);
    const RtdClip clip = rtdClip(cd, kk);
    const u32 i = s * kRtPxRows + slot;
    const bool live = i >= clip.i0 && i < clip.i1;
    for (u32 x0 = clip.x0; x0 < clip.x1; x0 += SP)
    {
      const u32 np = min(SP, clip.x1 - x0);
      const T* src = stage + (live ? rtdStageAt(ch, kk, i, x0) : 0);
      T* dst = raster + (live ? rtdRasterAt(cd, clip, i, x0) : 0);
      const u32 mis = ((u32)(uintptr_t)(planes ? src : dst) & 15u) / (u32)sizeof(T);
      if (live)
      {
        if (planes) rtdRunIn<T>(src, np * D, mis, sd, inv, li);
        else rtdCompact<T, false>(src, np * D, mis, D, P, su, inv, li);
      }
      __syncthreads();
      if (live)
      {
        if (planes) for (u32 d = 0; d < D; d++) rtdRowOut<T>(dst + (u64)d * cd.depthPitch, np, mis + d, D, su, inv, li);
        else for (u32 p = li; p < np; p += 32u) pxStoreRun<T>(dst + (u64)p * P, su, mis + p * P, D, inv);    // (never a gap's element)
      }
      __syncthreads();
    }
  }
}

template<class T>
static void rtdLaunch(bool cut, const void* from, void* to, const RtdChunk& cd, hipStream_t st)
{
  const RtChunk& ch = cd.ch;
  if (ch.n == 0 || ch.r == 0 || ch.c == 0 || ch.nBands == 0 || cd.winRows == 0 || cd.winCols == 0) return;
  const u32 stripsPerTile = (ch.r + kRtPxRows - 1) / kRtPxRows;
  const u64 nUnits = (u64)ch.n * stripsPerTile;
  const dim3 grid((unsigned)std::min<u64>(nUnits, 1u << 16)), block(32 * kRtPxRows);
  if (cut) hipLaunchKernelGGL(k_rtd_cut<T>, grid, block, 0, st, (const T*)from, (T*)to, cd, stripsPerTile, nUnits);
  else hipLaunchKernelGGL(k_rtd_paste<T>, grid, block, 0, st, (const T*)from, (T*)to, cd, stripsPerTile, nUnits);
}

static void rtdLaunchBySize(bool cut, const void* from, void* to, const RtdChunk& cd, u32 elemBytes, hipStream_t st)
{
  if (cd.pixelPitch != 1 && cd.depthPitch != 1) return;    // (one of the two layouts: the host's check)
  switch (elemBytes)    // (as rtLaunchBySize: an instantiation a size)
  {
    case 1: rtdLaunch<u8>(cut, from, to, cd, st); break;
    case 2: rtdLaunch<u16>(cut, from, to, cd, st); break;
    case 4: rtdLaunch<u32>(cut, from, to, cd, st); break;
    case 8: rtdLaunch<u64>(cut, from, to, cd, st); break;
    default: break;
  }
}

void launchRasterCutDepth(const void* dRaster, void* dStage, const RtdChunk& cd, u32 elemBytes, hipStream_t st) { rtdLaunchBySize(true, dRaster, dStage, cd, elemBytes, st); }

void launchRasterPasteDepth(const void* dStage, void* dRaster, const RtdChunk& cd, u32 elemBytes, hipStream_t st) { rtdLaunchBySize(false, dStage, dRaster, cd, elemBytes, st); }

}    // namespace lerc
