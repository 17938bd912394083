// raster_window.hip -- the clipped paste of the window decode (lerc_amd_decode_raster_window_device, codec_raster_tiles.cpp): the tiles
// a window of a mosaic touches are decoded into the staging buffer as [n][nBands][r][c], and of every staged tile the rows and columns
// that fall inside the window go to the caller's buffer, which holds the window and nothing else.  k_rw_paste writes planes (band-
// sequential, line-interleaved, the mask), k_rw_paste_px a pixel-interleaved buffer.  The reference has no counterpart: a tiled-LERC
// reader there decodes whole tiles on the host and copies the parts it wants.
//
// What clipping changes against k_rt_paste / k_rt_paste_px is where a row begins and ends, per tile: a staged row is read from the
// tile's first column inside the window on (clip.x0 elements in), and lands wherever the window puts it, so the two alignments are
// arbitrary, differ from tile to tile and are taken from the addresses, as in those kernels: 16-byte streaming loads from the first
// aligned SOURCE address on, stores in the widest pieces the DESTINATION address admits (planes) or through the padded LDS layout of
// raster_tiles_px.hip (pixels: dense runs out as whole vectors, gapped pixels in pieces, never an element of a gap; a pixelPitch above
// kRtPxMaxPitch a lane an element), heads and tails by the element.  Units are those of the unclipped kernels -- a strip of rows of one
// plane, a strip of kRtPxRows rows of one tile -- and a unit whose rows miss the window does nothing.  Nothing outside the window's
// elements is written, nothing of the window buffer is read.  All addresses are 64-bit.  The kernels wait for nobody
// (__syncthreads only, its loops uniform in a workgroup: the clip is a tile's, not a row's), so tools/hipsim runs them as they are.
#include "raster_tiles_dev.h"

#include <algorithm>

namespace lerc {

namespace {

// the part of the chunk's tile kk inside the window: rows [i0, i1) and columns [x0, x1) of the tile (empty: the tile misses the
// window), and the raster row / column of the tile's first pixel
struct RwClip { u32 i0, i1, x0, x1, row0, col0; };

__device__ __forceinline__ RwClip rwClip(const RwChunk& cw, u32 kk)
{
  const RtChunk& ch = cw.ch;
  const u32 k = ch.k0 + kk;
  RwClip q;
  q.row0 = (ch.ty0 + k / ch.classW) * ch.tileRows; q.col0 = (ch.tx0 + k % ch.classW) * ch.tileCols;
  const u32 rowEnd = cw.winRow0 + cw.winRows, colEnd = cw.winCol0 + cw.winCols;    // (inside the raster: no overflow)
  q.i0 = cw.winRow0 > q.row0 ? cw.winRow0 - q.row0 : 0u;
  q.i1 = rowEnd > q.row0 ? min(ch.r, rowEnd - q.row0) : 0u;
  q.x0 = cw.winCol0 > q.col0 ? cw.winCol0 - q.col0 : 0u;
  q.x1 = colEnd > q.col0 ? min(ch.c, colEnd - q.col0) : 0u;
  if (q.x0 >= q.x1 || q.i0 >= q.i1) q.i0 = q.i1 = q.x0 = q.x1 = 0u;
  return q;
}

// where row i (i0 <= i < i1) of the tile lands in the window buffer, at the tile's first column inside the window, band 0: elements
__device__ __forceinline__ u64 rwWindowAt(const RwChunk& cw, const RwClip& q, u32 i)
{
  return (u64)(q.row0 + i - cw.winRow0) * cw.ch.rowPitch + (u64)(q.col0 + q.x0 - cw.winCol0) * cw.pixelPitch;
}

}    // namespace

// rtMove (raster_tiles.hip) with a clip: four rows' first vectors are loaded before any is stored.
template<class T>
__global__ void __launch_bounds__(256) k_rw_paste(const T* __restrict__ stage, T* __restrict__ window, RwChunk cw, u32 lanesLog2, u32 stripRows, u32 stripsPerPlane, u64 nUnits)
{
  constexpr u32 V = 16u / (u32)sizeof(T);    // elements a vector
  const RtChunk& ch = cw.ch;
  const u32 lanes = 1u << lanesLog2, li = threadIdx.x & (lanes - 1u), rowInPass = threadIdx.x >> lanesLog2, rowsPerPass = blockDim.x >> lanesLog2;
  for (u64 unit = blockIdx.x; unit < nUnits; unit += gridDim.x)
  {
    const u32 s = (u32)(unit % stripsPerPlane);
    const u64 plane = unit / stripsPerPlane;
    const u32 b = (u32)(plane % ch.nBands), kk = (u32)(plane / ch.nBands);
    const RwClip clip = rwClip(cw, kk);
    const u32 n = clip.x1 - clip.x0;
    const u32 iBegin = max(clip.i0, s * stripRows), iEnd = min(clip.i1, (s + 1u) * stripRows);
    for (u32 i0 = iBegin + rowInPass; i0 < iEnd; i0 += 4u * rowsPerPass)
    {
      const T* src[4];
      T* dst[4];
      u32 head[4], nVec[4];
      uint4 x[4];
#pragma unroll
      for (int q = 0; q < 4; q++)
      {
        const u32 i = i0 + (u32)q * rowsPerPass;
        src[q] = stage; dst[q] = window; head[q] = 0u; nVec[q] = 0u;
        x[q] = make_uint4(0u, 0u, 0u, 0u);
        if (i >= iEnd) continue;
        src[q] = stage + rtStageAt(ch, kk, b, i) + clip.x0;
        dst[q] = window + (u64)b * ch.bandPitch + rwWindowAt(cw, clip, i);
        const u32 mis = ((u32)(uintptr_t)src[q] & 15u) / (u32)sizeof(T);
        head[q] = min(n, (V - mis) & (V - 1u));
        nVec[q] = (n - head[q]) / V;
        if (li < nVec[q]) x[q] = loadStreaming(reinterpret_cast<const uint4*>(src[q] + head[q]) + li);
      }
#pragma unroll
      for (int q = 0; q < 4; q++)
      {
        if (i0 + (u32)q * rowsPerPass >= iEnd) continue;
        const uint4* sv = reinterpret_cast<const uint4*>(src[q] + head[q]);
        T* d = dst[q] + head[q];
        const u32 dstAlign = (u32)(uintptr_t)d & 15u;
        if (li < nVec[q]) rtStore16<T>(d + (size_t)li * V, x[q], dstAlign);
        for (u32 v = li + lanes; v < nVec[q]; v += lanes) rtStore16<T>(d + (size_t)v * V, loadStreaming(sv + v), dstAlign);    // (rows of more than 64 vectors)
        for (u32 e = li; e < head[q]; e += lanes) dst[q][e] = src[q][e];
        for (u32 e = head[q] + nVec[q] * V + li; e < n; e += lanes) dst[q][e] = src[q][e];
      }
    }
  }
}

// k_rt_paste_px (raster_tiles_px.hip) with a clip: a half-wave a row, a row in segments of kRtPxSegBytes / sizeof(T) pixels from the
// tile's first column inside the window on.
template<class T>
__global__ void __launch_bounds__(256) k_rw_paste_px(const T* __restrict__ stage, T* __restrict__ window, RwChunk cw, u32 stripsPerTile, u64 nUnits)
{
  using U = typename PxLds<T>::U;
  constexpr u32 V = PxLds<T>::V, SP = kRtPxSegBytes / (u32)sizeof(T);
  __shared__ u32 lds[kRtPxRows * kRtPxSlotDwords];
  const RtChunk& ch = cw.ch;
  const u32 li = threadIdx.x & 31u, slot = threadIdx.x >> 5, nB = ch.nBands;
  if (cw.pixelPitch > kRtPxMaxPitch)
  {
    // the plain form: a lane an element
    for (u64 unit = blockIdx.x; unit < nUnits; unit += gridDim.x)
    {
      const u32 s = (u32)(unit % stripsPerTile), kk = (u32)(unit / stripsPerTile);
      const RwClip clip = rwClip(cw, kk);
      const u32 i = s * kRtPxRows + slot;
      if (i < clip.i0 || i >= clip.i1) continue;
      T* dst = window + rwWindowAt(cw, clip, i);
      for (u32 b = 0; b < nB; b++)
      {
        const T* sp = stage + rtStageAt(ch, kk, b, i) + clip.x0;
        for (u32 x = li; x < clip.x1 - clip.x0; x += 32u) dst[(u64)x * cw.pixelPitch + b] = sp[x];
      }
    }
    return;
  }

  const u32 P = (u32)cw.pixelPitch, inv = ((1u << 20) + V * P - 1u) / (V * P);
  u32* sd = lds + slot * kRtPxSlotDwords;
  U* su = reinterpret_cast<U*>(sd);
  for (u64 unit = blockIdx.x; unit < nUnits; unit += gridDim.x)
  {
    const u32 s = (u32)(unit % stripsPerTile), kk = (u32)(unit / stripsPerTile);
    const RwClip clip = rwClip(cw, kk);
    const u32 i = s * kRtPxRows + slot;
    const bool live = i >= clip.i0 && i < clip.i1;
    const u64 wa = live ? rwWindowAt(cw, clip, i) : 0;
    for (u32 x0 = clip.x0; x0 < clip.x1; x0 += SP)
    {
      const u32 np = min(SP, clip.x1 - x0);
      T* dst = window + wa + (u64)(x0 - clip.x0) * P;
      const u32 mis = ((u32)(uintptr_t)dst & 15u) / (u32)sizeof(T);
      if (live)
      {
        // (1) the staged rows, a band at a time, spread to where the run has them
        for (u32 b = 0; b < nB; b++)
        {
          const T* sp = stage + rtStageAt(ch, kk, b, i) + x0;
          const u32 hd = pxHead<T>(sp, np), nv = (np - hd) / V;
          const uint4* sv = reinterpret_cast<const uint4*>(sp + hd);
          for (u32 v = li; v < nv; v += 32u)
          {
            T t[V];
            pxUnpack<T>(loadStreaming(sv + v), t);
            const u32 e0 = mis + (hd + v * V) * P + b;
#pragma unroll
            for (u32 q = 0; q < V; q++) pxWrite<T>(su, e0 + q * P, inv, t[q]);
          }
          for (u32 p = li; p < hd; p += 32u) pxWrite<T>(su, mis + p * P + b, inv, sp[p]);
          for (u32 p = hd + nv * V + li; p < np; p += 32u) pxWrite<T>(su, mis + p * P + b, inv, sp[p]);
        }
      }
      __syncthreads();
      if (live)
      {
        if (P == nB)
        {
          // (2) dense: the run as it lies, whole vectors
          const u32 len = np * P;
          const u32 head = pxHead<T>(dst, len), nVec = (len - head) / V, k0 = (mis + head) / V;
          for (u32 v = li; v < nVec; v += 32u)
          {
            const u32 d = pxVecAt<T>(k0 + v, inv);
            *reinterpret_cast<uint4*>(dst + head + v * V) = make_uint4(sd[d], sd[d + 1], sd[d + 2], sd[d + 3]);
          }
          for (u32 e = li; e < head; e += 32u) dst[e] = pxRead<T>(su, mis + e, inv);
          for (u32 e = head + nVec * V + li; e < len; e += 32u) dst[e] = pxRead<T>(su, mis + e, inv);
        }
        else
        {
          // (2) gapped: a lane a pixel, never a gap's element
          for (u32 p = li; p < np; p += 32u) pxStoreRun<T>(dst + (u64)p * P, su, mis + p * P, nB, inv);
        }
      }
      __syncthreads();    // (the next segment overwrites the buffer)
    }
  }
}

template<class T>
static void rwLaunch(const void* from, void* to, const RwChunk& cw, hipStream_t st)
{
  const RtChunk& ch = cw.ch;
  if (ch.n == 0 || ch.r == 0 || ch.c == 0 || ch.nBands == 0 || cw.winRows == 0 || cw.winCols == 0) return;
  if (cw.pixelPitch == 1)
  {
    const u32 lanesLog2 = rtLanesPerRowLog2(ch.c, (u32)sizeof(T));
    const u32 stripRows = std::max(kRtStripRows, 256u >> lanesLog2);    // (short rows: every lane of the workgroup has a row)
    const u32 stripsPerPlane = (ch.r + stripRows - 1) / stripRows;
    const u64 nUnits = (u64)ch.n * ch.nBands * stripsPerPlane;
    const dim3 grid((unsigned)std::min<u64>(nUnits, 1u << 16)), block(256);
    hipLaunchKernelGGL(k_rw_paste<T>, grid, block, 0, st, (const T*)from, (T*)to, cw, lanesLog2, stripRows, stripsPerPlane, nUnits);
  }
  else
  {
    const u32 stripsPerTile = (ch.r + kRtPxRows - 1) / kRtPxRows;
    const u64 nUnits = (u64)ch.n * stripsPerTile;
    const dim3 grid((unsigned)std::min<u64>(nUnits, 1u << 16)), block(32 * kRtPxRows);
    hipLaunchKernelGGL(k_rw_paste_px<T>, grid, block, 0, st, (const T*)from, (T*)to, cw, stripsPerTile, nUnits);
  }
}

static void rwLaunchBySize(const void* from, void* to, const RwChunk& cw, u32 elemBytes, hipStream_t st)
{
  switch (elemBytes)    // (as rtLaunchBySize: an instantiation a size)
  {
    case 1: rwLaunch<u8>(from, to, cw, st); break;
    case 2: rwLaunch<u16>(from, to, cw, st); break;
    case 4: rwLaunch<u32>(from, to, cw, st); break;
    case 8: rwLaunch<u64>(from, to, cw, st); break;
    default: break;
  }
}

void launchWindowPaste(const void* dStage, void* dWindow, const RwChunk& cw, u32 elemBytes, hipStream_t st)
{
  if (cw.pixelPitch == 1) rwLaunchBySize(dStage, dWindow, cw, elemBytes, st);
}

void launchWindowPastePx(const void* dStage, void* dWindow, const RwChunk& cw, u32 elemBytes, hipStream_t st)
{
  if (cw.pixelPitch >= 2) rwLaunchBySize(dStage, dWindow, cw, elemBytes, st);
}

}    // namespace lerc
