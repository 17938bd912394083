// raster_tiles.hip -- the staging pass of the raster tile calls (codec_raster_tiles.cpp): k_rt_cut gathers the rectangles of a chunk
// of tiles, all bands, out of a pitched raster into the layout the tile batches take, [n][nBands][r][c]; k_rt_paste scatters them
// back.  The reference has no counterpart: whoever tiles a raster there copies the rectangles on the host.
//
// A bandwidth kernel and nothing else.  A workgroup takes a strip of kRtStripRows rows (more where rows are short) of one plane of one tile; 8 .. 64 lanes (by the
// row's length) run along a row, the workgroup's other lanes take the rows beside it.  A row is read in 16-byte vectors from the first
// 16-byte aligned SOURCE address on, with a head and a tail by the element; a vector is stored in the widest pieces the DESTINATION's
// address admits (16, 8, 4, 2, 1 bytes, never less than an element) -- a row of a raster that begins an element into its buffer, or a
// staged tile of an edge class, which begins at t * r * c elements, is 16-byte aligned only by luck.  Nothing outside [0, c) of a
// row is read or written.  All addresses are 64-bit: rowPitch * nRows passes 2^32 elements on large rasters.
#include "raster_tiles_dev.h"

#include <algorithm>

namespace lerc {

// where row i of band b of the chunk's tile kk lies in the raster, in elements from its first (in the staging buffer: rtStageAt)
__device__ __forceinline__ u64 rtRasterAt(const RtChunk& ch, u32 kk, u32 b, u32 i)
{
  const u32 k = ch.k0 + kk;
  const u32 ty = ch.ty0 + k / ch.classW, tx = ch.tx0 + k % ch.classW;
  return (u64)b * ch.bandPitch + ((u64)ty * ch.tileRows + i) * ch.rowPitch + (u64)tx * ch.tileCols;
}

// A unit: a strip of stripRows rows of one plane (units beyond the grid are taken in further rounds).  A lane works on four rows at a
// time: the first vector of each is loaded before any is stored, so that a wave has four loads in flight, not one.  What is read is
// read once (the raster on the way in, the staged tiles on the way back): streaming loads, which leave the caches to the tile kernels.
template<class T, bool CUT>
__device__ __forceinline__ void rtMove(const T* __restrict__ from, T* __restrict__ to, const RtChunk& ch, u32 lanesLog2, u32 stripRows, u32 stripsPerPlane, u64 nUnits)
{
  constexpr u32 V = 16u / (u32)sizeof(T);    // elements a vector
  const u32 lanes = 1u << lanesLog2, li = threadIdx.x & (lanes - 1u), rowInPass = threadIdx.x >> lanesLog2, rowsPerPass = blockDim.x >> lanesLog2;
  const u32 n = ch.c;
  for (u64 unit = blockIdx.x; unit < nUnits; unit += gridDim.x)
  {
    const u32 s = (u32)(unit % stripsPerPlane);
    const u64 plane = unit / stripsPerPlane;
    const u32 b = (u32)(plane % ch.nBands), kk = (u32)(plane / ch.nBands);
    const u32 iEnd = min(ch.r, (s + 1u) * stripRows);
    for (u32 i0 = s * stripRows + rowInPass; i0 < iEnd; i0 += 4u * rowsPerPass)
    {
      const T* src[4];
      T* dst[4];
      u32 head[4], nVec[4];
      uint4 x[4];
#pragma unroll
      for (int q = 0; q < 4; q++)
      {
        const u32 i = i0 + (u32)q * rowsPerPass;
        src[q] = from; dst[q] = to; head[q] = 0u; nVec[q] = 0u;
        x[q] = make_uint4(0u, 0u, 0u, 0u);
        if (i >= iEnd) continue;
        const u64 ra = rtRasterAt(ch, kk, b, i), sa = rtStageAt(ch, kk, b, i);
        src[q] = from + (CUT ? ra : sa); dst[q] = to + (CUT ? sa : ra);
        // (16-byte vectors from the first 16-byte aligned source address on; the elements in front of it and behind the last whole vector one by one)
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

template<class T>
__global__ void __launch_bounds__(256) k_rt_cut(const T* __restrict__ raster, T* __restrict__ stage, RtChunk ch, u32 lanesLog2, u32 stripRows, u32 stripsPerPlane, u64 nUnits)
{
  rtMove<T, true>(raster, stage, ch, lanesLog2, stripRows, stripsPerPlane, nUnits);
}

template<class T>
__global__ void __launch_bounds__(256) k_rt_paste(const T* __restrict__ stage, T* __restrict__ raster, RtChunk ch, u32 lanesLog2, u32 stripRows, u32 stripsPerPlane, u64 nUnits)
{
  rtMove<T, false>(stage, raster, ch, lanesLog2, stripRows, stripsPerPlane, nUnits);
}

template<class T>
static void rtLaunch(bool cut, const void* from, void* to, const RtChunk& ch, hipStream_t st)
{
  if (ch.n == 0 || ch.r == 0 || ch.c == 0 || ch.nBands == 0) return;
  const u32 lanesLog2 = rtLanesPerRowLog2(ch.c, (u32)sizeof(T));
  const u32 stripRows = std::max(kRtStripRows, 256u >> lanesLog2);    // (short rows: every lane of the workgroup has a row)
  const u32 stripsPerPlane = (ch.r + stripRows - 1) / stripRows;
  const u64 nUnits = (u64)ch.n * ch.nBands * stripsPerPlane;
  const dim3 grid((unsigned)std::min<u64>(nUnits, 1u << 16)), block(256);
  if (cut) hipLaunchKernelGGL(k_rt_cut<T>, grid, block, 0, st, (const T*)from, (T*)to, ch, lanesLog2, stripRows, stripsPerPlane, nUnits);
  else hipLaunchKernelGGL(k_rt_paste<T>, grid, block, 0, st, (const T*)from, (T*)to, ch, lanesLog2, stripRows, stripsPerPlane, nUnits);
}

static void rtLaunchBySize(bool cut, const void* from, void* to, const RtChunk& ch, u32 elemBytes, hipStream_t st)
{
  switch (elemBytes)    // (the copy does not care about signedness or float: an instantiation a size)
  {
    case 1: rtLaunch<u8>(cut, from, to, ch, st); break;
    case 2: rtLaunch<u16>(cut, from, to, ch, st); break;
    case 4: rtLaunch<u32>(cut, from, to, ch, st); break;
    case 8: rtLaunch<u64>(cut, from, to, ch, st); break;
    default: break;
  }
}

void launchRasterCut(const void* dRaster, void* dStage, const RtChunk& ch, u32 elemBytes, hipStream_t st) { rtLaunchBySize(true, dRaster, dStage, ch, elemBytes, st); }

void launchRasterPaste(const void* dStage, void* dRaster, const RtChunk& ch, u32 elemBytes, hipStream_t st) { rtLaunchBySize(false, dStage, dRaster, ch, elemBytes, st); }

}    // namespace lerc
