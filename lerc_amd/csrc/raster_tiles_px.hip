// raster_tiles_px.hip -- the staging pass of the raster tile calls for PIXEL-INTERLEAVED rasters (codec_raster_tiles.cpp): element
// (band b, row i, column j) lies at b + i * rowPitch + j * pixelPitch, pixelPitch >= 2 elements, nBands <= pixelPitch.  k_rt_cut_px
// gathers the rectangles of a chunk of tiles into the layout the tile batches take, planes [n][nBands][r][c]; k_rt_paste_px scatters
// them back.  The mask is a plane and goes through k_rt_cut / k_rt_paste (raster_tiles.hip), which this file leaves alone.
//
// A bandwidth kernel with a transposition in the middle.  A unit is a strip of kRtPxRows rows of one tile with ALL its bands, so the
// interleaved rows are read (written) once.  A half-wave of 32 lanes has a row; a row goes in segments of kRtPxSegBytes / sizeof(T)
// pixels, so the LDS a workgroup takes (kRtPxRows * kRtPxSlotDwords * 4 = 37376 bytes) does not depend on the tile's width.
//
// Cut: (1) the segment's run -- from band 0 of its first pixel to the last band of its last one, the gaps between the pixels with it --
// is copied to LDS as it lies: 16-byte vectors from the first 16-byte aligned source address on, head and tail by the element; the run
// sits in LDS as far behind a 16-byte boundary as it does in memory.  (2) Per band a lane collects 16 / sizeof(T) consecutive pixels
// from LDS, one element a read with the register index fixed by unrolling, and stores them as ONE 16-byte vector at a 16-byte
// aligned address of the staged row; the pixels in front of the first such address and behind the last whole vector go by the element.
// Paste is the mirror image: staged rows in 16-byte vectors from their first aligned address on are spread into LDS, and the run is
// written back.  Dense (pixelPitch == nBands): the whole run in 16-byte vectors from the first aligned raster address on.  Gapped
// (pixelPitch > nBands): a lane a pixel, its nBands elements in the widest pieces (16, 8, 4, 2, 1 bytes, never less than an element)
// the address of each piece admits, never an element of a gap -- those are neither written nor read back.
//
// The LDS layout.  In (2) lane l of a row reads the elements of pixels l * V .. l * V + V - 1 (V = 16 / sizeof(T)): 16 * pixelPitch bytes
// from lane to lane, a multiple of 16 bytes, which laid out as in memory puts the 32 lanes of a ds_read_b32 / _u16 / _u8 group onto
// 8 / gcd(pixelPitch, 8) banks: 8-way for pixelPitch 2, 4-way (in practice: 32 lanes on 8 banks) for 3, 16-way for 4.  So the run is
// stored with ONE PADDING DWORD after every 16 * pixelPitch bytes: byte a of the run (counted from the 16-byte boundary in front of
// it) lies at a + 4 * floor(a / (16 * pixelPitch)).  The lane stride becomes 4 * pixelPitch + 1 dwords, odd, and the 32 lanes of a
// group fall on 32 different banks for every pixelPitch: conflict degree 1 for P = 2, 3 and 4 (and 5 .. 8) on the transposing side,
// for every element size (a 64-bit element is two dwords, read one after the other).  The price is on the copying side: a 16-byte
// vector of the run no longer lies 16-byte aligned in LDS, so it is moved as four dwords, lane l's at dword 4 l + floor(l / P) + j:
// 2-way within a 32-lane group for P = 2 .. 7, 1 for P = 8 -- which a ds_write_b32 hides behind its own four cycles (the cut) and a
// ds_read_b32 pays as a second cycle (the dense paste).  tools/lds_conflicts_px.py counts both sides from the address arithmetic.
//
// A pixelPitch above kRtPxMaxPitch -- a pixel that does not fit the segment buffer -- goes the plain way: a lane an element, strided,
// no LDS.  Same results, and such rasters have more gap than data in every line they fetch anyway.
// Nothing in front of band 0 of a row's first pixel or behind the last band of its last pixel is read or written.  All addresses are
// 64-bit.  The kernels wait for nobody (__syncthreads only), so tools/hipsim runs them as they are.
#include "raster_tiles_dev.h"

#include <algorithm>

namespace lerc {

namespace {

// (the LDS layout's pieces -- PxLds, pxRead / pxWrite, pxVecAt, pxPack / pxUnpack, pxHead, pxStoreRun --: raster_tiles_dev.h)
// where row i of the chunk's tile kk begins (band 0 of its first pixel), and a staged row of band b
__device__ __forceinline__ u64 pxRasterAt(const RtChunkPx& cx, u32 kk, u32 i)
{
  const RtChunk& ch = cx.ch;
  const u32 k = ch.k0 + kk;
  const u32 ty = ch.ty0 + k / ch.classW, tx = ch.tx0 + k % ch.classW;
  return ((u64)ty * ch.tileRows + i) * ch.rowPitch + (u64)tx * ch.tileCols * cx.pixelPitch;
}
__device__ __forceinline__ u64 pxStageAt(const RtChunk& ch, u32 kk, u32 b, u32 i)
{
  return (((u64)kk * ch.nBands + b) * ch.r + i) * ch.c;
}

// the plain form: a lane an element
template<class T, bool CUT>
__device__ __forceinline__ void pxPlain(const T* __restrict__ from, T* __restrict__ to, const RtChunkPx& cx, u32 stripsPerTile, u64 nUnits)
{
  const RtChunk& ch = cx.ch;
  const u32 li = threadIdx.x & 31u, slot = threadIdx.x >> 5;
  for (u64 unit = blockIdx.x; unit < nUnits; unit += gridDim.x)
  {
    const u32 s = (u32)(unit % stripsPerTile), kk = (u32)(unit / stripsPerTile);
    const u32 i = s * kRtPxRows + slot;
    if (i >= ch.r) continue;
    const u64 ra = pxRasterAt(cx, kk, i);
    for (u32 b = 0; b < ch.nBands; b++)
    {
      const u64 sa = pxStageAt(ch, kk, b, i);
      for (u32 x = li; x < ch.c; x += 32u)
      {
        if (CUT) to[sa + x] = from[ra + (u64)x * cx.pixelPitch + b];
        else to[ra + (u64)x * cx.pixelPitch + b] = from[sa + x];
      }
    }
  }
}

}    // namespace

template<class T>
__global__ void __launch_bounds__(256) k_rt_cut_px(const T* __restrict__ raster, T* __restrict__ stage, RtChunkPx cx, u32 stripsPerTile, u64 nUnits)
{
  using U = typename PxLds<T>::U;
  constexpr u32 V = PxLds<T>::V, SP = kRtPxSegBytes / (u32)sizeof(T);
  __shared__ u32 lds[kRtPxRows * kRtPxSlotDwords];
  if (cx.pixelPitch > kRtPxMaxPitch) { pxPlain<T, true>(raster, stage, cx, stripsPerTile, nUnits); return; }

  const RtChunk& ch = cx.ch;
  const u32 P = (u32)cx.pixelPitch, nB = ch.nBands, inv = ((1u << 20) + V * P - 1u) / (V * P);
  const u32 li = threadIdx.x & 31u, slot = threadIdx.x >> 5;
  u32* sd = lds + slot * kRtPxSlotDwords;
  U* su = reinterpret_cast<U*>(sd);
  for (u64 unit = blockIdx.x; unit < nUnits; unit += gridDim.x)
  {
    const u32 s = (u32)(unit % stripsPerTile), kk = (u32)(unit / stripsPerTile);
    const u32 i = s * kRtPxRows + slot;
    const bool live = i < ch.r;
    const u64 ra = live ? pxRasterAt(cx, kk, i) : 0;
    for (u32 x0 = 0; x0 < ch.c; x0 += SP)
    {
      const u32 np = min(SP, ch.c - x0);
      u32 mis = 0;
      if (live)
      {
        // (1) the run, as it lies
        const T* src = raster + ra + (u64)x0 * P;
        const u32 len = (np - 1u) * P + nB;
        mis = ((u32)(uintptr_t)src & 15u) / (u32)sizeof(T);
        const u32 head = pxHead<T>(src, len), nVec = (len - head) / V, k0 = (mis + head) / V;
        const uint4* sv = reinterpret_cast<const uint4*>(src + head);
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
        for (u32 e = li; e < head; e += 32u) pxWrite<T>(su, mis + e, inv, src[e]);
        for (u32 e = head + nVec * V + li; e < len; e += 32u) pxWrite<T>(su, mis + e, inv, src[e]);
      }
      __syncthreads();
      if (live)
      {
        // (2) a band at a time: V pixels a lane, one aligned vector out
        for (u32 b = 0; b < nB; b++)
        {
          T* d = stage + pxStageAt(ch, kk, b, i) + x0;
          const u32 hd = pxHead<T>(d, np), nv = (np - hd) / V;
          for (u32 v = li; v < nv; v += 32u)
          {
            const u32 e0 = mis + (hd + v * V) * P + b;
            T t[V];
#pragma unroll
            for (u32 q = 0; q < V; q++) t[q] = pxRead<T>(su, e0 + q * P, inv);
            *reinterpret_cast<uint4*>(d + hd + v * V) = pxPack<T>(t);
          }
          for (u32 p = li; p < hd; p += 32u) d[p] = pxRead<T>(su, mis + p * P + b, inv);
          for (u32 p = hd + nv * V + li; p < np; p += 32u) d[p] = pxRead<T>(su, mis + p * P + b, inv);
        }
      }
      __syncthreads();    // (the next segment overwrites the buffer)
    }
  }
}

template<class T>
__global__ void __launch_bounds__(256) k_rt_paste_px(const T* __restrict__ stage, T* __restrict__ raster, RtChunkPx cx, u32 stripsPerTile, u64 nUnits)
{
  using U = typename PxLds<T>::U;
  constexpr u32 V = PxLds<T>::V, SP = kRtPxSegBytes / (u32)sizeof(T);
  __shared__ u32 lds[kRtPxRows * kRtPxSlotDwords];
  if (cx.pixelPitch > kRtPxMaxPitch) { pxPlain<T, false>(stage, raster, cx, stripsPerTile, nUnits); return; }

  const RtChunk& ch = cx.ch;
  const u32 P = (u32)cx.pixelPitch, nB = ch.nBands, inv = ((1u << 20) + V * P - 1u) / (V * P);
  const u32 li = threadIdx.x & 31u, slot = threadIdx.x >> 5;
  u32* sd = lds + slot * kRtPxSlotDwords;
  U* su = reinterpret_cast<U*>(sd);
  for (u64 unit = blockIdx.x; unit < nUnits; unit += gridDim.x)
  {
    const u32 s = (u32)(unit % stripsPerTile), kk = (u32)(unit / stripsPerTile);
    const u32 i = s * kRtPxRows + slot;
    const bool live = i < ch.r;
    const u64 ra = live ? pxRasterAt(cx, kk, i) : 0;
    for (u32 x0 = 0; x0 < ch.c; x0 += SP)
    {
      const u32 np = min(SP, ch.c - x0);
      T* dst = raster + ra + (u64)x0 * P;
      const u32 mis = ((u32)(uintptr_t)dst & 15u) / (u32)sizeof(T);
      if (live)
      {
        // (1) the staged rows, a band at a time, spread to where the run has them
        for (u32 b = 0; b < nB; b++)
        {
          const T* sp = stage + pxStageAt(ch, kk, b, i) + x0;
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
      __syncthreads();
    }
  }
}

template<class T>
static void pxLaunch(bool cut, const void* from, void* to, const RtChunkPx& cx, hipStream_t st)
{
  const RtChunk& ch = cx.ch;
  if (ch.n == 0 || ch.r == 0 || ch.c == 0 || ch.nBands == 0) return;
  const u32 stripsPerTile = (ch.r + kRtPxRows - 1) / kRtPxRows;
  const u64 nUnits = (u64)ch.n * stripsPerTile;
  const dim3 grid((unsigned)std::min<u64>(nUnits, 1u << 16)), block(32 * kRtPxRows);
  if (cut) hipLaunchKernelGGL(k_rt_cut_px<T>, grid, block, 0, st, (const T*)from, (T*)to, cx, stripsPerTile, nUnits);
  else hipLaunchKernelGGL(k_rt_paste_px<T>, grid, block, 0, st, (const T*)from, (T*)to, cx, stripsPerTile, nUnits);
}

static void pxLaunchBySize(bool cut, const void* from, void* to, const RtChunkPx& cx, u32 elemBytes, hipStream_t st)
{
  switch (elemBytes)    // (as rtLaunchBySize: an instantiation a size)
  {
    case 1: pxLaunch<u8>(cut, from, to, cx, st); break;
    case 2: pxLaunch<u16>(cut, from, to, cx, st); break;
    case 4: pxLaunch<u32>(cut, from, to, cx, st); break;
    case 8: pxLaunch<u64>(cut, from, to, cx, st); break;
    default: break;
  }
}

void launchRasterCutPx(const void* dRaster, void* dStage, const RtChunkPx& cx, u32 elemBytes, hipStream_t st) { pxLaunchBySize(true, dRaster, dStage, cx, elemBytes, st); }

void launchRasterPastePx(const void* dStage, void* dRaster, const RtChunkPx& cx, u32 elemBytes, hipStream_t st) { pxLaunchBySize(false, dStage, dRaster, cx, elemBytes, st); }

}    // namespace lerc
