// raster_nodata.hip -- the staging pass of the noData raster calls (include/lerc_amd_nodata.h, codec_raster_tiles.cpp): a raster that
// says "no data" with a VALUE is cut into the tile batches' layout and pasted back, and the byte mask the masked tile batches want
// is made on the way.  It never exists as a raster-sized buffer: k_rtn_cut stores, beside every staged element, its valid byte
// (staged mask [n][r][c], 1 = the element is not the noData value); k_rtn_paste writes select(valid byte, staged element, noData)
// and, where the caller asked for them, the window's valid bytes.  The reference has no counterpart: a tiled-LERC writer compares the
// raster with its noData value on the host, in a pass of its own, before lerc_encode, and writes the value back after lerc_decode.
//
// Units, lanes and alignment are k_rt_cut's and k_rw_paste's (raster_tiles.hip, raster_window.hip): a strip of kRtStripRows rows (more
// where rows are short) of one tile a workgroup round, 8 .. 64 lanes along a row, four rows' first vectors loaded before any is stored;
// 16-byte streaming loads from the first 16-byte aligned SOURCE address on, stores in the widest pieces the DESTINATION's address admits
// -- the data's by rtStore16, the 16 / sizeof(T) valid bytes of a vector by rtnStoreValid --, heads and tails by the element.  A
// pixelPitch >= 2 (one channel of an interleaved image) goes the plain way in the same units, a lane an element; the results are the
// same.  One band always (ch.nBands 1, ch.bandPitch unused).
//
// The compare (rtnInvalid): the raw pattern for integers, so one instantiation serves both signs; for float and double `==` on the
// values (-0.0 matches 0.0, an infinity matches itself, a NaN matches nothing) or, where the call's noData is NaN, `v != v`.
// Nothing outside [0, c) of a row (of the window's part of it) is read or written, nothing of the window buffer is read.  All
// addresses are 64-bit.  No workgroup waits for another and there is no barrier at all, so tools/hipsim runs the kernels as they are.
#include "raster_tiles_dev.h"

#include <algorithm>
#include <cstring>

namespace lerc {

namespace {

// the unsigned type that holds T's pattern
template<class T> struct RtnRaw { using U = T; };
template<> struct RtnRaw<float> { using U = u32; };
template<> struct RtnRaw<double> { using U = u64; };

template<class T>
__device__ __forceinline__ bool rtnInvalid(typename RtnRaw<T>::U bits, typename RtnRaw<T>::U nd, bool ndIsNaN)
{
  if constexpr (std::is_floating_point<T>::value)
  {
    T v, w;
    memcpy(&v, &bits, sizeof(T)); memcpy(&w, &nd, sizeof(T));
    return ndIsNaN ? v != v : v == w;
  }
  else return bits == nd;
}

// V valid bytes (V = 16, 8, 4, 2: those of one 16-byte vector of elements), the first in lo's lowest byte, in the widest pieces p admits
template<u32 V>
__device__ __forceinline__ void rtnStoreValid(u8* p, u64 lo, u64 hi)
{
  const u32 a = (u32)(uintptr_t)p;
  if constexpr (V == 16)
  {
    rtStore16<u8>(p, make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32)), a & 15u);
    return;
  }
  else
  {
    if constexpr (V == 8)
      if ((a & 7u) == 0u) { *reinterpret_cast<u64*>(p) = lo; return; }
    if constexpr (V >= 4)
      if ((a & 3u) == 0u)
      {
#pragma unroll
        for (u32 q = 0; q < V / 4u; q++) reinterpret_cast<u32*>(p)[q] = (u32)(lo >> (32u * q));
        return;
      }
    if ((a & 1u) == 0u)
    {
#pragma unroll
      for (u32 q = 0; q < V / 2u; q++) reinterpret_cast<u16*>(p)[q] = (u16)(lo >> (16u * q));
      return;
    }
#pragma unroll
    for (u32 q = 0; q < V; q++) p[q] = (u8)(lo >> (8u * q));
  }
}

// the V valid bytes at p, as rtnStoreValid packs them (lo; hi for V == 16): one load where p admits it
template<u32 V>
__device__ __forceinline__ void rtnLoadValid(const u8* p, u64& lo, u64& hi)
{
  const u32 a = (u32)(uintptr_t)p;
  lo = 0; hi = 0;
  if constexpr (V == 16)
  {
    if ((a & 15u) == 0u)
    {
      const uint4 x = *reinterpret_cast<const uint4*>(p);
      lo = (u64)x.x | ((u64)x.y << 32); hi = (u64)x.z | ((u64)x.w << 32);
      return;
    }
#pragma unroll
    for (u32 q = 0; q < 8u; q++) { lo |= (u64)p[q] << (8u * q); hi |= (u64)p[8u + q] << (8u * q); }
  }
  else
  {
    if constexpr (V == 8)
      if ((a & 7u) == 0u) { lo = *reinterpret_cast<const u64*>(p); return; }
    if constexpr (V == 4)
      if ((a & 3u) == 0u) { lo = *reinterpret_cast<const u32*>(p); return; }
    if constexpr (V == 2)
      if ((a & 1u) == 0u) { lo = *reinterpret_cast<const u16*>(p); return; }
#pragma unroll
    for (u32 q = 0; q < V; q++) lo |= (u64)p[q] << (8u * q);
  }
}

// where row i of the chunk's tile kk begins in the raster (one band): elements
__device__ __forceinline__ u64 rtnRasterAt(const RtChunk& ch, u64 pixelPitch, u32 kk, u32 i)
{
  const u32 k = ch.k0 + kk;
  const u32 ty = ch.ty0 + k / ch.classW, tx = ch.tx0 + k % ch.classW;
  return ((u64)ty * ch.tileRows + i) * ch.rowPitch + (u64)tx * ch.tileCols * pixelPitch;
}

// the part of the chunk's tile kk inside the window (rwClip of raster_window.hip)
struct RtnClip { u32 i0, i1, x0, x1, row0, col0; };

__device__ __forceinline__ RtnClip rtnClip(const RwChunk& cw, u32 kk)
{
  const RtChunk& ch = cw.ch;
  const u32 k = ch.k0 + kk;
  RtnClip q;
  q.row0 = (ch.ty0 + k / ch.classW) * ch.tileRows; q.col0 = (ch.tx0 + k % ch.classW) * ch.tileCols;
  const u32 rowEnd = cw.winRow0 + cw.winRows, colEnd = cw.winCol0 + cw.winCols;    // (inside the raster: no overflow)
  q.i0 = cw.winRow0 > q.row0 ? cw.winRow0 - q.row0 : 0u;
  q.i1 = rowEnd > q.row0 ? min(ch.r, rowEnd - q.row0) : 0u;
  q.x0 = cw.winCol0 > q.col0 ? cw.winCol0 - q.col0 : 0u;
  q.x1 = colEnd > q.col0 ? min(ch.c, colEnd - q.col0) : 0u;
  if (q.x0 >= q.x1 || q.i0 >= q.i1) q.i0 = q.i1 = q.x0 = q.x1 = 0u;
  return q;
}

}    // namespace

// staged tiles [n][r][c] and staged mask [n][r][c] <- raster.  T: u8 / u16 / u32 (integers of either sign), float, double.
template<class T>
__global__ void __launch_bounds__(256) k_rtn_cut(const typename RtnRaw<T>::U* __restrict__ raster, typename RtnRaw<T>::U* __restrict__ stage,
                                                 u8* __restrict__ stageMask, RtnCut cn, u32 lanesLog2, u32 stripRows, u32 stripsPerTile, u64 nUnits)
{
  using U = typename RtnRaw<T>::U;
  constexpr u32 V = 16u / (u32)sizeof(U);    // elements a vector
  const RtChunk& ch = cn.ch;
  const U nd = (U)cn.ndBits;
  const bool ndIsNaN = cn.ndIsNaN != 0u;
  const u32 lanes = 1u << lanesLog2, li = threadIdx.x & (lanes - 1u), rowInPass = threadIdx.x >> lanesLog2, rowsPerPass = blockDim.x >> lanesLog2;
  const u32 n = ch.c;
  for (u64 unit = blockIdx.x; unit < nUnits; unit += gridDim.x)
  {
    const u32 s = (u32)(unit % stripsPerTile), kk = (u32)(unit / stripsPerTile);
    const u32 iEnd = min(ch.r, (s + 1u) * stripRows);
    if (cn.pixelPitch != 1)
    {
      // the plain form: a lane an element
      for (u32 i = s * stripRows + rowInPass; i < iEnd; i += rowsPerPass)
      {
        const U* src = raster + rtnRasterAt(ch, cn.pixelPitch, kk, i);
        const u64 sa = rtStageAt(ch, kk, 0, i);
        for (u32 e = li; e < n; e += lanes)
        {
          const U v = src[(u64)e * cn.pixelPitch];
          stage[sa + e] = v;
          stageMask[sa + e] = rtnInvalid<T>(v, nd, ndIsNaN) ? 0u : 1u;
        }
      }
      continue;
    }
    for (u32 i0 = s * stripRows + rowInPass; i0 < iEnd; i0 += 4u * rowsPerPass)
    {
      const U* src[4];
      u64 sa[4];
      u32 head[4], nVec[4];
      uint4 x[4];
#pragma unroll
      for (int q = 0; q < 4; q++)
      {
        const u32 i = i0 + (u32)q * rowsPerPass;
        src[q] = raster; sa[q] = 0; head[q] = 0u; nVec[q] = 0u;
        x[q] = make_uint4(0u, 0u, 0u, 0u);
        if (i >= iEnd) continue;
        src[q] = raster + rtnRasterAt(ch, 1, kk, i); sa[q] = rtStageAt(ch, kk, 0, i);
        const u32 mis = ((u32)(uintptr_t)src[q] & 15u) / (u32)sizeof(U);
        head[q] = min(n, (V - mis) & (V - 1u));
        nVec[q] = (n - head[q]) / V;
        if (li < nVec[q]) x[q] = loadStreaming(reinterpret_cast<const uint4*>(src[q] + head[q]) + li);
      }
#pragma unroll
      for (int q = 0; q < 4; q++)
      {
        if (i0 + (u32)q * rowsPerPass >= iEnd) continue;
        const uint4* sv = reinterpret_cast<const uint4*>(src[q] + head[q]);
        U* d = stage + sa[q] + head[q];
        u8* m = stageMask + sa[q] + head[q];
        const u32 dstAlign = (u32)(uintptr_t)d & 15u;
        for (u32 v = li; v < nVec[q]; v += lanes)    // (the first round's vector is loaded already; rows of more than 64 vectors go on)
        {
          const uint4 xv = v == li ? x[q] : loadStreaming(sv + v);
          rtStore16<U>(d + (size_t)v * V, xv, dstAlign);
          U t[V];
          pxUnpack<U>(xv, t);
          u64 lo = 0, hi = 0;
#pragma unroll
          for (u32 k = 0; k < V; k++)
          {
            const u64 ok = rtnInvalid<T>(t[k], nd, ndIsNaN) ? 0u : 1u;
            if (k < 8u) lo |= ok << (8u * k); else hi |= ok << (8u * (k - 8u));
          }
          rtnStoreValid<V>(m + (size_t)v * V, lo, hi);
        }
        auto one = [&](u32 e)
        {
          const U v = src[q][e];
          stage[sa[q] + e] = v;
          stageMask[sa[q] + e] = rtnInvalid<T>(v, nd, ndIsNaN) ? 0u : 1u;
        };
        for (u32 e = li; e < head[q]; e += lanes) one(e);
        for (u32 e = head[q] + nVec[q] * V + li; e < n; e += lanes) one(e);
      }
    }
  }
}

// window <- select(staged valid byte, staged element, fill), the window's valid bytes <- the staged ones (windowMask != nullptr).
// U: u8 / u16 / u32 / u64 (the select does not care about signedness or float: an instantiation a size).
template<class U>
__global__ void __launch_bounds__(256) k_rtn_paste(const U* __restrict__ stage, const u8* __restrict__ stageMask, U* __restrict__ window,
                                                   u8* __restrict__ windowMask, RtnPaste pn, u32 lanesLog2, u32 stripRows, u32 stripsPerTile, u64 nUnits)
{
  constexpr u32 V = 16u / (u32)sizeof(U);    // elements a vector
  const RwChunk& cw = pn.cw;
  const RtChunk& ch = cw.ch;
  const U fill = (U)pn.fillBits;
  const u32 lanes = 1u << lanesLog2, li = threadIdx.x & (lanes - 1u), rowInPass = threadIdx.x >> lanesLog2, rowsPerPass = blockDim.x >> lanesLog2;
  for (u64 unit = blockIdx.x; unit < nUnits; unit += gridDim.x)
  {
    const u32 s = (u32)(unit % stripsPerTile), kk = (u32)(unit / stripsPerTile);
    const RtnClip clip = rtnClip(cw, kk);
    const u32 n = clip.x1 - clip.x0;
    const u32 iBegin = max(clip.i0, s * stripRows), iEnd = min(clip.i1, (s + 1u) * stripRows);
    if (cw.pixelPitch != 1)
    {
      // the plain form: a lane an element
      for (u32 i = iBegin + rowInPass; i < iEnd; i += rowsPerPass)
      {
        const u64 sa = rtStageAt(ch, kk, 0, i) + clip.x0;
        const u64 wr = (u64)(clip.row0 + i - cw.winRow0), wc = (u64)(clip.col0 + clip.x0 - cw.winCol0);
        U* dst = window + wr * ch.rowPitch + wc * cw.pixelPitch;
        u8* dm = windowMask ? windowMask + wr * pn.maskRowPitch + wc : nullptr;
        for (u32 e = li; e < n; e += lanes)
        {
          const u8 ok = stageMask[sa + e];
          dst[(u64)e * cw.pixelPitch] = ok ? stage[sa + e] : fill;
          if (dm) dm[e] = ok;
        }
      }
      continue;
    }
    for (u32 i0 = iBegin + rowInPass; i0 < iEnd; i0 += 4u * rowsPerPass)
    {
      u64 sa[4], wr[4];
      u32 head[4], nVec[4];
      uint4 x[4];
      const u64 wc = (u64)(clip.col0 + clip.x0 - cw.winCol0);
#pragma unroll
      for (int q = 0; q < 4; q++)
      {
        const u32 i = i0 + (u32)q * rowsPerPass;
        sa[q] = 0; wr[q] = 0; head[q] = 0u; nVec[q] = 0u;
        x[q] = make_uint4(0u, 0u, 0u, 0u);
        if (i >= iEnd) continue;
        sa[q] = rtStageAt(ch, kk, 0, i) + clip.x0;
        wr[q] = (u64)(clip.row0 + i - cw.winRow0);
        const u32 mis = ((u32)(uintptr_t)(stage + sa[q]) & 15u) / (u32)sizeof(U);
        head[q] = min(n, (V - mis) & (V - 1u));
        nVec[q] = (n - head[q]) / V;
        if (li < nVec[q]) x[q] = loadStreaming(reinterpret_cast<const uint4*>(stage + sa[q] + head[q]) + li);
      }
#pragma unroll
      for (int q = 0; q < 4; q++)
      {
        if (i0 + (u32)q * rowsPerPass >= iEnd) continue;
        const U* src = stage + sa[q];
        const u8* sm = stageMask + sa[q];
        const uint4* sv = reinterpret_cast<const uint4*>(src + head[q]);
        U* dst = window + wr[q] * ch.rowPitch + wc;
        u8* dm = windowMask ? windowMask + wr[q] * pn.maskRowPitch + wc : nullptr;
        U* d = dst + head[q];
        const u32 dstAlign = (u32)(uintptr_t)d & 15u;
        for (u32 v = li; v < nVec[q]; v += lanes)
        {
          const uint4 xv = v == li ? x[q] : loadStreaming(sv + v);
          u64 lo, hi;
          rtnLoadValid<V>(sm + head[q] + (size_t)v * V, lo, hi);
          U t[V];
          pxUnpack<U>(xv, t);
#pragma unroll
          for (u32 k = 0; k < V; k++)
          {
            const u32 ok = (u32)((k < 8u ? lo >> (8u * k) : hi >> (8u * (k - 8u))) & 0xFFu);
            t[k] = ok ? t[k] : fill;
          }
          const uint4 y = pxPack<U>(t);
          if (dstAlign == 0u) storeStreaming(reinterpret_cast<uint4*>(d + (size_t)v * V), y);
          else rtStore16<U>(d + (size_t)v * V, y, dstAlign);
          if (dm) rtnStoreValid<V>(dm + head[q] + (size_t)v * V, lo, hi);
        }
        auto one = [&](u32 e)
        {
          const u8 ok = sm[e];
          dst[e] = ok ? src[e] : fill;
          if (dm) dm[e] = ok;
        };
        for (u32 e = li; e < head[q]; e += lanes) one(e);
        for (u32 e = head[q] + nVec[q] * V + li; e < n; e += lanes) one(e);
      }
    }
  }
}

namespace {

struct RtnGeometry { u32 lanesLog2, stripRows, stripsPerTile; u64 nUnits; };

RtnGeometry rtnGeometry(const RtChunk& ch, u32 elemBytes)
{
  RtnGeometry g;
  g.lanesLog2 = rtLanesPerRowLog2(ch.c, elemBytes);
  g.stripRows = std::max(kRtStripRows, 256u >> g.lanesLog2);    // (short rows: every lane of the workgroup has a row)
  g.stripsPerTile = (ch.r + g.stripRows - 1) / g.stripRows;
  g.nUnits = (u64)ch.n * g.stripsPerTile;
  return g;
}

template<class T>
void rtnLaunchCut(const void* dRaster, void* dStage, u8* dStageMask, const RtnCut& cn, hipStream_t st)
{
  using U = typename RtnRaw<T>::U;
  const RtnGeometry g = rtnGeometry(cn.ch, (u32)sizeof(U));
  const dim3 grid((unsigned)std::min<u64>(g.nUnits, 1u << 16)), block(256);
  hipLaunchKernelGGL(k_rtn_cut<T>, grid, block, 0, st, (const U*)dRaster, (U*)dStage, dStageMask, cn, g.lanesLog2, g.stripRows, g.stripsPerTile, g.nUnits);
}

template<class U>
void rtnLaunchPaste(const void* dStage, const u8* dStageMask, void* dWindow, u8* dWindowMask, const RtnPaste& pn, hipStream_t st)
{
  const RtnGeometry g = rtnGeometry(pn.cw.ch, (u32)sizeof(U));
  const dim3 grid((unsigned)std::min<u64>(g.nUnits, 1u << 16)), block(256);
  hipLaunchKernelGGL(k_rtn_paste<U>, grid, block, 0, st, (const U*)dStage, dStageMask, (U*)dWindow, dWindowMask, pn, g.lanesLog2, g.stripRows, g.stripsPerTile,
                     g.nUnits);
}

}    // namespace

void launchRasterCutNoData(const void* dRaster, void* dStage, u8* dStageMask, const RtnCut& cn, int dt, hipStream_t st)
{
  const RtChunk& ch = cn.ch;
  if (ch.n == 0 || ch.r == 0 || ch.c == 0 || ch.nBands != 1 || cn.pixelPitch == 0) return;
  switch (dt)
  {
    case DT_Char: case DT_Byte: rtnLaunchCut<u8>(dRaster, dStage, dStageMask, cn, st); break;
    case DT_Short: case DT_UShort: rtnLaunchCut<u16>(dRaster, dStage, dStageMask, cn, st); break;
    case DT_Int: case DT_UInt: rtnLaunchCut<u32>(dRaster, dStage, dStageMask, cn, st); break;
    case DT_Float: rtnLaunchCut<float>(dRaster, dStage, dStageMask, cn, st); break;
    case DT_Double: rtnLaunchCut<double>(dRaster, dStage, dStageMask, cn, st); break;
    default: break;
  }
}

void launchWindowPasteNoData(const void* dStage, const u8* dStageMask, void* dWindow, u8* dWindowMask, const RtnPaste& pn, u32 elemBytes, hipStream_t st)
{
  const RtChunk& ch = pn.cw.ch;
  if (ch.n == 0 || ch.r == 0 || ch.c == 0 || ch.nBands != 1 || pn.cw.pixelPitch == 0 || pn.cw.winRows == 0 || pn.cw.winCols == 0) return;
  switch (elemBytes)
  {
    case 1: rtnLaunchPaste<u8>(dStage, dStageMask, dWindow, dWindowMask, pn, st); break;
    case 2: rtnLaunchPaste<u16>(dStage, dStageMask, dWindow, dWindowMask, pn, st); break;
    case 4: rtnLaunchPaste<u32>(dStage, dStageMask, dWindow, dWindowMask, pn, st); break;
    case 8: rtnLaunchPaste<u64>(dStage, dStageMask, dWindow, dWindowMask, pn, st); break;
    default: break;
  }
}

}    // namespace lerc
