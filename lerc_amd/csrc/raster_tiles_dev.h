// raster_tiles_dev.h -- device pieces the staging kernels of the raster tile calls share (raster_tiles.hip, raster_tiles_px.hip,
// raster_window.hip): the store of a 16-byte vector in the widest pieces an address admits, where a staged row lies, and the padded
// LDS layout through which an interleaved row is transposed (described in raster_tiles_px.hip).  All of it is inlined: the kernels
// of the three files are what they were when each file held its own copy.
#pragma once
#include "raster_tiles.h"
#include "wave_utils.h"

#include <type_traits>

namespace lerc {

template<class T>
__device__ __forceinline__ void rtStore16(T* p, const uint4& x, u32 dstAlign)
{
  const u32 w[4] = { x.x, x.y, x.z, x.w };
  if (dstAlign == 0u) { *reinterpret_cast<uint4*>(p) = x; return; }
  if ((dstAlign & 7u) == 0u)
  {
    u64* q = reinterpret_cast<u64*>(p);
    q[0] = (u64)w[0] | ((u64)w[1] << 32);
    q[1] = (u64)w[2] | ((u64)w[3] << 32);
    return;
  }
  if (sizeof(T) <= 4 && (dstAlign & 3u) == 0u)
  {
    u32* q = reinterpret_cast<u32*>(p);
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = w[i];
    return;
  }
  if (sizeof(T) <= 2 && (dstAlign & 1u) == 0u)
  {
    u16* q = reinterpret_cast<u16*>(p);
#pragma unroll
    for (int i = 0; i < 8; i++) q[i] = (u16)(w[i >> 1] >> (16 * (i & 1)));
    return;
  }
  if (sizeof(T) == 1)
  {
    u8* q = reinterpret_cast<u8*>(p);
#pragma unroll
    for (int i = 0; i < 16; i++) q[i] = (u8)(w[i >> 2] >> (8 * (i & 3)));
  }
}

// where row i of band b of the chunk's tile kk lies in the staging buffer
__device__ __forceinline__ u64 rtStageAt(const RtChunk& ch, u32 kk, u32 b, u32 i)
{
  return (((u64)kk * ch.nBands + b) * ch.r + i) * ch.c;
}

// ---- the LDS layout of an interleaved row (raster_tiles_px.hip)

// T in LDS: units of T (1, 2, 4 bytes) or two dwords (8 bytes); a chunk is the V * pixelPitch elements one lane transposes
template<class T> struct PxLds
{
  using U = typename std::conditional<sizeof(T) == 8, u32, T>::type;
  static constexpr u32 V = 16u / (u32)sizeof(T);            // elements a 16-byte vector
  static constexpr u32 UE = (u32)(sizeof(T) / sizeof(U));   // units an element
  static constexpr u32 PU = 4u / (u32)sizeof(U);            // units a padding dword
};

// the chunk an element lies in, e / (V * pixelPitch), by multiplication: inv = ceil(2^20 / (V * P)) is exact while e * V * P < 2^20,
// and e < 16 + 512 * 8, V * P <= 128
__device__ __forceinline__ u32 pxChunkOf(u32 e, u32 inv) { return (e * inv) >> 20; }

template<class T> __device__ __forceinline__ u32 pxUnitAt(u32 e, u32 inv) { return e * PxLds<T>::UE + PxLds<T>::PU * pxChunkOf(e, inv); }

template<class T> __device__ __forceinline__ T pxRead(const typename PxLds<T>::U* s, u32 e, u32 inv)
{
  const u32 u = pxUnitAt<T>(e, inv);
  if constexpr (sizeof(T) == 8) return (T)s[u] | ((T)s[u + 1] << 32);
  else return s[u];
}

template<class T> __device__ __forceinline__ void pxWrite(typename PxLds<T>::U* s, u32 e, u32 inv, T x)
{
  const u32 u = pxUnitAt<T>(e, inv);
  if constexpr (sizeof(T) == 8) { s[u] = (u32)x; s[u + 1] = (u32)(x >> 32); }
  else s[u] = x;
}

// the dword at which 16-byte vector k of the run (elements k * V ..: a chunk is a whole number of vectors) begins
template<class T> __device__ __forceinline__ u32 pxVecAt(u32 k, u32 inv) { return 4u * k + pxChunkOf(k * PxLds<T>::V, inv); }

template<class T> __device__ __forceinline__ uint4 pxPack(const T (&t)[PxLds<T>::V])
{
  constexpr u32 V = PxLds<T>::V;
  u32 w[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
  for (u32 q = 0; q < V; q++)
  {
    if constexpr (sizeof(T) == 8) { w[2 * q] = (u32)t[q]; w[2 * q + 1] = (u32)(t[q] >> 32); }
    else w[q * (u32)sizeof(T) / 4u] |= (u32)t[q] << (8u * (u32)sizeof(T) * (q % (4u / (u32)sizeof(T))) % 32u);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template<class T> __device__ __forceinline__ void pxUnpack(const uint4& x, T (&t)[PxLds<T>::V])
{
  constexpr u32 V = PxLds<T>::V;
  const u32 w[4] = { x.x, x.y, x.z, x.w };
#pragma unroll
  for (u32 q = 0; q < V; q++)
  {
    if constexpr (sizeof(T) == 8) t[q] = (T)w[2 * q] | ((T)w[2 * q + 1] << 32);
    else t[q] = (T)(w[q * (u32)sizeof(T) / 4u] >> (8u * (u32)sizeof(T) * (q % (4u / (u32)sizeof(T))) % 32u));
  }
}

// elements of a row in front of the first 16-byte aligned address (at most n)
template<class T> __device__ __forceinline__ u32 pxHead(const T* p, u32 n)
{
  constexpr u32 V = PxLds<T>::V;
  const u32 mis = ((u32)(uintptr_t)p & 15u) / (u32)sizeof(T);
  return min(n, (V - mis) & (V - 1u));
}

// a pixel's nb elements, LDS elements e .., to g: the widest pieces the address of each admits
template<class T>
__device__ __forceinline__ void pxStoreRun(T* g, const typename PxLds<T>::U* su, u32 e, u32 nb, u32 inv)
{
  constexpr u32 V = PxLds<T>::V;
  u32 k = 0;
  while (k < nb)
  {
    T* p = g + k;
    const u32 a = (u32)(uintptr_t)p, left = nb - k;
    if ((a & 15u) == 0u && left >= V)
    {
      T t[V];
#pragma unroll
      for (u32 q = 0; q < V; q++) t[q] = pxRead<T>(su, e + k + q, inv);
      *reinterpret_cast<uint4*>(p) = pxPack<T>(t);
      k += V;
      continue;
    }
    if constexpr (sizeof(T) <= 4)
    {
      constexpr u32 N8 = 8u / (u32)sizeof(T);
      if ((a & 7u) == 0u && left >= N8)
      {
        u64 x = 0;
#pragma unroll
        for (u32 q = 0; q < N8; q++) x |= (u64)pxRead<T>(su, e + k + q, inv) << (8u * (u32)sizeof(T) * q);
        *reinterpret_cast<u64*>(p) = x;
        k += N8;
        continue;
      }
    }
    if constexpr (sizeof(T) <= 2)
    {
      constexpr u32 N4 = 4u / (u32)sizeof(T);
      if ((a & 3u) == 0u && left >= N4)
      {
        u32 x = 0;
#pragma unroll
        for (u32 q = 0; q < N4; q++) x |= (u32)pxRead<T>(su, e + k + q, inv) << (8u * (u32)sizeof(T) * q);
        *reinterpret_cast<u32*>(p) = x;
        k += N4;
        continue;
      }
    }
    if constexpr (sizeof(T) == 1)
    {
      if ((a & 1u) == 0u && left >= 2u)
      {
        *reinterpret_cast<u16*>(p) = (u16)((u32)pxRead<T>(su, e + k, inv) | ((u32)pxRead<T>(su, e + k + 1u, inv) << 8));
        k += 2u;
        continue;
      }
    }
    *p = pxRead<T>(su, e + k, inv);
    k++;
  }
}

}    // namespace lerc
