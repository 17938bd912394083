// tile_batch_dev.h -- what a workgroup of 256 threads that owns one tile of a batch needs (tile_mask_batch.hip, tile_byte_batch.hip):
// sums, Fletcher32 over a finished blob, an exclusive scan in place.
#pragma once
#include "lerc_common.h"
#include "wave_utils.h"

namespace lerc {

// sums of a workgroup's 256 threads (s: 4 words of LDS); every thread gets the result
__device__ __forceinline__ u64 blockSum(u64 v, u64* s)
{
  v = waveSum(v);
  __syncthreads();
  if (laneId() == 0) s[waveId()] = v;
  __syncthreads();
  return s[0] + s[1] + s[2] + s[3];
}

// Fletcher32 terms of bytes[0 .. len): byte p counts as byte << 8 where p is even, with weight p >> 1 (misc_kernels.hip:
// k_fletcher); A, B mod 65535 in every thread.  16-byte loads from the first aligned address on.
__device__ __forceinline__ void blockFletcher(const u8* __restrict__ bytes, u32 len, u64* s, u64& Aout, u64& Bout)
{
  u64 A = 0, B = 0;
  const u32 head = min(len, (u32)((16u - ((u32)(uintptr_t)bytes & 15u)) & 15u));
  const u32 nVec = (len - head) >> 4;
  const uint4* vec = reinterpret_cast<const uint4*>(bytes + head);
  for (u32 i = threadIdx.x; i < nVec; i += 256u)
  {
    const u32 q = head + (i << 4), odd = q & 1u;
    const uint4 x = vec[i];
    const u32 w[4] = { x.x, x.y, x.z, x.w };
    u32 sumC = 0, inner = 0;
#pragma unroll
    for (u32 j = 0; j < 16u; j++)
    {
      const u32 byte = (w[j >> 2] >> (8u * (j & 3u))) & 255u;
      const u32 c = byte << (((odd + j) & 1u) ? 0u : 8u);
      sumC += c;
      inner += ((odd + j) >> 1) * c;
    }
    A += sumC;
    B += (u64)(q >> 1) * sumC + inner;
  }
  if (threadIdx.x == 0)
  {
    for (u32 p = 0; p < head; p++) { const u32 c = (u32)bytes[p] << ((p & 1u) ? 0 : 8); A += c; B += (u64)(p >> 1) * c; }
    for (u32 p = head + (nVec << 4); p < len; p++) { const u32 c = (u32)bytes[p] << ((p & 1u) ? 0 : 8); A += c; B += (u64)(p >> 1) * c; }
  }
  A %= 65535u; B %= 65535u;
  Aout = blockSum(A, s) % 65535u;
  Bout = blockSum(B, s) % 65535u;
}

__device__ __forceinline__ u32 fletcherFold(u64 A, u64 B, u32 len)    // fletcherFinish (misc_kernels.hip)
{
  const u64 N = ((u64)len + 1) / 2;
  u64 s1 = A % 65535u;
  u64 s2 = ((N % 65535u) * s1 + 65535u - (B % 65535u)) % 65535u;
  if (s1 == 0) s1 = 0xffff;
  if (s2 == 0) s2 = 0xffff;
  return (u32)((s2 << 16) | s1);
}

// exclusive scan of x[0 .. n) in place by one workgroup of 256 threads, x[n] = the total (s: 256 words of LDS)
__device__ __forceinline__ u32 blockScanInPlace(u32* __restrict__ x, u32 n, u32* s)
{
  const u32 per = (n + 255u) / 256u, from = min(n, threadIdx.x * per), to = min(n, from + per);
  u32 sum = 0;
  for (u32 i = from; i < to; i++) sum += x[i];
  s[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) { u32 run = 0; for (u32 i = 0; i < 256u; i++) { const u32 y = s[i]; s[i] = run; run += y; } s[256] = run; }
  __syncthreads();
  u32 run = s[threadIdx.x];
  for (u32 i = from; i < to; i++) { const u32 y = x[i]; x[i] = run; run += y; }
  const u32 total = s[256];
  if (threadIdx.x == 0) x[n] = total;
  return total;
}

}    // namespace lerc
