// tile_encode_dev.h -- device functions of the general block encoder (tile_encode.hip) that other kernels share: the byte image of one block.
#pragma once
#include "wave_utils.h"
#include "block_plan.h"

namespace lerc {

// element i of a bit-stuffed field of n elements, nb bits each, that starts at bit `at` of the block image
// (BitStuffer2::BitStuff, BitStuffer2.cpp:432-472; codec 2: BitStuff_Before_Lerc2v3, :292-351)
__device__ __forceinline__ void stuffElement(u32* obuf, u32 at, u32 i, u32 v, int nb, u32 n, int version)
{
  if (version >= 3) { orBits(obuf, at + i * (u32)nb, v, nb); return; }
  const OldBitLayout o = oldBitLayout(i, nb, n);
  orBits(obuf, at + o.pos0, v >> o.n1, (int)o.n0);
  if (o.n1) orBits(obuf, at + o.pos1, v & ((1u << o.n1) - 1u), (int)o.n1);
}

// Distinct values of the block in increasing order (what the reference gets from SortQuantArray,
// Lerc2.cpp:2255-2266): repeated wave-min extraction.  Returns the number of distinct values, stores
// them to lutOut (if not null) and the per-element index into idx.
template<int E>
__device__ __forceinline__ u32 extractDistinct(const u32 (&q)[E], const int (&rank)[E], u32* lutOut, u32 (&idx)[E])
{
  u32 count = 0, last = 0;
  for (;;)
  {
    u32 m = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < E; k++)
      if (rank[k] >= 0 && (count == 0 || q[k] > last) && q[k] < m) m = q[k];
    m = waveMin(m);
    if (m == 0xFFFFFFFFu) break;
#pragma unroll
    for (int k = 0; k < E; k++)
      if (rank[k] >= 0 && q[k] == m) idx[k] = count;
    if (lutOut && laneId() == 0) lutOut[count] = m;
    last = m;
    count++;
  }
  return count;
}


// Builds the byte image of one block in LDS (obuf, zeroed here) -- Lerc2::WriteTile.
template<class Z, int E>
__device__ __forceinline__ void composeBlock(u32* obuf, u32* lutBuf, const BandParams& p, const Plan& pl, int n, int j0,
                                             bool diff, Z zMin, const Z (&val)[E], const u32 (&q)[E],
                                             const int (&rank)[E], u32 qMax)
{
  const int lane = laneId();
  const int nWords = (pl.nBytes + 3) / 4 + 2;
  for (int i = lane; i < nWords; i += 64) obuf[i] = 0;
  waveSync();

  u32 flag = (u32)(((j0 >> 3) & 15) << 2);
  if (p.version >= 5) flag = diff ? (flag | 4u) : (flag & 0x38u);

  if (pl.kind == 0)
  {
    if (lane == 0) orBits(obuf, 0, flag | 2u, 8);
  }
  else if (pl.kind == 1)
  {
    if (lane == 0) orBits(obuf, 0, flag, 8);
#pragma unroll
    for (int k = 0; k < E; k++)
      if (rank[k] >= 0)
      {
        u64 bits = 0;
        Z tmp = val[k];
        memcpy(&bits, &tmp, sizeof(Z));
        const u32 bp = 8u * (1u + (u32)rank[k] * (u32)sizeof(Z));
        if (sizeof(Z) <= 4) orBits(obuf, bp, (u32)bits, 8 * (int)sizeof(Z));
        else { orBits(obuf, bp, (u32)bits, 32); orBits(obuf, bp + 32, (u32)(bits >> 32), 32); }
      }
  }
  else
  {
    flag |= (pl.kind == 2) ? 3u : 1u;
    flag |= (u32)pl.tc << 6;
    const int offBytes = dtSize(pl.dtRed);
    if (lane == 0)
    {
      orBits(obuf, 0, flag, 8);
      const u64 ob = typedBits((double)zMin, pl.dtRed);
      if (offBytes <= 4) orBits(obuf, 8, (u32)ob, 8 * offBytes);
      else { orBits(obuf, 8, (u32)ob, 32); orBits(obuf, 40, (u32)(ob >> 32), 32); }
    }
    if (pl.kind >= 3)
    {
      const int cb = countFieldBytes((u32)n);
      const u32 code = (cb == 4) ? 0u : (u32)(3 - cb);
      const int nb = bitLen(qMax);
      u32 at = 8u * (1u + (u32)offBytes);    // bit cursor
      if (pl.kind == 3)
      {
        if (lane == 0) { orBits(obuf, at, (u32)nb | (code << 6), 8); orBits(obuf, at + 8, (u32)n, 8 * cb); }
        at += 8u * (1u + (u32)cb);
#pragma unroll
        for (int k = 0; k < E; k++)
          if (rank[k] >= 0) stuffElement(obuf, at, (u32)rank[k], q[k], nb, (u32)n, p.version);
      }
      else
      {
        u32 idx[E];
#pragma unroll
        for (int k = 0; k < E; k++) idx[k] = 0;
        const u32 nDistinct = extractDistinct<E>(q, rank, lutBuf, idx);
        waveSync();
        const u32 nLut = nDistinct - 1;
        const int nbIdx = bitLen(nLut);
        if (lane == 0)
        {
          orBits(obuf, at, (u32)nb | (code << 6) | 32u, 8);
          orBits(obuf, at + 8, (u32)n, 8 * cb);
          orBits(obuf, at + 8u * (1u + (u32)cb), nLut + 1, 8);
        }
        at += 8u * (2u + (u32)cb);
        for (u32 i = (u32)lane; i < nLut; i += 64) stuffElement(obuf, at, i, lutBuf[i + 1], nb, nLut, p.version);
        at += 8u * ((nLut * (u32)nb + 7) >> 3);
#pragma unroll
        for (int k = 0; k < E; k++)
          if (rank[k] >= 0) stuffElement(obuf, at, (u32)rank[k], idx[k], nbIdx, (u32)n, p.version);
      }
    }
  }
  waveSync();
}

}    // namespace lerc
