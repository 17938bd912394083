// tile_encode_dev.h -- the stages of a block encoder's wave body, composed by the general kernel (tile_encode.hip: all depth slices,
// slice differences) and by the tile batches (tile_batch_dev.h: one value a pixel): the lanes of a block
// (blockLanes), a slice's values (gatherSlice), its statistics, quantised values and plan (analyseSlice), its byte image (composeBlock).
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


// ---- stage 1, the lanes of a block: the wave owns block position pos of a band cut into mb x mb blocks; lane l holds elements
// l, l + 64, ... of the block in row-major order.  The encoders' only place for a block's geometry and its elements' ranks.
struct BlockGeom { int i0, j0, tileW, nElem; };

__device__ __forceinline__ BlockGeom blockGeom(const BandParams& p, int pos, int mb)
{
  const int it = pos / p.nTH, jt = pos - it * p.nTH;
  BlockGeom g;
  g.i0 = it * mb; g.j0 = jt * mb;
  g.tileW = min(mb, p.nCols - g.j0);
  g.nElem = min(mb, p.nRows - g.i0) * g.tileW;
  return g;
}

// element k * 64 + lane: its pixel (the block's first where the element lies outside the block, e >= nElem) and its rank among the
// block's valid pixels, which is the reference's dataBuf index (-1: not valid); n counts the valid pixels of the steps so far.
// MASKED: valid pixels are compacted with __ballot / __popcll (every lane of the wave calls this); else every pixel of the block is
// valid, rank = element, and n is not touched.
template<bool MASKED>
__device__ __forceinline__ void blockLaneStep(const BandParams& p, const BlockGeom& g, int k, const u8* __restrict__ maskBits, int& n, i64& pix, int& rank)
{
  const int e = k * 64 + laneId();
  const bool inb = e < g.nElem;
  const int r = inb ? e / g.tileW : 0, c = inb ? e - r * g.tileW : 0;
  pix = (i64)(g.i0 + r) * p.nCols + (g.j0 + c);
  if (MASKED)
  {
    const bool valid = inb && (p.allValid || maskBit(maskBits, pix));
    const u64 bal = __ballot(valid);
    rank = valid ? n + __popcll(bal & laneMaskLt()) : -1;
    n += __popcll(bal);
  }
  else rank = inb ? e : -1;
}

template<int E>
struct BlockLanes
{
  int rank[E];
  i64 pix[E];
  int n, j0, nElem;    // valid pixels, first column, elements of the block
};

template<int E, bool MASKED>
__device__ __forceinline__ BlockLanes<E> blockLanes(const BandParams& p, int pos, const u8* __restrict__ maskBits)
{
  const BlockGeom g = blockGeom(p, pos, E == 1 ? 8 : 16);
  BlockLanes<E> L;
  L.j0 = g.j0; L.nElem = g.nElem;
  L.n = MASKED ? 0 : g.nElem;
#pragma unroll
  for (int k = 0; k < E; k++) blockLaneStep<MASKED>(p, g, k, maskBits, L.n, L.pix[k], L.rank[k]);
  return L;
}

// the one byte of a position without valid pixels, "all zero" (Lerc2.cpp:1534-1538, :1960-1966)
__device__ __forceinline__ u8 emptyBlockByte(const BandParams& p, int j0)
{
  u32 flag = (u32)(((j0 >> 3) & 15) << 2);
  if (p.version >= 5) flag &= 0x38u;
  return (u8)(flag | 2u);
}

// ---- stage 2, a slice's values: slice iD of nD of the block's valid pixels into the lanes' registers and, by rank, into the wave's
// valBuf (the reference's dataBuf)
template<class T, int E>
__device__ __forceinline__ void gatherSlice(const BlockLanes<E>& L, const T* __restrict__ data, int nD, int iD, T* valBuf, T (&v)[E])
{
#pragma unroll
  for (int k = 0; k < E; k++)
  {
    v[k] = T(0);
    if (L.rank[k] >= 0) { v[k] = data[L.pix[k] * nD + iD]; valBuf[L.rank[k]] = v[k]; }
  }
  waveSync();
}

// ---- stage 3, slice analysis: range, "same as the previous element" count, quantised values and the plan of a block's n > 0 values
// v (also in valBuf by rank) of type Z -- a slice's values (GetValidDataAndStats, Lerc2.cpp:1717-1799) or their int differences to
// the previous depth slice (ComputeDiffSliceInt, :1803-1874).  What the two differ in is said by the caller:
//   dtZ        the values' data type for the plan: the band's, or DT_Int for differences
//   prevIsZero whether the element of rank 0 is compared with a "previous value" of 0: GetValidDataAndStats starts prevVal at 0 on
//              its all-valid branch only (:1735, against :1762-1775, where the first valid pixel counts as not the same);
//              ComputeDiffSliceInt starts it at 0 on both branches (:1822)
//   quantise   whether the block is quantised at all: maxZErr > 0 (NeedToQuantize, Lerc2.h:345-357); differences are tried for integer
//              lossless bands only, where maxZErr is 0.5
//   lossless   the quantiser is the integer subtraction (Quantize, Lerc2.h:359-376: maxZErr == 0.5 and an integer type); for differences
//              quantLossless<int> is the reference's (unsigned int)((int64)d - (int64)zMin) literally
template<class Z, int E>
struct SliceCode
{
  Z zMin;
  u32 q[E], qMax;
  Plan plan;
};

template<class Z, int E>
__device__ __forceinline__ SliceCode<Z, E> analyseSlice(const BandParams& p, int n, const Z (&v)[E], const int (&rank)[E], const Z* valBuf,
                                                        int dtZ, bool prevIsZero, bool quantise, bool lossless)
{
  SliceCode<Z, E> s;
  Z mn = valBuf[0], mx = valBuf[0];
#pragma unroll
  for (int k = 0; k < E; k++)
    if (rank[k] >= 0) { mn = (v[k] < mn) ? v[k] : mn; mx = (v[k] > mx) ? v[k] : mx; }
  mn = waveMinT(mn);
  mx = waveMaxT(mx);
  int same = 0;
#pragma unroll
  for (int k = 0; k < E; k++)
  {
    bool eq = false;
    if (rank[k] > 0) eq = (v[k] == valBuf[rank[k] - 1]);
    else if (rank[k] == 0) eq = prevIsZero && (v[k] == Z(0));
    same += __popcll(__ballot(eq));
  }
  const bool tryLut = (n > 4) && ((double)mx > (double)mn + 3 * p.maxZErr) && (2 * same > n);

  double mv = 0;
  bool quantOk = false;
  if (quantise)
  {
    mv = ((double)mx - (double)mn) * p.scale;
    quantOk = !(mv > (double)p.maxQ || (u32)(mv + 0.5) == 0);
  }
  s.qMax = 0;
#pragma unroll
  for (int k = 0; k < E; k++) s.q[k] = 0;
  if (quantOk)
  {
    const double z0 = (double)mn;
#pragma unroll
    for (int k = 0; k < E; k++)
      if (rank[k] >= 0)
      {
        s.q[k] = lossless ? quantLossless<Z>(v[k], mn) : (u32)(((double)v[k] - z0) * p.scale + 0.5);
        s.qMax = s.q[k] > s.qMax ? s.q[k] : s.qMax;
      }
    s.qMax = waveMax(s.qMax);
  }
  u32 nDistinct = 0;
  if (tryLut && quantOk)
  {
    u32 idxTmp[E];
    nDistinct = extractDistinct<E>(s.q, rank, nullptr, idxTmp);
  }
  s.zMin = mn;
  s.plan = planBlock<Z>(p, n, mn, mx, dtZ, tryLut, mv, s.qMax, nDistinct);
  return s;
}

// ---- stage 4, the byte image of one block in LDS (obuf, zeroed here) -- Lerc2::WriteTile.
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
