// tile_decode_dev.h -- device functions of the general block decoder (tile_decode.hip) that other kernels share: a block's header, its length, its elements.
#pragma once
#include "kernels.h"
#include "wave_utils.h"

namespace lerc {

struct BlkInfo
{
  u32 len;        // total bytes of the block
  u32 cnt;        // element count stored in the bit stuffer header
  u32 nLut;       // LUT entries without the implicit 0
  u32 payload;    // offset of the first payload byte relative to the block start
  u8 flag, mode, diff, tc, offBytes, nb, lut, dtUsed;
};

// The first 16 bytes of a block, which hold every header field there is (flag, offset of up to 8 bytes, the bit stuffer's
// first byte, a count of up to 4 bytes, the LUT size: 15 bytes) -- fetched with five aligned 32-bit loads that are all in
// flight at once, where a parse that goes byte by byte waits for memory half a dozen times in a row (flag -> offset type
// -> bit width -> count -> LUT size).  Bytes at or behind `end` read as zero; no load touches a 4-byte unit that lies
// entirely outside [blob, blob + end).
struct Win16
{
  u64 lo, hi;
  __device__ __forceinline__ u32 byteAt(u32 k) const { return (u32)((k < 8u ? lo >> (8u * k) : hi >> (8u * (k - 8u))) & 255u); }
};

__device__ __forceinline__ Win16 funnel16(const u32 (&d)[5], u32 sh, u32 have)
{
  u32 x[4];
#pragma unroll
  for (int k = 0; k < 4; k++) x[k] = (u32)((((u64)d[k + 1] << 32) | d[k]) >> sh);
  Win16 w;
  w.lo = ((u64)x[1] << 32) | x[0];
  w.hi = ((u64)x[3] << 32) | x[2];
  // blank what lies at or behind the end (have = bytes of the window inside the blob)
  if (have < 16u)
  {
    if (have <= 8u) { w.hi = 0; w.lo = have == 0u ? 0ull : (w.lo & (~0ull >> (64u - 8u * have))); }
    else w.hi &= ~0ull >> (64u - 8u * (have - 8u));
  }
  return w;
}

// bytes pos ... pos + 15 of blob (any memory, any alignment)
__device__ __forceinline__ Win16 loadWin16(const u8* __restrict__ blob, u32 pos, u32 end)
{
  const uintptr_t A = (uintptr_t)blob + pos, E = (uintptr_t)blob + end;
  const u32* wp = reinterpret_cast<const u32*>(A & ~(uintptr_t)3);
  u32 d[5];
#pragma unroll
  for (int k = 0; k < 5; k++) d[k] = ((uintptr_t)(wp + k) < E) ? wp[k] : 0u;
  return funnel16(d, (u32)(A & 3u) * 8u, end > pos ? min(16u, end - pos) : 0u);
}

// the same out of an LDS array that starts on a 4-byte boundary (kept apart so that the loads stay LDS loads)
__device__ __forceinline__ Win16 loadWin16Words(const u32* words, u32 pos, u32 end)
{
  const u32 w0 = pos >> 2;
  u32 d[5];
#pragma unroll
  for (int k = 0; k < 5; k++) d[k] = (4u * (w0 + k) < end) ? words[w0 + k] : 0u;
  return funnel16(d, (pos & 3u) * 8u, end > pos ? min(16u, end - pos) : 0u);
}

// ... where the array is known to reach 20 bytes beyond `pos` (what lies behind `end` is blanked all the same): five loads
// without a condition, which the compiler can issue together
__device__ __forceinline__ Win16 loadWin16WordsRoomy(const u32* words, u32 pos, u32 end)
{
  const u32 w0 = pos >> 2;
  u32 d[5];
#pragma unroll
  for (int k = 0; k < 5; k++) d[k] = words[w0 + k];
  return funnel16(d, (pos & 3u) * 8u, end > pos ? min(16u, end - pos) : 0u);
}

// 0 = ok, 1 = not a valid block here, 2 = raw block whose valid count is not known to the caller.
// Mirrors the checks of Lerc2::ReadTile and BitStuffer2::Decode; additionally refuses element counts
// that differ from the block's valid pixel count (the reference would read past its buffer there).
// `h` holds the block's first 16 bytes, pos / end say where it lies in its stream.
template<int TBYTES>
__device__ __forceinline__ int parseWindow(const Win16& h, u32 pos, u32 end, const BandParams& p, int nValid, u32 maxCount, BlkInfo& b)
{
  b.len = 0;
  if (pos >= end) return 1;
  const u32 flag = h.byteAt(0);
  b.flag = (u8)flag;
  b.diff = (p.version >= 5 && (flag & 4u)) ? 1 : 0;
  b.mode = (u8)(flag & 3u);
  b.tc = (u8)(flag >> 6);
  b.offBytes = 0; b.nb = 0; b.lut = 0; b.cnt = 0; b.nLut = 0; b.payload = 1; b.dtUsed = (u8)p.dt;
  u64 len = 1;
  if (b.diff && p.nDepth == 1) return 1;    // (difference to the slice before: there is none, Lerc2.cpp ReadTile refuses)
  if (b.mode == 2) { b.len = 1; return 0; }
  if (b.mode == 0)
  {
    if (b.diff) return 1;
    if (nValid < 0) return 2;
    len = 1 + (u64)nValid * TBYTES;
  }
  else
  {
    const int dtU = typeUsed((b.diff && p.dt < DT_Float) ? (int)DT_Int : p.dt, b.tc);
    if (dtU == DT_Undefined) return 1;
    b.dtUsed = (u8)dtU;
    b.offBytes = (u8)dtSize(dtU);
    len = 1 + b.offBytes;
    if (b.mode == 1)
    {
      const u32 at = (u32)len;                      // (relative to the block's start from here on: <= 9)
      if ((u64)pos + at >= end) return 1;
      const u32 b0 = h.byteAt(at);
      const u32 code = b0 >> 6;
      const int cb = (code == 0) ? 4 : 3 - (int)code;
      if (cb == 0) return 1;
      b.lut = (b0 & 32u) ? 1 : 0;
      b.nb = (u8)(b0 & 31u);
      if ((u64)pos + at + 1 + cb > end) return 1;
      // the count's cb bytes start at at + 1 <= 10: inside the window
      const u32 sh = 8u * (at + 1u);
      const u64 two = sh < 64u ? ((h.lo >> sh) | (sh ? h.hi << (64u - sh) : 0ull)) : (h.hi >> (sh - 64u));
      const u32 cnt = (u32)two & (cb == 4 ? 0xFFFFFFFFu : ((1u << (8 * cb)) - 1u));
      b.cnt = cnt;
      if (cnt == 0 || cnt > maxCount || b.nb == 0) return 1;
      if (nValid >= 0 && cnt != (u32)nValid) return 1;
      len += 1 + cb;
      if (!b.lut) { b.payload = (u32)len; len += ((u64)cnt * b.nb + 7) >> 3; }
      else
      {
        if ((u64)pos + len >= end) return 1;
        const int nLut = (int)h.byteAt((u32)len) - 1;    // (at most byte 14)
        if (nLut < 1) return 1;
        b.nLut = (u32)nLut;
        len += 1;
        b.payload = (u32)len;
        len += ((u64)nLut * b.nb + 7) >> 3;
        len += ((u64)cnt * bitLen((u32)nLut) + 7) >> 3;
      }
    }
  }
  if ((u64)pos + len > end) return 1;
  b.len = (u32)len;
  return 0;
}

// What a walk needs of parseWindow -- the block's length, or that there is none -- without a branch: every lane of a wave looks
// at another position, so every branch of the parse is taken by some lane, and the bookkeeping of who is in which costs more
// than the arithmetic (k_rank_chunks parses every position of the stream: 480 instructions a position that way, R this way).
// offPack: bytes of the offset for type code tc and difference flag d, 4 bits at (tc * 2 + d) * 4, 0 = no such type
// (typeUsed, Lerc2.h:528-542), see offsetBytesPack.  Returns the length, 0 = no block, kLenRawUnknown = a raw block whose
// valid count the caller does not know (nValid < 0).
static const u32 kLenRawUnknown = 0xFFFFFFFFu;

__device__ __forceinline__ u32 offsetBytesPack(const BandParams& p)
{
  u32 pack = 0;
  for (int tc = 0; tc < 4; tc++)
    for (int d = 0; d < 2; d++)
    {
      const int dtU = typeUsed((d && p.dt < DT_Float) ? (int)DT_Int : p.dt, tc);
      const u32 n = (dtU == DT_Undefined) ? 0u : (u32)dtSize(dtU);
      pack |= (n > 8u ? 0u : n) << ((tc * 2 + d) * 4);    // (8 fits 4 bits)
    }
  return pack;
}

template<int TBYTES>
__device__ __forceinline__ u32 blockLength(const Win16& h, u32 pos, u32 end, const BandParams& p, u32 offPack, int nValid, u32 maxCount)
{
  const u32 flag = (u32)h.lo & 255u;
  const u32 mode = flag & 3u, tc = flag >> 6;
  const u32 diff = (p.version >= 5) ? ((flag >> 2) & 1u) : 0u;
  const u32 offB = (offPack >> ((tc * 2u + diff) * 4u)) & 15u;
  // the bit stuffer's header behind the offset: first byte, count (1, 2 or 4 bytes), LUT size -- bytes at + 0 ... at + 5
  const u32 at = 1u + offB;                         // <= 9
  const u32 sh = 8u * at;
  const u64 six = sh < 64u ? ((h.lo >> sh) | ((h.hi << 1) << (63u - sh))) : h.hi >> (sh - 64u);    // (sh >= 8)
  const u32 b0 = (u32)six & 255u;
  const u32 code = b0 >> 6;
  const u32 cb = (code == 0u) ? 4u : 3u - code;     // 0: no such code
  const u32 nb = b0 & 31u, lut = (b0 >> 5) & 1u;
  const u32 cnt = (u32)(six >> 8) & (cb == 4u ? 0xFFFFFFFFu : ((1u << (8u * cb)) - 1u));
  const u32 hdr = at + 1u + cb;
  const u32 nLut = ((u32)(six >> (8u * (1u + cb))) & 255u) - 1u;    // (the byte behind the count; 0xFFFFFFFF for a zero byte)
  const u32 nbIdx = (u32)bitLen(nLut & 255u);
  const u32 plain = hdr + ((cnt * nb + 7u) >> 3);
  const u32 withLut = hdr + 1u + (((nLut & 255u) * nb + 7u) >> 3) + ((cnt * nbIdx + 7u) >> 3);
  const bool okStuffed = (offB != 0u) & (cb != 0u) & (cnt != 0u) & (cnt <= maxCount) & (nb != 0u) & ((nValid < 0) | (cnt == (u32)nValid))
                       & ((lut == 0u) | ((nLut >= 1u) & (nLut < 255u)));
  u32 len = lut ? withLut : plain;
  len = okStuffed ? len : 0u;
  len = (mode == 3u) ? (offB ? 1u + offB : 0u) : len;
  len = (mode == 2u) ? 1u : len;
  const u32 raw = diff ? 0u : (nValid < 0 ? kLenRawUnknown : 1u + (u32)nValid * (u32)TBYTES);
  len = (mode == 0u) ? raw : len;
  if (diff && p.nDepth == 1) len = 0u;
  if (len != kLenRawUnknown && ((u64)pos + len > end || pos >= end)) len = 0u;
  return len;
}

template<int TBYTES>
__device__ __forceinline__ int parseBlock(const u8* __restrict__ blob, u32 pos, u32 end, const BandParams& p, int nValid,
                                          u32 maxCount, BlkInfo& b)
{
  return parseWindow<TBYTES>(loadWin16(blob, pos, end), pos, end, p, nValid, maxCount, b);
}

// the block at byte `pos` of an LDS array given as words
template<int TBYTES>
__device__ __forceinline__ int parseBlockWords(const u32* words, u32 pos, u32 end, const BandParams& p, int nValid,
                                               u32 maxCount, BlkInfo& b)
{
  return parseWindow<TBYTES>(loadWin16Words(words, pos, end), pos, end, p, nValid, maxCount, b);
}

// little-endian bit field read with a hard upper bound on the bytes touched
__device__ __forceinline__ u32 readBits(const u8* __restrict__ blob, u64 bitPos, int nbits, u32 end)
{
  const u64 byte = bitPos >> 3;
  const int sh = (int)(bitPos & 7);
  const int need = (sh + nbits + 7) >> 3;    // <= 5
  u64 v = 0;
  for (int i = 0; i < need; i++)
    if (byte + i < end) v |= (u64)blob[byte + i] << (8 * i);
  return (u32)((v >> sh) & ((nbits >= 32) ? 0xFFFFFFFFull : ((1ull << nbits) - 1)));
}

// element i of a bit-stuffed field of n elements, nb bits each, that starts at bit `at` of the blob
// (BitStuffer2::BitUnStuff, BitStuffer2.cpp:476-540; codec 2: BitUnStuff_Before_Lerc2v3, :355-425)
__device__ __forceinline__ u32 unstuffElement(const u8* __restrict__ blob, u64 at, u32 i, int nb, u32 n, u32 end, int version)
{
  if (version >= 3) return readBits(blob, at + (u64)i * nb, nb, end);
  const OldBitLayout o = oldBitLayout(i, nb, n);
  u32 v = readBits(blob, at + o.pos0, (int)o.n0, end) << o.n1;
  if (o.n1) v |= readBits(blob, at + o.pos1, (int)o.n1, end);
  return v;
}

}    // namespace lerc
