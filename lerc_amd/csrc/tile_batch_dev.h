// tile_batch_dev.h -- the device code the two families of tile batches share (tile_mask_batch.hip, tile_byte_batch.hip).  What a
// workgroup of 256 threads that owns one tile needs: sums, Fletcher32 over a finished blob, an exclusive scan in place, the codec 6
// header to and from bytes, the blobs' places in a packed arena, the walk over a tile's block headers, and a tile's mask (byte mask to
// bit mask, its run-length stream each way, counts, ranks, header and mask section written).  And what a wave that owns one
// block needs: the block encoder's body, a composition of the stages the general kernel uses (tile_encode_dev.h), and the
// block decoder's body.  Every piece of LDS is handed in by the kernel that owns it.
#pragma once
#include "lerc_common.h"
#include "wave_utils.h"
#include "block_plan.h"
#include "tile_encode_dev.h"
#include "tile_decode_dev.h"
#include "tile_batch.h"

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

// ---- Fletcher32 over blob[14 .. blobSize) (Lerc2.cpp:1037-1064), compared with / stored into the header's field at byte 10 (s: 4 words of LDS)
__device__ __forceinline__ bool tbChecksumOk(const u8* __restrict__ blob, u32 blobSize, u32 want, u64* s)
{
  u64 A, B;
  blockFletcher(blob + 14, blobSize - 14u, s, A, B);
  return fletcherFold(A, B, blobSize - 14u) == want;
}

// a workgroup per tile: the checksum of a finished blob the batch made
__device__ __forceinline__ void tbWriteChecksum(u8* __restrict__ arena, const TileBatchRec& rec, u64* s)
{
  if (rec.flags) return;
  u8* __restrict__ blob = arena + rec.offset;
  u64 A, B;
  blockFletcher(blob + 14, rec.blobSize - 14u, s, A, B);
  if (threadIdx.x == 0) putBytes(blob + 10, (u64)fletcherFold(A, B, rec.blobSize - 14u), 4);
}

// ---- packed arena: the batch's blobs back to back at 16-byte aligned offsets from arenaBase on, in tile order, by ONE workgroup
// (s: 257 words of LDS)
template<class Rec>
__device__ __forceinline__ void tbArenaPlace(Rec* __restrict__ tiles, u32 nTiles, u64 arenaBase, u64 arenaCapacity, u64* s)
{
  const u32 per = (nTiles + 255u) / 256u, from = min(nTiles, threadIdx.x * per), to = min(nTiles, from + per);
  u64 sum = 0;
  for (u32 i = from; i < to; i++) if (!tiles[i].head.flags) sum += ((u64)tiles[i].head.blobSize + 15ull) & ~15ull;
  s[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) { u64 run = 0; for (u32 i = 0; i < 256u; i++) { const u64 y = s[i]; s[i] = run; run += y; } s[256] = run; }
  __syncthreads();
  u64 run = arenaBase + s[threadIdx.x];
  for (u32 i = from; i < to; i++)
  {
    TileBatchRec& r = tiles[i].head;
    if (r.flags) continue;
    r.offset = run;
    if (run + r.blobSize > arenaCapacity) r.flags |= kTbArenaFull;
    run += ((u64)r.blobSize + 15ull) & ~15ull;
  }
}

// ---- band stacks: ONE workgroup folds the planes (tile * nBands + band) into tiles and places the tiles -- a tile's room is the sum
// of its planes' blobs, packed at 16-byte aligned offsets from arenaBase on or in the tile's slot; a plane's offset is the running sum
// inside its tile (any byte alignment).  A tile with a flagged plane, or one that does not fit, claims nothing: every plane of it is
// flagged.  (s: 257 words of LDS)
template<class Rec>
__device__ __forceinline__ void tbPlaceBands(Rec* __restrict__ planes, u32 nTiles, u32 nBands, u64 arenaBase, u64 arenaCapacity, u64 slotBytes,
                                             u64 firstTile, u64* s)
{
  const u32 per = (nTiles + 255u) / 256u, from = min(nTiles, threadIdx.x * per), to = min(nTiles, from + per);
  auto flagAll = [&](u32 i, u32 own, u32 others)
  {
    for (u32 k = 0; k < nBands; k++) { TileBatchRec& r = planes[(u64)i * nBands + k].head; if (!r.flags) r.flags = k == 0 ? own : others; }
  };
  u64 sum = 0;
  for (u32 i = from; i < to; i++)
  {
    u32 fl = 0;
    u64 size = 0;
    for (u32 k = 0; k < nBands; k++) { const TileBatchRec& r = planes[(u64)i * nBands + k].head; fl |= r.flags; size += r.blobSize; }
    if (!fl && (size > 0xFFFFFFFFull || (slotBytes && size > slotBytes))) { flagAll(i, kTbCapacity, kTbBand); continue; }
    if (fl) { flagAll(i, kTbBand, kTbBand); continue; }
    if (!slotBytes) sum += (size + 15ull) & ~15ull;
  }
  s[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) { u64 run = 0; for (u32 i = 0; i < 256u; i++) { const u64 y = s[i]; s[i] = run; run += y; } s[256] = run; }
  __syncthreads();
  u64 run = arenaBase + s[threadIdx.x];
  for (u32 i = from; i < to; i++)
  {
    if (planes[(u64)i * nBands].head.flags) continue;    // (folded above: flagged as a whole or not at all)
    u64 size = 0;
    for (u32 k = 0; k < nBands; k++) size += planes[(u64)i * nBands + k].head.blobSize;
    const u64 base = slotBytes ? (firstTile + i) * slotBytes : run;
    run += (size + 15ull) & ~15ull;
    if (!slotBytes && base + size > arenaCapacity) { flagAll(i, kTbArenaFull, kTbArenaFull); continue; }
    u64 at = base;
    for (u32 k = 0; k < nBands; k++) { TileBatchRec& r = planes[(u64)i * nBands + k].head; r.offset = at; at += r.blobSize; }
  }
}

// ---- the codec 6 header (Lerc2.cpp:724-786), 90 bytes
static const u32 kHdr6 = 90;    // headerBytes(6), codec_common.cpp

struct TbHeader6
{
  int version;
  u32 checksum;
  int nRows, nCols, nDepth, numValid, microBlockSize, blobSize, dt, nBlobsMore;
  u32 flagBytes;          // passNoData, isInt, two reserved bytes
  double maxZErr, zMin, zMax;
};

// false: not the magic.  Which values a batch takes is its parse kernel's business.
__device__ __forceinline__ bool tbReadHeader6(const u8* __restrict__ blob, TbHeader6& h)
{
  const char magic[6] = { 'L', 'e', 'r', 'c', '2', ' ' };
  bool ok = true;
  for (int i = 0; i < 6; i++) if (blob[i] != (u8)magic[i]) ok = false;
  int ints[10];
  for (int i = 0; i < 10; i++) ints[i] = (int)(u32)getBytes(blob + 6 + 4 * i, 4);
  double dbl[3];
  for (int i = 0; i < 3; i++) { const u64 bits = getBytes(blob + 50 + 8 * i, 8); memcpy(&dbl[i], &bits, 8); }
  h.version = ints[0]; h.checksum = (u32)ints[1]; h.nRows = ints[2]; h.nCols = ints[3]; h.nDepth = ints[4]; h.numValid = ints[5];
  h.microBlockSize = ints[6]; h.blobSize = ints[7]; h.dt = ints[8]; h.nBlobsMore = ints[9];
  h.flagBytes = (u32)getBytes(blob + 46, 4);
  h.maxZErr = dbl[0]; h.zMin = dbl[1]; h.zMax = dbl[2];
  return ok;
}

// (no noData values; the checksum's field is patched once the blob is finished: tbWriteChecksum)
__device__ __forceinline__ void tbWriteHeader6(u8* out, const TbHeader6& h)
{
  const char magic[6] = { 'L', 'e', 'r', 'c', '2', ' ' };
  for (int i = 0; i < 6; i++) out[i] = (u8)magic[i];
  const int ints[10] = { h.version, (int)h.checksum, h.nRows, h.nCols, h.nDepth, h.numValid, h.microBlockSize, h.blobSize, h.dt, h.nBlobsMore };
  for (int i = 0; i < 10; i++) putBytes(out + 6 + 4 * i, (u64)(u32)ints[i], 4);
  putBytes(out + 46, (u64)h.flagBytes, 4);
  const double dbl[5] = { h.maxZErr, h.zMin, h.zMax, 0.0, 0.0 };
  for (int i = 0; i < 5; i++) { u64 bits; memcpy(&bits, &dbl[i], 8); putBytes(out + 50 + 8 * i, bits, 8); }
}

// ---- band stacks, decode: a thread per tile walks the chain of band blobs -- band k + 1 begins where band k's header says band k
// ends; every header names the stack's shape and type and the number of blobs behind it; the sizes add up to the tile's.  -> the
// planes' places for the plane-parallel kernels; a chain that does not hold leaves sizes of 0, which the parse kernels refuse plane
// by plane.  G: a family's geometry (TileGeom's nRows, nCols, dt)
template<class G>
__device__ __forceinline__ void tbBandChain(const G& g, u32 nTiles, u32 nBands, const u8* __restrict__ arena, const u64* __restrict__ offsets,
                                            const u32* __restrict__ sizes, u64* __restrict__ planeOff, u32* __restrict__ planeSize)
{
  const u32 t = blockIdx.x * 256u + threadIdx.x;
  if (t >= nTiles) return;
  const u64 base = offsets[t];
  const u32 total = sizes[t];
  u32 at = 0;
  bool ok = true;
  for (u32 k = 0; k < nBands && ok; k++)
  {
    if (total - at < kHdr6 + 4u) { ok = false; break; }
    TbHeader6 h;
    ok = tbReadHeader6(arena + base + at, h) && h.version == kCodecVersion && h.nRows == g.nRows && h.nCols == g.nCols && h.nDepth == 1 && h.dt == g.dt
      && h.nBlobsMore == (int)(nBands - 1u - k) && h.blobSize >= (int)(kHdr6 + 4u) && (u32)h.blobSize <= total - at;
    if (!ok) break;
    planeOff[(u64)t * nBands + k] = base + at;
    planeSize[(u64)t * nBands + k] = (u32)h.blobSize;
    at += (u32)h.blobSize;
  }
  if (ok && at != total) ok = false;
  if (!ok) for (u32 k = 0; k < nBands; k++) { planeOff[(u64)t * nBands + k] = base; planeSize[(u64)t * nBands + k] = 0u; }
}

// ---- a tile's mask, by the workgroup that owns the tile (masked batches of any pixel type)
// byte mask -> bit mask (BitMask's layout: most significant bit first) into LDS (nBytes + 16 bytes, the last 16 zero) and into global
// memory; f(k) is called for every valid pixel k.  -> this thread's count of valid pixels.  (No barrier: the caller's comes next.)
template<class F>
__device__ __forceinline__ u32 tbMaskToBits(const u8* __restrict__ vb, u32 nPix, u8* s_bits, u8* __restrict__ bitsOut, F f)
{
  const u32 nBytes = (nPix + 7u) >> 3;
  u32 cnt = 0;
  for (u32 by = threadIdx.x; by < nBytes; by += 256u)
  {
    u32 m = 0;
    for (u32 j = 0; j < 8u; j++)
    {
      const u32 k = 8u * by + j;
      if (k >= nPix) { m |= 0x80u >> j; continue; }    // tail bits stay set, like BitMask::SetAllValid + SetInvalid (Lerc.cpp:959-975)
      if (vb[k] == 0) continue;
      m |= 0x80u >> j;
      cnt++;
      f(k);
    }
    s_bits[by] = (u8)m;
    bitsOut[by] = (u8)m;
  }
  for (u32 by = nBytes + threadIdx.x; by < nBytes + 16u; by += 256u) s_bits[by] = 0;
  return cnt;
}

// the mask's run-length stream by ONE thread out of LDS (RLE.cpp:123-254, the same bytes as rleEncode, codec_common.cpp):
// [int16 n][payload] ..., n > 0 literal bytes, n < 0 one byte -n times, -32768 ends it; a run is opened only where at least 5 equal
// bytes start and one more byte follows; segments are cut at 32767.  -> the stream's length, 0: it outgrew cap
__device__ __forceinline__ u32 tbMaskRle(const u8* s_bits, u32 n, u8* __restrict__ out, u32 cap)
{
  u32 at = 0, i = 0;
  bool fits = true;
  while (i < n && fits)
  {
    const u32 litBeg = i;
    while (i < n)
    {
      const bool runStarts = (i + 5 < n) && s_bits[i] == s_bits[i + 1] && s_bits[i] == s_bits[i + 2] && s_bits[i] == s_bits[i + 3] && s_bits[i] == s_bits[i + 4];
      if (runStarts) break;
      i++;
    }
    for (u32 p = litBeg; p < i && fits;)
    {
      const u32 len = min(32767u, i - p);
      if (at + 2u + len + 8u > cap) { fits = false; break; }
      out[at] = (u8)(len & 255u); out[at + 1] = (u8)(len >> 8); at += 2;
      for (u32 q = 0; q < len; q++) out[at + q] = s_bits[p + q];
      at += len; p += len;
    }
    if (i >= n || !fits) break;
    u32 e = i;
    while (e + 1 < n && s_bits[e + 1] == s_bits[i]) e++;
    for (u32 left = e - i + 1; left > 0 && fits;)
    {
      const u32 len = min(32767u, left);
      if (at + 3u + 8u > cap) { fits = false; break; }
      const u32 neg = (u32)(-(int)len) & 0xFFFFu;
      out[at] = (u8)(neg & 255u); out[at + 1] = (u8)(neg >> 8); out[at + 2] = s_bits[i]; at += 3;
      left -= len;
    }
    i = e + 1;
  }
  if (!fits || at + 2u > cap) return 0u;
  out[at] = 0x00; out[at + 1] = 0x80;
  return at + 2u;
}

// the run-length stream src[0 .. nm) expanded into s_bits[0 .. nBytes) by ONE thread (rleDecode, codec_common.cpp: what it does not
// fill stays as it is), bounded by the section's length and the mask's size.  -> false: the stream is damaged
__device__ __forceinline__ bool tbMaskUnrle(const u8* __restrict__ src, u32 nm, u8* s_bits, u32 nBytes)
{
  u32 left = nm, at = 0, sp = 0;
  for (;;)
  {
    if (left < 2u) return false;
    const int cnt = (int)(short)(u16)(src[sp] | (src[sp + 1] << 8));
    sp += 2; left -= 2;
    if (cnt == -32768) return true;
    const u32 n = (u32)(cnt < 0 ? -cnt : cnt), payload = cnt > 0 ? n : 1u;
    if (left < payload + 2u || at + n > nBytes) return false;    // + 2: a count always follows (RLE.cpp:310)
    if (cnt > 0) for (u32 k = 0; k < n; k++) s_bits[at + k] = src[sp + k];
    else { const u8 v = src[sp]; for (u32 k = 0; k < n; k++) s_bits[at + k] = v; }
    at += n; sp += payload; left -= payload;
  }
}

// The pixels of a tile in row order, the valid ones with their rank among the valid ones, by one workgroup of 256 threads: a thread
// takes a byte of the bit mask (8 pixels) a round, a round's popcounts are scanned over the workgroup.  f(pixel, valid, rank) is
// called once for every pixel below nPix (the tail bits of an encoder's mask are set: they do not count).  s: 4 words of LDS.
template<class F>
__device__ __forceinline__ u32 tbRankedSweep(const u8* bits, u32 nPix, u32* s, F f)
{
  const u32 nBytes = (nPix + 7u) >> 3;
  u32 run = 0;
  for (u32 base = 0; base < nBytes; base += 256u)
  {
    const u32 by = base + threadIdx.x;
    u32 m = by < nBytes ? (u32)bits[by] : 0u;
    if (8u * by + 8u > nPix) m &= (8u * by < nPix) ? (0xFF00u >> (nPix - 8u * by)) & 0xFFu : 0u;
    const u32 c = (u32)__popc(m), inc = waveInclusiveScan(c);
    if (laneId() == 63) s[waveId()] = inc;
    __syncthreads();
    u32 r = run + inc - c;
    for (int w = 0; w < waveId(); w++) r += s[w];
    run += s[0] + s[1] + s[2] + s[3];
    for (u32 j = 0; j < 8u && 8u * by + j < nPix; j++)
    {
      const bool valid = (m & (0x80u >> j)) != 0u;
      f(8u * by + j, valid, r);
      r += valid ? 1u : 0u;
    }
    __syncthreads();
  }
  return run;
}

// the mask's own count of valid pixels below nPix, by the workgroup (s: 4 words of LDS)
__device__ __forceinline__ u32 tbMaskCount(const u8* s_bits, u32 nPix, u64* s)
{
  const u32 nBytes = (nPix + 7u) >> 3;
  u32 cnt = 0;
  for (u32 by = threadIdx.x; by < nBytes; by += 256u)
  {
    u32 m = s_bits[by];
    if (8u * by + 8u > nPix) m &= (0xFF00u >> (nPix - 8u * by)) & 0xFFu;
    cnt += (u32)__popc(m);
  }
  return (u32)blockSum((u64)cnt, s);
}

// valid pixels per MB x MB block out of the bit mask in LDS, nv[pos] (at most 256 each); no barrier behind it
__device__ __forceinline__ void tbBlockValidCounts(const u8* s_bits, u32 nRows, u32 nCols, u32 MB, u16* nv)
{
  const u32 nTV = (nRows + MB - 1u) / MB, nTH = (nCols + MB - 1u) / MB, nPos = nTV * nTH;
  for (u32 pos = threadIdx.x; pos < nPos; pos += 256u)
  {
    const u32 it = pos / nTH, jt = pos - it * nTH;
    const u32 i1 = min(nRows, it * MB + MB), j1 = min(nCols, jt * MB + MB);
    u32 n = 0;
    for (u32 i = it * MB; i < i1; i++)
      for (u32 j = jt * MB; j < j1; j++) { const u32 k = i * nCols + j; n += (s_bits[k >> 3] >> (7u - (k & 7u))) & 1u; }
    nv[pos] = (u16)n;
  }
}

// header (checksum patched later: tbWriteChecksum) and mask section -- the stream's length and the stream -- of a tile of any kind,
// by the workgroup.  s_hdr: 96 bytes of LDS.
__device__ __forceinline__ void tbWriteHeaderMask(u8* __restrict__ blob, const TbHeader6& h, const u8* __restrict__ rle, u32 rleLen, u8* s_hdr)
{
  if (threadIdx.x == 0)
  {
    tbWriteHeader6(s_hdr, h);
    putBytes(s_hdr + kHdr6, (u64)rleLen, 4);
  }
  __syncthreads();
  for (u32 i = threadIdx.x; i < kHdr6 + 4u; i += 256u) blob[i] = s_hdr[i];
  for (u32 i = threadIdx.x; i < rleLen; i += 256u) blob[kHdr6 + 4u + i] = rle[i];
}

// ---- the walk over a tile's block stream by ONE thread: block k + 1 starts where block k ends; a block's length follows from its
// header and its count of valid pixels, nValidOf(k, elements of block k).  table[k]: where block k begins, table[nPos]: where the
// last one ends.  p: tbFillBandParams(g, MB).  -> 0 or kTbBlocks
template<int TBYTES, u32 MB, class NV>
__device__ __forceinline__ u32 tbWalkBlocks(const u8* __restrict__ blob, u32 begin, u32 blobEnd, const BandParams& p, u32* __restrict__ table, NV nValidOf)
{
  const u32 nTH = (u32)p.nTH, nPos = (u32)(p.nTV * p.nTH);
  const u32 pattern = 14u;    // codec >= 5: bit 2 of the flag is the difference flag
  u32 pos = begin, fl = 0;
  for (u32 k = 0; k < nPos; k++)
  {
    table[k] = pos;
    const u32 it = k / nTH, jt = k - it * nTH;
    const u32 nElem = min(MB, (u32)p.nRows - it * MB) * min(MB, (u32)p.nCols - jt * MB);
    const int nv = nValidOf(k, nElem);
    BlkInfo bi;
    const int rc = parseBlock<TBYTES>(blob, pos, blobEnd, p, nv, nElem, bi);
    // (a block of a position without valid pixels is the one "all zero" byte)
    if (rc != 0 || bi.len == 0 || (((u32)bi.flag >> 2) & pattern) != (((jt * MB) >> 3) & pattern) || bi.diff || (nv == 0 && bi.mode != 2)) { fl = kTbBlocks; break; }
    pos += bi.len;
  }
  if (!fl && pos != blobEnd) fl = kTbBlocks;
  table[nPos] = pos;
  return fl;
}

// ---- the block encoder's wave body for one value a pixel and a tile of a batch: the stages of tile_encode_dev.h.  The wave owns block
// pos of the tile px (p: the tile's nRows, nCols, nTH, block size, error bound).
// MASKED: maskBits says which pixels are valid unless p.allValid, and the error bound may be any; else every pixel is valid and the
// tile lossless (p.maxZErr 0.5, p.intLossless).  WRITE: the block's bytes go to data + table[pos] (data: where the tile's block stream
// begins); else its size goes to table[pos].  LDS of the wave: valBuf E * 64 values; WRITE: obuf (1 + E * 64 * sizeof(T) + 3) / 4 + 4
// words, lutBuf E * 64 words.
template<class T, int E, bool MASKED, bool WRITE>
__device__ __forceinline__ void tbEncodeBlock(const BandParams& p, int pos, const T* __restrict__ px, const u8* __restrict__ maskBits,
                                              u32* __restrict__ table, u8* __restrict__ data, T* valBuf, u32* obuf, u32* lutBuf)
{
  const int lane = laneId();
  const BlockLanes<E> L = blockLanes<E, MASKED>(p, pos, maskBits);
  if (MASKED && L.n == 0)
  {
    if (WRITE) { if (lane == 0) data[table[pos]] = emptyBlockByte(p, L.j0); }
    else if (lane == 0) table[pos] = 1u;
    return;
  }
  T v[E];
  gatherSlice<T, E>(L, px, 1, 0, valBuf, v);
  const SliceCode<T, E> s = analyseSlice<T, E>(p, L.n, v, L.rank, valBuf, p.dt, !MASKED || p.allValid, !MASKED || p.maxZErr > 0, !MASKED || p.intLossless);
  if (!WRITE) { if (lane == 0) table[pos] = (u32)s.plan.nBytes; return; }

  composeBlock<T, E>(obuf, lutBuf, p, s.plan, L.n, L.j0, false, s.zMin, v, s.q, L.rank, s.qMax);
  const u8* ob8 = reinterpret_cast<const u8*>(obuf);
  u8* __restrict__ dst = data + table[pos];
  for (int i = lane; i < s.plan.nBytes; i += 64) dst[i] = ob8[i];
}

// ---- the block decoder's wave body: k_decode_tiles (tile_decode.hip) for one value a pixel and a tile of a batch.  The wave owns block
// pos, which begins at blob + off; p: the tile's nRows, nCols, nTH, block size, invScale, version; zMax: the header's.  MASKED: as
// above; pixels of the block that are not valid are written as 0.  LDS of the wave: lut 256 words, head 64 bytes (16-byte aligned).
// -> true: the block cannot be decoded (the caller raises kTbSibling)
template<class T, int E, bool MASKED>
__device__ __forceinline__ bool tbDecodeBlock(const BandParams& p, double zMax, int pos, const u8* __restrict__ blob, u32 blobEnd, u32 off,
                                              const u8* __restrict__ maskBits, T* __restrict__ out, u32* lut, u8* head)
{
  constexpr int MB = E == 1 ? 8 : 16;
  const int lane = laneId();
  const int it = pos / p.nTH, jt = pos - it * p.nTH;
  const int i0 = it * MB, j0 = jt * MB;
  const int tileH = min(MB, p.nRows - i0), tileW = min(MB, p.nCols - j0);
  const int nElem = tileH * tileW;

  int rank[E];
  i64 px[E];
  int nValid = MASKED ? 0 : nElem;
#pragma unroll
  for (int k = 0; k < E; k++)
  {
    const int e = k * 64 + lane;
    const bool inb = e < nElem;
    const int r = inb ? e / tileW : 0, c = inb ? e - r * tileW : 0;
    px[k] = inb ? (i64)(i0 + r) * p.nCols + (j0 + c) : -1;
    if (MASKED)
    {
      const bool valid = inb && (p.allValid || maskBit(maskBits, px[k]));
      const u64 bal = __ballot(valid);
      rank[k] = valid ? nValid + __popcll(bal & laneMaskLt()) : -1;
      nValid += __popcll(bal);
    }
    else rank[k] = inb ? e : -1;
  }

  head[lane] = ((u64)off + (u64)lane < (u64)blobEnd) ? blob[(u64)off + lane] : (u8)0;
  waveSync();
  BlkInfo bi;
  const int rc = (off < blobEnd) ? parseBlockWords<(int)sizeof(T)>(reinterpret_cast<const u32*>(head), 0u, blobEnd - off, p, nValid, (u32)nElem, bi) : 1;
  bool failed = rc != 0 || (((u32)bi.flag >> 2) & 14u) != (((u32)j0 >> 3) & 14u) || bi.diff;
  if (!failed)
  {
    double offset = 0;
    if (bi.mode == 1 || bi.mode == 3) offset = typedFromBits(getBytes(head + 1, bi.offBytes), bi.dtUsed);
    const u64 payloadBit = 8ull * ((u64)off + bi.payload);
    const int nbIdx = bi.lut ? bitLen(bi.nLut) : 0;
    u64 idxBit = 0;
    if (bi.mode == 1 && bi.lut)
    {
      lut[0] = 0;
      for (u32 i = (u32)lane; i < bi.nLut; i += 64) lut[i + 1] = unstuffElement(blob, payloadBit, i, bi.nb, bi.nLut, blobEnd, p.version);
      idxBit = payloadBit + 8ull * (((u64)bi.nLut * bi.nb + 7) >> 3);
      waveSync();
    }
    bool badIdx = false;
#pragma unroll
    for (int k = 0; k < E; k++)
    {
      T val = T(0);
      if (rank[k] >= 0)
      {
        if (bi.mode == 2) val = T(0);
        else if (bi.mode == 0)
        {
          const u64 bits = getBytes(blob + off + 1 + (u64)rank[k] * sizeof(T), (int)sizeof(T));
          memcpy(&val, &bits, sizeof(T));
        }
        else if (bi.mode == 3) val = (T)offset;
        else
        {
          u32 q;
          if (!bi.lut) q = unstuffElement(blob, payloadBit, (u32)rank[k], bi.nb, bi.cnt, blobEnd, p.version);
          else
          {
            const u32 ix = unstuffElement(blob, idxBit, (u32)rank[k], nbIdx, bi.cnt, blobEnd, p.version);
            if (ix > bi.nLut) { badIdx = true; q = 0; } else q = lut[ix];
          }
          const double z = offset + (double)q * p.invScale;
          val = (T)(z < zMax ? z : zMax);    // std::min(z, zMax)
        }
      }
      if (px[k] >= 0) out[px[k]] = val;
    }
    failed = __any(badIdx);
  }
  return failed;
}

}    // namespace lerc
