// tile_byte_batch.hip -- batches of 8-BIT tiles (DT_Char / DT_Byte, every pixel valid, lossless): nTiles rasters of one shape encoded into
// (decoded from) nTiles independent Lerc2 blobs by ONE set of launches, a tile per workgroup -- no launch, no copy and no host wait per
// tile, and the Huffman code book of every tile built on the device.
//
// Encode (launchTbbEncode):
//   1. k_tbb_stats     a workgroup per tile: the plain and the delta histogram of Lerc2::ComputeHistoForHuffman (Lerc2.cpp:2311-2380, all
//                      valid: the predecessor is the left neighbour, the pixel above in column 0, 0 at the origin) in LDS; the range
//                      follows from the plain one
//   2. k_tbb_blocks<false>   a wave per 8 x 8 block: the block's size (the general encoder's decisions, tile_encode.hip)
//   3. k_tbb_decide    a workgroup per tile: the sizes' exclusive scan; two threads build the two code books (Huffman::ComputeCodes,
//                      Huffman.cpp:35-81, with std::priority_queue's heap discipline restated: tbbBuildBook), their canonical codes, index
//                      range, serialised table and compressed size; then the mode (Lerc2.cpp:2289-2306, :285-360), the blob's size, the
//                      slot check.   k_tbb_arena: one workgroup places the blobs in a packed arena (16-byte aligned)
//   4. k_tbb_blocks<true>    tiling mode tiles: the blocks' bytes
//   5. k_tbb_write     a workgroup per tile: header, mask section, ranges, "not one sweep", mode byte; Huffman modes: the table and the
//                      pixel stream -- 4096 pixels a step, 16 a thread: code lengths summed, scanned over the workgroup, the code words
//                      put together in LDS and stored as whole words -- and its padding words
//   6. k_tbb_checksum  a workgroup per tile: Fletcher32 over blob[14 ..), stored into the header
// Tiles whose outcome is decided elsewhere (TbbTile::flags) are left alone; the host encodes them one by one behind the batch.
//
// Decode (launchTbbDecode):
//   1. k_tbbd_parse    a workgroup per tile: header, Fletcher32, mode byte; tiling mode: the walk over the block headers; Huffman modes:
//                      the code table with parseTable's checks (huffman_host.cpp)
//   2. k_tbbd_blocks   tiling mode tiles, a wave per block: the general decoder's block (tile_decode.hip)
//   3. k_tbbd_huff     Huffman mode tiles, a workgroup per tile: the look-up table in LDS, the stream staged in LDS where it fits, 256
//                      self-synchronising sub-sequences (huffman_kernels.hip: k_huff_sync) whose starts are corrected inside the workgroup
//                      until every one begins where the one in front ended, the symbols stored, the predictor undone (column 0 by a
//                      scan over the rows, then every row by a wave)
// Every loop over a blob is bounded by the blob's size and the pixel count; whatever does not fit raises a flag and the host repeats
// that tile with the single-blob decoder, which also yields the exact status of a damaged blob.
// No workgroup waits for another one inside a launch, so the emulator build runs the same path.
//
// MASKED (a template argument of the kernels above; the masked calls with 8-bit tiles): a byte mask per tile.  k_tbb_stats makes bit
// mask, valid count and the mask's run-length stream first (tile_batch_dev.h, shared with tile_mask_batch.hip), the histograms count
// valid pixels only with the masked predictor (Lerc2.cpp:2350-2379), the blocks are the masked block coder's, the decisions take the
// valid count, k_tbb_blocks16 / k_tbb_decide16 settle the low-bit-rate retry, k_tbb_write puts the mask section in front and codes an
// invalid pixel with length 0; k_tbbd_parse expands and checks the mask, k_tbbd_huff wants numValid code words, sends them to the
// valid positions by rank and undoes the masked predictor row by row.  Tiles without a valid pixel stay inside.
//
// BANDS (a second template argument of k_tbb_stats, k_tbb_write and k_tbbd_parse, MASKED form only; launchTbbEncodeBands /
// launchTbbDecodeBands): tiles that are band stacks, the unit a plane (tile * nBands + band).  A tile's planes share its mask; band 0
// writes the mask section, the bands behind it the count 0; every header names the band blobs behind it.  k_tbb_place_bands gives a
// tile the sum of its planes' sizes and each plane the running sum inside it -- a band begins at any byte --, and sends a tile with a
// flagged plane back whole; k_tbbd_chain finds the planes of a tile's blob by the headers' sizes.
#include <cstdio>
#include <cstdlib>
#include "kernels.h"
#include "wave_utils.h"
#include "huffman_dev.h"
#include "tile_byte_batch.h"
#include "tile_batch_dev.h"

namespace lerc {

// histogram bin of a raw byte: value + 128 for DT_Char (Lerc2.cpp:2320), the value itself for DT_Byte
template<class T> __device__ __forceinline__ u32 tbbBin(u32 raw) { return (DtOf<T>::v == DT_Char) ? (raw ^ 0x80u) & 255u : raw & 255u; }

// the predictor's difference at pixel k, as a raw byte
__device__ __forceinline__ u32 tbbDelta(const u8* __restrict__ px, u32 k, u32 nCols)
{
  const u32 i = k / nCols, j = k - i * nCols;
  const u32 pred = j > 0u ? px[k - 1u] : (i > 0u ? px[k - nCols] : 0u);
  return ((u32)px[k] - pred) & 255u;
}

// ---- the masked predictor (Lerc2.cpp:2350-2379): only valid pixels count; the predecessor of valid pixel k is its left neighbour if
// that is valid (never across a row's start), else the pixel above if that is valid, else the last valid pixel in scan order,
// however far back (0 in front of the first).  "The last valid pixel below k" is asked of the bit mask: inside k's word of 32
// pixels a bit scan, else the last non-empty word below it -- a table made once per tile.
struct TbbmMask
{
  // the tile's bit mask (BitMask's layout: most significant bit first) in LDS, 16 zero bytes behind it -- or, k_tbb_write's large form,
  // where it lies in the workspace, its last word of 32 pixels padded with zero bytes (k_tbb_stats)
  const u8* bits;
  const u16* last;        // last[w]: 1 + the last word below w with a valid pixel in it, 0: none
  __device__ __forceinline__ u32 word(u32 w) const
  {
    const u8* q = bits + 4u * w;
    return ((u32)q[0] << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | (u32)q[3];
  }
  __device__ __forceinline__ bool valid(u32 k) const { return ((bits[k >> 3] >> (7u - (k & 7u))) & 1u) != 0u; }
  __device__ __forceinline__ int prev(u32 k) const    // -1: none
  {
    u32 w = k >> 5;
    u32 x = word(w) & ~(0xFFFFFFFFu >> (k & 31u));    // pixel w * 32 + i is bit 31 - i
    if (!x)
    {
      const u32 lw = last[w];
      if (!lw) return -1;
      w = lw - 1u;
      x = word(w);
    }
    return (int)((w << 5) + 32u - (u32)__ffs((int)x));
  }
};

// TbbmMask::last out of the bit mask in LDS (complete, behind a barrier), by the workgroup; s_scan: 256 words; a barrier ends it
__device__ __forceinline__ void tbbmLastWords(const u8* s_bits, u32 nPix, u16* s_last, u32* s_scan)
{
  const TbbmMask m = { s_bits, s_last };
  const u32 nW = (nPix + 31u) >> 5, per = (nW + 255u) / 256u, from = min(nW, threadIdx.x * per), to = min(nW, from + per);
  u32 last = 0;
  for (u32 w = from; w < to; w++) if (m.word(w)) last = w + 1u;
  s_scan[threadIdx.x] = last;
  __syncthreads();
  if (threadIdx.x == 0) { u32 run = 0; for (u32 i = 0; i < 256u; i++) { const u32 y = s_scan[i]; s_scan[i] = run; run = max(run, y); } }
  __syncthreads();
  u32 run = s_scan[threadIdx.x];
  for (u32 w = from; w < to; w++) { s_last[w] = (u16)run; if (m.word(w)) run = w + 1u; }
  __syncthreads();
}

// the masked predictor's difference at VALID pixel k, as a raw byte
__device__ __forceinline__ u32 tbbmDelta(const u8* __restrict__ px, const TbbmMask& m, u32 k, u32 nCols)
{
  const u32 i = k / nCols, j = k - i * nCols;
  u32 pred = 0;
  if (j > 0u && m.valid(k - 1u)) pred = px[k - 1u];
  else if (i > 0u && m.valid(k - nCols)) pred = px[k - nCols];
  else { const int kp = m.prev(k); if (kp >= 0) pred = px[kp]; }
  return ((u32)px[k] - pred) & 255u;
}

// ================================================================================================
// encode
// ================================================================================================
// MASKED: in front of the histograms the masked batch's prelude (tile_batch_dev.h) -- byte mask -> bit mask, the count of valid pixels,
// the mask's run-length stream by one lane -- and the histograms over valid pixels only
// BANDS (MASKED only): t is a plane, tile * nBands + band (tile_byte_batch.h); the tile's mask lies at b.m.valid + tile * validStride,
// and only band 0 makes the mask's run-length stream -- the bands behind it write the count 0
// LARGE (MASKED only): the form for tiles beyond the small form's mask bytes (tile_batch.h: TbForm), picked by the host from the shape
template<class T, bool MASKED, bool BANDS = false, bool LARGE = false>
__global__ void __launch_bounds__(256) k_tbb_stats(TbbGeom g, const u8* __restrict__ data, TbbEncodeBuffers b, u32 nBands, u64 validStride)
{
  __shared__ u32 s_h[512];
  __shared__ u32 s_mn[4], s_mx[4];
  const u32 t = blockIdx.x;
  const u32 nPix = (u32)g.tileElems, nCols = (u32)g.nCols;
  const u8* __restrict__ px = data + (u64)t * g.tileElems;
  s_h[threadIdx.x] = 0; s_h[threadIdx.x + 256u] = 0;
  u32 numValid = nPix, rleFlag = 0;
  if constexpr (MASKED)
  {
    __shared__ __align__(16) u8 s_bits[TbForm<LARGE>::kMaskBytes + 16];
    __shared__ u16 s_last[TbForm<LARGE>::kMaskWords];
    __shared__ u32 s_scan[256];
    __shared__ u64 s_red[4];
    const u8* __restrict__ vb = BANDS ? b.m.valid + (u64)(t / nBands) * validStride : b.m.valid + (u64)t * g.tileElems;
    const u32 cnt = tbMaskToBits(vb, nPix, s_bits, b.m.bits + (u64)t * b.m.bitStride, [](u32) {});
    // (k_tbb_write's large form reads the mask as words of 32 pixels where it lies: the last word's bytes behind the mask are zero)
    if (LARGE && threadIdx.x < 4u) b.m.bits[(u64)t * b.m.bitStride + ((nPix + 7u) >> 3) + threadIdx.x] = 0;
    numValid = (u32)blockSum((u64)cnt, s_red);    // (its barriers cover s_h and s_bits)
    if (threadIdx.x == 0)
    {
      TbbMaskRec mr = { numValid, 0u };
      if (numValid > 0u && numValid < nPix && (!BANDS || t % nBands == 0u))
      {
        mr.rleLen = tbMaskRle(s_bits, (nPix + 7u) >> 3, b.m.rle + (u64)t * b.m.rleStride, b.m.rleStride);
        if (!mr.rleLen) rleFlag = kTbbRle;
      }
      b.m.rec[t] = mr;
    }
    tbbmLastWords(s_bits, nPix, s_last, s_scan);
    const TbbmMask m = { s_bits, s_last };
    for (u32 k = threadIdx.x; k < nPix; k += 256u)
    {
      if (!m.valid(k)) continue;
      atomicAdd(&s_h[tbbBin<T>(px[k])], 1u);
      atomicAdd(&s_h[256u + tbbBin<T>(tbbmDelta(px, m, k, nCols))], 1u);
    }
  }
  else
  {
    __syncthreads();
    for (u32 k = threadIdx.x; k < nPix; k += 256u)
    {
      atomicAdd(&s_h[tbbBin<T>(px[k])], 1u);
      atomicAdd(&s_h[256u + tbbBin<T>(tbbDelta(px, k, nCols))], 1u);
    }
  }
  __syncthreads();
  u32* __restrict__ out = b.histo + (u64)t * 512u;
  out[threadIdx.x] = s_h[threadIdx.x]; out[threadIdx.x + 256u] = s_h[threadIdx.x + 256u];
  const bool used = s_h[threadIdx.x] != 0u;
  const u32 mn = waveMin(used ? threadIdx.x : 255u), mx = waveMax(used ? threadIdx.x : 0u);
  if (laneId() == 0) { s_mn[waveId()] = mn; s_mx[waveId()] = mx; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  TbbTile ti;
  memset(&ti, 0, sizeof(ti));
  ti.symMin = min(min(s_mn[0], s_mn[1]), min(s_mn[2], s_mn[3]));
  ti.symMax = max(max(s_mx[0], s_mx[1]), max(s_mx[2], s_mx[3]));
  ti.head.flags = (ti.symMin == ti.symMax) ? kTbbConst : 0u;
  if (MASKED && numValid == 0u) { ti.head.flags = 0u; ti.mode = kTbbModeEmpty; }    // (header and mask section are all of it: Lerc2.cpp:240)
  if (MASKED && rleFlag) ti.head.flags = rleFlag;
  b.tiles[t] = ti;
}

// A wave per 8 x 8 block of a tile (blockIdx.y): k_encode_tiles (tile_encode.hip) for one value a pixel, every pixel valid, with the
// tile's own place in the arena.  WRITE: tiling mode tiles only.  MASKED: the masked block coder with the tile's bit mask.
template<class T, bool WRITE, bool MASKED>
__global__ void __launch_bounds__(256)
k_tbb_blocks(TbbGeom g, BandParams p, const T* __restrict__ data, u8* __restrict__ arena, TbbEncodeBuffers b)
{
  constexpr int NMAX = 64;
  constexpr int OBW = (1 + NMAX * (int)sizeof(T) + 3) / 4 + 4;
  __shared__ T s_val[4][NMAX];
  __shared__ u32 s_obuf[4][WRITE ? OBW : 1];
  __shared__ u32 s_lut[4][WRITE ? NMAX : 1];
  const u32 t = blockIdx.y;
  const TbbTile ti = b.tiles[t];
  if (ti.head.flags || (WRITE && ti.mode != (u32)IEM_Tiling)) return;
  if (MASKED && ti.mode == kTbbModeEmpty) return;
  const int w = waveId();
  const int pos = (int)blockIdx.x * 4 + w;
  if (pos >= g.nTV * g.nTH) return;    // whole wave leaves together
  if constexpr (MASKED)
  {
    const TbbMaskRec mr = b.m.rec[t];
    p.allValid = (mr.numValid == (u32)g.tileElems) ? 1 : 0;
    tbEncodeBlock<T, 1, true, WRITE>(p, pos, data + (u64)t * g.tileElems, b.m.bits + (u64)t * b.m.bitStride, b.blockOff + (u64)t * g.posStride,
                                     WRITE ? arena + ti.head.offset + kTbbDataBegin + mr.rleLen : nullptr, s_val[w], s_obuf[w], s_lut[w]);
  }
  else
    tbEncodeBlock<T, 1, false, WRITE>(p, pos, data + (u64)t * g.tileElems, nullptr, b.blockOff + (u64)t * g.posStride,
                                      WRITE ? arena + ti.head.offset + kTbbDataBegin : nullptr, s_val[w], s_obuf[w], s_lut[w]);
}

// ---- a code book, built by ONE thread in LDS
struct TbbBook
{
  u32 heapW[256];         // the heap: symbol counts ...
  u16 heapNode[256];      // ... and the tree node each stands for
  u16 c0[512], c1[512];   // children of the inner nodes (nodes [0, nLeaves) are leaves, in symbol order)
  u8 depth[512];
  u8 leafSym[256];
  u8 len[256];
  u32 code[256];
  u32 start[33];
  u8 table[kTbbTableCap];
  u32 tableBytes, nBytes, ok;
  u64 nBits;
};

// std::priority_queue<HeapItem> with operator< on minus the count (huffman_host.cpp:22-27): comp(a, b) = a's count > b's count.
// std::push_heap: the new element sifts up from the end while comp(parent, value).
__device__ __forceinline__ void tbbHeapPush(TbbBook& k, int& n, u32 w, u32 node)
{
  int hole = n++;
  int parent = (hole - 1) / 2;
  while (hole > 0 && k.heapW[parent] > w)
  {
    k.heapW[hole] = k.heapW[parent]; k.heapNode[hole] = k.heapNode[parent];
    hole = parent;
    parent = (hole - 1) / 2;
  }
  k.heapW[hole] = w; k.heapNode[hole] = (u16)node;
}

// std::pop_heap + pop_back: the last element is taken out, the hole at the top sifts down to a leaf along the children that
// do NOT compare less (std::__adjust_heap), and the element then sifts up from there (std::__push_heap).
__device__ __forceinline__ void tbbHeapPop(TbbBook& k, int& n, u32& w, u32& node)
{
  w = k.heapW[0]; node = k.heapNode[0];
  n--;
  if (n < 1) return;
  const u32 vw = k.heapW[n];
  const u16 vn = k.heapNode[n];
  const int len = n;
  int hole = 0, child = 0;
  while (child < (len - 1) / 2)
  {
    child = 2 * (child + 1);
    if (k.heapW[child] > k.heapW[child - 1]) child--;    // comp(first[child], first[child - 1])
    k.heapW[hole] = k.heapW[child]; k.heapNode[hole] = k.heapNode[child];
    hole = child;
  }
  if ((len & 1) == 0 && child == (len - 2) / 2)
  {
    child = 2 * (child + 1);
    k.heapW[hole] = k.heapW[child - 1]; k.heapNode[hole] = k.heapNode[child - 1];
    hole = child - 1;
  }
  int parent = (hole - 1) / 2;
  while (hole > 0 && k.heapW[parent] > vw)
  {
    k.heapW[hole] = k.heapW[parent]; k.heapNode[hole] = k.heapNode[parent];
    hole = parent;
    parent = (hole - 1) / 2;
  }
  k.heapW[hole] = vw; k.heapNode[hole] = vn;
}

// buildCodes + codeRange + serialiseTable + compressedBytes of huffman_host.cpp for a 256-bin histogram
__device__ void tbbBuildBook(const u32* __restrict__ histo, TbbBook& k)
{
  k.ok = 0; k.tableBytes = 0; k.nBytes = 0; k.nBits = 0;
  int n = 0, nNodes = 0;
  for (int i = 0; i < 256; i++)
  {
    k.len[i] = 0; k.code[i] = 0;
    if (histo[i] > 0u) { k.leafSym[nNodes] = (u8)i; tbbHeapPush(k, n, histo[i], (u32)nNodes); nNodes++; }
  }
  const int nLeaves = nNodes;
  if (nLeaves < 2) return;
  while (n > 1)
  {
    u32 wa, na, wb, nb;
    tbbHeapPop(k, n, wa, na);
    tbbHeapPop(k, n, wb, nb);
    k.c0[nNodes] = (u16)na; k.c1[nNodes] = (u16)nb;
    tbbHeapPush(k, n, wa + wb, (u32)nNodes);
    nNodes++;
  }
  // depths: a node's children were made before it
  int maxLen = 0;
  k.depth[nNodes - 1] = 0;
  for (int m = nNodes - 1; m >= nLeaves; m--)
  {
    const int d = k.depth[m] + 1;
    if (d > 32) return;    // a code longer than 32 bits: no code book (Huffman.h:84-99)
    k.depth[k.c0[m]] = (u8)d; k.depth[k.c1[m]] = (u8)d;
  }
  for (int m = 0; m < nLeaves; m++) { k.len[k.leafSym[m]] = k.depth[m]; maxLen = max(maxLen, (int)k.depth[m]); }
  // canonical codes: longest first, ties by ascending symbol (Huffman.cpp:541-572)
  for (int l = 0; l <= 32; l++) k.start[l] = 0;
  for (int i = 0; i < 256; i++) if (k.len[i]) k.start[k.len[i]]++;
  {
    u32 code = 0;
    int cur = maxLen;
    for (int l = maxLen; l >= 1; l--)
    {
      const u32 cnt = k.start[l];
      if (!cnt) continue;
      code >>= (cur - l);
      cur = l;
      k.start[l] = code;
      code += cnt;
    }
  }
  for (int i = 0; i < 256; i++) if (k.len[i]) k.code[i] = k.start[k.len[i]]++;

  // the smallest (possibly wrapping) index range that covers the used symbols (Huffman.cpp:383-438)
  int i0 = 0, i1 = 0;
  {
    int i = 0;
    while (i < 256 && k.len[i] == 0) i++;
    i0 = i;
    i = 255;
    while (i >= 0 && k.len[i] == 0) i--;
    i1 = i + 1;
    int gapAt = 0, gapLen = 0;
    for (int j = 0; j < 256;)
    {
      while (j < 256 && k.len[j] > 0) j++;
      const int k0 = j;
      while (j < 256 && k.len[j] == 0) j++;
      if (j - k0 > gapLen) { gapAt = k0; gapLen = j - k0; }
    }
    if (256 - gapLen < i1 - i0) { i0 = gapAt + gapLen; i1 = gapAt + 256; }
    if (i1 <= i0) return;
  }
  // the table (Huffman.cpp:126-166): version, size, range; the lengths as a BitStuffer2 "simple" stream; the codes MSB first in words
  u8* out = k.table;
  const int hdr[4] = { 4, 256, i0, i1 };
  for (int i = 0; i < 4; i++) putBytes(out + 4 * i, (u64)(u32)hdr[i], 4);
  const u32 cnt = (u32)(i1 - i0);
  const int nb = bitLen((u32)maxLen), cb = countFieldBytes(cnt);
  u32 at = 16;
  out[at++] = (u8)(nb | (((cb == 4) ? 0 : 3 - cb) << 6));
  for (int i = 0; i < cb; i++) out[at++] = (u8)(cnt >> (8 * i));
  const u32 lenBytes = (cnt * (u32)nb + 7u) >> 3;
  for (u32 i = 0; i < lenBytes; i++) out[at + i] = 0;
  for (u32 i = 0; i < cnt; i++)
  {
    const int sym = i0 + (int)i - ((i0 + (int)i) < 256 ? 0 : 256);
    const u32 bit = i * (u32)nb;
    const u32 v = (u32)k.len[sym] << (bit & 7u);    // (six bits at most, shifted by seven at most)
    out[at + (bit >> 3)] |= (u8)v;
    if (v >> 8) out[at + (bit >> 3) + 1u] |= (u8)(v >> 8);
  }
  at += lenBytes;
  u32 cur = 0;
  int used = 0;
  for (int i = i0; i < i1; i++)
  {
    const int sym = i - (i < 256 ? 0 : 256);
    const int len = k.len[sym];
    if (!len) continue;
    const u32 v = k.code[sym];
    if (32 - used >= len)
    {
      cur |= (len == 32) ? v : (v << (32 - used - len));
      used += len;
      if (used == 32) { putBytes(out + at, (u64)cur, 4); at += 4; cur = 0; used = 0; }
    }
    else
    {
      const int rest = len - (32 - used);
      cur |= v >> rest;
      putBytes(out + at, (u64)cur, 4); at += 4;
      cur = v << (32 - rest);
      used = rest;
    }
  }
  if (used > 0) { putBytes(out + at, (u64)cur, 4); at += 4; }
  k.tableBytes = at;
  // Huffman::ComputeCompressedSize (Huffman.cpp:85-111)
  u64 bits = 0;
  for (int i = 0; i < 256; i++) bits += (u64)histo[i] * k.len[i];
  if (bits == 0 || bits > (u64)INT_MAX) return;    // the reference sums the bits in an int
  k.nBits = bits;
  k.nBytes = at + 4u * (u32)(((((bits + 7u) >> 3) + 3u) >> 2) + 1u);
  k.ok = 1;
}

// MASKED: the count of valid pixels where the all-valid code has the pixel count (Lerc2.cpp:331-364) -- but for the bit rate of the
// low-bit-rate rule, which counts every pixel (:335) --, and the mask section's length in the blob's size.  Where the low-bit-rate
// rule holds the tile is not handed back at once: with few valid pixels it holds for most Huffman tiles, and the 16 x 16 blocks
// then lose (:346).  The tile is marked, k_tbb_blocks16 sizes its 16 x 16 blocks, and k_tbb_decide16 hands it back only if they win.
template<bool MASKED>
__global__ void __launch_bounds__(256) k_tbb_decide(TbbGeom g, u64 slotBytes, u64 firstTile, TbbEncodeBuffers b)
{
  __shared__ u32 s_scan[257];
  __shared__ u32 s_h[512];
  __shared__ TbbBook s_book[2];
  __shared__ u32 s_pick;
  const u32 t = blockIdx.x;
  if (b.tiles[t].head.flags) return;
  if constexpr (MASKED)
    if (b.tiles[t].mode == kTbbModeEmpty)
    {
      if (threadIdx.x != 0) return;
      TbbTile& ti = b.tiles[t];
      ti.head.blobSize = kHdr6 + 4u;
      if (slotBytes)
      {
        ti.head.offset = (firstTile + t) * slotBytes;
        if ((u64)ti.head.blobSize > slotBytes) ti.head.flags = kTbCapacity;
      }
      return;
    }
  const u32 nPos = (u32)(g.nTV * g.nTH);
  const u32* __restrict__ histo = b.histo + (u64)t * 512u;
  s_h[threadIdx.x] = histo[threadIdx.x]; s_h[threadIdx.x + 256u] = histo[threadIdx.x + 256u];
  const u32 nBytesTiling = blockScanInPlace(b.blockOff + (u64)t * g.posStride, nPos, s_scan);    // (its barriers cover s_h)
  if (threadIdx.x == 0) tbbBuildBook(s_h, s_book[0]);
  if (threadIdx.x == 64) tbbBuildBook(s_h + 256, s_book[1]);
  __syncthreads();
  if (threadIdx.x == 0)
  {
    TbbTile& ti = b.tiles[t];
    const u64 nPix = g.tileElems;
    u64 numValid = nPix;
    u32 dataBegin = kTbbDataBegin;
    if constexpr (MASKED) { const TbbMaskRec mr = b.m.rec[t]; numValid = mr.numValid; dataBegin += mr.rleLen; }
    // Lerc2.cpp:2289-2306: the better of the two books; the plain one where they tie
    const u32 n0 = s_book[0].ok ? s_book[0].nBytes : 0u, n1 = s_book[1].ok ? s_book[1].nBytes : 0u;
    u32 pick = 2u, nBytesHuffman = 0;
    if (n0 > 0u && n1 > 0u) { pick = (n0 <= n1) ? 0u : 1u; nBytesHuffman = min(n0, n1); }
    else if (n0 > 0u || n1 > 0u) { pick = (n0 > n1) ? 0u : 1u; nBytesHuffman = max(n0, n1); }
    // Lerc2.cpp:285-304
    u32 mode = (u32)IEM_Tiling, nBytesData = nBytesTiling;
    if (pick < 2u && nBytesHuffman < nBytesTiling) { mode = pick == 0u ? (u32)IEM_Huffman : (u32)IEM_DeltaHuffman; nBytesData = nBytesHuffman; }
    else pick = 2u;
    u32 fl = 0;
    // 16 x 16 blocks at low bit rates (Lerc2.cpp:333-357)
    if ((double)((u64)nBytesTiling * 8u) < (double)nPix * 1.5 && (u64)nBytesTiling < 4u * numValid
      && (nBytesHuffman == 0u || (u64)nBytesTiling < 2ull * nBytesHuffman) && (g.nRows > 8 || g.nCols > 8))
    {
      if (MASKED) ti.retry = 1u; else fl |= kTbbRetry16;
    }
    nBytesData += 1u;    // the mode byte
    if (numValid <= (u64)nBytesData) fl |= kTbbOneSweep;
    ti.mode = mode;
    ti.nBytesTiling = nBytesTiling;
    ti.nBytesHuffman = nBytesHuffman;
    ti.tableBytes = pick < 2u ? s_book[pick].tableBytes : 0u;
    ti.nBits = pick < 2u ? s_book[pick].nBits : 0ull;
    ti.head.blobSize = dataBegin - 1u + nBytesData;
    if (slotBytes)
    {
      ti.head.offset = (firstTile + t) * slotBytes;
      if ((u64)ti.head.blobSize > slotBytes) fl |= kTbCapacity;
    }
    ti.head.flags = fl;
    s_pick = fl ? 2u : pick;
  }
  __syncthreads();
  const u32 pick = s_pick;
  if (pick >= 2u) return;
  const TbbBook& k = s_book[pick];
  b.codes[(u64)t * 256u + threadIdx.x] = ((u64)k.len[threadIdx.x] << 32) | k.code[threadIdx.x];
  u8* __restrict__ tab = b.table + (u64)t * kTbbTableCap;
  for (u32 i = threadIdx.x; i < k.tableBytes; i += 256u) tab[i] = k.table[i];
}

// masked form, the tiles k_tbb_decide marked: a wave per 16 x 16 block, the block's size
template<class T>
__global__ void __launch_bounds__(256) k_tbb_blocks16(TbbGeom g, BandParams p, const T* __restrict__ data, TbbEncodeBuffers b)
{
  __shared__ T s_val[4][256];
  __shared__ u32 s_obuf[4][1];
  __shared__ u32 s_lut[4][1];
  const u32 t = blockIdx.y;
  const TbbTile ti = b.tiles[t];
  if (ti.head.flags || !ti.retry) return;
  const int nTV = (g.nRows + 15) / 16, nTH = (g.nCols + 15) / 16;
  const int w = waveId();
  const int pos = (int)blockIdx.x * 4 + w;
  if (pos >= nTV * nTH) return;    // whole wave leaves together
  p.mb = 16; p.nTV = nTV; p.nTH = nTH;
  p.allValid = (b.m.rec[t].numValid == (u32)g.tileElems) ? 1 : 0;
  tbEncodeBlock<T, 4, true, false>(p, pos, data + (u64)t * g.tileElems, b.m.bits + (u64)t * b.m.bitStride, b.m.blockOff16 + (u64)t * b.m.pos16Stride,
                                   nullptr, s_val[w], s_obuf[w], s_lut[w]);
}

// ... and Lerc2.cpp:346: 16 x 16 blocks that are no longer than what the tile has so far win -- the tile is handed back
__global__ void __launch_bounds__(256) k_tbb_decide16(TbbGeom g, TbbEncodeBuffers b)
{
  __shared__ u32 s_scan[257];
  __shared__ u32 s_rec[2];
  const u32 t = blockIdx.x;
  if (threadIdx.x == 0) { s_rec[0] = b.tiles[t].head.flags; s_rec[1] = b.tiles[t].retry; }
  __syncthreads();
  if (s_rec[0] || !s_rec[1]) return;
  const u32 nBytes16 = blockScanInPlace(b.m.blockOff16 + (u64)t * b.m.pos16Stride, (u32)(((g.nRows + 15) / 16) * ((g.nCols + 15) / 16)), s_scan);
  if (threadIdx.x != 0) return;
  TbbTile& ti = b.tiles[t];
  const u32 nBytesData = ti.mode == (u32)IEM_Tiling ? ti.nBytesTiling : ti.nBytesHuffman;
  if (nBytes16 <= nBytesData) ti.head.flags = kTbbRetry16;
}

__global__ void __launch_bounds__(256) k_tbb_arena(u32 nTiles, u64 arenaBase, u64 arenaCapacity, TbbEncodeBuffers b)
{
  __shared__ u64 s_part[257];
  tbArenaPlace(b.tiles, nTiles, arenaBase, arenaCapacity, s_part);
}

static const u32 kTbbRun = 16;                      // pixels a thread packs in one step
static const u32 kTbbStep = 256u * kTbbRun;         // ... and the workgroup
static const u32 kTbbStageWords = kTbbStep + 4u;    // 32 bits a code word at most, the word carried over, one to spill into

// MASKED: header and mask section as the masked batch writes them (tbWriteHeaderMask), for a tile without a valid pixel nothing else;
// in the pixel stream an invalid pixel is a code of length 0 -- the step's scan is the compaction
// BANDS (MASKED only): the header says how many band blobs follow; the blob begins at any byte (every store here is a byte's, but
// for the stream's words, which ask the address)
// LARGE (MASKED only): the bit mask is read where k_tbb_stats left it in the workspace, not copied into LDS -- with a copy of 33 KB
// the kernel would hold more than 64 KB; only the table of last words is made in LDS
template<class T, bool MASKED, bool BANDS = false, bool LARGE = false>
__global__ void __launch_bounds__(256) k_tbb_write(TbbGeom g, const u8* __restrict__ data, u8* __restrict__ arena, TbbEncodeBuffers b, u32 nBands)
{
  __shared__ u8 s_hdr[kTbbDataBegin + 2];
  __shared__ u64 s_code[256];
  __shared__ u32 s_stage[kTbbStageWords];
  __shared__ u32 s_wave[4];
  const u32 t = blockIdx.x;
  const TbbTile ti = b.tiles[t];
  if (ti.head.flags) return;
  const u32 nPix = (u32)g.tileElems, nCols = (u32)g.nCols;
  u8* __restrict__ blob = arena + ti.head.offset;
  // ---- header (Lerc2.cpp:724-786; checksum patched by k_tbb_checksum), the mask section, ranges, "not one sweep", mode
  u32 dataBegin = kTbbDataBegin;
  if constexpr (MASKED)
  {
    const TbbMaskRec mr = b.m.rec[t];
    const bool empty = ti.mode == kTbbModeEmpty;
    const int off = (g.dt == DT_Char) ? 128 : 0;
    const TbHeader6 hd = { kCodecVersion, 0u, g.nRows, g.nCols, 1, (int)mr.numValid, 8, (int)ti.head.blobSize, g.dt,
                           BANDS ? (int)(nBands - 1u - t % nBands) : 0, 0u, 0.5, empty ? 0.0 : (double)((int)ti.symMin - off), empty ? 0.0 : (double)((int)ti.symMax - off) };
    s_code[threadIdx.x] = b.codes[(u64)t * 256u + threadIdx.x];
    tbWriteHeaderMask(blob, hd, b.m.rle + (u64)t * b.m.rleStride, mr.rleLen, s_hdr);    // (its barrier covers s_code)
    if (empty) return;
    dataBegin += mr.rleLen;
    if (threadIdx.x == 0)
    {
      u8* r = blob + kHdr6 + 4u + mr.rleLen;
      r[0] = (u8)((int)ti.symMin - off);
      r[1] = (u8)((int)ti.symMax - off);
      r[2] = 0;
      r[3] = (u8)ti.mode;
    }
  }
  else
  {
    if (threadIdx.x == 0)
    {
      u8* h = s_hdr;
      const int off = (g.dt == DT_Char) ? 128 : 0;
      const TbHeader6 hd = { kCodecVersion, 0u, g.nRows, g.nCols, 1, (int)nPix, 8, (int)ti.head.blobSize, g.dt, 0, 0u,
                             0.5, (double)((int)ti.symMin - off), (double)((int)ti.symMax - off) };
      tbWriteHeader6(h, hd);
      putBytes(h + kHdr6, 0ull, 4);
      h[kHdr6 + 4u] = (u8)((int)ti.symMin - off);
      h[kHdr6 + 5u] = (u8)((int)ti.symMax - off);
      h[kHdr6 + 6u] = 0;
      h[kHdr6 + 7u] = (u8)ti.mode;
    }
    s_code[threadIdx.x] = b.codes[(u64)t * 256u + threadIdx.x];
    __syncthreads();
    for (u32 i = threadIdx.x; i < kTbbDataBegin; i += 256u) blob[i] = s_hdr[i];
  }
  if (ti.mode == (u32)IEM_Tiling) return;
  const u8* __restrict__ tab = b.table + (u64)t * kTbbTableCap;
  for (u32 i = threadIdx.x; i < ti.tableBytes; i += 256u) blob[dataBegin + i] = tab[i];

  // ---- the pixel stream: code words MSB first in little-endian 32-bit words (Huffman::PushValue)
  const u8* __restrict__ px = data + (u64)t * g.tileElems;
  u8* __restrict__ stream = blob + dataBegin + ti.tableBytes;    // (masked: any alignment, with the mask section's length)
  const bool aligned = ((uintptr_t)stream & 3u) == 0u;
  const bool delta = ti.mode == (u32)IEM_DeltaHuffman;
  TbbmMask m = { nullptr, nullptr };
  if constexpr (MASKED)
  {
    __shared__ u16 s_last[TbForm<LARGE>::kMaskWords];
    __shared__ u32 s_scan[256];
    const u32 nBytes = (nPix + 7u) >> 3;
    const u8* __restrict__ bits = b.m.bits + (u64)t * b.m.bitStride;
    if constexpr (LARGE) m.bits = bits;
    else
    {
      __shared__ __align__(16) u8 s_bits[kTbSmallMaskBytes + 16];
      for (u32 i = threadIdx.x; i < nBytes + 16u; i += 256u) s_bits[i] = i < nBytes ? bits[i] : (u8)0;
      __syncthreads();
      m.bits = s_bits;
    }
    if (delta) tbbmLastWords(m.bits, nPix, s_last, s_scan);
    m.last = s_last;
  }
  u32 carryBits = 0, carryWord = 0, wordBase = 0;
  for (u32 k0 = 0; k0 < nPix; k0 += kTbbStep)
  {
    for (u32 i = threadIdx.x; i < kTbbStageWords; i += 256u) s_stage[i] = (i == 0u) ? carryWord : 0u;
    u32 len[kTbbRun], code[kTbbRun];
    u32 sum = 0;
    const u32 first = k0 + threadIdx.x * kTbbRun;
#pragma unroll
    for (u32 j = 0; j < kTbbRun; j++)
    {
      const u32 k = first + j;
      u64 c = 0;
      if constexpr (MASKED) { if (k < nPix && m.valid(k)) c = s_code[tbbBin<T>(delta ? tbbmDelta(px, m, k, nCols) : (u32)px[k])]; }
      else if (k < nPix) c = s_code[tbbBin<T>(delta ? tbbDelta(px, k, nCols) : (u32)px[k])];
      len[j] = (u32)(c >> 32); code[j] = (u32)c;
      sum += len[j];
    }
    const u32 incl = waveInclusiveScan(sum);
    if (laneId() == 63) s_wave[waveId()] = incl;
    __syncthreads();    // (s_stage cleared, the waves' sums there)
    u32 before = 0, total = 0;
    for (int w = 0; w < 4; w++) { if (w < waveId()) before += s_wave[w]; total += s_wave[w]; }
    u32 p = carryBits + before + incl - sum;
    u32 w = p >> 5, fill = p & 31u, cur = 0;
#pragma unroll
    for (u32 j = 0; j < kTbbRun; j++)
    {
      if (!len[j]) continue;
      const u64 x = (((u64)code[j]) << (64u - len[j])) >> fill;
      cur |= (u32)(x >> 32);
      fill += len[j];
      if (fill >= 32u) { atomicOr(&s_stage[w], cur); w++; cur = (u32)x; fill -= 32u; }
    }
    if (cur) atomicOr(&s_stage[w], cur);
    __syncthreads();
    const u32 segBits = carryBits + total, nFull = segBits >> 5;
    for (u32 i = threadIdx.x; i < nFull; i += 256u)
    {
      const u32 v = s_stage[i];
      u8* dst = stream + 4ull * (wordBase + i);
      if (aligned) *reinterpret_cast<u32*>(dst) = v;
      else { dst[0] = (u8)v; dst[1] = (u8)(v >> 8); dst[2] = (u8)(v >> 16); dst[3] = (u8)(v >> 24); }
    }
    carryBits = segBits & 31u;
    carryWord = carryBits ? s_stage[nFull] : 0u;
    wordBase += nFull;
    __syncthreads();    // (everybody has read s_stage and s_wave)
  }
  // the last, partly filled word and one more (Lerc2.cpp:2464: the decoder's look-up may read ahead)
  if (threadIdx.x < 8u)
  {
    const u32 nTail = carryBits ? 2u : 1u;
    const u32 wordIdx = threadIdx.x >> 2, byteIdx = threadIdx.x & 3u;
    if (wordIdx < nTail)
    {
      const u32 v = (carryBits && wordIdx == 0u) ? carryWord : 0u;
      stream[4ull * (wordBase + wordIdx) + byteIdx] = (u8)(v >> (8u * byteIdx));
    }
  }
}

__global__ void __launch_bounds__(256) k_tbb_checksum(u8* __restrict__ arena, TbbEncodeBuffers b)
{
  __shared__ u64 s_red[4];
  tbWriteChecksum(arena, b.tiles[blockIdx.x].head, s_red);
}

template<class T, bool MASKED>
static void tbbEncodeT(const TbbGeom& g, const BandParams& bp, const void* dTiles, u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes,
                       u64 firstTile, const TbbEncodeBuffers& b, hipStream_t st)
{
  const int nPos = g.nTV * g.nTH;
  const dim3 perTile(g.nTiles), blk(256), perBlock((nPos + 3) / 4, g.nTiles);
  const bool large = MASKED && tbLargeForm(g);    // (the forms without a mask hold no array that grows with the tile)
  if (large) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbb_stats<T, MASKED, false, MASKED>), perTile, blk, 0, st, g, (const u8*)dTiles, b, 1u, (u64)0); }
  else { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbb_stats<T, MASKED, false, false>), perTile, blk, 0, st, g, (const u8*)dTiles, b, 1u, (u64)0); }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbb_blocks<T, false, MASKED>), perBlock, blk, 0, st, g, bp, (const T*)dTiles, (u8*)nullptr, b);
  hipLaunchKernelGGL(k_tbb_decide<MASKED>, perTile, blk, 0, st, g, slotBytes, firstTile, b);
  if constexpr (MASKED)
  {
    // (over the whole batch, whether a tile is marked or not: the host knows nothing yet, and does not wait to learn it)
    const int nPos16 = ((g.nRows + 15) / 16) * ((g.nCols + 15) / 16);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbb_blocks16<T>), dim3((nPos16 + 3) / 4, g.nTiles), blk, 0, st, g, bp, (const T*)dTiles, b);
    hipLaunchKernelGGL(k_tbb_decide16, perTile, blk, 0, st, g, b);
  }
  if (!slotBytes) hipLaunchKernelGGL(k_tbb_arena, dim3(1), blk, 0, st, g.nTiles, arenaBase, arenaCapacity, b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbb_blocks<T, true, MASKED>), perBlock, blk, 0, st, g, bp, (const T*)dTiles, dArena, b);
  if (large) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbb_write<T, MASKED, false, MASKED>), perTile, blk, 0, st, g, (const u8*)dTiles, dArena, b, 1u); }
  else { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbb_write<T, MASKED, false, false>), perTile, blk, 0, st, g, (const u8*)dTiles, dArena, b, 1u); }
  hipLaunchKernelGGL(k_tbb_checksum, perTile, blk, 0, st, dArena, b);
}

// band stacks: ONE workgroup folds the planes into tiles and places the tiles (tbPlaceBands, tile_batch_dev.h)
__global__ void __launch_bounds__(256) k_tbb_place_bands(u32 nTiles, u32 nBands, u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile,
                                                         TbbEncodeBuffers b)
{
  __shared__ u64 s[257];
  tbPlaceBands(b.tiles, nTiles, nBands, arenaBase, arenaCapacity, slotBytes, firstTile, s);
}

// the masked launch set over the planes; the slot check and the placement are k_tbb_place_bands' for whole tiles
template<class T>
static void tbbEncodeBandsT(const TbbGeom& g, u32 nBands, const BandParams& bp, const void* dTiles, u64 validStride, u8* dArena, u64 arenaBase,
                            u64 arenaCapacity, u64 slotBytes, u64 firstTile, const TbbEncodeBuffers& b, hipStream_t st)
{
  const int nPos = g.nTV * g.nTH, nPos16 = ((g.nRows + 15) / 16) * ((g.nCols + 15) / 16);
  const dim3 perPlane(g.nTiles), blk(256), perBlock((nPos + 3) / 4, g.nTiles);
  const bool large = tbLargeForm(g);
  if (large) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbb_stats<T, true, true, true>), perPlane, blk, 0, st, g, (const u8*)dTiles, b, nBands, validStride); }
  else { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbb_stats<T, true, true, false>), perPlane, blk, 0, st, g, (const u8*)dTiles, b, nBands, validStride); }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbb_blocks<T, false, true>), perBlock, blk, 0, st, g, bp, (const T*)dTiles, (u8*)nullptr, b);
  hipLaunchKernelGGL(k_tbb_decide<true>, perPlane, blk, 0, st, g, (u64)0, (u64)0, b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbb_blocks16<T>), dim3((nPos16 + 3) / 4, g.nTiles), blk, 0, st, g, bp, (const T*)dTiles, b);
  hipLaunchKernelGGL(k_tbb_decide16, perPlane, blk, 0, st, g, b);
  hipLaunchKernelGGL(k_tbb_place_bands, dim3(1), blk, 0, st, g.nTiles / nBands, nBands, arenaBase, arenaCapacity, slotBytes, firstTile, b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbb_blocks<T, true, true>), perBlock, blk, 0, st, g, bp, (const T*)dTiles, dArena, b);
  if (large) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbb_write<T, true, true, true>), perPlane, blk, 0, st, g, (const u8*)dTiles, dArena, b, nBands); }
  else { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbb_write<T, true, true, false>), perPlane, blk, 0, st, g, (const u8*)dTiles, dArena, b, nBands); }
  hipLaunchKernelGGL(k_tbb_checksum, perPlane, blk, 0, st, dArena, b);
}

void launchTbbEncodeBands(const TbbGeom& g, u32 nBands, const BandParams& bp, const void* dTiles, u64 validStride, u8* dArena, u64 arenaBase,
                          u64 arenaCapacity, u64 slotBytes, u64 firstTile, const TbbEncodeBuffers& b, hipStream_t st)
{
  if (g.dt == DT_Char) tbbEncodeBandsT<signed char>(g, nBands, bp, dTiles, validStride, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st);
  else if (g.dt == DT_Byte) tbbEncodeBandsT<unsigned char>(g, nBands, bp, dTiles, validStride, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st);
}

void launchTbbEncode(const TbbGeom& g, const BandParams& bp, const void* dTiles, u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes,
                     u64 firstTile, const TbbEncodeBuffers& b, hipStream_t st)
{
  const bool masked = b.m.valid != nullptr;
  if (g.dt == DT_Char)
  {
    if (masked) tbbEncodeT<signed char, true>(g, bp, dTiles, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st);
    else tbbEncodeT<signed char, false>(g, bp, dTiles, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st);
  }
  else if (g.dt == DT_Byte)
  {
    if (masked) tbbEncodeT<unsigned char, true>(g, bp, dTiles, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st);
    else tbbEncodeT<unsigned char, false>(g, bp, dTiles, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, b, st);
  }
}

// ================================================================================================
// decode
// ================================================================================================
// parseTable (huffman_host.cpp) for codec 6, by one thread; the batch takes tables of 256 symbols whose range does not lap itself and
// whose lengths are stored in at most 6 bits -- every table an encoder writes -- and leaves any other to the single-blob decoder
__device__ bool tbbParseTable(const u8* __restrict__ p, u32 n, u8* __restrict__ lens, u32* __restrict__ codes, u32& used)
{
  if (n < 16u) return false;
  int hdr[4];
  for (int i = 0; i < 4; i++) hdr[i] = (int)(u32)getBytes(p + 4 * i, 4);
  if (hdr[0] < 2) return false;
  const int size = hdr[1], i0 = hdr[2], i1 = hdr[3];
  if (size != 256 || i0 >= i1 || i0 < 0 || i0 >= size || i1 - 1 >= 2 * size || i1 - i0 > size) return false;
  u32 at = 16;
  if (n < at + 1u) return false;
  const u8 b0 = p[at++];
  const int code = b0 >> 6, cb = (code == 0) ? 4 : 3 - code;
  const int nb = b0 & 31;
  if (cb == 0 || (b0 & 32) || n < at + (u32)cb || nb > 6) return false;
  u32 cnt = 0;
  for (int i = 0; i < cb; i++) cnt |= (u32)p[at + i] << (8 * i);
  at += (u32)cb;
  if (cnt != (u32)(i1 - i0)) return false;
  for (int i = 0; i < 256; i++) { lens[i] = 0; codes[i] = 0; }
  if (nb > 0)
  {
    const u32 nBytes = (cnt * (u32)nb + 7u) >> 3;
    if (n < at + nBytes) return false;
    for (u32 i = 0; i < cnt; i++)
    {
      const u32 bit = i * (u32)nb, q = bit >> 3;
      const u32 v = (u32)p[at + q] | (q + 1u < nBytes ? (u32)p[at + q + 1u] << 8 : 0u);
      const int sym = i0 + (int)i - ((i0 + (int)i) < 256 ? 0 : 256);
      lens[sym] = (u8)((v >> (bit & 7u)) & ((1u << nb) - 1u));
    }
    at += nBytes;
  }
  // the codes themselves, MSB first in little-endian words (Huffman.cpp:471-537)
  u32 word = 0;
  int bitPos = 0;
  for (int i = i0; i < i1; i++)
  {
    const int sym = i - (i < 256 ? 0 : 256);
    const int len = lens[sym];
    if (len == 0) continue;
    if (len > 32) return false;
    if (n < at + 4u * (word + 1u)) return false;
    const u32 w0 = (u32)getBytes(p + at + 4u * word, 4);
    u32 c = (w0 << bitPos) >> (32 - len);
    if (32 - bitPos >= len) { bitPos += len; if (bitPos == 32) { bitPos = 0; word++; } }
    else
    {
      bitPos += len - 32;
      word++;
      if (n < at + 4u * (word + 1u)) return false;
      const u32 w1 = (u32)getBytes(p + at + 4u * word, 4);
      c |= w1 >> (32 - bitPos);
    }
    codes[sym] = c;
  }
  used = at + 4u * (word + (bitPos > 0 ? 1u : 0u));
  return used <= n;
}

// MASKED: a mask section of any length in front of the ranges; the run-length stream expanded into LDS (tbMaskUnrle, as the masked
// batch's parse does), the mask's own count held against the header's, the bit mask left in the workspace, the caller's valid
// bytes written; tiling mode: the valid counts per block out of the bit mask
// BANDS (MASKED only): t is a plane, tile * nBands + band, offsets / sizes are the planes' (k_tbbd_chain).  A band behind band 0
// carries no mask section of its own: its count of valid pixels is band 0's, and between none and all it takes band 0's run-length
// stream ("the mask stays in force").  A band with a mask section of its own, or a count that is not band 0's, is refused: the
// single-blob decoder takes the whole stack.  The caller's valid bytes are written by band 0; without them (b.m.valid null) a blob
// with an invalid pixel is refused.
// LARGE (MASKED only): the form for tiles beyond the small form's mask bytes or blocks (tile_batch.h: TbForm)
template<class T, bool MASKED, bool BANDS = false, bool LARGE = false>
__global__ void __launch_bounds__(256)
k_tbbd_parse(TbbGeom g, const u8* __restrict__ arena, const u64* __restrict__ offsets, const u32* __restrict__ sizes, TbbDecodeBuffers b, u32 nBands)
{
  __shared__ u64 s_red[4];
  __shared__ TbbTile s_ti;
  __shared__ u16 s_nv[MASKED ? TbForm<LARGE>::kBlocks : 1];
  __shared__ TbbMaskRec s_mr;
  const u32 t = blockIdx.x;
  const u8* __restrict__ blob = arena + offsets[t];
  const u32 sizeGiven = sizes[t];
  const u32 nPix = (u32)g.tileElems;
  const u32 band = BANDS ? t % nBands : 0u, plane0 = t - band;
  // (band 0's blob: read by the bands behind it only where their own header, and so the chain, has held)
  const u8* __restrict__ blob0 = BANDS ? arena + offsets[plane0] : blob;
  const u32 size0 = BANDS ? sizes[plane0] : sizeGiven;

  if (threadIdx.x == 0)
  {
    TbbTile ti;
    memset(&ti, 0, sizeof(ti));
    u32 fl = 0;
    if constexpr (MASKED)
    {
      TbbMaskRec mr = { 0u, 0u };
      if (sizeGiven < kHdr6 + 4u) fl = kTbHeader;
      else
      {
        TbHeader6 h;
        if (!tbReadHeader6(blob, h)) fl = kTbHeader;
        ti.checksum = h.checksum;
        ti.head.blobSize = (u32)h.blobSize;
        if (h.version != kCodecVersion || h.nRows != g.nRows || h.nCols != g.nCols || h.nDepth != 1 || h.numValid < 0 || (u32)h.numValid > nPix
          || h.microBlockSize != 8 || h.blobSize < (int)(kHdr6 + 4u) || (u32)h.blobSize > sizeGiven || h.dt != g.dt
          || h.nBlobsMore != (BANDS ? (int)(nBands - 1u - band) : 0) || (h.flagBytes & 0xFFu) != 0u)
          fl = kTbHeader;
        if (BANDS && !fl)
        {
          if (!b.m.valid && (u32)h.numValid != nPix) fl = kTbHeader;
          if (band > 0u && (size0 < kHdr6 + 4u || (u32)getBytes(blob0 + 26, 4) != (u32)h.numValid)) fl = kTbHeader;
        }
        if (!fl)
        {
          mr.numValid = (u32)h.numValid;
          mr.rleLen = (u32)getBytes(blob + kHdr6, 4);
          const bool noStream = mr.numValid == nPix || mr.numValid == 0u;
          if ((noStream || band > 0u) ? mr.rleLen != 0u : (mr.rleLen < 2u || mr.rleLen > ti.head.blobSize)) fl = kTbHeader;
          else if (mr.numValid == 0u)
          {
            // no valid pixel: nothing may follow the mask section's length (Lerc2.cpp:235-241); range and error bound are not asked
            ti.mode = kTbbModeEmpty;
            if (ti.head.blobSize != kHdr6 + 4u) fl = kTbHeader;
          }
          else if (!(h.maxZErr == 0.5) || !(h.zMin < h.zMax) || (u64)kTbbDataBegin + mr.rleLen + 1u > (u64)ti.head.blobSize) fl = kTbHeader;
          else
          {
            const u8* r = blob + kHdr6 + 4u + mr.rleLen;
            if (r[0] == r[1] || r[2] != 0 || r[3] > 2) fl = kTbHeader;    // constant, one sweep, a later mode
            ti.mode = r[3];
          }
        }
      }
      s_mr = mr;
    }
    else if (sizeGiven < kTbbDataBegin + 1u) fl = kTbHeader;
    else
    {
      TbHeader6 h;
      if (!tbReadHeader6(blob, h)) fl = kTbHeader;
      ti.checksum = h.checksum;
      ti.head.blobSize = (u32)h.blobSize;
      if (h.version != kCodecVersion || h.nRows != g.nRows || h.nCols != g.nCols || h.nDepth != 1 || (u32)h.numValid != nPix || h.microBlockSize != 8
        || h.blobSize < (int)(kTbbDataBegin + 1u) || (u32)h.blobSize > sizeGiven || h.dt != g.dt || h.nBlobsMore != 0 || (h.flagBytes & 0xFFu) != 0u)
        fl = kTbHeader;
      // (the mode byte is there for an error bound of 0.5 only: Lerc2::HeaderInfo::TryHuffmanInt)
      if (!(h.maxZErr == 0.5) || !(h.zMin < h.zMax)) fl = kTbHeader;
      if (!fl)
      {
        const u8* r = blob + kHdr6;
        if (getBytes(r, 4) != 0ull || r[4] == r[5] || r[6] != 0 || r[7] > 2) fl = kTbHeader;    // a mask, constant, one sweep, a later mode
        ti.mode = r[7];
      }
    }
    ti.head.flags = fl;
    s_ti = ti;
  }
  __syncthreads();
  if (s_ti.head.flags) { if (threadIdx.x == 0) b.tiles[t] = s_ti; return; }
  const u32 blobEnd = s_ti.head.blobSize;

  // ---- Fletcher32 over blob[14 .. blobSize)
  if (!tbChecksumOk(blob, blobEnd, s_ti.checksum, s_red))
  {
    if (threadIdx.x == 0) { s_ti.head.flags = kTbChecksum; b.tiles[t] = s_ti; }
    return;
  }
  u32 dataBegin = kTbbDataBegin;
  if constexpr (MASKED)
  {
    // ---- the mask: all ones, all zeros, or the run-length stream expanded (what it does not fill stays zero)
    __shared__ __align__(16) u8 s_bits[TbForm<LARGE>::kMaskBytes + 16];
    const TbbMaskRec mr = s_mr;
    const u32 nBytes = (nPix + 7u) >> 3;
    const bool allValid = mr.numValid == nPix, empty = mr.numValid == 0u;
    dataBegin += mr.rleLen;
    for (u32 i = threadIdx.x; i < nBytes + 16u; i += 256u) s_bits[i] = (allValid && i < nBytes) ? (u8)0xFF : (u8)0;
    __syncthreads();
    if (!allValid && !empty && threadIdx.x == 0)
    {
      if (band > 0u)
      {
        const u32 nm0 = (u32)getBytes(blob0 + kHdr6, 4);
        if (nm0 < 2u || (u64)kHdr6 + 4u + nm0 > (u64)size0 || !tbMaskUnrle(blob0 + kHdr6 + 4u, nm0, s_bits, nBytes)) s_ti.head.flags = kTbbMaskStream;
      }
      else if (!tbMaskUnrle(blob + kHdr6 + 4u, mr.rleLen, s_bits, nBytes)) s_ti.head.flags = kTbbMaskStream;
    }
    __syncthreads();
    // (a mask that names another number of valid pixels than the header does is the single-blob decoder's business: it asks the mask)
    const u32 own = tbMaskCount(s_bits, nPix, s_red);
    if (s_ti.head.flags || own != mr.numValid)
    {
      if (threadIdx.x == 0) { if (!s_ti.head.flags) s_ti.head.flags = kTbHeader; b.tiles[t] = s_ti; }
      return;
    }
    u8* __restrict__ bitsOut = b.m.bits + (u64)t * b.m.bitStride;
    for (u32 i = threadIdx.x; i < nBytes; i += 256u) bitsOut[i] = s_bits[i];
    if (!BANDS || (band == 0u && b.m.valid))
    {
      u8* __restrict__ vOut = b.m.valid + (u64)(BANDS ? t / nBands : t) * g.tileElems;
      for (u32 k = threadIdx.x; k < nPix; k += 256u) vOut[k] = (u8)((s_bits[k >> 3] >> (7u - (k & 7u))) & 1u);
    }
    if (threadIdx.x == 0) b.m.rec[t] = mr;
    if (s_ti.mode == (u32)IEM_Tiling)
    {
      tbBlockValidCounts(s_bits, (u32)g.nRows, (u32)g.nCols, 8u, s_nv);
      __syncthreads();
    }
  }
  if (threadIdx.x != 0) return;

  if (s_ti.mode == (u32)IEM_Tiling)
  {
    // ---- the walk over the block headers; a block's length follows from its header and its count of valid pixels
    const BandParams p = tbFillBandParams(g, 8);
    if constexpr (MASKED)
      s_ti.head.flags = tbWalkBlocks<1, 8u>(blob, dataBegin, blobEnd, p, b.blockOff + (u64)t * g.posStride, [&](u32 k, u32) { return (int)s_nv[k]; });
    else
      s_ti.head.flags = tbWalkBlocks<1, 8u>(blob, kTbbDataBegin, blobEnd, p, b.blockOff + (u64)t * g.posStride, [](u32, u32 nElem) { return (int)nElem; });
  }
  else if (!MASKED || s_ti.mode != kTbbModeEmpty)
  {
    u32 used = 0;
    if (!tbbParseTable(blob + dataBegin, blobEnd - dataBegin, b.lens + (u64)t * 256u, b.codes + (u64)t * 256u, used)) s_ti.head.flags = kTbbTable;
    else if (dataBegin + used + 4u > blobEnd) s_ti.head.flags = kTbbStream;
    s_ti.tableBytes = dataBegin + used;
  }
  b.tiles[t] = s_ti;
}

// a wave per block: k_decode_tiles (tile_decode.hip) for one value a pixel, every pixel valid, with the tile's own blob
template<class T, bool MASKED>
__global__ void __launch_bounds__(256)
k_tbbd_blocks(TbbGeom g, const u8* __restrict__ arena, const u64* __restrict__ offsets, T* __restrict__ outAll, TbbDecodeBuffers b)
{
  __shared__ u32 s_lut[4][256];
  __shared__ __align__(16) u8 s_head[4][64];
  const u32 t = blockIdx.y;
  if ((b.tiles[t].head.flags & ~kTbSibling) || b.tiles[t].mode != (u32)IEM_Tiling) return;
  const int w = waveId();
  const int pos = (int)blockIdx.x * 4 + w;
  if (pos >= g.nTV * g.nTH) return;
  BandParams p = tbFillBandParams(g, 8);
  p.allValid = 1;
  p.invScale = 1.0;    // 2 * maxZErr
  const u8* __restrict__ blob = arena + offsets[t];
  double zMax;
  { const u64 bits = getBytes(blob + 66, 8); memcpy(&zMax, &bits, 8); }
  bool failed;
  if constexpr (MASKED)
  {
    p.allValid = (b.m.rec[t].numValid == (u32)g.tileElems) ? 1 : 0;
    failed = tbDecodeBlock<T, 1, true>(p, zMax, pos, blob, b.tiles[t].head.blobSize, b.blockOff[(u64)t * g.posStride + pos],
                                       b.m.bits + (u64)t * b.m.bitStride, outAll + (u64)t * g.tileElems, s_lut[w], s_head[w]);
  }
  else
    failed = tbDecodeBlock<T, 1, false>(p, zMax, pos, blob, b.tiles[t].head.blobSize, b.blockOff[(u64)t * g.posStride + pos], nullptr,
                                        outAll + (u64)t * g.tileElems, s_lut[w], s_head[w]);
  if (failed && laneId() == 0) atomicOr(&b.tiles[t].head.flags, kTbSibling);
}

static const u32 kTbbdStageWords = 10240;    // 40 KB of stream in LDS: 4.9 bits a pixel at 256 x 256; a longer stream is read where it lies

struct TbbdBits
{
  const u32* s_str;       // the staged words, or nullptr
  const u8* bytes;        // the stream where it lies
  u32 nWords;
  __device__ __forceinline__ u32 word(u32 w) const
  {
    if (w >= nWords) return 0u;    // (words beyond the stream read as zero: peek32, huffman_kernels.hip)
    if (s_str) return s_str[w];
    const u8* q = bytes + 4ull * w;
    return (u32)q[0] | ((u32)q[1] << 8) | ((u32)q[2] << 16) | ((u32)q[3] << 24);
  }
  __device__ __forceinline__ u32 top(u32 pos) const
  {
    const u32 w = pos >> 5;
    const u64 x = ((u64)word(w) << 32) | word(w + 1u);
    return (u32)((x << (pos & 31u)) >> 32);
  }
};

struct TbbdTable
{
  u32 lut[1 << kHuffLutBits];    // (symbol << 8) | length for codes of <= 12 bits, 0: none
  u32 longCode[256];
  u16 longLenSym[256];           // sorted by length, then symbol
  u32 nLong;
};

// returns the code length (0 = no code matches): decodeOne (huffman_kernels.hip)
__device__ __forceinline__ int tbbdDecodeOne(const TbbdTable& s, u32 top, u32& sym)
{
  const u32 e = s.lut[top >> (32 - kHuffLutBits)];
  if (e) { sym = e >> 8; return (int)(e & 255u); }
  const u32 nLong = s.nLong;
  for (u32 i = 0; i < nLong; i++)
  {
    const u32 ls = s.longLenSym[i];
    const int len = (int)(ls >> 8);
    if ((top >> (32 - len)) == s.longCode[i]) { sym = ls & 0xFFu; return len; }
  }
  return 0;
}

// The masked predictor undone in place by ONE wave (Lerc2.cpp:2546-2575; the wave step of k_huff_undelta, huffman_kernels.hip): row
// by row -- a pixel and the pixel above it never share a step --, 64 pixels a step: a prefix sum over the step's differences, restarts
// from the pixel above where a segment's head has no valid left neighbour but a valid pixel above (found by a ballot), and a carry
// for "the last valid pixel so far".  out: the differences at valid pixels, 0 elsewhere; bits: the tile's bit mask where it lies.
// The load of out[k - nCols] reads what ANOTHER lane of this wave stored a row earlier, with no fence between: a wave's vector memory
// instructions are issued and performed in order, and a load behind a store of the same wave to the same address returns the stored
// value (k_huff_undelta, huffman_kernels.hip, stands on the same ground).  It holds for ONE wave only -- do not spread the rows over waves.
__device__ __forceinline__ void tbbdUndeltaMasked(u8* __restrict__ out, const u8* __restrict__ bits, u32 nRows, u32 nCols)
{
  const u32 lane = (u32)laneId();
  const u64 le = laneMaskLt() | (1ull << lane);
  u32 carry = 0;
  for (u32 i = 0; i < nRows; i++)
    for (u32 j0 = 0; j0 < nCols; j0 += 64u)
    {
      const u32 j = j0 + lane;
      const bool inb = j < nCols;
      const u32 k = i * nCols + j;
      const bool valid = inb && maskBit(bits, (i64)k);
      const bool leftOk = valid && j > 0u && maskBit(bits, (i64)k - 1);
      const bool fromAbove = valid && !leftOk && i > 0u && maskBit(bits, (i64)k - nCols);
      const u32 d = valid ? (u32)out[k] : 0u;
      const u32 above = fromAbove ? (u32)out[k - nCols] : 0u;
      const u32 s = waveInclusiveScan(d);
      const u64 mine = __ballot(fromAbove) & le;
      const int h = mine ? 63 - __clzll((long long)mine) : 0;
      const u32 sH = __shfl(s, h), dH = __shfl(d, h), aH = __shfl(above, h);
      const u32 val = (mine ? (aH + s - (sH - dH)) : (carry + s)) & 0xFFu;
      if (valid) out[k] = (u8)val;
      const u64 vmask = __ballot(valid);
      if (vmask) carry = __shfl(val, 63 - __clzll((long long)vmask));
    }
}

// MASKED: exactly numValid code words; a partly valid tile's symbols go to the workspace in the order of the stream and from there to
// the valid positions (a pixel's rank: tbRankedSweep over the bit mask in the workspace), zeros elsewhere; a tile without a valid
// pixel is zeros
template<class T, bool MASKED>
__global__ void __launch_bounds__(256)
k_tbbd_huff(TbbGeom g, const u8* __restrict__ arena, const u64* __restrict__ offsets, u8* __restrict__ outAll, TbbDecodeBuffers b)
{
  __shared__ TbbdTable s_tab;
  __shared__ u32 s_str[kTbbdStageWords];
  __shared__ u8 s_len[256];
  __shared__ u32 s_code[256];
  __shared__ u32 s_exit[256];
  __shared__ u32 s_scan[257];
  __shared__ u32 s_any, s_bad;
  const u32 t = blockIdx.x;
  const TbbTile ti = b.tiles[t];
  if (ti.head.flags || ti.mode == (u32)IEM_Tiling) return;
  const u32 nPix = (u32)g.tileElems, nCols = (u32)g.nCols, nRows = (u32)g.nRows;
  const u8* __restrict__ blob = arena + offsets[t];
  u8* __restrict__ out = outAll + (u64)t * g.tileElems;
  u32 numValid = nPix;
  if constexpr (MASKED)
  {
    if (ti.mode == kTbbModeEmpty) { for (u32 k = threadIdx.x; k < nPix; k += 256u) out[k] = 0; return; }
    numValid = b.m.rec[t].numValid;
  }
  const bool partial = MASKED && numValid != nPix;
  const u32 streamBegin = ti.tableBytes, blobEnd = ti.head.blobSize;

  // ---- the look-up table (buildDecodeTable, huffman_host.cpp): the host fills it symbol by symbol, so where two codes claim an entry
  // the larger symbol has it
  const u32 sym = threadIdx.x;
  const u32 myLen = b.lens[(u64)t * 256u + sym], myCode = b.codes[(u64)t * 256u + sym];
  s_len[sym] = (u8)myLen; s_code[sym] = myCode;
  for (u32 i = threadIdx.x; i < (1u << kHuffLutBits); i += 256u) s_tab.lut[i] = 0;
  if (threadIdx.x == 0) { s_any = 0; s_bad = 0; s_tab.nLong = 0; }
  __syncthreads();
  if (myLen > 0u && myLen <= (u32)kHuffLutBits)
  {
    const u32 span = 1u << (kHuffLutBits - myLen), base = myCode << (kHuffLutBits - myLen);
    if (myCode >= (1u << myLen)) s_bad = 1;    // (base + span > the table: the host refuses the blob)
    else for (u32 j = 0; j < span; j++) atomicMax(&s_tab.lut[base + j], (sym << 8) | myLen);
  }
  else if (myLen > (u32)kHuffLutBits)
  {
    u32 rank = 0;
    for (u32 j = 0; j < 256u; j++)
    {
      const u32 l = s_len[j];
      if (l > (u32)kHuffLutBits && (l < myLen || (l == myLen && j < sym))) rank++;
    }
    s_tab.longCode[rank] = myCode;
    s_tab.longLenSym[rank] = (u16)((myLen << 8) | sym);
    atomicAdd(&s_tab.nLong, 1u);
  }
  if (myLen) s_any = 1;
  // ---- the stream, as whole words; staged where it fits
  const u32 nWords = (blobEnd - streamBegin) >> 2, streamBits = nWords * 32u;
  TbbdBits in;
  in.bytes = blob + streamBegin; in.nWords = nWords;
  in.s_str = (nWords <= kTbbdStageWords) ? s_str : nullptr;
  if (in.s_str)
    for (u32 i = threadIdx.x; i < nWords; i += 256u)
    {
      const u8* q = in.bytes + 4ull * i;
      s_str[i] = (u32)q[0] | ((u32)q[1] << 8) | ((u32)q[2] << 16) | ((u32)q[3] << 24);
    }
  __syncthreads();
  if (s_bad || !s_any)    // (no code at all: codeRange fails on the host)
  {
    if (threadIdx.x == 0) b.tiles[t].head.flags = kTbbTable;
    return;
  }

  // ---- 256 sub-sequences: decode from the own start to the own end; then every thread whose predecessor ended somewhere else starts
  // over from there, until the chain fits (at most one pass a thread: a pass settles at least the first unsettled one)
  const u32 subBits = ((nWords + 255u) / 256u) * 32u;
  const u32 end = min((threadIdx.x + 1u) * subBits, streamBits);
  u32 start = min(threadIdx.x * subBits, streamBits), count = 0, exitPos = start;
  bool todo = true;
  for (u32 pass = 0; pass < 258u; pass++)
  {
    if (todo)
    {
      u32 pos = start, n = 0;
      while (pos < end)
      {
        u32 sy;
        const int len = tbbdDecodeOne(s_tab, in.top(pos), sy);
        if (len == 0) break;    // (no code word matches: nothing behind it counts)
        pos += (u32)len;
        n++;
      }
      exitPos = pos; count = n;
    }
    __syncthreads();
    s_exit[threadIdx.x] = exitPos;
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    todo = false;
    if (threadIdx.x > 0u)
    {
      const u32 before = s_exit[threadIdx.x - 1u];
      if (before != start) { start = before; todo = true; s_any = 1; }
    }
    __syncthreads();
    if (!s_any) break;
  }
  // ---- where each sub-sequence's symbols go
  __syncthreads();
  s_scan[threadIdx.x] = count;
  __syncthreads();
  if (threadIdx.x == 0) { u32 run = 0; for (u32 i = 0; i < 256u; i++) { const u32 y = s_scan[i]; s_scan[i] = run; run += y; } s_scan[256] = run; }
  __syncthreads();
  if (s_any || s_scan[256] < numValid)    // (the chain did not settle -- it cannot be --, or fewer code words than (valid) pixels)
  {
    if (threadIdx.x == 0) b.tiles[t].head.flags = kTbbStream;
    return;
  }
  {
    u8* dst = partial ? b.m.sym + (u64)t * g.tileElems : out;    // (no __restrict__: `sym` below names the same bytes)
    u32 pos = start, k = s_scan[threadIdx.x];
    for (u32 i = 0; i < count && k < numValid; i++, k++)
    {
      u32 sy = 0;
      const int len = tbbdDecodeOne(s_tab, in.top(pos), sy);
      pos += (u32)len;
      dst[k] = (u8)tbbBin<T>(sy);    // (T)(symbol - offset): the same flip of the top bit
    }
  }
  if constexpr (MASKED)
    if (partial)
    {
      const u8* __restrict__ bits = b.m.bits + (u64)t * b.m.bitStride;
      const u8* __restrict__ sym = b.m.sym + (u64)t * g.tileElems;
      __syncthreads();    // (every thread's symbols are in the workspace)
      tbRankedSweep(bits, nPix, s_scan, [&](u32 k, bool valid, u32 rank) { out[k] = valid ? sym[rank] : (u8)0; });
      if (ti.mode != (u32)IEM_DeltaHuffman) return;
      __syncthreads();
      if (waveId() == 0) tbbdUndeltaMasked(out, bits, nRows, nCols);
      return;
    }
  if (ti.mode != (u32)IEM_DeltaHuffman) return;

  // ---- the predictor undone (Lerc2.cpp:2499-2523): column 0 sums down the rows, then every row sums along itself; bytes wrap
  __syncthreads();
  u32 carry = 0;
  for (u32 r0 = 0; r0 < nRows; r0 += 256u)
  {
    const u32 r = r0 + threadIdx.x;
    const u32 v = r < nRows ? out[(u64)r * nCols] : 0u;
    const u32 incl = waveInclusiveScan(v);
    if (laneId() == 63) s_scan[waveId()] = incl;
    __syncthreads();
    u32 before = carry, total = 0;
    for (int w = 0; w < 4; w++) { if (w < waveId()) before += s_scan[w]; total += s_scan[w]; }
    if (r < nRows) out[(u64)r * nCols] = (u8)(before + incl);
    carry += total;
    __syncthreads();
  }
  for (u32 r = (u32)waveId(); r < nRows; r += 4u)
  {
    u8* __restrict__ row = out + (u64)r * nCols;
    u32 run = 0;
    for (u32 j0 = 0; j0 < nCols; j0 += 64u)
    {
      const u32 j = j0 + (u32)laneId();
      const u32 v = j < nCols ? row[j] : 0u;
      const u32 incl = waveInclusiveScan(v) + run;
      if (j < nCols) row[j] = (u8)incl;
      run = __shfl(incl, 63);
    }
  }
}

template<class T, bool MASKED>
static void tbbDecodeT(const TbbGeom& g, const u8* dArena, const u64* dOffsets, const u32* dSizes, void* dTiles, const TbbDecodeBuffers& b, hipStream_t st)
{
  const int nPos = g.nTV * g.nTH;
  if (MASKED && tbLargeForm(g)) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbbd_parse<T, MASKED, false, MASKED>), dim3(g.nTiles), dim3(256), 0, st, g, dArena, dOffsets, dSizes, b, 1u); }
  else { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbbd_parse<T, MASKED, false, false>), dim3(g.nTiles), dim3(256), 0, st, g, dArena, dOffsets, dSizes, b, 1u); }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbbd_blocks<T, MASKED>), dim3((nPos + 3) / 4, g.nTiles), dim3(256), 0, st, g, dArena, dOffsets, (T*)dTiles, b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbbd_huff<T, MASKED>), dim3(g.nTiles), dim3(256), 0, st, g, dArena, dOffsets, (u8*)dTiles, b);
}

// band stacks: a thread per tile walks the chain of band blobs (tbBandChain, tile_batch_dev.h)
__global__ void __launch_bounds__(256)
k_tbbd_chain(TbbGeom g, u32 nTiles, u32 nBands, const u8* __restrict__ arena, const u64* __restrict__ offsets, const u32* __restrict__ sizes,
             u64* __restrict__ planeOff, u32* __restrict__ planeSize)
{
  tbBandChain(g, nTiles, nBands, arena, offsets, sizes, planeOff, planeSize);
}

template<class T>
static void tbbDecodeBandsT(const TbbGeom& g, u32 nBands, const u8* dArena, const u64* dOffsets, const u32* dSizes, u64* planeOff, u32* planeSize,
                            void* dTiles, const TbbDecodeBuffers& b, hipStream_t st)
{
  const int nPos = g.nTV * g.nTH;
  const u32 nTiles = g.nTiles / nBands;
  hipLaunchKernelGGL(k_tbbd_chain, dim3((nTiles + 255u) / 256u), dim3(256), 0, st, g, nTiles, nBands, dArena, dOffsets, dSizes, planeOff, planeSize);
  if (tbLargeForm(g)) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbbd_parse<T, true, true, true>), dim3(g.nTiles), dim3(256), 0, st, g, dArena, (const u64*)planeOff, (const u32*)planeSize, b, nBands); }
  else { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbbd_parse<T, true, true, false>), dim3(g.nTiles), dim3(256), 0, st, g, dArena, (const u64*)planeOff, (const u32*)planeSize, b, nBands); }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbbd_blocks<T, true>), dim3((nPos + 3) / 4, g.nTiles), dim3(256), 0, st, g, dArena, (const u64*)planeOff, (T*)dTiles, b);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tbbd_huff<T, true>), dim3(g.nTiles), dim3(256), 0, st, g, dArena, (const u64*)planeOff, (u8*)dTiles, b);
}

void launchTbbDecodeBands(const TbbGeom& g, u32 nBands, const u8* dArena, const u64* dOffsets, const u32* dSizes, u64* planeOff, u32* planeSize,
                          void* dTiles, const TbbDecodeBuffers& b, hipStream_t st)
{
  if (g.dt == DT_Char) tbbDecodeBandsT<signed char>(g, nBands, dArena, dOffsets, dSizes, planeOff, planeSize, dTiles, b, st);
  else if (g.dt == DT_Byte) tbbDecodeBandsT<unsigned char>(g, nBands, dArena, dOffsets, dSizes, planeOff, planeSize, dTiles, b, st);
}

void launchTbbDecode(const TbbGeom& g, const u8* dArena, const u64* dOffsets, const u32* dSizes, void* dTiles, const TbbDecodeBuffers& b, hipStream_t st)
{
  const bool masked = b.m.valid != nullptr;
  if (g.dt == DT_Char)
  {
    if (masked) tbbDecodeT<signed char, true>(g, dArena, dOffsets, dSizes, dTiles, b, st);
    else tbbDecodeT<signed char, false>(g, dArena, dOffsets, dSizes, dTiles, b, st);
  }
  else if (g.dt == DT_Byte)
  {
    if (masked) tbbDecodeT<unsigned char, true>(g, dArena, dOffsets, dSizes, dTiles, b, st);
    else tbbDecodeT<unsigned char, false>(g, dArena, dOffsets, dSizes, dTiles, b, st);
  }
}

}    // namespace lerc
