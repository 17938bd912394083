// tile_byte_batch.h -- batches of 8-BIT tiles (tile_byte_batch.hip): what the host hands the kernels and reads back.  Two forms of
// one launch set: every pixel valid (TbbMaskBuffers unused), and MASKED -- a byte mask per tile, the Huffman modes over valid pixels.
#pragma once
#include "tile_batch.h"

namespace lerc {

// why a tile left the batch (it is then encoded / decoded by itself behind the batch): this family's own reasons beside the shared ones
// (tile_batch.h).  kTbHeader here: codec < 6, another shape or type, a mask, 16 x 16 blocks, constant, one sweep, ...
enum : u32
{
  kTbbConst = 2u,         // every pixel has the same value
  kTbbRetry16 = 32u,      // the low-bit-rate rule asks for 16 x 16 blocks (Lerc2.cpp:335-338)
  kTbbOneSweep = 256u,    // the raw form is no longer than the coded one
  kTbbRle = 512u,         // masked: the mask's run-length stream outgrew its scratch
  // decode
  kTbbTable = 4096u,      // the code table fails one of parseTable's checks, or is one the batch leaves alone
  kTbbStream = 32768u,    // the pixel stream holds fewer code words than the tile has (valid) pixels
  kTbbMaskStream = 65536u // masked: the mask's run-length stream is damaged
};

struct TbbTile    // one per tile, device; copied home after the batch
{
  TileBatchRec head;
  u32 mode;               // ImageEncodeMode: 0 tiling, 1 delta Huffman, 2 Huffman
  u32 nBytesTiling;       // bytes of the 8 x 8 block stream
  u32 nBytesHuffman;      // code table + pixel stream + padding words of the better code book (0: none)
  u32 tableBytes;         // encode: the serialised code table; decode: where the pixel stream begins in the blob
  u64 nBits;              // bits of the pixel stream
  u32 symMin, symMax;     // range as histogram bins (value + 128 for DT_Char)
  u32 checksum;           // decode: the header's
  u32 retry;              // masked encode: the low-bit-rate rule asks for the sizes of 16 x 16 blocks (k_tbb_decide -> k_tbb_decide16)
};

static_assert(sizeof(TbbTile) % 8 == 0, "records lie back to back");

struct TbbGeom : TileGeom {};

// the masked form's part of a tile's record, and of the workspace (behind the buffers both forms have: their members stay where they are)
struct TbbMaskRec
{
  u32 numValid;
  u32 rleLen;             // bytes of the mask section's run-length stream (0: every pixel valid, or none)
};

struct TbbMaskBuffers
{
  TbbMaskRec* rec;        // [nTiles]
  u8* bits;               // [nTiles][bitStride]: the bit masks
  u8* rle;                // encode: [nTiles][rleStride]
  u32* blockOff16;        // encode: [nTiles][pos16Stride], the sizes of 16 x 16 blocks of the tiles with TbbTile::retry
  u8* sym;                // decode: [nTiles][tileElems], a Huffman tile's symbols in the order of the stream
  u8* valid;              // the caller's valid bytes (encode: read)
  u32 bitStride, rleStride, pos16Stride;
};

// (the size limits are the batches' common ones, tile_batch.h.  A Huffman code longer than 32 bits needs a histogram whose counts grow
// like the Fibonacci numbers, 9 227 465 pixels at the least: far more than kTbMaxPixels, so tbbBuildBook's refusal is never met)
static const u32 kTbbTableCap = 1280;         // 16 + 3 + 256 * 6 / 8 + 256 * 32 / 8 + 4, rounded up
static const u32 kTbbDataBegin = 98;          // header 90, mask section 4, ranges 2, "not one sweep" 1, mode 1; masked: + TbbMaskRec::rleLen
static const u32 kTbbModeEmpty = 3;           // TbbTile::mode of a masked tile without a valid pixel: header and mask section are all of it

struct TbbEncodeBuffers
{
  TbbTile* tiles;
  u32* histo;             // [nTiles][512]: plain, then delta
  u32* blockOff;          // [nTiles][posStride]: sizes, then their exclusive scan
  u64* codes;             // [nTiles][256]: (length << 32) | code of the chosen book
  u8* table;              // [nTiles][kTbbTableCap]: its serialised table
  TbbMaskBuffers m;       // masked form only
};
// masked: b.m.valid != nullptr
void launchTbbEncode(const TbbGeom& g, const BandParams& bp, const void* dTiles, u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes,
                     u64 firstTile, const TbbEncodeBuffers& b, hipStream_t st);

struct TbbDecodeBuffers
{
  TbbTile* tiles;
  u32* blockOff;          // [nTiles][posStride] (tiling mode)
  u32* codes;             // [nTiles][256] (Huffman modes)
  u8* lens;               // [nTiles][256]
  TbbMaskBuffers m;       // masked form only
};
// masked: b.m.valid != nullptr
void launchTbbDecode(const TbbGeom& g, const u8* dArena, const u64* dOffsets, const u32* dSizes, void* dTiles, const TbbDecodeBuffers& b, hipStream_t st);

// ---- band stacks: a tile is nBands rasters [nBands][nRows][nCols] under ONE mask, its blob the bands' blobs byte-adjacent.  The
// kernels' unit is the plane, tile * nBands + band: g.nTiles counts planes, and so do the records and every buffer above.  Always the
// MASKED form: a call without masks hands all ones.
// Encode: b.m.valid is never null, tile t's mask lies at b.m.valid + t * validStride (0: one mask for all).  Band 0 carries the mask
// section, the bands behind it the 4-byte count 0; a tile with a plane that leaves the batch (a constant band, one sweep, 16 x 16
// blocks, ...) leaves it whole (kTbBand on its other planes) and claims no room.  firstTile counts tiles.
void launchTbbEncodeBands(const TbbGeom& g, u32 nBands, const BandParams& bp, const void* dTiles, u64 validStride, u8* dArena, u64 arenaBase,
                          u64 arenaCapacity, u64 slotBytes, u64 firstTile, const TbbEncodeBuffers& b, hipStream_t st);
// Decode: dOffsets / dSizes are per TILE; a thread per tile walks the chain of band headers into planeOff / planeSize (per plane; a
// chain that does not hold leaves sizes of 0, which the parse refuses).  b.m.valid: [tiles][nRows][nCols], written from band 0, or
// null (then a blob with an invalid pixel is refused).
void launchTbbDecodeBands(const TbbGeom& g, u32 nBands, const u8* dArena, const u64* dOffsets, const u32* dSizes, u64* planeOff, u32* planeSize,
                          void* dTiles, const TbbDecodeBuffers& b, hipStream_t st);

}    // namespace lerc
