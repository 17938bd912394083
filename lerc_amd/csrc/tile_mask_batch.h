// tile_mask_batch.h -- batches of MASKED tiles (tile_mask_batch.hip): what the host hands the kernels and reads back.
#pragma once
#include "tile_batch.h"

namespace lerc {

// why a tile left the batch (it is then encoded / decoded by itself behind the batch, with its mask): this family's own reasons beside
// the shared ones (tile_batch.h).  kTbHeader here: codec < 6, another shape or type, blocks other than 8 x 8 or 16 x 16, a mode byte,
// bytes behind the last section, a count of valid pixels the mask does not share, ...
enum : u32
{
  kTmbNaN = 4u,           // a NaN at a valid pixel (the mask changes)
  kTmbRle = 512u,         // the mask's run-length stream outgrew its scratch
  // decode
  kTmbMaskStream = 4096u  // the mask's run-length stream is damaged
};

// what a tile's blob holds behind header and mask section (TmbTile::kind)
enum : u32
{
  kTmbKindBlocks8 = 0u,   // ranges, a 0 byte, the stream of 8 x 8 blocks
  kTmbKindBlocks16 = 1u,  // the same with 16 x 16 blocks: the low-bit-rate retry won (Lerc2.cpp:333-357)
  kTmbKindEmpty = 2u,     // no valid pixel: nothing
  kTmbKindConst = 3u,     // every valid pixel has the header's zMin: nothing
  kTmbKindOneSweep = 4u   // ranges, a 1 byte, the valid pixels raw in row order
};

struct TmbTile    // one per tile, device; copied home after the batch
{
  TileBatchRec head;
  u32 numValid;
  u32 rleLen;             // bytes of the mask section's run-length stream (0: every pixel valid)
  u32 nBytesTiling;       // bytes of the block stream
  u32 dataBegin;          // where the block stream begins in the blob
  u64 minBits, maxBits;   // range over the valid pixels, as raw values of the tile's type
  double zMin, zMax;
  double maxZErr;         // the tile's own error bound (encode: k_tmb_prelude decides it; decode: the header's)
  u32 checksum;           // decode: the header's
  u32 isInt;              // encode: float values that are all integers (header byte)
  u32 kind;               // kTmbKind...
  u32 retry;              // encode: the low-bit-rate rule asks for the sizes of 16 x 16 blocks (k_tmb_decide)
  u32 mbSize;             // encode: the header's microBlockSize -- 16 once the retry has won, even if one sweep then beats the blocks
  u32 nBlobsMore;         // encode: the header's count of band blobs that follow (0 unless the tile is a band of a stack)
};

static_assert(sizeof(TmbTile) % 8 == 0, "records lie back to back");

struct TmbGeom    // TileGeom's fields and this family's strides
{
  int nRows, nCols, nTV, nTH, dt;
  u32 nTiles;
  u32 bitStride;          // bytes between the tiles' bit masks (a multiple of 16)
  u32 rleStride;          // bytes between the tiles' run-length scratch
  u32 posStride;          // words between the tiles' block tables (>= nTV * nTH + 1)
  u32 pos16Stride;        // encode: words between the tiles' tables of 16 x 16 blocks (>= their number + 1)
  u64 tileElems;
};

struct TmbEncodeBuffers
{
  TmbTile* tiles;
  u8* bits;               // [nTiles][bitStride]
  u8* rle;                // [nTiles][rleStride]
  u32* blockOff;          // [nTiles][posStride]: sizes, then their exclusive scan
  u32* blockOff16;        // [nTiles][pos16Stride]: the same for 16 x 16 blocks, tiles with TmbTile::retry only
};
// maxZErr: the header's for a tile whose statistics decide nothing else; cand: TryRaiseMaxZError candidates whose error bound beats it (bit c: factor c)
void launchTmbEncode(const TmbGeom& g, const BandParams& bp, double maxZErr, u32 cand, const void* dTiles, const u8* dValidBytes, u8* dArena,
                     u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile, const TmbEncodeBuffers& b, hipStream_t st);

struct TmbDecodeBuffers
{
  TmbTile* tiles;
  u8* bits;               // [nTiles][bitStride]
  u32* blockOff;          // [nTiles][posStride]
};
void launchTmbDecode(const TmbGeom& g, const u8* dArena, const u64* dOffsets, const u32* dSizes, void* dTiles, u8* dValidBytes,
                     const TmbDecodeBuffers& b, hipStream_t st);

// ---- band stacks: a tile is nBands rasters [nBands][nRows][nCols] under ONE mask, its blob the bands' blobs byte-adjacent.  The
// kernels' unit is the plane, tile * nBands + band: g.nTiles counts planes, and so do the records and every buffer above.
// Encode: dValidBytes is never null (the caller hands all ones for a call without masks), tile t's mask lies at dValidBytes + t *
// validStride (0: one mask for all).  Band 0 carries the mask section, the bands behind it the 4-byte count 0; a tile with a plane
// that leaves the batch leaves it whole (kTbBand on its other planes) and claims no room.  firstTile counts tiles.
void launchTmbEncodeBands(const TmbGeom& g, u32 nBands, const BandParams& bp, double maxZErr, u32 cand, const void* dTiles, const u8* dValidBytes,
                          u64 validStride, u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile, const TmbEncodeBuffers& b, hipStream_t st);
// Decode: dOffsets / dSizes are per TILE; a thread per tile walks the chain of band headers into planeOff / planeSize (per plane; a
// chain that does not hold leaves sizes of 0, which the parse refuses).  dValidBytes: [tiles][nRows][nCols], written from band 0, or
// null (then a blob with an invalid pixel is refused).
void launchTmbDecodeBands(const TmbGeom& g, u32 nBands, const u8* dArena, const u64* dOffsets, const u32* dSizes, u64* planeOff, u32* planeSize,
                          void* dTiles, u8* dValidBytes, const TmbDecodeBuffers& b, hipStream_t st);

}    // namespace lerc
