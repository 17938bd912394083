// tile_depth_batch.h -- batches of DEPTH tiles (tile_depth_batch.hip): nTiles rasters [nRows][nCols][nDepth] of one shape, each with a
// validity mask [nRows][nCols] of its own, every tile one Lerc2 blob with the header's nDepth.  What the host hands the kernels and
// reads back.  The geometry is the masked family's (TmbGeom: tileElems counts PIXELS), the depth travels beside it.
#pragma once
#include "tile_mask_batch.h"

namespace lerc {

static const int kTdbMaxDepth = 8;    // the per-slice statistics live in registers and in the tile's record

// TdbTile::kind: the masked family's kinds (tile_mask_batch.h) and one more
enum : u32
{
  kTdbKindConstSlices = 5u    // every slice is constant, the slices differ: header, mask section, ranges (Lerc2.cpp:273-278)
};

struct TdbTile    // one per tile, device; copied home after the batch
{
  TileBatchRec head;
  u32 numValid;
  u32 rleLen;             // bytes of the mask section's run-length stream (0: every pixel valid)
  u32 nBytesTiling;       // bytes of the block stream
  u32 dataBegin;          // where the block stream (the raw sweep) begins in the blob
  double zMin, zMax;      // over all slices: the header's
  double maxZErr;         // the tile's own error bound (encode: k_tdb_prelude decides it; decode: the header's)
  u32 checksum;           // decode: the header's
  u32 isInt;              // encode: float values that are all integers (header byte)
  u32 kind;
  u32 retry;              // encode: the low-bit-rate rule asks for the sizes of 16 x 16 blocks
  u32 mbSize;             // encode: the header's microBlockSize
  u32 checkOverflow;      // encode: a slice difference may leave int (Lerc2.h:312-315)
  u64 minBits[kTdbMaxDepth], maxBits[kTdbMaxDepth];    // the slices' ranges over the valid pixels, as raw values of the tile's type
};

static_assert(sizeof(TdbTile) % 8 == 0, "records lie back to back");

struct TdbEncodeBuffers
{
  TdbTile* tiles;
  u8* bits;               // [nTiles][bitStride]
  u8* rle;                // [nTiles][rleStride]
  u32* blockOff;          // [nTiles][posStride]: a position's size over all its slices, then the exclusive scan
  u32* blockOff16;        // [nTiles][pos16Stride]: the same for 16 x 16 blocks, tiles with TdbTile::retry only
};
// dTiles: [nTiles][nRows][nCols][nDepth]; dValidBytes is never null (the caller hands all ones for a call without masks), tile t's mask
// lies at dValidBytes + t * validStride (0: one mask for all).  maxZErr, cand: as launchTmbEncode's.
void launchTdbEncode(const TmbGeom& g, int nDepth, const BandParams& bp, double maxZErr, u32 cand, const void* dTiles, const u8* dValidBytes,
                     u64 validStride, u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile, const TdbEncodeBuffers& b,
                     hipStream_t st);

struct TdbDecodeBuffers
{
  TdbTile* tiles;
  u8* bits;               // [nTiles][bitStride]
  u32* blockOff;          // [nTiles][posStride]: where a position's first sub-block begins
};
// dValidBytes: [nTiles][nRows][nCols], written 1 / 0, or null (then a blob with an invalid pixel is refused)
void launchTdbDecode(const TmbGeom& g, int nDepth, const u8* dArena, const u64* dOffsets, const u32* dSizes, void* dTiles, u8* dValidBytes,
                     const TdbDecodeBuffers& b, hipStream_t st);

}    // namespace lerc
