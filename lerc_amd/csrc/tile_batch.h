// tile_batch.h -- what the two families of tile batches share, on the host and on the device (tile_mask_batch.h, tile_byte_batch.h,
// codec_tiles_batch.cpp): the head of a tile's record, the reasons both know for handing a tile back, the geometry of a batch.
#pragma once
#include "lerc_common.h"

namespace lerc {

// why a tile left the batch (it is then encoded / decoded by itself behind the batch); each family's own reasons are in its header
enum : u32
{
  kTbCapacity = 64u,      // the blob does not fit its slot (encoded by itself, that tile says BufferTooSmall)
  kTbArenaFull = 128u,    // the blob does not fit what is left of the arena
  // decode
  kTbHeader = 1024u,      // not a header the batch takes
  kTbChecksum = 2048u,    // Fletcher32 differs
  kTbBlocks = 8192u,      // the walk met a block header that cannot be, or the blocks do not end where the blob does
  kTbSibling = 16384u,    // a block's decode failed (raised by the block kernel's waves)
  // band stacks
  kTbBand = 131072u       // another band of the tile left the batch: the tile goes back whole
};

// the head of every tile's record (TmbTile, TbbTile): all the host driver reads of one
struct TileBatchRec
{
  u32 flags;              // 0: the batch's kernels did the tile
  u32 blobSize;
  u64 offset;             // where the blob lies in the arena
};

struct TileGeom    // (TmbGeom, tile_mask_batch.h, has these fields too, with its strides among them)
{
  int nRows, nCols, nTV, nTH, dt;    // nTV x nTH blocks of 8 x 8
  u32 nTiles;
  u32 posStride;          // words between the tiles' block tables (>= nTV * nTH + 1)
  u64 tileElems;
};

// ---- how large a tile (a plane of a band stack) the batches take: its bit mask and its per-block counts live in the LDS of the
// kernels that own a tile.  513 x 513 is 263 169 pixels and 4 225 blocks of 8 x 8; both limits also admit long thin shapes.  Larger
// tiles go one by one inside the call.
static const u32 kTbMaxPixels = 264192;       // 516 x 512; 33 024 mask bytes
static const u32 kTbMaxMaskBytes = kTbMaxPixels / 8;
static const u32 kTbMaxBlocks = 4352;
// the kernels with such arrays come in two forms, picked by the host from the shape (tbLargeForm): the small one holds what the batches
// took before 512 x 512 tiles came in (256 x 256, 257 x 257: 8 257 mask bytes) and keeps its occupancy, the large one the limits above
static const u32 kTbSmallMaskBytes = 16384;
static const u32 kTbSmallBlocks = 4096;

template<bool LARGE> struct TbForm
{
  static const u32 kMaskBytes = LARGE ? kTbMaxMaskBytes : kTbSmallMaskBytes;
  static const u32 kBlocks = LARGE ? kTbMaxBlocks : kTbSmallBlocks;
  static const u32 kMaskWords = kMaskBytes / 4u;    // words of 32 pixels
};

inline bool tbShapeFits(int nRows, int nCols)
{
  const u64 nPix = (u64)nRows * (u64)nCols, nPos = (u64)((nRows + 7) / 8) * (u64)((nCols + 7) / 8);
  return nPix <= kTbMaxPixels && nPos <= kTbMaxBlocks;
}

template<class G>
inline bool tbLargeForm(const G& g)
{
  return ((g.tileElems + 7u) >> 3) > kTbSmallMaskBytes || (u64)g.nTV * (u64)g.nTH > kTbSmallBlocks;
}

// the fields of BandParams that follow from a batch's geometry and a block size alone, the others zero
template<class G>
LERC_HD BandParams tbFillBandParams(const G& g, int mb)
{
  BandParams p;
  memset(&p, 0, sizeof(p));
  p.nRows = g.nRows; p.nCols = g.nCols; p.nDepth = 1; p.dt = g.dt; p.version = kCodecVersion;
  p.mb = mb; p.nTV = (g.nRows + mb - 1) / mb; p.nTH = (g.nCols + mb - 1) / mb;
  return p;
}

}    // namespace lerc
