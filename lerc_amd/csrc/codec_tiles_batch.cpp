// codec_tiles_batch.cpp -- host side of the tile batches that do a mosaic's tiles in ONE set of launches and one host wait per sub-batch:
// the masked batch (lerc_amd_encode_tiles_device_masked / lerc_amd_decode_tiles_device_masked; kernels in tile_mask_batch.hip) and the
// 8-bit batch (DT_Char / DT_Byte, lossless, through the tile batch calls; kernels in tile_byte_batch.hip) -- every pixel valid, or, through
// the masked calls, with a mask per tile.  One driver, tbEncode / tbDecode, runs them all: the sub-batches, the workspace, the records'
// way home, the arena's bookkeeping -- per plane (tile * nBands + band) where a tile is a band stack (MaskedBandsBatch), folded into
// tiles in one walk over the records.  Tiles the kernels hand back (TileBatchRec::flags) are done one by one behind their sub-batch
// by encodeDevice / decodeDevice -- byte for byte what those calls make, and their exact status.  A family (MaskedBatch, BytesBatch,
// BytesMaskedBatch, and over band stacks MaskedBandsBatch, BytesBandsBatch) supplies what differs: its workspace, its launches, whether a tile by itself carries a mask, its words for a reason.
#include "codec.h"
#include "tile_mask_batch.h"
#include "tile_byte_batch.h"
#include "tile_depth_batch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace lerc {

// the fields every family's geometry has, the others zero
template<class G>
static G tileGeom(int dt, int nRows, int nCols)
{
  G g;
  memset(&g, 0, sizeof(g));
  g.nRows = nRows; g.nCols = nCols; g.nTV = (nRows + 7) / 8; g.nTH = (nCols + 7) / 8; g.dt = dt;
  g.tileElems = (u64)nRows * (u64)nCols;
  g.posStride = ((u32)(g.nTV * g.nTH) + 1u + 3u) & ~3u;
  return g;
}

// how many bands and masks a tile has: every family is constructed with it, the single-band ones leave it unread
struct TbStack { int nBands, nMasks; int nDepth = 1; };

// ================================================================================================
// the masked family
// ================================================================================================
static bool tmbShapeOk(int dt, int nRows, int nCols)
{
  return dt >= DT_Short && dt <= DT_Double && tbShapeFits(nRows, nCols);
}

// What the families that keep a tile's mask the masked family's way share (MaskedBatch, DepthBatch): the geometry with the mask's
// strides, the workspace per tile and its carving for a record type of their own (Rec: TmbTile, TdbTile; the buffer structs have the
// same members), the band parameters, the words for a reason.
struct MaskedGeometry
{
  static constexpr bool kMasked = true;    // a tile done by itself carries its mask

  TmbGeom g;

  MaskedGeometry(int dt, int nRows, int nCols) : g(tileGeom<TmbGeom>(dt, nRows, nCols))
  {
    const u32 nBytes = (u32)((g.tileElems + 7) >> 3);
    g.bitStride = (nBytes + 16u + 15u) & ~15u;
    g.rleStride = (2u * nBytes + 64u + 15u) & ~15u;    // (no stream is longer: a literal byte costs 1 + 2 / 32767, a run of five 3)
    g.pos16Stride = ((u32)(((nRows + 15) / 16) * ((nCols + 15) / 16)) + 1u + 3u) & ~3u;
  }

  template<class Rec> size_t encodeBytesOf() const { return sizeof(Rec) + g.bitStride + g.rleStride + ((size_t)g.posStride + g.pos16Stride) * 4; }
  template<class Rec> size_t decodeBytesOf() const { return sizeof(Rec) + g.bitStride + (size_t)g.posStride * 4 + 16; }

  // the workspace of n tiles -> their records, nullptr: no room
  template<class Rec, class EB> void* carveEncodeInto(Context& ctx, size_t n, EB& eb) const
  {
    eb.tiles = ctx.allocT<Rec>(n);
    eb.bits = ctx.allocT<u8>(n * g.bitStride);
    eb.rle = ctx.allocT<u8>(n * g.rleStride);
    eb.blockOff = ctx.allocT<u32>(n * g.posStride);
    eb.blockOff16 = ctx.allocT<u32>(n * g.pos16Stride);
    return (eb.bits && eb.rle && eb.blockOff && eb.blockOff16) ? eb.tiles : nullptr;
  }
  template<class Rec, class DB> void* carveDecodeInto(Context& ctx, size_t n, DB& db) const
  {
    db.tiles = ctx.allocT<Rec>(n);
    db.bits = ctx.allocT<u8>(n * g.bitStride);
    db.blockOff = ctx.allocT<u32>(n * g.posStride);
    return (db.bits && db.blockOff) ? db.tiles : nullptr;
  }
  // what the encode kernels are told beside the geometry: the band parameters, the call's error bound, the TryRaiseMaxZError candidates
  BandParams encodeParams(double maxZErr, u32& cand) const
  {
    const bool isFlt = g.dt >= DT_Float;
    cand = 0;
    if (isFlt)
    {
      static const double errCand[9] = { 1, 0.5, 0.1, 0.05, 0.01, 0.005, 0.001, 0.0005, 0.0001 };
      for (int c = 0; c < 9; c++) if (errCand[c] / 2 > maxZErr) cand |= 1u << c;
    }
    BandParams bp = tbFillBandParams(g, 8);
    bp.maxQ = maxValToQuantize(g.dt);
    bp.maxZErr = isFlt ? maxZErr : std::max(0.5, floor(maxZErr));
    bp.scale = 1 / (2 * bp.maxZErr);
    bp.invScale = 2 * bp.maxZErr;
    bp.intLossless = (!isFlt && bp.maxZErr == 0.5) ? 1 : 0;
    return bp;
  }

  static const char* reason(u32 flags)
  {
    if (flags & kTmbNaN) return "a NaN at a valid pixel";
    if (flags & kTbCapacity) return "the blob does not fit its slot";
    if (flags & kTbArenaFull) return "the arena is full";
    if (flags & kTmbRle) return "the mask's run-length stream outgrew its scratch";
    if (flags & kTbHeader) return "not a header the batch takes";
    if (flags & kTbChecksum) return "the checksum differs";
    if (flags & kTmbMaskStream) return "the mask's run-length stream is damaged";
    if (flags & (kTbBlocks | kTbSibling)) return "the block stream";
    return "unknown";
  }
};

struct MaskedBatch : MaskedGeometry
{
  static constexpr const char* kName = "masked";
  static constexpr const char* kLaunchError = "lerc_amd: a masked tile batch kernel could not be launched";
  static constexpr const char* kEncodeScope = "tiles_masked_encode";
  static constexpr const char* kDecodeScope = "tiles_masked_decode";
  static constexpr size_t kRecBytes = sizeof(TmbTile);

  TmbEncodeBuffers eb;
  TmbDecodeBuffers db;

  MaskedBatch(int dt, int nRows, int nCols, TbStack = { 1, 1 }) : MaskedGeometry(dt, nRows, nCols) {}

  size_t encodeBytesPerTile() const { return encodeBytesOf<TmbTile>(); }
  size_t encodeBytesPerBatch() const { return 0; }    // (workspace a sub-batch needs once, whatever its tile count)
  size_t decodeBytesPerTile() const { return decodeBytesOf<TmbTile>(); }
  void* carveEncode(Context& ctx, size_t n) { return carveEncodeInto<TmbTile>(ctx, n, eb); }
  void* carveDecode(Context& ctx, size_t n) { return carveDecodeInto<TmbTile>(ctx, n, db); }

  void launchEncode(u32 n, double maxZErr, const void* dTiles, const u8* dValid, u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile,
                    hipStream_t st)
  {
    g.nTiles = n;
    u32 cand = 0;    // TryRaiseMaxZError candidates whose error bound beats maxZErr
    const BandParams bp = encodeParams(maxZErr, cand);
    launchTmbEncode(g, bp, bp.maxZErr, cand, dTiles, dValid, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, eb, st);
  }
  void launchDecode(u32 n, const u8* dArena, const u64* dOff, const u32* dSize, void* dTiles, u8* dValid, hipStream_t st)
  {
    g.nTiles = n;
    launchTmbDecode(g, dArena, dOff, dSize, dTiles, dValid, db, st);
  }
};

// ---- the masked family over band stacks: the same kernels over planes (tile_mask_batch.h), nMasks 0 or 1.  Without masks the planes
// run under one mask of all ones, as all-valid tiles inside a masked batch do.
struct MaskedBandsBatch : MaskedBatch
{
  static constexpr const char* kName = "band stack";
  static constexpr const char* kLaunchError = "lerc_amd: a band stack tile batch kernel could not be launched";
  static constexpr const char* kEncodeScope = "tiles_bands_encode";
  static constexpr const char* kDecodeScope = "tiles_bands_decode";

  int nBands, nMasks;
  u8* ones = nullptr;         // encode without masks: tileElems bytes of 1
  u64* planeOff = nullptr;    // decode: [planes], k_tmbd_chain's
  u32* planeSize = nullptr;

  MaskedBandsBatch(int dt, int nRows, int nCols, TbStack s) : MaskedBatch(dt, nRows, nCols), nBands(s.nBands), nMasks(s.nMasks) {}

  size_t encodeBytesPerTile() const { return (size_t)nBands * MaskedBatch::encodeBytesPerTile(); }
  size_t decodeBytesPerTile() const { return (size_t)nBands * (MaskedBatch::decodeBytesPerTile() + 16); }
  size_t encodeBytesPerBatch() const { return nMasks ? 0 : (size_t)g.tileElems + 64; }    // (the all-ones mask, one for the sub-batch)

  void* carveEncode(Context& ctx, size_t n)
  {
    void* rec = MaskedBatch::carveEncode(ctx, n * (size_t)nBands);
    if (!nMasks) { ones = ctx.allocT<u8>((size_t)g.tileElems); if (!ones) return nullptr; }
    return rec;
  }
  void* carveDecode(Context& ctx, size_t n)
  {
    void* rec = MaskedBatch::carveDecode(ctx, n * (size_t)nBands);
    planeOff = ctx.allocT<u64>(n * (size_t)nBands);
    planeSize = ctx.allocT<u32>(n * (size_t)nBands);
    return (planeOff && planeSize) ? rec : nullptr;
  }
  void launchEncode(u32 n, double maxZErr, const void* dTiles, const u8* dValid, u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile,
                    hipStream_t st)
  {
    g.nTiles = n * (u32)nBands;
    u32 cand = 0;
    const BandParams bp = encodeParams(maxZErr, cand);
    if (!nMasks) hipMemsetAsync(ones, 1, (size_t)g.tileElems, st);
    launchTmbEncodeBands(g, (u32)nBands, bp, bp.maxZErr, cand, dTiles, nMasks ? dValid : ones, nMasks ? g.tileElems : 0, dArena, arenaBase, arenaCapacity,
                         slotBytes, firstTile, eb, st);
  }
  void launchDecode(u32 n, const u8* dArena, const u64* dOff, const u32* dSize, void* dTiles, u8* dValid, hipStream_t st)
  {
    g.nTiles = n * (u32)nBands;
    launchTmbDecodeBands(g, (u32)nBands, dArena, dOff, dSize, planeOff, planeSize, dTiles, nMasks ? dValid : nullptr, db, st);
  }

  static const char* reason(u32 flags)
  {
    if (flags == kTbBand) return "another band of the tile";
    return MaskedBatch::reason(flags & ~kTbBand);
  }
};

// ================================================================================================
// the depth family: tiles [nRows][nCols][nDepth] under one mask, one blob with the header's nDepth a tile (tile_depth_batch.hip).  The
// geometry, the mask's workspace and the error bounds are the masked family's; the records carry the slices' ranges.
// ================================================================================================
struct DepthBatch : MaskedGeometry
{
  static constexpr const char* kName = "depth";
  static constexpr const char* kLaunchError = "lerc_amd: a depth tile batch kernel could not be launched";
  static constexpr const char* kEncodeScope = "tiles_depth_encode";
  static constexpr const char* kDecodeScope = "tiles_depth_decode";
  static constexpr size_t kRecBytes = sizeof(TdbTile);

  int nDepth, nMasks;
  TdbEncodeBuffers deb = {};    // (the depth family's records, TdbTile: the slices' ranges ride in them)
  TdbDecodeBuffers ddb = {};
  u8* ones = nullptr;         // encode without masks: tileElems bytes of 1

  DepthBatch(int dt, int nRows, int nCols, TbStack s) : MaskedGeometry(dt, nRows, nCols), nDepth(s.nDepth), nMasks(s.nMasks) {}

  size_t encodeBytesPerTile() const { return encodeBytesOf<TdbTile>(); }
  size_t encodeBytesPerBatch() const { return nMasks ? 0 : (size_t)g.tileElems + 64; }    // (the all-ones mask, one for the sub-batch, as the band stacks have it)
  size_t decodeBytesPerTile() const { return decodeBytesOf<TdbTile>(); }

  void* carveEncode(Context& ctx, size_t n)
  {
    void* rec = carveEncodeInto<TdbTile>(ctx, n, deb);
    if (!nMasks) { ones = ctx.allocT<u8>((size_t)g.tileElems); if (!ones) return nullptr; }
    return rec;
  }
  void* carveDecode(Context& ctx, size_t n) { return carveDecodeInto<TdbTile>(ctx, n, ddb); }
  void launchEncode(u32 n, double maxZErr, const void* dTiles, const u8* dValid, u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile,
                    hipStream_t st)
  {
    g.nTiles = n;
    u32 cand = 0;
    const BandParams bp = encodeParams(maxZErr, cand);
    if (!nMasks) hipMemsetAsync(ones, 1, (size_t)g.tileElems, st);
    launchTdbEncode(g, nDepth, bp, bp.maxZErr, cand, dTiles, nMasks ? dValid : ones, nMasks ? g.tileElems : 0, dArena, arenaBase, arenaCapacity, slotBytes,
                    firstTile, deb, st);
  }
  void launchDecode(u32 n, const u8* dArena, const u64* dOff, const u32* dSize, void* dTiles, u8* dValid, hipStream_t st)
  {
    g.nTiles = n;
    launchTdbDecode(g, nDepth, dArena, dOff, dSize, dTiles, nMasks ? dValid : nullptr, ddb, st);
  }
};

// ================================================================================================
// the 8-bit family
// ================================================================================================
static bool tbbShapeOk(int dt, int nRows, int nCols)
{
  return (dt == DT_Char || dt == DT_Byte) && tbShapeFits(nRows, nCols);
}

bool tilesBytesEncodeEligible(const TilesEncodeRequest& rq)
{
  // (maxZErr < 1 on an integer type is lossless: the header says 0.5.  From 1 on there is no Huffman mode: the general path's business)
  return !rq.dValidBytes && rq.maxZErr < 1 && tbbShapeOk(rq.dt, rq.nRows, rq.nCols);
}

bool tilesBytesDecodeEligible(const TilesDecodeRequest& rq) { return !rq.dValidBytes && tbbShapeOk(rq.dt, rq.nRows, rq.nCols); }

struct BytesBatch
{
  static constexpr bool kMasked = false;
  static constexpr const char* kName = "8-bit";
  static constexpr const char* kLaunchError = "lerc_amd: an 8-bit tile batch kernel could not be launched";
  static constexpr const char* kEncodeScope = "tiles_bytes_encode";
  static constexpr const char* kDecodeScope = "tiles_bytes_decode";
  static constexpr size_t kRecBytes = sizeof(TbbTile);

  TbbGeom g;
  TbbEncodeBuffers eb = {};
  TbbDecodeBuffers db = {};

  BytesBatch(int dt, int nRows, int nCols, TbStack = { 1, 0 }) : g(tileGeom<TbbGeom>(dt, nRows, nCols)) {}

  size_t encodeBytesPerTile() const { return sizeof(TbbTile) + 512 * 4 + (size_t)g.posStride * 4 + 256 * 8 + kTbbTableCap; }
  size_t encodeBytesPerBatch() const { return 0; }
  size_t decodeBytesPerTile() const { return sizeof(TbbTile) + (size_t)g.posStride * 4 + 256 * 4 + 256 + 16; }

  void* carveEncode(Context& ctx, size_t n)
  {
    eb.tiles = ctx.allocT<TbbTile>(n);
    eb.histo = ctx.allocT<u32>(n * 512);
    eb.blockOff = ctx.allocT<u32>(n * g.posStride);
    eb.codes = ctx.allocT<u64>(n * 256);
    eb.table = ctx.allocT<u8>(n * kTbbTableCap);
    return (eb.histo && eb.blockOff && eb.codes && eb.table) ? eb.tiles : nullptr;
  }
  void* carveDecode(Context& ctx, size_t n)
  {
    db.tiles = ctx.allocT<TbbTile>(n);
    db.blockOff = ctx.allocT<u32>(n * g.posStride);
    db.codes = ctx.allocT<u32>(n * 256);
    db.lens = ctx.allocT<u8>(n * 256);
    return (db.blockOff && db.codes && db.lens) ? db.tiles : nullptr;
  }
  void launchEncode(u32 n, double, const void* dTiles, const u8*, u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile, hipStream_t st)
  {
    g.nTiles = n;
    BandParams bp = tbFillBandParams(g, 8);    // (lossless: the header says 0.5)
    bp.allValid = 1;
    bp.maxQ = maxValToQuantize(g.dt);
    bp.maxZErr = 0.5; bp.scale = 1.0; bp.invScale = 1.0;
    bp.intLossless = 1;
    launchTbbEncode(g, bp, dTiles, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, eb, st);
  }
  void launchDecode(u32 n, const u8* dArena, const u64* dOff, const u32* dSize, void* dTiles, u8*, hipStream_t st)
  {
    g.nTiles = n;
    launchTbbDecode(g, dArena, dOff, dSize, dTiles, db, st);
  }

  static const char* reason(u32 flags)
  {
    if (flags & kTbbConst) return "a constant tile";
    if (flags & kTbbRetry16) return "the low-bit-rate rule asks for 16 x 16 blocks";
    if (flags & kTbbOneSweep) return "one sweep";
    if (flags & kTbCapacity) return "the blob does not fit its slot";
    if (flags & kTbArenaFull) return "the arena is full";
    if (flags & kTbHeader) return "not a header the batch takes";
    if (flags & kTbChecksum) return "the checksum differs";
    if (flags & kTbbTable) return "the code table";
    if (flags & (kTbBlocks | kTbSibling)) return "the block stream";
    if (flags & kTbbStream) return "the pixel stream is short";
    return "unknown";
  }
};

// ---- the 8-bit family's masked form: the same launch set with the mask's workspace behind it (tile_byte_batch.h: TbbMaskBuffers)
struct BytesMaskedBatch : BytesBatch
{
  static constexpr bool kMasked = true;
  static constexpr const char* kName = "masked 8-bit";
  static constexpr const char* kLaunchError = "lerc_amd: a masked 8-bit tile batch kernel could not be launched";
  static constexpr const char* kEncodeScope = "tiles_bytes_masked_encode";
  static constexpr const char* kDecodeScope = "tiles_bytes_masked_decode";

  u32 bitStride, rleStride, pos16Stride;

  BytesMaskedBatch(int dt, int nRows, int nCols, TbStack = { 1, 1 }) : BytesBatch(dt, nRows, nCols)
  {
    const u32 nBytes = (u32)((g.tileElems + 7) >> 3);
    bitStride = (nBytes + 16u + 15u) & ~15u;
    rleStride = (2u * nBytes + 64u + 15u) & ~15u;    // (no stream is longer: MaskedBatch)
    pos16Stride = ((u32)(((nRows + 15) / 16) * ((nCols + 15) / 16)) + 1u + 3u) & ~3u;
  }

  size_t encodeBytesPerTile() const { return BytesBatch::encodeBytesPerTile() + sizeof(TbbMaskRec) + bitStride + rleStride + (size_t)pos16Stride * 4 + 32; }
  size_t decodeBytesPerTile() const { return BytesBatch::decodeBytesPerTile() + sizeof(TbbMaskRec) + bitStride + (size_t)g.tileElems + 32; }

  void* carveEncode(Context& ctx, size_t n)
  {
    void* rec = BytesBatch::carveEncode(ctx, n);
    eb.m.rec = ctx.allocT<TbbMaskRec>(n);
    eb.m.bits = ctx.allocT<u8>(n * bitStride);
    eb.m.rle = ctx.allocT<u8>(n * rleStride);
    eb.m.blockOff16 = ctx.allocT<u32>(n * pos16Stride);
    eb.m.bitStride = bitStride; eb.m.rleStride = rleStride; eb.m.pos16Stride = pos16Stride;
    return (eb.m.rec && eb.m.bits && eb.m.rle && eb.m.blockOff16) ? rec : nullptr;
  }
  void* carveDecode(Context& ctx, size_t n)
  {
    void* rec = BytesBatch::carveDecode(ctx, n);
    db.m.rec = ctx.allocT<TbbMaskRec>(n);
    db.m.bits = ctx.allocT<u8>(n * bitStride);
    db.m.sym = ctx.allocT<u8>(n * (size_t)g.tileElems);
    db.m.bitStride = bitStride; db.m.rleStride = 0;
    return (db.m.rec && db.m.bits && db.m.sym) ? rec : nullptr;
  }
  void launchEncode(u32 n, double maxZErr, const void* dTiles, const u8* dValid, u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile,
                    hipStream_t st)
  {
    eb.m.valid = const_cast<u8*>(dValid);    // (read only: k_tbb_stats)
    BytesBatch::launchEncode(n, maxZErr, dTiles, dValid, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, st);
  }
  void launchDecode(u32 n, const u8* dArena, const u64* dOff, const u32* dSize, void* dTiles, u8* dValid, hipStream_t st)
  {
    db.m.valid = dValid;
    BytesBatch::launchDecode(n, dArena, dOff, dSize, dTiles, dValid, st);
  }

  static const char* reason(u32 flags)
  {
    if (flags & kTbbConst) return "a constant tile";
    if (flags & kTbbRle) return "the mask's run-length stream outgrew its scratch";
    if (flags & kTbbMaskStream) return "the mask's run-length stream is damaged";
    return BytesBatch::reason(flags);
  }
};

// ---- the 8-bit family over band stacks: the masked form's kernels over planes (tile_byte_batch.h), nMasks 0 or 1.  Without masks
// the planes run under one mask of all ones.  A band of a kind this family hands back takes its whole tile with it.
struct BytesBandsBatch : BytesMaskedBatch
{
  static constexpr const char* kName = "8-bit band stack";
  static constexpr const char* kLaunchError = "lerc_amd: an 8-bit band stack tile batch kernel could not be launched";
  static constexpr const char* kEncodeScope = "tiles_bytes_bands_encode";
  static constexpr const char* kDecodeScope = "tiles_bytes_bands_decode";

  int nBands, nMasks;
  u8* ones = nullptr;         // encode without masks: tileElems bytes of 1
  u64* planeOff = nullptr;    // decode: [planes], k_tbbd_chain's
  u32* planeSize = nullptr;

  BytesBandsBatch(int dt, int nRows, int nCols, TbStack s) : BytesMaskedBatch(dt, nRows, nCols), nBands(s.nBands), nMasks(s.nMasks) {}

  size_t encodeBytesPerTile() const { return (size_t)nBands * BytesMaskedBatch::encodeBytesPerTile(); }
  size_t decodeBytesPerTile() const { return (size_t)nBands * (BytesMaskedBatch::decodeBytesPerTile() + 16); }
  size_t encodeBytesPerBatch() const { return nMasks ? 0 : (size_t)g.tileElems + 64; }

  void* carveEncode(Context& ctx, size_t n)
  {
    void* rec = BytesMaskedBatch::carveEncode(ctx, n * (size_t)nBands);
    if (!nMasks) { ones = ctx.allocT<u8>((size_t)g.tileElems); if (!ones) return nullptr; }
    return rec;
  }
  void* carveDecode(Context& ctx, size_t n)
  {
    void* rec = BytesMaskedBatch::carveDecode(ctx, n * (size_t)nBands);
    planeOff = ctx.allocT<u64>(n * (size_t)nBands);
    planeSize = ctx.allocT<u32>(n * (size_t)nBands);
    return (planeOff && planeSize) ? rec : nullptr;
  }
  void launchEncode(u32 n, double, const void* dTiles, const u8* dValid, u8* dArena, u64 arenaBase, u64 arenaCapacity, u64 slotBytes, u64 firstTile,
                    hipStream_t st)
  {
    g.nTiles = n * (u32)nBands;
    BandParams bp = tbFillBandParams(g, 8);    // (lossless: the header says 0.5)
    bp.allValid = 1;
    bp.maxQ = maxValToQuantize(g.dt);
    bp.maxZErr = 0.5; bp.scale = 1.0; bp.invScale = 1.0;
    bp.intLossless = 1;
    if (!nMasks) hipMemsetAsync(ones, 1, (size_t)g.tileElems, st);
    eb.m.valid = nMasks ? const_cast<u8*>(dValid) : ones;    // (read only: k_tbb_stats)
    launchTbbEncodeBands(g, (u32)nBands, bp, dTiles, nMasks ? g.tileElems : 0, dArena, arenaBase, arenaCapacity, slotBytes, firstTile, eb, st);
  }
  void launchDecode(u32 n, const u8* dArena, const u64* dOff, const u32* dSize, void* dTiles, u8* dValid, hipStream_t st)
  {
    g.nTiles = n * (u32)nBands;
    db.m.valid = nMasks ? dValid : nullptr;
    launchTbbDecodeBands(g, (u32)nBands, dArena, dOff, dSize, planeOff, planeSize, dTiles, db, st);
  }

  static const char* reason(u32 flags)
  {
    if (flags == kTbBand) return "another band of the tile";
    return BytesMaskedBatch::reason(flags & ~kTbBand);
  }
};

// ================================================================================================
// the driver
// ================================================================================================
// tiles per sub-batch: a tile is a blockIdx.y, at most 65535 of them per launch, and 256 MiB of workspace (perBatch of it needed once).
// LERC_AMD_TEST_TILE_SUBBATCH=n (tests only, read per call) makes it n, so that a handful of tiles takes several sub-batches.
static const size_t kTbWorkspace = (size_t)256 << 20;
static const size_t kTbMaxPlanes = 65535;

// one tile's planes fit a launch's grid and the workspace; where not, the tiles go one by one
static bool tbTileFits(size_t perTile, size_t perBatch, int nBands) { return (size_t)nBands <= kTbMaxPlanes && perTile + perBatch <= kTbWorkspace; }

static int tbMaxBatch(int nTiles, size_t perTile, size_t perBatch, int nBands)
{
  size_t most = std::min<size_t>(kTbMaxPlanes / (size_t)nBands, (kTbWorkspace - perBatch) / perTile);    // (a band stack's planes are blockIdx.y each)
  const char* e = getenv("LERC_AMD_TEST_TILE_SUBBATCH");
  const long knob = e ? strtol(e, nullptr, 0) : 0;
  if (knob >= 1) most = std::min<size_t>(most, (size_t)knob);
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)nTiles, most));
}

static const TileBatchRec& tbRec(const u8* recs, size_t stride, int i) { return *reinterpret_cast<const TileBatchRec*>(recs + (size_t)i * stride); }

// per sub-batch, the first tile handed back
template<class F>
static void tbNote(Context& ctx, int tile, const char* what, u32 flags)
{
  char msg[192];
  snprintf(msg, sizeof(msg), "tile %d of the %s batch is %s by itself: %s (reason bits 0x%x)", tile, F::kName, what, F::reason(flags), flags);
  ctx.lastNote = msg;
}

// a tile's planes folded: all their flags (0: the batch did every band), the band that says why -- the first with a reason of its own
struct TbFold { u32 flags; int band; u32 bandFlags; };
static TbFold tbFold(const u8* recs, size_t stride, int tile, int nBands)
{
  TbFold f = { 0u, -1, 0u };
  for (int k = 0; k < nBands; k++)
  {
    const u32 fl = tbRec(recs, stride, tile * nBands + k).flags;
    f.flags |= fl;
    if (fl && (f.band < 0 || (f.bandFlags == kTbBand && fl != kTbBand))) { f.band = k; f.bandFlags = fl; }
  }
  return f;
}

template<class F>
static void tbNoteBand(Context& ctx, int tile, const TbFold& f, const char* what)
{
  char msg[224];
  snprintf(msg, sizeof(msg), "tile %d of the %s batch is %s by itself, all its bands: band %d, %s (reason bits 0x%x)", tile, F::kName, what, f.band,
           F::reason(f.bandFlags), f.bandFlags);
  ctx.lastNote = msg;
}

// every tile went one by one because of its size alone: said last, behind whatever the single encoder / decoder noted
static void tbNoteSize(Context& ctx, int nRows, int nCols, const char* what)
{
  if (tbShapeFits(nRows, nCols)) return;
  char msg[224];
  snprintf(msg, sizeof(msg), "every tile of the batch is %s by itself: the size, %d x %d pixels, is beyond what the tile batches take (%u pixels and %u blocks of 8 x 8)",
           what, nRows, nCols, kTbMaxPixels, kTbMaxBlocks);
  ctx.lastNote = msg;
}

// batchOk == false: every tile one by one (a request the family's kernels do not take)
template<class F>
static u32 tbEncode(Context& ctx, const TilesEncodeRequest& rq, u64& arenaUsed, bool batchOk)
{
  arenaUsed = 0;
  const bool slotted = rq.slotBytes != 0;
  const int tb = dtSize(rq.dt);
  const int nB = rq.nBands, nM = rq.nMasks >= 0 ? rq.nMasks : (F::kMasked ? 1 : 0);
  const u64 tileElems = (u64)rq.nRows * (u64)rq.nCols, tileBytes = tileElems * (u64)tb * (u64)nB * (u64)rq.nDepth, maskBytes = tileElems * (u64)nM;
  u64 end = 0;    // arena bytes in use

  auto encodeOne = [&](int t) -> u32
  {
    end = slotted ? (u64)t * rq.slotBytes : (end + 15) & ~15ull;
    EncodeRequest one;
    one.dData = (const u8*)rq.dData + (size_t)t * tileBytes;
    one.dt = rq.dt; one.nDepth = rq.nDepth; one.nCols = rq.nCols; one.nRows = rq.nRows; one.nBands = nB; one.nMasks = nM;
    one.dValidBytes = nM ? rq.dValidBytes + (size_t)t * maskBytes : nullptr;
    one.maxZErr = rq.maxZErr;
    one.dOut = rq.dArena + end;
    one.outCapacity = (u32)std::min<u64>(slotted ? rq.slotBytes : (rq.arenaCapacity > end ? rq.arenaCapacity - end : 0), 0xFFFFFFFFull);
    u32 needed = 0, written = 0;
    const u32 rc = encodeDevice(ctx, one, needed, written);
    if (rc != kOk) return rc;
    rq.hOffsets[t] = end; rq.hSizes[t] = written;
    end += written;
    ctx.tileBatchCount[1]++;
    return kOk;
  };

  if (slotted && rq.arenaCapacity < (u64)rq.nTiles * rq.slotBytes) return kBufferTooSmall;
  auto oneByOne = [&]() -> u32
  {
    for (int t = 0; t < rq.nTiles; t++) { const u32 rc = encodeOne(t); if (rc != kOk) return rc; }
    arenaUsed = slotted ? (u64)rq.nTiles * rq.slotBytes : end;
    return kOk;
  };
  if (!batchOk)
  {
    const u32 rc = oneByOne();
    if (rc == kOk) tbNoteSize(ctx, rq.nRows, rq.nCols, "encoded");    // (a failure keeps what the single encoder said about it)
    return rc;
  }

  hipStream_t st = ctx.activeStream();
  F f(rq.dt, rq.nRows, rq.nCols, TbStack{ nB, nM, rq.nDepth });
  const size_t perTile = f.encodeBytesPerTile(), perBatch = f.encodeBytesPerBatch();
  if (!tbTileFits(perTile, perBatch, nB)) return oneByOne();
  const int maxBatch = tbMaxBatch(rq.nTiles, perTile, perBatch, nB);
  std::vector<int> redo;
  for (int t0 = 0; t0 < rq.nTiles; t0 += maxBatch)
  {
    const int n = std::min(maxBatch, rq.nTiles - t0);
    ctx.reset();
    if (!ctx.reserve((size_t)n * perTile + perBatch + (1u << 16))) return kFailed;
    const size_t recBytes = (size_t)n * (size_t)nB * F::kRecBytes;
    void* rec = f.carveEncode(ctx, (size_t)n);
    u8* pin = (u8*)ctx.pinned(recBytes);
    if (!rec || !pin) return kFailed;
    end = (end + 15) & ~15ull;
    (void)hipGetLastError();
    {
      ProfScope ps(ctx, F::kEncodeScope);
      f.launchEncode((u32)n, rq.maxZErr, (const u8*)rq.dData + (size_t)t0 * tileBytes, nM ? rq.dValidBytes + (size_t)t0 * maskBytes : nullptr,
                     rq.dArena, end, rq.arenaCapacity, rq.slotBytes, (u64)t0, st);
    }
    if (hipGetLastError() != hipSuccess) { ctx.lastError = F::kLaunchError; return kFailed; }
    hipMemcpyAsync(pin, rec, recBytes, hipMemcpyDeviceToHost, st);
    if (!ctx.sync()) return kFailed;
    if (ctx.profOn()) ctx.profCollect();
    redo.clear();
    for (int i = 0; i < n; i++)
    {
      // (a band stack: the tile begins where its first plane does, and is as long as its planes together)
      const TbFold fold = tbFold(pin, F::kRecBytes, i, nB);
      if (fold.flags)
      {
        if (!slotted && (fold.flags & kTbArenaFull)) return kBufferTooSmall;
        if (redo.empty()) { if (nB > 1) tbNoteBand<F>(ctx, t0 + i, fold, "encoded"); else tbNote<F>(ctx, t0 + i, "encoded", fold.flags); }
        redo.push_back(t0 + i);    // (slotted: a tile that does not fit its slot says so when it is encoded by itself)
        continue;
      }
      const u64 offset = tbRec(pin, F::kRecBytes, i * nB).offset;
      u32 blobSize = 0;
      for (int k = 0; k < nB; k++) blobSize += tbRec(pin, F::kRecBytes, i * nB + k).blobSize;
      rq.hOffsets[t0 + i] = offset;
      rq.hSizes[t0 + i] = blobSize;
      // (the arena is in use up to the last byte of the batch's last blob: an arena of exactly that size is enough)
      if (!slotted) end = std::max<u64>(end, offset + blobSize);
      ctx.pathCount[0]++; ctx.tileBatchCount[0]++;
    }
    const std::string note = ctx.lastNote;
    for (int t : redo) { const u32 rc = encodeOne(t); if (rc != kOk) return rc; }    // (reuses the workspace: the batch is done with it)
    if (nB > 1 && !redo.empty()) ctx.lastNote = note;    // (a band stack: the note that names tile and band outlives the single encoder's)
  }
  arenaUsed = slotted ? (u64)rq.nTiles * rq.slotBytes : end;
  return kOk;
}

template<class F>
static u32 tbDecode(Context& ctx, const TilesDecodeRequest& rq, bool batchOk)
{
  const int tb = dtSize(rq.dt);
  const int nB = rq.nBands, nM = rq.nMasks >= 0 ? rq.nMasks : (F::kMasked ? 1 : 0);
  const u64 tileElems = (u64)rq.nRows * (u64)rq.nCols, tileBytes = tileElems * (u64)tb * (u64)nB * (u64)rq.nDepth, maskBytes = tileElems * (u64)nM;
  hipStream_t st = ctx.activeStream();
  u32 firstError = kOk;
  // a tile by itself; one that fails is left zeroed, mask too, and the call goes on with the tiles behind it
  auto decodeOne = [&](int t)
  {
    DecodeRequest one;
    one.dBlob = rq.dArena + rq.hOffsets[t]; one.blobSize = rq.hSizes[t]; one.dt = rq.dt; one.nDepth = rq.nDepth; one.nCols = rq.nCols;
    one.nRows = rq.nRows; one.nBands = nB; one.nMasks = nM;
    one.dValidBytes = nM ? rq.dValidBytes + (size_t)t * maskBytes : nullptr;
    one.dOut = (u8*)rq.dOut + (size_t)t * tileBytes;
    const u32 rc = decodeDevice(ctx, one);
    ctx.tileBatchCount[3]++;
    if (rc != kOk)
    {
      hipStream_t s = ctx.activeStream();
      hipMemsetAsync(one.dOut, 0, (size_t)tileBytes, s);
      if (nM) hipMemsetAsync(one.dValidBytes, 0, (size_t)maskBytes, s);
      hipStreamSynchronize(s);
      if (firstError == kOk) firstError = rc;
    }
  };
  auto oneByOne = [&]() -> u32
  {
    for (int t = 0; t < rq.nTiles; t++) decodeOne(t);
    return firstError;
  };
  if (!batchOk)
  {
    const u32 rc = oneByOne();
    if (rc == kOk) tbNoteSize(ctx, rq.nRows, rq.nCols, "decoded");
    return rc;
  }

  F f(rq.dt, rq.nRows, rq.nCols, TbStack{ nB, nM, rq.nDepth });
  const size_t perTile = f.decodeBytesPerTile();
  if (!tbTileFits(perTile, 0, nB)) return oneByOne();
  const int maxBatch = tbMaxBatch(rq.nTiles, perTile, 0, nB);
  std::vector<int> redo;
  for (int t0 = 0; t0 < rq.nTiles; t0 += maxBatch)
  {
    const int n = std::min(maxBatch, rq.nTiles - t0);
    ctx.reset();
    if (!ctx.reserve((size_t)n * perTile + (1u << 16))) return kFailed;
    void* rec = f.carveDecode(ctx, (size_t)n);
    u64* dOff = ctx.allocT<u64>((size_t)n + 1);
    u32* dSize = ctx.allocT<u32>((size_t)n + 1);
    // (pinned: the tables on their way up, then -- a region of its own -- the records' way back)
    const size_t upBytes = ((size_t)n * 12 + 64 + 63) & ~(size_t)63, recBytes = (size_t)n * (size_t)nB * F::kRecBytes;
    u8* pinUp = (u8*)ctx.pinned(upBytes + recBytes);
    if (!rec || !dOff || !dSize || !pinUp) return kFailed;
    u8* pin = pinUp + upBytes;
    u64* hOff = reinterpret_cast<u64*>(pinUp);
    u32* hSize = reinterpret_cast<u32*>(pinUp + (size_t)n * 8);
    for (int i = 0; i < n; i++) { hOff[i] = rq.hOffsets[t0 + i]; hSize[i] = rq.hSizes[t0 + i]; }
    (void)hipGetLastError();
    hipMemcpyAsync(dOff, hOff, (size_t)n * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(dSize, hSize, (size_t)n * 4, hipMemcpyHostToDevice, st);
    {
      ProfScope ps(ctx, F::kDecodeScope);
      f.launchDecode((u32)n, rq.dArena, dOff, dSize, (u8*)rq.dOut + (size_t)t0 * tileBytes, nM ? rq.dValidBytes + (size_t)t0 * maskBytes : nullptr, st);
    }
    if (hipGetLastError() != hipSuccess) { ctx.lastError = F::kLaunchError; return kFailed; }
    hipMemcpyAsync(pin, rec, recBytes, hipMemcpyDeviceToHost, st);
    if (!ctx.sync()) return kFailed;
    if (ctx.profOn()) ctx.profCollect();
    redo.clear();
    for (int i = 0; i < n; i++)
    {
      const TbFold fold = tbFold(pin, F::kRecBytes, i, nB);
      if (!fold.flags) { ctx.pathCount[2]++; ctx.tileBatchCount[2]++; continue; }
      if (redo.empty()) { if (nB > 1) tbNoteBand<F>(ctx, t0 + i, fold, "decoded"); else tbNote<F>(ctx, t0 + i, "decoded", fold.flags); }
      redo.push_back(t0 + i);
    }
    const std::string note = ctx.lastNote;
    for (int t : redo) decodeOne(t);    // (reuses the workspace: the batch is done with it)
    if (nB > 1 && !redo.empty()) ctx.lastNote = note;
  }
  return firstError;
}

// ================================================================================================
// the calls
// ================================================================================================
u32 encodeTilesDeviceMasked(Context& ctx, const TilesEncodeRequest& rq, u64& arenaUsed)
{
  if (!rq.dValidBytes) return encodeTilesDevice(ctx, rq, arenaUsed);
  arenaUsed = 0;
  if (!rq.dData || !rq.dArena || !rq.hOffsets || !rq.hSizes || rq.nTiles <= 0 || rq.nRows <= 0 || rq.nCols <= 0 || rq.dt < 0 || rq.dt > DT_Double
    || rq.maxZErr < 0 || (rq.slotBytes & 15u) != 0)
    return kWrongParam;
  // (an error bound of 0 on float values is the lossless float mode's business, 777 the bit plane mode's)
  // (8-bit tiles, lossless: the 8-bit family's masked form; from maxZErr 1 on they have no Huffman mode and go one by one)
  if (rq.maxZErr < 1 && tbbShapeOk(rq.dt, rq.nRows, rq.nCols)) return tbEncode<BytesMaskedBatch>(ctx, rq, arenaUsed, true);
  const bool batchOk = tmbShapeOk(rq.dt, rq.nRows, rq.nCols) && rq.maxZErr != 777 && !(rq.dt >= DT_Float && rq.maxZErr == 0);
  return tbEncode<MaskedBatch>(ctx, rq, arenaUsed, batchOk);
}

u32 decodeTilesDeviceMasked(Context& ctx, const TilesDecodeRequest& rq)
{
  if (!rq.dValidBytes) return decodeTilesDevice(ctx, rq);
  if (!rq.dArena || !rq.hOffsets || !rq.hSizes || !rq.dOut || rq.nTiles <= 0 || rq.nRows <= 0 || rq.nCols <= 0 || rq.dt < 0 || rq.dt > DT_Double)
    return kWrongParam;
  if (tbbShapeOk(rq.dt, rq.nRows, rq.nCols)) return tbDecode<BytesMaskedBatch>(ctx, rq, true);
  return tbDecode<MaskedBatch>(ctx, rq, tmbShapeOk(rq.dt, rq.nRows, rq.nCols));
}

// ---- band stacks.  One band: the calls above.  The batch's own launches take the wide types (MaskedBandsBatch) and lossless 8-bit
// stacks (BytesBandsBatch) with no mask or one mask a tile; a mask per band, 8-bit stacks from maxZErr 1 on, the error bounds and sizes
// the masked family leaves alone go one by one, a whole stack per encodeDevice / decodeDevice call.
u32 encodeTilesDeviceBands(Context& ctx, const TilesEncodeRequest& rq, u64& arenaUsed)
{
  arenaUsed = 0;
  if (!rq.dData || !rq.dArena || !rq.hOffsets || !rq.hSizes || rq.nTiles <= 0 || rq.nRows <= 0 || rq.nCols <= 0 || rq.dt < 0 || rq.dt > DT_Double
    || rq.maxZErr < 0 || (rq.slotBytes & 15u) != 0 || rq.nBands <= 0 || (rq.nMasks != 0 && rq.nMasks != 1 && rq.nMasks != rq.nBands)
    || (rq.nMasks == 0) != (rq.dValidBytes == nullptr))
    return kWrongParam;
  if (rq.nBands == 1)
  {
    TilesEncodeRequest one = rq;
    one.nMasks = -1;
    return encodeTilesDeviceMasked(ctx, one, arenaUsed);
  }
  if (rq.nMasks <= 1 && rq.maxZErr < 1 && tbbShapeOk(rq.dt, rq.nRows, rq.nCols)) return tbEncode<BytesBandsBatch>(ctx, rq, arenaUsed, true);
  // (whatever is left of the 8-bit types -- maxZErr >= 1, a mask per band, oversized -- falls through with batchOk false: tmbShapeOk takes
  // no 8-bit type, so MaskedBandsBatch is only the name under which every tile goes one by one; the same on the way back)
  const bool batchOk = rq.nMasks <= 1 && tmbShapeOk(rq.dt, rq.nRows, rq.nCols) && rq.maxZErr != 777 && !(rq.dt >= DT_Float && rq.maxZErr == 0);
  return tbEncode<MaskedBandsBatch>(ctx, rq, arenaUsed, batchOk);
}

u32 decodeTilesDeviceBands(Context& ctx, const TilesDecodeRequest& rq)
{
  if (!rq.dArena || !rq.hOffsets || !rq.hSizes || !rq.dOut || rq.nTiles <= 0 || rq.nRows <= 0 || rq.nCols <= 0 || rq.dt < 0 || rq.dt > DT_Double
    || rq.nBands <= 0 || (rq.nMasks != 0 && rq.nMasks != 1 && rq.nMasks != rq.nBands) || (rq.nMasks == 0) != (rq.dValidBytes == nullptr))
    return kWrongParam;
  if (rq.nBands == 1)
  {
    TilesDecodeRequest one = rq;
    one.nMasks = -1;
    return decodeTilesDeviceMasked(ctx, one);
  }
  if (rq.nMasks <= 1 && tbbShapeOk(rq.dt, rq.nRows, rq.nCols)) return tbDecode<BytesBandsBatch>(ctx, rq, true);
  return tbDecode<MaskedBandsBatch>(ctx, rq, rq.nMasks <= 1 && tmbShapeOk(rq.dt, rq.nRows, rq.nCols));
}

// ---- depth tiles.  One value a pixel: the masked calls.  The batch's own launches take the wide types with 2 .. kTdbMaxDepth values a
// pixel and no mask or one mask a tile; 8-bit tiles (their Huffman modes over depth), deeper tiles, and the error bounds and sizes the
// masked family leaves alone go one by one, a tile per encodeDevice / decodeDevice call with its nDepth.
static const char* tdbWhyNot(int dt, int nDepth, int nRows, int nCols, double maxZErr, bool encode)
{
  if (dt == DT_Char || dt == DT_Byte) return "8-bit values";
  if (nDepth > kTdbMaxDepth) return "more values a pixel than the depth batches take";
  if (!tbShapeFits(nRows, nCols)) return "the size";
  if (encode && maxZErr == 777) return "the bit plane mode's error bound";
  if (encode && dt >= DT_Float && maxZErr == 0) return "an error bound of 0 on float values";
  return nullptr;
}

static void tdbNoteAll(Context& ctx, const char* what, const char* why)
{
  char msg[224];
  snprintf(msg, sizeof(msg), "every tile of the depth batch is %s by itself, from tile 0 on: %s", what, why);
  ctx.lastNote = msg;
}

u32 encodeTilesDeviceDepth(Context& ctx, const TilesEncodeRequest& rq, u64& arenaUsed)
{
  arenaUsed = 0;
  if (!rq.dData || !rq.dArena || !rq.hOffsets || !rq.hSizes || rq.nTiles <= 0 || rq.nRows <= 0 || rq.nCols <= 0 || rq.dt < 0 || rq.dt > DT_Double
    || rq.maxZErr < 0 || (rq.slotBytes & 15u) != 0 || rq.nDepth <= 0)
    return kWrongParam;
  TilesEncodeRequest one = rq;
  one.nBands = 1;
  if (rq.nDepth == 1)
  {
    one.nMasks = -1;
    return encodeTilesDeviceMasked(ctx, one, arenaUsed);
  }
  one.nMasks = rq.dValidBytes ? 1 : 0;
  const char* why = tdbWhyNot(rq.dt, rq.nDepth, rq.nRows, rq.nCols, rq.maxZErr, true);
  const u32 rc = tbEncode<DepthBatch>(ctx, one, arenaUsed, why == nullptr);
  if (why && rc == kOk) tdbNoteAll(ctx, "encoded", why);
  return rc;
}

u32 decodeTilesDeviceDepth(Context& ctx, const TilesDecodeRequest& rq)
{
  if (!rq.dArena || !rq.hOffsets || !rq.hSizes || !rq.dOut || rq.nTiles <= 0 || rq.nRows <= 0 || rq.nCols <= 0 || rq.dt < 0 || rq.dt > DT_Double
    || rq.nDepth <= 0)
    return kWrongParam;
  TilesDecodeRequest one = rq;
  one.nBands = 1;
  if (rq.nDepth == 1)
  {
    one.nMasks = -1;
    return decodeTilesDeviceMasked(ctx, one);
  }
  one.nMasks = rq.dValidBytes ? 1 : 0;
  const char* why = tdbWhyNot(rq.dt, rq.nDepth, rq.nRows, rq.nCols, 0, false);
  const u32 rc = tbDecode<DepthBatch>(ctx, one, why == nullptr);
  if (why && rc == kOk) tdbNoteAll(ctx, "decoded", why);
  return rc;
}

// (encodeTilesDevice / decodeTilesDevice have checked the arguments and the eligibility)
u32 encodeTilesBytes(Context& ctx, const TilesEncodeRequest& rq, u64& arenaUsed) { return tbEncode<BytesBatch>(ctx, rq, arenaUsed, true); }

u32 decodeTilesBytes(Context& ctx, const TilesDecodeRequest& rq) { return tbDecode<BytesBatch>(ctx, rq, true); }

}    // namespace lerc
