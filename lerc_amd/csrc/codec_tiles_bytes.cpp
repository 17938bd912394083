// codec_tiles_bytes.cpp -- host side of the 8-bit tile batches: a mosaic of DT_Char / DT_Byte tiles, every pixel valid, lossless, through
// the tile batch calls in one set of launches and one host wait per sub-batch.  The kernels are in tile_byte_batch.hip.  Tiles the
// kernels hand back (TbbTile::flags) are done one by one behind their sub-batch by encodeDevice / decodeDevice -- byte for byte what
// those calls make, and their exact status.
#include "codec.h"
#include "tile_byte_batch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace lerc {

static bool tbbShapeOk(int dt, int nRows, int nCols)
{
  const u64 nPix = (u64)nRows * (u64)nCols, nPos = (u64)((nRows + 7) / 8) * (u64)((nCols + 7) / 8);
  return (dt == DT_Char || dt == DT_Byte) && nPix <= kTbbMaxPixels && nPos <= kTbbMaxBlocks;
}

bool tilesBytesEncodeEligible(const TilesEncodeRequest& rq)
{
  // (maxZErr < 1 on an integer type is lossless: the header says 0.5.  From 1 on there is no Huffman mode: the general path's business)
  return !rq.dValidBytes && rq.maxZErr < 1 && tbbShapeOk(rq.dt, rq.nRows, rq.nCols);
}

bool tilesBytesDecodeEligible(const TilesDecodeRequest& rq) { return !rq.dValidBytes && tbbShapeOk(rq.dt, rq.nRows, rq.nCols); }

static TbbGeom tbbGeom(int dt, int nRows, int nCols, u32 nTiles)
{
  TbbGeom g;
  memset(&g, 0, sizeof(g));
  g.nRows = nRows; g.nCols = nCols; g.nTV = (nRows + 7) / 8; g.nTH = (nCols + 7) / 8; g.dt = dt;
  g.nTiles = nTiles;
  g.tileElems = (u64)nRows * (u64)nCols;
  g.posStride = ((u32)(g.nTV * g.nTH) + 1u + 3u) & ~3u;
  return g;
}

static const char* tbbReason(u32 flags)
{
  if (flags & kTbbConst) return "a constant tile";
  if (flags & kTbbRetry16) return "the low-bit-rate rule asks for 16 x 16 blocks";
  if (flags & kTbbOneSweep) return "one sweep";
  if (flags & kTbbCapacity) return "the blob does not fit its slot";
  if (flags & kTbbArenaFull) return "the arena is full";
  if (flags & kTbbHeader) return "not a header the batch takes";
  if (flags & kTbbChecksum) return "the checksum differs";
  if (flags & kTbbTable) return "the code table";
  if (flags & (kTbbBlocks | kTbbSibling)) return "the block stream";
  if (flags & kTbbStream) return "the pixel stream is short";
  return "unknown";
}

u32 encodeTilesBytes(Context& ctx, const TilesEncodeRequest& rq, u64& arenaUsed)
{
  arenaUsed = 0;
  const bool slotted = rq.slotBytes != 0;
  const u64 tileElems = (u64)rq.nRows * (u64)rq.nCols;
  u64 end = 0;    // arena bytes in use

  auto encodeOne = [&](int t) -> u32
  {
    end = slotted ? (u64)t * rq.slotBytes : (end + 15) & ~15ull;
    EncodeRequest one;
    one.dData = (const u8*)rq.dData + (size_t)t * tileElems;
    one.dt = rq.dt; one.nDepth = 1; one.nCols = rq.nCols; one.nRows = rq.nRows; one.nBands = 1; one.nMasks = 0; one.dValidBytes = nullptr;
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
  hipStream_t st = ctx.activeStream();
  const TbbGeom g1 = tbbGeom(rq.dt, rq.nRows, rq.nCols, 1);
  const size_t perTile = sizeof(TbbTile) + 512 * 4 + (size_t)g1.posStride * 4 + 256 * 8 + kTbbTableCap;
  // (a tile is a blockIdx.y: at most 65535 of them per launch)
  const int maxBatch = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)rq.nTiles, 65535), ((size_t)256 << 20) / perTile));
  BandParams bp;
  memset(&bp, 0, sizeof(bp));
  bp.nRows = rq.nRows; bp.nCols = rq.nCols; bp.nDepth = 1; bp.dt = rq.dt; bp.version = kCodecVersion;
  bp.mb = 8; bp.nTV = (rq.nRows + 7) / 8; bp.nTH = (rq.nCols + 7) / 8;
  bp.allValid = 1;
  bp.maxQ = maxValToQuantize(rq.dt);
  bp.maxZErr = 0.5; bp.scale = 1.0; bp.invScale = 1.0;
  bp.intLossless = 1;

  std::vector<int> redo;
  for (int t0 = 0; t0 < rq.nTiles; t0 += maxBatch)
  {
    const int n = std::min(maxBatch, rq.nTiles - t0);
    const TbbGeom g = tbbGeom(rq.dt, rq.nRows, rq.nCols, (u32)n);
    ctx.reset();
    if (!ctx.reserve((size_t)n * perTile + (1u << 16))) return kFailed;
    TbbEncodeBuffers b;
    const size_t recBytes = (size_t)n * sizeof(TbbTile);
    b.tiles = ctx.allocT<TbbTile>((size_t)n);
    b.histo = ctx.allocT<u32>((size_t)n * 512);
    b.blockOff = ctx.allocT<u32>((size_t)n * g.posStride);
    b.codes = ctx.allocT<u64>((size_t)n * 256);
    b.table = ctx.allocT<u8>((size_t)n * kTbbTableCap);
    u8* pin = (u8*)ctx.pinned(recBytes);
    if (!b.tiles || !b.histo || !b.blockOff || !b.codes || !b.table || !pin) return kFailed;
    end = (end + 15) & ~15ull;
    (void)hipGetLastError();
    {
      ProfScope ps(ctx, "tiles_bytes_encode");
      launchTbbEncode(g, bp, (const u8*)rq.dData + (size_t)t0 * tileElems, rq.dArena, end, rq.arenaCapacity, rq.slotBytes, (u64)t0, b, st);
    }
    if (hipGetLastError() != hipSuccess) { ctx.lastError = "lerc_amd: an 8-bit tile batch kernel could not be launched"; return kFailed; }
    hipMemcpyAsync(pin, b.tiles, recBytes, hipMemcpyDeviceToHost, st);
    if (!ctx.sync()) return kFailed;
    if (ctx.profOn()) ctx.profCollect();
    const TbbTile* res = reinterpret_cast<const TbbTile*>(pin);
    redo.clear();
    for (int i = 0; i < n; i++)
    {
      if (res[i].flags)
      {
        if (!slotted && (res[i].flags & kTbbArenaFull)) return kBufferTooSmall;
        char msg[160];
        snprintf(msg, sizeof(msg), "tile %d of the 8-bit batch is encoded by itself: %s (reason bits 0x%x)", t0 + i, tbbReason(res[i].flags), res[i].flags);
        ctx.lastNote = msg;
        redo.push_back(t0 + i);    // (slotted: a tile that does not fit its slot says so when it is encoded by itself)
        continue;
      }
      rq.hOffsets[t0 + i] = res[i].offset;
      rq.hSizes[t0 + i] = res[i].blobSize;
      ctx.pathCount[0]++; ctx.tileBatchCount[0]++;
    }
    // (the arena is in use up to the last byte of the batch's last blob: an arena of exactly that size is enough)
    if (!slotted) for (int i = 0; i < n; i++) if (!res[i].flags) end = std::max<u64>(end, res[i].offset + res[i].blobSize);
    for (int t : redo) { const u32 rc = encodeOne(t); if (rc != kOk) return rc; }    // (reuses the workspace: the batch is done with it)
  }
  arenaUsed = slotted ? (u64)rq.nTiles * rq.slotBytes : end;
  return kOk;
}

u32 decodeTilesBytes(Context& ctx, const TilesDecodeRequest& rq)
{
  const u64 tileElems = (u64)rq.nRows * (u64)rq.nCols;
  hipStream_t st = ctx.activeStream();
  u32 firstError = kOk;
  // a tile by itself; one that fails is left zeroed, and the call goes on with the tiles behind it
  auto decodeOne = [&](int t)
  {
    DecodeRequest one;
    one.dBlob = rq.dArena + rq.hOffsets[t]; one.blobSize = rq.hSizes[t]; one.dt = rq.dt; one.nDepth = 1; one.nCols = rq.nCols;
    one.nRows = rq.nRows; one.nBands = 1; one.nMasks = 0; one.dValidBytes = nullptr;
    one.dOut = (u8*)rq.dOut + (size_t)t * tileElems;
    const u32 rc = decodeDevice(ctx, one);
    ctx.tileBatchCount[3]++;
    if (rc != kOk)
    {
      hipStream_t s = ctx.activeStream();
      hipMemsetAsync(one.dOut, 0, (size_t)tileElems, s);
      hipStreamSynchronize(s);
      if (firstError == kOk) firstError = rc;
    }
  };

  const TbbGeom g1 = tbbGeom(rq.dt, rq.nRows, rq.nCols, 1);
  const size_t perTile = sizeof(TbbTile) + (size_t)g1.posStride * 4 + 256 * 4 + 256 + 16;
  const int maxBatch = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)rq.nTiles, 65535), ((size_t)256 << 20) / perTile));
  std::vector<int> redo;
  for (int t0 = 0; t0 < rq.nTiles; t0 += maxBatch)
  {
    const int n = std::min(maxBatch, rq.nTiles - t0);
    const TbbGeom g = tbbGeom(rq.dt, rq.nRows, rq.nCols, (u32)n);
    ctx.reset();
    if (!ctx.reserve((size_t)n * perTile + (1u << 16))) return kFailed;
    TbbDecodeBuffers b;
    b.tiles = ctx.allocT<TbbTile>((size_t)n);
    b.blockOff = ctx.allocT<u32>((size_t)n * g.posStride);
    b.codes = ctx.allocT<u32>((size_t)n * 256);
    b.lens = ctx.allocT<u8>((size_t)n * 256);
    u64* dOff = ctx.allocT<u64>((size_t)n + 1);
    u32* dSize = ctx.allocT<u32>((size_t)n + 1);
    // (pinned: the tables on their way up, then -- a region of its own -- the records' way back)
    const size_t upBytes = ((size_t)n * 12 + 64 + 63) & ~(size_t)63, recBytes = (size_t)n * sizeof(TbbTile);
    u8* pinUp = (u8*)ctx.pinned(upBytes + recBytes);
    if (!b.tiles || !b.blockOff || !b.codes || !b.lens || !dOff || !dSize || !pinUp) return kFailed;
    u8* pin = pinUp + upBytes;
    u64* hOff = reinterpret_cast<u64*>(pinUp);
    u32* hSize = reinterpret_cast<u32*>(pinUp + (size_t)n * 8);
    for (int i = 0; i < n; i++) { hOff[i] = rq.hOffsets[t0 + i]; hSize[i] = rq.hSizes[t0 + i]; }
    (void)hipGetLastError();
    hipMemcpyAsync(dOff, hOff, (size_t)n * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(dSize, hSize, (size_t)n * 4, hipMemcpyHostToDevice, st);
    {
      ProfScope ps(ctx, "tiles_bytes_decode");
      launchTbbDecode(g, rq.dArena, dOff, dSize, (u8*)rq.dOut + (size_t)t0 * tileElems, b, st);
    }
    if (hipGetLastError() != hipSuccess) { ctx.lastError = "lerc_amd: an 8-bit tile batch kernel could not be launched"; return kFailed; }
    hipMemcpyAsync(pin, b.tiles, recBytes, hipMemcpyDeviceToHost, st);
    if (!ctx.sync()) return kFailed;
    if (ctx.profOn()) ctx.profCollect();
    const TbbTile* res = reinterpret_cast<const TbbTile*>(pin);
    redo.clear();
    for (int i = 0; i < n; i++)
    {
      if (!res[i].flags) { ctx.pathCount[2]++; ctx.tileBatchCount[2]++; continue; }
      char msg[160];
      snprintf(msg, sizeof(msg), "tile %d of the 8-bit batch is decoded by itself: %s (reason bits 0x%x)", t0 + i, tbbReason(res[i].flags), res[i].flags);
      ctx.lastNote = msg;
      redo.push_back(t0 + i);
    }
    for (int t : redo) decodeOne(t);    // (reuses the workspace: the batch is done with it)
  }
  return firstError;
}

}    // namespace lerc
