// codec_tiles_masked.cpp -- host side of the masked tile batches: a mosaic's tiles AND their validity masks in one call
// (lerc_amd_encode_tiles_device_masked / lerc_amd_decode_tiles_device_masked).  The kernels are in tile_mask_batch.hip; one
// host wait per sub-batch.  Tiles the kernels hand back (TmbTile::flags) are done one by one behind their sub-batch by
// encodeDevice / decodeDevice with the tile's mask -- byte for byte what those calls make, and their exact status.
#include "codec.h"
#include "tile_mask_batch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace lerc {

static bool tmbShapeOk(int dt, int nRows, int nCols)
{
  const u64 nPix = (u64)nRows * (u64)nCols, nPos = (u64)((nRows + 7) / 8) * (u64)((nCols + 7) / 8);
  return dt >= DT_Short && dt <= DT_Double && nPix <= (u64)kTmbMaxMaskBytes * 8u && nPos <= kTmbMaxBlocks;
}

static TmbGeom tmbGeom(int dt, int nRows, int nCols, u32 nTiles)
{
  TmbGeom g;
  memset(&g, 0, sizeof(g));
  g.nRows = nRows; g.nCols = nCols; g.nTV = (nRows + 7) / 8; g.nTH = (nCols + 7) / 8; g.dt = dt;
  g.nTiles = nTiles;
  g.tileElems = (u64)nRows * (u64)nCols;
  const u32 nBytes = (u32)((g.tileElems + 7) >> 3);
  g.bitStride = (nBytes + 16u + 15u) & ~15u;
  g.rleStride = (2u * nBytes + 64u + 15u) & ~15u;    // (no stream is longer: a literal byte costs 1 + 2 / 32767, a run of five 3)
  g.posStride = ((u32)(g.nTV * g.nTH) + 1u + 3u) & ~3u;
  g.pos16Stride = ((u32)(((nRows + 15) / 16) * ((nCols + 15) / 16)) + 1u + 3u) & ~3u;
  return g;
}

u32 encodeTilesDeviceMasked(Context& ctx, const TilesEncodeRequest& rq, u64& arenaUsed)
{
  if (!rq.dValidBytes) return encodeTilesDevice(ctx, rq, arenaUsed);
  arenaUsed = 0;
  if (!rq.dData || !rq.dArena || !rq.hOffsets || !rq.hSizes || rq.nTiles <= 0 || rq.nRows <= 0 || rq.nCols <= 0 || rq.dt < 0 || rq.dt > DT_Double
    || rq.maxZErr < 0 || (rq.slotBytes & 15u) != 0)
    return kWrongParam;
  const bool slotted = rq.slotBytes != 0;
  const int tb = dtSize(rq.dt);
  const u64 tileElems = (u64)rq.nRows * (u64)rq.nCols;
  const bool isFlt = rq.dt >= DT_Float;
  // (an error bound of 0 on float values is the lossless float mode's business, 777 the bit plane mode's)
  const bool batchOk = tmbShapeOk(rq.dt, rq.nRows, rq.nCols) && rq.maxZErr != 777 && !(isFlt && rq.maxZErr == 0);
  u64 end = 0;    // arena bytes in use

  auto encodeOne = [&](int t) -> u32
  {
    end = slotted ? (u64)t * rq.slotBytes : (end + 15) & ~15ull;
    EncodeRequest one;
    one.dData = (const u8*)rq.dData + (size_t)t * tileElems * tb;
    one.dt = rq.dt; one.nDepth = 1; one.nCols = rq.nCols; one.nRows = rq.nRows; one.nBands = 1; one.nMasks = 1;
    one.dValidBytes = rq.dValidBytes + (size_t)t * tileElems;
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
  if (!batchOk)
  {
    for (int t = 0; t < rq.nTiles; t++) { const u32 rc = encodeOne(t); if (rc != kOk) return rc; }
    arenaUsed = slotted ? (u64)rq.nTiles * rq.slotBytes : end;
    return kOk;
  }

  hipStream_t st = ctx.activeStream();
  const TmbGeom g1 = tmbGeom(rq.dt, rq.nRows, rq.nCols, 1);
  const size_t perTile = sizeof(TmbTile) + g1.bitStride + g1.rleStride + ((size_t)g1.posStride + g1.pos16Stride) * 4;
  // (a tile is a blockIdx.y: at most 65535 of them per launch)
  const int maxBatch = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)rq.nTiles, 65535), ((size_t)256 << 20) / perTile));
  u32 cand = 0;
  if (isFlt)
  {
    static const double errCand[9] = { 1, 0.5, 0.1, 0.05, 0.01, 0.005, 0.001, 0.0005, 0.0001 };
    for (int c = 0; c < 9; c++) if (errCand[c] / 2 > rq.maxZErr) cand |= 1u << c;
  }
  BandParams bp;
  memset(&bp, 0, sizeof(bp));
  bp.nRows = rq.nRows; bp.nCols = rq.nCols; bp.nDepth = 1; bp.dt = rq.dt; bp.version = kCodecVersion;
  bp.mb = 8; bp.nTV = (rq.nRows + 7) / 8; bp.nTH = (rq.nCols + 7) / 8;
  bp.maxQ = maxValToQuantize(rq.dt);
  bp.maxZErr = isFlt ? rq.maxZErr : std::max(0.5, floor(rq.maxZErr));
  bp.scale = 1 / (2 * bp.maxZErr);
  bp.invScale = 2 * bp.maxZErr;
  bp.intLossless = (!isFlt && bp.maxZErr == 0.5) ? 1 : 0;

  std::vector<int> redo;
  for (int t0 = 0; t0 < rq.nTiles; t0 += maxBatch)
  {
    const int n = std::min(maxBatch, rq.nTiles - t0);
    const TmbGeom g = tmbGeom(rq.dt, rq.nRows, rq.nCols, (u32)n);
    ctx.reset();
    if (!ctx.reserve((size_t)n * perTile + (1u << 16))) return kFailed;
    TmbEncodeBuffers b;
    const size_t recBytes = (size_t)n * sizeof(TmbTile);
    u8* rec = ctx.allocT<u8>(recBytes);
    b.tiles = reinterpret_cast<TmbTile*>(rec);
    b.bits = ctx.allocT<u8>((size_t)n * g.bitStride);
    b.rle = ctx.allocT<u8>((size_t)n * g.rleStride);
    b.blockOff = ctx.allocT<u32>((size_t)n * g.posStride);
    b.blockOff16 = ctx.allocT<u32>((size_t)n * g.pos16Stride);
    u8* pin = (u8*)ctx.pinned(recBytes);
    if (!rec || !b.bits || !b.rle || !b.blockOff || !b.blockOff16 || !pin) return kFailed;
    end = (end + 15) & ~15ull;
    (void)hipGetLastError();
    {
      ProfScope ps(ctx, "tiles_masked_encode");
      launchTmbEncode(g, bp, bp.maxZErr, cand, (const u8*)rq.dData + (size_t)t0 * tileElems * tb, rq.dValidBytes + (size_t)t0 * tileElems,
                      rq.dArena, end, rq.arenaCapacity, rq.slotBytes, (u64)t0, b, st);
    }
    if (hipGetLastError() != hipSuccess) { ctx.lastError = "lerc_amd: a masked tile batch kernel could not be launched"; return kFailed; }
    hipMemcpyAsync(pin, rec, recBytes, hipMemcpyDeviceToHost, st);
    if (!ctx.sync()) return kFailed;
    if (ctx.profOn()) ctx.profCollect();
    const TmbTile* res = reinterpret_cast<const TmbTile*>(pin);
    redo.clear();
    for (int i = 0; i < n; i++)
    {
      if (res[i].flags)
      {
        if (!slotted && (res[i].flags & kTmbArenaFull)) return kBufferTooSmall;
        if (redo.empty())
        {
          char msg[128];
          snprintf(msg, sizeof(msg), "tile %d of the masked batch is encoded by itself (reason bits 0x%x)", t0 + i, res[i].flags);
          ctx.lastNote = msg;
        }
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

u32 decodeTilesDeviceMasked(Context& ctx, const TilesDecodeRequest& rq)
{
  if (!rq.dValidBytes) return decodeTilesDevice(ctx, rq);
  if (!rq.dArena || !rq.hOffsets || !rq.hSizes || !rq.dOut || rq.nTiles <= 0 || rq.nRows <= 0 || rq.nCols <= 0 || rq.dt < 0 || rq.dt > DT_Double)
    return kWrongParam;
  const int tb = dtSize(rq.dt);
  const u64 tileElems = (u64)rq.nRows * (u64)rq.nCols;
  hipStream_t st = ctx.activeStream();
  u32 firstError = kOk;
  // a tile by itself; one that fails is left zeroed, mask too, and the call goes on with the tiles behind it
  auto decodeOne = [&](int t)
  {
    DecodeRequest one;
    one.dBlob = rq.dArena + rq.hOffsets[t]; one.blobSize = rq.hSizes[t]; one.dt = rq.dt; one.nDepth = 1; one.nCols = rq.nCols;
    one.nRows = rq.nRows; one.nBands = 1; one.nMasks = 1;
    one.dValidBytes = rq.dValidBytes + (size_t)t * tileElems;
    one.dOut = (u8*)rq.dOut + (size_t)t * tileElems * tb;
    const u32 rc = decodeDevice(ctx, one);
    ctx.tileBatchCount[3]++;
    if (rc != kOk)
    {
      hipStream_t s = ctx.activeStream();
      hipMemsetAsync(one.dOut, 0, (size_t)tileElems * tb, s);
      hipMemsetAsync(one.dValidBytes, 0, (size_t)tileElems, s);
      hipStreamSynchronize(s);
      if (firstError == kOk) firstError = rc;
    }
  };
  if (!tmbShapeOk(rq.dt, rq.nRows, rq.nCols))
  {
    for (int t = 0; t < rq.nTiles; t++) decodeOne(t);
    return firstError;
  }

  const TmbGeom g1 = tmbGeom(rq.dt, rq.nRows, rq.nCols, 1);
  const size_t perTile = sizeof(TmbTile) + g1.bitStride + (size_t)g1.posStride * 4 + 16;
  const int maxBatch = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)rq.nTiles, 65535), ((size_t)256 << 20) / perTile));
  std::vector<int> redo;
  for (int t0 = 0; t0 < rq.nTiles; t0 += maxBatch)
  {
    const int n = std::min(maxBatch, rq.nTiles - t0);
    const TmbGeom g = tmbGeom(rq.dt, rq.nRows, rq.nCols, (u32)n);
    ctx.reset();
    if (!ctx.reserve((size_t)n * perTile + (1u << 16))) return kFailed;
    TmbDecodeBuffers b;
    b.tiles = ctx.allocT<TmbTile>((size_t)n);
    b.bits = ctx.allocT<u8>((size_t)n * g.bitStride);
    b.blockOff = ctx.allocT<u32>((size_t)n * g.posStride);
    u64* dOff = ctx.allocT<u64>((size_t)n + 1);
    u32* dSize = ctx.allocT<u32>((size_t)n + 1);
    // (pinned: the tables on their way up, then -- a region of its own -- the records' way back)
    const size_t upBytes = ((size_t)n * 12 + 64 + 63) & ~(size_t)63, recBytes = (size_t)n * sizeof(TmbTile);
    u8* pinUp = (u8*)ctx.pinned(upBytes + recBytes);
    if (!b.tiles || !b.bits || !b.blockOff || !dOff || !dSize || !pinUp) return kFailed;
    u8* pin = pinUp + upBytes;
    u64* hOff = reinterpret_cast<u64*>(pinUp);
    u32* hSize = reinterpret_cast<u32*>(pinUp + (size_t)n * 8);
    for (int i = 0; i < n; i++) { hOff[i] = rq.hOffsets[t0 + i]; hSize[i] = rq.hSizes[t0 + i]; }
    (void)hipGetLastError();
    hipMemcpyAsync(dOff, hOff, (size_t)n * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(dSize, hSize, (size_t)n * 4, hipMemcpyHostToDevice, st);
    {
      ProfScope ps(ctx, "tiles_masked_decode");
      launchTmbDecode(g, rq.dArena, dOff, dSize, (u8*)rq.dOut + (size_t)t0 * tileElems * tb, rq.dValidBytes + (size_t)t0 * tileElems, b, st);
    }
    if (hipGetLastError() != hipSuccess) { ctx.lastError = "lerc_amd: a masked tile batch kernel could not be launched"; return kFailed; }
    hipMemcpyAsync(pin, b.tiles, recBytes, hipMemcpyDeviceToHost, st);
    if (!ctx.sync()) return kFailed;
    if (ctx.profOn()) ctx.profCollect();
    const TmbTile* res = reinterpret_cast<const TmbTile*>(pin);
    redo.clear();
    for (int i = 0; i < n; i++)
    {
      if (!res[i].flags) { ctx.pathCount[2]++; ctx.tileBatchCount[2]++; continue; }
      if (redo.empty())
      {
        char msg[128];
        snprintf(msg, sizeof(msg), "tile %d of the masked batch is decoded by itself (reason bits 0x%x)", t0 + i, res[i].flags);
        ctx.lastNote = msg;
      }
      redo.push_back(t0 + i);
    }
    for (int t : redo) decodeOne(t);    // (reuses the workspace: the batch is done with it)
  }
  return firstError;
}

}    // namespace lerc
