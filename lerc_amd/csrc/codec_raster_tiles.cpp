// codec_raster_tiles.cpp -- a pitched device raster in, a grid of tile blobs out, and back (lerc_amd_encode_raster_tiles_device /
// lerc_amd_decode_raster_tiles_device).  The reference has no counterpart: a tiled-LERC writer (MRF, a tile cache) cuts the raster on
// the host and calls lerc_encode per tile.
//
// A grid has at most four shape classes -- interior, right column, bottom row, corner --, and a class is a mosaic of one shape, which
// is what the tile batch calls take.  Per class, in chunks that fit the staging buffer: k_rt_cut gathers the chunk's rectangles into
// [n][nBands][r][c] (the mask's into [n][r][c]), the chunk goes to encodeTilesDevice (one band, no mask: the one-launch tile encoder),
// encodeTilesDeviceMasked (one band, a mask) or encodeTilesDeviceBands with the arena pointed at the bytes still free (the class's run
// of rooms, if slotted), and its offsets and sizes are scattered into the caller's arrays by tile index.  The way back gathers the
// tables, decodes into the staging buffer and pastes.  Size limits, hand-backs, notes, lerc_amd_tile_batch_counters and the status of a
// failing tile are those calls' own.  Tiles that lie as [n][r][c] already (one band, a tile as wide as the raster, no padding) are handed
// over where they lie.  A pixel-interleaved raster (pixelPitch >= 2, the _strided calls) differs in the kernels that cut and paste its
// data, k_rt_cut_px / k_rt_paste_px (raster_tiles_px.hip), and in nothing else: same staging buffer, same chunks, same counters; it is
// never coded where it lies.
//
// Both ways take a RANGE of the grid's tiles (RasterTilesRequest: the whole grid by default; lerc_amd_encode_raster_tiles_device_range
// names one): every class is cut down to it, which leaves classes, so nothing behind rtGrid knows about ranges but the tables' indices
// and the slots' count.  lerc_amd_decode_raster_window_device is the decode of the range of tiles a window touches into a buffer that
// holds the window only: the same chunks, tables gathered at those tiles alone, the same tile calls into the staging buffer -- and a
// clipped paste behind them, k_rw_paste / k_rw_paste_px (raster_window.hip).
//
// A DEPTH raster (nDepth > 1, lerc_amd_depth.h) is one band whose tiles are staged as [n][r][c][nDepth] and handed to
// encodeTilesDeviceDepth / decodeTilesDeviceDepth; it differs in how it is cut and pasted, and in nothing else, ranges and windows
// included.  Packed pixels are runs of elements: the band kernels with the column counts scaled by nDepth (a window's too).  Gapped
// pixels, planes and lines go through k_rtd_cut / k_rtd_paste (raster_tiles_depth.hip), whose paste is clipped to a window always.
//
// A NODATA raster (useNoData, lerc_amd_nodata.h) says which pixels are invalid with a value, not with a mask.  It is one band staged as
// nMasks 1: k_rtn_cut (raster_nodata.hip) stores the staged mask beside the staged tiles in the one launch that cuts them, the chunk
// goes to encodeTilesDeviceMasked / decodeTilesDeviceMasked untouched, and k_rtn_paste writes noData wherever the decoded valid byte is
// 0 (a failed tile: everywhere) and the window's valid bytes where the caller wants them.  It is never coded where it lies, and the
// way back is a window always (the whole raster: the window that covers it).
#include "codec.h"
#include "raster_tiles.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

namespace lerc {

// the staging buffer's cap (like kTbWorkspace of the tile batches): a class larger than that goes in several chunks
static const size_t kRtStageBytes = (size_t)256 << 20;

namespace {

struct RtClass { u32 ty0, tx0, nTY, nTX, r, c; u64 tiles() const { return (u64)nTY * nTX; } };

struct RtGrid
{
  u32 nTY = 0, nTX = 0;            // the whole grid
  std::vector<RtClass> classes;    // of the request's tile range: every shape class cut down to it
  u64 nRange = 0;                  // tiles in the range (0: the range is empty or not inside the grid)
  bool inPlace = false;
  u64 nTiles() const { return (u64)nTY * nTX; }
};

// The layouts taken.  pixelPitch 1: band-sequential (rows inside a band), and for the _strided calls line-interleaved as well (bands
// inside a row) -- rtRasterAt is linear in its pitches, so k_rt_cut / k_rt_paste serve both.  pixelPitch >= 2 (the _strided calls
// only): pixel-interleaved, one band or bands one element apart that fit into a pixel; a row holds its last pixel's last band.
bool rtLayoutOk(const RasterTilesRequest& rq, u64 nCols, u64 nRows)
{
  const u64 nBands = (u64)rq.nBands;
  if (rq.pixelPitch == 1)
  {
    if (rq.rowPitch >= nCols && (nBands == 1 || rq.bandPitch >= (nRows - 1) * rq.rowPitch + nCols)) return true;
    // (line-interleaved: rowPitch >= (nBands - 1) * bandPitch + nCols, without the product)
    return rq.anyLayout && nBands > 1 && rq.bandPitch >= nCols && rq.rowPitch >= nCols && (rq.rowPitch - nCols) / (nBands - 1) >= rq.bandPitch;
  }
  if (!rq.anyLayout || rq.pixelPitch == 0) return false;
  if (nBands > 1 && (rq.bandPitch != 1 || nBands > rq.pixelPitch)) return false;
  // (rowPitch >= (nCols - 1) * pixelPitch + nBands, without the product)
  return rq.rowPitch >= nBands && (nCols == 1 || (rq.rowPitch - nBands) / (nCols - 1) >= rq.pixelPitch);
}

// The layouts of a depth raster (nDepth > 1; lerc_amd_depth.h): element (row, col, d) at row * rowPitch + col * pixelPitch + d * depthPitch.
// Packed pixels are runs of elements and go through the band kernels with the column counts scaled by nDepth; the others through
// k_rtd_cut / k_rtd_paste (raster_tiles_depth.hip).  Rows, lines or planes that overlap are no layout.  (The products of the header's
// table are never taken: the pitches are any 64-bit numbers.)
enum RtDepthLayout { kRtdNone, kRtdPacked, kRtdGapped, kRtdPlanes, kRtdLines };

RtDepthLayout rtDepthLayout(const RasterTilesRequest& rq, u64 nCols, u64 nRows)
{
  const u64 D = (u64)rq.nDepth, pp = rq.pixelPitch, rp = rq.rowPitch, dp = rq.depthPitch;
  if (dp == 1 && pp >= D)
  {
    // (rowPitch >= (nCols - 1) * pixelPitch + nDepth)
    if (rp >= D && (nCols == 1 || (rp - D) / (nCols - 1) >= pp)) return pp == D ? kRtdPacked : kRtdGapped;
    return kRtdNone;
  }
  if (pp != 1 || rp < nCols || dp < nCols) return kRtdNone;
  if (nRows == 1 || (dp - nCols) / (nRows - 1) >= rp) return kRtdPlanes;    // (depthPitch >= (nRows - 1) * rowPitch + nCols)
  if ((rp - nCols) / (D - 1) >= dp) return kRtdLines;                       // (rowPitch >= (nDepth - 1) * depthPitch + nCols)
  return kRtdNone;
}

// noData as an element of type dt: its raw bits, a quiet NaN where it is NaN
u64 rtNoDataBits(int dt, double noData)
{
  if (dt == DT_Float) { const float f = noData != noData ? std::numeric_limits<float>::quiet_NaN() : (float)noData; u32 b; memcpy(&b, &f, 4); return b; }
  if (dt == DT_Double) { const double d = noData != noData ? std::numeric_limits<double>::quiet_NaN() : noData; u64 b; memcpy(&b, &d, 8); return b; }
  const long long v = (long long)noData;    // (an integer within the type's range: rtNoDataOk)
  return (u64)v & (dtSize(dt) == 1 ? 0xFFull : dtSize(dt) == 2 ? 0xFFFFull : 0xFFFFFFFFull);
}

// (double)(T)noData == noData, or NaN for the two float types (capi.cpp asks the same before the size checks)
bool rtNoDataOk(int dt, double noData)
{
  if (noData != noData) return dt == DT_Float || dt == DT_Double;
  if (dt == DT_Double) return true;
  if (dt == DT_Float) return std::isinf(noData) || (std::fabs(noData) <= (double)std::numeric_limits<float>::max() && (double)(float)noData == noData);
  static const double lo[6] = { -128.0, 0.0, -32768.0, 0.0, -2147483648.0, 0.0 }, hi[6] = { 127.0, 255.0, 32767.0, 65535.0, 2147483647.0, 4294967295.0 };
  return dt >= DT_Char && dt <= DT_UInt && noData >= lo[dt] && noData <= hi[dt] && std::trunc(noData) == noData;
}

// (win: the buffer at dRaster and the mask hold that window of the raster, and the layout's rules apply to its size)
bool rtArgsOk(const RasterTilesRequest& rq, bool encode, const RasterWindow* win = nullptr)
{
  if (win && (win->cols <= 0 || win->rows <= 0 || win->col0 < 0 || win->row0 < 0 || win->cols > rq.nCols - win->col0 || win->rows > rq.nRows - win->row0))
    return false;
  const u64 bufCols = (u64)(win ? win->cols : rq.nCols), bufRows = (u64)(win ? win->rows : rq.nRows);
  if (!rq.dRaster || !rq.dArena || !rq.hOffsets || !rq.hSizes || rq.dt < 0 || rq.dt > DT_Double || rq.nCols <= 0 || rq.nRows <= 0 || rq.nBands <= 0
    || rq.tileCols <= 0 || rq.tileRows <= 0 || (rq.nMasks != 0 && rq.nMasks != 1))
    return false;
  if (rq.useNoData)
  {
    // (validity by value: one band staged with a mask of the cut's making; the caller has none on the way in and may want one back)
    if (rq.nMasks != 1 || rq.nBands != 1 || rq.nDepth != 1 || !rq.anyLayout || (encode && rq.dValidBytes) || !rtNoDataOk(rq.dt, rq.noData)) return false;
    if (rq.dValidBytes && rq.maskRowPitch < bufCols) return false;
  }
  else if ((rq.nMasks == 0) != (rq.dValidBytes == nullptr) || (rq.nMasks && rq.maskRowPitch < bufCols)) return false;
  // (depth tiles: one band in a layout of its own; a tile's row of elements is counted in 32 bits)
  if (rq.nDepth < 1 || (rq.nDepth > 1 && (rq.nBands != 1 || (u64)std::min(rq.tileCols, rq.nCols) * (u64)rq.nDepth > 0x7FFFFFFFull)))
    return false;
  if (rq.nDepth > 1 ? rtDepthLayout(rq, bufCols, bufRows) == kRtdNone : !rtLayoutOk(rq, bufCols, bufRows)) return false;
  if (((uintptr_t)rq.dRaster & (uintptr_t)(dtSize(rq.dt) - 1)) != 0) return false;    // (elements lie on their own boundaries)
  if (encode && (rq.maxZErr < 0 || (rq.slotBytes & 15u) != 0)) return false;
  return true;
}

RtGrid rtGrid(const RasterTilesRequest& rq)
{
  RtGrid g;
  const u32 tr = (u32)rq.tileRows, tc = (u32)rq.tileCols, nR = (u32)rq.nRows, nC = (u32)rq.nCols;
  const u32 fullY = nR / tr, fullX = nC / tc, remR = nR % tr, remC = nC % tc;
  g.nTY = fullY + (remR ? 1 : 0); g.nTX = fullX + (remC ? 1 : 0);
  // the request's tile range [y0, y1) x [x0, x1): the whole grid unless it says otherwise
  if (rq.tileRow0 < 0 || rq.tileCol0 < 0 || rq.nTileRows == 0 || rq.nTileCols == 0 || (u32)rq.tileRow0 >= g.nTY || (u32)rq.tileCol0 >= g.nTX) return g;
  const u32 y0 = (u32)rq.tileRow0, x0 = (u32)rq.tileCol0;
  if ((rq.nTileRows > 0 && (u32)rq.nTileRows > g.nTY - y0) || (rq.nTileCols > 0 && (u32)rq.nTileCols > g.nTX - x0)) return g;
  const u32 y1 = rq.nTileRows < 0 ? g.nTY : y0 + (u32)rq.nTileRows, x1 = rq.nTileCols < 0 ? g.nTX : x0 + (u32)rq.nTileCols;
  g.nRange = (u64)(y1 - y0) * (x1 - x0);
  auto add = [&](u32 ty0, u32 tx0, u32 nTY, u32 nTX, u32 r, u32 c)
  {
    const u32 a0 = std::max(ty0, y0), a1 = std::min(ty0 + nTY, y1), b0 = std::max(tx0, x0), b1 = std::min(tx0 + nTX, x1);
    if (a0 < a1 && b0 < b1) g.classes.push_back({ a0, b0, a1 - a0, b1 - b0, r, c });
  };
  if (fullY && fullX) add(0, 0, fullY, fullX, tr, tc);
  if (fullY && remC) add(0, fullX, fullY, 1, tr, remC);
  if (remR && fullX) add(fullY, 0, 1, fullX, remR, tc);
  if (remR && remC) add(fullY, fullX, 1, 1, remR, remC);
  g.inPlace = !rq.useNoData && rq.pixelPitch == 1 && rq.nBands == 1 && rq.nDepth == 1 && tc >= nC && rq.rowPitch == (u64)nC && (!rq.nMasks || rq.maskRowPitch == (u64)nC);
  return g;
}

struct RtStagePlan { size_t dataPerTile, maskPerTile; u32 maxChunk; };

// tiles a chunk: what fits the cap (one at least); LERC_AMD_TEST_RASTER_CHUNK=n (tests only, read per call) makes it n
RtStagePlan rtPlan(const RasterTilesRequest& rq, const RtClass& k)
{
  RtStagePlan p;
  const size_t pix = (size_t)k.r * k.c;
  p.dataPerTile = pix * (size_t)rq.nBands * (size_t)rq.nDepth * (size_t)dtSize(rq.dt);
  p.maskPerTile = rq.nMasks ? pix : 0;
  size_t most = std::max<size_t>(1, kRtStageBytes / (p.dataPerTile + p.maskPerTile));
  const char* e = getenv("LERC_AMD_TEST_RASTER_CHUNK");
  const long knob = e ? strtol(e, nullptr, 0) : 0;
  if (knob >= 1) most = std::min<size_t>(most, (size_t)knob);
  p.maxChunk = (u32)std::min<u64>(std::min<u64>(k.tiles(), most), 0x7FFFFFFFu);
  return p;
}

size_t rtMaskAt(const RtStagePlan& p, u32 n) { return ((size_t)n * p.dataPerTile + 255) & ~(size_t)255; }

// the staging buffer for the largest chunk of the call, allocated once (growing it later would wait for the stream)
u8* rtStageFor(Context& ctx, const RasterTilesRequest& rq, const RtGrid& g)
{
  size_t need = 0;
  for (const RtClass& k : g.classes)
  {
    const RtStagePlan p = rtPlan(rq, k);
    need = std::max(need, rtMaskAt(p, p.maxChunk) + (size_t)p.maxChunk * p.maskPerTile);
  }
  return ctx.rasterStage(need);
}

RtChunk rtChunk(const RasterTilesRequest& rq, const RtClass& k, u32 k0, u32 n, bool mask)
{
  RtChunk ch;
  ch.rowPitch = mask ? rq.maskRowPitch : rq.rowPitch; ch.bandPitch = mask ? 0 : rq.bandPitch;
  ch.tileRows = (u32)rq.tileRows; ch.tileCols = (u32)rq.tileCols; ch.r = k.r; ch.c = k.c;
  ch.ty0 = k.ty0; ch.tx0 = k.tx0; ch.classW = k.nTX; ch.k0 = k0; ch.n = n; ch.nBands = mask ? 1u : (u32)rq.nBands;
  return ch;
}

// the whole raster as a window of itself
RasterWindow rtWholeRaster(const RasterTilesRequest& rq) { RasterWindow w; w.cols = rq.nCols; w.rows = rq.nRows; return w; }

// Packed depth pixels seen as a run of elements, one band: a tile's rows are runs of c * nDepth elements, a tile column is tileCols *
// nDepth elements wide, and so is a window's rectangle; the mask stays at pixel width.  (A tile wider than the raster is clipped to it
// first -- its column index is 0 then, so nothing changes --: rtArgsOk has bounded min(tileCols, nCols) * nDepth, and that is the
// product taken here.)
RwChunk rtPackedChunk(const RasterTilesRequest& rq, const RtClass& k, u32 k0, u32 n, const RasterWindow& win)
{
  const u32 D = (u32)rq.nDepth;
  RwChunk cw{ rtChunk(rq, k, k0, n, false), 1, (u32)win.row0, (u32)win.col0 * D, (u32)win.rows, (u32)win.cols * D };
  cw.ch.tileCols = (u32)std::min(rq.tileCols, rq.nCols) * D; cw.ch.c *= D;
  return cw;
}
// (a raster whose rows of elements leave 32 bits: the window's columns cannot be scaled, and the depth kernels take the pixels as they are)
bool rtPackedAsRuns(const RasterTilesRequest& rq, const RasterWindow* win)
{
  return rtDepthLayout(rq, (u64)(win ? win->cols : rq.nCols), (u64)(win ? win->rows : rq.nRows)) == kRtdPacked && (!win || (u64)rq.nCols * (u64)rq.nDepth <= 0x7FFFFFFFull);
}

RtdChunk rtDepthChunk(const RasterTilesRequest& rq, const RtClass& k, u32 k0, u32 n, const RasterWindow& win)
{
  RtdChunk cd{ rtChunk(rq, k, k0, n, false), rq.pixelPitch, rq.depthPitch, (u32)win.row0, (u32)win.col0, (u32)win.rows, (u32)win.cols };
  cd.ch.nBands = (u32)rq.nDepth;
  return cd;
}

// the data of a chunk: planes through k_rt_cut / k_rt_paste, an interleaved raster through k_rt_cut_px / k_rt_paste_px, a depth raster
// as runs of elements through the former or through k_rtd_cut / k_rtd_paste; win: the clipped paste of each
void rtCutData(const RasterTilesRequest& rq, const RtClass& k, u32 k0, u32 n, u8* stage, u32 eb, hipStream_t st)
{
  if (rq.nDepth > 1)
  {
    if (rtPackedAsRuns(rq, nullptr)) launchRasterCut(rq.dRaster, stage, rtPackedChunk(rq, k, k0, n, rtWholeRaster(rq)).ch, eb, st);
    else launchRasterCutDepth(rq.dRaster, stage, rtDepthChunk(rq, k, k0, n, rtWholeRaster(rq)), eb, st);
    return;
  }
  const RtChunk ch = rtChunk(rq, k, k0, n, false);
  if (rq.pixelPitch == 1) launchRasterCut(rq.dRaster, stage, ch, eb, st);
  else launchRasterCutPx(rq.dRaster, stage, RtChunkPx{ ch, rq.pixelPitch }, eb, st);
}
void rtPasteData(const RasterTilesRequest& rq, const RtClass& k, u32 k0, u32 n, const u8* stage, u32 eb, hipStream_t st, const RasterWindow* win)
{
  if (rq.nDepth > 1)
  {
    if (!rtPackedAsRuns(rq, win)) launchRasterPasteDepth(stage, rq.dRaster, rtDepthChunk(rq, k, k0, n, win ? *win : rtWholeRaster(rq)), eb, st);
    else if (win) launchWindowPaste(stage, rq.dRaster, rtPackedChunk(rq, k, k0, n, *win), eb, st);
    else launchRasterPaste(stage, rq.dRaster, rtPackedChunk(rq, k, k0, n, rtWholeRaster(rq)).ch, eb, st);
    return;
  }
  const RtChunk ch = rtChunk(rq, k, k0, n, false);
  if (win)
  {
    const RwChunk cw{ ch, rq.pixelPitch, (u32)win->row0, (u32)win->col0, (u32)win->rows, (u32)win->cols };
    if (rq.pixelPitch == 1) launchWindowPaste(stage, rq.dRaster, cw, eb, st);
    else launchWindowPastePx(stage, rq.dRaster, cw, eb, st);
  }
  else if (rq.pixelPitch == 1) launchRasterPaste(stage, rq.dRaster, ch, eb, st);
  else launchRasterPastePx(stage, rq.dRaster, RtChunkPx{ ch, rq.pixelPitch }, eb, st);
}

size_t rtTileIndex(const RtGrid& g, const RtClass& k, u32 i) { return (size_t)(k.ty0 + i / k.nTX) * g.nTX + (k.tx0 + i % k.nTX); }

}    // namespace

u32 encodeRasterTilesDevice(Context& ctx, const RasterTilesRequest& rq, u64& arenaUsed)
{
  arenaUsed = 0;
  if (!rtArgsOk(rq, true)) return kWrongParam;
  const RtGrid g = rtGrid(rq);
  if (g.nTiles() > 0x7FFFFFFFull) return kDimsTooLarge;
  if (g.nRange == 0) return kWrongParam;
  const bool slotted = rq.slotBytes != 0;
  if (slotted && rq.arenaCapacity < g.nRange * rq.slotBytes) return kBufferTooSmall;
  const u32 eb = (u32)dtSize(rq.dt);
  hipStream_t st = ctx.activeStream();
  u8* stage = g.inPlace ? nullptr : rtStageFor(ctx, rq, g);
  if (!g.inPlace && !stage) return kFailed;

  u64 base = 0, room = 0;    // packed: arena bytes in use; slotted: rooms handed out
  std::vector<u64> offs;
  std::vector<u32> sizes;
  for (const RtClass& k : g.classes)
  {
    const RtStagePlan p = rtPlan(rq, k);
    const u32 nClass = (u32)k.tiles(), step = g.inPlace ? nClass : p.maxChunk;
    for (u32 k0 = 0; k0 < nClass; k0 += step)
    {
      const u32 n = std::min(step, nClass - k0);
      TilesEncodeRequest sub;
      if (g.inPlace)
      {
        // (tiles as wide as the raster: the class is a run of rows, [n][r][c] as it lies)
        const u64 first = (u64)k.ty0 * (u64)rq.tileRows * (u64)rq.nCols;
        sub.dData = (const u8*)rq.dRaster + first * eb;
        sub.dValidBytes = rq.nMasks ? rq.dValidBytes + first : nullptr;
        ctx.rasterTilesCount[1] += n;
      }
      else
      {
        (void)hipGetLastError();
        if (rq.useNoData)
          launchRasterCutNoData(rq.dRaster, stage, stage + rtMaskAt(p, n), RtnCut{ rtChunk(rq, k, k0, n, false), rq.pixelPitch, rtNoDataBits(rq.dt, rq.noData), rq.noData != rq.noData ? 1u : 0u }, rq.dt, st);
        else rtCutData(rq, k, k0, n, stage, eb, st);
        if (rq.nMasks && !rq.useNoData) launchRasterCut(rq.dValidBytes, stage + rtMaskAt(p, n), rtChunk(rq, k, k0, n, true), 1, st);
        if (hipGetLastError() != hipSuccess) { ctx.lastError = "lerc_amd: the raster cut kernel could not be launched"; return kFailed; }
        sub.dData = stage;
        sub.dValidBytes = rq.nMasks ? stage + rtMaskAt(p, n) : nullptr;
        ctx.rasterTilesCount[0] += n;
      }
      offs.assign(n, 0); sizes.assign(n, 0);
      sub.dt = rq.dt; sub.nCols = (int)k.c; sub.nRows = (int)k.r; sub.nTiles = (int)n; sub.maxZErr = rq.maxZErr;
      sub.hOffsets = offs.data(); sub.hSizes = sizes.data(); sub.slotBytes = rq.slotBytes;
      if (slotted) { base = room * rq.slotBytes; sub.arenaCapacity = (u64)n * rq.slotBytes; }
      else
      {
        base = (base + 15) & ~15ull;
        if (base >= rq.arenaCapacity) return kBufferTooSmall;
        sub.arenaCapacity = rq.arenaCapacity - base;
      }
      sub.dArena = rq.dArena + base;
      u64 used = 0;
      u32 rc;
      if (rq.nDepth > 1) { sub.nDepth = rq.nDepth; rc = encodeTilesDeviceDepth(ctx, sub, used); }
      else if (rq.nBands == 1) rc = rq.nMasks ? encodeTilesDeviceMasked(ctx, sub, used) : encodeTilesDevice(ctx, sub, used);
      else { sub.nBands = rq.nBands; sub.nMasks = rq.nMasks; rc = encodeTilesDeviceBands(ctx, sub, used); }
      if (rc != kOk) return rc;
      for (u32 i = 0; i < n; i++)
      {
        const size_t t = rtTileIndex(g, k, k0 + i);
        rq.hOffsets[t] = base + (slotted ? (u64)i * rq.slotBytes : offs[i]);
        rq.hSizes[t] = sizes[i];
      }
      if (slotted) room += n; else base += used;
    }
  }
  arenaUsed = slotted ? g.nRange * rq.slotBytes : base;
  return kOk;
}

// The way back.  win == nullptr: the request's tiles into the raster at rq.dRaster.  win: into a buffer that holds that window of the
// raster -- the request's tile range is the tiles the window touches, they are never decoded where they lie, and the paste is the
// clipped one.
static u32 rtDecode(Context& ctx, const RasterTilesRequest& rq, const RasterWindow* win)
{
  if (!rtArgsOk(rq, false, win)) return kWrongParam;
  RtGrid g = rtGrid(rq);
  if (g.nTiles() > 0x7FFFFFFFull) return kDimsTooLarge;
  if (g.nRange == 0) return kWrongParam;
  if (win) g.inPlace = false;
  const u32 eb = (u32)dtSize(rq.dt);
  u8* stage = g.inPlace ? nullptr : rtStageFor(ctx, rq, g);
  if (!g.inPlace && !stage) return kFailed;

  u32 firstError = kOk;
  std::vector<u64> offs;
  std::vector<u32> sizes;
  for (const RtClass& k : g.classes)
  {
    const RtStagePlan p = rtPlan(rq, k);
    const u32 nClass = (u32)k.tiles(), step = g.inPlace ? nClass : p.maxChunk;
    for (u32 k0 = 0; k0 < nClass; k0 += step)
    {
      const u32 n = std::min(step, nClass - k0);
      offs.resize(n); sizes.resize(n);
      for (u32 i = 0; i < n; i++) { const size_t t = rtTileIndex(g, k, k0 + i); offs[i] = rq.hOffsets[t]; sizes[i] = rq.hSizes[t]; }
      TilesDecodeRequest sub;
      sub.dArena = rq.dArena; sub.hOffsets = offs.data(); sub.hSizes = sizes.data();
      sub.dt = rq.dt; sub.nCols = (int)k.c; sub.nRows = (int)k.r; sub.nTiles = (int)n;
      if (g.inPlace)
      {
        const u64 first = (u64)k.ty0 * (u64)rq.tileRows * (u64)rq.nCols;
        sub.dOut = (u8*)rq.dRaster + first * eb;
        sub.dValidBytes = rq.nMasks ? rq.dValidBytes + first : nullptr;
        ctx.rasterTilesCount[3] += n;
      }
      else
      {
        sub.dOut = stage;
        sub.dValidBytes = rq.nMasks ? stage + rtMaskAt(p, n) : nullptr;
        ctx.rasterTilesCount[2] += n;
      }
      u32 rc;
      if (rq.nDepth > 1) { sub.nDepth = rq.nDepth; rc = decodeTilesDeviceDepth(ctx, sub); }
      else if (rq.nBands > 1) { sub.nBands = rq.nBands; sub.nMasks = rq.nMasks; rc = decodeTilesDeviceBands(ctx, sub); }
      else if (rq.nMasks) rc = decodeTilesDeviceMasked(ctx, sub);
      else
      {
        rc = decodeTilesDevice(ctx, sub);
        if (rc != kOk)
        {
          // (the plain call stops at the tile that fails: here every tile is decoded all the same, so the chunk goes once more, tile
          // by tile, and a tile that fails is left zeroed)
          rc = kOk;
          const size_t tileBytes = (size_t)k.r * k.c * eb;
          for (u32 i = 0; i < n; i++)
          {
            TilesDecodeRequest one = sub;
            one.hOffsets = offs.data() + i; one.hSizes = sizes.data() + i; one.nTiles = 1;
            one.dOut = (u8*)sub.dOut + (size_t)i * tileBytes;
            const u32 rc1 = decodeTilesDevice(ctx, one);
            if (rc1 == kOk) continue;
            hipMemsetAsync(one.dOut, 0, tileBytes, ctx.activeStream());
            if (rc == kOk) rc = rc1;
          }
        }
      }
      if (rc != kOk && firstError == kOk) firstError = rc;
      if (!g.inPlace)
      {
        hipStream_t st = ctx.activeStream();
        (void)hipGetLastError();
        if (rq.useNoData)    // (a window always: decodeRasterWindowDevice)
          launchWindowPasteNoData(stage, stage + rtMaskAt(p, n), rq.dRaster, rq.dValidBytes,
                                  RtnPaste{ RwChunk{ rtChunk(rq, k, k0, n, false), rq.pixelPitch, (u32)win->row0, (u32)win->col0, (u32)win->rows, (u32)win->cols },
                                            rtNoDataBits(rq.dt, rq.noData), rq.maskRowPitch }, eb, st);
        else rtPasteData(rq, k, k0, n, stage, eb, st, win);
        const bool pasteMask = rq.nMasks && !rq.useNoData;    // (noData: the valid bytes went with the pixels)
        if (pasteMask && win) launchWindowPaste(stage + rtMaskAt(p, n), rq.dValidBytes, RwChunk{ rtChunk(rq, k, k0, n, true), 1, (u32)win->row0, (u32)win->col0, (u32)win->rows, (u32)win->cols }, 1, st);
        else if (pasteMask) launchRasterPaste(stage + rtMaskAt(p, n), rq.dValidBytes, rtChunk(rq, k, k0, n, true), 1, st);
        if (hipGetLastError() != hipSuccess) { ctx.lastError = "lerc_amd: the raster paste kernel could not be launched"; return kFailed; }
      }
    }
  }
  if (!ctx.sync()) return kFailed;    // (the pastes: the raster is the caller's when the call returns)
  return firstError;
}

u32 decodeRasterTilesDevice(Context& ctx, const RasterTilesRequest& rq) { return rq.useNoData ? (u32)kWrongParam : rtDecode(ctx, rq, nullptr); }

bool rasterNoDataOk(int dt, double noData) { return rtNoDataOk(dt, noData); }

u32 decodeRasterWindowDevice(Context& ctx, const RasterTilesRequest& rq, const RasterWindow& win)
{
  if (rq.tileCols <= 0 || rq.tileRows <= 0 || !rtArgsOk(rq, false, &win)) return kWrongParam;
  // the tiles the window touches are a rectangle of the grid
  RasterTilesRequest sub = rq;
  sub.tileRow0 = win.row0 / rq.tileRows; sub.nTileRows = (win.row0 + win.rows - 1) / rq.tileRows - sub.tileRow0 + 1;
  sub.tileCol0 = win.col0 / rq.tileCols; sub.nTileCols = (win.col0 + win.cols - 1) / rq.tileCols - sub.tileCol0 + 1;
  return rtDecode(ctx, sub, &win);
}

}    // namespace lerc
