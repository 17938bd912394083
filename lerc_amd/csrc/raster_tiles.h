// raster_tiles.h -- a pitched device raster cut into tiles and pasted back (raster_tiles.hip, codec_raster_tiles.cpp): the staging
// pass in front of / behind the tile batch calls, which take tiles of one shape laid out as [n][nBands][r][c].
#pragma once
#include "lerc_common.h"

namespace lerc {

// One shape class of a tile grid (interior, right column, bottom row, corner): a rectangle of the grid whose tiles all are r x c.
// Its tiles are numbered row by row inside the class; a launch moves tiles [k0, k0 + n) of it.
struct RtChunk
{
  u64 rowPitch, bandPitch;    // of the raster, in elements (the mask: its own row pitch, nBands 1)
  u32 tileRows, tileCols;     // the grid's steps
  u32 r, c;                   // the class's tile shape (r <= tileRows, c <= tileCols)
  u32 ty0, tx0, classW;       // the class's first tile row / column in the grid, and how many tiles wide it is
  u32 k0, n;                  // the chunk: tiles of the class
  u32 nBands;
};

// the rows of a plane a workgroup takes (at least: a workgroup of short rows takes as many as it has lanes for), and how many lanes run along one row (a power of two, 8 .. 64: a lane moves 16 bytes a step)
static const u32 kRtStripRows = 16;
inline u32 rtLanesPerRowLog2(u32 c, u32 elemBytes)
{
  const u64 vecs = ((u64)c * elemBytes + 15) / 16 + 1;    // (+ 1: a row that begins inside a vector)
  u32 lg = 3;
  while (lg < 6 && (1ull << lg) < vecs) lg++;
  return lg;
}

// staging <- raster (cut) and raster <- staging (paste); elemBytes 1, 2, 4 or 8; both pointers aligned to the element.  One launch.
void launchRasterCut(const void* dRaster, void* dStage, const RtChunk& ch, u32 elemBytes, hipStream_t st);
void launchRasterPaste(const void* dStage, void* dRaster, const RtChunk& ch, u32 elemBytes, hipStream_t st);

// ---- pixel-interleaved rasters (raster_tiles_px.hip): element (b, i, j) lies at b + i * rowPitch + j * pixelPitch, pixelPitch >= 2
// and nBands <= pixelPitch (one band: channel 0 of the pointer handed over).  ch.bandPitch is not used.
struct RtChunkPx
{
  RtChunk ch;
  u64 pixelPitch;
};

// The staged form takes a row in segments of kRtPxSegBytes / elemBytes pixels (512, 256, 128, 64 for 1, 2, 4, 8 bytes), kRtPxRows rows
// of a tile at a time, through an LDS buffer of kRtPxSlotDwords a row: room for a segment at kRtPxMaxPitch elements a pixel, the up to
// 15 bytes the run begins behind a 16-byte boundary, and the padding dword after every 16 * pixelPitch bytes.  A pixelPitch above
// kRtPxMaxPitch goes the plain way, a lane an element; the results are the same.
static const u32 kRtPxMaxPitch = 8;
static const u32 kRtPxSegBytes = 512;
static const u32 kRtPxRows = 8;
static const u32 kRtPxSlotDwords = 1168;    // >= (15 + kRtPxSegBytes * kRtPxMaxPitch) * (1 + 1 / 8) / 4: pixelPitch 2 pads most, 4 bytes in 32

// staging <- interleaved raster and back, data only (the mask is a plane: launchRasterCut / launchRasterPaste).  One launch.
void launchRasterCutPx(const void* dRaster, void* dStage, const RtChunkPx& cx, u32 elemBytes, hipStream_t st);
void launchRasterPastePx(const void* dStage, void* dRaster, const RtChunkPx& cx, u32 elemBytes, hipStream_t st);

// ---- the clipped paste of the window decode (raster_window.hip): the staged tiles of a chunk go into a buffer that holds a WINDOW of
// the raster, rows [winRow0, winRow0 + winRows) by columns [winCol0, winCol0 + winCols) in raster coordinates, and nothing else.  ch's
// pitches (and pixelPitch) are the window buffer's; ch's grid and class are the raster's.  Of every staged tile the rows and columns
// inside the window are written, at (row - winRow0, col - winCol0); a tile that misses the window writes nothing.
struct RwChunk
{
  RtChunk ch;
  u64 pixelPitch;    // of the window buffer: 1 planes or line-interleaved (k_rw_paste), >= 2 pixel-interleaved (k_rw_paste_px)
  u32 winRow0, winCol0, winRows, winCols;
};

// window <- staging.  pixelPitch 1 only (the mask plane: its own row pitch, nBands 1) / pixelPitch >= 2 only.  One launch.
void launchWindowPaste(const void* dStage, void* dWindow, const RwChunk& cw, u32 elemBytes, hipStream_t st);
void launchWindowPastePx(const void* dStage, void* dWindow, const RwChunk& cw, u32 elemBytes, hipStream_t st);

// ---- depth rasters (raster_tiles_depth.hip): element (i, j, d) lies at i * rowPitch + j * pixelPitch + d * depthPitch, the staged form
// is [n][r][c][nDepth].  ch: the grid and the class in PIXELS, nBands = nDepth, rowPitch the raster's; ch.bandPitch is not used.  One of
// pixelPitch (planes, lines) and depthPitch (gapped pixels; packed ones, pixelPitch == nDepth, are taken too) is 1.  The window is
// RwChunk's: the buffer at dRaster holds rows [winRow0, winRow0 + winRows) by columns [winCol0, winCol0 + winCols) of the raster and
// the pitches are its own; the whole raster: 0, 0, nRows, nCols.  The segment buffer of the pixel-interleaved kernels serves a pixel
// of up to kRtPxMaxPitch elements (nDepth; pixelPitch where it has gaps); beyond that a lane moves an element, with the same results.
struct RtdChunk
{
  RtChunk ch;
  u64 pixelPitch, depthPitch;
  u32 winRow0, winCol0, winRows, winCols;
};

// staging <- raster (of the tiles' parts inside the window; the encode's: everything) and raster <- staging, data only.  One launch.
void launchRasterCutDepth(const void* dRaster, void* dStage, const RtdChunk& cd, u32 elemBytes, hipStream_t st);
void launchRasterPasteDepth(const void* dStage, void* dRaster, const RtdChunk& cd, u32 elemBytes, hipStream_t st);

// ---- noData rasters (raster_nodata.hip; include/lerc_amd_nodata.h): one band, element (i, j) at i * rowPitch + j * pixelPitch, whose
// validity is a VALUE.  The cut stores the staged tiles [n][r][c] and, beside them, the staged mask [n][r][c] (1: the element is not
// the noData value) in one launch; the paste is the window's clipped one with select(staged valid byte, staged element, fill) on the
// way, and writes the window's valid bytes [winRows][maskRowPitch] too where dWindowMask is not NULL.  ch.nBands is 1, ch.bandPitch is
// not used; pixelPitch 1 moves 16-byte vectors, pixelPitch >= 2 (one channel of an interleaved image) a lane an element.
struct RtnCut
{
  RtChunk ch;
  u64 pixelPitch;
  u64 ndBits;       // (T)noData as raw bits of the element's type
  u32 ndIsNaN;      // float / double only: an element is invalid when it is a NaN (ndBits is not looked at)
};
struct RtnPaste
{
  RwChunk cw;
  u64 fillBits;     // what an invalid pixel gets, raw bits of the element's type
  u64 maskRowPitch;
};

// dt: the raster's data type (the compare is by `==` / `v != v` for the float types, on the raw pattern for integers).  One launch.
void launchRasterCutNoData(const void* dRaster, void* dStage, u8* dStageMask, const RtnCut& cn, int dt, hipStream_t st);
void launchWindowPasteNoData(const void* dStage, const u8* dStageMask, void* dWindow, u8* dWindowMask, const RtnPaste& pn, u32 elemBytes, hipStream_t st);

}    // namespace lerc
