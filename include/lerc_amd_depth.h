/* lerc_amd_depth.h -- tile batches and raster mosaics of DEPTH tiles: Lerc's own pixel-interleaved form, one Lerc2 blob with the
 * header's nDepth a tile.  That is what a tiled-LERC writer (a GeoTIFF, an MRF) makes of an [H, W, C] raster: lerc_encode(tile,
 * nDepth = C, nBands = 1).  (The band stack calls of lerc_amd_device.h code such a tile as C blobs back to back: another blob.)
 *
 * Contexts, statuses, notes and counters are those of lerc_amd_device.h. */
#ifndef LERC_AMD_DEPTH_H
#define LERC_AMD_DEPTH_H

#include "lerc_amd_device.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A mosaic of depth tiles in ONE set of launches and one host wait per sub-batch.
 *   dTiles       device, [nTiles][nRows][nCols][nDepth]
 *   dValidBytes  device, [nTiles][nRows][nCols], 0 = invalid: one mask a tile; NULL: every pixel valid
 *   slotBytes    0: the blobs lie packed in the arena at 16-byte aligned offsets; else a multiple of 16: tile t's blob lies at
 *                dArena + t * slotBytes
 * Tile t's blob is byte for byte what lerc_encode(tile t, nDepth, nBands 1, nMasks 0 | 1, mask t, maxZErr) writes.  offsets, sizes:
 * host, [nTiles]; arenaUsed: host, may be NULL.  nDepth == 1 is lerc_amd_encode_tiles_device_masked.
 * The batch's own launches take int16 / uint16 / int32 / uint32 / float32 / float64 tiles of 2 .. 8 values a pixel and every size the
 * masked batches take.  8-bit tiles, nDepth > 8, a NaN at a valid pixel, maxZErr 777 or 0 on float values, larger tiles and a blob that
 * does not fit its slot are done one by one inside the call, same bytes and status; lerc_amd_last_note names the first such tile and the
 * reason, lerc_amd_tile_batch_counters counts both kinds.
 * WrongParam: a NULL pointer, a count < 1 (nDepth included), maxZErr < 0, a slotBytes that is no multiple of 16. */
LERC_AMD_API lerc_status lerc_amd_encode_tiles_device_depth(lerc_amd_context* ctx, const void* dTiles, unsigned int dataType, int nCols, int nRows,
    int nDepth, int nTiles, const unsigned char* dValidBytes, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity,
    unsigned long long slotBytes, unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed);

/* The way back: pixels and valid bytes are exactly what lerc_amd_decode_device writes for each blob.  dValidBytes: device,
 * [nTiles][nRows][nCols], written 1 / 0 for every tile, or NULL (then a blob with an invalid pixel is the single-blob decoder's to
 * refuse).  A blob of codec < 6, of another nDepth, shape or type, one with noData values or a Huffman mode, and anything damaged is
 * decoded by itself inside the call; a tile that fails is left zeroed, the tiles behind it are decoded, and the first failing tile's
 * status is returned. */
LERC_AMD_API lerc_status lerc_amd_decode_tiles_device_depth(lerc_amd_context* ctx, const unsigned char* dArena, const unsigned long long* offsets,
    const unsigned int* sizes, int nTiles, int nCols, int nRows, int nDepth, unsigned int dataType, void* dTiles, unsigned char* dValidBytes);

/* A pixel-interleaved device raster, pixels packed, cut into the grid of lerc_amd_raster_tile_grid and coded as depth tiles.
 *   dRaster      device: element (row, col, d) at row * rowPitch + col * pixelPitch + d, in elements
 *   pixelPitch   must equal nDepth (packed pixels); rowPitch >= nCols * nDepth, so a view into a wider raster is taken
 *   dValidBytes  device byte mask [nRows][maskRowPitch] (nMasks 1) or NULL (nMasks 0)
 * Offsets, sizes, slots, shape classes, chunks through the staging buffer and lerc_amd_raster_tiles_counters are those of
 * lerc_amd_encode_raster_tiles_device.  Every other pitch description -- pixelPitch > nDepth (RGB out of RGBA) included -- is
 * WrongParam for these two calls; the _strided calls below take them. */
LERC_AMD_API lerc_status lerc_amd_encode_raster_tiles_device_depth(lerc_amd_context* ctx, const void* dRaster, unsigned int dataType, int nCols,
    int nRows, int nDepth, unsigned long long pixelPitch, unsigned long long rowPitch, int tileCols, int tileRows, int nMasks,
    const unsigned char* dValidBytes, unsigned long long maskRowPitch, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity,
    unsigned long long slotBytes, unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed);

LERC_AMD_API lerc_status lerc_amd_decode_raster_tiles_device_depth(lerc_amd_context* ctx, const unsigned char* dArena, const unsigned long long* offsets,
    const unsigned int* sizes, unsigned int dataType, int nCols, int nRows, int nDepth, unsigned long long pixelPitch, unsigned long long rowPitch,
    int tileCols, int tileRows, void* dRaster, int nMasks, unsigned char* dValidBytes, unsigned long long maskRowPitch);

/* The same for a depth raster in ANY of four layouts, described by three pitches in elements: element (row, col, d) lies at
 * row * rowPitch + col * pixelPitch + d * depthPitch.
 *   packed pixels   depthPitch == 1, pixelPitch == nDepth, rowPitch >= nCols * nDepth                  the two calls above
 *   gapped pixels   depthPitch == 1, pixelPitch > nDepth,  rowPitch >= (nCols - 1) * pixelPitch + nDepth
 *                   RGB out of RGBA, two channels of an interleaved frame; a gap's elements are neither read nor written
 *   planes          pixelPitch == 1, rowPitch >= nCols, depthPitch >= (nRows - 1) * rowPitch + nCols
 *                   [C, H, W], also a view chw[:, a:b, c:d]
 *   lines           pixelPitch == 1, depthPitch >= nCols, rowPitch >= (nDepth - 1) * depthPitch + nCols   GDAL's INTERLEAVE=LINE
 * Every other description -- both of pixelPitch and depthPitch above 1, rows, lines or planes that overlap -- is WrongParam.  The
 * blobs are those of the packed call on a packed copy of the raster, byte for byte; nothing is copied to get them: the staging pass
 * reads (writes) the raster where it lies.  nDepth == 1 ignores depthPitch and is lerc_amd_encode_raster_tiles_device_strided /
 * lerc_amd_decode_raster_tiles_device_strided with one band.  Masks, slots, counters, statuses and size limits: the packed calls'. */
LERC_AMD_API lerc_status lerc_amd_encode_raster_tiles_device_depth_strided(lerc_amd_context* ctx, const void* dRaster, unsigned int dataType,
    int nCols, int nRows, int nDepth, unsigned long long pixelPitch, unsigned long long rowPitch, unsigned long long depthPitch, int tileCols,
    int tileRows, int nMasks, const unsigned char* dValidBytes, unsigned long long maskRowPitch, double maxZErr, unsigned char* dArena,
    unsigned long long arenaCapacity, unsigned long long slotBytes, unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed);

LERC_AMD_API lerc_status lerc_amd_decode_raster_tiles_device_depth_strided(lerc_amd_context* ctx, const unsigned char* dArena,
    const unsigned long long* offsets, const unsigned int* sizes, unsigned int dataType, int nCols, int nRows, int nDepth,
    unsigned long long pixelPitch, unsigned long long rowPitch, unsigned long long depthPitch, int tileCols, int tileRows, void* dRaster, int nMasks,
    unsigned char* dValidBytes, unsigned long long maskRowPitch);

/* The strided encode for a rectangle of the grid's tiles, [tileRow0, tileRow0 + nTileRows) x [tileCol0, tileCol0 + nTileCols), as
 * lerc_amd_encode_raster_tiles_device_range: dRaster and the mask are the WHOLE raster, offsets and sizes the full grid's tables of
 * which only the range's entries are written, every blob is what the whole-raster call makes of that tile, and with slotBytes != 0 the
 * range takes the first nTileRows * nTileCols rooms of the arena.  WrongParam: a range that is empty or not inside the grid. */
LERC_AMD_API lerc_status lerc_amd_encode_raster_tiles_device_depth_range(lerc_amd_context* ctx, const void* dRaster, unsigned int dataType,
    int nCols, int nRows, int nDepth, unsigned long long pixelPitch, unsigned long long rowPitch, unsigned long long depthPitch, int tileCols,
    int tileRows, int tileCol0, int tileRow0, int nTileCols, int nTileRows, int nMasks, const unsigned char* dValidBytes,
    unsigned long long maskRowPitch, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity, unsigned long long slotBytes,
    unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed);

/* A window of a depth mosaic, as lerc_amd_decode_raster_window_device: nCols, nRows, nDepth, the tile size and the full-grid tables
 * describe the mosaic; rows [winRow0, winRow0 + winRows) by columns [winCol0, winCol0 + winCols) of it go into the buffer at dWindow,
 * which holds the window ONLY and is described by the three pitches (any of the four layouts, the rules applied to the window's size),
 * with a mask plane [winRows][maskRowPitch] or none.  Only the tiles the window touches are read and decoded; nothing beside the
 * window's elements is written.  A tile whose blob fails leaves its part of the window zeroed, and the first failing tile's status
 * is returned.  WrongParam: a window that is empty or not inside the raster. */
LERC_AMD_API lerc_status lerc_amd_decode_raster_window_device_depth(lerc_amd_context* ctx, const unsigned char* dArena,
    const unsigned long long* offsets, const unsigned int* sizes, unsigned int dataType, int nCols, int nRows, int nDepth, int tileCols,
    int tileRows, int winCol0, int winRow0, int winCols, int winRows, void* dWindow, unsigned long long pixelPitch, unsigned long long rowPitch,
    unsigned long long depthPitch, int nMasks, unsigned char* dValidBytes, unsigned long long maskRowPitch);

#ifdef __cplusplus
}
#endif
#endif
