/* lerc_amd_nodata.h -- raster mosaics whose validity is a noData VALUE, not a byte mask: a DEM with -9999, a scene band with 0 or
 * 65535, a float product with NaN holes.  A tiled-LERC writer (LERC in GeoTIFF, MRF) turns that value into a mask on the host before
 * lerc_encode and writes it back where the mask says 0 after lerc_decode; here the staging pass that cuts the raster into tiles and
 * pastes them back does both on the way, and the mask never exists as a raster-sized buffer.
 *
 * A pixel value v of type T is INVALID under the call's `double noData` when
 *   - noData is NaN, T is float or double, and v != v; or
 *   - noData is not NaN and v == (T)noData by the type's own == (so -0.0f matches 0.0, and +-inf matches itself).
 * noData must be exactly representable in T: (double)(T)noData == noData, or NaN for the two float types.  NaN for an integer type, a
 * fraction for an integer type, a double that float cannot hold: WrongParam(2), decided with the other argument checks and before
 * DimsTooLarge(6).
 *
 * Both calls: ONE band, all eight data types; element (i, j) of the raster (of the window's buffer) lies at i * rowPitch + j * pixelPitch,
 * in elements, 64-bit addresses -- the layouts the _strided calls of lerc_amd_device.h take with nBands == 1: a pitched raster, a view
 * into a larger tensor, one channel of an interleaved image (pixelPitch >= 2).  pixelPitch 1 moves 16-byte vectors; a pixelPitch >= 2
 * goes the plain way, a lane an element, with the same results (as the existing calls do for pitches above 8).
 * There is no nBands argument (bands disagree about validity: that needs a mask a band) and no nDepth (mixed validity inside a pixel is
 * the reference's noData-in-header form, which the depth batches hand back).
 *
 * Contexts, statuses, notes and counters are those of lerc_amd_device.h. */
#ifndef LERC_AMD_NODATA_H
#define LERC_AMD_NODATA_H

#include "lerc_amd_device.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The raster cut into the grid of lerc_amd_raster_tile_grid, every tile a blob.  Tile t's blob is byte for byte what lerc_encode makes
 * of that rectangle with nDepth 1, nBands 1, nMasks 1 and pValidBytes[k] = !invalid(v[k]) -- which is what
 * lerc_amd_encode_raster_tiles_device_strided makes of the same raster when handed that mask.  Values at invalid pixels, NaN included,
 * never influence a byte; so a float raster with NaN holes and noData = NaN stays inside the masked batches' own launches.
 *   tileCol0, tileRow0, nTileCols, nTileRows   (0, 0, -1, -1): the whole grid.  Anything else follows
 *                lerc_amd_encode_raster_tiles_device_range: a rectangle of the grid's tiles, offsets / sizes stay the full grid's tables
 *                of which only the range's entries are written, and with slotBytes != 0 the range takes rooms 0 .. nRange - 1
 * Offsets, sizes, arenaUsed, slots, shape classes, chunks through the staging buffer, statuses, lerc_amd_last_note,
 * lerc_amd_tile_batch_counters and lerc_amd_raster_tiles_counters are the existing raster calls' with a mask; so are the hand-backs
 * (tiles beyond the size limits, maxZErr 0 on float values, 777).  The raster is never coded where it lies.
 * WrongParam: a NULL pointer, a size < 1, a type that is none, maxZErr < 0, a slotBytes that is no multiple of 16, a pitch below the
 * width, a range that is empty or not inside the grid, a noData that is no element of the type. */
LERC_AMD_API lerc_status lerc_amd_encode_raster_tiles_device_nodata(lerc_amd_context* ctx, const void* dRaster, unsigned int dataType, int nCols,
    int nRows, unsigned long long pixelPitch, unsigned long long rowPitch, int tileCols, int tileRows, int tileCol0, int tileRow0, int nTileCols,
    int nTileRows, double noData, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity, unsigned long long slotBytes,
    unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed);

/* The way back, a window of the mosaic as lerc_amd_decode_raster_window_device: nCols, nRows, the tile size and the full-grid tables
 * describe the mosaic; rows [winRow0, winRow0 + winRows) by columns [winCol0, winCol0 + winCols) of it go into the buffer at dWindow,
 * which holds the window ONLY and is described by pixelPitch and rowPitch.  The whole raster is the window (0, 0, nCols, nRows).
 *   - a valid pixel holds what lerc_amd_decode_raster_window_device writes there;
 *   - an invalid pixel holds (T)noData, a quiet NaN when noData is NaN;
 *   - a tile whose blob fails leaves its part of the window filled with noData and its valid bytes 0; the other tiles are decoded all
 *     the same, and the first such status is returned.
 *   dValidBytes  device, [winRows][maskRowPitch], written 1 / 0, or NULL: for the caller who wants to tell a valid pixel that decoded
 *                to the noData value from a hole.  maskRowPitch >= winCols where it is not NULL
 * Only the tiles the window touches are read and decoded.  Nothing outside [0, winCols) of a row is written, nothing of the destination
 * is read.  WrongParam: as above, and a window that is empty or not inside the raster. */
LERC_AMD_API lerc_status lerc_amd_decode_raster_window_device_nodata(lerc_amd_context* ctx, const unsigned char* dArena,
    const unsigned long long* offsets, const unsigned int* sizes, unsigned int dataType, int nCols, int nRows, int tileCols, int tileRows,
    int winCol0, int winRow0, int winCols, int winRows, void* dWindow, unsigned long long pixelPitch, unsigned long long rowPitch, double noData,
    unsigned char* dValidBytes, unsigned long long maskRowPitch);

#ifdef __cplusplus
}
#endif
#endif
