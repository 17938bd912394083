/*
 * lerc_amd_device.h -- the part of liblerc_amd.so's C ABI that has NO counterpart in Esri/lerc: the codec of
 * lerc_amd.h on DEVICE pointers (synchronous, stream-asynchronous, batched tile mosaics) plus diagnostics.
 * The stock twelve lerc_* entry points are declared in lerc_amd.h (which includes this file).
 */
#ifndef LERC_AMD_DEVICE_H
#define LERC_AMD_DEVICE_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef LERC_AMD_API
#define LERC_AMD_API __attribute__((visibility("default")))
typedef unsigned int lerc_status;
#endif

typedef struct lerc_amd_context lerc_amd_context;

/* hipStream: a hipStream_t cast to void* on which all work is enqueued; NULL is the HIP default
 * (NULL) stream, with its usual ordering against other blocking streams.  A context owns its scratch HBM; use one context per host thread. */
LERC_AMD_API lerc_amd_context* lerc_amd_create(void* hipStream);
LERC_AMD_API void lerc_amd_destroy(lerc_amd_context* ctx);
LERC_AMD_API void lerc_amd_set_stream(lerc_amd_context* ctx, void* hipStream);
LERC_AMD_API const char* lerc_amd_last_error(lerc_amd_context* ctx);

/* Same contracts as lerc_encode / lerc_decode, but pData, pValidBytes, pOutBuffer / pLercBlob are
 * DEVICE pointers.  dOutBuffer == NULL turns lerc_amd_encode_device into the exact size query.
 * The calls return after the stream has been synchronised (the blob size is a host-visible result). */
LERC_AMD_API lerc_status lerc_amd_encode_device(lerc_amd_context* ctx, const void* dData, unsigned int dataType,
    int nDepth, int nCols, int nRows, int nBands, int nMasks, const unsigned char* dValidBytes, double maxZErr,
    unsigned char* dOutBuffer, unsigned int outBufferSize, unsigned int* nBytesWritten);
LERC_AMD_API lerc_status lerc_amd_decode_device(lerc_amd_context* ctx, const unsigned char* dLercBlob,
    unsigned int blobSize, int nMasks, unsigned char* dValidBytes, int nDepth, int nCols, int nRows, int nBands,
    unsigned int dataType, void* dData);

/* The same two calls without the wait: the operation is enqueued on the context's stream and the call returns a ticket.
 * Operations of one context run in the order they were enqueued, so a decode may be enqueued right behind the encode
 * that writes its blob: pass the CAPACITY of the blob buffer as blobSizeBound, the true size is read from the header on
 * the device.  lerc_amd_finish(ctx, ticket, &n) waits for the stream, returns that operation's lerc_status (and, for an
 * encode, the bytes written / needed) and forgets it; ticket 0 waits for everything and drops all results.  Requests
 * the streaming kernels do not take blind (masks, several bands, nDepth > 1, ...) are carried out inside the _async call
 * itself, in order.  If the device hands an operation back to the general path (a constant raster, a damaged blob,
 * ...), lerc_amd_finish repeats it and everything enqueued behind it synchronously -- results are the same as with
 * the synchronous calls, only later.  Buffers must stay untouched until the operation has been finished.  At most 31
 * unfinished results are kept; older ones are completed and dropped. */
LERC_AMD_API lerc_status lerc_amd_encode_device_async(lerc_amd_context* ctx, const void* dData, unsigned int dataType,
    int nDepth, int nCols, int nRows, int nBands, int nMasks, const unsigned char* dValidBytes, double maxZErr,
    unsigned char* dOutBuffer, unsigned int outBufferSize, unsigned int* ticket);
LERC_AMD_API lerc_status lerc_amd_decode_device_async(lerc_amd_context* ctx, const unsigned char* dLercBlob,
    unsigned int blobSizeBound, int nMasks, unsigned char* dValidBytes, int nDepth, int nCols, int nRows, int nBands,
    unsigned int dataType, void* dData, unsigned int* ticket);
LERC_AMD_API lerc_status lerc_amd_finish(lerc_amd_context* ctx, unsigned int ticket, unsigned int* nBytes);

/* Tile mosaics: nTiles rasters of one shape, contiguous on the device ([nTiles][nRows][nCols], 1 band, nDepth 1,
 * no masks -- see the _masked calls below, and the _bands calls for tiles that are band stacks), in ONE call (tiles are independent blobs; ranks of a multi-GPU job take tile ranges).
 * Tile t becomes exactly the blob lerc_encode() would make of it, at dArena + offsets[t] (16-byte aligned), sizes[t]
 * bytes long; offsets / sizes / arenaUsed are HOST arrays the caller provides.  BufferTooSmall(3) if the arena is
 * too small (lerc_computeCompressedSize bounds a tile; nRows * nCols * sizeof(T) + 128 per tile always suffices).
 * Decoding takes the same description back.  Blobs that need the general kernels are handled inside, one by one.
 * 8-bit tiles (int8 / uint8, maxZErr < 1, up to 264 192 pixels and 4 352 blocks of 8 x 8: 256 x 256, 257 x 257, 512 x 512, 513 x 513) are a batch as well, one set of
 * launches and one host wait per sub-batch: statistics, both Huffman code books, the choice between Huffman, delta Huffman and 8 x 8
 * tiling, table, pixel stream and checksum are made on the device, a workgroup per tile.  Handed back and encoded one by one inside the
 * call, with the same bytes: a constant tile, one sweep, the 16 x 16 retry of the low-bit-rate rule (lerc_amd_last_note names the reason).
 * Decoding takes codec 6 blobs of those types in any of the three modes; every other blob (16 x 16 blocks, one sweep, constant, older
 * codecs, a mask section, damaged ...) is decoded by itself inside the call: a blob that fails leaves its tile zeroed, the other tiles
 * are decoded all the same, and the call returns the first such status.  Larger 8-bit tiles and maxZErr >= 1 go one by one as before. */
LERC_AMD_API lerc_status lerc_amd_encode_tiles_device(lerc_amd_context* ctx, const void* dTiles, unsigned int dataType, int nCols,
    int nRows, int nTiles, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity, unsigned long long* offsets,
    unsigned int* sizes, unsigned long long* arenaUsed);
LERC_AMD_API lerc_status lerc_amd_decode_tiles_device(lerc_amd_context* ctx, const unsigned char* dArena,
    const unsigned long long* offsets, const unsigned int* sizes, int nTiles, int nCols, int nRows, unsigned int dataType, void* dTiles);

/* The same with a slot per tile, the way a caller of lerc_encode() hands every tile a buffer of its own: tile t's blob goes to
 * dSlots + t * slotBytes (slotBytes: a multiple of 16, the capacity of every slot), sizes[t] bytes long -- nothing is moved
 * behind the encode kernel (the packed form costs one more pass over the blobs).  BufferTooSmall(3) if a tile's blob does
 * not fit its slot. */
LERC_AMD_API lerc_status lerc_amd_encode_tiles_device_slots(lerc_amd_context* ctx, const void* dTiles, unsigned int dataType, int nCols,
    int nRows, int nTiles, double maxZErr, unsigned char* dSlots, unsigned long long slotBytes, unsigned int* sizes);
LERC_AMD_API lerc_status lerc_amd_decode_tiles_device_slots(lerc_amd_context* ctx, const unsigned char* dSlots, unsigned long long slotBytes,
    const unsigned int* sizes, int nTiles, int nCols, int nRows, unsigned int dataType, void* dTiles);

/* Masked mosaics: nTiles rasters of one shape AND their validity masks, one call.  dValidBytes: device, [nTiles][nRows][nCols] bytes,
 * 0 = invalid (as lerc_encode's pValidBytes with nMasks == 1, per tile); NULL = all valid (then identical to lerc_amd_encode_tiles_device /
 * _slots).  slotBytes == 0: packed arena, offsets[t] 16-byte aligned; slotBytes != 0 (a multiple of 16): tile t at dArena + t * slotBytes,
 * offsets[t] is set to that (arenaCapacity >= nTiles * slotBytes).  Tile t's blob is byte for byte what lerc_encode(tile t, nMasks = 1,
 * mask t) makes; a tile without an invalid pixel gets no mask section.  The batch's own launches (one set per sub-batch, one host wait)
 * take float32, float64 and the 16- and 32-bit integer types, tiles of up to 264 192 pixels and 4 352 blocks of 8 x 8 (256 x 256, 257 x 257, 512 x 512, 513 x 513), and
 * write header, mask section (run-length coded on the device), ranges, block stream and checksum -- of tiles without a valid pixel
 * (header only), constant tiles (header and mask section), one-sweep tiles (the valid pixels raw) and tiles whose low-bit-rate retry
 * ends in 16 x 16 blocks as well.  8-bit tiles (int8 / uint8, maxZErr < 1) WITH a mask pointer are a batch too, the masked form of the
 * 8-bit batch described above: the mask section, both Huffman code books over the valid pixels (the reference's masked predictor), the
 * mode choice, 8 x 8 blocks, table, pixel stream and checksum are made on the device, for partly valid, all-valid and empty tiles
 * alike; handed back and encoded one by one inside the call, same bytes: constant tiles (a single valid pixel included), one sweep,
 * tiles whose 16 x 16 blocks win, a blob that does not fit (lerc_amd_last_note names the reason).  A tile with a NaN at a valid pixel
 * (its mask changes), larger tiles, 8-bit tiles at maxZErr >= 1, maxZErr == 777 or 0 on float values are encoded inside the call, one
 * by one, with the same result (8-bit tiles with dValidBytes == NULL are the 8-bit batch described above).  Status codes as for the
 * unmasked calls. */
LERC_AMD_API lerc_status lerc_amd_encode_tiles_device_masked(lerc_amd_context* ctx, const void* dTiles, unsigned int dataType, int nCols, int nRows,
    int nTiles, const unsigned char* dValidBytes, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity,
    unsigned long long slotBytes, unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed);
/* The way back.  dValidBytes: device, [nTiles][nRows][nCols], written 1 / 0 for EVERY tile (all ones for a blob without a mask section,
 * all zeros for a blob without valid pixels); NULL: the call is lerc_amd_decode_tiles_device (WrongParam(2) as soon as a blob carries a
 * mask).  Pixels: exactly what lerc_amd_decode_device writes for that blob (0 at invalid pixels).  The batch's launches take codec 6
 * blobs of the types and sizes above, with or without a mask section: blocks of 8 x 8 or 16 x 16, one sweep, constant and empty blobs;
 * every other blob (older codecs, damaged, or one the batch's parse is not certain of: bytes behind the last section, a mask whose count
 * of valid pixels is not the header's ...) is decoded by itself inside the call.  8-bit blobs (maxZErr 0.5 in the header), with or
 * without a mask section, in a Huffman mode or with 8 x 8 blocks, and 8-bit blobs without a valid pixel, are the masked 8-bit batch's;
 * constant, one-sweep and 16 x 16 ones go one by one.  A blob that fails leaves its tile zeroed, mask too; the other tiles are
 * decoded all the same, and the call returns the first such status. */
LERC_AMD_API lerc_status lerc_amd_decode_tiles_device_masked(lerc_amd_context* ctx, const unsigned char* dArena, const unsigned long long* offsets,
    const unsigned int* sizes, int nTiles, int nCols, int nRows, unsigned int dataType, void* dTiles, unsigned char* dValidBytes);
/* Mosaics of BAND STACKS: every tile is nBands rasters of one shape, one blob a tile.  dTiles: device, [nTiles][nBands][nRows][nCols];
 * dValidBytes: device, [nTiles][nMasks][nRows][nCols]; nMasks is 0 (dValidBytes must be NULL), 1 (one mask a tile, shared by its bands)
 * or nBands.  slotBytes, offsets, sizes and arenaUsed as in the _masked calls, one blob a tile: a packed tile begins 16-byte aligned,
 * the bands inside a tile are byte-adjacent.  Tile t's blob is byte for byte what lerc_encode(tile t, nDepth 1, nBands, nMasks, mask t,
 * maxZErr) makes: the band blobs back to back, each header naming the number of blobs behind it, the mask section in the first band
 * only.  With nBands == 1 these are the calls above.
 * The batch's own launches (one set per sub-batch, one host wait; the unit is the plane, tile * nBands + band, and a tile is the
 * batch's only if all its planes are) take the wide types -- float32, float64, the 16- and 32-bit integers -- with nMasks 0 or 1, up to
 * 264 192 pixels and 4 352 blocks of 8 x 8 a band: per band its own statistics, error bound (all-integer float values, TryRaiseMaxZError), kind
 * (8 x 8 or 16 x 16 blocks, one sweep, constant, empty) and checksum; the mask's run-length stream once a tile, in band 0 -- the bands
 * behind it carry the header's count of valid pixels and an empty mask section.  With nMasks == 0 the planes run through the masked
 * family's kernels under a mask of all ones, as all-valid tiles inside a masked batch do; the fast one-launch tile encoder of
 * lerc_amd_encode_tiles_device is not involved.  They also take 8-bit stacks (int8 / uint8, maxZErr < 1: lossless) with nMasks 0 or
 * 1, through the masked 8-bit batch's kernels over planes (nMasks == 0: under all ones): per band its own histograms, code book and
 * mode -- Huffman, delta Huffman or 8 x 8 blocks --, the Huffman stream written from whatever byte the band begins at; bands without
 * a valid pixel stay inside.
 * Handed back and encoded one by one inside the call, a whole stack per lerc_amd_encode_device call, same bytes and status
 * (lerc_amd_last_note names tile, band and reason): an 8-bit tile with a band of a kind the 8-bit batch hands back (constant, one
 * sweep, winning 16 x 16 blocks -- the tile goes back whole), 8-bit stacks at maxZErr >= 1, nMasks == nBands (masks per band need the masks-differ comparison and a second mask section), a tile with a NaN at a valid
 * pixel in any band (the mask then changes across the bands), maxZErr 777 or 0 on float values, tiles beyond that size (lerc_amd_last_note then names the size), a blob that does not
 * fit its slot. */
LERC_AMD_API lerc_status lerc_amd_encode_tiles_device_bands(lerc_amd_context* ctx, const void* dTiles, unsigned int dataType, int nCols, int nRows,
    int nBands, int nTiles, int nMasks, const unsigned char* dValidBytes, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity,
    unsigned long long slotBytes, unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed);
/* The way back: pixels and valid bytes exactly as lerc_amd_decode_device(blob t, nMasks, ..., nBands, ...) writes them; dValidBytes is
 * written once a tile, from band 0 (nMasks == 1).  A thread per tile walks the chain of band blobs (band b + 1 begins where band b's
 * header says it ends; every header is checked against nBands, shape and type; the sizes add up to sizes[t]); the planes are then
 * parsed and decoded side by side.  A band behind band 0 whose count of valid pixels lies between none and all takes band 0's mask
 * (Lerc2's "mask stays in force").  Decoded by the single-blob decoder inside the call, a whole stack at a time, with its exact
 * result or status: an 8-bit tile with a constant, one-sweep or 16 x 16 band, nMasks == nBands, codec < 6, a band behind band 0 with a mask section of its own or a count of valid
 * pixels that is not band 0's, nMasks == 0 with an invalid pixel, anything damaged or uncertain.  A tile whose blob fails is left
 * zeroed, all bands and mask; the other tiles are decoded all the same, and the call returns the first such status.
 * lerc_amd_tile_batch_counters counts tiles, not bands. */
LERC_AMD_API lerc_status lerc_amd_decode_tiles_device_bands(lerc_amd_context* ctx, const unsigned char* dArena, const unsigned long long* offsets,
    const unsigned int* sizes, int nTiles, int nCols, int nRows, int nBands, unsigned int dataType, void* dTiles, int nMasks,
    unsigned char* dValidBytes);
/* Diagnostics of the tile batch calls (masked or not): out[0] tiles whose blob the batch's own launches made, out[1] tiles encoded one by
 * one behind the batch, out[2] / out[3] the same for decodes. */
LERC_AMD_API void lerc_amd_tile_batch_counters(lerc_amd_context* ctx, unsigned long long out[4]);

/* Raster mosaics: a raster that lies in device memory as it is -- nBands planes of nRows rows, rowPitch ELEMENTS from row to row
 * (>= nCols) and bandPitch elements from band to band (>= (nRows - 1) * rowPitch + nCols; ignored with one band), a view into a larger
 * allocation included -- is cut into a grid of tiles of tileRows x tileCols and every tile coded, in ONE call.  The grid:
 * nTY = ceil(nRows / tileRows) by nTX = ceil(nCols / tileCols) tiles, tile (ty, tx) has index t = ty * nTX + tx and covers rows
 * [ty * tileRows, min(nRows, (ty + 1) * tileRows)) and the columns likewise: the last row and column of tiles are smaller where the
 * raster is no multiple of the tile.  offsets / sizes: HOST arrays of nTY * nTX entries.  nMasks is 0 (dValidBytes NULL) or 1: one
 * byte mask [nRows][nCols] for the raster, maskRowPitch bytes from row to row, shared by the bands; WrongParam(2) for any other nMasks
 * (a mask per band is not taken here), for a pitch below the width, sizes that are not positive, slotBytes that is no multiple of 16.
 * Tile t's blob is byte for byte what lerc_encode makes of that rectangle (nDepth 1, nBands, nMasks, the rectangle's part of the mask,
 * maxZErr) -- what lerc_amd_encode_tiles_device_bands, _masked or the unmasked tile call makes of the same tile.  slotBytes == 0,
 * packed: every blob begins 16-byte aligned at dArena + offsets[t]; the order in the arena is the call's own.  slotBytes != 0 (a
 * multiple of 16, arenaCapacity >= nTiles * slotBytes): every blob has a room of slotBytes that begins at a multiple of slotBytes,
 * offsets[t] says which -- rooms are handed out per shape class, so room k is not necessarily tile k.  arenaUsed and the status codes
 * as in the tile calls above.
 * Inside, the grid's tiles of one shape -- at most four classes: interior, right column, bottom row, corner -- are gathered, a chunk of
 * at most 256 MiB at a time, into a staging buffer the context owns (one launch a chunk, one more for the mask), and the chunk is
 * handed to the tile calls above: their size limits, hand-backs, lerc_amd_last_note and lerc_amd_tile_batch_counters hold as they
 * stand.  With one band, tiles as wide as the raster (tileCols >= nCols) and no padding (rowPitch == nCols; maskRowPitch == nCols)
 * the tiles lie as a mosaic already and are coded where they lie.  The raster is only read. */
LERC_AMD_API lerc_status lerc_amd_encode_raster_tiles_device(lerc_amd_context* ctx, const void* dRaster, unsigned int dataType, int nCols,
    int nRows, int nBands, unsigned long long rowPitch, unsigned long long bandPitch, int tileCols, int tileRows, int nMasks,
    const unsigned char* dValidBytes, unsigned long long maskRowPitch, double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity,
    unsigned long long slotBytes, unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed);
/* The way back, same description: pixels and valid bytes of every rectangle are exactly what lerc_amd_decode_tiles_device_bands writes
 * for that blob (one band and no mask pointer: what lerc_amd_decode_tiles_device writes).  A blob that fails leaves its rectangle
 * zeroed, all bands and the mask's rectangle; the other tiles are decoded all the same, and the call returns the first such status.
 * Bytes of the raster and of the mask outside [0, nCols) of a row -- the pitch's padding, whatever lies beside a view -- are never
 * written and never read. */
LERC_AMD_API lerc_status lerc_amd_decode_raster_tiles_device(lerc_amd_context* ctx, const unsigned char* dArena, const unsigned long long* offsets,
    const unsigned int* sizes, unsigned int dataType, int nCols, int nRows, int nBands, unsigned long long rowPitch, unsigned long long bandPitch,
    int tileCols, int tileRows, void* dRaster, int nMasks, unsigned char* dValidBytes, unsigned long long maskRowPitch);
/* The two calls above with one more stride: element (band b, row i, column j) lies at dRaster + b * bandPitch + i * rowPitch +
 * j * pixelPitch, all pitches in ELEMENTS, all address arithmetic 64-bit.  Grid, tile order, offsets / sizes / arenaUsed, slots, status
 * codes, hand-backs, lerc_amd_last_note, both counter calls and every blob are those of the calls above: tile t's blob is what
 * lerc_encode makes of that rectangle as a band stack (nDepth 1, nBands, nMasks), whatever the layout it was read from.  The mask stays
 * one [nRows][nCols] byte plane with maskRowPitch.  The layouts taken, WrongParam(2) for every other description:
 *  - pixelPitch == 1, band-sequential (rowPitch >= nCols, bandPitch >= (nRows - 1) * rowPitch + nCols): the call IS the call above, same
 *    checks, same path (coded where it lies included), same counters.
 *  - pixelPitch == 1, line-interleaved (BIL): nBands > 1, bandPitch >= nCols, rowPitch >= (nBands - 1) * bandPitch + nCols.
 *  - pixelPitch >= 2, pixel-interleaved (RGB / RGBA frames, [H, W, C] tensors, GDAL's INTERLEAVE=PIXEL): nBands == 1 (one channel of
 *    an interleaved image, dRaster pointing at it; bandPitch ignored), or bandPitch == 1 and nBands <= pixelPitch;
 *    rowPitch >= (nCols - 1) * pixelPitch + nBands.  pixelPitch > nBands is a raster with channels that are not coded (RGB out of RGBA, a
 *    slice of a channel axis): the elements between a pixel's last band and the next pixel, like the row padding and whatever lies
 *    beside a view, are never written by the decode and their values never used by either call (the encode fetches a row from band 0
 *    of its first pixel to the last band of its last pixel in whole 16-byte vectors, nothing in front or behind).
 * A pixel-interleaved raster always goes through the staging buffer (out[0] / out[2] of lerc_amd_raster_tiles_counters); the
 * transposition is done by the kernels that fill and empty it (k_rt_cut_px / k_rt_paste_px), so the caller needs no planar copy.
 * A pixelPitch of more than 8 elements is taken by a plain form of those kernels (a lane an element): same results, slower. */
LERC_AMD_API lerc_status lerc_amd_encode_raster_tiles_device_strided(lerc_amd_context* ctx, const void* dRaster, unsigned int dataType, int nCols,
    int nRows, int nBands, unsigned long long pixelPitch, unsigned long long rowPitch, unsigned long long bandPitch, int tileCols, int tileRows,
    int nMasks, const unsigned char* dValidBytes, unsigned long long maskRowPitch, double maxZErr, unsigned char* dArena,
    unsigned long long arenaCapacity, unsigned long long slotBytes, unsigned long long* offsets, unsigned int* sizes, unsigned long long* arenaUsed);
LERC_AMD_API lerc_status lerc_amd_decode_raster_tiles_device_strided(lerc_amd_context* ctx, const unsigned char* dArena,
    const unsigned long long* offsets, const unsigned int* sizes, unsigned int dataType, int nCols, int nRows, int nBands,
    unsigned long long pixelPitch, unsigned long long rowPitch, unsigned long long bandPitch, int tileCols, int tileRows, void* dRaster, int nMasks,
    unsigned char* dValidBytes, unsigned long long maskRowPitch);
/* A RANGE of the grid's tiles, coded: lerc_amd_encode_raster_tiles_device_strided with tileCol0, tileRow0, nTileCols, nTileRows behind
 * tileRows.  dRaster and its sizes, pitches and mask describe the WHOLE raster, as above; only the tiles (ty, tx) with tileRow0 <= ty <
 * tileRow0 + nTileRows and tileCol0 <= tx < tileCol0 + nTileCols are cut and coded -- the tiles a dirty region touches, a rank's rows of
 * tiles.  offsets / sizes stay the full grid's tables (nTY * nTX entries, tile order as above): only the range's entries are written.
 * Offsets are relative to dArena; packed, 16-byte aligned; slotted, the range's tiles take rooms 0 .. nRange - 1 (nRange = nTileRows *
 * nTileCols) and arenaCapacity >= nRange * slotBytes, else BufferTooSmall(3).  arenaUsed counts the range only.  Every blob is byte
 * for byte what the whole-raster call makes of that tile; coded where they lie under the condition above (a range of tile rows then).
 * WrongParam(2) for an empty range or one not inside the grid. */
LERC_AMD_API lerc_status lerc_amd_encode_raster_tiles_device_range(lerc_amd_context* ctx, const void* dRaster, unsigned int dataType, int nCols,
    int nRows, int nBands, unsigned long long pixelPitch, unsigned long long rowPitch, unsigned long long bandPitch, int tileCols, int tileRows,
    int tileCol0, int tileRow0, int nTileCols, int nTileRows, int nMasks, const unsigned char* dValidBytes, unsigned long long maskRowPitch,
    double maxZErr, unsigned char* dArena, unsigned long long arenaCapacity, unsigned long long slotBytes, unsigned long long* offsets,
    unsigned int* sizes, unsigned long long* arenaUsed);
/* A WINDOW of a mosaic, decoded: rows [winRow0, winRow0 + winRows) by columns [winCol0, winCol0 + winCols) of the raster, into a buffer
 * of the caller's that holds the window only.  nCols, nRows, tileCols, tileRows describe the mosaic and its grid as above; offsets /
 * sizes are the full grid's HOST tables, of which only the entries of tiles that intersect the window are read, and only those tiles
 * are decoded.  Element (band b, row i, column j) of the window is pixel (winRow0 + i, winCol0 + j) of band b and lies at dWindow +
 * b * bandPitch + i * rowPitch + j * pixelPitch (ELEMENTS); the layouts are those of the _strided calls with their rules applied to
 * winCols / winRows: band-sequential, line-interleaved, pixel-interleaved with nBands <= pixelPitch (the plain kernel form above 8).
 * dValidBytes (nMasks 1): the window's mask, [winRows][winCols] bytes, maskRowPitch >= winCols from row to row; NULL with nMasks 0.
 * Pixels and valid bytes are exactly what lerc_amd_decode_raster_tiles_device[_strided] writes at those positions for the same blobs.
 * Nothing outside [0, winCols) of a window row is written -- gaps between pixels, row padding, whatever lies beside a view -- and
 * nothing of the destination is read.  A blob that fails leaves its part of the window zeroed, all bands and the mask's part; the
 * other tiles are decoded all the same, and the call returns the first such status.  WrongParam(2) for a window with a size that is
 * not positive or one not inside [0, nRows) x [0, nCols), a layout the strided calls would refuse for a raster of the window's size,
 * nMasks other than 0 or 1.  The window's tiles always go through the staging buffer (out[2] of lerc_amd_raster_tiles_counters: the
 * intersecting tiles), a chunk of a shape class at a time as above, and are written by a clipped paste (k_rw_paste / k_rw_paste_px). */
LERC_AMD_API lerc_status lerc_amd_decode_raster_window_device(lerc_amd_context* ctx, const unsigned char* dArena, const unsigned long long* offsets,
    const unsigned int* sizes, unsigned int dataType, int nCols, int nRows, int nBands, int tileCols, int tileRows, int winCol0, int winRow0,
    int winCols, int winRows, void* dWindow, unsigned long long pixelPitch, unsigned long long rowPitch, unsigned long long bandPitch, int nMasks,
    unsigned char* dValidBytes, unsigned long long maskRowPitch);
/* Diagnostics of the calls above: tiles out[0] cut through the staging buffer, out[1] encoded where they lie, out[2] pasted from
 * the staging buffer, out[3] decoded where they lie. */
LERC_AMD_API void lerc_amd_raster_tiles_counters(lerc_amd_context* ctx, unsigned long long out[4]);

/* Per-kernel timing with HIP events on the context's stream (used by bench.py for the roofline of the
 * dominant kernel).  lerc_amd_profile_read writes lines "kernel_group total_ms launches" into buf. */
LERC_AMD_API void lerc_amd_profile_enable(lerc_amd_context* ctx, int on);
LERC_AMD_API int lerc_amd_profile_read(lerc_amd_context* ctx, char* buf, int cap, int reset);

/* Which kernels served the successful calls of a context so far: out[0] encodes by the streaming kernels, out[1]
 * encodes by the general kernels, out[2] / out[3] the same for decodes.  ctx == NULL: the calling thread's context
 * behind lerc_encode / lerc_decode.  Diagnostics only (tests assert that the streaming path really ran). */
LERC_AMD_API void lerc_amd_path_counters(lerc_amd_context* ctx, unsigned long long out[4]);
/* Which of the streaming decoders served the bands / tiles counted in out[2] above: out[3] the scanning decoder (one launch, no
 * walks), out[2] the walking one-launch decoder, out[1] discovery + decode in two launches; out[0] counts bands WITH a mask whose blocks the scanning decoder's first half found
 * (the general kernels decode their pixels).  Same ctx convention. */
LERC_AMD_API void lerc_amd_decode_forms(lerc_amd_context* ctx, unsigned long long out[4]);
/* The mosaic job's ONE exchange step (the reference has no counterpart: whoever tiles a mosaic moves the blobs
 * himself): the gather of the ranks' compressed blobs on the rank that writes the container, over RCCL -- xGMI inside a node.
 *   ncclComm      an ncclComm_t of the caller's (ncclCommInitRank; librccl is opened with dlopen when this is first called, inside a
 *                 PyTorch process that is the RCCL torch.distributed uses); rank and size are the communicator's
 *   dMessage      this rank's message, nBytes of device memory: its arena as lerc_amd_encode_tiles_device left it -- with the per-tile
 *                 (offset, size) table in front, if the caller laid it out so: one message a rank
 *   dRootBuffer   on the root: where the messages land, rank r's at hOffsets[r] (16-byte aligned, back to back); ignored elsewhere
 *   hLengths      out, host, one word a rank: every rank's message length (all ranks get them); may be NULL
 *   hOffsets      out, host, ranks + 1 words; may be NULL
 *   stream        the HIP stream everything is enqueued on: one ncclAllGather of the lengths, then a sender's ncclSend at once (it needs
 *                 nobody's length but its own), on the root one group of ncclRecv behind the only host wait there is (the lengths, 8 bytes
 *                 a rank through pinned memory) and a copy of its own message.  The call returns when the transfers are POSTED; wait
 *                 for the stream before the bytes are read.  Order it behind the encodes' stream with an event.
 * Returns 0, 2 (WrongParam), 3 (BufferTooSmall: rootCapacity), 1 (Failed: lerc_amd_last_error says which RCCL call). */
LERC_AMD_API unsigned int lerc_amd_gather_blobs(lerc_amd_context* ctx, void* ncclComm, int root, const void* dMessage, unsigned long long nBytes,
                                                void* dRootBuffer, unsigned long long rootCapacity, unsigned long long* hLengths,
                                                unsigned long long* hOffsets, void* stream);
/* Attempts that were thrown away on the way down the tiers -- each is a launch (or several) whose result nobody used: out[0] the decode
 * kernels refused the block offsets the scan had proposed for a band with a mask (a raw block's length is a guess there; the general
 * discovery then takes the band), out[1] that scan handed a masked band on by itself, out[2] a streaming decode tier (scan, walk, two
 * launches) handed a band to the next one; out[3] unused.  Same ctx convention. */
LERC_AMD_API void lerc_amd_decode_refusals(lerc_amd_context* ctx, unsigned long long out[4]);
/* why the last call that left the streaming kernels did so ("" if none did); same ctx convention */
LERC_AMD_API const char* lerc_amd_last_note(lerc_amd_context* ctx);

/* The run-length coding of a validity BIT mask (the mask section of a Lerc2 blob, RLE.cpp:123-254: nBytes = (nPix + 7) / 8
 * bytes, most significant bit first) on the device, as the masked encode uses it: dBits and dOut device pointers (dBits 16-byte
 * aligned), *size = bytes written incl. the end marker.  Returns 0, or 3 (BufferTooSmall) if the stream does not fit cap. */
LERC_AMD_API unsigned int lerc_amd_mask_rle_device(lerc_amd_context* ctx, const unsigned char* dBits, unsigned int nBytes,
                                                   unsigned char* dOut, unsigned int cap, unsigned int* size);

/* The other way, as the masked decode uses it: nBytes mask bytes out of a stream of rleBytes bytes (RLE.cpp:259-330); what the
 * stream does not hold stays zero.  Returns 0, or 1 (Failed) for a damaged stream (no end marker, a segment that runs over
 * either end). */
LERC_AMD_API unsigned int lerc_amd_mask_rle_decode_device(lerc_amd_context* ctx, const unsigned char* dRle, unsigned int rleBytes,
                                                          unsigned char* dBits, unsigned int nBytes);

/* library / build identification: "lerc_amd <version> gfx950 hip" (or "... hipsim" for the CPU test build) */
LERC_AMD_API const char* lerc_amd_build_info(void);

#ifdef __cplusplus
}
#endif
#endif
