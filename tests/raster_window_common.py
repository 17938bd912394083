"""Shared by test_sim_raster_window.py (CPU emulator library) and test_gpu_raster_window.py (MI355X): a driver for
lerc_amd_decode_raster_window_device and lerc_amd_encode_raster_tiles_device_range (include/lerc_amd_device.h), and the checks.  The
judge is raster_tiles_common's: the reference's blobs of the numpy slices, and the raster assembled from its decode of every tile, of
which a window is a slice.  A window must also be bit-equal to the same slice of what lerc_amd_decode_raster_tiles_device writes.

Addressing: the window's buffer is a raster_px_common.StridedLayout of the WINDOW's size (planes with padding, line-interleaved,
pixel-interleaved), GUARD + 1 elements into its allocation, rows 5 elements longer than they need to be; guards, padding and the gaps
between the pixels hold the sentinel and must still do so after the decode.  The window's mask has a pitch of its own, winCols + 3.
"""
import ctypes as ct

import numpy as np

import capi
import raster_px_common as PX
import raster_tiles_common as RT

T = RT.T
ALL_CLASSES, THIN_EDGES = RT.ALL_CLASSES, RT.THIN_EDGES

# (row0, col0, rows, cols) on ALL_CLASSES (83 x 101, tiles 32 x 40), and the tiles that may be decoded
WINDOWS = [((0, 0, 83, 101), 9), ((40, 50, 1, 1), 1), ((33, 41, 27, 37), 1), ((32, 40, 32, 40), 1), ((31, 39, 34, 42), 9),
           ((17, 23, 66, 78), 9), ((70, 90, 13, 11), 1)]
THIN_WINDOW = ((30, 45, 3, 4), 4)        # on THIN_EDGES (33 x 49, tiles 16 x 24): four tiles, the 1 x 1 corner among them
CLIPPED = (17, 23, 66, 78)               # all four classes, clipped at the top and on the left
OVER_EVERY_EDGE = (31, 39, 34, 42)

# (dtype, maxZErr, nBands, mask, how the window's buffer lies, window): types x destinations, not the full product
PLANES, LINES = ("planes",), ("lines",)
CASES = [
    (np.uint8, 0, 1, True, PLANES, CLIPPED),
    (np.uint8, 0, 3, True, ("pixels", 3), CLIPPED),
    (np.uint8, 0, 3, False, ("pixels", 4), OVER_EVERY_EDGE),
    (np.uint8, 0, 3, True, LINES, CLIPPED),
    (np.uint16, 0, 1, False, PLANES, OVER_EVERY_EDGE),
    (np.uint16, 0, 3, False, ("pixels", 3), CLIPPED),
    (np.uint16, 0, 3, True, ("pixels", 11), CLIPPED),        # (the plain form: a pixel pitch above 8 elements)
    (np.uint16, 0, 1, False, ("pixels", 2), CLIPPED),        # (one channel of an interleaved image)
    (np.float32, 0.01, 1, True, PLANES, CLIPPED),
    (np.float32, 0.01, 3, True, ("pixels", 4), CLIPPED),
    (np.float32, 0.01, 3, False, LINES, OVER_EVERY_EDGE),
    (np.float32, 0.01, 3, False, ("pixels", 3), OVER_EVERY_EDGE),
    (np.float64, 0.001, 1, True, PLANES, CLIPPED),
    (np.float64, 0.001, 3, False, ("pixels", 3), CLIPPED),
    (np.float64, 0.001, 3, True, PLANES, OVER_EVERY_EDGE),
]

# (tileRow0, tileCol0, nTileRows, nTileCols) on ALL_CLASSES' grid of 3 x 3
RANGES = [(0, 0, 3, 3), (1, 1, 1, 1), (2, 0, 1, 3), (0, 2, 3, 1), (2, 2, 1, 1), (1, 1, 2, 2)]

DEAD64, DEAD32 = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF      # table entries of tiles the window decode must not read
KEPT64, KEPT32 = 0xEEEEEEEEEEEEEEEE, 0xEEEEEEEE      # table entries the range encode must not write


def case_id(case):
    dtype, e, nb, with_mask, how, win = case
    return "%s%s%s-%s-%s" % ("%dx" % nb if nb > 1 else "", np.dtype(dtype).name, "-mask" if with_mask else "", "".join(str(v) for v in how),
                             "x".join(str(v) for v in win))


def bind(L):
    PX.bind(L)
    vp, u64, u32, i = ct.c_void_p, ct.c_ulonglong, ct.c_uint, ct.c_int
    L.lerc_amd_encode_raster_tiles_device_range.restype = u32
    L.lerc_amd_encode_raster_tiles_device_range.argtypes = [vp, vp, u32, i, i, i, u64, u64, u64, i, i, i, i, i, i, i, vp, u64, ct.c_double, vp, u64, u64,
                                                            vp, vp, vp]
    L.lerc_amd_decode_raster_window_device.restype = u32
    L.lerc_amd_decode_raster_window_device.argtypes = [vp, vp, vp, vp, u32, i, i, i, i, i, i, i, i, i, vp, u64, u64, u64, i, vp, u64]
    return L


def window_tiles(n_rows, n_cols, tile, window):
    """indices, in tile order, of the tiles the window (row0, col0, rows, cols) touches"""
    r0, c0, h, w = window
    return [t for t, (a0, a1, b0, b1) in enumerate(RT.grid(n_rows, n_cols, tile)) if a0 < r0 + h and r0 < a1 and b0 < c0 + w and c0 < b1]


def range_tiles(n_rows, n_cols, tile, rng):
    ty0, tx0, nty, ntx = rng
    n_tx = -(-n_cols // tile[1])
    return [ty * n_tx + tx for ty in range(ty0, ty0 + nty) for tx in range(tx0, tx0 + ntx)]


def dest(how, nb, h, w, dtype):
    """the window's buffer: a StridedLayout of the window's size"""
    if how[0] == "planes":
        return PX.StridedLayout.planes(nb, h, w, dtype)
    if how[0] == "lines":
        return PX.StridedLayout.lines(nb, h, w, dtype)
    return PX.StridedLayout.pixels(nb, h, w, dtype, how[1], **(how[2] if len(how) > 2 else {}))


def lay_arena(blobs):
    """blobs (None: no blob for that tile) at 16-byte aligned offsets -> (arena bytes, offsets, sizes); a tile without a blob gets the
    dead entries"""
    n = len(blobs)
    offs = np.full(n, DEAD64, np.uint64)
    sizes = np.full(n, DEAD32, np.uint32)
    at = 0
    for t, b in enumerate(blobs):
        if b is not None:
            offs[t], sizes[t] = at, len(b)
            at += (len(b) + 15) & ~15
    arena = np.zeros(at + 64, np.uint8)
    for t, b in enumerate(blobs):
        if b is not None:
            arena[int(offs[t]):int(offs[t]) + len(b)] = np.frombuffer(b, np.uint8)
    return arena, offs, sizes


class WindowBatch(PX.PxBatch):
    """one context of library L: the window decode and the tile range encode beside PxBatch's calls"""

    def __init__(self, L, mem):
        bind(L)
        PX.PxBatch.__init__(self, L, mem)

    def decode_window(self, blobs, shape, dtype, tile, window, how, with_mask, table=None, mask_pad=3, **told):
        """blobs in tile order (None: that tile's table entries are dead), or table = (arena address, offsets, sizes) of an arena that
        lies on the device already -> (status, pixels [nb, h, w], valid [h, w] or None); asserts that everything in the window's and
        the mask's buffer that is no element of the window still holds the sentinel.  told: what the call is told where that is not
        the truth (window_arg, pixel_pitch, pitch, band_pitch, n_bands, n_masks, mask_pitch)"""
        nb, n_rows, n_cols = shape
        r0, c0, h, w = window
        if table is None:
            arena, offs, sizes = lay_arena(blobs)
            ka, pa = self.mem.up(arena)
        else:
            pa, offs, sizes = table
        assert len(offs) == len(sizes) == len(RT.grid(n_rows, n_cols, tile))
        lay = dest(how, nb, h, w, dtype)
        kr, pr = self.mem.up(lay.fill())
        mlay = RT.Layout(1, h, w, np.uint8, mask_pad) if with_mask else None
        km, pm = self.mem.up(mlay.fill()) if with_mask else (None, None)
        tr0, tc0, th, tw = told.get("window_arg", window)
        rc = self.L.lerc_amd_decode_raster_window_device(
            self.h, pa, offs.ctypes.data, sizes.ctypes.data, capi.dt_code(dtype), n_cols, n_rows, told.get("n_bands", nb), tile[1], tile[0],
            tc0, tr0, tw, th, lay.address(pr), told.get("pixel_pitch", lay.pixel_pitch), told.get("pitch", lay.pitch),
            told.get("band_pitch", lay.band_pitch), told.get("n_masks", 1 if with_mask else 0), mlay.address(pm) if with_mask else None,
            told.get("mask_pitch", mlay.pitch if with_mask else 0))
        pix, clean = lay.take(self.mem.down(kr))
        assert clean, "the decode wrote beside the window's elements"
        valid = None
        if with_mask:
            valid, clean = mlay.take(self.mem.down(km))
            assert clean, "the decode wrote outside the window's mask rows"
            valid = valid[0]
        return rc, pix, valid

    def encode_range(self, lay, raster, mask, e, tile, rng, slot_bytes=0, arena_cap=None, mask_pad=3, **told):
        """raster [nb, R, C] laid out as `lay` says, the tiles of rng = (tileRow0, tileCol0, nTileRows, nTileCols)
        -> (status, {tile: blob} of the range, offsets, sizes, arena bytes used, (arena, its address)); offsets / sizes are full-grid
        tables that held KEPT64 / KEPT32 before the call.  told: range"""
        nb, n_rows, n_cols = raster.shape
        src = lay.fill(raster)
        kr, pr = self.mem.up(src)
        mlay = RT.Layout(1, n_rows, n_cols, np.uint8, mask_pad) if mask is not None else None
        msrc = mlay.fill(mask) if mask is not None else None
        km, pm = self.mem.up(msrc) if mask is not None else (None, None)
        n = len(RT.grid(n_rows, n_cols, tile))
        members = range_tiles(n_rows, n_cols, tile, rng)
        per_tile = min(tile[0], n_rows) * min(tile[1], n_cols)
        cap = int(arena_cap) if arena_cap is not None else len(members) * (slot_bytes if slot_bytes else nb * (per_tile * raster.itemsize + per_tile // 4 + 1024) + 16)
        ka, pa = self.mem.empty(cap + 16)
        offs = np.full(n, KEPT64, np.uint64)
        sizes = np.full(n, KEPT32, np.uint32)
        used = ct.c_ulonglong(0)
        ty0, tx0, nty, ntx = told.get("range", rng)
        rc = self.L.lerc_amd_encode_raster_tiles_device_range(
            self.h, lay.address(pr), capi.dt_code(raster.dtype), n_cols, n_rows, nb, lay.pixel_pitch, lay.pitch, lay.band_pitch, tile[1], tile[0],
            tx0, ty0, ntx, nty, 0 if mask is None else 1, mlay.address(pm) if mask is not None else None, mlay.pitch if mask is not None else 0,
            float(e), pa, cap, int(slot_bytes), offs.ctypes.data, sizes.ctypes.data, ct.byref(used))
        assert np.array_equal(self.mem.down(kr)[:len(src)], src), "the encode changed its source"
        if mask is not None:
            assert np.array_equal(self.mem.down(km)[:len(msrc)], msrc), "the encode changed its mask"
        arena = self.mem.down(ka)
        blobs = {}
        if rc == 0:
            outside = np.ones(n, bool)
            outside[members] = False
            assert (offs[outside] == KEPT64).all() and (sizes[outside] == KEPT32).all(), "table entries outside the range were written"
            blobs = {t: arena[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() for t in members}
            assert arena[cap:cap + 16].tolist() == [0xCD] * 16, "bytes behind the arena were written"
        return rc, blobs, offs, sizes, int(used.value), (ka, pa)


# ---- content: a raster, the reference's blobs of its tiles and the raster the reference decodes from them; made once a key -------------
class Content:
    pass


_CONTENT = {}
_WHOLE = {}


def content(R, dtype, e, nb, with_mask, shape_tile, noisy=False):
    key = (np.dtype(dtype).name, e, nb, with_mask, shape_tile, noisy)
    if key in _CONTENT:
        return _CONTENT[key]
    (n_rows, n_cols), tile = shape_tile
    C = Content()
    C.key, C.tile, C.with_mask, C.e = key, tile, with_mask, e
    C.raster = RT.noisy_float(n_rows, n_cols) if noisy else RT.raster_of(dtype, nb, n_rows, n_cols)
    C.mask = RT.mask_of(n_rows, n_cols) if with_mask else None
    C.blobs = RT.ref_blobs(R, C.raster, C.mask, e, tile)
    C.ref_pix = np.zeros(C.raster.shape, C.raster.dtype)
    C.ref_valid = np.zeros((n_rows, n_cols), np.uint8)
    for t, (r0, r1, c0, c1) in enumerate(RT.grid(n_rows, n_cols, tile)):
        rc, p, m = R.decode(C.blobs[t], want_masks=1, n_bands=nb)
        assert rc == 0
        C.ref_pix[:, r0:r1, c0:c1] = np.asarray(p).reshape(nb, r1 - r0, c1 - c0)
        C.ref_valid[r0:r1, c0:c1] = m[0]
    C.ref_pix.setflags(write=False)
    C.ref_valid.setflags(write=False)
    _CONTENT[key] = C
    return C


def whole(B, C):
    """what lerc_amd_decode_raster_tiles_device of B's library writes for C's blobs: (pixels, valid or None), made once a library"""
    key = (id(B.L), C.key)
    if key not in _WHOLE:
        rc, pix, valid = B.decode_raster(C.blobs, C.raster.shape, C.raster.dtype, C.tile, C.with_mask)
        assert rc == 0
        _WHOLE[key] = (pix, valid)
    return _WHOLE[key]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def compare_window(B, C, window, pix, valid):
    """the window's pixels and valid bytes against the slice of the reference's raster (at valid pixels) and of the whole-raster call's"""
    r0, c0, h, w = window
    rows, cols = slice(r0, r0 + h), slice(c0, c0 + w)
    m = C.ref_valid[rows, cols] > 0
    if C.with_mask:
        assert np.array_equal(valid, C.ref_valid[rows, cols]), "valid bytes differ from the reference's"
    else:
        assert m.all() and valid is None
    for k in range(C.raster.shape[0]):
        assert same_bits(pix[k][m], C.ref_pix[k, rows, cols][m]), "band %d: valid pixels differ from the reference's" % k
    whole_pix, whole_valid = whole(B, C)
    assert same_bits(pix, whole_pix[:, rows, cols]), "pixels differ from the whole-raster decode's"
    if C.with_mask:
        assert np.array_equal(valid, whole_valid[rows, cols])


def check_window(B, C, window, how, n_tiles=None, blobs=None):
    """-> (pixels, valid).  n_tiles: the tiles that may be decoded (out[2] of the raster counters, and the tile batches' decodes)"""
    (n_rows, n_cols) = C.raster.shape[1:]
    whole(B, C)    # (before the counters are read)
    r0, b0 = B.raster_counters(), B.counters()
    rc, pix, valid = B.decode_window(C.blobs if blobs is None else blobs, C.raster.shape, C.raster.dtype, C.tile, window, how, C.with_mask)
    assert rc == 0, (rc, B.note())
    r1, b1 = B.raster_counters(), B.counters()
    touched = window_tiles(n_rows, n_cols, C.tile, window)
    assert n_tiles is None or len(touched) == n_tiles
    assert PX.delta(r0, r1) == [0, 0, len(touched), 0], (r0, r1)
    assert PX.delta(b0, b1)[:2] == [0, 0] and sum(PX.delta(b0, b1)[2:]) == len(touched), (b0, b1)
    compare_window(B, C, window, pix, valid)
    return pix, valid


def check_windows(B, R, window, n_tiles, shape_tile=ALL_CLASSES):
    """float32 at 0.01 with a mask into planes, and uint8 x 3 into RGB pixels"""
    check_window(B, content(R, np.float32, 0.01, 1, True, shape_tile), window, PLANES, n_tiles)
    check_window(B, content(R, np.uint8, 0, 3, False, shape_tile), window, ("pixels", 3), n_tiles)


def check_case(B, R, case):
    dtype, e, nb, with_mask, how, window = case
    check_window(B, content(R, dtype, e, nb, with_mask, ALL_CLASSES), window, how)


def check_alignment_sweep(B, R):
    """uint8 x 3, 16 x 80 at tiles of 16 x 40: windows of 33 columns from every column 0 .. 16 on -- the staged rows are read from every
    offset into a 16-byte vector, and the second tile lands at every offset of the window's rows"""
    C = content(R, np.uint8, 0, 3, False, ((16, 80), (16, 40)))
    for c0 in range(17):
        for how in (PLANES, ("pixels", 3)):
            check_window(B, C, (0, c0, 16, 33), how, 2 if c0 + 33 > 40 else 1)


def check_only_the_windows_tiles(B, R):
    """the table entries of every tile outside the window are dead: the same result, status 0, and the counters move by the window's tiles"""
    for C, how in ((content(R, np.float32, 0.01, 1, True, ALL_CLASSES), PLANES), (content(R, np.uint8, 0, 3, False, ALL_CLASSES), ("pixels", 3))):
        n_rows, n_cols = C.raster.shape[1:]
        for window, n_tiles in ((33, 41, 27, 37), 1), ((40, 50, 30, 45), 4), ((0, 0, 20, 101), 3):
            touched = window_tiles(n_rows, n_cols, C.tile, window)
            blobs = [b if t in touched else None for t, b in enumerate(C.blobs)]
            check_window(B, C, window, how, n_tiles, blobs=blobs)


def check_chunks(B, R):
    """chunks of 2 tiles, tile sub-batches of 1: the same bytes"""
    for C, how in ((content(R, np.float32, 0.01, 1, True, ALL_CLASSES), PLANES), (content(R, np.uint8, 0, 3, True, ALL_CLASSES), ("pixels", 4)),
                   (content(R, np.uint16, 0, 1, False, ALL_CLASSES), PLANES)):
        plain = check_window(B, C, CLIPPED, how, 9)
        with RT.knobs(LERC_AMD_TEST_RASTER_CHUNK=2, LERC_AMD_TEST_TILE_SUBBATCH=1):
            chunked = check_window(B, C, CLIPPED, how, 9)
        assert same_bits(plain[0], chunked[0]) and (plain[1] is None or np.array_equal(plain[1], chunked[1]))


def damaged(blob):
    bad = bytearray(blob)
    bad[len(bad) - 9] ^= 0x10    # (a bit flipped under the old checksum, as raster_tiles_common.check_failing_tile)
    return bytes(bad)


def check_damaged_blob(B, R):
    """tile 4 damaged, window (40, 50, 30, 45) over tiles 4, 5, 7, 8: the part of tile 4 inside the window is zero in every band and in
    the mask, all else is right, and the reference's status comes back.  Tile 0 damaged, which the window misses: status 0"""
    window, how_list = (40, 50, 30, 45), (PLANES, ("pixels", 4))
    for C, how in zip((content(R, np.float32, 0.01, 1, True, ALL_CLASSES, noisy=True), content(R, np.uint8, 0, 3, True, ALL_CLASSES)), how_list):
        n_rows, n_cols = C.raster.shape[1:]
        good_pix, good_valid = check_window(B, C, window, how, 4)
        bad = damaged(C.blobs[4])
        want_rc = R.decode(bad, want_masks=1, n_bands=C.raster.shape[0])[0]
        assert want_rc != 0
        rc, pix, valid = B.decode_window(C.blobs[:4] + [bad] + C.blobs[5:], C.raster.shape, C.raster.dtype, C.tile, window, how, True)
        assert rc == want_rc, (rc, want_rc)
        r0, r1, c0, c1 = RT.grid(n_rows, n_cols, C.tile)[4]
        part = (slice(max(r0, window[0]) - window[0], min(r1, window[0] + window[2]) - window[0]),
                slice(max(c0, window[1]) - window[1], min(c1, window[1] + window[3]) - window[1]))
        assert pix[(slice(None),) + part].size and not pix[(slice(None),) + part].any() and not valid[part].any()
        others = np.ones((window[2], window[3]), bool)
        others[part] = False
        assert same_bits(pix[:, others], good_pix[:, others]) and np.array_equal(valid[others], good_valid[others])
        rc, pix, valid = B.decode_window([damaged(C.blobs[0])] + C.blobs[1:], C.raster.shape, C.raster.dtype, C.tile, window, how, True)
        assert rc == 0 and same_bits(pix, good_pix) and np.array_equal(valid, good_valid)


def check_window_arguments(B, R):
    C = content(R, np.uint8, 0, 3, True, ALL_CLASSES)
    window = (17, 23, 66, 78)

    def call(how=("pixels", 3), **told):
        return B.decode_window(C.blobs, C.raster.shape, C.raster.dtype, C.tile, window, how, True, **told)[0]
    assert call() == 0
    for bad in ((17, 23, 0, 78), (17, 23, 66, 0), (17, 23, -1, 78), (-1, 23, 66, 78), (17, -1, 66, 78), (18, 23, 66, 78), (17, 24, 66, 78),
                (83, 23, 1, 1), (17, 101, 1, 1)):
        assert call(window_arg=bad) == 2, bad
    assert call(window_arg=(17, 23, 66, 78)) == 0 and call(window_arg=(82, 100, 1, 1)) == 0
    # layouts the strided calls refuse for a raster of the window's size
    assert call(pixel_pitch=0) == 2
    assert call(n_bands=4) == 2                                      # (pixelPitch 3, nBands 4)
    assert call(band_pitch=2) == 2
    assert call(pitch=(78 - 1) * 3 + 3 - 1) == 2
    assert call(how=PLANES) == 0 and call(how=PLANES, pitch=77) == 2
    assert call(how=PLANES, band_pitch=65 * (78 + 5) + 78 - 1) == 2
    assert call(how=LINES) == 0 and call(how=LINES, band_pitch=77) == 2
    assert call(n_masks=2) == 2 and call(n_masks=0) == 2             # (a mask pointer with nMasks 0)
    assert call(mask_pitch=77) == 2


# ---- the tile range encode --------------------------------------------------------------------------------------------------------
def check_range(B, lay, raster, mask, e, tile, rng, want, slot_bytes=0):
    """-> the range's blobs by tile"""
    n_rows, n_cols = raster.shape[1:]
    members = range_tiles(n_rows, n_cols, tile, rng)
    rc, blobs, offs, sizes, used, _ = B.encode_range(lay, raster, mask, e, tile, rng, slot_bytes=slot_bytes)
    assert rc == 0, (rc, B.note())
    for t in members:
        assert T.same_blob(blobs[t], want[t], raster.itemsize), "tile %d: %d bytes, the reference makes %d (%s)" % (t, len(blobs[t]), len(want[t]), B.note())
    RT.check_layout(offs[members], sizes[members], used, slot_bytes)
    if slot_bytes:
        assert used == len(members) * slot_bytes
    return blobs


def check_ranges(B, R, rng):
    """uint16 planes: packed and slotted, BufferTooSmall(3) one byte under nRange * slotBytes; the whole grid equals the existing call"""
    C = content(R, np.uint16, 0, 1, False, ALL_CLASSES)
    n_rows, n_cols = C.raster.shape[1:]
    lay = PX.StridedLayout.planes(1, n_rows, n_cols, np.uint16)
    slot = RT.slot_for(C.raster, C.tile)
    n_range = rng[2] * rng[3]
    c0 = B.raster_counters()
    check_range(B, lay, C.raster, None, 0, C.tile, rng, C.blobs)
    assert PX.delta(c0, B.raster_counters()) == [n_range, 0, 0, 0]
    check_range(B, lay, C.raster, None, 0, C.tile, rng, C.blobs, slot_bytes=slot)
    assert B.encode_range(lay, C.raster, None, 0, C.tile, rng, slot_bytes=slot, arena_cap=n_range * slot - 1)[0] == 3
    assert B.encode_range(lay, C.raster, None, 0, C.tile, rng, slot_bytes=slot, arena_cap=n_range * slot)[0] == 0
    if n_range == 9:
        old = B.encode_at(lay, C.raster, None, 0, C.tile, slot_bytes=slot)
        new = B.encode_range(lay, C.raster, None, 0, C.tile, rng, slot_bytes=slot)
        assert old[0] == new[0] == 0 and [new[1][t] for t in range(9)] == old[1]
        assert np.array_equal(new[2], old[2]) and np.array_equal(new[3], old[3]) and new[4] == old[4]
        old = B.encode_at(lay, C.raster, None, 0, C.tile)
        new = B.encode_range(lay, C.raster, None, 0, C.tile, rng)
        assert old[0] == new[0] == 0 and [new[1][t] for t in range(9)] == old[1] and np.array_equal(new[3], old[3]) and new[4] == old[4]


def check_range_kinds(B, R):
    """with a mask, with three bands, from a pixel-interleaved source: the 2 x 2 block and the right column"""
    for dtype, e, nb, with_mask, pp in ((np.float32, 0.01, 1, True, 1), (np.uint8, 0, 3, True, 1), (np.uint8, 0, 3, False, 4), (np.float32, 0.01, 3, True, 3)):
        C = content(R, dtype, e, nb, with_mask, ALL_CLASSES)
        n_rows, n_cols = C.raster.shape[1:]
        lay = PX.StridedLayout.planes(nb, n_rows, n_cols, dtype) if pp == 1 else PX.StridedLayout.pixels(nb, n_rows, n_cols, dtype, pp)
        for rng in ((1, 1, 2, 2), (0, 2, 3, 1)):
            check_range(B, lay, C.raster, C.mask, e, C.tile, rng, C.blobs)
        check_range(B, lay, C.raster, C.mask, e, C.tile, (1, 1, 2, 2), C.blobs, slot_bytes=RT.slot_for(C.raster, C.tile))


def check_range_in_place(B, R):
    """tiles as wide as the raster and no padding, tile rows 1 .. 2: coded where they lie (out[1]); with padding through the staging buffer"""
    shape_tile = ((83, 56), (32, 56))
    C = content(R, np.uint16, 0, 1, False, shape_tile)
    for pad, moved in ((0, [0, 2, 0, 0]), (5, [2, 0, 0, 0])):
        lay = PX.StridedLayout.planes(1, 83, 56, np.uint16, pad=pad)
        c0 = B.raster_counters()
        blobs = check_range(B, lay, C.raster, None, 0, C.tile, (1, 0, 2, 1), C.blobs)
        assert PX.delta(c0, B.raster_counters()) == moved, (pad, c0, B.raster_counters())
        assert [blobs[1], blobs[2]] == C.blobs[1:]


def check_range_arguments(B, R):
    C = content(R, np.uint16, 0, 1, False, ALL_CLASSES)
    lay = PX.StridedLayout.planes(1, 83, 101, np.uint16)

    def call(rng):
        return B.encode_range(lay, C.raster, None, 0, C.tile, (0, 0, 3, 3), **{"range": rng})[0]
    assert call((0, 0, 3, 3)) == 0 and call((2, 2, 1, 1)) == 0
    for bad in ((0, 0, 0, 3), (0, 0, 3, 0), (0, 0, -1, 3), (-1, 0, 1, 1), (0, -1, 1, 1), (3, 0, 1, 1), (0, 3, 1, 1), (1, 0, 3, 1), (0, 1, 1, 3),
                (0, 0, 4, 3), (0, 0, 3, 4)):
        assert call(bad) == 2, bad


def check_round_trip(B, R):
    """a range encode, then a window decode of the range's rectangle from a table that holds the range only: the pixels back (lossless),
    or the reference's decode"""
    rng, window = (1, 1, 2, 2), (32, 40, 51, 61)
    for dtype, e, nb, with_mask, how in ((np.uint16, 0, 1, False, PLANES), (np.uint8, 0, 3, True, ("pixels", 3)), (np.float32, 0.01, 1, True, PLANES)):
        C = content(R, dtype, e, nb, with_mask, ALL_CLASSES)
        n_rows, n_cols = C.raster.shape[1:]
        lay = PX.StridedLayout.planes(nb, n_rows, n_cols, dtype) if how == PLANES else PX.StridedLayout.pixels(nb, n_rows, n_cols, dtype, how[1])
        rc, blobs, offs, sizes, used, (ka, pa) = B.encode_range(lay, C.raster, C.mask, e, C.tile, rng)
        assert rc == 0
        outside = np.ones(len(offs), bool)
        outside[range_tiles(n_rows, n_cols, C.tile, rng)] = False
        offs[outside], sizes[outside] = DEAD64, DEAD32
        rc, pix, valid = B.decode_window(None, C.raster.shape, dtype, C.tile, window, how, with_mask, table=(pa, offs, sizes))
        assert rc == 0, (rc, B.note())
        rows, cols = slice(32, 83), slice(40, 101)
        m = C.ref_valid[rows, cols] > 0
        if with_mask:
            assert np.array_equal(valid, C.ref_valid[rows, cols])
        for k in range(nb):
            assert same_bits(pix[k][m], C.ref_pix[k, rows, cols][m])
            if e == 0:
                assert np.array_equal(pix[k][m], C.raster[k, rows, cols][m])


def check_shard_rows():
    """the ranks' runs of tile rows partition the grid, for grids with fewer tile rows than ranks too"""
    from lerc_amd import shard
    for world in (1, 2, 3, 8):
        for n_rows, tile_rows in ((83, 32), (33, 16), (256, 256), (1030, 256), (5, 1), (4097, 64)):
            n_ty = -(-n_rows // tile_rows)
            runs = [shard.raster_tile_rows(r, world, n_rows, tile_rows) for r in range(world)]
            assert runs == [shard.tile_range(r, world, n_ty) for r in range(world)]
            at = 0
            for first, count in runs:
                assert first == at and count >= 0
                at += count
            assert at == n_ty and max(c for _, c in runs) - min(c for _, c in runs) <= 1
