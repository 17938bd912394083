"""Shared by test_sim_raster_depth_layouts.py (CPU emulator library) and test_gpu_raster_depth_layouts.py (MI355X): a driver for the
four depth raster calls that take a layout (include/lerc_amd_depth.h: lerc_amd_encode_raster_tiles_device_depth_strided,
lerc_amd_decode_raster_tiles_device_depth_strided, lerc_amd_encode_raster_tiles_device_depth_range,
lerc_amd_decode_raster_window_device_depth), and the checks.  The checker's word, as in raster_depth_common.py: every blob equals
lerc_encode(np.ascontiguousarray(rect), nDepth = C) of that rectangle, and the way back writes what lerc_decode makes of it.

A raster is [H, W, C] here whatever its layout; a DepthLayout says where element (row, col, d) lies in a buffer that holds the
sentinel byte everywhere else -- in front of the raster, behind it, in the padding of its rows, lines and planes and in the gaps
between gapped pixels (the alpha channel) --, and every decode asserts that all of that still holds it."""
import ctypes as ct

import numpy as np

import capi
import raster_depth_common as RC

D = RC.D
SENT = RC.SENT
GUARD = 16                                # elements in front of and behind every buffer
SHAPE, TILE = (37, 45), (16, 16)          # four shape classes, ragged last tiles: a grid of 3 x 3
KEPT64, KEPT32 = 0xEEEEEEEEEEEEEEEE, 0xEEEEEEEE      # table entries the range encode must not write
DEAD64, DEAD32 = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF      # table entries of tiles the window decode must not read

# (dtype, maxZErr, nDepth): element sizes 1, 2, 4, 8 at nDepth 3, and nDepth 2 and 8 for one type
TYPES = [(np.uint8, 0, 3), (np.uint16, 0, 3), (np.float32, 0.01, 3), (np.float64, 0.001, 3), (np.uint16, 0, 2), (np.uint16, 0, 8)]
# (with a mask, slotted)
MODES = [(False, False), (True, False), (True, True)]
# (row0, col0, rows, cols) on SHAPE at TILE, and the tiles each touches
WINDOWS = [((18, 19, 9, 10), 1), ((10, 12, 14, 13), 4), ((20, 30, 1, 1), 1), ((28, 28, 9, 17), 4), ((0, 0, 37, 45), 9)]
# (tileRow0, tileCol0, nTileRows, nTileCols): one tile, a row of tiles, the bottom-right 2 x 2
RANGES = [(1, 1, 1, 1), (2, 0, 1, 3), (1, 1, 2, 2)]


def layouts_for(c):
    """the layouts a raster of nDepth c is checked in: packed; gapped by one element; gapped beyond kRtPxMaxPitch = 8 (the plain form);
    planes; planes as a view; lines"""
    return ["packed", "gapped%d" % (c + 1)] + (["gapped9"] if c + 1 < 9 else []) + ["planes", "planes_view", "lines"]


# (dtype, maxZErr, nDepth, layout, with a mask, slotted).  The 8-bit tiles go one by one in the tile layer, which the emulator takes
# seconds for: they leave out the middle mode
PARITY = [(dtype, e, c, lay, m, s) for dtype, e, c in TYPES for lay in layouts_for(c) for m, s in MODES if np.dtype(dtype).itemsize > 1 or m == s]
PARITY_IDS = ["%s-x%d-%s%s%s" % (np.dtype(p[0]).name, p[2], p[3], "-mask" if p[4] else "", "-slots" if p[5] else "") for p in PARITY]


def bind(L):
    RC.bind(L)
    vp, u64, u32, i = ct.c_void_p, ct.c_ulonglong, ct.c_uint, ct.c_int
    L.lerc_amd_encode_raster_tiles_device_depth_strided.restype = u32
    L.lerc_amd_encode_raster_tiles_device_depth_strided.argtypes = [vp, vp, u32, i, i, i, u64, u64, u64, i, i, i, vp, u64, ct.c_double, vp, u64, u64, vp, vp, vp]
    L.lerc_amd_decode_raster_tiles_device_depth_strided.restype = u32
    L.lerc_amd_decode_raster_tiles_device_depth_strided.argtypes = [vp, vp, vp, vp, u32, i, i, i, u64, u64, u64, i, i, vp, i, vp, u64]
    L.lerc_amd_encode_raster_tiles_device_depth_range.restype = u32
    L.lerc_amd_encode_raster_tiles_device_depth_range.argtypes = [vp, vp, u32, i, i, i, u64, u64, u64, i, i, i, i, i, i, i, vp, u64, ct.c_double, vp, u64, u64,
                                                                  vp, vp, vp]
    L.lerc_amd_decode_raster_window_device_depth.restype = u32
    L.lerc_amd_decode_raster_window_device_depth.argtypes = [vp, vp, vp, vp, u32, i, i, i, i, i, i, i, i, i, vp, u64, u64, u64, i, vp, u64]
    L.lerc_amd_raster_tiles_counters.restype = None
    L.lerc_amd_raster_tiles_counters.argtypes = [vp, ct.POINTER(u64)]
    return L


class DepthLayout:
    """where an [h, w, c] raster lies in a buffer of `total` elements: element (i, j, d) at start + i * row_pitch + j * pixel_pitch +
    d * depth_pitch"""

    def __init__(self, name, h, w, c, dtype):
        self.name, self.h, self.w, self.c, self.dtype = name, h, w, c, np.dtype(dtype)
        if name == "packed":            # a view big[:, 5:5 + w] of an [h, w + 8, c] tensor
            self.pixel_pitch, self.depth_pitch, self.row_pitch, self.start = c, 1, (w + 8) * c, GUARD + 5 * c
        elif name.startswith("gapped"):  # c channels out of pp: rgba[..., :3]
            pp = int(name[6:])
            self.pixel_pitch, self.depth_pitch, self.row_pitch, self.start = pp, 1, w * pp + 5, GUARD + 1
        elif name == "planes":          # [c, h, w], contiguous
            self.pixel_pitch, self.depth_pitch, self.row_pitch, self.start = 1, h * w, w, GUARD
        elif name == "planes_view":     # chw[:, a:b, c:d]: rows longer than w, and 5 elements into the buffer: 8-bit rows begin off a 16-byte boundary
            self.pixel_pitch, self.depth_pitch, self.row_pitch, self.start = 1, (h + 2) * (w + 7), w + 7, GUARD + 5
        elif name == "lines":           # GDAL's INTERLEAVE=LINE: the c lines of a row one behind the other
            self.pixel_pitch, self.depth_pitch, self.row_pitch, self.start = 1, w + 3, c * (w + 3) + 2, GUARD + 1
        else:
            raise ValueError(name)
        i, j, d = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
        self.index = self.start + i * self.row_pitch + j * self.pixel_pitch + d * self.depth_pitch
        self.total = int(self.index.max()) + 1 + GUARD
        assert len(np.unique(self.index)) == h * w * c

    def fill(self, raster=None):
        """the buffer's bytes: the sentinel everywhere, the raster's elements where they lie"""
        buf = np.full(self.total * self.dtype.itemsize, SENT, np.uint8).view(self.dtype)
        if raster is not None:
            buf[self.index.ravel()] = np.ascontiguousarray(raster, self.dtype).ravel()
        return buf.view(np.uint8)

    def address(self, base):
        return base + self.start * self.dtype.itemsize

    def take(self, raw):
        """-> ([h, w, c], whether every byte that is no element of the raster still holds the sentinel)"""
        buf = np.array(raw[:self.total * self.dtype.itemsize], copy=True).view(self.dtype)
        pix = buf[self.index.ravel()].reshape(self.h, self.w, self.c)
        rest = np.ones(self.total, bool)
        rest[self.index.ravel()] = False
        clean = bool((buf[rest].view(np.uint8) == SENT).all())
        return pix, clean


class MaskPlane:
    """a byte plane [h][w + 7], GUARD bytes into its buffer"""

    def __init__(self, h, w):
        self.h, self.w, self.pitch = h, w, w + 7

    def fill(self, mask=None):
        buf = np.full(2 * GUARD + self.h * self.pitch, SENT, np.uint8)
        if mask is not None:
            buf[GUARD:GUARD + self.h * self.pitch].reshape(self.h, self.pitch)[:, :self.w] = mask
        return buf

    def take(self, raw):
        body = raw[GUARD:GUARD + self.h * self.pitch].reshape(self.h, self.pitch)
        clean = bool((raw[:GUARD] == SENT).all() and (raw[GUARD + self.h * self.pitch:2 * GUARD + self.h * self.pitch] == SENT).all() and (body[:, self.w:] == SENT).all())
        return np.array(body[:, :self.w], copy=True), clean


def grid(h, w, tile):
    return [(y, min(h, y + tile[0]), x, min(w, x + tile[1])) for y in range(0, h, tile[0]) for x in range(0, w, tile[1])]


def window_tiles(h, w, tile, window):
    """lerc_amd.api.raster_window_tiles: the tiles a window touches, in tile order"""
    from lerc_amd import api
    return api.raster_window_tiles(h, w, tile, window)


def range_tiles(h, w, tile, rng):
    ty0, tx0, nty, ntx = rng
    n_tx = -(-w // tile[1])
    return [ty * n_tx + tx for ty in range(ty0, ty0 + nty) for tx in range(tx0, tx0 + ntx)]


def slot_for(tile, c, dtype):
    return (tile[0] * tile[1] * c * np.dtype(dtype).itemsize + tile[0] * tile[1] + 2048 + 15) & ~15


def lay_arena(blobs):
    """blobs (None: dead table entries for that tile) at 16-byte aligned offsets -> (arena bytes, offsets, sizes)"""
    n = len(blobs)
    offs, sizes = np.full(n, DEAD64, np.uint64), np.full(n, DEAD32, np.uint32)
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


def delta(before, after):
    return [b - a for a, b in zip(before, after)]


class DepthLayouts(RC.RasterDepth):
    """one context of library L: the four calls with a layout beside RasterDepth's packed two"""

    def __init__(self, L, mem):
        bind(L)
        RC.RasterDepth.__init__(self, L, mem)

    def raster_counters(self):
        out = (ct.c_ulonglong * 4)()
        self.L.lerc_amd_raster_tiles_counters(self.h, out)
        return [int(v) for v in out]

    def encode(self, lay, raster, mask, tile, e, slot_bytes=0, rng=None, packed_call=False):
        """raster [h, w, c] laid out as `lay` says; rng: the range call for (tileRow0, tileCol0, nTileRows, nTileCols); packed_call: the
        call without a depthPitch (lay packed) -> (status, {tile: blob}, offsets, sizes, arena bytes used); the tables are full-grid
        and held KEPT64 / KEPT32 before the call"""
        h, w, c = raster.shape
        src = lay.fill(raster)
        kr, pr = self.mem.up(src)
        ml = MaskPlane(h, w) if mask is not None else None
        msrc = ml.fill(mask) if ml else None
        km, pm = self.mem.up(msrc) if ml else (None, None)
        n = len(grid(h, w, tile))
        members = list(range(n)) if rng is None else range_tiles(h, w, tile, rng)
        cap = len(members) * (slot_bytes if slot_bytes else slot_for(tile, c, raster.dtype))
        ka, pa = self.mem.empty(cap + 16)
        offs, sizes = np.full(n, KEPT64, np.uint64), np.full(n, KEPT32, np.uint32)
        used = ct.c_ulonglong(0)
        head = (self.h, lay.address(pr), capi.dt_code(raster.dtype), w, h, c, lay.pixel_pitch, lay.row_pitch)
        tail = (1 if ml else 0, pm + GUARD if ml else None, ml.pitch if ml else 0, float(e), pa, cap, int(slot_bytes), offs.ctypes.data, sizes.ctypes.data, ct.byref(used))
        if packed_call:
            assert rng is None and lay.depth_pitch == 1 and lay.pixel_pitch == c
            rc = self.L.lerc_amd_encode_raster_tiles_device_depth(*head, tile[1], tile[0], *tail)
        elif rng is None:
            rc = self.L.lerc_amd_encode_raster_tiles_device_depth_strided(*head, lay.depth_pitch, tile[1], tile[0], *tail)
        else:
            rc = self.L.lerc_amd_encode_raster_tiles_device_depth_range(*head, lay.depth_pitch, tile[1], tile[0], rng[1], rng[0], rng[3], rng[2], *tail)
        assert np.array_equal(self.mem.down(kr)[:len(src)], src), "the encode changed its source"
        if ml:
            assert np.array_equal(self.mem.down(km)[:len(msrc)], msrc), "the encode changed its mask"
        arena = self.mem.down(ka)
        assert arena[cap:cap + 16].tolist() == [0xCD] * 16, "bytes behind the arena were written"
        blobs = {}
        if rc == 0:
            outside = np.ones(n, bool)
            outside[members] = False
            assert (offs[outside] == KEPT64).all() and (sizes[outside] == KEPT32).all(), "table entries outside the range were written"
            blobs = {t: arena[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() for t in members}
        return rc, blobs, offs, sizes, int(used.value)

    def decode(self, layname, blobs, shape, dtype, tile, with_mask, window=None):
        """blobs in tile order (None: that tile's table entries are dead) into a buffer of the raster's size (window None) or of the
        window's, (row0, col0, rows, cols) -> (status, pixels [h, w, c] of the buffer, valid [h, w] or None); asserts the sentinels"""
        n_rows, n_cols, c = shape
        h, w = (n_rows, n_cols) if window is None else (window[2], window[3])
        lay = DepthLayout(layname, h, w, c, dtype)
        arena, offs, sizes = lay_arena(blobs)
        ka, pa = self.mem.up(arena)
        kr, pr = self.mem.up(lay.fill())
        ml = MaskPlane(h, w) if with_mask else None
        km, pm = self.mem.up(ml.fill()) if ml else (None, None)
        mask_args = (1 if ml else 0, pm + GUARD if ml else None, ml.pitch if ml else 0)
        if window is None:
            rc = self.L.lerc_amd_decode_raster_tiles_device_depth_strided(self.h, pa, offs.ctypes.data, sizes.ctypes.data, capi.dt_code(dtype), n_cols, n_rows, c,
                                                                          lay.pixel_pitch, lay.row_pitch, lay.depth_pitch, tile[1], tile[0], lay.address(pr), *mask_args)
        else:
            rc = self.L.lerc_amd_decode_raster_window_device_depth(self.h, pa, offs.ctypes.data, sizes.ctypes.data, capi.dt_code(dtype), n_cols, n_rows, c, tile[1],
                                                                   tile[0], window[1], window[0], window[3], window[2], lay.address(pr), lay.pixel_pitch,
                                                                   lay.row_pitch, lay.depth_pitch, *mask_args)
        pix, clean = lay.take(self.mem.down(kr))
        assert clean, "the decode wrote beside the raster's elements (%s)" % layname
        valid = None
        if ml:
            valid, clean = ml.take(self.mem.down(km))
            assert clean, "the decode wrote into the mask's padding"
        return rc, pix, valid


# ---- content: a raster, the reference's blobs of its tiles and what the reference decodes from them; made once a key ------------------
class Content:
    pass


_CONTENT = {}
_WHOLE = {}


def content(R, dtype, e, c, with_mask, shape=SHAPE, tile=TILE):
    dtype = np.dtype(dtype)
    key = (dtype.name, e, c, with_mask, shape, tile)
    if key in _CONTENT:
        return _CONTENT[key]
    h, w = shape
    rng = np.random.default_rng(7 + c)
    C = Content()
    C.key, C.tile, C.with_mask, C.e, C.dtype, C.shape = key, tile, with_mask, e, dtype, (h, w, c)
    if dtype.itemsize == 1:
        C.raster = (D.tiles_of(rng, 1, h, w, c, np.int16)[0] % 251).astype(dtype)
    else:
        C.raster = D.tiles_of(rng, 1, h, w, c, dtype)[0]
    C.mask = None
    if with_mask:
        C.mask = D.random_blob_mask(rng, 1, h, w)[0]
        C.mask[:10, :10] = 0    # (a part of the first tile invalid, whatever the blobs did)
    C.blobs = []
    C.ref_pix = np.zeros((h, w, c), dtype)
    C.ref_valid = np.ones((h, w), np.uint8)
    for y0, y1, x0, x1 in grid(h, w, tile):
        rc, blob = R.encode(np.ascontiguousarray(C.raster[y0:y1, x0:x1]), e, n_depth=c, mask=None if C.mask is None else np.ascontiguousarray(C.mask[y0:y1, x0:x1]))
        assert rc == 0
        C.blobs.append(blob)
        rc, p, m = R.decode(blob, want_masks=1 if with_mask else 0)
        assert rc == 0
        C.ref_pix[y0:y1, x0:x1] = np.asarray(p).reshape(y1 - y0, x1 - x0, c)
        if with_mask:
            C.ref_valid[y0:y1, x0:x1] = np.asarray(m).reshape(y1 - y0, x1 - x0)
    for a in (C.raster, C.ref_pix, C.ref_valid):
        a.setflags(write=False)
    _CONTENT[key] = C
    return C


def whole(B, C):
    """what the whole-raster decode of B's library writes for C's blobs into packed pixels: (pixels, valid or None), once a library"""
    key = (id(B.L), C.key)
    if key not in _WHOLE:
        rc, pix, valid = B.decode("packed", C.blobs, C.shape, C.dtype, C.tile, C.with_mask)
        assert rc == 0, (rc, B.note())
        _WHOLE[key] = (pix, valid)
    return _WHOLE[key]


def same_bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- parity both ways ---------------------------------------------------------------------------------------------------------------
def check_parity(B, R, dtype, e, c, layname, with_mask, slotted, shape=SHAPE, tile=TILE):
    C = content(R, dtype, e, c, with_mask, shape, tile)
    h, w, _ = C.shape
    n = len(C.blobs)
    lay = DepthLayout(layname, h, w, c, dtype)
    slot = slot_for(tile, c, dtype) if slotted else 0
    c0 = B.counters()
    rc, blobs, offs, sizes, used = B.encode(lay, C.raster, C.mask, tile, e, slot_bytes=slot)
    c1 = B.counters()
    assert rc == 0, (rc, B.note())
    for t in range(n):
        assert D.same_blob(blobs[t], C.blobs[t], C.dtype.itemsize), "tile %d: %d bytes, the reference makes %d (%s)" % (t, len(blobs[t]), len(C.blobs[t]), B.note())
    if C.dtype.itemsize > 1:    # (8-bit values go one by one in the tile layer, by its rule)
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (n, 0), (c0, c1, B.note())
    if slotted:
        assert sorted(int(o) for o in offs) == [t * slot for t in range(n)] and used == n * slot
    # the packed call on a contiguous copy: the same blobs
    rc, packed, _, _, _ = B.encode(DepthLayout("packed", h, w, c, dtype), np.ascontiguousarray(C.raster), C.mask, tile, e, slot_bytes=slot, packed_call=True)
    assert rc == 0 and [packed[t] for t in range(n)] == [blobs[t] for t in range(n)], "the blobs differ from the packed call's"
    # ---- the way back
    rc, pix, valid = B.decode(layname, C.blobs, C.shape, dtype, tile, with_mask)
    assert rc == 0, (rc, B.note())
    assert same_bits(pix, C.ref_pix), "pixels differ from the reference's"
    if with_mask:
        assert np.array_equal(valid, C.ref_valid), "valid bytes differ from the reference's"


# ---- windows ------------------------------------------------------------------------------------------------------------------------
WINDOW_CONTENT = [(np.uint16, 0, 3, True), (np.uint8, 0, 3, False)]


def check_window(B, R, window, n_tiles, layname):
    h, w = SHAPE
    for dtype, e, c, with_mask in WINDOW_CONTENT:
        C = content(R, dtype, e, c, with_mask)
        whole_pix, whole_valid = whole(B, C)    # (before the counters are read)
        touched = window_tiles(h, w, TILE, window)
        assert len(touched) == n_tiles
        blobs = [b if t in touched else None for t, b in enumerate(C.blobs)]    # (only the window's tiles are read)
        r0 = B.raster_counters()
        rc, pix, valid = B.decode(layname, blobs, C.shape, dtype, TILE, with_mask, window=window)
        assert rc == 0, (rc, B.note())
        assert delta(r0, B.raster_counters()) == [0, 0, n_tiles, 0], (r0, B.raster_counters())
        rows, cols = slice(window[0], window[0] + window[2]), slice(window[1], window[1] + window[3])
        assert same_bits(pix, whole_pix[rows, cols]) and same_bits(pix, C.ref_pix[rows, cols]), "pixels differ from the whole-raster decode's"
        if with_mask:
            assert np.array_equal(valid, whole_valid[rows, cols]) and np.array_equal(valid, C.ref_valid[rows, cols])


def damaged(blob):
    bad = bytearray(blob)
    bad[len(bad) - 9] ^= 0x10    # (a bit flipped under the checksum)
    return bytes(bad)


def check_damaged_blob(B, R, layname):
    """tile 4 damaged, the window over tiles 0, 1, 3, 4: its part of the window is zero, mask too, all else is right, and the reference's
    status for that blob comes back"""
    window = (10, 12, 14, 13)
    C = content(R, np.uint16, 0, 3, True)
    h, w, c = C.shape
    bad = damaged(C.blobs[4])
    want_rc = R.decode(bad, want_masks=1)[0]
    assert want_rc != 0
    rc, pix, valid = B.decode(layname, C.blobs[:4] + [bad] + C.blobs[5:], C.shape, C.dtype, TILE, True, window=window)
    assert rc == want_rc, (rc, want_rc, B.note())
    y0, y1, x0, x1 = grid(h, w, TILE)[4]
    part = (slice(max(y0, window[0]) - window[0], min(y1, window[0] + window[2]) - window[0]),
            slice(max(x0, window[1]) - window[1], min(x1, window[1] + window[3]) - window[1]))
    assert pix[part].size and not pix[part].any() and not valid[part].any(), "the failing tile's part is not zeroed"
    others = np.ones((window[2], window[3]), bool)
    others[part] = False
    rows, cols = slice(window[0], window[0] + window[2]), slice(window[1], window[1] + window[3])
    assert same_bits(pix[others], C.ref_pix[rows, cols][others]) and np.array_equal(valid[others], C.ref_valid[rows, cols][others])


# ---- ranges -------------------------------------------------------------------------------------------------------------------------
def check_range(B, R, rng, layname):
    h, w = SHAPE
    for dtype, e, c, with_mask in ((np.uint16, 0, 3, True), (np.float32, 0.01, 3, False)):
        C = content(R, dtype, e, c, with_mask)
        lay = DepthLayout(layname, h, w, c, dtype)
        members = range_tiles(h, w, TILE, rng)
        rc, everything, _, _, _ = B.encode(lay, C.raster, C.mask, TILE, e)
        assert rc == 0
        for slot in (0, slot_for(TILE, c, dtype)):
            r0 = B.raster_counters()
            rc, blobs, offs, sizes, used = B.encode(lay, C.raster, C.mask, TILE, e, slot_bytes=slot, rng=rng)    # (asserts the entries outside the range)
            assert rc == 0, (rc, B.note())
            assert delta(r0, B.raster_counters()) == [len(members), 0, 0, 0]
            for t in members:
                assert blobs[t] == everything[t] and D.same_blob(blobs[t], C.blobs[t], C.dtype.itemsize), "tile %d" % t
            if slot:
                assert sorted(int(offs[t]) for t in members) == [k * slot for k in range(len(members))] and used == len(members) * slot


# ---- the boundary: status rows of the four calls.  A good call: a 16 x 16 x 3 uint16 raster, packed, tiles of 8 x 8, no mask; the window
# call: the whole raster as its window; the range call: the whole grid.  (row name, what differs from the good call, status, the calls
# the row is asked of -- e: the strided encode, d: the strided decode, r: the range encode, w: the window decode)
OK = dict(ctx=1, raster=1, arena=1, offs=1, sizes=1, dt=3, w=16, h=16, d=3, pp=3, rp=48, dp=1, tc=8, tr=8, nm=0, mask=0, mp=0, e=0.0, slot=0,
          win=(0, 0, 16, 16), rng=(0, 0, 2, 2))
ALL, ENC = "edrw", "er"
TABLE = [
    ("the good call", dict(), 0, ENC),
    ("no context", dict(ctx=0), 2, ALL), ("no raster", dict(raster=0), 2, ALL), ("no arena", dict(arena=0), 2, ALL), ("no offsets", dict(offs=0), 2, ALL),
    ("no sizes", dict(sizes=0), 2, ALL), ("a mask counted but not given", dict(nm=1, mp=16), 2, ALL), ("a mask given but not counted", dict(mask=1, mp=16), 2, ALL),
    ("nCols 0", dict(w=0), 2, ALL), ("nCols -1", dict(w=-1), 2, ALL), ("nRows 0", dict(h=0), 2, ALL), ("nRows -5", dict(h=-5), 2, ALL),
    ("tileCols 0", dict(tc=0), 2, ALL), ("tileRows -1", dict(tr=-1), 2, ALL), ("nDepth 0", dict(d=0, pp=0), 2, ALL), ("nDepth -1", dict(d=-1), 2, ALL),
    ("a type that is none", dict(dt=8), 2, ALL),
    ("nDepth 1 does not look at depthPitch", dict(d=1, pp=1, rp=16, dp=777), 0, ENC),
    ("both pitches above 1", dict(pp=3, dp=2), 2, ALL), ("both pitches above 1, far apart", dict(pp=4, rp=64, dp=4096), 2, ALL),
    ("pixelPitch below nDepth", dict(pp=2), 2, ALL), ("pixelPitch 0", dict(pp=0), 2, ALL), ("depthPitch 0", dict(dp=0), 2, ALL),
    ("packed: rows that just fit", dict(rp=48), 0, ENC), ("packed: rows that overlap", dict(rp=47), 2, ALL),
    ("gapped: rows that just fit", dict(pp=4, rp=63), 0, ENC), ("gapped: rows that overlap", dict(pp=4, rp=62), 2, ALL),
    ("planes that just fit", dict(pp=1, rp=16, dp=256), 0, ENC), ("planes that overlap", dict(pp=1, rp=16, dp=255), 2, ALL),
    ("planes: rows that overlap", dict(pp=1, rp=15, dp=256), 2, ALL),
    ("planes of padded rows that just fit", dict(pp=1, rp=20, dp=316), 0, ENC), ("planes of padded rows that overlap", dict(pp=1, rp=20, dp=315), 2, ALL),
    ("lines that just fit", dict(pp=1, rp=48, dp=16), 0, ENC), ("lines: rows that overlap", dict(pp=1, rp=47, dp=16), 2, ALL),
    ("lines that overlap", dict(pp=1, rp=48, dp=15), 2, ALL), ("padded lines that just fit", dict(pp=1, rp=56, dp=20), 0, ENC),
    ("padded lines: rows that overlap", dict(pp=1, rp=55, dp=20), 2, ALL),
    ("a mask pitch below nCols", dict(nm=1, mask=1, mp=15), 2, ALL),
    ("maxZErr < 0", dict(e=-1.0), 2, ENC), ("slotBytes 24", dict(slot=24), 2, ENC),
    ("a window beyond the last column", dict(win=(0, 1, 16, 16)), 2, "w"), ("a window beyond the last row", dict(win=(9, 0, 8, 16)), 2, "w"),
    ("a window of no rows", dict(win=(0, 0, 0, 16)), 2, "w"), ("a window of -1 columns", dict(win=(0, 0, 16, -1)), 2, "w"),
    ("a window in front of the raster", dict(win=(-1, 0, 16, 16)), 2, "w"),
    ("a window whose rows overlap in its buffer", dict(win=(4, 4, 8, 8), rp=23), 2, "w"),
    ("a window whose planes overlap in its buffer", dict(win=(4, 4, 8, 8), pp=1, rp=8, dp=63), 2, "w"),
    ("a range beyond the last tile row", dict(rng=(0, 0, 3, 2)), 2, "r"), ("a range that begins behind the grid", dict(rng=(0, 2, 1, 1)), 2, "r"),
    ("a range of no tiles", dict(rng=(0, 0, 0, 2)), 2, "r"), ("a range in front of the grid", dict(rng=(-1, 0, 1, 1)), 2, "r"),
    ("a tile beyond INT_MAX", dict(w=65536, h=65536, rp=65536 * 3, tc=65536, tr=65536), 6, ALL),
    ("a tile beyond INT_MAX by its depth", dict(w=32768, h=32768, d=4, pp=4, rp=32768 * 4, tc=32768, tr=32768), 6, ALL),
    ("nDepth 0 beside a tile beyond INT_MAX", dict(w=65536, h=65536, d=0, pp=0, rp=65536 * 3, tc=65536, tr=65536), 2, ALL),
]


def check_refused(B):
    kr, pr = B.mem.up(np.zeros(16 * 16 * 32, np.uint16))
    ka, pa = B.mem.empty(1 << 16)
    km, pm = B.mem.up(np.ones((16, 16), np.uint8))
    offs = np.zeros(16, np.uint64)
    sizes = np.zeros(16, np.uint32)
    for name, change, status, calls in TABLE:
        a = dict(OK, **change)
        h = B.h if a["ctx"] else None
        ras, arena, mask = (pr if a["raster"] else None), (pa if a["arena"] else None), (pm if a["mask"] else None)
        po, ps = (offs.ctypes.data if a["offs"] else None), (sizes.ctypes.data if a["sizes"] else None)
        win, rng = a["win"], a["rng"]
        enc_tail = (a["nm"], mask, a["mp"], a["e"], arena, 1 << 16, a["slot"], po, ps, None)
        if "e" in calls:
            rc = B.L.lerc_amd_encode_raster_tiles_device_depth_strided(h, ras, a["dt"], a["w"], a["h"], a["d"], a["pp"], a["rp"], a["dp"], a["tc"], a["tr"], *enc_tail)
            assert rc == status, (name, "encode", rc, status)
        if "r" in calls:
            rc = B.L.lerc_amd_encode_raster_tiles_device_depth_range(h, ras, a["dt"], a["w"], a["h"], a["d"], a["pp"], a["rp"], a["dp"], a["tc"], a["tr"],
                                                                     rng[1], rng[0], rng[3], rng[2], *enc_tail)
            assert rc == status, (name, "range", rc, status)
        if "d" in calls:
            rc = B.L.lerc_amd_decode_raster_tiles_device_depth_strided(h, arena, po, ps, a["dt"], a["w"], a["h"], a["d"], a["pp"], a["rp"], a["dp"], a["tc"], a["tr"],
                                                                       ras, a["nm"], mask, a["mp"])
            assert rc == status, (name, "decode", rc, status)
        if "w" in calls:
            rc = B.L.lerc_amd_decode_raster_window_device_depth(h, arena, po, ps, a["dt"], a["w"], a["h"], a["d"], a["tc"], a["tr"], win[1], win[0], win[3], win[2],
                                                                ras, a["pp"], a["rp"], a["dp"], a["nm"], mask, a["mp"])
            assert rc == status, (name, "window", rc, status)


# ---- the header: every LERC_AMD_API symbol of include/lerc_amd_depth.h is exported -----------------------------------------------------
def check_header(L):
    import os
    import re
    text = open(os.path.join(capi.ROOT, "include", "lerc_amd_depth.h")).read()
    names = re.findall(r"LERC_AMD_API\s+\w+\s+(\w+)\s*\(", text)
    assert len(names) >= 8 and len(set(names)) == len(names), names
    for fn in ("lerc_amd_encode_raster_tiles_device_depth_strided", "lerc_amd_decode_raster_tiles_device_depth_strided",
               "lerc_amd_encode_raster_tiles_device_depth_range", "lerc_amd_decode_raster_window_device_depth"):
        assert fn in names, fn
    for fn in names:
        assert hasattr(L, fn), "%s is declared in lerc_amd_depth.h and not exported" % fn
