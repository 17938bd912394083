"""Shared by test_sim_raster_nodata.py (CPU emulator library) and test_gpu_raster_nodata.py (MI355X): a driver for the noData raster
calls of include/lerc_amd_nodata.h (lerc_amd_encode_raster_tiles_device_nodata / lerc_amd_decode_raster_window_device_nodata), rasters
with holes to feed them, and the checks.

The checker's word is always this: a pixel is invalid when it equals the noData value by the type's own == (a NaN where noData is
NaN); tile t's blob equals R.encode(rectangle, e, mask=derived) and the decoded window equals np.where(mask, R.decode(blob), no_data),
NaN compared by isnan.  The base raster is raster_tiles_common.ALL_CLASSES: 83 x 101 at tiles of 32 x 40 -- four shape classes, a
grid of 3 x 3, rows that are no multiple of 16 bytes for any type.  Surfaces follow tiles_depth_common.surface, holes are blob-shaped
(random_blob_mask) and hold the noData value.

Addressing: a raster (a window's buffer) is an NdLayout -- raster_px_common.StridedLayout with one band and guard bytes of 0xCD --:
GUARD + lead elements into its allocation, rows 5 elements longer than they need to be, pixel_pitch - 1 elements between pixels.
Guards, padding and gaps must hold 0xCD after a decode, and an encode must leave its source as it was.  The window's valid bytes have a
pitch of their own, winCols + 3.
"""
import ctypes as ct
import math

import numpy as np

import capi
import raster_px_common as PX
import raster_tiles_common as RT
import raster_window_common as RW
import tiles_depth_common as TD
from tiles_masked_common import GpuMem, HostMem, random_blob_mask    # noqa: F401

T = RT.T
ALL_CLASSES = RT.ALL_CLASSES
GUARD_BYTE = 0xCD
WINDOWS, RANGES = RW.WINDOWS, RW.RANGES
DEAD64, DEAD32, KEPT64, KEPT32 = RW.DEAD64, RW.DEAD32, RW.KEPT64, RW.KEPT32
NAN = float("nan")

TYPES = [(np.int8, 0), (np.uint8, 0), (np.int16, 0), (np.uint16, 0), (np.int32, 0), (np.uint32, 0), (np.float32, 0.01), (np.float64, 0.001)]


def bind(L):
    RW.bind(L)
    vp, u64, u32, i, dbl = ct.c_void_p, ct.c_ulonglong, ct.c_uint, ct.c_int, ct.c_double
    L.lerc_amd_encode_raster_tiles_device_nodata.restype = u32
    L.lerc_amd_encode_raster_tiles_device_nodata.argtypes = [vp, vp, u32, i, i, u64, u64, i, i, i, i, i, i, dbl, dbl, vp, u64, u64, vp, vp, vp]
    L.lerc_amd_decode_raster_window_device_nodata.restype = u32
    L.lerc_amd_decode_raster_window_device_nodata.argtypes = [vp, vp, vp, vp, u32, i, i, i, i, i, i, i, i, vp, u64, u64, dbl, vp, u64]
    return L


class NdLayout(PX.StridedLayout):
    """one band [R, C]: element (i, j) at start + i * pitch + j * pixel_pitch; everything else holds 0xCD"""

    def __init__(self, n_rows, n_cols, dtype, pixel_pitch=1, pad=5, lead=1, first=0):
        PX.StridedLayout.__init__(self, 1, n_rows, n_cols, dtype, pixel_pitch, (n_cols - 1) * pixel_pitch + 1 + pad, 1, lead + first)

    def fill(self, a=None):
        buf = np.full(self.n_elems * self.dtype.itemsize, GUARD_BYTE, np.uint8).view(self.dtype)
        if a is not None:
            buf[self.index()] = np.asarray(a, self.dtype).reshape(1, self.n_rows, self.n_cols)
        return buf.view(np.uint8)

    def take(self, raw):
        """-> (the raster [R, C], whether everything around its elements still holds 0xCD)"""
        buf = np.asarray(raw, np.uint8)[:self.n_elems * self.dtype.itemsize].view(self.dtype)
        inside = np.zeros(self.n_elems, bool)
        inside[self.index()] = True
        return buf[self.index()][0].copy(), bool((buf[~inside].view(np.uint8) == GUARD_BYTE).all())


class NoDataBatch(RW.WindowBatch):
    """one context of library L: the noData calls beside WindowBatch's"""

    def __init__(self, L, mem):
        bind(L)
        RW.WindowBatch.__init__(self, L, mem)

    def encode_nd(self, raster, no_data, e, tile, rng=None, slot_bytes=0, arena_cap=None, lay=None, **told):
        """raster [R, C] -> (status, {tile: blob} of the range (None: the whole grid), offsets, sizes, arena bytes used, (arena, address));
        offsets / sizes are full-grid tables that held KEPT64 / KEPT32 before the call.  told: range, pitch, pixel_pitch"""
        n_rows, n_cols = raster.shape
        lay = lay or NdLayout(n_rows, n_cols, raster.dtype)
        src = lay.fill(raster)
        kr, pr = self.mem.up(src)
        n = len(RT.grid(n_rows, n_cols, tile))
        members = list(range(n)) if rng is None else RW.range_tiles(n_rows, n_cols, tile, rng)
        per_tile = min(tile[0], n_rows) * min(tile[1], n_cols)
        cap = int(arena_cap) if arena_cap is not None else len(members) * (slot_bytes if slot_bytes else per_tile * raster.itemsize + per_tile // 4 + 1024 + 16)
        ka, pa = self.mem.empty(cap + 16)
        offs = np.full(n, KEPT64, np.uint64)
        sizes = np.full(n, KEPT32, np.uint32)
        used = ct.c_ulonglong(0)
        ty0, tx0, nty, ntx = told.get("range", (0, 0, -1, -1) if rng is None else rng)
        rc = self.L.lerc_amd_encode_raster_tiles_device_nodata(
            self.h, lay.address(pr), capi.dt_code(raster.dtype), n_cols, n_rows, told.get("pixel_pitch", lay.pixel_pitch), told.get("pitch", lay.pitch),
            tile[1], tile[0], tx0, ty0, ntx, nty, float(no_data), float(e), pa, cap, int(slot_bytes), offs.ctypes.data, sizes.ctypes.data, ct.byref(used))
        assert np.array_equal(self.mem.down(kr)[:len(src)], src), "the encode changed its source"
        arena = self.mem.down(ka)
        assert arena[cap:cap + 16].tolist() == [GUARD_BYTE] * 16, "bytes behind the arena were written"
        blobs = {}
        if rc == 0:
            outside = np.ones(n, bool)
            outside[members] = False
            assert (offs[outside] == KEPT64).all() and (sizes[outside] == KEPT32).all(), "table entries outside the range were written"
            blobs = {t: arena[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() for t in members}
        return rc, blobs, offs, sizes, int(used.value), (ka, pa)

    def decode_nd(self, blobs, shape, dtype, tile, window, no_data, pixel_pitch=1, want_valid=True, table=None, lead=1, mask_pad=3, **told):
        """blobs in tile order (None: that tile's table entries are dead), or table = (arena address, offsets, sizes) -> (status, pixels
        [h, w], valid [h, w] or None); asserts the 0xCD around the window's elements and around its valid bytes.  told: window_arg, pitch,
        mask_pitch"""
        n_rows, n_cols = shape
        r0, c0, h, w = window
        if table is None:
            arena, offs, sizes = RW.lay_arena(blobs)
            ka, pa = self.mem.up(arena)
        else:
            pa, offs, sizes = table
        assert len(offs) == len(sizes) == len(RT.grid(n_rows, n_cols, tile))
        lay = NdLayout(h, w, dtype, pixel_pitch, lead=lead, first=1 if pixel_pitch > 1 else 0)
        kr, pr = self.mem.up(lay.fill())
        mlay = NdLayout(h, w, np.uint8, pad=mask_pad) if want_valid else None
        km, pm = self.mem.up(mlay.fill()) if want_valid else (None, None)
        tr0, tc0, th, tw = told.get("window_arg", window)
        rc = self.L.lerc_amd_decode_raster_window_device_nodata(
            self.h, pa, offs.ctypes.data, sizes.ctypes.data, capi.dt_code(dtype), n_cols, n_rows, tile[1], tile[0], tc0, tr0, tw, th, lay.address(pr),
            lay.pixel_pitch, told.get("pitch", lay.pitch), float(no_data), mlay.address(pm) if want_valid else None,
            told.get("mask_pitch", mlay.pitch if want_valid else 0))
        pix, clean = lay.take(self.mem.down(kr))
        assert clean, "the decode wrote beside the window's elements"
        valid = None
        if want_valid:
            valid, clean = mlay.take(self.mem.down(km))
            assert clean, "the decode wrote outside the window's valid bytes"
        return rc, pix, valid


# ---- content ---------------------------------------------------------------------------------------------------------------------
def surface_of(dtype, n_rows, n_cols, seed=11):
    """a smooth surface in the middle of the type's range; float types get a fractional part"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    s = TD.surface(rng, 1, n_rows, n_cols, amp=30.0 if dtype.itemsize == 1 else 600.0)[0]
    if dtype.kind == "f":
        return (s + rng.normal(0, 0.3, s.shape)).astype(dtype)
    if dtype.itemsize == 1:
        return np.rint(s + (128 if dtype.kind == "u" else 0)).clip(np.iinfo(dtype).min + 1, np.iinfo(dtype).max - 1).astype(dtype)
    if dtype.kind == "u":
        s = s + 3000
    if dtype.itemsize == 4:
        s = s * 37
    return np.rint(s).astype(dtype)


def holes_of(n_rows, n_cols, seed=5):
    """True where a hole is: blob-shaped, 20 .. 60 % of the raster"""
    return RT.mask_of(n_rows, n_cols, seed=seed) == 0


def no_data_for(dtype, kind, surface):
    """the noData values of the issue: inside the data's range (a value the surface takes itself), outside it, 0; NaN and -inf for floats"""
    dtype = np.dtype(dtype)
    if kind == "inside":
        return float(surface[surface.shape[0] // 2, surface.shape[1] // 2])
    if kind == "outside":
        return -9999.0 if dtype.kind == "f" else float(np.iinfo(dtype).max if dtype.kind == "u" else np.iinfo(dtype).min)
    return {"zero": 0.0, "nan": NAN, "-inf": -math.inf}[kind]


def invalid_of(raster, no_data):
    return np.isnan(raster) if math.isnan(no_data) else raster == raster.dtype.type(no_data)


class Content:
    pass


_CONTENT = {}


def judge(R, raster, no_data, e, tile, key=None):
    """the checker's word on a raster: the derived mask, the reference's blobs of the tiles with it, and the raster it decodes from
    them with noData where the mask says 0"""
    if key is not None and key in _CONTENT:
        return _CONTENT[key]
    n_rows, n_cols = raster.shape
    C = Content()
    C.raster, C.no_data, C.e, C.tile = raster, no_data, e, tile
    C.mask = (~invalid_of(raster, no_data)).astype(np.uint8)
    C.blobs = RT.ref_blobs(R, raster[None], C.mask, e, tile)
    C.want = np.zeros(raster.shape, raster.dtype)
    for t, (r0, r1, c0, c1) in enumerate(RT.grid(n_rows, n_cols, tile)):
        rc, p, m = R.decode(C.blobs[t], want_masks=1)
        assert rc == 0 and np.array_equal(m[0], C.mask[r0:r1, c0:c1])
        C.want[r0:r1, c0:c1] = np.where(m[0] > 0, np.asarray(p).reshape(r1 - r0, c1 - c0), raster.dtype.type(no_data))
    for a in (C.raster, C.mask, C.want):
        a.setflags(write=False)
    if key is not None:
        _CONTENT[key] = C
    return C


def content(R, dtype, e, kind, shape_tile=ALL_CLASSES):
    """the surface of that type with holes that hold the noData value of that kind"""
    (n_rows, n_cols), tile = shape_tile
    key = (np.dtype(dtype).name, e, kind, shape_tile)
    if key in _CONTENT:
        return _CONTENT[key]
    raster = surface_of(dtype, n_rows, n_cols)
    no_data = no_data_for(dtype, kind, raster)
    raster[holes_of(n_rows, n_cols)] = no_data
    return judge(R, raster, no_data, e, tile, key)


def same_pixels(a, b):
    """bit for bit, NaN compared by isnan"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and RW.same_bits(a[~na], b[~nb])


# ---- checks ----------------------------------------------------------------------------------------------------------------------
def check_encode(B, C, rng=None, slot_bytes=0, lay=None):
    """-> {tile: blob}: the range's blobs equal the reference's with the derived mask; the tables' layout holds"""
    n_rows, n_cols = C.raster.shape
    c0 = B.raster_counters()
    rc, blobs, offs, sizes, used, _ = B.encode_nd(np.array(C.raster), C.no_data, C.e, C.tile, rng=rng, slot_bytes=slot_bytes, lay=lay)
    assert rc == 0, (rc, B.note())
    members = sorted(blobs)
    assert PX.delta(c0, B.raster_counters()) == [len(members), 0, 0, 0]
    for t in members:
        assert T.same_blob(blobs[t], C.blobs[t], C.raster.itemsize), "tile %d: %d bytes, the reference makes %d (%s)" % (t, len(blobs[t]), len(C.blobs[t]), B.note())
    RT.check_layout(offs[members], sizes[members], used, slot_bytes)
    if slot_bytes:
        assert used == len(members) * slot_bytes
    return blobs


def check_decode(B, C, window=None, blobs=None, **how):
    """-> (pixels, valid): the window of C's mosaic equals the slice of np.where(mask, reference's decode, noData), valid bytes the mask's"""
    n_rows, n_cols = C.raster.shape
    window = window or (0, 0, n_rows, n_cols)
    r0, c0, h, w = window
    k0 = B.raster_counters()
    rc, pix, valid = B.decode_nd(C.blobs if blobs is None else blobs, C.raster.shape, C.raster.dtype, C.tile, window, C.no_data, **how)
    assert rc == 0, (rc, B.note())
    assert PX.delta(k0, B.raster_counters()) == [0, 0, len(RW.window_tiles(n_rows, n_cols, C.tile, window)), 0]
    assert same_pixels(pix, C.want[r0:r0 + h, c0:c0 + w]), "pixels differ from np.where(mask, the reference's decode, noData)"
    if valid is not None:
        assert np.array_equal(valid, C.mask[r0:r0 + h, c0:c0 + w]), "valid bytes differ from the derived mask"
    return pix, valid


def check_both_ways(B, C):
    check_encode(B, C)
    check_decode(B, C)
    if C.e == 0:
        m = C.mask > 0
        assert np.array_equal(C.want[m], C.raster[m])


def check_type_and_value(B, R, dtype, e, kind):
    C = content(R, dtype, e, kind)
    assert 0 < C.mask.sum() < C.mask.size
    check_both_ways(B, C)
    check_decode(B, C, want_valid=False)


def check_negative_zero(B, R):
    """float32 and float64, noData 0.0, some holes hold -0.0, some 0.0: both are invalid, the fill is +0.0"""
    for dtype, e in ((np.float32, 0.01), (np.float64, 0.001)):
        (n_rows, n_cols), tile = ALL_CLASSES
        raster = surface_of(dtype, n_rows, n_cols) + dtype(5000)    # (the surface itself never is zero)
        holes = holes_of(n_rows, n_cols)
        raster[holes] = 0.0
        minus = holes & (np.arange(n_cols)[None, :] % 2 == 1)
        raster[minus] = -0.0
        assert minus.any() and np.signbit(raster[minus]).all() and np.array_equal(invalid_of(raster, 0.0), holes)
        C = judge(R, raster, 0.0, e, tile)
        check_both_ways(B, C)
        pix, _ = check_decode(B, C)
        assert not np.signbit(pix[holes]).any()


def check_no_pixel_matches(B, R):
    """no pixel holds the value: the blobs are the unmasked reference's (a mask that is all valid is not written)"""
    for dtype, e in ((np.uint16, 0), (np.float32, 0.01)):
        (n_rows, n_cols), tile = ALL_CLASSES
        raster = surface_of(dtype, n_rows, n_cols)
        no_data = 65535.0 if dtype == np.uint16 else -9999.0
        assert not invalid_of(raster, no_data).any()
        C = judge(R, raster, no_data, e, tile)
        assert C.blobs == RT.ref_blobs(R, raster[None], None, e, tile)
        check_both_ways(B, C)


def check_one_tile_all_holes(B, R):
    """every pixel of tile 4 matches: its blob is the empty one"""
    for dtype, e, no_data in ((np.int16, 0, -9999.0), (np.float32, 0.01, NAN)):
        (n_rows, n_cols), tile = ALL_CLASSES
        raster = surface_of(dtype, n_rows, n_cols)
        r0, r1, c0, c1 = RT.grid(n_rows, n_cols, tile)[4]
        raster[r0:r1, c0:c1] = no_data
        C = judge(R, raster, no_data, e, tile)
        assert TD.header(C.blobs[4])["num_valid"] == 0
        blobs = check_encode(B, C)
        assert TD.header(blobs[4])["num_valid"] == 0
        check_decode(B, C)


def nan_holed(n_rows, n_cols, tile):
    """noisy float32 content (every tile is one the masked batches keep) with NaN holes, one in every tile at the least"""
    raster = np.array(RT.noisy_float(n_rows, n_cols)[0])
    rng = np.random.default_rng(17)
    for (r0, r1, c0, c1) in RT.grid(n_rows, n_cols, tile):
        hole = random_blob_mask(rng, 1, r1 - r0, c1 - c0, 0.5, 0.9)[0] == 0    # (blobs of the tile's own: 10 .. 50 % of it)
        assert hole.any() and not hole.all()
        raster[r0:r1, c0:c1][hole] = NAN
    return raster


def check_nan_holes_stay_inside(B, R, shape_tile=ALL_CLASSES):
    """float32 with NaN holes in every tile, noData = NaN: every tile through the masked batch's own launches, none one by one, both ways.
    The existing strided call with no mask on the same raster does not keep them all inside: the gain"""
    (n_rows, n_cols), tile = shape_tile
    raster = nan_holed(n_rows, n_cols, tile)
    C = judge(R, raster, NAN, 0.01, tile)
    n = len(C.blobs)
    _, moved = RT.batch_delta(B, 0, lambda: check_encode(B, C))
    assert moved == (n, 0), ("tiles left the batch's launches", moved, B.note())
    _, moved = RT.batch_delta(B, 2, lambda: check_decode(B, C))
    assert moved == (n, 0), ("tiles left the batch's launches", moved, B.note())
    lay = PX.StridedLayout.planes(1, n_rows, n_cols, np.float32)
    _, moved = RT.batch_delta(B, 0, lambda: B.encode_at(lay, raster[None], None, 0.01, tile))
    print("NaN holes, no mask, lerc_amd_encode_raster_tiles_device_strided: %d of %d tiles in the batch's launches, %d one by one" % (moved[0], n, moved[1]))
    assert moved[0] < n, "the unmasked call kept every NaN-holed tile inside: nothing gained"


def check_invalid_values_never_count(B, R):
    """two rasters equal at valid pixels, garbage at different invalid pixels of one mask: raster A holds NaN and is coded with noData =
    NaN; raster B holds a huge value exactly at A's NaN positions and is coded with that value.  Identical blobs tile for tile"""
    (n_rows, n_cols), tile = ALL_CLASSES
    for dtype, e, huge in ((np.float32, 0.01, 3.0e38), (np.float64, 0.001, 1.0e300)):
        a = surface_of(dtype, n_rows, n_cols)
        holes = holes_of(n_rows, n_cols, seed=9)
        b = np.array(a)
        a[holes] = NAN
        huge = float(dtype(huge))
        b[holes] = huge
        CA, CB = judge(R, a, NAN, e, tile), judge(R, b, huge, e, tile)
        assert np.array_equal(CA.mask, CB.mask) and CA.blobs == CB.blobs, "the reference itself lets invalid values count"
        got_a, got_b = check_encode(B, CA), check_encode(B, CB)
        assert got_a == got_b
        check_decode(B, CA)
        check_decode(B, CB)


def check_alignment_sweep(B, R):
    """a view big[a:b, c:d] whose first element lies at every offset 0 .. 15 elements (uint8) / 0 .. 3 (float32) behind a 16-byte
    boundary, both ways: the cut's source and the paste's destination at every alignment"""
    for dtype, e, kind, n in ((np.uint8, 0, "outside", 16), (np.float32, 0.01, "nan", 4)):
        C = content(R, dtype, e, kind)
        want = None
        for lead in range(n):
            lay = NdLayout(C.raster.shape[0], C.raster.shape[1], dtype, lead=lead)
            blobs = check_encode(B, C, lay=lay)
            assert want is None or blobs == want
            want = blobs
            check_decode(B, C, window=RW.CLIPPED, lead=lead)


def check_pixel_pitches(B, R):
    """one channel of an interleaved image, pixelPitch 3 and 9: the plain form, the same blobs and pixels; the other channels keep 0xCD"""
    for dtype, e, kind in ((np.uint8, 0, "zero"), (np.uint16, 0, "outside"), (np.float32, 0.01, "nan"), (np.float64, 0.001, "inside")):
        C = content(R, dtype, e, kind)
        for pp in (3, 9):
            lay = NdLayout(C.raster.shape[0], C.raster.shape[1], dtype, pixel_pitch=pp, first=1)
            check_encode(B, C, lay=lay)
            check_decode(B, C, pixel_pitch=pp)
            check_decode(B, C, window=RW.OVER_EVERY_EDGE, pixel_pitch=pp)


def check_range(B, R, rng):
    """a range's blobs equal the whole call's, packed and slotted; BufferTooSmall(3) one byte under nRange * slotBytes"""
    C = content(R, np.float32, 0.01, "nan")
    whole = check_encode(B, C)
    slot = RT.slot_for(C.raster[None], C.tile)
    n_range = rng[2] * rng[3]
    for s in (0, slot):
        blobs = check_encode(B, C, rng=rng, slot_bytes=s)
        assert len(blobs) == n_range and all(blobs[t] == whole[t] for t in blobs)
    raster = np.array(C.raster)
    assert B.encode_nd(raster, NAN, 0.01, C.tile, rng=rng, slot_bytes=slot, arena_cap=n_range * slot - 1)[0] == 3
    assert B.encode_nd(raster, NAN, 0.01, C.tile, rng=rng, slot_bytes=slot, arena_cap=n_range * slot)[0] == 0


def check_window(B, R, window, n_tiles):
    """a window equals the slice of the whole decode; only the touched tiles' table entries are read (the others are dead)"""
    for dtype, e, kind in ((np.float32, 0.01, "nan"), (np.uint8, 0, "zero")):
        C = content(R, dtype, e, kind)
        n_rows, n_cols = C.raster.shape
        touched = RW.window_tiles(n_rows, n_cols, C.tile, window)
        assert len(touched) == n_tiles
        whole_pix, whole_valid = check_decode(B, C)
        r0, c0, h, w = window
        b0 = B.counters()
        pix, valid = check_decode(B, C, window=window, blobs=[b if t in touched else None for t, b in enumerate(C.blobs)])
        assert sum(PX.delta(b0, B.counters())[2:]) == n_tiles
        assert same_pixels(pix, whole_pix[r0:r0 + h, c0:c0 + w]) and np.array_equal(valid, whole_valid[r0:r0 + h, c0:c0 + w])


def check_chunks(B, R):
    """LERC_AMD_TEST_RASTER_CHUNK=2, tile sub-batches of 1: several chunks a class, the same bytes both ways"""
    for dtype, e, kind in ((np.float32, 0.01, "nan"), (np.uint16, 0, "outside")):
        C = content(R, dtype, e, kind)
        plain = check_encode(B, C)
        plain_pix = check_decode(B, C, window=RW.CLIPPED)
        with RT.knobs(LERC_AMD_TEST_RASTER_CHUNK=2, LERC_AMD_TEST_TILE_SUBBATCH=1):
            assert check_encode(B, C) == plain
            assert check_encode(B, C, rng=(1, 1, 2, 2), slot_bytes=RT.slot_for(C.raster[None], C.tile)) == {t: plain[t] for t in (4, 5, 7, 8)}
            pix = check_decode(B, C, window=RW.CLIPPED)
        assert same_pixels(pix[0], plain_pix[0]) and np.array_equal(pix[1], plain_pix[1])


def check_round_trip(B, R):
    """a range encode, then a window decode inside the range from the arena where it lies and a table that holds the range only"""
    rng, window = (1, 1, 2, 2), (40, 50, 40, 45)
    for dtype, e, kind in ((np.int32, 0, "outside"), (np.float32, 0.01, "nan")):
        C = content(R, dtype, e, kind)
        n_rows, n_cols = C.raster.shape
        rc, blobs, offs, sizes, used, (ka, pa) = B.encode_nd(np.array(C.raster), C.no_data, e, C.tile, rng=rng)
        assert rc == 0
        outside = np.ones(len(offs), bool)
        outside[RW.range_tiles(n_rows, n_cols, C.tile, rng)] = False
        offs[outside], sizes[outside] = DEAD64, DEAD32
        rc, pix, valid = B.decode_nd(None, C.raster.shape, dtype, C.tile, window, C.no_data, table=(pa, offs, sizes))
        assert rc == 0, (rc, B.note())
        rows, cols = slice(40, 80), slice(50, 95)
        assert same_pixels(pix, C.want[rows, cols]) and np.array_equal(valid, C.mask[rows, cols])
        if e == 0:
            assert np.array_equal(pix, C.raster[rows, cols])    # (lossless: holes included, they hold the noData value again)


def check_damaged_blob(B, R):
    """tile 4 damaged, window (40, 50, 30, 45) over tiles 4, 5, 7, 8: tile 4's part holds noData and valid bytes 0, the rest is right, the
    status is lerc_amd_decode_device's on that blob.  Tile 0 damaged, which the window misses: status 0"""
    window = (40, 50, 30, 45)
    for dtype, e, kind in ((np.float32, 0.01, "nan"), (np.int16, 0, "outside")):
        C = content(R, dtype, e, kind)
        n_rows, n_cols = C.raster.shape
        good_pix, good_valid = check_decode(B, C, window=window)
        bad = RW.damaged(C.blobs[4])
        r0, r1, c0, c1 = RT.grid(n_rows, n_cols, C.tile)[4]
        want_rc = B.decode_one(bad, (r1 - r0, c1 - c0), dtype)[0]
        assert want_rc != 0
        rc, pix, valid = B.decode_nd(C.blobs[:4] + [bad] + C.blobs[5:], C.raster.shape, dtype, C.tile, window, C.no_data)
        assert rc == want_rc, (rc, want_rc)
        part = (slice(max(r0, window[0]) - window[0], min(r1, window[0] + window[2]) - window[0]),
                slice(max(c0, window[1]) - window[1], min(c1, window[1] + window[3]) - window[1]))
        assert pix[part].size and not valid[part].any()
        assert same_pixels(pix[part], np.full(pix[part].shape, C.no_data, dtype))
        others = np.ones((window[2], window[3]), bool)
        others[part] = False
        assert same_pixels(pix[others], good_pix[others]) and np.array_equal(valid[others], good_valid[others])
        rc, pix, valid = B.decode_nd([RW.damaged(C.blobs[0])] + C.blobs[1:], C.raster.shape, dtype, C.tile, window, C.no_data)
        assert rc == 0 and same_pixels(pix, good_pix) and np.array_equal(valid, good_valid)


def check_slot_too_small(B, R):
    """a slot 16 bytes short of the largest blob: BufferTooSmall(3), as in the masked calls; the next multiple of 16 is enough"""
    C = content(R, np.float32, 0.01, "nan")
    raster = np.array(C.raster)
    small = (max(len(b) for b in C.blobs) - 1) & ~15
    assert B.encode_nd(raster, NAN, 0.01, C.tile, slot_bytes=small)[0] == 3
    assert B.encode_nd(raster, NAN, 0.01, C.tile, slot_bytes=small + 16)[0] == 0


# ---- the boundary: status rows of the two entry points ------------------------------------------------------------------------------
INF = math.inf
# a good call: an 83 x 101 float32 raster (dt 6) at tiles of 32 x 40, rows of 106 elements; 1: a good pointer, 0: NULL
OK_ENC = dict(ctx=1, raster=1, dt=6, c=101, r=83, pp=1, pitch=106, tc=40, tr=32, rng=(0, 0, -1, -1), nd=NAN, e=0.01, arena=1, cap=1 << 20, slot=0, offs=1, sizes=1)
OK_DEC = dict(ctx=1, arena=1, offs=1, sizes=1, dt=6, c=101, r=83, tc=40, tr=32, win=(0, 0, 101, 83), out=1, pp=1, pitch=106, nd=NAN, valid=1, mpitch=104)
BIG = dict(c=50000, r=50000, tc=50000, tr=50000, dt=1, pitch=50000)    # (a tile beyond INT_MAX bytes)
# (row name, entry point, what differs from the good call, status); rng and win are (col0, row0, cols, rows)
TABLE = [
    ("encode: the good call", "enc", dict(), 0), ("encode: no context", "enc", dict(ctx=0), 2), ("encode: no raster", "enc", dict(raster=0), 2),
    ("encode: no arena", "enc", dict(arena=0), 2), ("encode: no offsets", "enc", dict(offs=0), 2), ("encode: no sizes", "enc", dict(sizes=0), 2),
    ("encode: nCols 0", "enc", dict(c=0), 2), ("encode: nRows -1", "enc", dict(r=-1), 2), ("encode: tileCols 0", "enc", dict(tc=0), 2),
    ("encode: tileRows -2", "enc", dict(tr=-2), 2), ("encode: a type that is none", "enc", dict(dt=8), 2), ("encode: slotBytes 24", "enc", dict(slot=24), 2),
    ("encode: maxZErr < 0", "enc", dict(e=-1.0), 2), ("encode: an empty range", "enc", dict(rng=(0, 0, 0, 3)), 2),
    ("encode: a range that begins outside", "enc", dict(rng=(3, 0, 1, 1)), 2), ("encode: a range that ends outside", "enc", dict(rng=(1, 0, 3, 1)), 2),
    ("encode: a negative range", "enc", dict(rng=(-1, 0, 1, 1)), 2), ("encode: all tiles from (1, 1) on", "enc", dict(rng=(1, 1, -1, -1)), 2),
    ("encode: a range inside", "enc", dict(rng=(1, 1, 2, 2)), 0), ("encode: a pitch below the width", "enc", dict(pitch=100), 2),
    ("encode: pixelPitch 0", "enc", dict(pp=0), 2), ("encode: pixelPitch 3, rows too short", "enc", dict(pp=3, pitch=300), 2),
    ("encode: noData NaN on uint16", "enc", dict(dt=3, nd=NAN), 2), ("encode: noData 0.5 on int32", "enc", dict(dt=4, nd=0.5), 2),
    ("encode: noData 300 on uint8", "enc", dict(dt=1, nd=300.0), 2), ("encode: noData -1 on uint32", "enc", dict(dt=5, nd=-1.0), 2),
    ("encode: noData 1e300 on float32", "enc", dict(nd=1e300), 2), ("encode: noData 0.1 on float32", "enc", dict(nd=0.1), 2),
    ("encode: noData inf on float32", "enc", dict(nd=INF), 0), ("encode: noData 0.1 on float64", "enc", dict(dt=7, nd=0.1, e=0.001), 0),
    ("encode: noData 4294967295 on uint32", "enc", dict(dt=5, nd=4294967295.0, e=0.0), 0),
    ("encode: beyond INT_MAX", "enc", dict(BIG, nd=0.0), 6), ("encode: noData 300 on uint8 beside beyond INT_MAX", "enc", dict(BIG, nd=300.0), 2),
    ("encode: noData NaN on uint8 beside beyond INT_MAX", "enc", dict(BIG, nd=NAN), 2),
    ("decode: the good call", "dec", dict(), 0), ("decode: no valid bytes", "dec", dict(valid=0, mpitch=0), 0), ("decode: no context", "dec", dict(ctx=0), 2),
    ("decode: no arena", "dec", dict(arena=0), 2), ("decode: no offsets", "dec", dict(offs=0), 2), ("decode: no sizes", "dec", dict(sizes=0), 2),
    ("decode: no window buffer", "dec", dict(out=0), 2), ("decode: nCols 0", "dec", dict(c=0), 2), ("decode: tileRows 0", "dec", dict(tr=0), 2),
    ("decode: a type that is none", "dec", dict(dt=9), 2), ("decode: an empty window", "dec", dict(win=(0, 0, 0, 83)), 2),
    ("decode: a window that begins outside", "dec", dict(win=(101, 0, 1, 1)), 2), ("decode: a window that ends outside", "dec", dict(win=(1, 0, 101, 83)), 2),
    ("decode: a negative window", "dec", dict(win=(0, -1, 101, 83)), 2), ("decode: a pitch below the width", "dec", dict(pitch=100), 2),
    ("decode: maskRowPitch below winCols", "dec", dict(mpitch=100), 2), ("decode: a window inside", "dec", dict(win=(23, 17, 60, 50), pitch=60, mpitch=60), 0),
    ("decode: noData NaN on uint16", "dec", dict(dt=3, nd=NAN), 2), ("decode: noData 0.5 on int32", "dec", dict(dt=4, nd=0.5), 2),
    ("decode: noData 300 on uint8", "dec", dict(dt=1, nd=300.0), 2), ("decode: noData 1e300 on float32", "dec", dict(nd=1e300), 2),
    ("decode: noData 0.1 on float32", "dec", dict(nd=0.1), 2), ("decode: beyond INT_MAX", "dec", dict(BIG, nd=0.0, win=(0, 0, 1, 1), mpitch=1), 6),
    ("decode: noData 300 on uint8 beside beyond INT_MAX", "dec", dict(BIG, nd=300.0, win=(0, 0, 1, 1), mpitch=1), 2),
]


def check_boundary(B, R):
    """the rows above.  A good call's arena holds blobs of the right type, so the rows that change the type to a good one re-encode"""
    (n_rows, n_cols), tile = ALL_CLASSES
    rasters = {dt: B.mem.up(np.zeros((n_rows, 106), capi.DT_NP[dt]) + capi.DT_NP[dt](7)) for dt in range(8)}
    ka, pa = B.mem.empty(1 << 20)
    kv, pv = B.mem.empty(83 * 106)
    for name, which, change, status in TABLE:
        a = dict(OK_ENC if which == "enc" else OK_DEC, **change)
        dt = a["dt"] if a["dt"] < 8 else 6
        kr, pr = rasters[dt]
        offs, sizes = np.zeros(9, np.uint64), np.zeros(9, np.uint32)
        if which == "enc":
            rc = B.L.lerc_amd_encode_raster_tiles_device_nodata(
                B.h if a["ctx"] else None, pr if a["raster"] else None, a["dt"], a["c"], a["r"], a["pp"], a["pitch"], a["tc"], a["tr"], *a["rng"], a["nd"],
                a["e"], pa if a["arena"] else None, a["cap"], a["slot"], offs.ctypes.data if a["offs"] else None, sizes.ctypes.data if a["sizes"] else None,
                None)
        else:
            if status == 0:
                nd = 0.0 if math.isnan(a["nd"]) and dt < 6 else a["nd"]
                assert B.L.lerc_amd_encode_raster_tiles_device_nodata(B.h, pr, dt, 101, 83, 1, 106, 40, 32, 0, 0, -1, -1, nd, 0.0, pa, 1 << 20, 0,
                                                                      offs.ctypes.data, sizes.ctypes.data, None) == 0
            rc = B.L.lerc_amd_decode_raster_window_device_nodata(
                B.h if a["ctx"] else None, pa if a["arena"] else None, offs.ctypes.data if a["offs"] else None, sizes.ctypes.data if a["sizes"] else None,
                a["dt"], a["c"], a["r"], a["tc"], a["tr"], *a["win"], pr if a["out"] else None, a["pp"], a["pitch"], a["nd"], pv if a["valid"] else None,
                a["mpitch"])
        assert rc == status, (name, rc, status, B.note())


# ---- GPU only ----------------------------------------------------------------------------------------------------------------------
def check_large_tiles(B, R):
    """1024 x 1024 float32 at tiles of 256 x 256 with NaN holes: a chunk of several full-size tiles, all of them the batch's, both ways"""
    shape_tile = ((1024, 1024), (256, 256))
    check_nan_holes_stay_inside(B, R, shape_tile)
