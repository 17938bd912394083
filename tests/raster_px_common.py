"""Shared by test_sim_raster_px.py (CPU emulator library) and test_gpu_raster_px.py (MI355X): a driver for the strided raster tile
calls of include/lerc_amd_device.h (lerc_amd_encode_raster_tiles_device_strided / lerc_amd_decode_raster_tiles_device_strided), buffers
that hold a raster pixel-interleaved, line-interleaved or in planes, and the checks.  The judge is raster_tiles_common's: the reference's
blobs of the numpy slices, its decode's pixels and valid bytes.

Addressing, the same for every case unless a case says otherwise: the raster begins GUARD + 1 elements into its buffer (plus the
channel it starts at), rows are 5 elements longer than they need to be, and guards, row padding and the gaps between the pixels hold
the sentinel 0xA5, which must still be everywhere outside the coded elements after a decode -- and the source must be unchanged after
an encode.
"""
import ctypes as ct

import numpy as np

import capi
import raster_tiles_common as RT

T = RT.T
SENTINEL, GUARD = RT.SENTINEL, RT.GUARD


def bind(L):
    RT.bind(L)
    vp, u64, u32, i = ct.c_void_p, ct.c_ulonglong, ct.c_uint, ct.c_int
    L.lerc_amd_encode_raster_tiles_device_strided.restype = u32
    L.lerc_amd_encode_raster_tiles_device_strided.argtypes = [vp, vp, u32, i, i, i, u64, u64, u64, i, i, i, vp, u64, ct.c_double, vp, u64, u64, vp, vp, vp]
    L.lerc_amd_decode_raster_tiles_device_strided.restype = u32
    L.lerc_amd_decode_raster_tiles_device_strided.argtypes = [vp, vp, vp, vp, u32, i, i, i, u64, u64, u64, i, i, vp, i, vp, u64]
    return L


class StridedLayout:
    """where a raster [nb, R, C] lies in its buffer, in elements: element (b, i, j) at start + b * band_pitch + i * pitch + j * pixel_pitch"""

    def __init__(self, nb, n_rows, n_cols, dtype, pixel_pitch, pitch, band_pitch, lead):
        self.nb, self.n_rows, self.n_cols, self.dtype = nb, n_rows, n_cols, np.dtype(dtype)
        self.pixel_pitch, self.pitch, self.band_pitch = pixel_pitch, pitch, band_pitch
        self.start = GUARD + lead
        self.n_elems = self.start + (nb - 1) * band_pitch + (n_rows - 1) * pitch + (n_cols - 1) * pixel_pitch + 1 + GUARD

    @classmethod
    def pixels(cls, nb, n_rows, n_cols, dtype, pixel_pitch, pad=5, lead=1, first=0):
        """pixel-interleaved: bands one element apart inside a pixel of pixel_pitch elements, the raster's band 0 the pixel's channel `first`"""
        return cls(nb, n_rows, n_cols, dtype, pixel_pitch, (n_cols - 1) * pixel_pitch + nb + pad, 1, lead + first)

    @classmethod
    def lines(cls, nb, n_rows, n_cols, dtype, pad=5, band_pad=3, lead=1):
        """line-interleaved [R][B][C]"""
        return cls(nb, n_rows, n_cols, dtype, 1, (nb - 1) * (n_cols + band_pad) + n_cols + pad, n_cols + band_pad, lead)

    @classmethod
    def planes(cls, nb, n_rows, n_cols, dtype, pad=5, band_pad=7, lead=1):
        """band-sequential, as raster_tiles_common.Layout"""
        return cls(nb, n_rows, n_cols, dtype, 1, n_cols + pad, n_rows * (n_cols + pad) + band_pad, lead)

    def index(self):
        b, i, j = np.meshgrid(np.arange(self.nb), np.arange(self.n_rows), np.arange(self.n_cols), indexing="ij")
        return self.start + b * self.band_pitch + i * self.pitch + j * self.pixel_pitch

    def fill(self, a=None):
        buf = np.full(self.n_elems * self.dtype.itemsize, SENTINEL, np.uint8).view(self.dtype)
        if a is not None:
            buf[self.index()] = np.asarray(a, self.dtype).reshape(self.nb, self.n_rows, self.n_cols)
        return buf.view(np.uint8)

    def take(self, raw):
        """the downloaded buffer -> (the raster [nb, R, C], whether everything around its elements still holds the sentinel)"""
        buf = np.asarray(raw, np.uint8)[:self.n_elems * self.dtype.itemsize].view(self.dtype)
        inside = np.zeros(self.n_elems, bool)
        inside[self.index()] = True
        around = buf[~inside].view(np.uint8)
        return buf[self.index()].copy(), bool((around == SENTINEL).all())

    def address(self, base):
        return base + self.start * self.dtype.itemsize


class PxBatch(RT.RasterBatch):
    """one context of library L: the strided raster tile calls beside RasterBatch's"""

    def __init__(self, L, mem):
        bind(L)
        RT.RasterBatch.__init__(self, L, mem)

    def encode_at(self, lay, raster, mask, e, tile, slot_bytes=0, arena_cap=None, mask_pad=3, strided=True, **told):
        """raster [nb, R, C] laid out as `lay` says -> (status, [blob per tile], offsets, sizes, arena bytes used).  told: what the call is told
        where that is not the truth (pixel_pitch, pitch, band_pitch, n_bands, n_masks).  strided False: the call without a pixel pitch"""
        nb, n_rows, n_cols = raster.shape
        src = lay.fill(raster)
        kr, pr = self.mem.up(src)
        mlay = RT.Layout(1, n_rows, n_cols, np.uint8, mask_pad) if mask is not None else None
        msrc = mlay.fill(mask) if mask is not None else None
        km, pm = self.mem.up(msrc) if mask is not None else (None, None)
        n = len(RT.grid(n_rows, n_cols, tile))
        per_tile = min(tile[0], n_rows) * min(tile[1], n_cols)
        cap = int(arena_cap) if arena_cap is not None else (n * slot_bytes if slot_bytes else n * (nb * (per_tile * raster.itemsize + per_tile // 4 + 1024) + 16))
        ka, pa = self.mem.empty(cap + 16)
        offs = np.zeros(n, np.uint64)
        sizes = np.zeros(n, np.uint32)
        used = ct.c_ulonglong(0)
        pitches = [told.get("pixel_pitch", lay.pixel_pitch), told.get("pitch", lay.pitch), told.get("band_pitch", lay.band_pitch)]
        f = self.L.lerc_amd_encode_raster_tiles_device_strided if strided else self.L.lerc_amd_encode_raster_tiles_device
        rc = f(self.h, lay.address(pr), capi.dt_code(raster.dtype), n_cols, n_rows, told.get("n_bands", nb), *(pitches if strided else pitches[1:]),
               tile[1], tile[0], told.get("n_masks", 0 if mask is None else 1), mlay.address(pm) if mask is not None else None,
               mlay.pitch if mask is not None else 0, float(e), pa, cap, int(slot_bytes), offs.ctypes.data, sizes.ctypes.data, ct.byref(used))
        assert np.array_equal(self.mem.down(kr)[:len(src)], src), "the encode changed its source"
        if mask is not None:
            assert np.array_equal(self.mem.down(km)[:len(msrc)], msrc), "the encode changed its mask"
        arena = self.mem.down(ka)
        blobs = []
        if rc == 0:
            blobs = [arena[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() for t in range(n)]
            assert arena[cap:cap + 16].tolist() == [0xCD] * 16, "bytes behind the arena were written"
        return rc, blobs, offs, sizes, int(used.value)

    def decode_at(self, lay, blobs, tile, with_mask, mask_pad=3, strided=True):
        """blobs in tile order, at 16-byte aligned offsets -> (status, pixels [nb, R, C], valid [R, C] or None); asserts that everything
        in the raster's and the mask's buffer that is no coded element still holds the sentinel"""
        nb, n_rows, n_cols = lay.nb, lay.n_rows, lay.n_cols
        n = len(blobs)
        assert n == len(RT.grid(n_rows, n_cols, tile))
        offs = np.zeros(n, np.uint64)
        sizes = np.array([len(b) for b in blobs], np.uint32)
        at = 0
        for t, b in enumerate(blobs):
            offs[t] = at
            at += (len(b) + 15) & ~15
        arena = np.zeros(at + 64, np.uint8)
        for t, b in enumerate(blobs):
            arena[int(offs[t]):int(offs[t]) + len(b)] = np.frombuffer(b, np.uint8)
        ka, pa = self.mem.up(arena)
        kr, pr = self.mem.up(lay.fill())
        mlay = RT.Layout(1, n_rows, n_cols, np.uint8, mask_pad) if with_mask else None
        km, pm = self.mem.up(mlay.fill()) if with_mask else (None, None)
        pitches = [lay.pixel_pitch, lay.pitch, lay.band_pitch]
        f = self.L.lerc_amd_decode_raster_tiles_device_strided if strided else self.L.lerc_amd_decode_raster_tiles_device
        rc = f(self.h, pa, offs.ctypes.data, sizes.ctypes.data, capi.dt_code(lay.dtype), n_cols, n_rows, nb, *(pitches if strided else pitches[1:]),
               tile[1], tile[0], lay.address(pr), 1 if with_mask else 0, mlay.address(pm) if with_mask else None, mlay.pitch if with_mask else 0)
        pix, clean = lay.take(self.mem.down(kr))
        assert clean, "the decode wrote beside the raster's coded elements"
        valid = None
        if with_mask:
            valid, clean = mlay.take(self.mem.down(km))
            assert clean, "the decode wrote outside the mask's rows"
            valid = valid[0]
        return rc, pix, valid


# ---- the cases: (dtype, nBands, pixelPitch, mask, maxZErr, (shape, tile), how it lies) ------------------------------------------------
LONG_ROWS = ((5, 700), (4, 650))         # tile rows of 650 uint16 pixels: two whole row segments of 256 and a part of one

PARITY = [
    (np.uint8, 3, 3, True, 0, RT.ALL_CLASSES, {}),
    (np.uint8, 4, 4, False, 0, RT.ALL_CLASSES, {}),
    (np.uint8, 3, 4, True, 0, RT.ALL_CLASSES, {}),
    (np.int8, 1, 3, False, 0, RT.ALL_CLASSES, {"first": 1}),
    (np.uint16, 4, 4, False, 0, RT.ALL_CLASSES, {}),
    (np.uint16, 3, 5, True, 0, RT.ALL_CLASSES, {}),
    (np.int32, 1, 2, False, 0, RT.ALL_CLASSES, {}),
    (np.float32, 2, 2, False, 0.01, RT.ALL_CLASSES, {}),
    (np.float32, 3, 3, True, 0.01, RT.ALL_CLASSES, {}),
    (np.float64, 2, 3, False, 0.001, RT.ALL_CLASSES, {}),
    (np.int16, 5, 7, False, 0, RT.ALL_CLASSES, {}),
    (np.uint16, 2, 11, False, 0, RT.ALL_CLASSES, {}),                       # (the plain form: a pixel pitch above 8 elements)
    (np.uint8, 3, 3, False, 0, RT.THIN_EDGES, {}),
    (np.float32, 4, 4, False, 0.01, RT.THIN_EDGES, {}),
    (np.uint16, 4, 4, False, 0, RT.ALL_CLASSES, {"pad": 0, "lead": 0}),     # (dense, no row padding, 16-byte aligned: whole vectors)
    (np.uint16, 2, 2, False, 0, LONG_ROWS, {}),
]
SAME_AS_PLANES = [PARITY[0], PARITY[5], PARITY[8]]


def case_id(case):
    dtype, nb, pp, with_mask, e, ((n_rows, n_cols), tile), how = case
    return "%sx%d-P%d%s-%dx%d%s" % (np.dtype(dtype).name, nb, pp, "-mask" if with_mask else "", n_rows, n_cols,
                                    "".join("-%s%d" % kv for kv in sorted(how.items())))


def content(case):
    dtype, nb, pp, with_mask, e, ((n_rows, n_cols), tile), how = case
    raster = RT.raster_of(dtype, nb, n_rows, n_cols)
    mask = RT.mask_of(n_rows, n_cols) if with_mask else None
    return raster, mask, StridedLayout.pixels(nb, n_rows, n_cols, dtype, pp, **how)


def check_encode(B, lay, raster, mask, e, tile, want, slot_bytes=0):
    rc, blobs, offs, sizes, used = B.encode_at(lay, raster, mask, e, tile, slot_bytes=slot_bytes)
    assert rc == 0, (rc, B.note())
    for t in range(len(want)):
        assert T.same_blob(blobs[t], want[t], raster.itemsize), "tile %d: %d bytes, the reference makes %d (%s)" % (t, len(blobs[t]), len(want[t]), B.note())
    RT.check_layout(offs, sizes, used, slot_bytes)
    return blobs


def check_decode(B, R, lay, blobs, tile, with_mask):
    """-> (pixels, valid): at valid positions the reference's pixels, and its valid bytes"""
    nb, n_rows, n_cols = lay.nb, lay.n_rows, lay.n_cols
    rc, pix, valid = B.decode_at(lay, blobs, tile, with_mask)
    assert rc == 0, (rc, B.note())
    for t, (r0, r1, c0, c1) in enumerate(RT.grid(n_rows, n_cols, tile)):
        rc_r, p_r, m_r = R.decode(blobs[t], want_masks=1, n_bands=nb)
        assert rc_r == 0
        p_r = p_r.reshape(nb, r1 - r0, c1 - c0)
        m = m_r[0] > 0
        if with_mask:
            assert np.array_equal(valid[r0:r1, c0:c1], m_r[0]), "tile %d: valid bytes differ from the reference's" % t
        else:
            assert m.all()
        for k in range(nb):
            assert np.array_equal(pix[k, r0:r1, c0:c1][m].view(np.uint8), p_r[k][m].view(np.uint8)), "tile %d band %d: valid pixels differ from the reference's" % (t, k)
    return pix, valid


def check_parity(B, R, case):
    """packed and slotted encode against the reference's blobs, and the decode of the reference's blobs"""
    dtype, nb, pp, with_mask, e, ((n_rows, n_cols), tile), how = case
    raster, mask, lay = content(case)
    want = RT.ref_blobs(R, raster, mask, e, tile)
    check_encode(B, lay, raster, mask, e, tile, want)
    check_encode(B, lay, raster, mask, e, tile, want, slot_bytes=RT.slot_for(raster, tile))
    pix, valid = check_decode(B, R, lay, want, tile, with_mask)
    if with_mask:
        assert np.array_equal(valid, (mask > 0).astype(np.uint8))
    if e == 0:
        m = np.ones((n_rows, n_cols), bool) if mask is None else mask > 0
        assert all(np.array_equal(pix[k][m], raster[k][m]) for k in range(nb))


def delta(before, after):
    return [b - a for a, b in zip(before, after)]


def check_same_as_planes(B, R, case):
    """the interleaved raster and its planar copy: the same blobs, the same moves of the tile batch counters (batch membership does not
    depend on the layout), and n tiles through the staging buffer each way"""
    dtype, nb, pp, with_mask, e, ((n_rows, n_cols), tile), how = case
    raster, mask, lay = content(case)
    n = len(RT.grid(n_rows, n_cols, tile))
    b0 = B.counters()
    rc, planar, _, _, _ = B.encode_raster(raster, mask, e, tile)
    assert rc == 0
    rc, _, _ = B.decode_raster(planar, raster.shape, raster.dtype, tile, with_mask)
    assert rc == 0
    b1, r1 = B.counters(), B.raster_counters()
    rc, blobs, _, _, _ = B.encode_at(lay, raster, mask, e, tile)
    assert rc == 0 and blobs == planar
    rc, _, _ = B.decode_at(lay, blobs, tile, with_mask)
    assert rc == 0
    b2, r2 = B.counters(), B.raster_counters()
    assert delta(b1, b2) == delta(b0, b1), (b0, b1, b2, B.note())
    assert delta(r1, r2) == [n, 0, n, 0], (r1, r2)


def check_pixel_pitch_one(B, R):
    """pixelPitch 1, band-sequential: the strided call is the call without a pixel pitch -- blobs, sizes, arena bytes used, counters, and
    the offsets where the layout determines them (slotted), on the two rasters of raster_tiles_common.check_in_place"""
    (n_rows, n_cols), tile = (83, 56), (32, 56)
    raster = RT.raster_of(np.uint16, 1, n_rows, n_cols)
    want = RT.ref_blobs(R, raster, None, 0, tile)
    for pad, moved in ((0, [0, 3, 0, 3]), (5, [3, 0, 3, 0])):
        lay = StridedLayout.planes(1, n_rows, n_cols, np.uint16, pad=pad)
        old = B.encode_at(lay, raster, None, 0, tile, strided=False)
        new = B.encode_at(lay, raster, None, 0, tile)
        assert old[0] == new[0] == 0 and new[1] == old[1] == want
        assert np.array_equal(new[3], old[3]) and new[4] == old[4], (new[3], old[3], new[4], old[4])
        RT.check_layout(new[2], new[3], new[4], 0)
        # (packed, the one-launch tile encoder hands out arena space in the order its workgroups finish -- "the order in the arena is the
        # call's own", two calls of ONE entry point differ there on a GPU --, so the offsets are compared where they are determined: slotted)
        slot = RT.slot_for(raster, tile)
        old_s = B.encode_at(lay, raster, None, 0, tile, slot_bytes=slot, strided=False)
        new_s = B.encode_at(lay, raster, None, 0, tile, slot_bytes=slot)
        assert old_s[0] == new_s[0] == 0 and new_s[1] == old_s[1] == want
        assert np.array_equal(new_s[2], old_s[2]) and np.array_equal(new_s[3], old_s[3]) and new_s[4] == old_s[4], (new_s[2:], old_s[2:])
        c0 = B.raster_counters()
        new = B.encode_at(lay, raster, None, 0, tile)
        assert new[0] == 0 and new[1] == want
        rc, pix, _ = B.decode_at(lay, want, tile, False)
        assert rc == 0 and np.array_equal(pix, raster)
        assert delta(c0, B.raster_counters()) == moved, (pad, c0, B.raster_counters())


def check_line_interleaved(B, R):
    """uint16 x 3 laid out [R][B][C] with padding: parity through the strided call; the call without a pixel pitch refuses the description"""
    (n_rows, n_cols), tile = RT.ALL_CLASSES
    raster = RT.raster_of(np.uint16, 3, n_rows, n_cols)
    lay = StridedLayout.lines(3, n_rows, n_cols, np.uint16)
    want = RT.ref_blobs(R, raster, None, 0, tile)
    c0 = B.raster_counters()
    check_encode(B, lay, raster, None, 0, tile, want)
    pix, _ = check_decode(B, R, lay, want, tile, False)
    assert np.array_equal(pix, raster)
    assert delta(c0, B.raster_counters()) == [9, 0, 9, 0]
    assert B.encode_at(lay, raster, None, 0, tile, strided=False)[0] == 2
    assert B.decode_at(lay, want, tile, False, strided=False)[0] == 2


def check_chunks(B, R):
    """160 x 200 float32 x 3 / P 4 with a mask at 32 x 40: 25 interior tiles in chunks of 3 whose tile batches go in sub-batches of 2"""
    (n_rows, n_cols), tile = (160, 200), (32, 40)
    raster, mask = RT.raster_of(np.float32, 3, n_rows, n_cols), RT.mask_of(n_rows, n_cols)
    lay = StridedLayout.pixels(3, n_rows, n_cols, np.float32, 4)
    want = RT.ref_blobs(R, raster, mask, 0.01, tile)
    assert len(want) == 25
    plain = check_encode(B, lay, raster, mask, 0.01, tile, want)
    with RT.knobs(LERC_AMD_TEST_RASTER_CHUNK=3, LERC_AMD_TEST_TILE_SUBBATCH=2):
        for s in (0, RT.slot_for(raster, tile)):
            assert check_encode(B, lay, raster, mask, 0.01, tile, want, slot_bytes=s) == plain
        _, valid = check_decode(B, R, lay, want, tile, True)
        assert np.array_equal(valid, (mask > 0).astype(np.uint8))


def check_failing_tile(B, R, shape_tile=RT.ALL_CLASSES):
    """uint8 x 3 / P 4 with a mask, tile 4 with a bit flipped under its old checksum: Failed(1), its rectangle zero in the three bands and in
    the mask, the fourth channel and every other sentinel intact (decode_at asserts it), the other tiles as before"""
    (n_rows, n_cols), tile = shape_tile
    raster, mask = RT.raster_of(np.uint8, 3, n_rows, n_cols), RT.mask_of(n_rows, n_cols)
    lay = StridedLayout.pixels(3, n_rows, n_cols, np.uint8, 4)
    want = RT.ref_blobs(R, raster, mask, 0, tile)
    rc, good_pix, good_valid = B.decode_at(lay, want, tile, True)
    assert rc == 0
    bad = bytearray(want[4])
    bad[len(bad) - 9] ^= 0x10
    rc, pix, valid = B.decode_at(lay, want[:4] + [bytes(bad)] + want[5:], tile, True)
    assert rc == 1, rc
    r0, r1, c0, c1 = RT.grid(n_rows, n_cols, tile)[4]
    assert not pix[:, r0:r1, c0:c1].any() and not valid[r0:r1, c0:c1].any()
    others = np.ones((n_rows, n_cols), bool)
    others[r0:r1, c0:c1] = False
    assert np.array_equal(pix[:, others], good_pix[:, others]) and np.array_equal(valid[others], good_valid[others])


def check_arguments(B, R, shape_tile=RT.ALL_CLASSES):
    (n_rows, n_cols), tile = shape_tile
    raster, mask = RT.raster_of(np.uint8, 3, n_rows, n_cols), RT.mask_of(n_rows, n_cols)
    lay = StridedLayout.pixels(3, n_rows, n_cols, np.uint8, 3)
    assert B.encode_at(lay, raster, mask, 0, tile)[0] == 0
    assert B.encode_at(lay, raster, mask, 0, tile, pixel_pitch=0)[0] == 2
    assert B.encode_at(lay, raster, mask, 0, tile, n_bands=4)[0] == 2                                  # (pixelPitch 3, nBands 4)
    assert B.encode_at(lay, raster, mask, 0, tile, band_pitch=2)[0] == 2
    assert B.encode_at(lay, raster, mask, 0, tile, pitch=(n_cols - 1) * 3 + 3 - 1)[0] == 2
    assert B.encode_at(lay, raster, mask, 0, tile, n_masks=2)[0] == 2
    slot = RT.slot_for(raster, tile)
    assert B.encode_at(lay, raster, mask, 0, tile, slot_bytes=slot + 1, arena_cap=9 * (slot + 16))[0] == 2
    used = B.encode_at(lay, raster, mask, 0, tile)[4]
    assert B.encode_at(lay, raster, mask, 0, tile, arena_cap=used - 1)[0] == 3
    assert B.encode_at(lay, raster, mask, 0, tile, arena_cap=used)[0] == 0
