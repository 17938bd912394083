"""Shared by test_sim_raster_tiles.py (CPU emulator library) and test_gpu_raster_tiles.py (MI355X): a driver for the raster tile calls
of include/lerc_amd_device.h (lerc_amd_encode_raster_tiles_device / lerc_amd_decode_raster_tiles_device), rasters to feed them, and the
checks.  The reference is the judge: the expected blob of tile t is the reference's lerc_encode of the numpy slice, bands and mask
slice included; expected pixels and valid bytes are its lerc_decode's.

Addressing, the same for every case unless a case says otherwise: the raster has a row pitch of nCols + 5 elements and begins one
element (plus a guard) into its buffer, so that rows are misaligned for every type; bands are 7 elements further apart than a band
is long; the mask has a pitch of its own, nCols + 3.  Padding, and a guard region in front of and behind everything, hold a
sentinel, which must still be there after a decode -- and the source must be unchanged after an encode.
"""
import contextlib
import ctypes as ct
import os
import struct

import numpy as np

import capi
import tiles_bands_common as T
import tiles_masked_common as M

SENTINEL = 0xA5
GUARD = 16                 # elements in front of and behind a buffer's payload (a multiple of 16 bytes for every type)

ALL_CLASSES = ((83, 101), (32, 40))      # 9 tiles, all four classes, edges of 19 rows and 21 columns
THIN_EDGES = ((33, 49), (16, 24))        # edge tiles one pixel wide and high, a 1 x 1 corner
ONE_CLASS = ((64, 80), (32, 40))
ONE_TILE = ((40, 56), (64, 64))          # one tile, smaller than the tile size
SHAPES = [ALL_CLASSES, THIN_EDGES, ONE_CLASS, ONE_TILE]


def bind(L):
    T.bind(L)
    vp, u64, u32, i = ct.c_void_p, ct.c_ulonglong, ct.c_uint, ct.c_int
    L.lerc_amd_encode_raster_tiles_device.restype = u32
    L.lerc_amd_encode_raster_tiles_device.argtypes = [vp, vp, u32, i, i, i, u64, u64, i, i, i, vp, u64, ct.c_double, vp, u64, u64, vp, vp, vp]
    L.lerc_amd_decode_raster_tiles_device.restype = u32
    L.lerc_amd_decode_raster_tiles_device.argtypes = [vp, vp, vp, vp, u32, i, i, i, u64, u64, i, i, vp, i, vp, u64]
    L.lerc_amd_raster_tiles_counters.restype = None
    L.lerc_amd_raster_tiles_counters.argtypes = [vp, ct.POINTER(u64)]
    return L


def grid(n_rows, n_cols, tile):
    """[(row0, row1, col0, col1)] in tile order"""
    tr, tc = tile
    return [(r0, min(n_rows, r0 + tr), c0, min(n_cols, c0 + tc)) for r0 in range(0, n_rows, tr) for c0 in range(0, n_cols, tc)]


def classes(n_rows, n_cols, tile):
    """{(r, c): [tile indices]} -- the grid's shape classes, each one's tiles in tile order"""
    out = {}
    for t, (r0, r1, c0, c1) in enumerate(grid(n_rows, n_cols, tile)):
        out.setdefault((r1 - r0, c1 - c0), []).append(t)
    return out


@contextlib.contextmanager
def knobs(**env):
    """environment variables around the calls inside (the library reads them per call), then as they were"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class Layout:
    """where a raster [nb, R, C] (or a mask [R, C], nb 1) lies in its buffer, in elements"""

    def __init__(self, nb, n_rows, n_cols, dtype, pad, band_pad=7, lead=1):
        self.nb, self.n_rows, self.n_cols, self.dtype = nb, n_rows, n_cols, np.dtype(dtype)
        self.pitch = n_cols + pad
        self.band_pitch = n_rows * self.pitch + band_pad
        self.start = GUARD + lead
        self.n_elems = self.start + nb * self.band_pitch + GUARD

    def index(self):
        """[nb, R, C] element indices into the buffer"""
        b, i, j = np.meshgrid(np.arange(self.nb), np.arange(self.n_rows), np.arange(self.n_cols), indexing="ij")
        return self.start + b * self.band_pitch + i * self.pitch + j

    def fill(self, a=None):
        """-> the buffer as bytes: the sentinel everywhere, `a` where the raster lies"""
        buf = np.full(self.n_elems * self.dtype.itemsize, SENTINEL, np.uint8).view(self.dtype)
        if a is not None:
            buf[self.index()] = np.asarray(a, self.dtype).reshape(self.nb, self.n_rows, self.n_cols)
        return buf.view(np.uint8)

    def take(self, raw):
        """the downloaded buffer -> (the raster [nb, R, C], whether everything around it still holds the sentinel)"""
        buf = np.asarray(raw, np.uint8)[:self.n_elems * self.dtype.itemsize].view(self.dtype)
        inside = np.zeros(self.n_elems, bool)
        inside[self.index()] = True
        around = buf[~inside].view(np.uint8)
        return buf[self.index()].copy(), bool((around == SENTINEL).all())

    def address(self, base):
        return base + self.start * self.dtype.itemsize


class RasterBatch(T.BandsBatch):
    """one context of library L: the raster tile calls beside the tile calls of BandsBatch"""

    def __init__(self, L, mem):
        bind(L)
        T.BandsBatch.__init__(self, L, mem)

    def raster_counters(self):
        out = (ct.c_ulonglong * 4)()
        self.L.lerc_amd_raster_tiles_counters(self.h, out)
        return [int(v) for v in out]

    def encode_raster(self, raster, mask, e, tile, slot_bytes=0, arena_cap=None, pad=5, mask_pad=3, n_masks=None, pitch=None, tile_arg=None):
        """raster [nb, R, C], mask [R, C] or None -> (status, [blob per tile], offsets, sizes, arena bytes used).  n_masks, pitch, tile_arg:
        what the call is told where that is not the truth (argument tests)"""
        nb, n_rows, n_cols = raster.shape
        lay = Layout(nb, n_rows, n_cols, raster.dtype, pad)
        src = lay.fill(raster)
        kr, pr = self.mem.up(src)
        mlay = Layout(1, n_rows, n_cols, np.uint8, mask_pad) if mask is not None else None
        msrc = mlay.fill(mask) if mask is not None else None
        km, pm = self.mem.up(msrc) if mask is not None else (None, None)
        n = len(grid(n_rows, n_cols, tile))
        per_tile = min(tile[0], n_rows) * min(tile[1], n_cols)
        cap = int(arena_cap) if arena_cap is not None else (n * slot_bytes if slot_bytes else n * (nb * (per_tile * raster.itemsize + per_tile // 4 + 1024) + 16))
        ka, pa = self.mem.empty(cap + 16)
        offs = np.zeros(n, np.uint64)
        sizes = np.zeros(n, np.uint32)
        used = ct.c_ulonglong(0)
        tr, tc = tile_arg or tile
        rc = self.L.lerc_amd_encode_raster_tiles_device(
            self.h, lay.address(pr), capi.dt_code(raster.dtype), n_cols, n_rows, nb, lay.pitch if pitch is None else pitch, lay.band_pitch, tc, tr,
            (0 if mask is None else 1) if n_masks is None else n_masks, mlay.address(pm) if mask is not None else None,
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

    def decode_raster(self, blobs, shape, dtype, tile, with_mask, pad=5, mask_pad=3):
        """blobs in tile order, laid out at 16-byte aligned offsets -> (status, pixels [nb, R, C], valid [R, C] or None); asserts that
        padding and guards of raster and mask still hold the sentinel"""
        nb, n_rows, n_cols = shape
        n = len(blobs)
        assert n == len(grid(n_rows, n_cols, tile))
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
        lay = Layout(nb, n_rows, n_cols, dtype, pad)
        kr, pr = self.mem.up(lay.fill())
        mlay = Layout(1, n_rows, n_cols, np.uint8, mask_pad) if with_mask else None
        km, pm = self.mem.up(mlay.fill()) if with_mask else (None, None)
        rc = self.L.lerc_amd_decode_raster_tiles_device(
            self.h, pa, offs.ctypes.data, sizes.ctypes.data, capi.dt_code(dtype), n_cols, n_rows, nb, lay.pitch, lay.band_pitch, tile[1], tile[0],
            lay.address(pr), 1 if with_mask else 0, mlay.address(pm) if with_mask else None, mlay.pitch if with_mask else 0)
        pix, clean = lay.take(self.mem.down(kr))
        assert clean, "the decode wrote outside the raster's rows"
        valid = None
        if with_mask:
            valid, clean = mlay.take(self.mem.down(km))
            assert clean, "the decode wrote outside the mask's rows"
            valid = valid[0]
        return rc, pix, valid


# ---- content ----------------------------------------------------------------------------------------------------------------
def raster_of(dtype, nb, n_rows, n_cols, seed=3):
    """terrain, another one a band; float types get a fractional part (tiles_bands_common.stacks)"""
    return T.stacks(np.random.default_rng(seed), 1, nb, n_rows, n_cols, dtype)[0]


def mask_of(n_rows, n_cols, seed=5, lo=0.4, hi=0.8):
    return M.random_blob_mask(np.random.default_rng(seed), 1, n_rows, n_cols, lo, hi)[0]


def noisy_float(n_rows, n_cols, seed=7):
    """smooth content with noise of several bits: every tile, edge tiles included, is one the masked family keeps"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n_rows, 0:n_cols]
    return (900 + 400 * np.sin(yy / 23.0 + 1.0) * np.cos(xx / 31.0) + rng.normal(0, 9.0, (n_rows, n_cols))).astype(np.float32)[None]


def ref_blobs(R, raster, mask, e, tile):
    nb, n_rows, n_cols = raster.shape
    out = []
    for (r0, r1, c0, c1) in grid(n_rows, n_cols, tile):
        cut = np.ascontiguousarray(raster[:, r0:r1, c0:c1])
        rc, blob = R.encode(cut if nb > 1 else cut[0], e, n_bands=nb, mask=None if mask is None else np.ascontiguousarray(mask[r0:r1, c0:c1]))
        assert rc == 0
        out.append(blob)
    return out


def check_layout(offs, sizes, used, slot_bytes, cap=None):
    n = len(offs)
    spans = sorted((int(offs[t]), int(offs[t]) + int(sizes[t])) for t in range(n))
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, "two blobs overlap"
    assert used >= spans[-1][1], "arenaUsed covers all blobs"
    if slot_bytes:
        rooms = [int(o) // slot_bytes for o in offs]
        assert all(int(o) % slot_bytes == 0 for o in offs), "a blob begins where its room does"
        assert sorted(rooms) == list(range(n)), ("every blob in a room of its own, the rooms are the first nTiles", rooms)
        assert all(int(s) <= slot_bytes for s in sizes)
    else:
        assert all(int(o) % 16 == 0 for o in offs), "offsets are 16-byte aligned"


def slot_for(raster, tile):
    nb, n_rows, n_cols = raster.shape
    per_tile = min(tile[0], n_rows) * min(tile[1], n_cols)
    return (nb * (per_tile * raster.itemsize + per_tile // 4 + 1024) + 15) & ~15


def check_encode(B, R, raster, mask, e, tile, slot_bytes=0, want=None):
    want = want or ref_blobs(R, raster, mask, e, tile)
    rc, blobs, offs, sizes, used = B.encode_raster(raster, mask, e, tile, slot_bytes=slot_bytes)
    assert rc == 0, (rc, B.note())
    for t in range(len(want)):
        assert T.same_blob(blobs[t], want[t], raster.itemsize), "tile %d: %d bytes, the reference makes %d (%s)" % (t, len(blobs[t]), len(want[t]), B.note())
    check_layout(offs, sizes, used, slot_bytes)
    return want


def check_decode(B, R, blobs, shape, dtype, tile, with_mask):
    """-> (pixels, valid): at valid positions the reference's pixels, and its valid bytes"""
    nb, n_rows, n_cols = shape
    rc, pix, valid = B.decode_raster(blobs, shape, dtype, tile, with_mask)
    assert rc == 0, (rc, B.note())
    for t, (r0, r1, c0, c1) in enumerate(grid(n_rows, n_cols, tile)):
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


def check_parity(B, R, dtype, e, nb, with_mask, shape_tile):
    """both layouts of the encode against the reference's blobs, and the decode of the reference's blobs"""
    (n_rows, n_cols), tile = shape_tile
    raster = raster_of(dtype, nb, n_rows, n_cols)
    mask = mask_of(n_rows, n_cols) if with_mask else None
    want = check_encode(B, R, raster, mask, e, tile)
    check_encode(B, R, raster, mask, e, tile, slot_bytes=slot_for(raster, tile), want=want)
    pix, valid = check_decode(B, R, want, raster.shape, raster.dtype, tile, with_mask)
    if with_mask:
        assert np.array_equal(valid, (mask > 0).astype(np.uint8))
    if e == 0:
        m = np.ones((n_rows, n_cols), bool) if mask is None else mask > 0
        assert all(np.array_equal(pix[k][m], raster[k][m]) for k in range(nb))
    return want


def batch_delta(B, k, f):
    c0 = B.counters()
    out = f()
    c1 = B.counters()
    return out, (c1[k] - c0[k], c1[k + 1] - c0[k + 1])


def check_is_a_batch(B, R, shape_tile=ALL_CLASSES):
    """the masked family keeps every kind of tile, so with content it codes in blocks every tile is the batch's, each way"""
    (n_rows, n_cols), tile = shape_tile
    raster, mask = noisy_float(n_rows, n_cols), mask_of(n_rows, n_cols)
    n = len(grid(n_rows, n_cols, tile))
    want, moved = batch_delta(B, 0, lambda: check_encode(B, R, raster, mask, 0.01, tile))
    assert moved == (n, 0), ("tiles left the batch's launches", moved, B.note())
    _, moved = batch_delta(B, 2, lambda: check_decode(B, R, want, raster.shape, raster.dtype, tile, True))
    assert moved == (n, 0), ("tiles left the batch's launches", moved, B.note())
    return want


def check_counters_match(B, R, dtype, e, nb, with_mask, shape_tile=ALL_CLASSES):
    """the raster call moves lerc_amd_tile_batch_counters as far as the existing tile calls do on the same tiles, cut with numpy, one
    call a class on the same context -- code this change does not touch"""
    (n_rows, n_cols), tile = shape_tile
    raster = raster_of(dtype, nb, n_rows, n_cols)
    mask = mask_of(n_rows, n_cols) if with_mask else None
    g = grid(n_rows, n_cols, tile)
    (rc, blobs, _, _, _), enc = batch_delta(B, 0, lambda: B.encode_raster(raster, mask, e, tile))
    assert rc == 0
    (rc, _, _), dec = batch_delta(B, 2, lambda: B.decode_raster(blobs, raster.shape, raster.dtype, tile, with_mask))
    assert rc == 0
    enc_tiles, dec_tiles = [0, 0], [0, 0]
    for (r, c), members in classes(n_rows, n_cols, tile).items():
        tiles = np.stack([raster[:, g[t][0]:g[t][1], g[t][2]:g[t][3]] for t in members])
        masks = np.stack([mask[g[t][0]:g[t][1], g[t][2]:g[t][3]] for t in members]) if with_mask else None
        if nb > 1:
            (out, d) = batch_delta(B, 0, lambda: B.encode_bands(tiles, masks, e))
        else:
            (out, d) = batch_delta(B, 0, lambda: B.encode(np.ascontiguousarray(tiles[:, 0]), masks, e, unmasked_call=not with_mask))
        assert out[0] == 0 and out[1] == [blobs[t] for t in members]
        enc_tiles = [enc_tiles[0] + d[0], enc_tiles[1] + d[1]]
        if nb > 1:
            (out, d) = batch_delta(B, 2, lambda: B.decode_bands(out[1], (nb, r, c), dtype, 1 if with_mask else 0))
        else:
            (out, d) = batch_delta(B, 2, lambda: B.decode(out[1], (r, c), dtype, want_valid=with_mask))
        assert out[0] == 0
        dec_tiles = [dec_tiles[0] + d[0], dec_tiles[1] + d[1]]
    print("tile batch counters: encode %s, decode %s; the tile calls on the same tiles %s, %s" % (enc, dec, enc_tiles, dec_tiles))
    assert enc == tuple(enc_tiles) and dec == tuple(dec_tiles), (enc, enc_tiles, dec, dec_tiles, B.note())


def check_chunks(B, R):
    """160 x 200 at 32 x 40, 25 interior tiles, in chunks of 3 whose tile batches go in sub-batches of 2"""
    (n_rows, n_cols), tile = (160, 200), (32, 40)
    mask = mask_of(n_rows, n_cols)
    for raster, m, e in ((noisy_float(n_rows, n_cols), mask, 0.01), (raster_of(np.uint16, 1, n_rows, n_cols), None, 0)):
        want = ref_blobs(R, raster, m, e, tile)
        assert len(want) == 25
        slot = slot_for(raster, tile)
        plain = [B.encode_raster(raster, m, e, tile, slot_bytes=s) for s in (0, slot)]
        with knobs(LERC_AMD_TEST_RASTER_CHUNK=3, LERC_AMD_TEST_TILE_SUBBATCH=2):
            for s, (rc0, blobs0, _, _, _) in zip((0, slot), plain):
                rc, blobs, offs, sizes, used = B.encode_raster(raster, m, e, tile, slot_bytes=s)
                assert rc == 0 and rc0 == 0 and blobs == blobs0 and all(T.same_blob(b, w, raster.itemsize) for b, w in zip(blobs, want))
                check_layout(offs, sizes, used, s)
                if s == 0:
                    ends = [max(int(offs[t]) + int(sizes[t]) for t in range(k, min(k + 3, 25))) for k in range(0, 25, 3)]
                    begins = [min(int(offs[t]) for t in range(k, min(k + 3, 25))) for k in range(0, 25, 3)]
                    assert all(b >= e_ for b, e_ in zip(begins[1:], ends)), "a later chunk's blobs lie behind an earlier one's"
            check_decode(B, R, want, raster.shape, raster.dtype, tile, m is not None)
            if m is not None:
                used = B.encode_raster(raster, m, e, tile)[4]
                rc, blobs, _, _, _ = B.encode_raster(raster, m, e, tile, arena_cap=used)
                assert rc == 0 and blobs == plain[0][1]
                assert B.encode_raster(raster, m, e, tile, arena_cap=used - 1)[0] == 3
                small = (max(len(w) for w in want) - 1) & ~15
                assert B.encode_raster(raster, m, e, tile, slot_bytes=small)[0] == 3
                assert B.encode_raster(raster, m, e, tile, slot_bytes=small + 16)[0] == 0


def check_in_place(B, R):
    """tiles as wide as the raster and no padding: coded where they lie; with padding: through the staging buffer -- the same bytes"""
    (n_rows, n_cols), tile = (83, 56), (32, 56)
    raster = raster_of(np.uint16, 1, n_rows, n_cols)
    want = ref_blobs(R, raster, None, 0, tile)
    for pad, moved in ((0, [0, 3, 0, 3]), (5, [3, 0, 3, 0])):
        c0 = B.raster_counters()
        rc, blobs, offs, sizes, used = B.encode_raster(raster, None, 0, tile, pad=pad)
        assert rc == 0 and blobs == want
        check_layout(offs, sizes, used, 0)
        rc, pix, _ = B.decode_raster(want, raster.shape, raster.dtype, tile, False, pad=pad)
        assert rc == 0 and np.array_equal(pix, raster)
        c1 = B.raster_counters()
        assert [b - a for a, b in zip(c0, c1)] == moved, (pad, c0, c1)


def check_failing_tile(B, R, shape_tile=ALL_CLASSES):
    """tile 4 with a bit flipped under its old checksum: Failed(1), its rectangle zero in every band and in the mask, the others as before"""
    (n_rows, n_cols), tile = shape_tile
    raster, mask = noisy_float(n_rows, n_cols), mask_of(n_rows, n_cols)
    want = ref_blobs(R, raster, mask, 0.01, tile)
    rc, good_pix, good_valid = B.decode_raster(want, raster.shape, raster.dtype, tile, True)
    assert rc == 0
    bad = bytearray(want[4])
    bad[len(bad) - 9] ^= 0x10
    rc, pix, valid = B.decode_raster(want[:4] + [bytes(bad)] + want[5:], raster.shape, raster.dtype, tile, True)    # (asserts the sentinels)
    assert rc == 1, rc
    r0, r1, c0, c1 = grid(n_rows, n_cols, tile)[4]
    assert not pix[:, r0:r1, c0:c1].any() and not valid[r0:r1, c0:c1].any()
    others = np.ones((n_rows, n_cols), bool)
    others[r0:r1, c0:c1] = False
    assert np.array_equal(pix[:, others].view(np.uint8), good_pix[:, others].view(np.uint8)) and np.array_equal(valid[others], good_valid[others])


def check_arguments(B, R, shape_tile=ALL_CLASSES):
    (n_rows, n_cols), tile = shape_tile
    raster, mask = noisy_float(n_rows, n_cols), mask_of(n_rows, n_cols)
    assert B.encode_raster(raster, mask, 0.01, tile)[0] == 0
    assert B.encode_raster(raster, mask, 0.01, tile, n_masks=2)[0] == 2
    assert B.encode_raster(raster, mask, 0.01, tile, pitch=n_cols - 1)[0] == 2
    assert B.encode_raster(raster, mask, 0.01, tile, tile_arg=(0, tile[1]))[0] == 2
    slot = slot_for(raster, tile)
    assert B.encode_raster(raster, mask, 0.01, tile, slot_bytes=slot + 1, arena_cap=9 * (slot + 16))[0] == 2
    assert B.encode_raster(raster, mask, 0.01, tile, slot_bytes=slot, arena_cap=9 * slot - 1)[0] == 3
    assert B.encode_raster(raster, mask, 0.01, tile, slot_bytes=slot, arena_cap=9 * slot)[0] == 0


def header_shape(blob):
    """(nRows, nCols) a blob's header states"""
    return struct.unpack_from("<i", blob, 14)[0], struct.unpack_from("<i", blob, 18)[0]


PARITY = [(np.uint8, 0, 1, True, ALL_CLASSES), (np.uint8, 0, 1, True, THIN_EDGES),
          (np.uint16, 0, 1, False, ALL_CLASSES), (np.uint16, 0, 1, False, THIN_EDGES),
          (np.float32, 0.01, 1, True, ALL_CLASSES), (np.float32, 0.01, 1, True, THIN_EDGES),
          (np.float64, 0.001, 1, True, ALL_CLASSES), (np.float64, 0.001, 1, True, THIN_EDGES),
          (np.int8, 0, 1, False, ALL_CLASSES), (np.int32, 0, 1, True, ALL_CLASSES),
          (np.uint8, 0, 3, True, ALL_CLASSES), (np.float32, 0.01, 2, False, ALL_CLASSES),
          (np.uint16, 0, 1, True, ONE_CLASS), (np.float32, 0.01, 1, False, ONE_TILE)]


def parity_id(p):
    dtype, e, nb, with_mask, ((n_rows, n_cols), tile) = p
    return "%s%s%s-%dx%d" % ("%dx" % nb if nb > 1 else "", np.dtype(dtype).name, "-mask" if with_mask else "", n_rows, n_cols)


# the types of the parity cases other than the float32 raster of check_is_a_batch: their counters are measured against the tile calls
COUNTERS = [(np.uint8, 0, 1, True), (np.uint16, 0, 1, False), (np.float64, 0.001, 1, True), (np.int8, 0, 1, False), (np.int32, 0, 1, True),
            (np.uint8, 0, 3, True), (np.float32, 0.01, 2, False)]
