"""Shared by test_sim_tiles_depth.py (CPU emulator library) and test_gpu_tiles_depth.py (MI355X): a driver for the depth tile batch
calls of include/lerc_amd_depth.h (lerc_amd_encode_tiles_device_depth / lerc_amd_decode_tiles_device_depth), depth tiles to feed them,
and the rule for what such a batch may hand back: nothing, unless the call's own arguments (8-bit values, nDepth > 8, maxZErr 0 on
float values, 777) or a tile's content (a NaN at a valid pixel, a blob of codec < 6, damage) say so -- every kind of blob the
reference makes of a wide type stays inside the batch's own launches.

Tiles are [nTiles, nRows, nCols, nDepth]; masks [nTiles, nRows, nCols] or None."""
import ctypes as ct
import struct

import numpy as np

import capi
import cases
import tiles_masked_common as M
from tiles_masked_common import HDR, GpuMem, HostMem, check_layout, random_blob_mask, sub_batches_of    # noqa: F401

TYPES = [(np.uint16, 0), (np.int16, 0), (np.int32, 0), (np.uint32, 0), (np.float32, 0.01), (np.float64, 0.001)]


def bind(L):
    M.bind(L)
    vp, u64, u32, i = ct.c_void_p, ct.c_ulonglong, ct.c_uint, ct.c_int
    L.lerc_amd_encode_tiles_device_depth.restype = u32
    L.lerc_amd_encode_tiles_device_depth.argtypes = [vp, vp, u32, i, i, i, i, vp, ct.c_double, vp, u64, u64, vp, vp, vp]
    L.lerc_amd_decode_tiles_device_depth.restype = u32
    L.lerc_amd_decode_tiles_device_depth.argtypes = [vp, vp, vp, vp, i, i, i, i, u32, vp, vp]
    return L


def slot_for(tiles):
    n, r, c, d = tiles.shape
    return (tiles[0].nbytes + r * c // 2 + 1024 + 15) & ~15


class DepthBatch(M.Batch):
    """one context of library L, the depth calls beside the masked ones of tiles_masked_common.Batch"""

    def __init__(self, L, mem):
        bind(L)
        M.Batch.__init__(self, L, mem)

    def encode_depth(self, tiles, masks, max_z_err, slot_bytes=0, arena_cap=None, arena_shift=0):
        """-> (status, [blob bytes per tile], offsets, sizes, arena bytes used); 0xCD guards in front of and behind the arena"""
        n, r, c, d = tiles.shape
        kt, pt = self.mem.up(tiles)
        km, pm = self.mem.up(masks) if masks is not None else (None, None)
        cap = int(arena_cap) if arena_cap is not None else (n * slot_bytes if slot_bytes else n * slot_for(tiles))
        ka, pa = self.mem.empty(arena_shift + cap + 16)
        pa += arena_shift
        offs = np.zeros(n, np.uint64)
        sizes = np.zeros(n, np.uint32)
        used = ct.c_ulonglong(0)
        rc = self.L.lerc_amd_encode_tiles_device_depth(self.h, pt, capi.dt_code(tiles.dtype), c, r, d, n, pm, float(max_z_err), pa, cap, int(slot_bytes),
                                                       offs.ctypes.data, sizes.ctypes.data, ct.byref(used))
        arena = self.mem.down(ka)
        assert arena[:arena_shift].tolist() == [0xCD] * arena_shift, "bytes in front of the arena were written"
        arena = arena[arena_shift:]
        assert arena[cap:].tolist() == [0xCD] * 16, "bytes behind the arena were written"
        blobs = []
        if rc == 0:
            blobs = [arena[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() for t in range(n)]
        return rc, blobs, offs, sizes, int(used.value)

    def decode_depth(self, blobs, shape, dtype, want_valid=True, depth_arg=None):
        """blobs laid out at 16-byte aligned offsets -> (status, pixels [n, r, c, d], valid bytes [n, r, c] or None)"""
        n = len(blobs)
        r, c, d = shape
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
        item = np.dtype(dtype).itemsize
        ko, po = self.mem.empty(n * r * c * d * item + 16)
        kv, pv = self.mem.empty(n * r * c + 16) if want_valid else (None, None)
        rc = self.L.lerc_amd_decode_tiles_device_depth(self.h, pa, offs.ctypes.data, sizes.ctypes.data, n, c, r, d if depth_arg is None else depth_arg,
                                                       capi.dt_code(dtype), po, pv)
        raw = self.mem.down(ko)
        assert raw[n * r * c * d * item:].tolist() == [0xCD] * 16, "bytes behind the pixels were written"
        pix = raw[:n * r * c * d * item].view(dtype).reshape(n, r, c, d)
        valid = None
        if want_valid:
            rawv = self.mem.down(kv)
            assert rawv[n * r * c:].tolist() == [0xCD] * 16, "bytes behind the valid bytes were written"
            valid = rawv[:n * r * c].reshape(n, r, c)
        return rc, pix, valid

    def decode_one_depth(self, blob, shape, dtype, want_valid=True):
        """lerc_amd_decode_device with nDepth -> (status, pixels [r, c, d], valid bytes [r, c] or None)"""
        r, c, d = shape
        kb, pb = self.mem.up(np.frombuffer(blob, np.uint8))
        item = np.dtype(dtype).itemsize
        ko, po = self.mem.empty(r * c * d * item)
        kv, pv = self.mem.empty(r * c) if want_valid else (None, None)
        rc = self.L.lerc_amd_decode_device(self.h, pb, len(blob), 1 if want_valid else 0, pv, d, c, r, 1, capi.dt_code(dtype), po)
        pix = self.mem.down(ko, r * c * d * item).view(dtype).reshape(r, c, d)
        return rc, pix, (self.mem.down(kv, r * c).reshape(r, c) if want_valid else None)


# ---- the reference's word --------------------------------------------------------------------------------------------------
def ref_blobs(R, tiles, masks, e):
    out = []
    for t in range(len(tiles)):
        rc, blob = R.encode(tiles[t], e, n_depth=tiles.shape[3], mask=None if masks is None else masks[t])
        assert rc == 0
        out.append(blob)
    return out


def header(blob):
    """-> dict of the codec 6 header's fields the tests ask about"""
    version, _, n_rows, n_cols, n_depth, num_valid, mb, blob_size, dt = struct.unpack_from("<iIiiiiiii", blob, 6)
    max_z_err, z_min, z_max = struct.unpack_from("<ddd", blob, 50)
    return dict(version=version, n_depth=n_depth, num_valid=num_valid, mb=mb, blob_size=blob_size, max_z_err=max_z_err, z_min=z_min, z_max=z_max,
                rle=struct.unpack_from("<i", blob, HDR)[0] if len(blob) >= HDR + 4 else 0)


def kind_of(blob, item):
    """what lies behind the mask section of a depth blob: empty, const, const_slices, one_sweep, blocks8, blocks16"""
    h = header(blob)
    if h["num_valid"] == 0:
        return "empty"
    if h["z_min"] == h["z_max"]:
        return "const"
    at = HDR + 4 + h["rle"] + 2 * h["n_depth"] * item
    if h["blob_size"] == at:
        return "const_slices"
    if blob[at] == 1:
        return "one_sweep"
    return "blocks%d" % h["mb"]


# ---- depth tiles -----------------------------------------------------------------------------------------------------------
def surface(rng, n, r, c, amp=600.0):
    yy, xx = np.mgrid[0:r, 0:c]
    out = np.zeros((n, r, c))
    for t in range(n):
        for _ in range(4):
            out[t] += rng.uniform(0.2, 1.0) * amp * np.sin(yy / rng.uniform(3, 15) + rng.uniform(0, 6)) * np.cos(xx / rng.uniform(3, 15) + rng.uniform(0, 6))
    return out


def tiles_of(rng, n, r, c, d, dtype):
    """a surface a slice, the slices of a tile related (a common part and a part of their own); float types get a fractional part"""
    dtype = np.dtype(dtype)
    common = surface(rng, n, r, c)[..., None]
    own = surface(rng, n * d, r, c, amp=80.0).reshape(n, d, r, c).transpose(0, 2, 3, 1)
    t = common + own + 100.0 * np.arange(d)
    if dtype.kind == "f":
        return (t + rng.normal(0, 0.3, t.shape)).astype(dtype)
    if dtype.kind == "u":
        t = t + 3000
    if dtype.itemsize == 4:
        t = t * 37
    return np.rint(t).astype(dtype)


def masks_of(rng, n, r, c):
    """partly valid tiles, with an all-valid tile among them"""
    m = random_blob_mask(rng, n, r, c)
    if n > 1:
        m[1][:] = 1
    return m


# ---- checks ----------------------------------------------------------------------------------------------------------------
def check_encode(B, R, tiles, masks, e, slot_bytes=0, want=None, single=0, arena_shift=0, arena_cap=None):
    """every tile's blob equals the reference's, the layout holds, `single` tiles went one by one and all others through the batch's
    own launches -> reference blobs"""
    want = want or ref_blobs(R, tiles, masks, e)
    n = len(tiles)
    c0 = B.counters()
    rc, blobs, offs, sizes, used = B.encode_depth(tiles, masks, e, slot_bytes=slot_bytes, arena_shift=arena_shift, arena_cap=arena_cap)
    c1 = B.counters()
    assert rc == 0, (rc, B.note())
    for t in range(n):
        assert same_blob(blobs[t], want[t], tiles.itemsize), "tile %d: %d bytes, the reference makes %d (%s)" % (t, len(blobs[t]), len(want[t]), B.note())
    check_layout(offs, sizes, used, slot_bytes)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (n - single, single), (c0, c1, B.note())
    return want


def same_blob(got, want, item):
    """byte for byte -- but for the bytes of a lossless float blob that the reference itself leaves to chance (cases.lossless_float_dont_care),
    which no blob of maxZErr > 0 and no integer blob has"""
    if got == want or len(got) != len(want):
        return got == want
    a, b = bytearray(got), bytearray(want)
    for k in cases.lossless_float_dont_care(want, item):
        a[k] = b[k] = 0
    return a == b


def check_decode(B, R, blobs, shape, dtype, want_valid=True, single=0):
    """pixels and valid bytes equal lerc_amd_decode_device's and the reference's, tile by tile"""
    r, c, d = shape
    c0 = B.counters()
    rc, pix, valid = B.decode_depth(blobs, shape, dtype, want_valid=want_valid)
    c1 = B.counters()
    assert rc == 0, (rc, B.note())
    for t, blob in enumerate(blobs):
        rc1, p1, v1 = B.decode_one_depth(blob, shape, dtype, want_valid=want_valid)
        assert rc1 == 0
        assert pix[t].tobytes() == p1.tobytes(), "tile %d: pixels differ from lerc_amd_decode_device's (%s)" % (t, B.note())
        rc_r, p_r, m_r = R.decode(blob, want_masks=1 if want_valid else 0)
        assert rc_r == 0
        assert pix[t].tobytes() == p_r.reshape(r, c, d).tobytes(), "tile %d: pixels differ from the reference's" % t
        if want_valid:
            assert np.array_equal(valid[t], v1) and np.array_equal(valid[t], m_r.reshape(r, c)), "tile %d: valid bytes differ" % t
    assert (c1[2] - c0[2], c1[3] - c0[3]) == (len(blobs) - single, single), (c0, c1, B.note())


def check_parity(B, R, dtype, e, d, with_mask, slotted, n=12, r=33, c=41, seed=1):
    rng = np.random.default_rng(seed + d)
    tiles = tiles_of(rng, n, r, c, d, dtype)
    masks = masks_of(rng, n, r, c) if with_mask else None
    want = check_encode(B, R, tiles, masks, e, slot_bytes=slot_for(tiles) if slotted else 0)
    check_decode(B, R, want, (r, c, d), dtype, want_valid=with_mask)


def diff_tiles(R, rng, n, r, c, d, dtype):
    """lossless integer tiles whose slices are one rough surface plus small noise: the difference to the slice in front is the shorter
    block.  Asserted here: the reference's codec 6 blob is smaller than its codec 4 blob, which has no difference coding (and a shorter
    header), so a difference block was chosen"""
    dtype = np.dtype(dtype)
    base = rng.integers(0, 20000, (n, r, c, 1)) + (3000 if dtype.kind == "u" else -9000)
    tiles = (base + rng.integers(0, 4, (n, r, c, d))).astype(dtype)
    for t in range(n):
        rc6, b6 = R.encode(tiles[t], 0, n_depth=d)
        rc4, _, _, b4 = R.encode_for_version(tiles[t], 4, 0, n_depth=d)
        assert rc6 == 0 and rc4 == 0 and len(b6) < len(b4), (len(b6), len(b4))
    return tiles


def check_slice_differences(B, R):
    rng = np.random.default_rng(11)
    r, c, d = 33, 41, 3
    for dtype in (np.uint16, np.int16, np.int32, np.uint32):
        tiles = np.concatenate([diff_tiles(R, rng, 4, r, c, d, dtype), tiles_of(rng, 2, r, c, d, dtype),
                                rng.integers(0, 30000, (2, r, c, d)).astype(dtype)])    # (independent noise a slice beside them)
        masks = masks_of(rng, len(tiles), r, c)
        want = check_encode(B, R, tiles, masks, 0)
        check_decode(B, R, want, (r, c, d), dtype)
    # int32 slices near INT_MIN and INT_MAX: the difference leaves int, the plain form is written; uint32 above 2^31
    lo = (-2**31 + rng.integers(0, 50, (1, r, c, 1))).astype(np.int64)
    hi = (2**31 - 1 - rng.integers(0, 50, (1, r, c, 1))).astype(np.int64)
    t32 = np.concatenate([lo, hi, lo + 7], axis=3).astype(np.int32)
    t32 = np.concatenate([t32, diff_tiles(R, rng, 1, r, c, d, np.int32)])
    want = check_encode(B, R, t32, None, 0)
    check_decode(B, R, want, (r, c, d), np.int32, want_valid=False)
    u32 = (2**31 + 5000 + rng.integers(0, 20000, (2, r, c, 1)) + rng.integers(0, 4, (2, r, c, d))).astype(np.uint32)
    u32[1, :, :, 1] = rng.integers(0, 100, (r, c))    # (a slice far below the others: differences near 2^31)
    want = check_encode(B, R, u32, None, 0)
    check_decode(B, R, want, (r, c, d), np.uint32, want_valid=False)


def kinds_float(rng, r=64, c=64, d=3):
    """float32 tiles at maxZErr 0.01, one of every kind -> (tiles, masks, the kinds the reference must make of them or None)"""
    yy, xx = np.mgrid[0:r, 0:c]
    n = 10
    t = np.zeros((n, r, c, d), np.float32)
    m = np.ones((n, r, c), np.uint8)
    kinds = [None] * n
    m[0][:] = 0; t[0] = 3.5; kinds[0] = "empty"
    t[1] = 7.25; m[1][::3] = 0; kinds[1] = "const"
    t[2] = np.array([1.5, -2.25, 100.0], np.float32); m[2][:, ::5] = 0; kinds[2] = "const_slices"
    t[3] = rng.uniform(-1e9, 1e9, (r, c, d)); kinds[3] = "one_sweep"    # (noise far beyond what 0.01 quantises)
    t[4] = (5 + (yy // 16) * 0.37)[..., None] + rng.normal(0, 0.001, (r, c, d)); kinds[4] = "blocks16"    # (four plains: next to nothing a block)
    lut = np.array([0.0, 100.5, 2000.25, 30000.125], np.float32)
    t[5] = lut[np.repeat(rng.integers(0, 4, (r, c // 8, d)), 8, axis=1)]; kinds[5] = "blocks8"    # (few distinct values in runs: LUT blocks)
    t[6] = np.rint(surface(rng, 1, r, c)[0][..., None] + 10 * np.arange(d))    # (all-integer values: the header says so)
    t[7] = np.round(surface(rng, 1, r, c, amp=20.0)[0][..., None] + np.arange(d), 1)    # (multiples of 0.1: TryRaiseMaxZError raises the bound)
    t[8] = surface(rng, 1, r, c)[0][..., None] + rng.normal(0, 0.3, (r, c, d)); m[8][:] = 0; m[8][17, 23] = 1    # (one valid pixel)
    t[9] = surface(rng, 1, r, c)[0][..., None] + rng.normal(0, 0.3, (r, c, d)); m[9] = random_blob_mask(rng, 1, r, c)[0]
    return t, m, kinds


def kinds_int(rng, r=64, c=64, d=2):
    """uint16 tiles, lossless, one of every kind"""
    n = 7
    t = np.zeros((n, r, c, d), np.uint16)
    m = np.ones((n, r, c), np.uint8)
    kinds = [None] * n
    m[0][:] = 0; kinds[0] = "empty"
    t[1] = 77; m[1][5:9] = 0; kinds[1] = "const"
    t[2] = np.array([4, 60000], np.uint16); kinds[2] = "const_slices"
    t[3] = rng.integers(0, 65536, (r, c, d)); m[3][:, ::7] = 0; kinds[3] = "one_sweep"
    t[4] = (500 + (np.mgrid[0:r, 0:c][0] // 16) * 3)[..., None] + np.arange(d); kinds[4] = "blocks16"
    t[5] = np.array([1, 900, 30000, 65535], np.uint16)[np.repeat(rng.integers(0, 4, (r, c // 8, d)), 8, axis=1)]; kinds[5] = "blocks8"
    t[6] = tiles_of(rng, 1, r, c, d, np.uint16)[0]; m[6][:] = 0; m[6][63, 63] = 1
    return t, m, kinds


def check_kinds(B, R):
    rng = np.random.default_rng(21)
    for make, e, dtype in ((kinds_float, 0.01, np.float32), (kinds_int, 0, np.uint16)):
        tiles, masks, kinds = make(rng)
        want = ref_blobs(R, tiles, masks, e)
        for t, k in enumerate(kinds):
            if k:
                assert kind_of(want[t], tiles.itemsize) == k, (t, k, kind_of(want[t], tiles.itemsize))
        if dtype == np.float32:
            h6, h7 = header(want[6]), header(want[7])
            assert h6["max_z_err"] == 0.5 and want[6][47] == 1, "tile 6: all-integer float values"
            assert h7["max_z_err"] > 0.01, "tile 7: TryRaiseMaxZError raises the bound"
        check_encode(B, R, tiles, masks, e, want=want)
        check_encode(B, R, tiles, masks, e, want=want, slot_bytes=slot_for(tiles))
        check_decode(B, R, want, tiles.shape[1:], dtype)


def check_hand_backs(B, R):
    rng = np.random.default_rng(31)
    r, c, d = 33, 41, 3
    n = 4
    masks = masks_of(rng, n, r, c)
    # ---- the call's arguments: every tile one by one, the reference's bytes
    t8 = (tiles_of(rng, n, r, c, d, np.int16) % 251).astype(np.uint8)
    want = check_encode(B, R, t8, masks, 0, single=n)
    assert "8-bit" in B.note() and "tile 0" in B.note(), B.note()
    check_decode(B, R, want, (r, c, d), np.uint8, single=n)
    assert "8-bit" in B.note(), B.note()
    t9 = tiles_of(rng, 2, 17, 9, 9, np.uint16)
    want = check_encode(B, R, t9, None, 0, single=2)
    assert "tile 0" in B.note() and "values a pixel" in B.note(), B.note()
    check_decode(B, R, want, (17, 9, 9), np.uint16, want_valid=False, single=2)
    tf = tiles_of(rng, n, r, c, d, np.float32)
    check_encode(B, R, tf, masks, 0, single=n)
    assert "error bound of 0" in B.note(), B.note()
    # ---- a tile's content: NaN in every slice of a valid pixel of tile 2 -- the reference makes the pixel invalid, and so does the
    # single encoder the tile is handed to; NaN in one slice only: the reference's status, NaN (4), is the call's
    tn = tf.copy()
    masks[2][4, 5] = 1
    tn[2, 4, 5, :] = np.nan
    check_encode(B, R, tn, masks, 0.01, single=1)
    assert "tile 2" in B.note() and "NaN" in B.note(), B.note()
    tn[2, 4, 5, 0] = 1.0
    assert R.encode(tn[2], 0.01, n_depth=d, mask=masks[2])[0] == 4
    assert B.encode_depth(tn, masks, 0.01)[0] == 4
    assert "tile 2" in B.note() and "NaN" in B.note(), B.note()
    # ---- a slot too small for one tile: that tile says so when it is encoded by itself
    ti = tiles_of(rng, n, r, c, d, np.uint16)
    ti[2] = rng.integers(0, 65536, (r, c, d))    # (noise: by far the largest blob)
    masks[2][:] = 1
    sizes = [len(b) for b in ref_blobs(R, ti, masks, 0)]
    slot = (max(sizes[:2] + sizes[3:]) + 15) & ~15
    assert slot < sizes[2], (slot, sizes)
    c0 = B.counters()
    rc = B.encode_depth(ti, masks, 0, slot_bytes=slot)[0]
    c1 = B.counters()
    assert rc == 3, (rc, B.note())    # BufferTooSmall: the reference's word for a buffer of that size
    assert R.encode(ti[2], 0, n_depth=d, mask=masks[2], buf_size=slot)[0] == 3
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (n - 1, 0), (c0, c1)    # (the others by the batch's launches, tile 2 not encoded at all)
    assert "tile 2" in B.note() and "slot" in B.note(), B.note()
    # ---- decode: a codec 4 blob, a blob with one corrupted byte, a blob of another nDepth
    want = ref_blobs(R, ti, masks, 0)
    rc4, _, _, b4 = R.encode_for_version(ti[1], 4, 0, n_depth=d, mask=masks[1])
    assert rc4 == 0
    mixed = [want[0], b4, want[2], want[3]]
    check_decode(B, R, mixed, (r, c, d), np.uint16, single=1)
    assert "tile 1" in B.note(), B.note()
    bad = bytearray(want[2])
    bad[len(bad) // 2] ^= 0x10
    bad = bytes(bad)
    rc1 = B.decode_one_depth(bad, (r, c, d), np.uint16)[0]
    assert rc1 != 0
    c0 = B.counters()
    rc, pix, valid = B.decode_depth([want[0], want[1], bad, want[3]], (r, c, d), np.uint16)
    c1 = B.counters()
    assert rc == rc1, (rc, rc1, B.note())
    assert (c1[2] - c0[2], c1[3] - c0[3]) == (3, 1)
    assert not pix[2].any() and not valid[2].any(), "a tile that fails is left zeroed"
    for t in (0, 1, 3):
        rc_r, p_r, m_r = R.decode(want[t], want_masks=1)
        assert pix[t].tobytes() == p_r.reshape(r, c, d).tobytes() and np.array_equal(valid[t], m_r.reshape(r, c))
    t2 = tiles_of(rng, 2, r, c, 2, np.uint16)
    w2 = ref_blobs(R, t2, None, 0)
    c0 = B.counters()
    rc, pix, _ = B.decode_depth(w2, (r, c, 3), np.uint16, want_valid=False)
    c1 = B.counters()
    assert rc != 0 and (c1[2] - c0[2], c1[3] - c0[3]) == (0, 2) and not pix.any(), (rc, B.note())


def check_sub_batches(B, R):
    rng = np.random.default_rng(41)
    r, c, d = 17, 9, 4
    tiles = tiles_of(rng, 8, r, c, d, np.int32)
    masks = masks_of(rng, 8, r, c)
    with sub_batches_of(3):
        want = check_encode(B, R, tiles, masks, 0)
        check_encode(B, R, tiles, masks, 0, want=want, slot_bytes=slot_for(tiles))
        check_encode(B, R, tiles, masks, 0, want=want, arena_shift=1)
        check_decode(B, R, want, (r, c, d), np.int32)
    used = B.encode_depth(tiles, masks, 0)[4]
    check_encode(B, R, tiles, masks, 0, want=want, arena_cap=used)
    assert B.encode_depth(tiles, masks, 0, arena_cap=used - 1)[0] == 3


def check_depth_one(B, R):
    """nDepth == 1 is the masked call: bytes and counters"""
    rng = np.random.default_rng(51)
    r, c = 33, 41
    tiles = tiles_of(rng, 5, r, c, 1, np.float32)
    masks = masks_of(rng, 5, r, c)
    c0 = B.counters()
    rc_m, blobs_m, offs_m, sizes_m, used_m = B.encode(tiles[..., 0], masks, 0.01)
    c1 = B.counters()
    rc_d, blobs_d, offs_d, sizes_d, used_d = B.encode_depth(tiles, masks, 0.01)
    c2 = B.counters()
    assert rc_m == 0 and rc_d == 0 and blobs_m == blobs_d and used_m == used_d and offs_m.tolist() == offs_d.tolist()
    assert [c1[k] - c0[k] for k in range(4)] == [c2[k] - c1[k] for k in range(4)]
    rc_m, pix_m, valid_m = B.decode(blobs_m, (r, c), np.float32)
    c3 = B.counters()
    rc_d, pix_d, valid_d = B.decode_depth(blobs_m, (r, c, 1), np.float32)
    c4 = B.counters()
    assert rc_m == 0 and rc_d == 0 and pix_m.tobytes() == pix_d.tobytes() and np.array_equal(valid_m, valid_d)
    assert [c3[k] - c2[k] for k in range(4)] == [c4[k] - c3[k] for k in range(4)]


def check_large(B, R):
    """the large form: tiles beyond the small form's mask bytes, and the mosaics' 256 x 256"""
    rng = np.random.default_rng(61)
    tiles = tiles_of(rng, 2, 513, 513, 2, np.uint16)
    masks = masks_of(rng, 2, 513, 513)
    masks[1][100:200, 50:300] = 0
    want = check_encode(B, R, tiles, masks, 0)
    check_decode(B, R, want, (513, 513, 2), np.uint16)
    tiles = tiles_of(rng, 4, 256, 256, 3, np.float32)
    want = check_encode(B, R, tiles, None, 0.01)
    check_decode(B, R, want, (256, 256, 3), np.float32, want_valid=False)


# ---- the boundary: status rows of the two tile entry points (the raster pair's: raster_depth_common.py) -----------------------
INT_MAX = 2**31 - 1
OK_ENC = dict(tiles=1, dt=3, c=8, r=8, d=2, n=1, e=0.0, arena=1, cap=4096, slot=0, offs=1, sizes=1)
OK_DEC = dict(arena=1, offs=1, sizes=1, n=1, c=8, r=8, d=2, dt=3, out=1)
# (row name, entry point, what differs from a good call, status)
TABLE = [
    ("encode: no tiles", "enc", dict(tiles=0), 2), ("encode: no arena", "enc", dict(arena=0), 2), ("encode: no offsets", "enc", dict(offs=0), 2),
    ("encode: no sizes", "enc", dict(sizes=0), 2), ("encode: nCols 0", "enc", dict(c=0), 2), ("encode: nRows -1", "enc", dict(r=-1), 2),
    ("encode: nTiles 0", "enc", dict(n=0), 2), ("encode: nDepth 0", "enc", dict(d=0), 2), ("encode: nDepth -1", "enc", dict(d=-1), 2),
    ("encode: maxZErr < 0", "enc", dict(e=-1.0), 2), ("encode: slotBytes 24", "enc", dict(slot=24), 2), ("encode: a type that is none", "enc", dict(dt=8), 2),
    ("encode: beyond INT_MAX", "enc", dict(c=65536, r=65536), 6), ("encode: depth beyond INT_MAX", "enc", dict(c=32768, r=32768, d=4), 6),
    ("encode: nDepth 0 beside beyond INT_MAX", "enc", dict(c=65536, r=65536, d=0), 2),
    ("decode: no arena", "dec", dict(arena=0), 2), ("decode: no offsets", "dec", dict(offs=0), 2), ("decode: no sizes", "dec", dict(sizes=0), 2),
    ("decode: no tiles", "dec", dict(out=0), 2), ("decode: nCols 0", "dec", dict(c=0), 2), ("decode: nTiles -3", "dec", dict(n=-3), 2),
    ("decode: nDepth 0", "dec", dict(d=0), 2), ("decode: nDepth -1", "dec", dict(d=-1), 2), ("decode: a type that is none", "dec", dict(dt=9), 2),
    ("decode: beyond INT_MAX", "dec", dict(c=65536, r=65536), 6),
]


def check_boundary(B):
    buf = np.zeros(8192, np.uint8)
    k, p = B.mem.up(buf)
    offs = np.zeros(4, np.uint64)
    sizes = np.zeros(4, np.uint32)
    for name, which, change, status in TABLE:
        if which == "enc":
            a = dict(OK_ENC, **change)
            rc = B.L.lerc_amd_encode_tiles_device_depth(B.h, p if a["tiles"] else None, a["dt"], a["c"], a["r"], a["d"], a["n"], None, a["e"],
                                                        p + 4096 if a["arena"] else None, a["cap"], a["slot"], offs.ctypes.data if a["offs"] else None,
                                                        sizes.ctypes.data if a["sizes"] else None, None)
        else:
            a = dict(OK_DEC, **change)
            rc = B.L.lerc_amd_decode_tiles_device_depth(B.h, p if a["arena"] else None, offs.ctypes.data if a["offs"] else None,
                                                        sizes.ctypes.data if a["sizes"] else None, a["n"], a["c"], a["r"], a["d"], a["dt"],
                                                        p + 4096 if a["out"] else None, None)
        assert rc == status, (name, rc, status)
    assert B.L.lerc_amd_encode_tiles_device_depth(None, p, 3, 8, 8, 2, 1, None, 0.0, p + 4096, 4096, 0, offs.ctypes.data, sizes.ctypes.data, None) == 2
