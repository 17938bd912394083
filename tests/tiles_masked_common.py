"""Shared by test_sim_tiles_masked.py (CPU emulator library) and test_gpu_tiles_masked.py (MI355X): drivers for the masked tile
batch calls of include/lerc_amd_device.h, the "island" mosaic, and the rule for what a batch may hand back.

Memory: the emulator's "device" pointers are host pointers (numpy), the product's are HIP allocations (torch uint8 tensors).
"""
import contextlib
import ctypes as ct
import os
import struct

import numpy as np

import capi

HDR = 90    # bytes of a codec 6 header


def bind(L):
    vp, u64, u32 = ct.c_void_p, ct.c_ulonglong, ct.c_uint
    L.lerc_amd_create.restype = vp
    L.lerc_amd_create.argtypes = [vp]
    L.lerc_amd_destroy.argtypes = [vp]
    L.lerc_amd_last_note.argtypes = [vp]
    L.lerc_amd_last_note.restype = ct.c_char_p
    L.lerc_amd_encode_tiles_device_masked.restype = u32
    L.lerc_amd_encode_tiles_device_masked.argtypes = [vp, vp, u32, ct.c_int, ct.c_int, ct.c_int, vp, ct.c_double, vp, u64, u64, vp, vp, vp]
    L.lerc_amd_decode_tiles_device_masked.restype = u32
    L.lerc_amd_decode_tiles_device_masked.argtypes = [vp, vp, vp, vp, ct.c_int, ct.c_int, ct.c_int, u32, vp, vp]
    L.lerc_amd_tile_batch_counters.restype = None
    L.lerc_amd_tile_batch_counters.argtypes = [vp, ct.POINTER(u64)]
    L.lerc_amd_encode_tiles_device.restype = u32
    L.lerc_amd_encode_tiles_device.argtypes = [vp, vp, u32, ct.c_int, ct.c_int, ct.c_int, ct.c_double, vp, u64, vp, vp, vp]
    L.lerc_amd_decode_tiles_device.restype = u32
    L.lerc_amd_decode_tiles_device.argtypes = [vp, vp, vp, vp, ct.c_int, ct.c_int, ct.c_int, u32, vp]
    L.lerc_amd_encode_device.restype = u32
    L.lerc_amd_encode_device.argtypes = [vp, vp, u32, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, vp, ct.c_double, vp, u32, vp]
    L.lerc_amd_decode_device.restype = u32
    L.lerc_amd_decode_device.argtypes = [vp, vp, u32, ct.c_int, vp, ct.c_int, ct.c_int, ct.c_int, ct.c_int, u32, vp]
    return L


@contextlib.contextmanager
def sub_batches_of(n):
    """LERC_AMD_TEST_TILE_SUBBATCH=n around the calls inside (the library reads it per call), then as it was"""
    old = os.environ.get("LERC_AMD_TEST_TILE_SUBBATCH")
    os.environ["LERC_AMD_TEST_TILE_SUBBATCH"] = str(n)
    try:
        yield
    finally:
        if old is None:
            del os.environ["LERC_AMD_TEST_TILE_SUBBATCH"]
        else:
            os.environ["LERC_AMD_TEST_TILE_SUBBATCH"] = old


class HostMem:
    """the emulator: device memory is host memory"""

    def up(self, a):
        a = np.ascontiguousarray(a)
        raw = np.zeros(a.nbytes + 64, np.uint8)
        shift = (-raw.ctypes.data) % 64
        buf = raw[shift:shift + a.nbytes]
        buf[:] = a.view(np.uint8).ravel()
        buf_keep = (raw, buf)
        return buf_keep, buf.ctypes.data

    def empty(self, nbytes, fill=0xCD):
        return self.up(np.full(max(int(nbytes), 1), fill, np.uint8))

    def down(self, keep, nbytes=None):
        buf = keep[1]
        return np.array(buf if nbytes is None else buf[:nbytes], copy=True)

    def sync(self):
        pass


class GpuMem:
    def __init__(self):
        import torch
        self.torch = torch
        assert torch.cuda.is_available(), "gpu tests need a GPU"

    def up(self, a):
        a = np.ascontiguousarray(a)
        t = self.torch.from_numpy(a.view(np.uint8).ravel().copy()).cuda()
        self.torch.cuda.synchronize()
        return t, t.data_ptr()

    def empty(self, nbytes, fill=0xCD):
        t = self.torch.full((max(int(nbytes), 1),), fill, dtype=self.torch.uint8, device="cuda")
        self.torch.cuda.synchronize()
        return t, t.data_ptr()

    def down(self, keep, nbytes=None):
        self.torch.cuda.synchronize()
        t = keep if nbytes is None else keep[:nbytes]
        return t.cpu().numpy().copy()

    def sync(self):
        self.torch.cuda.synchronize()


class Batch:
    """one context of library L (bound), memory through `mem`"""

    def __init__(self, L, mem):
        self.L, self.mem = bind(L), mem
        self.h = L.lerc_amd_create(None)
        assert self.h

    def close(self):
        if self.h:
            self.L.lerc_amd_destroy(self.h)
            self.h = None

    def counters(self):
        out = (ct.c_ulonglong * 4)()
        self.L.lerc_amd_tile_batch_counters(self.h, out)
        return [int(v) for v in out]

    def note(self):
        return self.L.lerc_amd_last_note(self.h).decode()

    def encode(self, tiles, masks, max_z_err, slot_bytes=0, arena_cap=None, unmasked_call=False, arena_shift=0):
        """-> (status, [blob bytes per tile], offsets, sizes, arena bytes used); arena_shift: the arena begins that many bytes behind
        an aligned address"""
        n, r, c = tiles.shape
        kt, pt = self.mem.up(tiles)
        km, pm = self.mem.up(masks) if masks is not None else (None, None)
        cap = int(arena_cap) if arena_cap is not None else (n * slot_bytes if slot_bytes else n * (tiles[0].nbytes + r * c // 4 + 1024))
        ka, pa = self.mem.empty(arena_shift + cap + 16)
        pa += arena_shift
        offs = np.zeros(n, np.uint64)
        sizes = np.zeros(n, np.uint32)
        used = ct.c_ulonglong(0)
        if unmasked_call:
            rc = self.L.lerc_amd_encode_tiles_device(self.h, pt, capi.dt_code(tiles.dtype), c, r, n, float(max_z_err), pa, cap,
                                                     offs.ctypes.data, sizes.ctypes.data, ct.byref(used))
        else:
            rc = self.L.lerc_amd_encode_tiles_device_masked(self.h, pt, capi.dt_code(tiles.dtype), c, r, n, pm, float(max_z_err), pa, cap,
                                                            int(slot_bytes), offs.ctypes.data, sizes.ctypes.data, ct.byref(used))
        arena = self.mem.down(ka)
        assert arena[:arena_shift].tolist() == [0xCD] * arena_shift, "bytes in front of the arena were written"
        arena = arena[arena_shift:]
        blobs = []
        if rc == 0:
            blobs = [arena[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() for t in range(n)]
            assert arena[cap:].tolist() == [0xCD] * 16, "bytes behind the arena were written"
        return rc, blobs, offs, sizes, int(used.value)

    def decode(self, blobs, shape, dtype, want_valid=True):
        """blobs laid out at 16-byte aligned offsets -> (status, pixels [n, r, c], valid bytes [n, r, c] or None)"""
        n = len(blobs)
        r, c = shape
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
        ko, po = self.mem.empty(n * r * c * item)
        kv, pv = self.mem.empty(n * r * c) if want_valid else (None, None)
        rc = self.L.lerc_amd_decode_tiles_device_masked(self.h, pa, offs.ctypes.data, sizes.ctypes.data, n, c, r, capi.dt_code(dtype), po, pv)
        pix = self.mem.down(ko, n * r * c * item).view(dtype).reshape(n, r, c)
        valid = self.mem.down(kv, n * r * c).reshape(n, r, c) if want_valid else None
        return rc, pix, valid

    def encode_one(self, tile, mask, max_z_err):
        """lerc_amd_encode_device with nMasks = 1 -> (status, blob)"""
        r, c = tile.shape
        kt, pt = self.mem.up(tile)
        km, pm = self.mem.up(mask)
        cap = tile.nbytes + r * c // 4 + 1024
        ka, pa = self.mem.empty(cap)
        written = ct.c_uint(0)
        rc = self.L.lerc_amd_encode_device(self.h, pt, capi.dt_code(tile.dtype), 1, c, r, 1, 1, pm, float(max_z_err), pa, cap, ct.byref(written))
        return rc, self.mem.down(ka, written.value).tobytes()

    def decode_one(self, blob, shape, dtype):
        """lerc_amd_decode_device with nMasks = 1 -> (status, pixels, valid bytes)"""
        r, c = shape
        kb, pb = self.mem.up(np.frombuffer(blob, np.uint8))
        item = np.dtype(dtype).itemsize
        ko, po = self.mem.empty(r * c * item)
        kv, pv = self.mem.empty(r * c)
        rc = self.L.lerc_amd_decode_device(self.h, pb, len(blob), 1, pv, 1, c, r, 1, capi.dt_code(dtype), po)
        return rc, self.mem.down(ko, r * c * item).view(dtype).reshape(r, c), self.mem.down(kv, r * c).reshape(r, c)


# ---- what the reference's blob says about how it coded a tile -------------------------------------------------------
def blob_facts(blob, n_pix, item):
    """-> dict(num_valid, mb, blob_size, rle, one_sweep, n_bytes_tiling) of a single-band codec 6 blob"""
    num_valid, mb, blob_size = struct.unpack_from("<i", blob, 26)[0], struct.unpack_from("<i", blob, 30)[0], struct.unpack_from("<i", blob, 34)[0]
    z_min, z_max = struct.unpack_from("<dd", blob, 58)
    rle = struct.unpack_from("<i", blob, HDR)[0]
    f = dict(num_valid=num_valid, mb=mb, blob_size=blob_size, rle=rle, one_sweep=None, n_bytes_tiling=None, const=z_min == z_max)
    if num_valid > 0 and z_min != z_max:
        at = HDR + 4 + rle + 2 * item
        f["one_sweep"] = blob[at]
        f["n_bytes_tiling"] = blob_size - (at + 1)
    return f


def must_batch(blob, n_pix, item):
    """ISSUE: among tiles with valid pixels, the batch's own launches must take a tile when its reference blob has 8 x 8 blocks, is not
    one sweep, and the low-bit-rate retry condition does not hold"""
    f = blob_facts(blob, n_pix, item)
    if f["num_valid"] <= 0 or f["const"] or f["mb"] != 8 or f["one_sweep"] != 0:
        return False
    nbt = f["n_bytes_tiling"]
    retry = nbt * 8 < n_pix * 1.5 and nbt < 4 * f["num_valid"] * item
    return not retry


# ---- the island mosaic (lerc_amd/synth.py) ----------------------------------------------------------------------------
def island(kind, size=4096, tile=256):
    from lerc_amd import synth
    return synth.island(kind, size, tile)


def random_blob_mask(rng, n, r, c, lo=0.3, hi=0.9):
    """smooth random blobs, lo .. hi valid"""
    out = np.zeros((n, r, c), np.uint8)
    yy, xx = np.mgrid[0:r, 0:c]
    for t in range(n):
        f = np.zeros((r, c))
        for _ in range(6):
            cy, cx, s = rng.uniform(0, r), rng.uniform(0, c), rng.uniform(0.08, 0.4) * max(r, c)
            f += rng.uniform(0.5, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
        want = rng.uniform(lo, hi)
        out[t] = (f >= np.quantile(f, 1.0 - want)).astype(np.uint8)
    return out


# ---- checks shared by the emulator and the GPU suite ------------------------------------------------------------------
def fletcher32(data):
    """Fletcher32 over big-endian 16-bit words as Lerc2 computes it (Lerc2.cpp:1037-1064), in closed form"""
    b = np.frombuffer(data, np.uint8).astype(np.uint64)
    p = np.arange(len(b), dtype=np.uint64)
    c = b << np.where(p % 2 == 0, 8, 0).astype(np.uint64)
    a_sum = int(c.sum()) % 65535
    b_sum = int(((p // 2) * c).sum() % 65535)
    n = (len(b) + 1) // 2
    s1 = a_sum or 0xFFFF
    s2 = ((n % 65535) * a_sum + 65535 - b_sum) % 65535 or 0xFFFF
    return (s2 << 16) | s1


def resign(blob):
    """the blob with its checksum recomputed (so that damage reaches the parsers behind the checksum test)"""
    b = bytearray(blob)
    b[10:14] = struct.pack("<I", fletcher32(bytes(b[14:])))
    return bytes(b)


def ref_blobs(R, tiles, masks, e):
    out = []
    for t in range(len(tiles)):
        rc, blob = R.encode(tiles[t], e, mask=None if masks is None else masks[t])
        assert rc == 0
        out.append(blob)
    return out


def check_layout(offs, sizes, used, slot_bytes=0):
    n = len(offs)
    assert all(int(o) % 16 == 0 for o in offs), "offsets are 16-byte aligned"
    spans = sorted((int(offs[t]), int(offs[t]) + int(sizes[t])) for t in range(n))
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, "two blobs overlap"
    assert used >= spans[-1][1], "arenaUsed covers all blobs"
    if slot_bytes:
        assert [int(o) for o in offs] == [t * slot_bytes for t in range(n)]


def check_encode(B, R, tiles, masks, e, slot_bytes=0, want=None, cap_counters=True):
    """every blob equals the reference's; counters respect the cap computed from the reference's blobs -> reference blobs"""
    want = want or ref_blobs(R, tiles, masks, e)
    n, n_pix, item = len(tiles), tiles[0].size, tiles.itemsize
    c0 = B.counters()
    rc, blobs, offs, sizes, used = B.encode(tiles, masks, e, slot_bytes=slot_bytes)
    c1 = B.counters()
    assert rc == 0, (rc, B.note())
    for t in range(n):
        assert blobs[t] == want[t], "tile %d: %d bytes, the reference makes %d (%s)" % (t, len(blobs[t]), len(want[t]), B.note())
    check_layout(offs, sizes, used, slot_bytes)
    batch, single = c1[0] - c0[0], c1[1] - c0[1]
    must = sum(must_batch(w, n_pix, item) for w in want)
    print("encode: %d tiles, %d by the batch's launches, %d one by one; the reference's blobs ask for at least %d in the batch" % (n, batch, single, must))
    assert batch + single == n
    if cap_counters:
        assert single <= n - must, (single, n - must, B.note())
    return want


def check_decode(B, R, blobs, shape, dtype, n_pix_must=True):
    """pixels and valid bytes equal the reference's lerc_decode and lerc_amd_decode_device with nMasks = 1, tile by tile"""
    n, item = len(blobs), np.dtype(dtype).itemsize
    c0 = B.counters()
    rc, pix, valid = B.decode(blobs, shape, dtype)
    c1 = B.counters()
    assert rc == 0, (rc, B.note())
    for t in range(n):
        rc_r, p_r, m_r = R.decode(blobs[t], want_masks=1)
        assert rc_r == 0
        m_r = m_r[0]
        assert np.array_equal(valid[t], m_r), "tile %d: valid bytes differ from the reference's" % t
        p_r = p_r.reshape(shape)
        assert np.array_equal(pix[t][m_r > 0].view(np.uint8), p_r[m_r > 0].view(np.uint8)), "tile %d: valid pixels differ from the reference's" % t
        rc_1, p_1, v_1 = B.decode_one(blobs[t], shape, dtype)
        assert rc_1 == 0
        assert np.array_equal(pix[t].view(np.uint8), p_1.view(np.uint8)), "tile %d: pixels differ from lerc_amd_decode_device's" % t
        assert np.array_equal(valid[t], v_1)
    batch, single = c1[2] - c0[2], c1[3] - c0[3]
    must = sum(must_batch(b, shape[0] * shape[1], item) for b in blobs)
    print("decode: %d tiles, %d by the batch's launches, %d one by one; at least %d asked for" % (n, batch, single, must))
    assert batch + single == n
    assert single <= n - must, (single, n - must, B.note())
    return pix, valid


def terrain_int(rng, n, r, c, dtype):
    yy, xx = np.mgrid[0:r, 0:c]
    out = np.zeros((n, r, c), dtype)
    for t in range(n):
        f = 900 + 400 * np.sin(yy / rng.uniform(9, 40)) * np.cos(xx / rng.uniform(9, 40)) + rng.normal(0, rng.uniform(0.5, 6), (r, c))
        out[t] = np.round(f).astype(dtype)
    return out


def check_ragged(B, R, n, r, c, dtype, seed):
    rng = np.random.default_rng(seed)
    tiles = terrain_int(rng, n, r, c, dtype)
    masks = random_blob_mask(rng, n, r, c)
    want = ref_blobs(R, tiles, masks, 0)
    parities = set(blob_facts(w, r * c, tiles.itemsize)["rle"] % 2 for w in want if blob_facts(w, r * c, tiles.itemsize)["rle"] > 0)
    assert parities == {0, 1}, "both parities of the mask section's length occur"
    for slot in (0, (tiles[0].nbytes + r * c // 4 + 1024 + 15) & ~15):
        check_encode(B, R, tiles, masks, 0, slot, want)
    check_decode(B, R, want, (r, c), dtype)


def check_fallbacks(B, R, r=40, c=56):
    rng = np.random.default_rng(7)
    # a uint8 batch
    t8 = terrain_int(rng, 5, r, c, np.int32).astype(np.uint8)
    m8 = random_blob_mask(rng, 5, r, c)
    w8 = check_encode(B, R, t8, m8, 0, cap_counters=False)
    check_decode_plain(B, R, w8, (r, c), np.uint8)
    # a NaN tile, a constant tile, a tile whose only valid pixels are one row -- among ordinary ones
    tf = (terrain_int(rng, 6, r, c, np.int32) + rng.normal(0, 0.3, (6, r, c))).astype(np.float32)
    mf = random_blob_mask(rng, 6, r, c)
    tf[1, r // 2, c // 2] = np.nan
    mf[1, r // 2, c // 2] = 1
    tf[2][:] = 42.5
    mf[3][:] = 0
    mf[3][r // 3, :] = 1
    wf = check_encode(B, R, tf, mf, 0.01, cap_counters=False)
    check_decode_plain(B, R, wf, (r, c), np.float32)
    # maxZErr = 777 (the bit plane mode's switch)
    ti = terrain_int(rng, 4, r, c, np.uint16)
    mi = random_blob_mask(rng, 4, r, c)
    wi = check_encode(B, R, ti, mi, 777, cap_counters=False)
    check_decode_plain(B, R, wi, (r, c), np.uint16)
    # dValidBytes == NULL: the existing unmasked call's blobs
    rc_a, blobs_a, _, _, _ = B.encode(tf[4:], None, 0.01)
    rc_b, blobs_b, _, _, _ = B.encode(tf[4:], None, 0.01, unmasked_call=True)
    assert rc_a == 0 and rc_b == 0 and blobs_a == blobs_b
    assert blobs_a == ref_blobs(R, tf[4:], None, 0.01)


def check_decode_plain(B, R, blobs, shape, dtype):
    rc, pix, valid = B.decode(blobs, shape, dtype)
    assert rc == 0, (rc, B.note())
    for t in range(len(blobs)):
        rc_1, p_1, v_1 = B.decode_one(blobs[t], shape, dtype)
        rc_r, p_r, m_r = R.decode(blobs[t], want_masks=1)
        assert rc_1 == 0 and rc_r == 0
        assert np.array_equal(pix[t].view(np.uint8), p_1.view(np.uint8)) and np.array_equal(valid[t], v_1) and np.array_equal(valid[t], m_r[0])
        assert np.array_equal(pix[t][valid[t] > 0].view(np.uint8), p_r.reshape(shape)[valid[t] > 0].view(np.uint8))


def check_errors(B, R, r=40, c=56, n_fuzz=8):
    rng = np.random.default_rng(11)
    n = 6
    tiles = terrain_int(rng, n, r, c, np.int16)
    masks = random_blob_mask(rng, n, r, c)
    want = ref_blobs(R, tiles, masks, 0)
    rc, blobs, offs, sizes, used = B.encode(tiles, masks, 0)
    assert rc == 0 and blobs == want
    # an arena one byte too small, a slot too small
    assert B.encode(tiles, masks, 0, arena_cap=used - 1)[0] == 3
    assert B.encode(tiles, masks, 0, arena_cap=used)[0] == 0
    small = (max(len(w) for w in want) - 1) & ~15
    assert B.encode(tiles, masks, 0, slot_bytes=small)[0] == 3
    assert B.encode(tiles, masks, 0, slot_bytes=small + 16)[0] == 0
    # dValidBytes == NULL with a masked blob present: what lerc_amd_decode_tiles_device says today
    assert B.decode(want, (r, c), np.int16, want_valid=False)[0] == 2
    # one flipped bit: Failed(1) and zeros for that tile, the neighbours untouched
    rc, good_pix, good_valid = B.decode(want, (r, c), np.int16)
    assert rc == 0
    f = blob_facts(want[2], r * c, 2)
    assert f["rle"] > 4 and must_batch(want[2], r * c, 2)
    for where in (HDR + 4 + 1, len(want[2]) - 9):    # the run-length stream, the block stream
        bad = bytearray(want[2])
        bad[where] ^= 0x10
        damaged = list(want)
        damaged[2] = bytes(bad)
        rc, pix, valid = B.decode(damaged, (r, c), np.int16)
        assert rc == 1, rc
        assert not pix[2].any() and not valid[2].any()
        for t in (0, 1, 3, 4, 5):
            assert np.array_equal(pix[t], good_pix[t]) and np.array_equal(valid[t], good_valid[t])
    # damage behind a checksum that is right again: a status and the single-blob decoder's result, never anything else
    for k in range(n_fuzz):
        bad = bytearray(want[2])
        where = int(rng.integers(HDR + 4, len(bad)))
        bad[where] ^= 1 << int(rng.integers(0, 8))
        damaged = list(want)
        damaged[2] = resign(bytes(bad))
        rc, pix, valid = B.decode(damaged, (r, c), np.int16)
        rc_1, p_1, v_1 = B.decode_one(damaged[2], (r, c), np.int16)
        assert rc == rc_1, (k, where, rc, rc_1)
        if rc_1 == 0:
            assert np.array_equal(pix[2], p_1) and np.array_equal(valid[2], v_1)
        else:
            assert not pix[2].any() and not valid[2].any()
        for t in (0, 1, 3, 4, 5):
            assert np.array_equal(pix[t], good_pix[t]) and np.array_equal(valid[t], good_valid[t])


def check_soak(L, mem, R, rounds, max_tiles, r, c):
    """batches of random size and random masks on ONE context, between unmasked batches and single-band masked calls"""
    rng = np.random.default_rng(23)
    B = Batch(L, mem)
    try:
        for k in range(rounds):
            n = int(rng.integers(1, max_tiles + 1))
            dtype = (np.float32, np.uint16, np.int32)[k % 3]
            e = 0.01 if dtype == np.float32 else 0
            tiles = terrain_int(rng, n, r, c, np.int32)
            tiles = (tiles + rng.normal(0, 0.3, tiles.shape)).astype(np.float32) if dtype == np.float32 else tiles.astype(dtype)
            masks = random_blob_mask(rng, n, r, c, 0.02, 1.0)
            if n > 2:
                masks[int(rng.integers(0, n))][:] = 1    # an all-valid tile among them
            want = check_encode(B, R, tiles, masks, e, slot_bytes=0 if k % 2 == 0 else (tiles[0].nbytes + r * c // 4 + 1024 + 15) & ~15, cap_counters=False)
            rc, pix, valid = B.decode(want, (r, c), dtype)
            assert rc == 0
            for t in range(n):
                assert np.array_equal(valid[t], (masks[t] > 0).astype(np.uint8))
                rc_r, p_r, _ = R.decode(want[t], want_masks=1)
                assert np.array_equal(pix[t][valid[t] > 0].view(np.uint8), p_r.reshape(r, c)[valid[t] > 0].view(np.uint8))
            # an unmasked batch and a single-band masked call in between
            rc_u, blobs_u, _, _, _ = B.encode(tiles[:2], None, e, unmasked_call=True)
            assert rc_u == 0 and blobs_u == ref_blobs(R, tiles[:2], None, e)
            rc_1, blob_1 = B.encode_one(tiles[0], masks[0], e)
            assert rc_1 == 0 and blob_1 == want[0]
    finally:
        B.close()


def check_float_decisions(B, R, r=40, c=56):
    """float tiles whose statistics change the error bound stay in the batch's launches: values that are all integers (isInt in the
    header, bound 0.5) and values that agree with a larger bound (TryRaiseMaxZError) -- capped like every other batch"""
    rng = np.random.default_rng(31)
    n = 8
    masks = random_blob_mask(rng, n, r, c)
    masks[5][:] = 1
    ints = terrain_int(rng, n, r, c, np.int32).astype(np.float32)
    ints[6] += 20000000.0    # beyond 2^23: "all integers" no longer holds for the tile, the candidates are tried instead
    for e in (0.01, 0.3, 2.0):
        want = check_encode(B, R, ints, masks, e)
        check_encode(B, R, ints, masks, e, slot_bytes=(ints[0].nbytes + r * c // 4 + 1024 + 15) & ~15, want=want)
        assert sum(must_batch(w, r * c, 4) for w in want) >= n - 2
        assert any(w[47] == 1 for w in want), "the reference flags the tiles as integer ones"
        check_decode(B, R, want, (r, c), np.float32)
    tenths = (terrain_int(rng, n, r, c, np.int32) / 10.0).astype(np.float32)          # multiples of 0.1: the bound rises to 0.05
    halves = (terrain_int(rng, n, r, c, np.int32) / 2.0).astype(np.float32)           # multiples of 0.5: to 0.25
    mixed = tenths.copy()
    mixed[::2] = (terrain_int(rng, n, r, c, np.int32) + rng.normal(0, 0.3, (n, r, c))).astype(np.float32)[::2]    # every other tile: nothing to raise
    for tiles, e in ((tenths, 0.01), (halves, 0.01), (mixed, 0.001), (tenths.astype(np.float64), 0.01)):
        want = check_encode(B, R, tiles, masks, e)
        raised = [struct.unpack_from("<d", w, 50)[0] for w in want]
        assert any(x > e for x in raised), "the reference raises the error bound of some tile"
        check_decode(B, R, want, (r, c), tiles.dtype)


def check_unaligned_arena(B, R, r=40, c=56):
    """an arena that begins at an odd address: still the batch's launches, the same blobs at 16-byte aligned OFFSETS"""
    rng = np.random.default_rng(37)
    tiles = terrain_int(rng, 6, r, c, np.uint16)
    masks = random_blob_mask(rng, 6, r, c)
    want = ref_blobs(R, tiles, masks, 0)
    for shift in (1, 6):
        c0 = B.counters()
        rc, blobs, offs, sizes, used = B.encode(tiles, masks, 0, arena_shift=shift)
        c1 = B.counters()
        assert rc == 0 and blobs == want
        check_layout(offs, sizes, used)
        assert c1[1] - c0[1] <= len(tiles) - sum(must_batch(w, r * c, 2) for w in want)


def check_fresh_contexts(L, mem, R, rounds, n, r, c):
    """create a context, run ONE masked batch each way on it, destroy it -- a few times over"""
    rng = np.random.default_rng(41)
    for k in range(rounds):
        dtype = (np.float32, np.int16)[k % 2]
        e = 0.01 if dtype == np.float32 else 0
        tiles = terrain_int(rng, n, r, c, np.int32)
        tiles = (tiles + rng.normal(0, 0.3, tiles.shape)).astype(np.float32) if dtype == np.float32 else tiles.astype(dtype)
        masks = random_blob_mask(rng, n, r, c)
        B = Batch(L, mem)
        try:
            want = check_encode(B, R, tiles, masks, e, slot_bytes=0 if k % 2 else (tiles[0].nbytes + r * c // 4 + 1024 + 15) & ~15)
        finally:
            B.close()
        B = Batch(L, mem)
        try:
            check_decode(B, R, want, (r, c), dtype)
        finally:
            B.close()


def check_sub_batches(B, R, r=40, c=56):
    """7 tiles in sub-batches of 3 + 3 + 1 (LERC_AMD_TEST_TILE_SUBBATCH), packed and slotted: the first tile and the arena's base of a
    LATER sub-batch, and a tile done again behind one.  Tile 4, in the second sub-batch, has a NaN at a valid pixel: the encoding batch
    hands it back.  Its blob is an ordinary one (the reference makes the pixel invalid), which the decoding batch must take; so the
    blobs are decoded a second time with tile 4's replaced by the reference's lossless blob (maxZErr 0 on float values), which the
    decoding batch hands back."""
    rng = np.random.default_rng(43)
    n, e = 7, 0.01
    tiles = (terrain_int(rng, n, r, c, np.int32) + rng.normal(0, 0.3, (n, r, c))).astype(np.float32)
    masks = random_blob_mask(rng, n, r, c)
    tiles[4, r // 2, c // 2] = np.nan
    masks[4, r // 2, c // 2] = 1
    want = ref_blobs(R, tiles, masks, e)
    with sub_batches_of(3):
        for slot in (0, (tiles[0].nbytes + r * c // 4 + 1024 + 15) & ~15):
            c0 = B.counters()
            check_encode(B, R, tiles, masks, e, slot, want, cap_counters=False)
            c1 = B.counters()
            assert (c1[0] - c0[0], c1[1] - c0[1]) == (n - 1, 1), (c0, c1, B.note())
        c0 = B.counters()
        check_decode(B, R, want, (r, c), np.float32)
        c1 = B.counters()
        assert (c1[2] - c0[2], c1[3] - c0[3]) == (n, 0), (c0, c1, B.note())
        rc, lossless = R.encode(tiles[3], 0, mask=masks[3])
        assert rc == 0
        blobs = want[:4] + [lossless] + want[5:]
        check_decode_plain(B, R, blobs, (r, c), np.float32)
        c2 = B.counters()
        assert (c2[2] - c1[2], c2[3] - c1[3]) == (n - 1, 1), (c1, c2, B.note())
