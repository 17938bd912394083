"""Shared by test_sim_tiles_bands.py (CPU emulator library) and test_gpu_tiles_bands.py (MI355X): a driver for the band stack tile
batch calls of include/lerc_amd_device.h (lerc_amd_encode_tiles_device_bands / lerc_amd_decode_tiles_device_bands), band stacks to
feed them, and the rule for what such a batch may hand back -- the family's rule (tiles_masked_common.must_batch for the wide types,
tiles_bytes_masked_common.must_batch, the 8-bit rule with the mask section's length taken from the blob, for int8 / uint8) asked of
every band blob of a tile.  A band behind band 0 has an empty mask section; both rules read the section's length out of the blob, so
their byte offsets follow by themselves.

Tiles are [nTiles, nBands, nRows, nCols]; masks [nTiles, nRows, nCols] (one mask a tile, nMasks 1), [nTiles, nBands, nRows, nCols]
(nMasks nBands) or None (nMasks 0)."""
import ctypes as ct
import struct

import numpy as np

import capi
import cases
import tiles_bytes_masked_common as BM
import tiles_masked_common as M
from tiles_masked_common import HDR, GpuMem, HostMem, check_layout, fletcher32, random_blob_mask, resign, sub_batches_of, terrain_int    # noqa: F401


def bind(L):
    M.bind(L)
    vp, u64, u32, i = ct.c_void_p, ct.c_ulonglong, ct.c_uint, ct.c_int
    L.lerc_amd_encode_tiles_device_bands.restype = u32
    L.lerc_amd_encode_tiles_device_bands.argtypes = [vp, vp, u32, i, i, i, i, i, vp, ct.c_double, vp, u64, u64, vp, vp, vp]
    L.lerc_amd_decode_tiles_device_bands.restype = u32
    L.lerc_amd_decode_tiles_device_bands.argtypes = [vp, vp, vp, vp, i, i, i, i, u32, vp, i, vp]
    return L


def n_masks_of(tiles, masks):
    return 0 if masks is None else (1 if masks.ndim == 3 else masks.shape[1])


def slot_for(tiles):
    n, nb, r, c = tiles.shape
    return (tiles[0].nbytes + nb * (r * c // 4 + 1024) + 15) & ~15


class BandsBatch(M.Batch):
    """one context of library L, the band stack calls beside the single-band ones of tiles_masked_common.Batch"""

    def __init__(self, L, mem):
        bind(L)
        M.Batch.__init__(self, L, mem)

    def encode_bands(self, tiles, masks, max_z_err, slot_bytes=0, arena_cap=None, arena_shift=0):
        """-> (status, [blob bytes per tile], offsets, sizes, arena bytes used)"""
        n, nb, r, c = tiles.shape
        nm = n_masks_of(tiles, masks)
        kt, pt = self.mem.up(tiles)
        km, pm = self.mem.up(masks) if masks is not None else (None, None)
        cap = int(arena_cap) if arena_cap is not None else (n * slot_bytes if slot_bytes else n * slot_for(tiles))
        ka, pa = self.mem.empty(arena_shift + cap + 16)
        pa += arena_shift
        offs = np.zeros(n, np.uint64)
        sizes = np.zeros(n, np.uint32)
        used = ct.c_ulonglong(0)
        rc = self.L.lerc_amd_encode_tiles_device_bands(self.h, pt, capi.dt_code(tiles.dtype), c, r, nb, n, nm, pm, float(max_z_err), pa, cap,
                                                       int(slot_bytes), offs.ctypes.data, sizes.ctypes.data, ct.byref(used))
        arena = self.mem.down(ka)
        assert arena[:arena_shift].tolist() == [0xCD] * arena_shift, "bytes in front of the arena were written"
        arena = arena[arena_shift:]
        blobs = []
        if rc == 0:
            blobs = [arena[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() for t in range(n)]
            assert arena[cap:].tolist() == [0xCD] * 16, "bytes behind the arena were written"
        return rc, blobs, offs, sizes, int(used.value)

    def decode_bands(self, blobs, shape, dtype, n_masks, sizes=None):
        """blobs laid out at 16-byte aligned offsets -> (status, pixels [n, nb, r, c], valid bytes [n, nMasks, r, c] or None)"""
        n = len(blobs)
        nb, r, c = shape
        offs = np.zeros(n, np.uint64)
        sizes = np.array([len(b) for b in blobs], np.uint32) if sizes is None else np.array(sizes, np.uint32)
        at = 0
        for t, b in enumerate(blobs):
            offs[t] = at
            at += (len(b) + 15) & ~15
        arena = np.zeros(at + 64, np.uint8)
        for t, b in enumerate(blobs):
            arena[int(offs[t]):int(offs[t]) + len(b)] = np.frombuffer(b, np.uint8)
        ka, pa = self.mem.up(arena)
        item = np.dtype(dtype).itemsize
        ko, po = self.mem.empty(n * nb * r * c * item)
        kv, pv = self.mem.empty(n * n_masks * r * c) if n_masks else (None, None)
        rc = self.L.lerc_amd_decode_tiles_device_bands(self.h, pa, offs.ctypes.data, sizes.ctypes.data, n, c, r, nb, capi.dt_code(dtype), po, n_masks, pv)
        pix = self.mem.down(ko, n * nb * r * c * item).view(dtype).reshape(n, nb, r, c)
        valid = self.mem.down(kv, n * n_masks * r * c).reshape(n, n_masks, r, c) if n_masks else None
        return rc, pix, valid

    def encode_stack(self, tile, mask, max_z_err):
        """lerc_amd_encode_device on one band stack -> (status, blob)"""
        nb, r, c = tile.shape
        nm = 0 if mask is None else (1 if mask.ndim == 2 else mask.shape[0])
        kt, pt = self.mem.up(tile)
        km, pm = self.mem.up(mask) if mask is not None else (None, None)
        cap = tile.nbytes + nb * (r * c // 4 + 1024)
        ka, pa = self.mem.empty(cap)
        written = ct.c_uint(0)
        rc = self.L.lerc_amd_encode_device(self.h, pt, capi.dt_code(tile.dtype), 1, c, r, nb, nm, pm, float(max_z_err), pa, cap, ct.byref(written))
        return rc, self.mem.down(ka, written.value).tobytes()

    def decode_stack(self, blob, shape, dtype, n_masks, size=None):
        """lerc_amd_decode_device on one band stack -> (status, pixels [nb, r, c], valid bytes [nMasks, r, c] or None)"""
        nb, r, c = shape
        kb, pb = self.mem.up(np.frombuffer(blob, np.uint8))
        item = np.dtype(dtype).itemsize
        ko, po = self.mem.empty(nb * r * c * item)
        kv, pv = self.mem.empty(n_masks * r * c) if n_masks else (None, None)
        rc = self.L.lerc_amd_decode_device(self.h, pb, len(blob) if size is None else int(size), n_masks, pv, 1, c, r, nb, capi.dt_code(dtype), po)
        pix = self.mem.down(ko, nb * r * c * item).view(dtype).reshape(nb, r, c)
        return rc, pix, (self.mem.down(kv, n_masks * r * c).reshape(n_masks, r, c) if n_masks else None)


# ---- the reference's word --------------------------------------------------------------------------------------------------
def ref_blobs(R, tiles, masks, e):
    out = []
    for t in range(len(tiles)):
        nb = tiles.shape[1]
        rc, blob = R.encode(tiles[t] if nb > 1 else tiles[t, 0], e, n_bands=nb, mask=None if masks is None else masks[t])
        assert rc == 0
        out.append(blob)
    return out


def split_bands(blob):
    """the band blobs of a stack's blob, by the headers' blobSize"""
    out, at = [], 0
    while at < len(blob):
        size = struct.unpack_from("<i", blob, at + 34)[0]
        assert size >= HDR + 4 and at + size <= len(blob)
        out.append(blob[at:at + size])
        at += size
    return out


def band_starts(blob):
    out, at = [], 0
    for b in split_bands(blob):
        out.append(at)
        at += len(b)
    return out


def must_batch(blob, n_pix, item):
    """a tile must stay in the batch's own launches when every band blob of it is a codec 6 blob that satisfies its family's rule"""
    rule = (lambda b: BM.must_batch(b, n_pix)) if item == 1 else (lambda b: M.must_batch(b, n_pix, item))
    return all(struct.unpack_from("<i", b, 6)[0] == 6 and rule(b) for b in split_bands(blob))


def join_bands(bands):
    return b"".join(bands)


# ---- band stacks -----------------------------------------------------------------------------------------------------------
def stacks(rng, n, nb, r, c, dtype):
    """terrain, another one a band; float types get a fractional part"""
    dtype = np.dtype(dtype)
    t = terrain_int(rng, n * nb, r, c, np.int32).reshape(n, nb, r, c)
    if dtype.kind == "f":
        return (t + rng.normal(0, 0.3, t.shape)).astype(dtype)
    if dtype == np.int8:
        return (t - 900).clip(-128, 127).astype(dtype)
    if dtype == np.uint8:
        return (t % 251).astype(dtype)
    return t.astype(dtype)


def three_forms(masks):
    """partly valid tiles, with an all-valid tile and a tile without a valid pixel among them"""
    if len(masks) > 2:
        masks[1][:] = 1
        masks[2][:] = 0
    return masks


def mixed_wide(rng, n, r, c, pads=(0, 1, 2, 3)):
    """float32 stacks of three bands of different kinds: band 0 terrain with a fractional part, band 1 all-integer values (the
    reference flags the band as an integer one), band 2 one bit of noise beside a constant strip, whose low-bit-rate retry ends in 16 x 16 blocks.
    pads: noise columns in band 0, which move the starts of the bands behind it over the residues mod 4"""
    t = np.zeros((n, 3, r, c), np.float32)
    tr = terrain_int(rng, 2 * n, r, c, np.int32)
    for k in range(n):
        t[k, 0] = tr[k] + rng.normal(0, 0.3, (r, c))
        t[k, 0, :, :pads[k % len(pads)] * 3] += rng.normal(0, 40, (r, pads[k % len(pads)] * 3))
        t[k, 1] = tr[n + k]
        t[k, 2] = 5 + (rng.random((r, c)) < 0.5)
        t[k, 2, :, :16 + k % 3] = 5
    return t


def mixed_bytes(rng, n, r, c):
    """uint8 stacks: band 0 smooth (delta Huffman), band 1 noise of seven bits (8 x 8 blocks; eight bits would be one sweep, which the
    8-bit family hands back), band 2 a palette of four values (Huffman)"""
    yy, xx = np.mgrid[0:r, 0:c]
    t = np.zeros((n, 3, r, c), np.uint8)
    for k in range(n):
        t[k, 0] = (100 + 60 * np.sin(yy / (7.0 + k)) * np.cos(xx / 9.0)).astype(np.uint8)
        t[k, 1] = rng.integers(0, 128, (r, c))
        t[k, 2] = np.array([3, 77, 140, 250], np.uint8)[rng.integers(0, 4, (r, c))]
    return t


# ---- checks ----------------------------------------------------------------------------------------------------------------
def check_encode(B, R, tiles, masks, e, slot_bytes=0, want=None, cap_counters=True, arena_shift=0, arena_cap=None):
    """every tile's blob equals the reference's; the layout holds; the counters count tiles and respect the cap -> reference blobs"""
    want = want or ref_blobs(R, tiles, masks, e)
    n, nb, r, c = tiles.shape
    c0 = B.counters()
    rc, blobs, offs, sizes, used = B.encode_bands(tiles, masks, e, slot_bytes=slot_bytes, arena_shift=arena_shift, arena_cap=arena_cap)
    c1 = B.counters()
    assert rc == 0, (rc, B.note())
    for t in range(n):
        assert same_blob(blobs[t], want[t], tiles.itemsize), "tile %d: %d bytes, the reference makes %d (%s)" % (t, len(blobs[t]), len(want[t]), B.note())
    check_layout(offs, sizes, used, slot_bytes)
    batch, single = c1[0] - c0[0], c1[1] - c0[1]
    must = sum(must_batch(w, r * c, tiles.itemsize) for w in want)
    print("encode: %d tiles of %d bands, %d by the batch's launches, %d one by one; the reference's blobs ask for at least %d" % (n, nb, batch, single, must))
    assert batch + single == n
    if cap_counters:
        assert single <= n - must, (single, n - must, B.note())
    return want


def same_blob(got, want, item):
    """byte for byte -- but for the bytes of a lossless float band that the reference itself leaves to chance (heap contents behind every
    Huffman coded byte plane, and the checksum over them: cases.lossless_float_dont_care), which no blob of maxZErr > 0
    and no integer blob has"""
    if got == want or len(got) != len(want):
        return got == want
    a, b = bytearray(got), bytearray(want)
    for k in cases.lossless_float_dont_care(want, item):
        a[k] = b[k] = 0
    return a == b


def check_four_layouts(B, R, tiles, masks, e, cap_counters=True):
    """packed, slotted, at an odd arena address, with an arena of exactly arenaUsed bytes; one byte less: BufferTooSmall"""
    want = check_encode(B, R, tiles, masks, e, cap_counters=cap_counters)
    check_encode(B, R, tiles, masks, e, slot_bytes=slot_for(tiles), want=want, cap_counters=cap_counters)
    check_encode(B, R, tiles, masks, e, want=want, cap_counters=cap_counters, arena_shift=1)
    used = B.encode_bands(tiles, masks, e)[4]
    check_encode(B, R, tiles, masks, e, want=want, cap_counters=cap_counters, arena_cap=used)
    assert B.encode_bands(tiles, masks, e, arena_cap=used - 1)[0] == 3
    return want


def check_decode(B, R, blobs, shape, dtype, n_masks, cap_counters=True):
    """pixels and valid bytes equal the reference's lerc_decode and lerc_amd_decode_device with nBands, tile by tile"""
    nb, r, c = shape
    n, item = len(blobs), np.dtype(dtype).itemsize
    c0 = B.counters()
    rc, pix, valid = B.decode_bands(blobs, shape, dtype, n_masks)
    c1 = B.counters()
    assert rc == 0, (rc, B.note())
    for t in range(n):
        rc_r, p_r, m_r = R.decode(blobs[t], want_masks=n_masks, n_bands=nb)
        assert rc_r == 0
        p_r = p_r.reshape(shape)
        rc_1, p_1, v_1 = B.decode_stack(blobs[t], shape, dtype, n_masks)
        assert rc_1 == 0
        assert np.array_equal(pix[t].view(np.uint8), p_1.view(np.uint8)), "tile %d: pixels differ from lerc_amd_decode_device's" % t
        if n_masks:
            assert np.array_equal(valid[t], m_r), "tile %d: valid bytes differ from the reference's" % t
            assert np.array_equal(valid[t], v_1)
            for k in range(nb):
                m = m_r[k if n_masks > 1 else 0] > 0
                assert np.array_equal(pix[t, k][m].view(np.uint8), p_r[k][m].view(np.uint8)), "tile %d band %d: valid pixels differ from the reference's" % (t, k)
        else:
            assert np.array_equal(pix[t].view(np.uint8), p_r.view(np.uint8))
    batch, single = c1[2] - c0[2], c1[3] - c0[3]
    must = sum(must_batch(b, r * c, item) for b in blobs)
    print("decode: %d tiles of %d bands, %d by the batch's launches, %d one by one; at least %d asked for" % (n, nb, batch, single, must))
    assert batch + single == n
    if cap_counters:
        assert single <= n - must, (single, n - must, B.note())
    return pix, valid


WIDE = [(np.uint16, 0), (np.int32, 0), (np.float32, 0.01), (np.float64, 0.001)]


def check_parity_wide(B, R, dtype, e, nb, with_mask, n=5, r=40, c=56, seed=1):
    rng = np.random.default_rng(seed)
    tiles = stacks(rng, n, nb, r, c, dtype)
    masks = three_forms(random_blob_mask(rng, n, r, c)) if with_mask else None
    want = check_four_layouts(B, R, tiles, masks, e)
    assert sum(must_batch(w, r * c, tiles.itemsize) for w in want) >= n - (1 if with_mask else 0)
    check_decode(B, R, want, (nb, r, c), dtype, 1 if with_mask else 0)


def check_parity_bytes(B, R, dtype, with_mask, n=4, r=40, c=56, seed=2):
    """8-bit stacks: the reference's bytes, and at most one tile handed back"""
    rng = np.random.default_rng(seed)
    tiles = stacks(rng, n, 3, r, c, dtype)
    masks = three_forms(random_blob_mask(rng, n, r, c)) if with_mask else None
    want = check_four_layouts(B, R, tiles, masks, 0)
    assert sum(must_batch(w, r * c, 1) for w in want) >= n - 1
    check_decode(B, R, want, (3, r, c), dtype, 1 if with_mask else 0)


def check_mix_wide(B, R, r=40, c=56):
    rng = np.random.default_rng(5)
    n = 8
    tiles = mixed_wide(rng, n, r, c)
    residues = set()
    for masks in (None, three_forms(random_blob_mask(rng, n, r, c, 0.6, 0.95))):
        want = ref_blobs(R, tiles, masks, 0.01)
        partly = [t for t in range(n) if masks is None or 0 < masks[t].sum() < r * c]
        bands = [split_bands(want[t]) for t in partly]
        assert all(len(b) == 3 for b in bands)
        assert any(b[1][47] == 1 for b in bands), "the reference flags band 1 as an integer band"
        assert any(struct.unpack_from("<i", b[2], 30)[0] == 16 for b in bands), "band 2's low-bit-rate retry ends in 16 x 16 blocks"
        assert any(struct.unpack_from("<i", b[0], 30)[0] == 8 and M.blob_facts(b[0], r * c, 4)["one_sweep"] == 0 for b in bands)
        residues |= set(s % 4 for t in partly for s in band_starts(want[t])[1:])
        check_four_layouts(B, R, tiles, masks, 0.01, cap_counters=False)
        c0 = B.counters()
        check_encode(B, R, tiles, masks, 0.01, want=want, cap_counters=False)
        c1 = B.counters()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (n, 0), ("every kind of band stays in the batch", c0, c1, B.note())
        c0 = B.counters()
        check_decode(B, R, want, (3, r, c), np.float32, 0 if masks is None else 1, cap_counters=False)
        c1 = B.counters()
        assert (c1[2] - c0[2], c1[3] - c0[3]) == (n, 0), (c0, c1, B.note())
    # (every block of an all-valid 40 x 56 band is a full one and its bytes come in pairs: the odd starts are the masked tiles')
    assert residues == {0, 1, 2, 3}, ("bands behind band 0 start at every residue mod 4", residues)


def check_mix_bytes(B, R, r=40, c=56):
    rng = np.random.default_rng(6)
    n = 6
    tiles = mixed_bytes(rng, n, r, c)
    residues = set()
    for masks in (None, three_forms(random_blob_mask(rng, n, r, c))):
        want = check_four_layouts(B, R, tiles, masks, 0)
        assert sum(must_batch(w, r * c, 1) for w in want) >= n - 1
        partly = [t for t in range(n) if masks is None or 0 < masks[t].sum() < r * c]
        kinds = [[BM.facts(b)["mode"] for b in split_bands(want[t])] for t in partly]
        assert any(k[0] == 1 for k in kinds), "band 0 is delta Huffman coded"
        assert any(sorted(k) == [0, 1, 2] for k in kinds), ("delta Huffman, 8 x 8 blocks and Huffman inside one tile", kinds)
        residues |= set(s % 4 for w in want for s in band_starts(w)[1:])
        check_decode(B, R, want, (3, r, c), np.uint8, 0 if masks is None else 1)
    # (an all-valid Huffman band is 98 bytes and whole words: the even starts are the masked tiles')
    assert residues == {0, 1, 2, 3}, ("bands behind band 0 start at every residue mod 4", residues)


def check_sub_batches(B, R, r=40, c=56):
    """7 uint8 tiles in sub-batches of 3 + 3 + 1, packed and slotted; band 1 of tile 4 is constant, which the 8-bit family hands back,
    and the tile goes back whole: the first tile and the arena's base of a later sub-batch, and a redo behind a sub-batch"""
    rng = np.random.default_rng(43)
    n = 7
    tiles = stacks(rng, n, 3, r, c, np.uint8)
    masks = random_blob_mask(rng, n, r, c)
    tiles[4, 1] = 77
    want = ref_blobs(R, tiles, masks, 0)
    assert [must_batch(w, r * c, 1) for w in want] == [t != 4 for t in range(n)]
    assert [BM.must_batch(b, r * c) for b in split_bands(want[4])] == [True, False, True], "band 1 alone sends tile 4 back"
    with sub_batches_of(3):
        for slot in (0, slot_for(tiles)):
            c0 = B.counters()
            check_encode(B, R, tiles, masks, 0, slot, want)
            c1 = B.counters()
            assert (c1[0] - c0[0], c1[1] - c0[1]) == (n - 1, 1), (c0, c1, B.note())
            assert "tile 4" in B.note() and "band 1" in B.note(), B.note()
        c0 = B.counters()
        check_decode(B, R, want, (3, r, c), np.uint8, 1)
        c1 = B.counters()
        assert (c1[2] - c0[2], c1[3] - c0[3]) == (n - 1, 1), (c0, c1, B.note())
        assert "tile 4" in B.note() and "band 1" in B.note(), B.note()


def check_sub_batches_wide(B, R, r=40, c=56):
    """7 tiles in sub-batches of 3 + 3 + 1, packed and slotted; tile 4 has a NaN at a valid pixel of band 1 and is handed back whole:
    the first tile and the arena's base of a later sub-batch, and a redo behind a sub-batch"""
    rng = np.random.default_rng(43)
    n, e = 7, 0.01
    tiles = stacks(rng, n, 3, r, c, np.float32)
    masks = random_blob_mask(rng, n, r, c)
    tiles[4, 1, r // 2, c // 2] = np.nan
    masks[4, r // 2, c // 2] = 1
    want = ref_blobs(R, tiles, masks, e)
    with sub_batches_of(3):
        for slot in (0, slot_for(tiles)):
            c0 = B.counters()
            check_encode(B, R, tiles, masks, e, slot, want, cap_counters=False)
            c1 = B.counters()
            assert (c1[0] - c0[0], c1[1] - c0[1]) == (n - 1, 1), (c0, c1, B.note())
            assert "tile 4" in B.note() and "band 1" in B.note(), B.note()
        # (decode: tile 4's blob replaced by the reference's codec 4 blob of tile 3, which the batch hands back)
        rc, _, _, older = R.encode_for_version(tiles[3], 4, e, n_bands=3, mask=masks[3])
        assert rc == 0 and struct.unpack_from("<i", older, 6)[0] == 4
        c0 = B.counters()
        check_decode(B, R, want[:4] + [older] + want[5:], (3, r, c), np.float32, 1, cap_counters=False)
        c1 = B.counters()
        assert (c1[2] - c0[2], c1[3] - c0[3]) == (n - 1, 1), (c0, c1, B.note())


def check_hand_backs(B, R, r=40, c=56):
    """requests the batch's launches do not take: status 0, the reference's bytes, every tile counted as done one by one"""
    rng = np.random.default_rng(7)
    n = 4

    def one_by_one(tiles, masks, e, n_single=n, decode_masks=None, decode_single=True):
        c0 = B.counters()
        want = check_encode(B, R, tiles, masks, e, cap_counters=False)
        c1 = B.counters()
        assert c1[1] - c0[1] >= n_single, (c0, c1)
        nm = n_masks_of(tiles, masks) if decode_masks is None else decode_masks
        check_decode(B, R, want, tiles.shape[1:], tiles.dtype, nm, cap_counters=False)
        if n_single == n and decode_single:
            assert B.counters()[3] - c1[3] >= n    # (the n of the batch call itself; check_decode's lerc_amd_decode_device calls do not count)
        return want

    f = stacks(rng, n, 3, r, c, np.float32)
    per_band = np.stack([random_blob_mask(rng, 3, r, c) for _ in range(n)])    # [n, 3, r, c], masks that differ per band
    one_by_one(f, per_band, 0.01)
    same = np.repeat(random_blob_mask(rng, n, r, c)[:, None], 3, axis=1).copy()
    one_by_one(f, same, 0.01)
    nan = f.copy()
    m1 = random_blob_mask(rng, n, r, c)
    nan[2, 1, 5, 7] = np.nan
    m1[2, 5, 7] = 1
    one_by_one(nan, m1, 0.01, n_single=1, decode_masks=3)    # (the NaN made band 1's mask another one: a mask a band on the way back)
    one_by_one(stacks(rng, n, 3, r, c, np.uint16), m1, 777, decode_single=False)    # (ordinary blobs: the decoding batch takes them)
    one_by_one(f, m1, 0, decode_single=False)    # (bands the reference wrote raw, one sweep, are the decoding batch's)


def check_errors(B, R, n_fuzz, r=40, c=56, dtype=np.int16):
    rng = np.random.default_rng(11)
    n, nb, shape = 6, 3, (3, r, c)
    tiles = stacks(rng, n, nb, r, c, dtype)
    masks = random_blob_mask(rng, n, r, c)
    want = ref_blobs(R, tiles, masks, 0)
    assert all(must_batch(w, r * c, tiles.itemsize) for w in want)
    rc, good_pix, good_valid = B.decode_bands(want, shape, dtype, 1)
    assert rc == 0
    others = (0, 1, 3, 4, 5)

    def untouched(pix, valid):
        for t in others:
            assert np.array_equal(pix[t], good_pix[t]) and np.array_equal(valid[t], good_valid[t])

    # a slot too small by 16
    small = (max(len(w) for w in want) - 1) & ~15
    assert B.encode_bands(tiles, masks, 0, slot_bytes=small)[0] == 3
    assert B.encode_bands(tiles, masks, 0, slot_bytes=small + 16)[0] == 0
    # one flipped bit in band 1's stream of tile 2: Failed, the whole tile zeroed, the neighbours untouched
    starts = band_starts(want[2])
    bad = bytearray(want[2])
    bad[starts[2] - 9] ^= 0x10
    damaged = list(want)
    damaged[2] = bytes(bad)
    rc, pix, valid = B.decode_bands(damaged, shape, dtype, 1)
    assert rc == 1, rc
    assert not pix[2].any() and not valid[2].any()
    untouched(pix, valid)

    # damage behind a checksum that is right again: status and pixels are the single-blob decoder's
    def same_as_single(blob, size=None):
        damaged = list(want)
        damaged[2] = blob
        sizes = [len(b) for b in damaged]
        if size is not None:
            sizes[2] = size
        rc, pix, valid = B.decode_bands(damaged, shape, dtype, 1, sizes=sizes)
        rc_1, p_1, v_1 = B.decode_stack(blob, shape, dtype, 1, size=size)
        assert rc == rc_1, (rc, rc_1, B.note())
        if rc_1 == 0:
            assert np.array_equal(pix[2], p_1) and np.array_equal(valid[2], v_1)
        else:
            assert not pix[2].any() and not valid[2].any()
        untouched(pix, valid)
        return rc

    bands = split_bands(want[2])

    def with_field(k, at, value):
        b = bytearray(bands[k])
        b[at:at + 4] = struct.pack("<i", value)
        out = list(bands)
        out[k] = resign(bytes(b))
        return join_bands(out)

    nv = struct.unpack_from("<i", bands[1], 26)[0]
    # (the first four, all the GPU runs: band 1's nBlobsMore, blobSize and numValidPixel, band 0's blobSize)
    cases = [with_field(1, 42, 0), with_field(1, 34, len(bands[1]) + 1), with_field(1, 26, nv - 1), with_field(0, 34, len(bands[0]) + 4),
             with_field(1, 42, 2), with_field(1, 34, len(bands[1]) - 1), with_field(1, 26, r * c), with_field(0, 34, len(bands[0]) - 2)]
    for blob in cases[:n_fuzz]:
        same_as_single(blob)
    same_as_single(want[2], size=len(want[2]) - 1)
    # a band behind band 0 that carries a mask section of its own: the reference writes one when the band's mask differs
    per_band = np.repeat(masks[2][None], 3, axis=0).copy()
    per_band[1, r // 2, :] = 0
    per_band[1, 0, :] = 1
    rc_r, own = R.encode(tiles[2], 0, n_bands=3, mask=per_band)
    assert rc_r == 0 and struct.unpack_from("<i", split_bands(own)[1], HDR)[0] > 0
    same_as_single(own)


def check_one_band(B, R, r=40, c=56):
    """nBands == 1: the blobs of the single-band calls, each way"""
    rng = np.random.default_rng(13)
    n = 5
    for dtype, e in ((np.float32, 0.01), (np.uint8, 0), (np.uint16, 0)):
        tiles = stacks(rng, n, 1, r, c, dtype)
        masks = random_blob_mask(rng, n, r, c)
        for m in (masks, None):
            rc_a, blobs_a, _, _, _ = B.encode_bands(tiles, m, e)
            rc_b, blobs_b, _, _, _ = B.encode(tiles[:, 0], m, e, unmasked_call=m is None)
            assert rc_a == 0 and rc_b == 0 and blobs_a == blobs_b
            assert blobs_a == ref_blobs(R, tiles, m, e)
            rc_a, pix_a, valid_a = B.decode_bands(blobs_a, (1, r, c), dtype, 0 if m is None else 1)
            rc_b, pix_b, valid_b = B.decode(blobs_a, (r, c), dtype, want_valid=m is not None)
            assert rc_a == 0 and rc_b == 0 and np.array_equal(pix_a[:, 0].view(np.uint8), pix_b.view(np.uint8))
            if m is not None:
                assert np.array_equal(valid_a[:, 0], valid_b)


def check_soak(L, mem, R, rounds, fresh_rounds, max_tiles, r=40, c=56):
    """band stack batches of random tile count between single-band masked and 8-bit batches on ONE context, then a fresh context a batch"""
    rng = np.random.default_rng(23)

    def one_round(B, k):
        n = int(rng.integers(1, max_tiles + 1))
        dtype, e = (WIDE + [(np.uint8, 0)])[k % 5]
        nb = (2, 3, 4)[k % 3]
        tiles = stacks(rng, n, nb, r, c, dtype)
        masks = random_blob_mask(rng, n, r, c, 0.02, 1.0) if k % 3 else None
        want = check_encode(B, R, tiles, masks, e, slot_bytes=0 if k % 2 == 0 else slot_for(tiles))
        check_decode(B, R, want, (nb, r, c), dtype, 0 if masks is None else 1)
        # a single-band masked batch and an 8-bit batch in between
        m1 = random_blob_mask(rng, 3, r, c)
        w1 = M.check_encode(B, R, np.ascontiguousarray(tiles[:3, 0]) if n >= 3 else stacks(rng, 3, 1, r, c, dtype)[:, 0].copy(), m1, e, cap_counters=False)
        assert len(w1) == 3
        t8 = stacks(rng, 3, 1, r, c, np.uint8)[:, 0].copy()
        rc, blobs, _, _, _ = B.encode(t8, None, 0, unmasked_call=True)
        assert rc == 0 and blobs == M.ref_blobs(R, t8, None, 0)

    B = BandsBatch(L, mem)
    try:
        for k in range(rounds):
            one_round(B, k)
    finally:
        B.close()
    for k in range(fresh_rounds):
        B = BandsBatch(L, mem)
        try:
            one_round(B, k)
        finally:
            B.close()
