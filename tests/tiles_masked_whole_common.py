"""Shared by test_sim_tiles_masked_whole.py (CPU emulator library) and test_gpu_tiles_masked_whole.py (MI355X): masked tile batches
whose empty, constant, one-sweep and 16 x 16 tiles stay inside the batch's launches.

The rule for what may leave is a condition on the INPUTS: in a batch, the number of tiles done one by one equals the number of tiles
with a NaN at a valid pixel.  A blob never holds a NaN at a valid pixel (the encoder takes such pixels out of the mask), so for a
decode that number is 0.  Every expected byte and pixel is the reference's; what kind of blob a tile makes is read from the
reference's blob (tiles_masked_common.blob_facts), never from the product's flags.
"""
import struct

import numpy as np

import tiles_masked_common as C

HDR = C.HDR
TYPES = (np.int16, np.uint16, np.int32, np.uint32, np.float32, np.float64)


def n_nan_tiles(tiles, masks):
    if tiles.dtype.kind != "f":
        return 0
    return int(sum(bool(np.isnan(tiles[t][masks[t] > 0]).any()) for t in range(len(tiles))))


def kind_of(blob, n_pix, item):
    """'empty' | 'const' | 'sweep' | 'mb16' | 'mb8retry' (8 x 8 blocks although the low-bit-rate rule tried 16 x 16) | 'mb8'"""
    f = C.blob_facts(blob, n_pix, item)
    if f["num_valid"] == 0:
        return "empty"
    if f["const"]:
        return "const"
    if f["one_sweep"]:
        return "sweep"
    if f["mb"] == 16:
        return "mb16"
    nbt = f["n_bytes_tiling"]
    return "mb8retry" if (nbt * 8 < n_pix * 1.5 and nbt < 4 * f["num_valid"] * item) else "mb8"


def max_z_err_of(blob):
    return struct.unpack_from("<d", blob, 50)[0]


def err_for(dtype):
    return 0.01 if np.dtype(dtype).kind == "f" else 0


def full_range_noise(rng, r, c, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return (rng.uniform(-1, 1, (r, c)) * (1e30 if dtype == np.float32 else 1e200)).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, (r, c), dtype=np.int64, endpoint=True).astype(dtype)


def smooth(rng, r, c, dtype, noise):
    yy, xx = np.mgrid[0:r, 0:c]
    f = 900 + 400 * np.sin(yy / rng.uniform(9, 40)) * np.cos(xx / rng.uniform(9, 40)) + rng.normal(0, noise, (r, c))
    return f.astype(dtype) if np.dtype(dtype).kind == "f" else np.round(f).astype(dtype)


def kinds_mosaic(dtype, r, c, seed=5):
    """-> (tiles, masks, MaxZError, names): one tile or more of every kind a masked batch can meet, built from `seed` alone"""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    flt = dtype.kind == "f"
    tiles, masks, names = [], [], []

    def add(name, tile, mask):
        tiles.append(np.asarray(tile, dtype).reshape(r, c))
        masks.append(np.asarray(mask, np.uint8).reshape(r, c))
        names.append(name)

    ones = np.ones((r, c), np.uint8)
    blobs = C.random_blob_mask(rng, 8, r, c)
    if r * c <= 64:
        blobs[:, 0, 0] = 1
        blobs[:, -1, -1] = 0
    add("empty", smooth(rng, r, c, dtype, 2), np.zeros((r, c), np.uint8))
    add("empty", np.zeros((r, c)), np.zeros((r, c), np.uint8))
    add("const all valid", np.full((r, c), 7), ones)
    for k in range(6):    # (masks of several sizes: both parities of the mask section's length)
        m = blobs[k].copy()
        m.reshape(-1)[:k] = 1 - m.reshape(-1)[:k]
        add("const partly valid", np.full((r, c), 1234), m)
    add("const at 0", np.zeros((r, c)), blobs[6])
    add("const at 0, all valid", np.zeros((r, c)), ones)
    if flt:
        add("float const, an integer", np.full((r, c), 42.0), blobs[7])
        add("float const, a fraction", np.full((r, c), 42.5), blobs[7])    # multiples of 0.5: the bound rises to 0.25
        add("float const, a fraction, all valid", np.full((r, c), 0.1), ones)
        add("float const, nothing to raise", np.full((r, c), 0.123456789), blobs[0])
        behind = smooth(rng, r, c, dtype, 2)    # constant over the VALID pixels only
        behind[blobs[1] > 0] = 17.25
        add("float const under the mask", behind, blobs[1])
    else:
        info = np.iinfo(dtype)
        add("int const at the type's maximum", np.full((r, c), info.max), blobs[7])
        add("int const at the type's minimum", np.full((r, c), info.min), blobs[0])
    add("one sweep all valid", full_range_noise(rng, r, c, dtype), ones)
    add("one sweep partly valid", full_range_noise(rng, r, c, dtype), blobs[2])
    add("one sweep partly valid", full_range_noise(rng, r, c, dtype), blobs[3])
    one = np.zeros((r, c), np.uint8)
    one[r // 2, c // 3] = 1
    add("one valid pixel", smooth(rng, r, c, dtype, 2), one)
    # sparsely valid smooth tiles: most 8 x 8 positions hold nothing, the low-bit-rate rule sends them to 16 x 16 blocks
    for p in (0.005, 0.01, 0.02, 0.03, 0.05, 0.08, 0.2):
        add("sparse smooth", smooth(rng, r, c, dtype, 0.3), rng.random((r, c)) < p)
    # one value per 8 x 8 position: a few bytes a block, so the low-bit-rate rule asks for the retry -- and 16 x 16 blocks, which
    # have to spend bits on four values each, lose it
    for m in (ones, blobs[5]):
        steps = rng.integers(900, 1100, ((r + 7) // 8, (c + 7) // 8))
        add("a value per 8 x 8 position", np.kron(steps, np.ones((8, 8), np.int64))[:r, :c], m)
    # smooth tiles at few bits a pixel, all valid or nearly so: the retry is tried, and may lose
    for noise in (0.0, 0.2, 0.4, 0.7, 1.0):
        m = ones.copy()
        m[rng.random((r, c)) < 0.02] = 0
        add("smooth nearly all valid", smooth(rng, r, c, dtype, noise), m)
        add("smooth all valid", smooth(rng, r, c, dtype, noise), ones)
    for k in range(3):
        add("ordinary", smooth(rng, r, c, dtype, 6), blobs[4 + k])
    return np.stack(tiles), np.stack(masks), err_for(dtype), names


def check_whole_encode(B, R, tiles, masks, e, slot_bytes=0, want=None):
    """blobs equal the reference's; as many tiles one by one as have a NaN at a valid pixel -> the reference's blobs"""
    want = want or C.ref_blobs(R, tiles, masks, e)
    c0 = B.counters()
    rc, blobs, offs, sizes, used = B.encode(tiles, masks, e, slot_bytes=slot_bytes)
    c1 = B.counters()
    assert rc == 0, (rc, B.note())
    for t in range(len(tiles)):
        assert blobs[t] == want[t], "tile %d: %d bytes, the reference makes %d (%s)" % (t, len(blobs[t]), len(want[t]), B.note())
    C.check_layout(offs, sizes, used, slot_bytes)
    batch, single = c1[0] - c0[0], c1[1] - c0[1]
    print("encode: %d tiles, %d by the batch's launches, %d one by one" % (len(tiles), batch, single))
    assert batch + single == len(tiles)
    assert single == n_nan_tiles(tiles, masks), (single, B.note())
    return want


def check_whole_decode(B, R, blobs, shape, dtype):
    """valid bytes and valid pixels equal the reference's, every pixel lerc_amd_decode_device's; no tile one by one"""
    c0 = B.counters()
    rc, pix, valid = B.decode(blobs, shape, dtype)
    c1 = B.counters()
    assert rc == 0, (rc, B.note())
    for t in range(len(blobs)):
        rc_r, p_r, m_r = R.decode(blobs[t], want_masks=1)
        assert rc_r == 0
        m_r = m_r[0].reshape(shape)
        assert np.array_equal(valid[t], m_r), "tile %d: valid bytes differ from the reference's" % t
        assert np.array_equal(pix[t][m_r > 0].view(np.uint8), p_r.reshape(shape)[m_r > 0].view(np.uint8)), "tile %d: valid pixels differ from the reference's" % t
        rc_1, p_1, v_1 = B.decode_one(blobs[t], shape, dtype)
        assert rc_1 == 0
        assert np.array_equal(pix[t].view(np.uint8), p_1.view(np.uint8)), "tile %d: pixels differ from lerc_amd_decode_device's" % t
        assert np.array_equal(valid[t], v_1)
    batch, single = c1[2] - c0[2], c1[3] - c0[3]
    print("decode: %d tiles, %d by the batch's launches, %d one by one" % (len(blobs), batch, single))
    assert batch + single == len(blobs)
    assert single == 0, (single, B.note())
    return pix, valid


def slot_for(tiles):
    r, c = tiles.shape[1:]
    return (tiles[0].nbytes + r * c // 4 + 1024 + 15) & ~15


def check_island(B, R, kind, size, tile, n_empty):
    tiles, masks, e = C.island(kind, size, tile)
    n_valid = masks.reshape(len(masks), -1).sum(axis=1)
    assert int((n_valid == 0).sum()) == n_empty and n_empty > 0, "the island has empty corner tiles"
    want = check_whole_encode(B, R, tiles, masks, e)
    check_whole_encode(B, R, tiles, masks, e, slot_bytes=slot_for(tiles), want=want)
    assert sum(kind_of(w, tile * tile, tiles.itemsize) == "empty" for w in want) == n_empty
    check_whole_decode(B, R, want, (tile, tile), tiles.dtype)


def check_kinds(B, R, dtype, r, c):
    """the mosaic of kinds, packed and slotted, and the decode of the reference's blobs"""
    tiles, masks, e, names = kinds_mosaic(dtype, r, c)
    want = C.ref_blobs(R, tiles, masks, e)
    n_pix, item = r * c, tiles.itemsize
    kinds = [kind_of(w, n_pix, item) for w in want]
    print(np.dtype(dtype).name, (r, c), {k: kinds.count(k) for k in sorted(set(kinds))})
    # every kind really occurs, by the reference's own blobs
    assert kinds.count("empty") >= 2 and kinds.count("const") >= 8 and kinds.count("sweep") >= 3 and kinds.count("mb8") >= 1
    facts = [C.blob_facts(w, n_pix, item) for w in want]
    const_rle = [f["rle"] for f, k in zip(facts, kinds) if k == "const"]
    assert 0 in const_rle, "a constant tile without a mask section"
    if n_pix > 64:
        assert {x % 2 for x in const_rle if x > 0} == {0, 1}, "constant tiles with both parities of the mask section's length"
    assert any(k == "sweep" and f["rle"] == 0 for f, k in zip(facts, kinds)) and any(k == "sweep" and f["rle"] > 0 for f, k in zip(facts, kinds))
    assert any(k == "const" and struct.unpack_from("<d", w, 58)[0] == 0 for w, k in zip(want, kinds)), "constant at 0"
    if np.dtype(dtype).kind == "f":
        assert any(k == "const" and w[47] == 1 for w, k in zip(want, kinds)), "a float constant the reference flags as an integer"
        assert any(k == "const" and w[47] == 0 and max_z_err_of(w) > e for w, k in zip(want, kinds)), "a fractional constant whose bound the reference raises"
        assert max_z_err_of(want[names.index("empty")]) == 0
    if r > 8 or c > 8:
        assert kinds.count("mb16") >= 2, "tiles for which the reference writes microBlockSize 16"
        # (no seed search: the tiles with one value per 8 x 8 position are built so that the low-bit-rate rule holds on their blob of
        # 8 x 8 blocks, which the reference keeps -- the retry was tried and lost)
        assert kinds.count("mb8retry") >= 2, "tiles whose retry with 16 x 16 blocks was tried and lost"
    else:
        assert kinds.count("mb16") == 0
    check_whole_encode(B, R, tiles, masks, e, want=want)
    check_whole_encode(B, R, tiles, masks, e, slot_bytes=slot_for(tiles), want=want)
    check_whole_decode(B, R, want, (r, c), dtype)
    return tiles, masks, e, want, kinds


def first_of(kinds, kind, facts=None, need_mask=False):
    for t, k in enumerate(kinds):
        if k == kind and (not need_mask or facts[t]["rle"] > 0):
            return t
    raise AssertionError("no tile of kind " + kind)


def check_damage(B, R, dtype, r, c, n_fuzz):
    """one blob of each new kind: a flipped bit under the old checksum, re-signed random bit flips, a size one byte short"""
    tiles, masks, e, names = kinds_mosaic(dtype, r, c)
    want = C.ref_blobs(R, tiles, masks, e)
    n_pix, item = r * c, tiles.itemsize
    kinds = [kind_of(w, n_pix, item) for w in want]
    facts = [C.blob_facts(w, n_pix, item) for w in want]
    rng = np.random.default_rng(13)
    for kind, need_mask in (("empty", False), ("const", True), ("sweep", True), ("mb16", False)):
        v = first_of(kinds, kind, facts, need_mask)
        others = [t for t in range(len(want)) if t != v][:5]
        group = [want[t] for t in others[:2]] + [want[v]] + [want[t] for t in others[2:]]
        at = 2
        rc, good_pix, good_valid = B.decode(group, (r, c), dtype)
        assert rc == 0

        def neighbours_intact(pix, valid):
            for t in range(len(group)):
                if t != at:
                    assert np.array_equal(pix[t].view(np.uint8), good_pix[t].view(np.uint8)) and np.array_equal(valid[t], good_valid[t])

        # a flipped bit under the old checksum
        for where in sorted({20, HDR + 1, len(want[v]) - 1}):
            bad = bytearray(want[v])
            bad[where] ^= 0x10
            damaged = list(group)
            damaged[at] = bytes(bad)
            rc, pix, valid = B.decode(damaged, (r, c), dtype)
            assert rc == 1, (kind, where, rc)
            assert not pix[at].view(np.uint8).any() and not valid[at].any()
            neighbours_intact(pix, valid)
        # damage behind a checksum that is right again: the single-blob decoder's status and result, never anything else
        for k in range(n_fuzz):
            bad = bytearray(want[v])
            where = int(rng.integers(14, len(bad)))
            bad[where] ^= 1 << int(rng.integers(0, 8))
            damaged = list(group)
            damaged[at] = C.resign(bytes(bad))
            rc, pix, valid = B.decode(damaged, (r, c), dtype)
            rc_1, p_1, v_1 = B.decode_one(damaged[at], (r, c), dtype)
            assert rc == rc_1, (kind, k, where, rc, rc_1)
            if rc_1 == 0:
                assert np.array_equal(pix[at].view(np.uint8), p_1.view(np.uint8)) and np.array_equal(valid[at], v_1), (kind, k, where)
            else:
                assert not pix[at].view(np.uint8).any() and not valid[at].any()
            neighbours_intact(pix, valid)
        # a size one byte short
        rc, pix, valid = decode_with_sizes(B, group, (r, c), dtype, {at: len(want[v]) - 1})
        assert rc == 1, (kind, rc)
        assert not pix[at].view(np.uint8).any() and not valid[at].any()
        neighbours_intact(pix, valid)


def decode_with_sizes(B, blobs, shape, dtype, sizes):
    """Batch.decode with the size of some blobs stated as `sizes` says (the bytes behind stay where they are)"""
    import ctypes as ct
    import capi
    n = len(blobs)
    r, c = shape
    offs = np.zeros(n, np.uint64)
    given = np.array([sizes.get(t, len(b)) for t, b in enumerate(blobs)], np.uint32)
    at = 0
    for t, b in enumerate(blobs):
        offs[t] = at
        at += (len(b) + 15) & ~15
    arena = np.zeros(at + 64, np.uint8)
    for t, b in enumerate(blobs):
        arena[int(offs[t]):int(offs[t]) + len(b)] = np.frombuffer(b, np.uint8)
    ka, pa = B.mem.up(arena)
    item = np.dtype(dtype).itemsize
    ko, po = B.mem.empty(n * r * c * item)
    kv, pv = B.mem.empty(n * r * c)
    rc = B.L.lerc_amd_decode_tiles_device_masked(B.h, pa, offs.ctypes.data, given.ctypes.data, n, c, r, capi.dt_code(dtype), po, pv)
    return rc, B.mem.down(ko, n * r * c * item).view(dtype).reshape(n, r, c), B.mem.down(kv, n * r * c).reshape(n, r, c)


def check_capacity(B, R, dtype, r, c):
    tiles, masks, e, names = kinds_mosaic(dtype, r, c)
    want = C.ref_blobs(R, tiles, masks, e)
    rc, blobs, offs, sizes, used = B.encode(tiles, masks, e)
    assert rc == 0 and blobs == want
    assert B.encode(tiles, masks, e, arena_cap=used)[0] == 0
    assert B.encode(tiles, masks, e, arena_cap=used - 1)[0] == 3
    # a slot 16 bytes too small for a one-sweep tile
    n_pix, item = r * c, tiles.itemsize
    kinds = [kind_of(w, n_pix, item) for w in want]
    largest = max(len(w) for w in want)
    assert kinds[[len(w) for w in want].index(largest)] == "sweep", "the largest blob is a one-sweep one"
    enough = (largest + 15) & ~15
    rc, blobs, _, _, _ = B.encode(tiles, masks, e, slot_bytes=enough)
    assert rc == 0 and blobs == want
    assert B.encode(tiles, masks, e, slot_bytes=enough - 16)[0] == 3


def check_nan(B, R, r, c):
    """a NaN tile among the kinds: the reference's bytes, and that tile alone is done one by one"""
    tiles, masks, e, names = kinds_mosaic(np.float32, r, c)
    t = names.index("ordinary")
    tiles[t, r // 2, c // 2] = np.nan
    masks[t, r // 2, c // 2] = 1
    tiles[0, 0, 0] = np.nan    # (under the mask of an empty tile: no valid pixel is a NaN there)
    assert n_nan_tiles(tiles, masks) == 1
    want = check_whole_encode(B, R, tiles, masks, e)
    check_whole_encode(B, R, tiles, masks, e, slot_bytes=slot_for(tiles), want=want)
    check_whole_decode(B, R, want, (r, c), np.float32)


def check_one_context(L, mem, R, rounds, r, c):
    """such batches on ONE context, between unmasked batches and single masked calls (as tiles_masked_common.check_soak does)"""
    B = C.Batch(L, mem)
    try:
        for k in range(rounds):
            dtype = TYPES[(2 * k + 1) % len(TYPES)]
            tiles, masks, e, names = kinds_mosaic(dtype, r, c, seed=50 + k)
            want = check_whole_encode(B, R, tiles, masks, e, slot_bytes=0 if k % 2 == 0 else slot_for(tiles))
            check_whole_decode(B, R, want, (r, c), dtype)
            rc_u, blobs_u, _, _, _ = B.encode(tiles[-2:], None, e, unmasked_call=True)
            assert rc_u == 0 and blobs_u == C.ref_blobs(R, tiles[-2:], None, e)
            for t in (0, 3, len(tiles) - 1):
                rc_1, blob_1 = B.encode_one(tiles[t], masks[t], e)
                assert rc_1 == 0 and blob_1 == want[t]
    finally:
        B.close()
