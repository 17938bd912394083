"""Shared by test_sim_tiles_bytes_masked.py (CPU emulator library) and test_gpu_tiles_bytes_masked.py (MI355X): MASKED 8-bit tile
batches -- int8 / uint8 tiles with a byte mask per tile, lossless -- through lerc_amd_encode_tiles_device_masked /
lerc_amd_decode_tiles_device_masked, and the rule for what such a batch may hand back.  Drivers, memory, masks and the re-signing
of damaged blobs come from tiles_masked_common.py, content from tiles_bytes_common.py.
"""
import struct

import numpy as np

import tiles_bytes_common as C
import tiles_masked_common as M
from tiles_masked_common import Batch, HostMem, GpuMem, HDR, check_layout, ref_blobs, resign, sub_batches_of    # noqa: F401


def facts(blob):
    """-> dict(num_valid, mb, blob_size, rle, const, one_sweep, mode, data) of a single-band codec 6 byte blob; the one-sweep and the
    mode byte lie at 90 + 4 + rle + 2"""
    num_valid, mb, blob_size = struct.unpack_from("<iii", blob, 26)
    z_min, z_max = struct.unpack_from("<dd", blob, 58)
    rle = struct.unpack_from("<i", blob, HDR)[0]
    f = dict(num_valid=num_valid, mb=mb, blob_size=blob_size, rle=rle, const=z_min == z_max, one_sweep=None, mode=None, data=None)
    if num_valid > 0 and z_min != z_max:
        at = HDR + 4 + rle + 2
        f["one_sweep"] = blob[at]
        if blob[at] == 0:
            f["mode"] = blob[at + 1]
            f["data"] = blob_size - (at + 2)    # nBytesTiling resp. nBytesHuffman
    return f


def must_batch(blob, n_pix):
    """the batch's own launches must take a tile when its reference blob has no valid pixel, or is not constant, not one sweep, and is
    either in a Huffman mode or in tiling mode with 8 x 8 blocks and the retry condition (Lerc2.cpp:335-338, with numValidPixel for
    the one-sweep size; nBytesHuffman is not in the blob, its clause is left out: the condition here is the wider one) false"""
    f = facts(blob)
    if f["num_valid"] == 0:
        return True
    if f["const"] or f["one_sweep"] != 0:
        return False
    if f["mode"] in (1, 2):
        return True
    if f["mode"] == 0 and f["mb"] == 8:
        return not (f["data"] * 8 < n_pix * 1.5 and f["data"] < 4 * f["num_valid"])
    return False


def modes(blobs, n_pix):
    """-> counts of (delta Huffman, Huffman, tiling) among the blobs the rule names that have a valid pixel"""
    out = [0, 0, 0]
    for b in blobs:
        f = facts(b)
        if f["num_valid"] > 0 and must_batch(b, n_pix):
            out[{1: 0, 2: 1, 0: 2}[f["mode"]]] += 1
    return out


def slot_for(tiles):
    return (tiles[0].nbytes + tiles[0].size // 4 + 1024 + 15) & ~15


def byte_island(size, tile, dtype=np.uint8):
    """-> (tiles, masks): the byte mosaic under the island mask"""
    from lerc_amd import synth
    return C.byte_mosaic(size, tile, dtype), synth.cut_tiles(synth.island_mask(size), tile)


# ---- masks for the predictor's corners --------------------------------------------------------------------------------
def corner_masks(r, c, seed=3):
    """-> (masks uint8 [k, r, c], names)"""
    yy, xx = np.mgrid[0:r, 0:c]
    ones = np.ones((r, c), np.uint8)
    out = []
    out.append(("checkerboard", ((yy + xx) % 2).astype(np.uint8)))                       # every predecessor is prevVal
    out.append(("stripes1", (xx % 2 == 0).astype(np.uint8)))                                # every segment head restarts from above
    out.append(("stripes3", ((xx // 3) % 2 == 1).astype(np.uint8)))
    m = ones.copy()
    m[:3] = 0
    m[3, :c // 2 + 1] = 0                                                                   # prevVal 0 away from the origin
    out.append(("late start", m))
    m = ones.copy()
    m[2:5] = 0
    m[9] = 0
    m[5, :] = (xx[5] % 5 == 4)                                                              # prevVal from rows back, no pixel above
    m[10, :] = (xx[10] > c // 3)
    out.append(("empty rows", m))
    m = ones.copy()
    m[1::2, 0] = 0                                                                          # column 0 invalid, the previous row's last pixel valid
    m[4, :] = 0
    m[5, 0] = 1                                                                             # column 0 valid, the pixel above invalid: not k - 1
    m[6, 0] = 1
    m[5, 1] = 0
    out.append(("column 0", m))
    m = ones.copy()
    m[-1, -1] = 0
    out.append(("last pixel", m))
    rng = np.random.default_rng(seed)
    out.append(("blob", M.random_blob_mask(rng, 1, r, c)[0]))
    out.append(("blob small", M.random_blob_mask(rng, 1, r, c, 0.05, 0.3)[0]))
    return np.stack([k[1] for k in out]), [k[0] for k in out]


def block_noise(r, c, seed=17):
    """4 bits of noise on a base of its own per 8 x 8 block: the blocks' ranges are narrow, the tile's histograms wide -- tiling mode"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:r, 0:c]
    base = rng.integers(0, 240, ((r + 7) // 8, (c + 7) // 8))
    return (base[yy // 8, xx // 8] + rng.integers(0, 16, (r, c))).astype(np.uint8)


def corner_batch(r, c, dtype=np.uint8):
    """every mask of corner_masks over five kinds of content: noise16 and palette (tiles_bytes_common.variety) go Huffman,
    smooth+noise and ramp delta Huffman, block_noise tiling -> (tiles, masks)"""
    content, names = C.variety(r, c)
    masks, _ = corner_masks(r, c)
    kinds = [content[names.index(k)] for k in ("noise16", "palette", "smooth+noise", "ramp")] + [block_noise(r, c)]
    tiles, ms = [], []
    for kind in kinds:
        for m in masks:
            tiles.append(kind)
            ms.append(m)
    tiles = np.stack(tiles)
    if dtype == np.int8:
        tiles = (tiles.astype(np.int16) - 128).astype(np.int8)
    return tiles, np.stack(ms)


# ---- checks -----------------------------------------------------------------------------------------------------------
def check_encode(B, R, tiles, masks, want=None, slot_bytes=0, arena_shift=0):
    """every blob equals the reference's, the layout holds, the counters respect the cap -> the reference's blobs"""
    want = want or ref_blobs(R, tiles, masks, 0)
    n, n_pix = len(tiles), tiles[0].size
    c0 = B.counters()
    rc, blobs, offs, sizes, used = B.encode(tiles, masks, 0, slot_bytes=slot_bytes, arena_shift=arena_shift)
    c1 = B.counters()
    assert rc == 0, (rc, B.note())
    for t in range(n):
        assert blobs[t] == want[t], "tile %d: %d bytes, the reference makes %d (%s)" % (t, len(blobs[t]), len(want[t]), B.note())
    check_layout(offs, sizes, used, slot_bytes)
    batch, single = c1[0] - c0[0], c1[1] - c0[1]
    must = sum(must_batch(w, n_pix) for w in want)
    print("encode: %d tiles, %d by the batch's launches, %d one by one; the reference's blobs ask for at least %d in the batch; modes %s"
          % (n, batch, single, must, modes(want, n_pix)))
    assert batch + single == n
    assert single <= n - must, (single, n - must, B.note())
    return want


def check_decode(B, R, blobs, shape, dtype, masks=None):
    """pixels at valid positions and valid bytes equal the reference's; everything equals lerc_amd_decode_device's with nMasks = 1"""
    n = len(blobs)
    c0 = B.counters()
    rc, pix, valid = B.decode(blobs, shape, dtype)
    c1 = B.counters()
    assert rc == 0, (rc, B.note())
    for t in range(n):
        rc_r, p_r, m_r = R.decode(blobs[t], want_masks=1)
        assert rc_r == 0
        m_r = m_r[0]
        assert np.array_equal(valid[t], m_r), "tile %d: valid bytes differ from the reference's" % t
        if masks is not None:
            assert np.array_equal(valid[t], (masks[t] > 0).astype(np.uint8))
        assert np.array_equal(pix[t][m_r > 0].view(np.uint8), p_r.reshape(shape)[m_r > 0].view(np.uint8)), "tile %d: valid pixels differ from the reference's" % t
        rc_1, p_1, v_1 = B.decode_one(blobs[t], shape, dtype)
        assert rc_1 == 0
        assert np.array_equal(pix[t].view(np.uint8), p_1.view(np.uint8)), "tile %d: pixels differ from lerc_amd_decode_device's" % t
        assert np.array_equal(valid[t], v_1)
    batch, single = c1[2] - c0[2], c1[3] - c0[3]
    must = sum(must_batch(b, shape[0] * shape[1]) for b in blobs)
    print("decode: %d tiles, %d by the batch's launches, %d one by one; at least %d asked for" % (n, batch, single, must))
    assert batch + single == n
    assert single <= n - must, (single, n - must, B.note())
    return pix, valid


def check_round_trip(B, R, tiles, masks, expect_must=None, shifted=True):
    """packed, slotted, at an odd arena address; then the decode; own blobs are the reference's -> the reference's blobs"""
    want = check_encode(B, R, tiles, masks)
    n_pix = tiles[0].size
    must = sum(must_batch(w, n_pix) for w in want)
    with_valid = sum(facts(w)["num_valid"] > 0 for w in want)
    must_valid = sum(must_batch(w, n_pix) and facts(w)["num_valid"] > 0 for w in want)
    assert 4 * must_valid >= 3 * with_valid, "the rule names %d of the %d tiles with a valid pixel" % (must_valid, with_valid)
    if expect_must is not None:
        assert must == expect_must, must
    check_encode(B, R, tiles, masks, want=want, slot_bytes=slot_for(tiles))
    if shifted:
        check_encode(B, R, tiles, masks, want=want, arena_shift=1)
    pix, _ = check_decode(B, R, want, tiles[0].shape, tiles.dtype, masks)
    assert np.array_equal(pix[masks > 0], tiles[masks > 0])
    return want


# what the reference's blobs of corner_batch ask for (of 45 tiles; one or two "blob small" tiles go to 16 x 16 blocks), checked on the CPU
CORNER_MUST = {(40, 56, "uint8"): 43, (40, 56, "int8"): 44, (65, 65, "uint8"): 44, (65, 65, "int8"): 44}


def check_corners(B, R, r, c, dtype=np.uint8):
    tiles, masks = corner_batch(r, c, dtype)
    want = check_round_trip(B, R, tiles, masks, expect_must=CORNER_MUST[(r, c, np.dtype(dtype).name)])
    parities = set(facts(w)["rle"] % 2 for w in want if facts(w)["rle"] > 0)
    assert parities == {0, 1}, "both parities of the mask section's length occur"
    m = modes(want, r * c)
    assert min(m) > 0, "delta Huffman, Huffman and tiling all occur among the tiles the rule names: %s" % m
    return want


def check_sub_batches(B, R, r=40, c=56):
    """7 tiles in sub-batches of 3 + 3 + 1, packed and slotted: tile 4, in the second sub-batch, is constant over its valid pixels and
    handed back, each way; tile 6, the third sub-batch, has no valid pixel and stays"""
    rng = np.random.default_rng(53)
    n = 7
    yy, xx = np.mgrid[0:r, 0:c]
    tiles = np.stack([np.clip(np.round(128 + 100 * np.sin(yy / rng.uniform(9, 40)) * np.cos(xx / rng.uniform(9, 40)) + rng.normal(0, rng.uniform(2, 6), (r, c))),
                              0, 255).astype(np.uint8) for _ in range(n)])
    masks = M.random_blob_mask(rng, n, r, c)
    masks[1][:] = 1
    tiles[4][masks[4] > 0] = 77
    masks[6][:] = 0
    want = ref_blobs(R, tiles, masks, 0)
    assert [must_batch(w, r * c) for w in want] == [True] * 4 + [False] + [True] * 2
    with sub_batches_of(3):
        for slot in (0, slot_for(tiles)):
            c0 = B.counters()
            check_encode(B, R, tiles, masks, want=want, slot_bytes=slot)
            c1 = B.counters()
            assert (c1[0] - c0[0], c1[1] - c0[1]) == (n - 1, 1), (c0, c1, B.note())
        c0 = B.counters()
        check_decode(B, R, want, (r, c), np.uint8, masks)
        c1 = B.counters()
        assert (c1[2] - c0[2], c1[3] - c0[3]) == (n - 1, 1), (c0, c1, B.note())


def error_batch(r=64, c=64):
    """5 tiles whose tile 2 is a partly valid Huffman tile the rule names"""
    rng = np.random.default_rng(59)
    content, names = C.variety(r, c)
    tiles = np.stack([content[names.index(k)] for k in ("smooth+noise", "palette", "noise16", "ramp", "smooth+noise")])
    masks = M.random_blob_mask(rng, 5, r, c, 0.4, 0.8)
    masks[3][:] = 1
    return tiles, masks


def check_errors(B, R, n_fuzz=8):
    tiles, masks = error_batch()
    n, shape, dtype = len(tiles), tiles[0].shape, tiles.dtype
    n_pix = tiles[0].size
    want = ref_blobs(R, tiles, masks, 0)
    f2 = facts(want[2])
    assert f2["mode"] in (1, 2) and must_batch(want[2], n_pix) and 0 < f2["num_valid"] < n_pix and f2["rle"] > 8
    assert sum(must_batch(w, n_pix) for w in want) == n, "the rule names every tile of this batch"
    check_encode(B, R, tiles, masks, want=want)    # (the counters: all five by the batch's launches)
    rc, blobs, offs, sizes, used = B.encode(tiles, masks, 0)
    assert rc == 0 and blobs == want
    # an arena one byte too small, a slot too small
    assert B.encode(tiles, masks, 0, arena_cap=used - 1)[0] == 3
    assert B.encode(tiles, masks, 0, arena_cap=used)[0] == 0
    small = (max(len(w) for w in want) - 1) & ~15
    assert B.encode(tiles, masks, 0, slot_bytes=small)[0] == 3
    assert B.encode(tiles, masks, 0, slot_bytes=small + 16)[0] == 0
    good, good_valid = check_decode(B, R, want, shape, dtype, masks)    # (the counters: all five by the batch's launches)
    others = [t for t in range(n) if t != 2]

    def decode_damaged(damaged):
        """-> (status, pixels, valid bytes); the four undamaged neighbours stay the batch's own, tile 2 may be handed back"""
        c0 = B.counters()
        out = B.decode(damaged, shape, dtype)
        c1 = B.counters()
        batch, single = c1[2] - c0[2], c1[3] - c0[3]
        print("decode with tile 2 damaged: %d by the batch's launches, %d one by one%s" % (batch, single, " (%s)" % B.note() if single else ""))
        assert batch + single == n and batch >= n - 1, (batch, single, B.note())
        return out

    def neighbours_untouched(pix, valid):
        for t in others:
            assert np.array_equal(pix[t], good[t]) and np.array_equal(valid[t], good_valid[t])

    # one flipped bit -- in the mask section, in the code table, in the pixel stream: Failed(1), zeros for that tile
    table = HDR + 4 + f2["rle"] + 4
    for where in (HDR + 4 + 3, table + 20, len(want[2]) - 9):
        bad = bytearray(want[2])
        bad[where] ^= 0x10
        damaged = list(want)
        damaged[2] = bytes(bad)
        rc, pix, valid = decode_damaged(damaged)
        assert rc == 1, (where, rc)
        assert not pix[2].any() and not valid[2].any()
        neighbours_untouched(pix, valid)
    # a header whose numValidPixel is off by one behind a right checksum, and seeded flips re-signed: the status and the result of
    # the single-blob decoder, never anything else
    cases = []
    for d in (1, -1):
        bad = bytearray(want[2])
        bad[26:30] = struct.pack("<i", f2["num_valid"] + d)
        cases.append(resign(bytes(bad)))
    rng = np.random.default_rng(61)
    for k in range(n_fuzz):
        bad = bytearray(want[2])
        hi = (table + 16 + 3 + 200, HDR + 4 + f2["rle"], len(bad))[k % 3]
        where = int(rng.integers(HDR, hi))
        bad[where] ^= 1 << int(rng.integers(0, 8))
        cases.append(resign(bytes(bad)))
    for k, blob in enumerate(cases):
        damaged = list(want)
        damaged[2] = blob
        rc, pix, valid = decode_damaged(damaged)
        rc_1, p_1, v_1 = B.decode_one(blob, shape, dtype)
        assert rc == rc_1, (k, rc, rc_1, B.note())
        if rc_1 == 0:
            assert np.array_equal(pix[2], p_1) and np.array_equal(valid[2], v_1), k
        else:
            assert not pix[2].any() and not valid[2].any()
        neighbours_untouched(pix, valid)


def check_soak(L, mem, R, rounds, max_tiles, size, tile):
    """masked byte batches of random size on ONE context, between all-valid byte batches, masked uint16 / float32 batches and
    unmasked float32 batches; then a fresh context per batch for three rounds.  Every blob is compared with the reference's."""
    rng = np.random.default_rng(67)
    src, src_masks = byte_island(size, tile)
    partial = [t for t in range(len(src)) if 0 < src_masks[t].sum() < src_masks[t].size]
    r = c = tile
    B = Batch(L, mem)
    try:
        for k in range(rounds):
            n = int(rng.integers(1, max_tiles + 1))
            pick = rng.choice(len(src), n, replace=False)
            pick[0] = partial[k % len(partial)]
            tiles = src[pick] if k % 2 == 0 else (src[pick].astype(np.int16) - 128).astype(np.int8)
            masks = src_masks[pick] if k % 3 else M.random_blob_mask(rng, n, r, c, 0.02, 1.0)
            want = check_encode(B, R, tiles, masks, slot_bytes=0 if k % 3 else slot_for(tiles))
            check_decode(B, R, want, (r, c), tiles.dtype, masks)
            C.check_encode(B, R, src[pick[:3]])
            other = M.terrain_int(rng, 3, r, c, np.int32)
            other = (other + rng.normal(0, 0.3, other.shape)).astype(np.float32) if k % 2 else other.astype(np.uint16)
            e = 0.01 if k % 2 else 0
            om = M.random_blob_mask(rng, 3, r, c)
            rc_m, blobs_m, _, _, _ = B.encode(other, om, e)
            assert rc_m == 0 and blobs_m == ref_blobs(R, other, om, e)
            flt = other.astype(np.float32)
            rc_u, blobs_u, _, _, _ = B.encode(flt, None, 0.01, unmasked_call=True)
            assert rc_u == 0 and blobs_u == ref_blobs(R, flt, None, 0.01)
    finally:
        B.close()
    for k in range(3):
        pick = partial[k::3][:4]
        tiles, masks = src[pick], src_masks[pick]
        B = Batch(L, mem)
        try:
            want = check_encode(B, R, tiles, masks)
        finally:
            B.close()
        B = Batch(L, mem)
        try:
            check_decode(B, R, want, (r, c), np.uint8, masks)
        finally:
            B.close()
