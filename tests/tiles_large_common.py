"""Shared by test_sim_tiles_large.py (CPU emulator library) and test_gpu_tiles_large.py (MI355X): tiles beyond the size the tile
batches took at first (131 072 pixels, 4 096 blocks of 8 x 8) -- up to 513 x 513 -- through every family of the shared driver.  The
drivers, the round-trip helpers and the rules for what a batch may hand back are the families' own (tiles_masked_common.py,
tiles_bytes_common.py, tiles_bytes_masked_common.py, tiles_bands_common.py); here are the shapes, the content, and the assertion
that makes these tests fail where such tiles are done one by one: every tile the rule names is counted as the batch's own.

The shapes: 8 x 16 392 crosses the old pixel limit alone (131 136 pixels, 2 049 blocks), 1 x 32 776 the old block limit alone (4 097
blocks), 513 x 513 both (263 169 pixels, 4 225 blocks; the width is odd, so mask bits cross byte boundaries at k - width).
"""
import struct

import numpy as np

import tiles_bands_common as T
import tiles_bytes_common as C
import tiles_bytes_masked_common as BM
import tiles_masked_common as M
from tiles_bytes_common import slot_for
from tiles_masked_common import must_batch, sub_batches_of    # noqa: F401

THIN_PIXELS = (8, 16392)
THIN_BLOCKS = (1, 32776)
REAL = (513, 513)
SHAPES = [THIN_PIXELS, THIN_BLOCKS, REAL]
STAGE_BYTES = 4 * 10240    # the 8-bit decoder's LDS stage (kTbbdStageWords, tile_byte_batch.hip)


def counted(B, k, f):
    """f() -> (its result, how far counter k and counter k + 1 moved)"""
    c0 = B.counters()
    out = f()
    c1 = B.counters()
    return out, c1[k] - c0[k], c1[k + 1] - c0[k + 1]


def all_in_batch(B, k, n, f):
    out, batch, single = counted(B, k, f)
    assert (batch, single) == (n, 0), ("tiles left the batch's launches", batch, single, B.note())
    return out


# ---- content ----------------------------------------------------------------------------------------------------------------
def terrain(rng, r, c, sigma=9.0):
    """smooth plus noise of several bits: at 40 % valid still well above the 1.5 bits a pixel of the low-bit-rate rule"""
    yy, xx = np.mgrid[0:r, 0:c]
    return 900 + 400 * np.sin(yy / rng.uniform(9, 40) + 1.0) * np.cos(xx / rng.uniform(9, 40)) + rng.normal(0, sigma, (r, c))


def masks_of(rng, n, r, c, lo=0.4, hi=0.8):
    return M.random_blob_mask(rng, n, r, c, lo, hi)


KINDS = ("all valid", "empty", "constant", "one sweep", "blocks16", "blocks8")


def wide_batch(shape, dtype, seed=71):
    """-> (tiles [6, r, c], masks): one tile of every whole-tile kind of the masked family, KINDS in this order"""
    r, c = shape
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    n = len(KINDS)
    tiles = np.stack([terrain(rng, r, c) for _ in range(n)])
    masks = masks_of(rng, n, r, c)
    masks[0][:] = 1
    masks[1][:] = 0
    tiles[2][:] = 1234
    tiles[3] = rng.uniform(-1e9, 1e9, (r, c)) if dtype.kind == "f" else rng.integers(0, 65536, (r, c))
    if r >= 16:
        # one bit of noise beside a constant strip: the low-bit-rate retry ends in 16 x 16 blocks (tiles_bands_common.mixed_wide)
        tiles[4] = 5 + (rng.random((r, c)) < 0.5)
        tiles[4][:, :c // 3] = 5
        masks[4] = masks_of(rng, 1, r, c, 0.6, 0.9)[0]
    else:
        # a few rows: a block's header outweighs one bit a pixel, so the rule holds only where most blocks are empty and the others
        # constant -- one value per 16 columns, two values in the tile
        yy, xx = np.mgrid[0:r, 0:c]
        tiles[4] = 5 + ((xx // 16) % 7 == 0)
        masks[4] = masks_of(rng, 1, r, c, 0.25, 0.35)[0]
    if dtype.kind == "f":
        tiles = tiles.copy()
        frac = rng.normal(0, 0.3, (r, c))
        for t in (0, 5):
            tiles[t] += frac
        return tiles.astype(dtype), masks
    return np.clip(np.round(tiles), 0, 65535).astype(dtype), masks


def wide_kinds(want, n_pix, item):
    out = []
    for w in want:
        f = M.blob_facts(w, n_pix, item)
        if f["num_valid"] == 0:
            out.append("empty")
        elif f["const"]:
            out.append("constant")
        elif f["one_sweep"] == 1:
            out.append("one sweep")
        elif f["mb"] == 16:
            out.append("blocks16")
        else:
            out.append("all valid" if f["num_valid"] == n_pix else "blocks8")
    return out


def byte_tiles(shape, dtype=np.uint8, seed=73):
    """-> tiles [3, r, c]: smooth plus noise (delta Huffman), 16 values of noise (Huffman: 4 bits a pixel), four bits of noise on a
    base per 8 x 8 block (tiling).  In a single row a block's two header bytes weigh two bits a pixel: there the blocks are constant,
    which is tiling where every pixel is valid and delta Huffman under a mask -- tiling cannot win under a mask in one row"""
    r, c = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:r, 0:c]
    smooth = 128 + 100 * np.sin(yy / 23.0 + 1.0) * np.cos(xx / 31.0) + rng.normal(0, 2, (r, c))
    blocks = BM.block_noise(r, c) if r >= 8 else rng.integers(0, 250, (1, (c + 7) // 8))[yy // 8, xx // 8].astype(np.uint8)
    tiles = np.stack([np.clip(np.round(smooth), 0, 255).astype(np.uint8), (rng.integers(0, 16, (r, c)) * 16).astype(np.uint8), blocks])
    return tiles if dtype == np.uint8 else (tiles.astype(np.int16) - 128).astype(np.int8)


# ---- the families ------------------------------------------------------------------------------------------------------------
def check_masked_wide(B, R, shape, dtype, e):
    """every whole-tile kind of the masked family at this shape, four layouts and the decode, nothing handed back"""
    tiles, masks = wide_batch(shape, dtype)
    n, n_pix, item = len(tiles), tiles[0].size, tiles.itemsize
    want = M.ref_blobs(R, tiles, masks, e)
    assert wide_kinds(want, n_pix, item) == list(KINDS), wide_kinds(want, n_pix, item)
    assert sum(must_batch(w, n_pix, item) for w in want) == 2, "the rule names the two tiles of 8 x 8 blocks; the family keeps the other kinds too"
    all_in_batch(B, 0, n, lambda: M.check_encode(B, R, tiles, masks, e, want=want))
    all_in_batch(B, 0, n, lambda: M.check_encode(B, R, tiles, masks, e, slot_bytes=slot_for(tiles), want=want))
    rc, blobs, offs, sizes, used = all_in_batch(B, 0, n, lambda: B.encode(tiles, masks, e, arena_shift=1))
    assert rc == 0 and blobs == want
    M.check_layout(offs, sizes, used)
    pix, valid = all_in_batch(B, 2, n, lambda: M.check_decode(B, R, want, shape, tiles.dtype))
    assert np.array_equal(valid, (masks > 0).astype(np.uint8))
    # the unmasked call and the masked call without a mask: the same blobs (the one-launch tile encoder's, which has no such limit)
    rc_a, blobs_a, _, _, _ = B.encode(tiles[5:], None, e)
    rc_b, blobs_b, _, _, _ = B.encode(tiles[5:], None, e, unmasked_call=True)
    assert rc_a == 0 and rc_b == 0 and blobs_a == blobs_b == M.ref_blobs(R, tiles[5:], None, e)
    return want


def check_bytes(B, R, shape, dtype):
    """8-bit, every pixel valid: packed, slotted, the unmasked call, an odd arena address, both decodes (check_round_trip)"""
    tiles = byte_tiles(shape, dtype)
    n = len(tiles)
    (want, batch, single) = counted(B, 0, lambda: C.check_round_trip(B, R, tiles, expect_must=n))
    assert single == 0 and batch == 5 * n, ("tiles left the batch's launches", batch, single, B.note())
    assert C.modes(want) == [1, 1, 1], C.modes(want)
    all_in_batch(B, 2, n, lambda: C.check_decode(B, R, want, shape, tiles.dtype))
    if tiles[0].size // 2 > STAGE_BYTES:
        assert want[1][C.AT + 1] == 2 and len(want[1]) > STAGE_BYTES + 2048, "the Huffman tile's stream is read where it lies"
    return want


def check_bytes_masked(B, R, shape, dtype):
    tiles = byte_tiles(shape, dtype, seed=79)
    n, n_pix = len(tiles), tiles[0].size
    masks = masks_of(np.random.default_rng(83), n, *shape)
    (want, batch, single) = counted(B, 0, lambda: BM.check_round_trip(B, R, tiles, masks, expect_must=n))
    assert single == 0 and batch == 3 * n, ("tiles left the batch's launches", batch, single, B.note())
    assert BM.modes(want, n_pix) == ([1, 1, 1] if shape[0] >= 8 else [2, 1, 0]), BM.modes(want, n_pix)
    all_in_batch(B, 2, n, lambda: BM.check_decode(B, R, want, shape, tiles.dtype, masks))
    if n_pix // 4 > STAGE_BYTES:
        f = BM.facts(want[1])
        assert f["mode"] == 2 and f["data"] > STAGE_BYTES + 2048, "the Huffman tile's stream is read where it lies"
    return want


def check_bands(B, R, dtype, nb, with_mask, shape=REAL, n=2, four_layouts=True):
    """band stacks whose planes are of this shape: four layouts (the emulator, where a plane takes seconds: packed, and slotted at an
    odd arena address) and the decode, nothing handed back"""
    r, c = shape
    rng = np.random.default_rng(89)
    if np.dtype(dtype).itemsize == 1:
        tiles = np.stack([np.stack([byte_tiles(shape, dtype, seed=97 + t)[k % 3] for k in range(nb)]) for t in range(n)])
    else:
        tiles = np.stack([np.stack([np.clip(np.round(terrain(rng, r, c, 3.0 + 5 * k)), 0, 65535) for k in range(nb)]) for t in range(n)]).astype(dtype)
    masks = masks_of(rng, n, r, c) if with_mask else None
    if four_layouts:
        (want, batch, single) = counted(B, 0, lambda: T.check_four_layouts(B, R, tiles, masks, 0))
        # (four layouts, the query for arenaUsed, and what fitted the arena that was a byte too small)
        assert single == 0 and batch >= 5 * n, ("tiles left the batch's launches", batch, single, B.note())
    else:
        want = all_in_batch(B, 0, n, lambda: T.check_encode(B, R, tiles, masks, 0))
        all_in_batch(B, 0, n, lambda: T.check_encode(B, R, tiles, masks, 0, slot_bytes=T.slot_for(tiles), want=want, arena_shift=1))
    assert sum(T.must_batch(w, r * c, tiles.itemsize) for w in want) == n
    residues = set(s % 4 for w in want for s in T.band_starts(w)[1:])
    assert len(residues) > 1, ("bands behind band 0 start at more than one residue mod 4", residues)
    all_in_batch(B, 2, n, lambda: T.check_decode(B, R, want, (nb, r, c), dtype, 1 if with_mask else 0))
    return want


def check_sub_batches(B, R, dtype, shape=THIN_PIXELS):
    """5 tiles in sub-batches of 2 + 2 + 1, packed and slotted: the larger records, the first tile and the arena's base of a later
    sub-batch; all five stay in the batch"""
    r, c = shape
    rng = np.random.default_rng(101)
    n = 5
    masks = masks_of(rng, n, r, c)
    with sub_batches_of(2):
        if np.dtype(dtype).itemsize == 1:
            tiles = np.stack([byte_tiles(shape, dtype, seed=103 + t)[t % 3] for t in range(n)])
            want = M.ref_blobs(R, tiles, masks, 0)
            assert sum(BM.must_batch(w, r * c) for w in want) == n
            for slot in (0, slot_for(tiles)):
                all_in_batch(B, 0, n, lambda: BM.check_encode(B, R, tiles, masks, want=want, slot_bytes=slot))
            all_in_batch(B, 2, n, lambda: BM.check_decode(B, R, want, shape, tiles.dtype, masks))
        else:
            tiles = np.clip(np.round(np.stack([terrain(rng, r, c) for _ in range(n)])), 0, 65535).astype(dtype)
            want = M.ref_blobs(R, tiles, masks, 0)
            assert sum(must_batch(w, r * c, tiles.itemsize) for w in want) == n
            for slot in (0, slot_for(tiles)):
                all_in_batch(B, 0, n, lambda: M.check_encode(B, R, tiles, masks, 0, slot_bytes=slot, want=want))
            all_in_batch(B, 2, n, lambda: M.check_decode(B, R, want, shape, tiles.dtype))


def check_errors(B, R, shape=REAL, n_fuzz=4):
    """3 int16 tiles: a slot 16 bytes too small; one flipped bit in tile 1 (mask section, block stream); damaged blobs re-signed"""
    r, c = shape
    rng = np.random.default_rng(107)
    n = 3
    tiles = np.round(np.stack([terrain(rng, r, c) for _ in range(n)])).astype(np.int16)
    masks = masks_of(rng, n, r, c)
    want = M.ref_blobs(R, tiles, masks, 0)
    assert sum(must_batch(w, r * c, 2) for w in want) == n
    small = (max(len(w) for w in want) - 1) & ~15
    assert B.encode(tiles, masks, 0, slot_bytes=small)[0] == 3
    (out, batch, single) = counted(B, 0, lambda: B.encode(tiles, masks, 0, slot_bytes=small + 16))
    assert out[0] == 0 and out[1] == want and (batch, single) == (n, 0), (out[0], batch, single, B.note())
    (out, batch, single) = counted(B, 2, lambda: B.decode(want, shape, np.int16))
    rc, good_pix, good_valid = out
    assert rc == 0 and (batch, single) == (n, 0), (rc, batch, single, B.note())
    f = M.blob_facts(want[1], r * c, 2)
    assert f["rle"] > 4

    def neighbours_untouched(pix, valid):
        for t in (0, 2):
            assert np.array_equal(pix[t], good_pix[t]) and np.array_equal(valid[t], good_valid[t])

    for where in (M.HDR + 4 + 1, len(want[1]) - 9):
        bad = bytearray(want[1])
        bad[where] ^= 0x10
        rc_1 = B.decode_one(bytes(bad), shape, np.int16)[0]
        rc, pix, valid = B.decode([want[0], bytes(bad), want[2]], shape, np.int16)
        assert rc == rc_1 and rc != 0, (where, rc, rc_1)
        assert not pix[1].any() and not valid[1].any()
        neighbours_untouched(pix, valid)
    for k in range(n_fuzz):
        bad = bytearray(want[1])
        where = int(rng.integers(M.HDR + 4, len(bad)))
        bad[where] ^= 1 << int(rng.integers(0, 8))
        blob = M.resign(bytes(bad))
        rc, pix, valid = B.decode([want[0], blob, want[2]], shape, np.int16)
        rc_1, p_1, v_1 = B.decode_one(blob, shape, np.int16)
        assert rc == rc_1, (k, where, rc, rc_1)
        if rc_1 == 0:
            assert np.array_equal(pix[1], p_1) and np.array_equal(valid[1], v_1)
        else:
            assert not pix[1].any() and not valid[1].any()
        neighbours_untouched(pix, valid)


def check_long_runs(B, R, shape=REAL):
    """a mask of more than 32 767 equal bytes: the run-length coder cuts a run there, which no smaller tile reaches -- one invalid
    pixel, the last, the first, and one in the middle of a tile, uint16 and uint8"""
    r, c = shape
    rng = np.random.default_rng(127)
    n = 3
    masks = np.ones((n, r, c), np.uint8)
    masks[0, -1, -1] = 0
    masks[1, 0, 0] = 0
    masks[2, r // 2, c // 2] = 0
    wide = np.round(np.stack([terrain(rng, r, c) for _ in range(n)])).astype(np.uint16)
    want = M.ref_blobs(R, wide, masks, 0)
    assert (r * c + 7) // 8 > 32767 + 6 and struct.unpack_from("<h", want[0], M.HDR + 4)[0] == -32767, "the reference cuts tile 0's run at 32 767 bytes"
    all_in_batch(B, 0, n, lambda: M.check_encode(B, R, wide, masks, 0, want=want))
    pix, valid = all_in_batch(B, 2, n, lambda: M.check_decode(B, R, want, shape, np.uint16))
    assert np.array_equal(valid, masks)
    byte = np.stack([byte_tiles(shape, seed=131 + t)[0] for t in range(n)])
    want = M.ref_blobs(R, byte, masks, 0)
    all_in_batch(B, 0, n, lambda: BM.check_encode(B, R, byte, masks, want=want))
    all_in_batch(B, 2, n, lambda: BM.check_decode(B, R, want, shape, np.uint8, masks))


def check_above_the_limit(B, R, shape):
    """one tile per family of a shape the batches do not take: status 0, the reference's bytes, done one by one, and the note says why"""
    r, c = shape
    rng = np.random.default_rng(109)
    mask = masks_of(rng, 1, r, c)

    def one_by_one(k, f):
        out, batch, single = counted(B, k, f)
        assert (batch, single) == (0, 1), (batch, single, B.note())
        assert "size" in B.note() and "%d x %d" % (r, c) in B.note(), B.note()
        return out

    wide = np.round(terrain(rng, r, c))[None].astype(np.uint16)
    flt = (terrain(rng, r, c))[None].astype(np.float32)
    byte = byte_tiles(shape)[:1]
    for tiles, e in ((wide, 0), (flt, 0.01)):
        want = one_by_one(0, lambda: M.check_encode(B, R, tiles, mask, e, cap_counters=False))
        one_by_one(2, lambda: B.decode(want, shape, tiles.dtype))
        M.check_decode_plain(B, R, want, shape, tiles.dtype)
    rc, blobs, _, _, _ = one_by_one(0, lambda: B.encode(byte, mask, 0))
    want = M.ref_blobs(R, byte, mask, 0)
    assert rc == 0 and blobs == want
    one_by_one(2, lambda: B.decode(want, shape, np.uint8))
    M.check_decode_plain(B, R, want, shape, np.uint8)
    # 8-bit, every pixel valid: the unmasked call's own path, which has no such limit and no such note
    rc, blobs, _, _, _ = B.encode(byte, None, 0, unmasked_call=True)
    assert rc == 0 and blobs == M.ref_blobs(R, byte, None, 0)
    # band stacks, wide and 8-bit
    for stack, nm in ((np.stack([wide[0], wide[0][::-1]])[None].copy(), 1), (np.stack([byte[0], byte[0][::-1]])[None].copy(), 0)):
        m = mask if nm else None
        want = one_by_one(0, lambda: T.check_encode(B, R, stack, m, 0, cap_counters=False))
        one_by_one(2, lambda: B.decode_bands(want, (2, r, c), stack.dtype, nm))
        T.check_decode(B, R, want, (2, r, c), stack.dtype, nm, cap_counters=False)
