"""Shared by test_sim_tiles_bytes.py (CPU emulator library) and test_gpu_tiles_bytes.py (MI355X): the 8-bit tile batches -- int8 /
uint8 tiles, every pixel valid, lossless -- through the tile batch calls of include/lerc_amd_device.h, and the rule for what such a
batch may hand back.  Drivers, memory and the re-signing of damaged blobs come from tiles_masked_common.py.
"""
import struct

import numpy as np

import tiles_masked_common as M
from tiles_masked_common import Batch, HostMem, GpuMem, check_layout, ref_blobs, resign, sub_batches_of    # noqa: F401

AT = 96    # the one-sweep byte of an all-valid single-band codec 6 byte blob; the mode byte follows


def must_batch(blob, n_pix):
    """the batch's own launches must take a tile when its reference blob is not constant, not one sweep, and either (a) a Huffman mode
    at 1.5 bits a pixel or more, or (b) tiling with 8 x 8 blocks where the low-bit-rate retry condition is false"""
    z_min, z_max = struct.unpack_from("<dd", blob, 58)
    if z_min == z_max or blob[AT] != 0:
        return False
    mode, mb, blob_size = blob[AT + 1], struct.unpack_from("<i", blob, 30)[0], struct.unpack_from("<i", blob, 34)[0]
    data = blob_size - (AT + 2)
    if mode in (1, 2):
        return data * 8 >= 1.5 * n_pix
    if mode == 0 and mb == 8:
        return not (data * 8 < 1.5 * n_pix and data < 4 * n_pix)
    return False


def modes(blobs):
    """-> counts of (delta Huffman, Huffman, tiling) among blobs that are neither constant nor one sweep"""
    out = [0, 0, 0]
    for b in blobs:
        z_min, z_max = struct.unpack_from("<dd", b, 58)
        if z_min != z_max and b[AT] == 0:
            out[{1: 0, 2: 1, 0: 2}[b[AT + 1]]] += 1
    return out


def byte_mosaic(size, tile, dtype=np.uint8):
    from lerc_amd import synth
    t = synth.byte_mosaic(size, tile)
    return t if dtype == np.uint8 else (t.astype(np.int16) - 128).astype(np.int8)


def variety(r, c, seed=5):
    """-> (tiles uint8 [11, r, c], names): the kinds of content the issue lists, each shape and kind in the same class"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:r, 0:c]
    smooth = 128 + 100 * np.sin(yy / 23.0) * np.cos(xx / 31.0)
    sparse = np.zeros((r, c))
    sparse[rng.random((r, c)) < 0.002] = 9
    two = rng.choice(256, 2, replace=False)
    kinds = [
        ("noise", rng.integers(0, 256, (r, c))),
        ("noise16", rng.integers(0, 16, (r, c)) * 16),
        ("palette", rng.choice([3, 80, 81, 200, 255], (r, c), p=[.6, .2, .1, .05, .05])),
        ("smooth", smooth),
        ("smooth+noise", smooth + rng.normal(0, 2, (r, c))),
        ("constant", np.full((r, c), 77)),
        ("checker", np.where(((yy // 4) + (xx // 4)) % 2 == 0, 0, 200)),
        ("sparse", sparse),
        ("stripes", np.where(xx % 2 == 0, 10, 250) + 0 * yy),
        ("ramp", (xx // 2 + yy // 3) % 256),
        ("two", two[rng.integers(0, 2, (r, c))]),
    ]
    tiles = np.stack([np.clip(np.round(k[1]), 0, 255).astype(np.uint8) for k in kinds])
    return tiles, [k[0] for k in kinds]


def tie_tiles(ks=(3, 5, 6, 7, 12, 33, 100, 255, 256), side=64, seed=9):
    """side x side tiles whose pixels are a seeded permutation of k values in equal counts (as equal as side^2 / k allows): the code
    book's tie-break shows in the blob"""
    rng = np.random.default_rng(seed)
    out = []
    for k in ks:
        vals = rng.permutation(256)[:k] if k < 256 else np.arange(256)
        px = np.resize(vals, side * side)
        out.append(rng.permutation(px).reshape(side, side).astype(np.uint8))
    return np.stack(out)


def slot_for(tiles):
    return (tiles[0].nbytes + tiles[0].size // 4 + 1024 + 15) & ~15


def check_encode(B, R, tiles, want=None, slot_bytes=0, arena_shift=0, unmasked_call=False):
    """every blob equals the reference's, the layout holds, the counters respect the cap -> the reference's blobs"""
    want = want or ref_blobs(R, tiles, None, 0)
    n, n_pix = len(tiles), tiles[0].size
    c0 = B.counters()
    rc, blobs, offs, sizes, used = B.encode(tiles, None, 0, slot_bytes=slot_bytes, arena_shift=arena_shift, unmasked_call=unmasked_call)
    c1 = B.counters()
    assert rc == 0, (rc, B.note())
    for t in range(n):
        assert blobs[t] == want[t], "tile %d: %d bytes, the reference makes %d (%s)" % (t, len(blobs[t]), len(want[t]), B.note())
    check_layout(offs, sizes, used, slot_bytes)
    batch, single = c1[0] - c0[0], c1[1] - c0[1]
    must = sum(must_batch(w, n_pix) for w in want)
    print("encode: %d tiles, %d by the batch's launches, %d one by one; the reference's blobs ask for at least %d in the batch; modes %s"
          % (n, batch, single, must, modes(want)))
    assert batch + single == n
    assert single <= n - must, (single, n - must, B.note())
    return want


def check_decode(B, R, blobs, shape, dtype):
    """pixels equal the reference's lerc_decode and lerc_amd_decode_device, tile by tile; the counters respect the cap"""
    n = len(blobs)
    c0 = B.counters()
    rc, pix, _ = B.decode(blobs, shape, dtype, want_valid=False)
    c1 = B.counters()
    assert rc == 0, (rc, B.note())
    for t in range(n):
        rc_r, p_r, _ = R.decode(blobs[t], want_masks=1)
        assert rc_r == 0
        assert np.array_equal(pix[t].view(np.uint8), p_r.reshape(shape).view(np.uint8)), "tile %d: pixels differ from the reference's" % t
        rc_1, p_1, _ = B.decode_one(blobs[t], shape, dtype)
        assert rc_1 == 0
        assert np.array_equal(pix[t].view(np.uint8), p_1.view(np.uint8)), "tile %d: pixels differ from lerc_amd_decode_device's" % t
    batch, single = c1[2] - c0[2], c1[3] - c0[3]
    must = sum(must_batch(b, shape[0] * shape[1]) for b in blobs)
    print("decode: %d tiles, %d by the batch's launches, %d one by one; at least %d asked for" % (n, batch, single, must))
    assert batch + single == n
    assert single <= n - must, (single, n - must, B.note())
    return pix


def check_round_trip(B, R, tiles, expect_must=None):
    """packed, slotted, through the unmasked call, at an odd arena address; then both decodes"""
    want = check_encode(B, R, tiles)
    if expect_must is not None:
        assert sum(must_batch(w, tiles[0].size) for w in want) == expect_must
    check_encode(B, R, tiles, want=want, slot_bytes=slot_for(tiles))
    check_encode(B, R, tiles, want=want, unmasked_call=True)
    check_encode(B, R, tiles, want=want, arena_shift=1)
    pix = check_decode(B, R, want, tiles[0].shape, tiles.dtype)
    assert np.array_equal(pix, tiles)
    rc, own, _, _, _ = B.encode(tiles, None, 0)
    assert rc == 0 and own == want
    return want


def check_errors(B, R, tiles, n_fuzz):
    """tiles: a batch whose tile 2 is a Huffman tile the batch must take"""
    n, shape, dtype = len(tiles), tiles[0].shape, tiles.dtype
    want = ref_blobs(R, tiles, None, 0)
    assert want[2][AT + 1] in (1, 2) and must_batch(want[2], tiles[0].size)
    rc, blobs, offs, sizes, used = B.encode(tiles, None, 0)
    assert rc == 0 and blobs == want
    # an arena one byte too small, a slot too small
    assert B.encode(tiles, None, 0, arena_cap=used - 1)[0] == 3
    assert B.encode(tiles, None, 0, arena_cap=used)[0] == 0
    small = (max(len(w) for w in want) - 1) & ~15
    assert B.encode(tiles, None, 0, slot_bytes=small)[0] == 3
    assert B.encode(tiles, None, 0, slot_bytes=small + 16)[0] == 0
    rc, good, _ = B.decode(want, shape, dtype, want_valid=False)
    assert rc == 0 and np.array_equal(good, tiles)
    others = [t for t in range(n) if t != 2]
    # one flipped bit: Failed(1) and zeros for that tile, the neighbours untouched -- in the code table, in the pixel stream
    for where in (AT + 2 + 20, len(want[2]) - 9):
        bad = bytearray(want[2])
        bad[where] ^= 0x10
        damaged = list(want)
        damaged[2] = bytes(bad)
        rc, pix, _ = B.decode(damaged, shape, dtype, want_valid=False)
        assert rc == 1, rc
        assert not pix[2].any()
        for t in others:
            assert np.array_equal(pix[t], good[t])
    # damage behind a checksum that is right again: the status and the pixels of the single-blob decoder, never anything else
    rng = np.random.default_rng(13)
    table_end = AT + 2 + 16 + 3 + 200
    for k in range(n_fuzz):
        bad = bytearray(want[2])
        where = int(rng.integers(AT - 2, table_end if k % 2 else len(bad)))
        bad[where] ^= 1 << int(rng.integers(0, 8))
        damaged = list(want)
        damaged[2] = resign(bytes(bad))
        rc, pix, _ = B.decode(damaged, shape, dtype, want_valid=False)
        rc_1, p_1, _ = B.decode_one(damaged[2], shape, dtype)
        assert rc == rc_1, (k, where, rc, rc_1, B.note())
        if rc_1 == 0:
            assert np.array_equal(pix[2], p_1), (k, where)
        else:
            assert not pix[2].any()
        for t in others:
            assert np.array_equal(pix[t], good[t])


def check_soak(L, mem, R, rounds, max_tiles, size, tile):
    """byte batches of random size on ONE context, between float32 / uint16 unmasked batches and masked batches; then a fresh context
    per batch for a few rounds"""
    rng = np.random.default_rng(29)
    src = byte_mosaic(size, tile)
    r = c = tile
    B = Batch(L, mem)
    try:
        for k in range(rounds):
            n = int(rng.integers(1, max_tiles + 1))
            pick = rng.choice(len(src), n, replace=False)
            tiles = src[pick] if k % 2 == 0 else (src[pick].astype(np.int16) - 128).astype(np.int8)
            want = check_encode(B, R, tiles, slot_bytes=0 if k % 3 else slot_for(tiles))
            assert np.array_equal(check_decode(B, R, want, (r, c), tiles.dtype), tiles)
            other = M.terrain_int(rng, 3, r, c, np.int32)
            other = (other + rng.normal(0, 0.3, other.shape)).astype(np.float32) if k % 2 else other.astype(np.uint16)
            e = 0.01 if k % 2 else 0
            rc_u, blobs_u, _, _, _ = B.encode(other, None, e, unmasked_call=True)
            assert rc_u == 0 and blobs_u == ref_blobs(R, other, None, e)
            masks = M.random_blob_mask(rng, 3, r, c)
            rc_m, blobs_m, _, _, _ = B.encode(other, masks, e)
            assert rc_m == 0 and blobs_m == ref_blobs(R, other, masks, e)
    finally:
        B.close()
    for k in range(3):
        tiles = src[k:k + 4]
        B = Batch(L, mem)
        try:
            want = check_encode(B, R, tiles)
        finally:
            B.close()
        B = Batch(L, mem)
        try:
            check_decode(B, R, want, (r, c), np.uint8)
        finally:
            B.close()


def check_sub_batches(B, R, r=40, c=56):
    """7 tiles in sub-batches of 3 + 3 + 1 (LERC_AMD_TEST_TILE_SUBBATCH), packed and slotted: the first tile and the arena's base of a
    LATER sub-batch, and a tile done again behind one -- tile 4, in the second sub-batch, is constant: the batch hands it back, each way"""
    rng = np.random.default_rng(47)
    n = 7
    yy, xx = np.mgrid[0:r, 0:c]
    tiles = np.stack([np.clip(np.round(128 + 100 * np.sin(yy / rng.uniform(9, 40)) * np.cos(xx / rng.uniform(9, 40)) + rng.normal(0, rng.uniform(2, 6), (r, c))),
                              0, 255).astype(np.uint8) for _ in range(n)])
    tiles[4][:] = 77
    want = ref_blobs(R, tiles, None, 0)
    assert sum(must_batch(w, r * c) for w in want) == n - 1, "every tile but the constant one is the batch's own"
    with sub_batches_of(3):
        for slot in (0, slot_for(tiles)):
            c0 = B.counters()
            check_encode(B, R, tiles, want=want, slot_bytes=slot)
            c1 = B.counters()
            assert (c1[0] - c0[0], c1[1] - c0[1]) == (n - 1, 1), (c0, c1, B.note())
        c0 = B.counters()
        assert np.array_equal(check_decode(B, R, want, (r, c), np.uint8), tiles)
        c1 = B.counters()
        assert (c1[2] - c0[2], c1[3] - c0[3]) == (n - 1, 1), (c0, c1, B.note())
