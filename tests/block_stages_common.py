"""The block stages shared by the general kernels and the tile batches (tile_encode_dev.h, tile_decode_dev.h): the smallest rasters at
which a stage's rules decide the bytes, each checked against the oracle -- the blob byte for byte, the decode of it pixel for pixel --
and, for one value a pixel, through the general call and through the tile batch call alike (both equal the oracle's blob, so both
hold the same block stream).  What a case is named for is read from the oracle's blob and asserted (property()).
Not here, because the lists of tests/cases.py already reach them in the emulator's and the GPU's parity tests: blobs of codec
2 .. 5 (old_codec_cases: old bit layout, 15-bit signature), slice differences that win and lose on terrain (u16-depth4, i32-depth4,
u16-depth3-identical, u16-depth3-mask), 16 x 16 blocks with every pixel valid (f32-mb16, f32-smooth-mb16)."""
import struct

import numpy as np

import tiles_masked_common as TM

HDR = {4: 66, 5: 66, 6: 90}


def edge_raster(r, c, dt):
    """r x c, r = 2 * 8 + 1 ... rows, c = 8 + 1 ... columns: edge blocks in both directions.  Block (0, 0) is left empty by the mask,
    (0, 1) keeps a single valid pixel, (1, 0) exactly 4 and (1, 1) exactly 5 -- three equal values and a far one, the `n > 4` edge of
    the LUT rule -- and the block at row 16, columns 0 .. 7 holds 0 0 0 0 0 7 9 500 in its first row: with the "previous value" 0 in
    front (every pixel valid) 5 of 8 are the same as the previous one and the LUT is tried, behind a mask 4 of 8 are and it is not."""
    rng = np.random.default_rng(r * 100 + c)
    x = (1000 + 50 * np.sin(np.arange(c)[None, :] / 3.0) + 20 * np.cos(np.arange(r)[:, None] / 5.0) + rng.integers(0, 4, (r, c))).astype(dt)
    m = np.ones((r, c), np.uint8)
    m[0:8, 0:8] = 0
    m[0:8, 8:16] = 0
    m[3, 8] = 1
    m[8:16, 0:8] = 0
    m[8:16, 8:16] = 0
    few = np.array([100, 100, 100, 900, 100], dt)
    for k, (i, j) in enumerate([(9, 1), (9, 5), (12, 2), (15, 7)]):
        m[i, j] = 1
        x[i, j] = few[k]
    for k in range(5):
        m[8 + k, 8] = 1
        x[8 + k, 8] = [100, 100, 100, 100, 900][k]
    x[16, 0:8] = np.array([0, 0, 0, 0, 0, 7, 9, 500], dt)
    return x, m


def cases():
    """-> [(name, array, MaxZError, keywords of capi's encode, property or None)]"""
    rng = np.random.default_rng(5)
    out = []
    for (r, c) in ((17, 9), (33, 18)):
        for dt, e in ((np.int16, 0), (np.float32, 0.01)):
            x, m = edge_raster(r, c, dt)
            out.append((f"edges-{r}x{c}-{np.dtype(dt).name}-masked", x, e, dict(mask=m), "edges-masked"))
            out.append((f"edges-{r}x{c}-{np.dtype(dt).name}-allvalid", x, e, {}, "edges-allvalid"))
    # few values over a wide range, most of them equal to the one in front: LUT blocks
    few = rng.choice(np.array([0, 5, 100000], np.int32), (16, 24), p=[0.8, 0.1, 0.1])
    out.append(("fewvalues-int32", few, 0, {}, "lut"))
    out.append(("fewvalues-int32-masked", few, 0, dict(mask=(rng.random((16, 24)) > 0.2).astype(np.uint8)), "lut"))
    # a 2 x 2 corner block 0 0 0 900 with every pixel valid: the only kind of block at which `n > 4` alone decides against the LUT
    # (behind a mask the first pixel never counts as "the same", and 2 * same > 4 cannot hold)
    corner = (200 + rng.integers(0, 50, (10, 10))).astype(np.int16)
    corner[8:10, 8:10] = [[0, 0], [0, 900]]
    out.append(("corner-2x2-int16-allvalid", corner, 0, {}, "corner4"))
    # three slices: the second is the first + 7 (its difference blocks are constant), the third independent noise
    base = (1500 + 300 * np.sin(np.arange(48)[None, :] / 7.0) * np.cos(np.arange(40)[:, None] / 9.0) + rng.integers(0, 30, (40, 48))).astype(np.uint16)
    cube = np.stack([base, base + 7, rng.integers(0, 60000, (40, 48)).astype(np.uint16)], axis=-1)
    out.append(("depth3-uint16", cube, 0, dict(n_depth=3), "differences"))
    out.append(("depth3-uint16-masked", cube, 0, dict(n_depth=3, mask=(rng.random((40, 48)) > 0.3).astype(np.uint8)), "differences"))
    # slice differences outside the int range: every difference block is refused (checkOverflow)
    lo = rng.integers(0, 1000, (24, 17))
    out.append(("overflow-int32", np.stack([lo - 2_000_000_000, lo + 2_000_000_000], axis=-1).astype(np.int32), 0, dict(n_depth=2), "no differences"))
    out.append(("overflow-uint32", np.stack([lo, lo + 4_000_000_000], axis=-1).astype(np.uint32), 0, dict(n_depth=2), "no differences"))
    # a smooth ramp: 16 x 16 blocks win
    ramp = (100 + 0.0005 * np.arange(48)[None, :] * np.ones((40, 1))).astype(np.float32)
    mr = np.ones((40, 48), np.uint8)
    mr[5:9, 30:41] = 0
    out.append(("ramp-mb16-allvalid", ramp, 0.01, {}, "mb16"))
    out.append(("ramp-mb16-masked", ramp, 0.01, dict(mask=mr), "mb16"))
    return out


DT_CODE = {"int8": 0, "uint8": 1, "int16": 2, "uint16": 3, "int32": 4, "uint32": 5, "float32": 6, "float64": 7}
DT_SIZE = [1, 1, 2, 2, 4, 4, 4, 8]


def type_used(dt, tc):
    """Lerc2::GetDataTypeUsed (Lerc2.h:528-542)"""
    if dt in (2, 4):
        return dt - tc
    if dt in (3, 5):
        return dt - 2 * tc
    if dt == 6:
        return dt if tc == 0 else (2 if tc == 1 else 1)
    if dt == 7:
        return dt if tc == 0 else dt - 2 * tc + 1
    return dt


def walk_blocks(blob, arr, n_depth, mask):
    """The block stream of a codec 6 blob of tiles, read as Lerc2::ReadTiles / ReadTile read it (Lerc2.cpp:1672-1713, :2025-2230):
    -> {(block row, block column, slice): dict(mode, diff, lut, n)}; mode 0 raw, 1 bit-stuffed, 2 all zero, 3 constant"""
    assert blob[:6] == b"Lerc2 " and struct.unpack_from("<i", blob, 6)[0] == 6
    rows, cols, nd, _, mb, size, dt = struct.unpack_from("<7i", blob, 14)
    assert (rows, cols, nd, size, dt) == (arr.shape[0], arr.shape[1], n_depth, len(blob), DT_CODE[arr.dtype.name])
    at = HDR[6]
    at += 4 + struct.unpack_from("<i", blob, at)[0]    # the mask
    at += 2 * nd * DT_SIZE[dt]                          # the slices' ranges
    assert blob[at] == 0, "written in one sweep: no tiles"
    at += 1
    valid = np.ones((rows, cols), bool) if mask is None else mask != 0
    out = {}
    for it in range((rows + mb - 1) // mb):
        for jt in range((cols + mb - 1) // mb):
            n = int(valid[it * mb:(it + 1) * mb, jt * mb:(jt + 1) * mb].sum())
            for d in range(nd):
                flag = blob[at]
                assert (flag >> 2) & 14 == ((jt * mb) >> 3) & 14, "column signature"
                mode, diff, tc = flag & 3, (flag >> 2) & 1, flag >> 6
                lut = False
                ln = 1
                if mode == 0:
                    ln += n * DT_SIZE[dt]
                elif mode != 2:
                    ln += DT_SIZE[type_used(4 if diff and dt < 6 else dt, tc)]
                    if mode == 1:
                        b0 = blob[at + ln]
                        cb = 4 if b0 >> 6 == 0 else 3 - (b0 >> 6)
                        nb, lut = b0 & 31, bool(b0 & 32)
                        cnt = int.from_bytes(blob[at + ln + 1:at + ln + 1 + cb], "little")
                        assert cnt == n
                        ln += 1 + cb
                        if not lut:
                            ln += (cnt * nb + 7) // 8
                        else:
                            n_lut = blob[at + ln] - 1
                            ln += 1 + (n_lut * nb + 7) // 8 + (cnt * n_lut.bit_length() + 7) // 8
                assert n > 0 or mode == 2
                out[(it, jt, d)] = dict(mode=mode, diff=bool(diff), lut=lut, n=n)
                at += ln
    assert at == len(blob), "the walk ends where the blob ends"
    return out


def check_property(name, arr, kw, prop, blob):
    """what the case is named for, read from the oracle's blob: the micro-block size from the header, the difference bit and the
    LUT bit from the blocks' own first bytes"""
    if prop is None:
        return
    mb = struct.unpack_from("<i", blob, 30)[0]
    if prop == "mb16":
        assert mb == 16, name
        return
    assert mb == 8, name
    blocks = walk_blocks(blob, arr, kw.get("n_depth", 1), kw.get("mask"))
    full = [k for k, b in blocks.items() if b["n"] > 0]
    if prop == "differences":    # slice 1 = slice 0 + 7: the difference wins everywhere; slice 2 is noise of its own: it loses everywhere
        assert full and all(blocks[k]["diff"] == (k[2] == 1) for k in full), name
    elif prop == "no differences":
        assert full and not any(blocks[k]["diff"] for k in full), name
    elif prop == "lut":
        assert any(blocks[k]["lut"] for k in full), name
    elif prop == "edges-masked":    # no pixel, one, four (n > 4 fails), five (LUT)
        assert [blocks[(i, j, 0)]["n"] for (i, j) in ((0, 0), (0, 1), (1, 0), (1, 1))] == [0, 1, 4, 5], name
        assert blocks[(0, 0, 0)]["mode"] == 2 and not blocks[(1, 0, 0)]["lut"] and blocks[(1, 1, 0)]["lut"], name
        if arr.shape[0] == 17:     # the one-row block 0 0 0 0 0 7 9 500 behind a mask: the first pixel is not "the same", 4 of 8
            assert blocks[(2, 0, 0)]["n"] == 8 and blocks[(2, 0, 0)]["mode"] == 1 and not blocks[(2, 0, 0)]["lut"], name
    elif prop == "edges-allvalid":
        if arr.shape[0] == 17:     # ... with every pixel valid: 5 of 8 with the 0 in front
            assert blocks[(2, 0, 0)]["n"] == 8 and blocks[(2, 0, 0)]["lut"], name
    elif prop == "corner4":        # 0 0 0 900, every pixel valid: 3 of 4 are the same, and n > 4 keeps the LUT away -- 8 bytes with a
        it, jt = (arr.shape[0] - 1) // 8, (arr.shape[1] - 1) // 8    # LUT, 9 bit-stuffed, which is no shorter than raw: the block is raw
        assert blocks[(it, jt, 0)]["n"] == 4 and blocks[(it, jt, 0)]["mode"] == 0, name
    else:
        raise AssertionError(prop)


def check_case(P, R, batch, name, arr, e, kw, prop):
    """P: the library under test (general calls), R: the oracle, batch: a tiles_masked_common.Batch of the library under test"""
    rc_r, want = R.encode(arr, e, **kw)
    assert rc_r == 0, name
    check_property(name, arr, kw, prop, want)
    rc, blob = P.encode(arr, e, **kw)
    assert rc == 0 and blob == want, (name, "general encode differs from the oracle's")
    d_r, d_p = R.decode(want), P.decode(want)
    assert d_r[0] == d_p[0] == 0, name
    assert np.array_equal(np.asarray(d_r[1]).view(np.uint8), np.asarray(d_p[1]).view(np.uint8)), (name, "general decode differs from the oracle's")
    if "mask" in kw:
        assert np.array_equal(np.asarray(d_r[2]), np.asarray(d_p[2])), name
    if kw.get("n_depth", 1) != 1:
        return
    # the same tile through the tile batch call: the same blob, hence the same block stream, and the same pixels
    mask = kw.get("mask")
    masks = mask[None] if mask is not None else np.ones((1,) + arr.shape, np.uint8)
    c0 = batch.counters()
    rc, blobs, _, _, _ = batch.encode(arr[None].copy(), masks.copy(), e)
    assert rc == 0 and blobs[0] == want, (name, "tile batch encode differs from the oracle's")
    c1 = batch.counters()
    rc, pix, valid = batch.decode([want], arr.shape, arr.dtype)
    assert rc == 0, name
    c2 = batch.counters()
    # (tiles coded by the batch's own launches, tiles handed back one by one: encode, then decode)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 0) and (c2[2] - c1[2], c2[3] - c1[3]) == (1, 0), (name, "the tile left the batch's launches", c0, c1, c2)
    ok = masks[0] != 0
    assert np.array_equal(valid[0] != 0, ok), name
    assert np.array_equal(pix[0][ok].view(np.uint8), np.asarray(d_r[1]).reshape(arr.shape)[ok].view(np.uint8)), (name, "tile batch decode differs from the oracle's")


CASES = cases()
IDS = [c[0] for c in CASES]


def batch_of(lib, mem):
    return TM.Batch(lib, mem)
