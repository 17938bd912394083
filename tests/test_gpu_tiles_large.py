"""Tile batches with tiles beyond 131 072 pixels or 4 096 blocks, up to 513 x 513, on the MI355X: every family of the shared driver
(tiles_large_common.py).  Every blob is compared with the reference library's, byte for byte; pixels and valid bytes with the
reference's and the single-blob decoder's; and every tile the families' rules name is counted as done by the batch's own launches --
where such tiles are done one by one inside the call, none is."""
import numpy as np
import pytest

import capi
import tiles_bands_common as T
import tiles_bytes_masked_common as BM
import tiles_large_common as L
import tiles_masked_common as M

pytestmark = [pytest.mark.gpu, pytest.mark.ref]


def _libs():
    import torch    # (before the library is loaded: both then share one HIP runtime)
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    P, R = capi.product(), capi.ref()
    assert P is not None, "lerc_amd/csrc/liblerc_amd.so is not built"
    assert R is not None, "oracle/_ref/libLercRef.so did not travel"
    return P, R


@pytest.fixture()
def batch():
    P, _ = _libs()
    B = T.BandsBatch(P.lib, M.GpuMem())
    yield B
    B.close()


@pytest.mark.parametrize("shape", L.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype,e", [(np.float32, 0.01), (np.uint16, 0)], ids=["float32", "uint16"])
def test_masked_wide(batch, shape, dtype, e):
    L.check_masked_wide(batch, _libs()[1], shape, dtype, e)


@pytest.mark.parametrize("shape", L.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype", [np.uint8, np.int8], ids=["uint8", "int8"])
def test_bytes(batch, shape, dtype):
    L.check_bytes(batch, _libs()[1], shape, dtype)


@pytest.mark.parametrize("shape", L.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype", [np.uint8, np.int8], ids=["uint8", "int8"])
def test_bytes_masked(batch, shape, dtype):
    L.check_bytes_masked(batch, _libs()[1], shape, dtype)


@pytest.mark.parametrize("dtype,nb,with_mask", [(np.uint8, 3, True), (np.uint16, 4, False), (np.uint16, 4, True)], ids=["3xuint8-mask", "4xuint16", "4xuint16-mask"])
def test_band_stacks_513(batch, dtype, nb, with_mask):
    L.check_bands(batch, _libs()[1], dtype, nb, with_mask)


@pytest.mark.parametrize("kind", ["float32", "uint16"])
def test_island_512(batch, kind):
    """a 2 048^2 island cut into 16 tiles of 512 x 512, all valid and partial ones: every tile stays in the batch"""
    R = _libs()[1]
    tiles, masks, e = M.island(kind, 2048, 512)
    n, n_pix, item = len(tiles), tiles[0].size, tiles.itemsize
    assert n == 16
    want = M.ref_blobs(R, tiles, masks, e)
    must = sum(M.must_batch(w, n_pix, item) for w in want)
    assert must == EXPECT_MUST[kind], must
    # (the tiles the rule does not name are the uint16 island's four of 16 x 16 blocks, which the masked family keeps too)
    L.all_in_batch(batch, 0, n, lambda: M.check_encode(batch, R, tiles, masks, e, want=want))
    L.all_in_batch(batch, 0, n, lambda: M.check_encode(batch, R, tiles, masks, e, slot_bytes=L.slot_for(tiles), want=want))
    L.all_in_batch(batch, 2, n, lambda: M.check_decode(batch, R, want, (512, 512), tiles.dtype))


def test_island_512_bytes(batch):
    R = _libs()[1]
    tiles, masks = BM.byte_island(2048, 512)
    n, n_pix = len(tiles), tiles[0].size
    assert n == 16
    want = M.ref_blobs(R, tiles, masks, 0)
    must = sum(BM.must_batch(w, n_pix) for w in want)
    assert must == EXPECT_MUST["uint8"], must
    L.all_in_batch(batch, 0, n, lambda: BM.check_encode(batch, R, tiles, masks, want=want))
    L.all_in_batch(batch, 0, n, lambda: BM.check_encode(batch, R, tiles, masks, want=want, slot_bytes=L.slot_for(tiles)))
    L.all_in_batch(batch, 2, n, lambda: BM.check_decode(batch, R, want, (512, 512), np.uint8, masks))


# what the reference's blobs of the 2 048^2 islands ask for (of 16 tiles), checked on the CPU
EXPECT_MUST = {"float32": 16, "uint16": 12, "uint8": 16}


@pytest.mark.parametrize("dtype,e", [(np.float32, 0.01), (np.uint16, 0)], ids=["float32", "uint16"])
def test_unmasked_wide_512(batch, dtype, e):
    """the unmasked call on wide types goes through the one-launch tile encoder, which never had the batches' size limit"""
    R = _libs()[1]
    rng = np.random.default_rng(113)
    tiles = np.stack([L.terrain(rng, 512, 512) for _ in range(3)])
    tiles = tiles.astype(np.float32) if dtype == np.float32 else np.round(tiles).astype(dtype)
    (out, batch_n, single) = L.counted(batch, 0, lambda: batch.encode(tiles, None, e, unmasked_call=True))
    rc, blobs, offs, sizes, used = out
    want = M.ref_blobs(R, tiles, None, e)
    assert rc == 0 and blobs == want
    assert (batch_n, single) == (3, 0), (batch_n, single, batch.note())
    rc, pix, _ = batch.decode(want, (512, 512), dtype, want_valid=False)
    assert rc == 0
    for t in range(3):
        rc_r, p_r, _ = R.decode(want[t], want_masks=0)
        assert rc_r == 0 and np.array_equal(pix[t].view(np.uint8), p_r.reshape(512, 512).view(np.uint8))


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8], ids=["uint16", "uint8"])
def test_sub_batches(batch, dtype):
    L.check_sub_batches(batch, _libs()[1], dtype)


def test_errors_513(batch):
    L.check_errors(batch, _libs()[1], n_fuzz=5)


def test_long_runs_513(batch):
    L.check_long_runs(batch, _libs()[1])


def test_above_the_limit(batch):
    L.check_above_the_limit(batch, _libs()[1], (1024, 1024))
