"""Masked 8-bit tile batches on the MI355X: the byte island (the byte mosaic under the island mask, 64^2 and 256^2 tiles), the
predictor's corners at 40 x 56 and 65 x 65, ragged 257^2 tiles, sub-batches, errors, a soak.  Every blob is compared with the reference
library's, byte for byte; what the batch may hand back is computed from the reference's own blobs
(tiles_bytes_masked_common.must_batch).  Before masked 8-bit tiles had launches of their own every tile of these batches went one by
one (single == n), so each counter assertion here fails on that code."""
import numpy as np
import pytest

import capi
import tiles_bytes_masked_common as C

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
    B = C.Batch(P.lib, C.GpuMem())
    yield B
    B.close()


@pytest.mark.parametrize("dtype", [np.uint8, np.int8])
def test_island_64(batch, dtype):
    """256 tiles of 64 x 64: 245 (uint8) resp. 247 (int8) are the batch's by the rule -- the others are rim tiles whose few valid
    pixels go one sweep or to 16 x 16 blocks"""
    _, R = _libs()
    tiles, masks = C.byte_island(1024, 64, dtype)
    C.check_round_trip(batch, R, tiles, masks, expect_must=245 if dtype == np.uint8 else 247)


@pytest.mark.parametrize("dtype", [np.uint8, np.int8])
def test_island_256(batch, dtype):
    """64 tiles of 256 x 256 (20 all valid, 12 empty, 32 partial, all delta Huffman): the stream outgrows one 4 096-pixel write
    step and approaches the staged-stream limit; every tile is the batch's, each way"""
    _, R = _libs()
    tiles, masks = C.byte_island(2048, 256, dtype)
    C.check_round_trip(batch, R, tiles, masks, expect_must=64)
    c = batch.counters()
    assert c[1] == 0 and c[3] == 0, c


@pytest.mark.parametrize("shape", [(40, 56), (65, 65)])
def test_predictor_corners(batch, shape):
    _, R = _libs()
    C.check_corners(batch, R, *shape)
    C.check_corners(batch, R, *shape, dtype=np.int8)


def test_ragged_257(batch):
    """the ragged edge, more than 65 536 pixels, mask bits that cross byte boundaries at k - width"""
    _, R = _libs()
    rng = np.random.default_rng(71)
    tiles = C.C.byte_mosaic(1028, 257)[:4]
    masks = C.M.random_blob_mask(rng, 4, 257, 257)
    C.check_round_trip(batch, R, tiles, masks, expect_must=4)


def test_sub_batches(batch):
    _, R = _libs()
    C.check_sub_batches(batch, R)


def test_errors(batch):
    _, R = _libs()
    C.check_errors(batch, R, n_fuzz=8)


def test_soak():
    P, R = _libs()
    C.check_soak(P.lib, C.GpuMem(), R, rounds=8, max_tiles=32, size=1024, tile=64)
