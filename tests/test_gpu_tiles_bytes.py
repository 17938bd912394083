"""8-bit tile batches on the MI355X: the byte mosaic (a 16 x 16 grid of 256^2 tiles, one channel of the C4 raster), 64^2 and ragged
257^2 tiles, a variety of content at five shapes, tie tiles, errors, a soak.  Every blob is compared with the reference library's,
byte for byte; what the batch may hand back is computed from the reference's own blobs (tiles_bytes_common.must_batch)."""
import numpy as np
import pytest

import capi
import tiles_bytes_common as C

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


def test_mosaic_encode_and_decode(batch):
    """256 tiles of 256 x 256, all delta Huffman: every one by the batch's launches, each way"""
    _, R = _libs()
    tiles = C.byte_mosaic(4096, 256)
    assert len(tiles) == 256
    want = C.check_round_trip(batch, R, tiles, expect_must=256)
    assert C.modes(want) == [256, 0, 0]
    c = batch.counters()
    assert c[1] == 0 and c[3] == 0, c


@pytest.mark.parametrize("dtype", [np.uint8, np.int8])
def test_mosaic_small_tiles_all_three_modes(batch, dtype):
    _, R = _libs()
    want = C.check_round_trip(batch, R, C.byte_mosaic(384, 32, dtype), expect_must=144)
    m = C.modes(want)
    assert m[0] > 0 and m[1] > 0 and (dtype == np.int8 or m[2] > 0), m


def test_mosaic_64_and_ragged(batch):
    _, R = _libs()
    C.check_round_trip(batch, R, C.byte_mosaic(512, 64), expect_must=64)
    C.check_round_trip(batch, R, C.byte_mosaic(1028, 257), expect_must=16)


@pytest.mark.parametrize("shape", [(256, 256), (257, 257), (64, 64), (65, 65), (40, 56)])
def test_variety(batch, shape):
    _, R = _libs()
    tiles, _ = C.variety(*shape)
    C.check_round_trip(batch, R, tiles)
    C.check_round_trip(batch, R, (tiles.astype(np.int16) - 128).astype(np.int8))


def test_ties(batch):
    _, R = _libs()
    C.check_round_trip(batch, R, C.tie_tiles())


def test_errors(batch):
    _, R = _libs()
    C.check_errors(batch, R, C.byte_mosaic(4096, 256)[:5], n_fuzz=8)


def test_soak():
    P, R = _libs()
    C.check_soak(P.lib, C.GpuMem(), R, rounds=12, max_tiles=64, size=1024, tile=64)


def test_sub_batches(batch):
    """sub-batches of 3 + 3 + 1 tiles, a tile handed back in the second one"""
    _, R = _libs()
    C.check_sub_batches(batch, R)
