"""Band stack tile batches on the MI355X: every tile's blob is compared with the reference library's, byte for byte, packed, slotted,
at an odd arena address and in an arena of exactly the bytes used; pixels and valid bytes with the reference's and the single-blob
decoder's; what a batch may hand back is computed from the reference's own blobs (tiles_bands_common.must_batch)."""
import numpy as np
import pytest

import capi
import tiles_bands_common as C

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
    B = C.BandsBatch(P.lib, C.GpuMem())
    yield B
    B.close()


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("nb", [2, 4])
@pytest.mark.parametrize("dtype,e", C.WIDE)
def test_parity_wide(batch, dtype, e, nb, with_mask):
    C.check_parity_wide(batch, _libs()[1], dtype, e, nb, with_mask, n=7)


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("dtype", [np.uint8, np.int8])
def test_parity_bytes(batch, dtype, with_mask):
    C.check_parity_bytes(batch, _libs()[1], dtype, with_mask)


@pytest.mark.parametrize("r,c", [(33, 41), (17, 9)])
def test_parity_ragged(batch, r, c):
    C.check_parity_wide(batch, _libs()[1], np.uint16, 0, 3, True, n=6, r=r, c=c, seed=3)
    C.check_parity_wide(batch, _libs()[1], np.float32, 0.01, 3, False, n=4, r=r, c=c, seed=4)


def test_parity_bytes_256(batch):
    C.check_parity_bytes(batch, _libs()[1], np.uint8, True, n=4, r=256, c=256)


def test_parity_wide_256(batch):
    """the largest tile shape of the mosaics: 256 x 256, four uint16 bands under one mask"""
    C.check_parity_wide(batch, _libs()[1], np.uint16, 0, 4, True, n=4, r=256, c=256, seed=9)


def test_mix_inside_a_tile_wide(batch):
    C.check_mix_wide(batch, _libs()[1])


def test_mix_inside_a_tile_bytes(batch):
    C.check_mix_bytes(batch, _libs()[1])


def test_sub_batches(batch):
    C.check_sub_batches(batch, _libs()[1])


def test_sub_batches_wide(batch):
    C.check_sub_batches_wide(batch, _libs()[1])


def test_hand_backs(batch):
    C.check_hand_backs(batch, _libs()[1])


def test_errors(batch):
    C.check_errors(batch, _libs()[1], n_fuzz=4)


def test_errors_bytes(batch):
    C.check_errors(batch, _libs()[1], n_fuzz=4, dtype=np.uint8)


def test_one_band(batch):
    C.check_one_band(batch, _libs()[1])


def test_soak():
    P, R = _libs()
    C.check_soak(P.lib, C.GpuMem(), R, rounds=12, fresh_rounds=3, max_tiles=11)
