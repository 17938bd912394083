"""Depth tile batches on the MI355X: every tile's blob is compared with the reference library's lerc_encode(nDepth), byte for byte,
packed and slotted; pixels and valid bytes with the reference's and the single-blob decoder's; lerc_amd_tile_batch_counters must show
every tile in the batch's own launches unless the test is about a hand-back (tiles_depth_common.py)."""
import numpy as np
import pytest

import capi
import tiles_depth_common as C

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
    B = C.DepthBatch(P.lib, C.GpuMem())
    yield B
    B.close()


@pytest.mark.parametrize("slotted", [False, True])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("d", [2, 3, 4, 8])
@pytest.mark.parametrize("dtype,e", C.TYPES)
def test_parity(batch, dtype, e, d, with_mask, slotted):
    C.check_parity(batch, _libs()[1], dtype, e, d, with_mask, slotted)


@pytest.mark.parametrize("dtype,e", C.TYPES)
def test_parity_shapes(batch, dtype, e):
    C.check_parity(batch, _libs()[1], dtype, e, 3, True, False, n=12, r=17, c=9, seed=5)
    C.check_parity(batch, _libs()[1], dtype, e, 2, True, True, n=4, r=64, c=64, seed=6)


def test_slice_differences(batch):
    C.check_slice_differences(batch, _libs()[1])


def test_every_kind(batch):
    C.check_kinds(batch, _libs()[1])


def test_hand_backs(batch):
    C.check_hand_backs(batch, _libs()[1])


def test_sub_batches(batch):
    C.check_sub_batches(batch, _libs()[1])


def test_depth_one_is_the_masked_call(batch):
    C.check_depth_one(batch, _libs()[1])


def test_large_form(batch):
    C.check_large(batch, _libs()[1])


def test_boundary(batch):
    C.check_boundary(batch)
