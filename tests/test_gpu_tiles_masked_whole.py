"""Masked tile batches on the MI355X whose empty, constant, one-sweep and 16 x 16 tiles stay inside the batch's launches: the island
mosaic (76 of its 256 tiles are empty), a mosaic of every kind of blob for all six types and ragged shapes, damaged blobs of the
new kinds, capacity, a NaN tile, one context.  Every blob is the reference library's, byte for byte; in a batch, as many tiles are
done one by one as have a NaN at a valid pixel (tiles_masked_whole_common.py).

Each test is meant to be run in a process of its own under a time limit (python -m pytest "file::test" under timeout)."""
import numpy as np
import pytest

import capi
import tiles_masked_common as C
import tiles_masked_whole_common as W

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


@pytest.mark.parametrize("kind", ["float32", "uint16"])
def test_island_nothing_leaves(batch, kind):
    """the 256-tile mosaic: 98 tiles all valid, 76 empty, 82 partial -- none is done one by one, each way, packed and slotted"""
    _, R = _libs()
    W.check_island(batch, R, kind, 4096, 256, n_empty=76)


@pytest.mark.parametrize("dtype", W.TYPES, ids=lambda d: np.dtype(d).name)
def test_kinds(batch, dtype):
    _, R = _libs()
    for r, c in ((40, 56), (65, 65), (257, 257), (8, 8)):
        W.check_kinds(batch, R, dtype, r, c)


@pytest.mark.parametrize("dtype", [np.float32, np.uint16], ids=lambda d: np.dtype(d).name)
def test_damage(batch, dtype):
    _, R = _libs()
    W.check_damage(batch, R, dtype, 40, 56, n_fuzz=8)


def test_capacity(batch):
    _, R = _libs()
    W.check_capacity(batch, R, np.int32, 65, 65)
    W.check_capacity(batch, R, np.float32, 40, 56)


def test_nan_tile_alone_leaves(batch):
    _, R = _libs()
    W.check_nan(batch, R, 65, 65)


def test_one_context():
    P, R = _libs()
    W.check_one_context(P.lib, C.GpuMem(), R, rounds=12, r=64, c=64)
