"""Masked tile batches on the MI355X: the island mosaic (a 16 x 16 grid of 256^2 tiles cut from a 4096^2 raster, a disc of valid
pixels minus salt holes), ragged tiles with both parities of the mask section's length, fallbacks, errors, a soak.  Every blob is
compared with the reference library's, byte for byte; what the batch may hand back is computed from the reference's own blobs
(tiles_masked_common.must_batch)."""
import numpy as np
import pytest

import capi
import tiles_masked_common as C

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
def test_island_encode_and_decode(batch, kind):
    _, R = _libs()
    tiles, masks, e = C.island(kind)
    assert len(tiles) == 256
    n_valid = masks.reshape(256, -1).sum(axis=1)
    assert (int((n_valid == 65536).sum()), int((n_valid == 0).sum())) == (98, 76)
    want = C.check_encode(batch, R, tiles, masks, e)                                            # packed
    C.check_encode(batch, R, tiles, masks, e, slot_bytes=tiles[0].nbytes + 16384 + 1024, want=want)    # slotted
    # blobs written by the reference, and the product's own (the same bytes, laid out by the product)
    C.check_decode(batch, R, want, (256, 256), tiles.dtype)
    rc, own, _, _, _ = batch.encode(tiles, masks, e)
    assert rc == 0 and own == want
    cap = 76 + (8 if kind == "float32" else 16)
    c = batch.counters()
    assert c[1] <= 3 * cap and c[3] <= cap, c    # (three encodes, one decode on this context)


def test_ragged_and_parity(batch):
    _, R = _libs()
    C.check_ragged(batch, R, 24, 257, 257, np.int32, 3)
    C.check_ragged(batch, R, 24, 40, 56, np.int16, 4)


def test_fallbacks(batch):
    _, R = _libs()
    C.check_fallbacks(batch, R)


def test_float_decisions_stay_in_the_batch(batch):
    _, R = _libs()
    C.check_float_decisions(batch, R, r=96, c=120)


def test_unaligned_arena(batch):
    _, R = _libs()
    C.check_unaligned_arena(batch, R)


def test_fresh_contexts():
    P, R = _libs()
    C.check_fresh_contexts(P.lib, C.GpuMem(), R, rounds=8, n=24, r=128, c=128)


def test_errors(batch):
    _, R = _libs()
    C.check_errors(batch, R, n_fuzz=8)


def test_soak():
    P, R = _libs()
    C.check_soak(P.lib, C.GpuMem(), R, rounds=20, max_tiles=96, r=64, c=64)


def test_sub_batches(batch):
    """sub-batches of 3 + 3 + 1 tiles, a tile handed back in the second one"""
    _, R = _libs()
    C.check_sub_batches(batch, R)
