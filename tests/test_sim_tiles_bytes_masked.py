"""Masked 8-bit tile batches (int8 / uint8 tiles with a byte mask per tile, lossless, through lerc_amd_encode_tiles_device_masked and
lerc_amd_decode_tiles_device_masked) on the CPU emulator library, with small tiles: the checks of tests/test_gpu_tiles_bytes_masked.py
(tiles_bytes_masked_common.py), against the real reference where it is built, else against the oracle.  The batch kernels wait for
no other workgroup, so the emulator runs the product's own path."""
import os
import subprocess

import numpy as np
import pytest

import capi
import tiles_bytes_masked_common as C


@pytest.fixture(scope="module")
def libs():
    """builds the emulator library and the oracle (as tests/test_sim_kernels.py does, under the same lock) -> (emulator, checker)"""
    import fcntl
    csrc = os.path.join(capi.ROOT, "lerc_amd", "csrc")
    os.makedirs(os.path.join(capi.ROOT, "tests", "_sim"), exist_ok=True)
    with open(os.path.join(capi.ROOT, "tests", "_sim", ".build.lock"), "w") as lock:    # (pytest-xdist workers: one make at a time)
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", csrc, "sim", "-j8"])
        subprocess.check_call(["make", "-s", "-C", os.path.join(capi.ROOT, "oracle")])
    S, R = capi.sim(), capi.ref() or capi.oracle()
    assert S is not None, "tests/_sim/liblerc_amd_sim.so was not built"
    assert R is not None, "oracle/liblerc_oracle.so was not built"
    return S, R


@pytest.fixture()
def batch(libs):
    B = C.Batch(libs[0].lib, C.HostMem())
    yield B
    B.close()


@pytest.mark.parametrize("dtype", [np.uint8, np.int8])
def test_island_64(libs, batch, dtype):
    """the byte island, 256 tiles of 64 x 64 -- all valid, empty and partial -- every tile the rule names in the batch, each way (the
    others: partial tiles at the rim whose few valid pixels go one sweep or to 16 x 16 blocks)"""
    tiles, masks = C.byte_island(1024, 64, dtype)
    C.check_round_trip(batch, libs[1], tiles, masks, expect_must=245 if dtype == np.uint8 else 247)


@pytest.mark.parametrize("shape", [(40, 56), (65, 65)])
def test_predictor_corners(libs, batch, shape):
    C.check_corners(batch, libs[1], *shape)
    C.check_corners(batch, libs[1], *shape, dtype=np.int8)


def test_ragged_257(libs, batch):
    """the ragged edge, more than 65 536 pixels, mask bits that cross byte boundaries at k - width"""
    rng = np.random.default_rng(71)
    tiles = C.C.byte_mosaic(1028, 257)[:4]
    masks = C.M.random_blob_mask(rng, 4, 257, 257)
    C.check_round_trip(batch, libs[1], tiles, masks, expect_must=4)


def test_sub_batches(libs, batch):
    C.check_sub_batches(batch, libs[1])


def test_errors(libs, batch):
    C.check_errors(batch, libs[1], n_fuzz=30)


def test_soak(libs):
    C.check_soak(libs[0].lib, C.HostMem(), libs[1], rounds=5, max_tiles=8, size=512, tile=32)
