"""Band stack tile batches (lerc_amd_encode_tiles_device_bands / lerc_amd_decode_tiles_device_bands) on the CPU emulator library, with
small tiles: the same checks as tests/test_gpu_tiles_bands.py (tiles_bands_common.py), against the real reference where it is built,
else against the oracle.  The batch kernels wait for no other workgroup, so the emulator runs the product's own path."""
import os
import subprocess

import numpy as np
import pytest

import capi
import tiles_bands_common as C


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
    B = C.BandsBatch(libs[0].lib, C.HostMem())
    yield B
    B.close()


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("nb", [2, 4])
@pytest.mark.parametrize("dtype,e", C.WIDE)
def test_parity_wide(libs, batch, dtype, e, nb, with_mask):
    C.check_parity_wide(batch, libs[1], dtype, e, nb, with_mask)


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("dtype", [np.uint8, np.int8])
def test_parity_bytes(libs, batch, dtype, with_mask):
    C.check_parity_bytes(batch, libs[1], dtype, with_mask)


@pytest.mark.parametrize("r,c", [(33, 41), (17, 9)])
def test_parity_ragged(libs, batch, r, c):
    C.check_parity_wide(batch, libs[1], np.uint16, 0, 3, True, n=6, r=r, c=c, seed=3)
    C.check_parity_wide(batch, libs[1], np.float32, 0.01, 3, False, n=4, r=r, c=c, seed=4)


def test_parity_bytes_256(libs, batch):
    C.check_parity_bytes(batch, libs[1], np.uint8, True, n=4, r=256, c=256)


def test_mix_inside_a_tile_wide(libs, batch):
    C.check_mix_wide(batch, libs[1])


def test_mix_inside_a_tile_bytes(libs, batch):
    C.check_mix_bytes(batch, libs[1])


def test_sub_batches(libs, batch):
    C.check_sub_batches(batch, libs[1])


def test_sub_batches_wide(libs, batch):
    C.check_sub_batches_wide(batch, libs[1])


def test_hand_backs(libs, batch):
    C.check_hand_backs(batch, libs[1])


def test_errors(libs, batch):
    C.check_errors(batch, libs[1], n_fuzz=8)


def test_errors_bytes(libs, batch):
    C.check_errors(batch, libs[1], n_fuzz=8, dtype=np.uint8)


def test_one_band(libs, batch):
    C.check_one_band(batch, libs[1])


def test_soak(libs):
    C.check_soak(libs[0].lib, C.HostMem(), libs[1], rounds=6, fresh_rounds=2, max_tiles=8)
