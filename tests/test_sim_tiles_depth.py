"""Depth tile batches (lerc_amd_encode_tiles_device_depth / lerc_amd_decode_tiles_device_depth, include/lerc_amd_depth.h) on the CPU
emulator library, with small tiles: the same checks as tests/test_gpu_tiles_depth.py (tiles_depth_common.py), against the real
reference where it is built, else against the oracle.  The batch kernels wait for no other workgroup, so the emulator runs the
product's own path."""
import os
import subprocess

import numpy as np
import pytest

import capi
import tiles_depth_common as C


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
    B = C.DepthBatch(libs[0].lib, C.HostMem())
    yield B
    B.close()


@pytest.mark.parametrize("slotted", [False, True])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("d", [2, 3, 4, 8])
@pytest.mark.parametrize("dtype,e", C.TYPES)
def test_parity(libs, batch, dtype, e, d, with_mask, slotted):
    """12 tiles of 33 x 41: ragged 8 x 8 and 16 x 16 blocks"""
    C.check_parity(batch, libs[1], dtype, e, d, with_mask, slotted)


@pytest.mark.parametrize("dtype,e", C.TYPES)
def test_parity_shapes(libs, batch, dtype, e):
    C.check_parity(batch, libs[1], dtype, e, 3, True, False, n=12, r=17, c=9, seed=5)
    C.check_parity(batch, libs[1], dtype, e, 2, True, True, n=4, r=64, c=64, seed=6)


def test_slice_differences(libs, batch):
    C.check_slice_differences(batch, libs[1])


def test_every_kind(libs, batch):
    C.check_kinds(batch, libs[1])


def test_hand_backs(libs, batch):
    C.check_hand_backs(batch, libs[1])


def test_sub_batches(libs, batch):
    C.check_sub_batches(batch, libs[1])


def test_depth_one_is_the_masked_call(libs, batch):
    C.check_depth_one(batch, libs[1])


def test_boundary(libs, batch):
    C.check_boundary(batch)
