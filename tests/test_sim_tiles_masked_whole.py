"""Masked tile batches whose empty, constant, one-sweep and 16 x 16 tiles stay inside the batch's launches, on the CPU emulator
library with small tiles: the same checks as tests/test_gpu_tiles_masked_whole.py (tiles_masked_whole_common.py), against the real
reference where it is built, else against the oracle.  In a batch, as many tiles are done one by one as have a NaN at a valid pixel."""
import os
import subprocess

import numpy as np
import pytest

import capi
import tiles_masked_common as C
import tiles_masked_whole_common as W


@pytest.fixture(scope="module")
def libs():
    """builds the emulator library and the oracle (as tests/test_sim_tiles_masked.py does, under the same lock) -> (emulator, checker)"""
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


@pytest.mark.parametrize("kind", ["float32", "uint16"])
def test_island_small_nothing_leaves(libs, batch, kind):
    """12 x 12 tiles of 32 x 32: the 32 empty tiles at the corners are the batch's own, each way, packed and slotted"""
    W.check_island(batch, libs[1], kind, 384, 32, n_empty=32)


@pytest.mark.parametrize("dtype", W.TYPES, ids=lambda d: np.dtype(d).name)
def test_kinds(libs, batch, dtype):
    W.check_kinds(batch, libs[1], dtype, 40, 56)
    W.check_kinds(batch, libs[1], dtype, 8, 8)


@pytest.mark.parametrize("dtype", W.TYPES, ids=lambda d: np.dtype(d).name)
def test_kinds_ragged_65(libs, batch, dtype):
    W.check_kinds(batch, libs[1], dtype, 65, 65)


@pytest.mark.parametrize("dtype", [np.float32, np.uint16], ids=lambda d: np.dtype(d).name)
def test_damage(libs, batch, dtype):
    W.check_damage(batch, libs[1], dtype, 40, 56, n_fuzz=60)


def test_capacity(libs, batch):
    W.check_capacity(batch, libs[1], np.int32, 40, 56)
    W.check_capacity(batch, libs[1], np.float32, 40, 56)


def test_nan_tile_alone_leaves(libs, batch):
    W.check_nan(batch, libs[1], 40, 56)


def test_one_context(libs):
    W.check_one_context(libs[0].lib, C.HostMem(), libs[1], rounds=6, r=40, c=56)
