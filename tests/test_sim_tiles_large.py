"""Tile batches with tiles beyond 131 072 pixels or 4 096 blocks, up to 513 x 513, on the CPU emulator library: every family of the
shared driver (tiles_large_common.py), against the real reference where it is built, else against the oracle.  The batch kernels
wait for no other workgroup, so the emulator runs the product's own path -- the large forms of the kernels that hold a tile's mask."""
import os
import subprocess

import numpy as np
import pytest

import capi
import tiles_bands_common as T
import tiles_large_common as L


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
    B = T.BandsBatch(libs[0].lib, L.M.HostMem())
    yield B
    B.close()


@pytest.mark.parametrize("shape", L.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype,e", [(np.float32, 0.01), (np.uint16, 0)], ids=["float32", "uint16"])
def test_masked_wide(libs, batch, shape, dtype, e):
    L.check_masked_wide(batch, libs[1], shape, dtype, e)


@pytest.mark.parametrize("shape", L.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype", [np.uint8, np.int8], ids=["uint8", "int8"])
def test_bytes(libs, batch, shape, dtype):
    L.check_bytes(batch, libs[1], shape, dtype)


@pytest.mark.parametrize("shape", L.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype", [np.uint8, np.int8], ids=["uint8", "int8"])
def test_bytes_masked(libs, batch, shape, dtype):
    L.check_bytes_masked(batch, libs[1], shape, dtype)


@pytest.mark.parametrize("dtype,nb,with_mask", [(np.uint8, 3, True), (np.uint16, 4, False), (np.uint16, 4, True)], ids=["3xuint8-mask", "4xuint16", "4xuint16-mask"])
def test_band_stacks_513(libs, batch, dtype, nb, with_mask):
    """two layouts here, not the four of tests/test_gpu_tiles_large.py: packed, and slotted at an odd arena address -- a 513 x 513 plane
    takes the emulator seconds, and the exact-size arena and the arena a byte too small are the driver's, covered at small shapes"""
    L.check_bands(batch, libs[1], dtype, nb, with_mask, four_layouts=False)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8], ids=["uint16", "uint8"])
def test_sub_batches(libs, batch, dtype):
    L.check_sub_batches(batch, libs[1], dtype)


def test_errors_513(libs, batch):
    L.check_errors(batch, libs[1], n_fuzz=5)


def test_long_runs_513(libs, batch):
    L.check_long_runs(batch, libs[1])


def test_above_the_limit(libs, batch):
    """a long thin shape of 4 353 blocks"""
    L.check_above_the_limit(batch, libs[1], (1, 8 * 4353))
