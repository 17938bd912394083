"""Raster mosaics of depth tiles (lerc_amd_encode_raster_tiles_device_depth / lerc_amd_decode_raster_tiles_device_depth) on the CPU emulator library:
an [H, W, C] raster, or a view of one with padded rows, cut into the grid and coded as blobs of nDepth = C (raster_depth_common.py)."""
import os
import subprocess

import numpy as np
import pytest

import capi
import raster_depth_common as C


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
    B = C.RasterDepth(libs[0].lib, C.D.HostMem())
    yield B
    B.close()


@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("dtype,e", [(np.uint16, 0), (np.float32, 0.01)])
def test_four_shape_classes(libs, batch, dtype, e, with_mask, view):
    """70 x 90 x 3, tile 32: interior, right column, bottom row, corner"""
    C.check_raster(batch, libs[1], dtype, e, 70, 90, 3, 32, with_mask, view)


@pytest.mark.parametrize("dtype,e", [(np.uint16, 0), (np.float32, 0.01)])
def test_whole_tiles_slotted(libs, batch, dtype, e):
    C.check_raster(batch, libs[1], dtype, e, 64, 64, 4, 32, True, False, slotted=True)


def test_refused(libs, batch):
    C.check_refused(batch)
