"""Depth rasters in any layout, windows and tile ranges (the four calls of include/lerc_amd_depth.h that take a depthPitch) on the CPU
emulator library: k_rtd_cut / k_rtd_paste of raster_tiles_depth.hip run as they are (raster_depth_layouts_common.py)."""
import os
import subprocess

import numpy as np
import pytest

import capi
import raster_depth_layouts_common as C


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
    B = C.DepthLayouts(libs[0].lib, C.D.HostMem())
    yield B
    B.close()


@pytest.mark.parametrize("dtype,e,c,lay,with_mask,slotted", C.PARITY, ids=C.PARITY_IDS)
def test_parity_both_ways(libs, batch, dtype, e, c, lay, with_mask, slotted):
    """37 x 45 x C, tiles of 16: four shape classes, ragged last tiles"""
    C.check_parity(batch, libs[1], dtype, e, c, lay, with_mask, slotted)


@pytest.mark.parametrize("lay", ["planes", "planes_view", "lines", "gapped"])
@pytest.mark.parametrize("dtype,e,shape", [(np.uint8, 0, (9, 520, 3)), (np.float64, 0.001, (9, 70, 2))], ids=["uint8", "float64"])
def test_rows_longer_than_a_segment(libs, batch, dtype, e, shape, lay):
    """one tile whose rows take two segments of kRtPxSegBytes = 512 bytes an element plane"""
    h, w, c = shape
    C.check_parity(batch, libs[1], dtype, e, c, "gapped%d" % (c + 1) if lay == "gapped" else lay, True, False, shape=(h, w), tile=(16, 1024))


@pytest.mark.parametrize("lay", C.layouts_for(3))
@pytest.mark.parametrize("window,n_tiles", C.WINDOWS, ids=["x".join(str(v) for v in w) for w, _ in C.WINDOWS])
def test_window(libs, batch, window, n_tiles, lay):
    C.check_window(batch, libs[1], window, n_tiles, lay)


@pytest.mark.parametrize("lay", C.layouts_for(3))
def test_window_with_a_damaged_blob(libs, batch, lay):
    C.check_damaged_blob(batch, libs[1], lay)


@pytest.mark.parametrize("lay", C.layouts_for(3))
@pytest.mark.parametrize("rng", C.RANGES, ids=["x".join(str(v) for v in r) for r in C.RANGES])
def test_tile_range(libs, batch, rng, lay):
    C.check_range(batch, libs[1], rng, lay)


def test_refused(libs, batch):
    C.check_refused(batch)


def test_header_symbols_are_exported(libs):
    C.check_header(libs[0].lib)
