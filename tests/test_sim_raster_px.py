"""The strided raster tile calls (lerc_amd_encode_raster_tiles_device_strided / lerc_amd_decode_raster_tiles_device_strided) on the CPU
emulator library: pixel-interleaved, gapped and line-interleaved rasters cut into a grid of tiles and back (raster_px_common.py),
against the real reference where it is built, else against the oracle.  k_rt_cut_px / k_rt_paste_px wait for nobody, so the emulator
runs the product's own path."""
import os
import subprocess

import pytest

import capi
import raster_px_common as PX


@pytest.fixture(scope="module")
def libs():
    """builds the emulator library and the oracle (as tests/test_sim_raster_tiles.py does, under the same lock) -> (emulator, checker)"""
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
    B = PX.PxBatch(libs[0].lib, PX.RT.M.HostMem())
    yield B
    B.close()


@pytest.mark.parametrize("case", PX.PARITY, ids=PX.case_id)
def test_parity(libs, batch, case):
    PX.check_parity(batch, libs[1], case)


@pytest.mark.parametrize("case", PX.SAME_AS_PLANES, ids=PX.case_id)
def test_same_bytes_as_the_planar_call(libs, batch, case):
    PX.check_same_as_planes(batch, libs[1], case)


def test_pixel_pitch_one_is_the_existing_call(libs, batch):
    PX.check_pixel_pitch_one(batch, libs[1])


def test_line_interleaved(libs, batch):
    PX.check_line_interleaved(batch, libs[1])


def test_chunks(libs, batch):
    PX.check_chunks(batch, libs[1])


def test_failing_tile(libs, batch):
    PX.check_failing_tile(batch, libs[1])


def test_arguments(libs, batch):
    PX.check_arguments(batch, libs[1])
