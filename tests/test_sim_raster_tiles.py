"""The raster tile calls (lerc_amd_encode_raster_tiles_device / lerc_amd_decode_raster_tiles_device) on the CPU emulator library: a
pitched, misaligned raster cut into a grid of tiles and back (raster_tiles_common.py), against the real reference where it is built,
else against the oracle.  The cut and paste kernels wait for nobody, so the emulator runs the product's own path."""
import os
import subprocess

import pytest

import capi
import raster_tiles_common as RT


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
    B = RT.RasterBatch(libs[0].lib, RT.M.HostMem())
    yield B
    B.close()


@pytest.mark.parametrize("case", RT.PARITY, ids=RT.parity_id)
def test_parity(libs, batch, case):
    dtype, e, nb, with_mask, shape_tile = case
    RT.check_parity(batch, libs[1], dtype, e, nb, with_mask, shape_tile)


def test_is_a_batch(libs, batch):
    RT.check_is_a_batch(batch, libs[1])


@pytest.mark.parametrize("case", RT.COUNTERS, ids=lambda c: "%s%s" % ("%dx" % c[2] if c[2] > 1 else "", c[0].__name__))
def test_counters_match_the_tile_calls(libs, batch, case):
    RT.check_counters_match(batch, libs[1], *case)


def test_chunks(libs, batch):
    RT.check_chunks(batch, libs[1])


def test_in_place(libs, batch):
    RT.check_in_place(batch, libs[1])


def test_failing_tile(libs, batch):
    RT.check_failing_tile(batch, libs[1])


def test_arguments(libs, batch):
    RT.check_arguments(batch, libs[1])
