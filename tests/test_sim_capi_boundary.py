"""The C boundary's answers (capi_boundary_common.py: every status-returning entry point, its valid call and one variation per
argument check) on the CPU emulator library."""
import os
import subprocess

import pytest

import capi
import capi_boundary_common as CB


@pytest.fixture(scope="module")
def env():
    """builds the emulator library (as tests/test_sim_raster_tiles.py does, under the same lock)"""
    import fcntl
    os.makedirs(os.path.join(capi.ROOT, "tests", "_sim"), exist_ok=True)
    with open(os.path.join(capi.ROOT, "tests", "_sim", ".build.lock"), "w") as lock:    # (pytest-xdist workers: one make at a time)
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", os.path.join(capi.ROOT, "lerc_amd", "csrc"), "sim", "-j8"])
    S = capi.sim()
    assert S is not None, "tests/_sim/liblerc_amd_sim.so was not built"
    e = CB.Env(S.lib, CB.M.HostMem())
    yield e
    e.close()


def test_table_names_every_status_returning_symbol():
    CB.check_names_every_symbol()


@pytest.mark.parametrize("name", sorted(CB.SPECS))
def test_boundary(env, name):
    CB.check(env, name)
