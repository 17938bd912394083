"""The shared block stages on the CPU emulator library: tests/block_stages_common.py, against the oracle."""
import os
import subprocess

import pytest

import capi
import block_stages_common as C
import tiles_masked_common as TM


@pytest.fixture(scope="module")
def libs():
    """builds the emulator library and the oracle (as tests/test_sim_kernels.py does, under the same lock) -> (emulator, oracle)"""
    import fcntl
    csrc = os.path.join(capi.ROOT, "lerc_amd", "csrc")
    os.makedirs(os.path.join(capi.ROOT, "tests", "_sim"), exist_ok=True)
    with open(os.path.join(capi.ROOT, "tests", "_sim", ".build.lock"), "w") as lock:    # (pytest-xdist workers: one make at a time)
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", csrc, "sim", "-j8"])
        subprocess.check_call(["make", "-s", "-C", os.path.join(capi.ROOT, "oracle")])
    S, R = capi.sim(), capi.oracle()
    assert S is not None, "tests/_sim/liblerc_amd_sim.so was not built"
    assert R is not None, "oracle/liblerc_oracle.so was not built"
    return S, R


@pytest.fixture(scope="module")
def batch(libs):
    B = C.batch_of(libs[0].lib, TM.HostMem())
    yield B
    B.close()


@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_sim_block_stages(libs, batch, case):
    C.check_case(libs[0], libs[1], batch, *case)
