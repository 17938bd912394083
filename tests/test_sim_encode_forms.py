"""The streaming encoder's knob-only forms on the CPU emulator library (encode_forms_common.py): one raster in two launches, a tile
batch in three, a slotted batch tile by tile (LERC_AMD_ENCODE_LAUNCHES=2), and the one-launch tile batch that copies its slots into
the arena (LERC_AMD_TILE_ARENA=copy, which is what emulator builds do unless asked).  tests/test_gpu_encode_forms.py runs the same on
the MI355X."""
import os
import subprocess

import pytest

import capi
import encode_forms_common as C


@pytest.fixture(scope="module")
def libs():
    """builds the emulator library and the oracle (as tests/test_sim_kernels.py does, under the same lock)"""
    import fcntl
    csrc = os.path.join(capi.ROOT, "lerc_amd", "csrc")
    os.makedirs(os.path.join(capi.ROOT, "tests", "_sim"), exist_ok=True)
    with open(os.path.join(capi.ROOT, "tests", "_sim", ".build.lock"), "w") as lock:    # (pytest-xdist workers: one make at a time)
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", csrc, "sim", "-j8"])
        subprocess.check_call(["make", "-s", "-C", os.path.join(capi.ROOT, "oracle")])


@pytest.mark.parametrize("check", ["single_rasters", "band_stack", "tile_batch"])
def test_sim_two_launch_forms(libs, check):
    C.run("sim", [check], LERC_AMD_ENCODE_LAUNCHES="2")


def test_sim_tile_batch_that_copies_its_slots(libs):
    C.run("sim", ["copy_arena"], LERC_AMD_TILE_ARENA="copy")


def test_fast_band_params_are_filled_as_they_were_by_hand(libs):
    """the kernels read BandParams as bytes: fastBandParams() / raiseCandidates() against a transcription of the filling they replaced,
    for every data type and a set of error bounds (tools/check_fast_band_params.cpp, host code linked against the emulator's objects)"""
    csrc = os.path.join(capi.ROOT, "lerc_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "bandparams"])
    out = subprocess.run([os.path.join(capi.ROOT, "tests", "_sim", "check_fast_band_params")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert out.returncode == 0 and b" 0 bad" in out.stdout, out.stdout.decode()[-2000:]
