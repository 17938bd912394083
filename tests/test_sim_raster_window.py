"""The window decode and the tile range encode (lerc_amd_decode_raster_window_device / lerc_amd_encode_raster_tiles_device_range) on
the CPU emulator library (raster_window_common.py), against the real reference where it is built, else against the oracle.
k_rw_paste / k_rw_paste_px wait for nobody, so the emulator runs the product's own path."""
import os
import subprocess

import pytest

import capi
import raster_window_common as RW


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
    B = RW.WindowBatch(libs[0].lib, RW.RT.M.HostMem())
    yield B
    B.close()


@pytest.mark.parametrize("window,n_tiles", RW.WINDOWS, ids=lambda v: "x".join(str(k) for k in v) if isinstance(v, tuple) else None)
def test_windows(libs, batch, window, n_tiles):
    RW.check_windows(batch, libs[1], window, n_tiles)


def test_window_on_thin_edges(libs, batch):
    RW.check_windows(batch, libs[1], *RW.THIN_WINDOW, shape_tile=RW.THIN_EDGES)


@pytest.mark.parametrize("case", RW.CASES, ids=RW.case_id)
def test_types_and_destinations(libs, batch, case):
    RW.check_case(batch, libs[1], case)


def test_alignment_sweep(libs, batch):
    RW.check_alignment_sweep(batch, libs[1])


def test_only_the_windows_tiles(libs, batch):
    RW.check_only_the_windows_tiles(batch, libs[1])


def test_window_chunks(libs, batch):
    RW.check_chunks(batch, libs[1])


def test_damaged_blob_inside_and_outside_the_window(libs, batch):
    RW.check_damaged_blob(batch, libs[1])


def test_window_arguments(libs, batch):
    RW.check_window_arguments(batch, libs[1])


@pytest.mark.parametrize("rng", RW.RANGES, ids=lambda r: "x".join(str(k) for k in r))
def test_tile_ranges(libs, batch, rng):
    RW.check_ranges(batch, libs[1], rng)


def test_tile_range_mask_bands_and_pixels(libs, batch):
    RW.check_range_kinds(batch, libs[1])


def test_tile_range_in_place(libs, batch):
    RW.check_range_in_place(batch, libs[1])


def test_tile_range_arguments(libs, batch):
    RW.check_range_arguments(batch, libs[1])


def test_range_encode_then_window_decode(libs, batch):
    RW.check_round_trip(batch, libs[1])


def test_ranks_tile_rows_partition_the_grid():
    RW.check_shard_rows()
