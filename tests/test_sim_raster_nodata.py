"""The noData raster calls (lerc_amd_encode_raster_tiles_device_nodata / lerc_amd_decode_raster_window_device_nodata,
include/lerc_amd_nodata.h) on the CPU emulator library (raster_nodata_common.py), against the real reference where it is built, else
against the oracle.  k_rtn_cut / k_rtn_paste wait for nobody, so the emulator runs the product's own path."""
import os
import subprocess

import numpy as np
import pytest

import capi
import raster_nodata_common as ND


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
    B = ND.NoDataBatch(libs[0].lib, ND.HostMem())
    yield B
    B.close()


VALUES = [(dtype, e, kind) for dtype, e in ND.TYPES for kind in ("inside", "outside", "zero")] + \
         [(dtype, e, kind) for dtype, e in ND.TYPES[6:] for kind in ("nan", "-inf")]


@pytest.mark.parametrize("dtype,e,kind", VALUES, ids=lambda v: v if isinstance(v, str) else (np.dtype(v).name if isinstance(v, type) else None))
def test_types_and_values(libs, batch, dtype, e, kind):
    ND.check_type_and_value(batch, libs[1], dtype, e, kind)


def test_negative_zero_matches_zero(libs, batch):
    ND.check_negative_zero(batch, libs[1])


def test_no_pixel_matches(libs, batch):
    ND.check_no_pixel_matches(batch, libs[1])


def test_a_tile_of_holes_is_an_empty_blob(libs, batch):
    ND.check_one_tile_all_holes(batch, libs[1])


def test_nan_holes_stay_inside_the_batch(libs, batch):
    ND.check_nan_holes_stay_inside(batch, libs[1])


def test_invalid_values_never_count(libs, batch):
    ND.check_invalid_values_never_count(batch, libs[1])


def test_alignment_sweep(libs, batch):
    ND.check_alignment_sweep(batch, libs[1])


def test_one_channel_of_an_interleaved_image(libs, batch):
    ND.check_pixel_pitches(batch, libs[1])


@pytest.mark.parametrize("rng", ND.RANGES, ids=lambda r: "x".join(str(k) for k in r))
def test_tile_ranges(libs, batch, rng):
    ND.check_range(batch, libs[1], rng)


@pytest.mark.parametrize("window,n_tiles", ND.WINDOWS, ids=lambda v: "x".join(str(k) for k in v) if isinstance(v, tuple) else None)
def test_windows(libs, batch, window, n_tiles):
    ND.check_window(batch, libs[1], window, n_tiles)


def test_several_chunks_a_class(libs, batch):
    ND.check_chunks(batch, libs[1])


def test_range_encode_then_window_decode(libs, batch):
    ND.check_round_trip(batch, libs[1])


def test_damaged_blob_inside_and_outside_the_window(libs, batch):
    ND.check_damaged_blob(batch, libs[1])


def test_slot_too_small(libs, batch):
    ND.check_slot_too_small(batch, libs[1])


def test_boundary(libs, batch):
    ND.check_boundary(batch, libs[1])
