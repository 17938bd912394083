"""Masked tile batches (lerc_amd_encode_tiles_device_masked / lerc_amd_decode_tiles_device_masked) on the CPU emulator library, with
small tiles: the same checks as tests/test_gpu_tiles_masked.py (tiles_masked_common.py), against the real reference where it is
built, else against the oracle.  The batch kernels wait for no other workgroup, so the emulator runs the product's own path."""
import os
import subprocess

import numpy as np
import pytest

import capi
import tiles_masked_common as C


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
    B = C.Batch(libs[0].lib, C.HostMem())
    yield B
    B.close()


@pytest.mark.parametrize("kind", ["float32", "uint16"])
def test_island_small(libs, batch, kind):
    """the island mosaic in small: 12 x 12 tiles of 32 x 32, packed and slotted, both ways"""
    R = libs[1]
    tiles, masks, e = C.island(kind, 384, 32)
    want = C.check_encode(batch, R, tiles, masks, e)
    C.check_encode(batch, R, tiles, masks, e, slot_bytes=tiles[0].nbytes + 1024, want=want)
    C.check_decode(batch, R, want, (32, 32), tiles.dtype)
    rc, own, _, _, _ = batch.encode(tiles, masks, e)
    assert rc == 0 and own == want


def test_ragged_and_parity(libs, batch):
    C.check_ragged(batch, libs[1], 6, 65, 65, np.int32, 3)
    C.check_ragged(batch, libs[1], 10, 40, 56, np.int16, 4)


def test_fallbacks(libs, batch):
    C.check_fallbacks(batch, libs[1])


def test_float_decisions_stay_in_the_batch(libs, batch):
    C.check_float_decisions(batch, libs[1])


def test_unaligned_arena(libs, batch):
    C.check_unaligned_arena(batch, libs[1])


def test_errors(libs, batch):
    C.check_errors(batch, libs[1], n_fuzz=60)


def test_fresh_contexts(libs):
    C.check_fresh_contexts(libs[0].lib, C.HostMem(), libs[1], rounds=4, n=5, r=40, c=56)


def test_soak(libs):
    C.check_soak(libs[0].lib, C.HostMem(), libs[1], rounds=6, max_tiles=10, r=40, c=56)


def test_counters_of_the_unmasked_batch(batch):
    """lerc_amd_tile_batch_counters also counts the existing batch calls"""
    tiles, _, e = C.island("float32", 128, 32)
    c0 = batch.counters()
    rc, blobs, _, _, _ = batch.encode(tiles, None, e, unmasked_call=True)
    c1 = batch.counters()
    assert rc == 0 and (c1[0] - c0[0]) + (c1[1] - c0[1]) == len(tiles)


def test_sub_batches(libs, batch):
    """sub-batches of 3 + 3 + 1 tiles, a tile handed back in the second one"""
    C.check_sub_batches(batch, libs[1])
