"""8-bit tile batches (int8 / uint8 tiles, every pixel valid, lossless, through lerc_amd_encode_tiles_device / _masked with
dValidBytes == NULL and their decoding counterparts) on the CPU emulator library, with small tiles: the same checks as
tests/test_gpu_tiles_bytes.py (tiles_bytes_common.py), against the real reference where it is built, else against the oracle.  The
batch kernels wait for no other workgroup, so the emulator runs the product's own path."""
import os
import subprocess

import numpy as np
import pytest

import capi
import tiles_bytes_common as C


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


@pytest.mark.parametrize("dtype", [np.uint8, np.int8])
def test_mosaic_small(libs, batch, dtype):
    """the byte mosaic in small: 12 x 12 tiles of 32 x 32 -- delta Huffman, plain Huffman and (uint8) tiling -- every one in the batch"""
    tiles = C.byte_mosaic(384, 32, dtype)
    want = C.check_round_trip(batch, libs[1], tiles, expect_must=144)
    m = C.modes(want)
    assert m[0] > 0 and m[1] > 0 and (dtype == np.int8 or m[2] > 0), m


def test_mosaic_64_and_ragged(libs, batch):
    C.check_round_trip(batch, libs[1], C.byte_mosaic(512, 64)[:8], expect_must=8)
    tiles = C.byte_mosaic(1028, 257)
    want = C.check_encode(batch, libs[1], tiles[:2])
    assert sum(C.must_batch(w, 257 * 257) for w in want) == 2
    C.check_decode(batch, libs[1], want, (257, 257), np.uint8)


@pytest.mark.parametrize("shape", [(64, 64), (65, 65), (40, 56)])
def test_variety(libs, batch, shape):
    """every kind of content, whatever path takes it: the reference's bytes, and the reference's pixels back"""
    tiles, _ = C.variety(*shape)
    C.check_round_trip(batch, libs[1], tiles)
    C.check_round_trip(batch, libs[1], (tiles.astype(np.int16) - 128).astype(np.int8))


def test_ties(libs, batch):
    """equal counts: the code lengths depend on how the reference's priority queue orders equal weights"""
    C.check_round_trip(batch, libs[1], C.tie_tiles())


def test_own_blobs_decode(libs, batch):
    tiles = C.byte_mosaic(384, 32)[:24]
    rc, own, _, _, _ = batch.encode(tiles, None, 0)
    assert rc == 0
    assert np.array_equal(C.check_decode(batch, libs[1], own, (32, 32), np.uint8), tiles)


def test_errors(libs, batch):
    C.check_errors(batch, libs[1], C.byte_mosaic(512, 64)[:5], n_fuzz=60)


def test_soak(libs):
    C.check_soak(libs[0].lib, C.HostMem(), libs[1], rounds=6, max_tiles=10, size=384, tile=32)


def test_sub_batches(libs, batch):
    """sub-batches of 3 + 3 + 1 tiles, a tile handed back in the second one"""
    C.check_sub_batches(batch, libs[1])
