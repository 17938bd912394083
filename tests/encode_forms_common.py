"""Shared by test_sim_encode_forms.py (CPU emulator library) and test_gpu_encode_forms.py (MI355X): the forms of the streaming
encoder's host that only a knob reaches --

  LERC_AMD_ENCODE_LAUNCHES=2   one raster in two launches (statistics, then a pack step whose first blocks scan and decide), a packed
                               tile batch in three (statistics, scan + decide + placement, pack), a slotted batch tile by tile
  LERC_AMD_TILE_ARENA=copy     the one-launch tile batch with a slot a tile and a pass that moves the blobs into the arena (the
                               emulator's default, an A/B knob on the GPU), and its second run with slots that hold raw blocks

-- checked like the default forms: every blob is the checker's, byte for byte, and the counters say which kernels served it.
The library reads both knobs once, so the checks run in a process of their own: `python encode_forms_common.py <sim|gpu> <check>...`
with the environment set (run() below starts it).

Memory: the emulator's "device" pointers are host pointers (numpy), the product's are HIP allocations (torch uint8 tensors).
"""
import ctypes as ct
import os
import subprocess
import sys

import numpy as np

import capi
import cases
import tiles_masked_common as T

# ---- the single rasters -------------------------------------------------------------------------------------------------
# (the emulator library is built with LERC_SMALL_GROUPS -- scan groups of 16 workgroups, pack groups of 4, scan slices of 4 -- so 64 x 64,
# one workgroup, and 136 x 200, 17 x 25 = 425 blocks = 7 workgroups and a width that is neither 64 blocks nor a power of two, are
# on both sides of every group boundary there)
SIM_SHAPES = ((64, 64), (136, 200))
# The product build (tile_fast.h): a workgroup is kFastBlocksPerWG = 64 blocks of 8 x 8 pixels; fastScanGroups(nWG) > 1 needs
# nWG > kFastScanGroup = 4096 (which is also kSoloSlice, the workgroups one scan block of the two-launch form places), i.e. more than
# 64 * 4096 = 262144 blocks, more than 4096 x 4096 pixels; fastPackGroups(nWG) > 1 needs nWG > kFastPackGroup = 16 only.  One block
# column more than 512 x 512 blocks: 512 x 513 = 262656 blocks, nWG = 4104 -- two scan groups / slices, 257 pack groups.
GPU_SHAPES = ((4096, 4104),)
KINDS = ((np.float32, 0.01), (np.uint16, 0))


def two_launches():
    return os.environ.get("LERC_AMD_ENCODE_LAUNCHES") == "2"


def handle_counters(L, h):
    """lerc_amd_path_counters of a handle -> [encode streaming, encode general, decode streaming, decode general]"""
    out = (ct.c_ulonglong * 4)()
    L.lerc_amd_path_counters.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    L.lerc_amd_path_counters.restype = None
    L.lerc_amd_path_counters(h, out)
    return [int(v) for v in out]


def raster(rng, r, c, dt):
    return cases._cast(cases.terrain(r, c, rng, amp=300, base=1000, sigma=1.5), dt)


def check_single_rasters(P, mem, R, shapes):
    """a size query (no output buffer) and an encode per raster: the streaming kernels serve both"""
    rng = np.random.default_rng(51)
    for dt, e in KINDS:
        for (r, c) in shapes:
            x = raster(rng, r, c, dt)
            rc_r, want = R.encode(x, e)
            assert rc_r == 0
            c0 = P.path_counters()
            assert P.compute_size(x, e) == (0, len(want)), (np.dtype(dt).name, r, c, P.last_note())
            rc, blob = P.encode(x, e, buf_size=len(want))
            c1 = P.path_counters()
            assert rc == 0 and blob == want, (np.dtype(dt).name, r, c, P.last_note())
            assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 0), (np.dtype(dt).name, r, c, c0, c1, P.last_note())


def check_ragged_raster(P, mem, R, shapes):
    """257 x 257: only the one-launch encoder takes sides that are no multiples of 8, so under LERC_AMD_ENCODE_LAUNCHES=2 the general
    kernels serve the raster -- same bytes"""
    rng = np.random.default_rng(52)
    for dt, e in KINDS:
        x = raster(rng, 257, 257, dt)
        rc_r, want = R.encode(x, e)
        c0 = P.path_counters()
        rc, blob = P.encode(x, e, buf_size=len(want))
        c1 = P.path_counters()
        assert rc_r == rc == 0 and blob == want, (np.dtype(dt).name, P.last_note())
        assert (c1[0] - c0[0], c1[1] - c0[1]) == ((0, 1) if two_launches() else (1, 0)), (np.dtype(dt).name, c0, c1, P.last_note())


def check_band_stack(P, mem, R, shapes):
    """3 bands of 64 x 72: a blob a band with "bands to follow" in its header, every band through the streaming kernels"""
    rng = np.random.default_rng(53)
    for dt, e in KINDS:
        x = np.stack([raster(rng, 64, 72, dt) + dt(50 * b) for b in range(3)])
        rc_r, want = R.encode(x, e, n_bands=3)
        assert rc_r == 0
        c0 = P.path_counters()
        assert P.compute_size(x, e, n_bands=3) == (0, len(want)), (np.dtype(dt).name, P.last_note())
        rc, blob = P.encode(x, e, n_bands=3, buf_size=len(want))
        c1 = P.path_counters()
        assert rc == 0 and blob == want, (np.dtype(dt).name, P.last_note())
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 0), (np.dtype(dt).name, c0, c1, P.last_note())    # (a call counts once)


def five_tiles(rng, dt):
    """5 tiles of 64 x 64, tile 2 constant: the streaming kernels hand it back, it is encoded by itself behind the batch"""
    tiles = np.stack([raster(rng, 64, 64, dt) + dt(10 * t) for t in range(5)])
    tiles[2] = tiles[2].flat[0]
    return tiles


def check_tile_batch(P, mem, R, shapes):
    """packed into an arena, then a slot a tile, then an arena one byte too small"""
    rng = np.random.default_rng(54)
    for dt, e in KINDS:
        tiles = five_tiles(rng, dt)
        want = T.ref_blobs(R, tiles, None, e)
        B = T.Batch(P.lib, mem)
        try:
            # packed: four tiles by the batch's launches, the constant one behind them
            t0, p0 = B.counters(), handle_counters(B.L, B.h)
            rc, blobs, offs, sizes, used = B.encode(tiles, None, e)
            t1, p1 = B.counters(), handle_counters(B.L, B.h)
            assert rc == 0 and blobs == want, (np.dtype(dt).name, rc, B.note())
            T.check_layout(offs, sizes, used)
            assert (t1[0] - t0[0], t1[1] - t0[1]) == (4, 1), (t0, t1, B.note())
            assert (p1[0] - p0[0], p1[1] - p0[1]) == (4, 1), (p0, p1, B.note())
            # an arena one byte too small, and the same arena at its exact size
            assert B.encode(tiles, None, e, arena_cap=used - 1)[0] == 3
            rc, blobs, offs, sizes, used1 = B.encode(tiles, None, e, arena_cap=used)
            assert rc == 0 and blobs == want and used1 == used
            # slotted: the three-launch form has no slots, so under LERC_AMD_ENCODE_LAUNCHES=2 a slotted batch goes tile by tile -- each
            # tile's own call through the streaming kernels, the constant tile's through the general ones
            slot = (tiles[0].nbytes + 1024 + 15) & ~15
            t0, p0 = B.counters(), handle_counters(B.L, B.h)
            rc, blobs, offs, sizes, used = B.encode(tiles, None, e, slot_bytes=slot)
            t1, p1 = B.counters(), handle_counters(B.L, B.h)
            assert rc == 0 and blobs == want, (np.dtype(dt).name, rc, B.note())
            T.check_layout(offs, sizes, used, slot)
            assert used == 5 * slot
            assert (t1[0] - t0[0], t1[1] - t0[1]) == ((0, 5) if two_launches() else (4, 1)), (t0, t1, B.note())
            assert (p1[0] - p0[0], p1[1] - p0[1]) == (4, 1), (p0, p1, B.note())
        finally:
            B.close()


def profiled_encode(B, tiles, e):
    """B.encode with the per-kernel profile on -> (its result, {scope name: launches})"""
    L = B.L
    L.lerc_amd_profile_enable.argtypes = [ct.c_void_p, ct.c_int]
    L.lerc_amd_profile_read.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int]
    L.lerc_amd_profile_enable(B.h, 1)
    res = B.encode(tiles, None, e)
    L.lerc_amd_profile_enable(B.h, 0)
    buf = ct.create_string_buffer(1 << 14)
    L.lerc_amd_profile_read(B.h, buf, len(buf), 1)
    return res, {ln.split()[0]: int(ln.split()[2]) for ln in buf.value.decode().splitlines()}


def check_copy_arena(P, mem, R, shapes):
    """LERC_AMD_TILE_ARENA=copy, the one-launch encoder: a slot a tile (half the tile's raw size + 4096 bytes) and a pass that moves the
    blobs into the arena.  12 tiles of 64 x 64 float32 at maxZErr 1e-6, 9 of them noise: each of those compresses to more than its slot
    and is handed back for that alone (kRedoCapacity); 9 is more than max(8, 12 / 32), so the batch is run once more with slots that
    hold raw blocks -- two launches of the batch kernel, no tile one by one.  Then 5 tiles, one of them constant."""
    assert os.environ.get("LERC_AMD_TILE_ARENA") == "copy" and not two_launches()
    rng = np.random.default_rng(55)
    e = 1e-6
    noise = [rng.uniform(0.0, 1000.0, (64, 64)).astype(np.float32) for _ in range(9)]
    calm = [(1000.0 + 0.2 * rng.random((64, 64))).astype(np.float32) for _ in range(3)]
    tiles = np.stack(noise[:4] + calm[:1] + noise[4:7] + calm[1:] + noise[7:])
    noisy = [t not in (4, 8, 9) for t in range(12)]
    want = T.ref_blobs(R, tiles, None, e)
    slot = 64 * 64 * 4 // 2 + 4096
    for t in range(12):    # (what the test relies on, from the checker's own blobs)
        assert (len(want[t]) > slot) == noisy[t], (t, len(want[t]), slot)
        assert len(want[t]) < 64 * 64 * 4, (t, len(want[t]))    # (and block by block beats one sweep of raw pixels: no other reason to hand it back)
    B = T.Batch(P.lib, mem)
    try:
        t0, p0 = B.counters(), handle_counters(B.L, B.h)
        (rc, blobs, offs, sizes, used), launches = profiled_encode(B, tiles, e)
        t1, p1 = B.counters(), handle_counters(B.L, B.h)
        assert rc == 0 and blobs == want, (rc, B.note())
        T.check_layout(offs, sizes, used)
        assert (t1[0] - t0[0], t1[1] - t0[1]) == (12, 0), (t0, t1, B.note())
        assert (p1[0] - p0[0], p1[1] - p0[1]) == (12, 0), (p0, p1, B.note())
        assert (launches.get("fast_encode1"), launches.get("fast_tile_move")) == (2, 2), launches
        for dt, e5 in KINDS:
            tiles5 = five_tiles(rng, dt)
            want5 = T.ref_blobs(R, tiles5, None, e5)
            t0, p0 = B.counters(), handle_counters(B.L, B.h)
            (rc, blobs, offs, sizes, used), launches = profiled_encode(B, tiles5, e5)
            t1, p1 = B.counters(), handle_counters(B.L, B.h)
            assert rc == 0 and blobs == want5, (np.dtype(dt).name, rc, B.note())
            T.check_layout(offs, sizes, used)
            assert (t1[0] - t0[0], t1[1] - t0[1]) == (4, 1), (t0, t1, B.note())
            assert (p1[0] - p0[0], p1[1] - p0[1]) == (4, 1), (p0, p1, B.note())
            assert launches.get("fast_tile_move") == 1, launches
            assert B.encode(tiles5, None, e5, arena_cap=used - 1)[0] == 3
            assert B.encode(tiles5, None, e5, arena_cap=used)[0] == 0
    finally:
        B.close()


CHECKS = {"single_rasters": check_single_rasters, "ragged_raster": check_ragged_raster, "band_stack": check_band_stack,
          "tile_batch": check_tile_batch, "copy_arena": check_copy_arena}


def run(backend, checks, **knobs):
    """the checks in a process of its own with the knobs in its environment; asserts that every one of them passed"""
    env = dict(os.environ, **knobs)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), backend] + list(checks), env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=600, cwd=capi.ROOT)
    assert out.returncode == 0 and ("forms ok: " + " ".join(checks)).encode() in out.stdout, out.stdout.decode()[-3000:]


def main(argv):
    backend, names = argv[0], argv[1:]
    if backend == "gpu":
        import torch    # (before the library is loaded: both then share one HIP runtime)
        assert torch.cuda.is_available(), "gpu tests need a GPU"
        P, mem, shapes = capi.product(), T.GpuMem(), GPU_SHAPES
    else:
        P, mem, shapes = capi.sim(), T.HostMem(), SIM_SHAPES
    R = capi.ref() or capi.oracle()
    assert P is not None and R is not None, "the libraries are not built"
    for name in names:
        CHECKS[name](P, mem, R, shapes)
    print("forms ok: " + " ".join(names))


if __name__ == "__main__":
    sys.path.insert(0, capi.ROOT)
    main(sys.argv[1:])
