"""CPU-only check of the REAL kernel sources: lerc_amd/csrc/*.hip compiled for the SIMT emulator in
tools/hipsim (tests/_sim/liblerc_amd_sim.so) and driven through the same C ABI as the product.
This is test infrastructure: it proves indexing / protocol logic of the kernels before GPU time is
spent; the product library itself is only ever run on a GPU (tests marked `gpu`)."""
import os
import subprocess

import numpy as np
import pytest

import capi
import cases
import huffblob


@pytest.fixture(scope="module")
def libs():
    import fcntl
    csrc = os.path.join(capi.ROOT, "lerc_amd", "csrc")
    os.makedirs(os.path.join(capi.ROOT, "tests", "_sim"), exist_ok=True)
    with open(os.path.join(capi.ROOT, "tests", "_sim", ".build.lock"), "w") as lock:    # (pytest-xdist workers: one make at a time)
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", csrc, "sim", "-j8"])
        subprocess.check_call(["make", "-s", "-C", os.path.join(capi.ROOT, "oracle")])
    return capi.oracle(), capi.sim()


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# cases the device path does not cover yet (tracked in DESIGN.md "not yet on the device")
def _unsupported(name):
    return False    # (the bit plane mode, maxZErr 777, used to be listed here)


_CASES = [c for c in cases.basic_cases() if c[1].size <= 36000 and not _unsupported(c[0])]
# keep the emulator run short: every 3rd plain terrain case, all special cases
_CASES = [c for i, c in enumerate(_CASES) if not c[0].startswith("terrain") or i % 3 == 0]


@pytest.mark.parametrize("idx", range(len(_CASES)), ids=[c[0] for c in _CASES])
def test_sim_matches_oracle(libs, idx):
    O, S = libs
    name, arr, kw = _CASES[idx]
    kw = dict(kw)
    e = kw.pop("max_z_err")
    assert S.compute_size(arr, e, **kw) == O.compute_size(arr, e, **kw)
    r1, b1 = O.encode(arr, e, **kw)
    r2, b2 = S.encode(arr, e, **kw)
    assert r1 == r2
    assert b1 == b2, "blob differs from the oracle"
    if r1 == 0:
        d1, d2 = O.decode(b1), S.decode(b1)
        assert d1[0] == d2[0] == 0
        assert _same(d1[1], d2[1]) and _same(d1[2], d2[2])
        assert O.blob_info(b1) == S.blob_info(b1)


def test_sim_decodes_reference_blobs(libs):
    O, S = libs
    d = os.path.join(capi.ROOT, "tests", "golden")
    names = ["california_400_400_1_float.lerc2", "js_sanity_v5.lerc2"]
    names += [os.path.join("blobs", f) for f in sorted(os.listdir(os.path.join(d, "blobs")))]
    for f in names:
        blob = open(os.path.join(d, f), "rb").read()
        d1, d2 = O.decode(blob), S.decode(blob)
        assert d1[0] == d2[0] == 0, f
        assert _same(d1[1], d2[1]) and _same(d1[2], d2[2]), f


def test_sim_rejects_corruption(libs):
    O, S = libs
    blob = bytearray(open(os.path.join(capi.ROOT, "tests", "golden", "blobs", "mixed-float32.lerc2"), "rb").read())
    blob[len(blob) // 2] ^= 0x40
    assert S.decode(bytes(blob))[0] == 1
    assert S.decode(bytes(blob[:300]))[0] != 0
    # a blob the streaming kernels take up, with one flipped payload bit: Failed, and the caller's buffer holds zeros, not the
    # pixels of a blob that did not pass its checksum (include/lerc_amd.h: lerc_decode; the harness pre-fills 0xCD)
    rng = np.random.default_rng(12)
    x = cases.terrain(64, 1024, rng, amp=300, base=1000, sigma=1.5).astype(np.float32)
    rc, good = O.encode(x, 0.01)
    assert rc == 0
    bad = bytearray(good)
    bad[len(bad) // 2] ^= 0x10
    rc, dec, _ = S.decode(bytes(bad))
    assert rc == 1 and dec is not None and not dec.view(np.uint8).any()
    rc, dec, _ = S.decode(good)
    assert rc == 0 and _same(dec, O.decode(good)[1])


def _fast_cases():
    """Rasters that qualify for the streaming kernels (unmasked, nDepth 1, rows % 8 == 0, cols % 512 == 0),
    plus the inputs that make the device-side decisions bail out to the general path."""
    rng = np.random.default_rng(11)
    out = []
    for dt in (np.float32, np.uint16, np.int16, np.int32, np.uint32, np.float64):
        kind = np.dtype(dt).kind
        for (r, c) in ((8, 512), (16, 1024)):
            x = cases.terrain(r, c, rng, amp=300, base=1000, sigma=1.5)
            for e in ([0.01, 3.0] if kind == "f" else [0, 2]):
                out.append((f"fast-terrain-{np.dtype(dt).name}-{r}x{c}-e{e}", cases._cast(x, dt), e))
            out.append((f"fast-mixed-{np.dtype(dt).name}-{r}x{c}", cases.mixed_regions(r, c, rng, dt), 0.01 if kind == "f" else 0))
    # narrow rasters: a workgroup's 64 blocks span several block rows (e.g. the 256 x 256 tiles of a mosaic)
    for dt in (np.float32, np.uint16, np.float64):
        for (r, c) in ((256, 256), (64, 128), (128, 64)):
            x = cases.terrain(r, c, rng, amp=300, base=1000, sigma=1.5)
            out.append((f"fast-narrow-{np.dtype(dt).name}-{r}x{c}", cases._cast(x, dt), 0.01 if np.dtype(dt).kind == "f" else 0))
    # any width that is a multiple of 8: a workgroup's blocks wrap around block row ends wherever they fall, and the
    # last workgroup holds fewer than 64 blocks
    for dt in (np.float32, np.uint16, np.float64, np.int32):
        for (r, c) in ((8, 1000), (24, 200), (16, 8), (40, 328), (8, 8), (72, 520), (256, 24)):
            x = cases.terrain(r, c, rng, amp=300, base=1000, sigma=1.5)
            out.append((f"fast-anywidth-{np.dtype(dt).name}-{r}x{c}", cases._cast(x, dt), 0.01 if np.dtype(dt).kind == "f" else 0))
    out.append(("fast-anywidth-mixed-f32-48x1048", cases.mixed_regions(48, 1048, rng, np.float32), 0.01))
    out.append(("fast-anywidth-mixed-u16-200x120", cases.mixed_regions(200, 120, rng, np.uint16), 0))
    f = np.float32
    out.append(("fast-f32-allint", np.rint(cases.terrain(16, 512, rng)).astype(f), 0.01))
    out.append(("fast-f32-round1", np.round(cases.terrain(16, 512, rng), 1).astype(f), 0.01))
    out.append(("fast-f32-const", np.full((16, 512), 3.5, f), 0.01))
    y = np.full((16, 512), 100.0, f)
    y[rng.random((16, 512)) < 0.05] += 0.02
    out.append(("fast-f32-mb16", y, 0.01))
    z = cases.terrain(16, 512, rng).astype(f)
    z[3, 5] = np.nan
    out.append(("fast-f32-nan", z, 0.01))
    zr = cases.terrain(16, 512, rng).astype(f)
    zr[5, 7] = 3e30
    out.append(("fast-f32-some-raw", zr, 0.01))
    out.append(("fast-f32-huge", (cases.terrain(16, 512, rng) * 1e30).astype(f), 0.01))
    return out


_FAST = _fast_cases()


@pytest.mark.parametrize("idx", range(len(_FAST)), ids=[c[0] for c in _FAST])
def test_sim_streaming_path(libs, idx):
    O, S = libs
    name, arr, e = _FAST[idx]
    r1, b1 = O.encode(arr, e)
    c0 = S.path_counters()
    r2, b2 = S.encode(arr, e)
    c1 = S.path_counters()
    assert r1 == r2 and b1 == b2
    if "anywidth" in name and "mixed" not in name:
        assert c1[0] > c0[0], (name, "the encode did not take the streaming kernels", S.last_note())
    if r1 == 0:
        d1, d2 = O.decode(b1), S.decode(b1)
        assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1])
        if "anywidth" in name and "mixed" not in name and len(b1) > 4096:
            assert S.path_counters()[2] > c1[2], (name, "the decode did not take the streaming kernels", S.last_note())


def _multi_chunk_cases():
    """Streams of many 4 KiB chunks: the walk has to agree on chunk exits and sub-chunk entries."""
    rng = np.random.default_rng(5)
    out = []
    for dt in (np.float32, np.uint16, np.int32, np.float64):
        kind = np.dtype(dt).kind
        x = cases.terrain(64, 1024, rng, amp=300, base=1000, sigma=1.5)
        out.append((f"chunks-terrain-{np.dtype(dt).name}", cases._cast(x, dt), 0.01 if kind == "f" else 0, True))
        # runs of 1-byte constant blocks make every window position a plausible start; wide windows (float64)
        # then exceed the survivor lists and the band goes to the general kernels
        out.append((f"chunks-mixed-{np.dtype(dt).name}", cases.mixed_regions(64, 1024, rng, dt), 2.0, dt is not np.float64))
    z = np.zeros((128, 1024), np.float32)
    z[40:56, 100:400] = cases.terrain(16, 300, rng).astype(np.float32)
    out.append(("chunks-sparse-f32", z, 0.01, False))       # thousands of 1-byte blocks per chunk: general kernels
    zr = cases.terrain(64, 1024, rng).astype(np.float32)
    zr[::8, ::8] *= 1e20
    out.append(("chunks-raw-f32", zr, 0.01, False))          # raw blocks: too many plausible block starts
    return out


_CHUNKS = _multi_chunk_cases()


@pytest.mark.parametrize("idx", range(len(_CHUNKS)), ids=[c[0] for c in _CHUNKS])
def test_sim_streaming_decode_many_chunks(libs, idx):
    O, S = libs
    name, arr, e, expect_streamed = _CHUNKS[idx]
    r1, b1 = O.encode(arr, e)
    r2, b2 = S.encode(arr, e)
    assert r1 == r2 == 0 and b1 == b2
    c0 = S.path_counters()
    d2 = S.decode(b1)
    c1 = S.path_counters()
    d1 = O.decode(b1)
    assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1])
    if expect_streamed:
        assert c1[2] == c0[2] + 1, "the streaming decode kernels fell back to the general path"


def _aligned(n_bytes, align=64):
    raw = np.zeros(n_bytes + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + n_bytes]


def _device_decode(S, blob, shape, dtype, mask=False):
    """lerc_amd_decode_device through the emulator (device pointers are host pointers there)."""
    import ctypes as ct
    L = S.lib
    L.lerc_amd_create.restype = ct.c_void_p
    L.lerc_amd_create.argtypes = [ct.c_void_p]
    L.lerc_amd_destroy.argtypes = [ct.c_void_p]
    L.lerc_amd_decode_device.restype = ct.c_uint
    L.lerc_amd_decode_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int,
                                         ct.c_int, ct.c_uint, ct.c_void_p]
    L.lerc_amd_path_counters.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    h = L.lerc_amd_create(None)
    assert h
    try:
        src = _aligned(len(blob))
        src[:] = np.frombuffer(blob, np.uint8)
        out = _aligned(int(np.prod(shape)) * np.dtype(dtype).itemsize).view(dtype).reshape(shape)
        valid = _aligned(int(np.prod(shape))) if mask else None
        rc = L.lerc_amd_decode_device(h, src.ctypes.data, len(blob), 1 if mask else 0, valid.ctypes.data if mask else None, 1,
                                      shape[1], shape[0], 1, capi.dt_code(dtype), out.ctypes.data)
        cnt = (ct.c_ulonglong * 4)()
        L.lerc_amd_path_counters(h, cnt)
        return rc, out.copy(), (valid.copy() if mask else None), tuple(int(v) for v in cnt)
    finally:
        L.lerc_amd_destroy(h)


def test_sim_device_decode_without_reading_the_header_on_the_host(libs):
    """Device-resident single-band blobs are enqueued blind (k_fast_header checks the header on the device)."""
    O, S = libs
    rng = np.random.default_rng(3)
    for dt, e in ((np.float32, 0.01), (np.uint16, 0), (np.int32, 2), (np.float64, 0.5)):
        arr = cases._cast(cases.terrain(32, 1024, rng, amp=300, base=1000, sigma=1.5), dt)
        rc, blob = O.encode(arr, e)
        assert rc == 0
        want = O.decode(blob)
        rc2, got, valid, cnt = _device_decode(S, blob, arr.shape, dt, mask=True)
        assert rc2 == 0 and _same(want[1].reshape(arr.shape), got) and valid.min() == 1
        assert cnt[2] == 1 and cnt[3] == 0, cnt                     # streaming kernels, no second pass
    # a blob the streaming kernels must refuse on the device: wrong checksum -> Failed from the general path
    arr = cases.terrain(16, 512, rng).astype(np.float32)
    rc, blob = O.encode(arr, 0.01)
    bad = bytearray(blob)
    bad[len(bad) // 2] ^= 0x10
    rc2, _, _, cnt = _device_decode(S, bytes(bad), arr.shape, np.float32)
    assert rc2 == 1
    # a masked blob is not theirs either, and still decodes
    m = np.ones(arr.shape, np.uint8)
    m[3:9, 100:200] = 0
    rc, blob = O.encode(arr, 0.01, mask=m)
    want = O.decode(blob)
    rc2, got, valid, cnt = _device_decode(S, blob, arr.shape, np.float32, mask=True)
    assert rc2 == 0 and cnt[3] == 1 and np.array_equal(valid.reshape(m.shape), m)
    assert _same(want[1].reshape(arr.shape) * m, got * m)


@pytest.mark.ref
def test_sim_streaming_decode_of_older_codec_versions(libs):
    """Header layouts of codec 3, 4 and 5 (no nDepth / no nBlobsMore / no noData fields) through k_fast_header."""
    import ctypes as ct
    R = capi.ref()
    if R is None:
        pytest.skip("reference library not built")
    O, S = libs
    rng = np.random.default_rng(17)
    for dt, e in ((np.float32, 0.01), (np.uint16, 0), (np.float64, 0.1)):
        arr = cases._cast(cases.terrain(16, 1024, rng, amp=300, base=1000, sigma=1.5), dt)
        for ver in (3, 4, 5):
            buf = np.empty(arr.nbytes + 4096, np.uint8)
            n = ct.c_uint(0)
            rc = R.lib.lerc_encodeForVersion(arr.ctypes.data, ver, capi.dt_code(dt), 1, arr.shape[1], arr.shape[0], 1, 0, None,
                                             float(e), buf.ctypes.data, buf.size, ct.byref(n))
            assert rc == 0
            blob = buf[:n.value].tobytes()
            want = R.decode(blob)
            c0 = S.path_counters()
            got = S.decode(blob)
            c1 = S.path_counters()
            assert want[0] == got[0] == 0 and _same(want[1], got[1])
            assert c1[2] == c0[2] + 1, (np.dtype(dt).name, ver, S.last_note())


def test_sim_tile_batches(libs):
    """lerc_amd_encode_tiles_device / decode_tiles_device: one launch sequence for a batch of tiles, every blob byte
    for byte what the per-tile call makes; tiles the streaming kernels hand back (constant, all-integer floats) are
    redone inside the call."""
    import ctypes as ct
    O, S = libs
    L = S.lib
    L.lerc_amd_create.restype = ct.c_void_p
    L.lerc_amd_create.argtypes = [ct.c_void_p]
    L.lerc_amd_destroy.argtypes = [ct.c_void_p]
    L.lerc_amd_encode_tiles_device.restype = ct.c_uint
    L.lerc_amd_encode_tiles_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int, ct.c_double, ct.c_void_p,
                                               ct.c_ulonglong, ct.c_void_p, ct.c_void_p, ct.c_void_p]
    L.lerc_amd_decode_tiles_device.restype = ct.c_uint
    L.lerc_amd_decode_tiles_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_uint,
                                               ct.c_void_p]
    h = L.lerc_amd_create(None)
    assert h
    rng = np.random.default_rng(4)
    try:
        for dt, e in ((np.float32, 0.01), (np.uint16, 0), (np.float64, 0.05)):
            # (24, 40): 15 blocks, one partly empty workgroup per tile; (20, 44): no whole blocks, tile by tile through the general kernels
            # (257, 257) / (33, 65): ragged tiles (Esri's elevation tiles are 257 x 257) through the batch kernels' ragged forms
            for (r, c, n_t) in ((256, 256, 5), (64, 128, 6), (24, 40, 3), (200, 200, 4), (20, 44, 3), (257, 257, 3), (33, 65, 5)):
                tiles = np.stack([cases._cast(cases.terrain(r, c, rng, amp=300, base=1000 + 10 * t, sigma=1.5), dt) for t in range(n_t)])
                if n_t >= 5:
                    tiles[2] = tiles[2].flat[0]
                    if np.dtype(dt).kind == "f":
                        tiles[3] = np.rint(tiles[3])
                src = _aligned(tiles.nbytes).view(dt).reshape(tiles.shape)
                src[...] = tiles
                arena = _aligned(tiles.nbytes + n_t * 256)
                offs, sizes, used = np.zeros(n_t, np.uint64), np.zeros(n_t, np.uint32), ct.c_ulonglong(0)
                rc = L.lerc_amd_encode_tiles_device(h, src.ctypes.data, capi.dt_code(dt), c, r, n_t, float(e), arena.ctypes.data, arena.size,
                                                    offs.ctypes.data, sizes.ctypes.data, ct.byref(used))
                assert rc == 0
                for t in range(n_t):
                    r1, b1 = O.encode(tiles[t], e)
                    assert r1 == 0 and offs[t] % 16 == 0 and int(offs[t]) + int(sizes[t]) <= used.value
                    assert arena[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() == b1, (np.dtype(dt).name, r, c, t)
                out = _aligned(tiles.nbytes).view(dt).reshape(tiles.shape)
                rc = L.lerc_amd_decode_tiles_device(h, arena.ctypes.data, offs.ctypes.data, sizes.ctypes.data, n_t, c, r, capi.dt_code(dt),
                                                    out.ctypes.data)
                assert rc == 0
                for t in range(n_t):
                    want = O.decode(arena[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes())
                    assert _same(want[1].reshape(r, c), out[t])
        # an arena that is too small
        tiles = np.stack([cases.terrain(64, 128, rng).astype(np.float32) for _ in range(4)])
        src = _aligned(tiles.nbytes).view(np.float32).reshape(tiles.shape)
        src[...] = tiles
        arena = _aligned(4096)
        offs, sizes, used = np.zeros(4, np.uint64), np.zeros(4, np.uint32), ct.c_ulonglong(0)
        rc = L.lerc_amd_encode_tiles_device(h, src.ctypes.data, 6, 128, 64, 4, 0.01, arena.ctypes.data, arena.size, offs.ctypes.data,
                                            sizes.ctypes.data, ct.byref(used))
        assert rc == 3
    finally:
        L.lerc_amd_destroy(h)


def test_sim_tile_batches_when_the_arena_claim_is_never_answered():
    """Batches straight into the arena (FastFused::arenaCursor: a tile's last workgroup claims the tile's room, the others wait for its
    word) under the emulator, which runs workgroups one after the other: nobody in front of a tile's last workgroup ever gets an answer,
    every such workgroup gives up, says so, and the host encodes those tiles by themselves -- the hand-back path; same blobs."""
    import sys
    env = dict(os.environ, LERC_AMD_TILE_ARENA="cursor")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", "test_sim_tile_batches and not badly and not never_answered"],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200, cwd=capi.ROOT)
    assert out.returncode == 0 and b" passed" in out.stdout and b"failed" not in out.stdout, out.stdout.decode()[-2000:]


def test_sim_tile_batches_that_compress_badly(libs):
    """A batch whose tiles compress to more than half their raw size (lossless noise; a tiny error bound) does not fit the
    one-launch encoder's first slots: the batch is then encoded once more with slots that hold raw blocks -- one launch again,
    not tile after tile -- and every blob is the per-tile oracle blob; a batch with only a few such tiles keeps its slots and
    encodes those few behind it."""
    import ctypes as ct
    O, S = libs
    L = S.lib
    L.lerc_amd_create.restype = ct.c_void_p
    L.lerc_amd_create.argtypes = [ct.c_void_p]
    L.lerc_amd_destroy.argtypes = [ct.c_void_p]
    L.lerc_amd_path_counters.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    L.lerc_amd_encode_tiles_device.restype = ct.c_uint
    L.lerc_amd_encode_tiles_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int, ct.c_double, ct.c_void_p,
                                               ct.c_ulonglong, ct.c_void_p, ct.c_void_p, ct.c_void_p]
    h = L.lerc_amd_create(None)
    assert h
    rng = np.random.default_rng(41)
    try:
        for dt, e, n_t, n_noisy in ((np.int16, 0, 24, 24), (np.float32, 1e-5, 16, 16), (np.uint16, 0, 40, 3)):
            tiles = []
            for t in range(n_t):
                if t < n_noisy:
                    x = rng.integers(0, 30000, size=(128, 128)) if np.dtype(dt).kind != "f" else rng.normal(1000, 300, size=(128, 128))
                else:
                    x = cases.terrain(128, 128, rng, amp=300, base=1000, sigma=1.5)
                tiles.append(cases._cast(np.asarray(x, np.float64), dt))
            tiles = np.stack(tiles)
            src = _aligned(tiles.nbytes).view(dt).reshape(tiles.shape)
            src[...] = tiles
            arena = _aligned(2 * tiles.nbytes + n_t * 512)
            offs, sizes, used = np.zeros(n_t, np.uint64), np.zeros(n_t, np.uint32), ct.c_ulonglong(0)
            c0 = (ct.c_ulonglong * 4)()
            L.lerc_amd_path_counters(h, c0)
            L.lerc_amd_profile_enable.argtypes = [ct.c_void_p, ct.c_int]
            L.lerc_amd_profile_read.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int]
            L.lerc_amd_profile_enable(h, 1)
            rc = L.lerc_amd_encode_tiles_device(h, src.ctypes.data, capi.dt_code(dt), 128, 128, n_t, float(e), arena.ctypes.data, arena.size,
                                                offs.ctypes.data, sizes.ctypes.data, ct.byref(used))
            assert rc == 0
            L.lerc_amd_profile_enable(h, 0)
            buf = ct.create_string_buffer(1 << 14)
            L.lerc_amd_profile_read(h, buf, len(buf), 1)
            launches = {ln.split()[0]: int(ln.split()[2]) for ln in buf.value.decode().splitlines()}
            c1 = (ct.c_ulonglong * 4)()
            L.lerc_amd_path_counters(h, c1)
            spans = []
            for t in range(n_t):
                r1, b1 = O.encode(tiles[t], e)
                assert r1 == 0 and arena[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() == b1, (np.dtype(dt).name, t)
                spans.append((int(offs[t]), int(offs[t]) + int(sizes[t])))
            spans.sort()
            assert all(spans[i][1] <= spans[i + 1][0] for i in range(n_t - 1)) and spans[-1][1] <= used.value
            if n_noisy == n_t:    # the whole batch went through the batch kernels (second time round), none tile by tile
                assert c1[0] - c0[0] == n_t and c1[1] == c0[1], (np.dtype(dt).name, list(c0), list(c1))
                assert launches.get("fast_encode1") == 2, launches
            else:                 # the batch, then the few tiles that did not fit
                assert launches.get("fast_encode1") == 1 + n_noisy, launches
    finally:
        L.lerc_amd_destroy(h)


def test_sim_tile_batches_with_a_slot_per_tile(libs):
    """lerc_amd_encode_tiles_device_slots / decode_tiles_device_slots: tile t's blob at t * slotBytes, written there by the
    encode kernel itself (no packing pass); bytes are the per-tile call's, tiles the streaming kernels hand back are redone
    into their slot, a tile that does not fit its slot is BufferTooSmall."""
    import ctypes as ct
    O, S = libs
    L = S.lib
    L.lerc_amd_create.restype = ct.c_void_p
    L.lerc_amd_create.argtypes = [ct.c_void_p]
    L.lerc_amd_destroy.argtypes = [ct.c_void_p]
    L.lerc_amd_encode_tiles_device_slots.restype = ct.c_uint
    L.lerc_amd_encode_tiles_device_slots.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int, ct.c_double, ct.c_void_p,
                                                     ct.c_ulonglong, ct.c_void_p]
    L.lerc_amd_decode_tiles_device_slots.restype = ct.c_uint
    L.lerc_amd_decode_tiles_device_slots.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_ulonglong, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_uint,
                                                     ct.c_void_p]
    h = L.lerc_amd_create(None)
    assert h
    rng = np.random.default_rng(41)
    try:
        for dt, e in ((np.float32, 0.01), (np.uint16, 0), (np.float64, 0.05)):
            for (r, c, n_t) in ((256, 256, 5), (64, 128, 6), (24, 40, 3), (20, 44, 3), (257, 257, 3), (33, 65, 5)):
                tiles = np.stack([cases._cast(cases.terrain(r, c, rng, amp=300, base=1000 + 10 * t, sigma=1.5), dt) for t in range(n_t)])
                if n_t >= 5:
                    tiles[2] = tiles[2].flat[0]
                    if np.dtype(dt).kind == "f":
                        tiles[3] = np.rint(tiles[3])
                src = _aligned(tiles.nbytes).view(dt).reshape(tiles.shape)
                src[...] = tiles
                slot = (tiles[0].nbytes + 256 + 15) // 16 * 16
                slots = _aligned(n_t * slot)
                slots[...] = 0xEE
                sizes = np.zeros(n_t, np.uint32)
                rc = L.lerc_amd_encode_tiles_device_slots(h, src.ctypes.data, capi.dt_code(dt), c, r, n_t, float(e), slots.ctypes.data, slot, sizes.ctypes.data)
                assert rc == 0
                for t in range(n_t):
                    r1, b1 = O.encode(tiles[t], e)
                    assert r1 == 0 and slots[t * slot:t * slot + int(sizes[t])].tobytes() == b1, (np.dtype(dt).name, r, c, t)
                out = _aligned(tiles.nbytes).view(dt).reshape(tiles.shape)
                rc = L.lerc_amd_decode_tiles_device_slots(h, slots.ctypes.data, slot, sizes.ctypes.data, n_t, c, r, capi.dt_code(dt), out.ctypes.data)
                assert rc == 0
                for t in range(n_t):
                    want = O.decode(slots[t * slot:t * slot + int(sizes[t])].tobytes())
                    assert _same(want[1].reshape(r, c), out[t])
        # slots that are too small for the blobs, a slot size that is no multiple of 16
        tiles = np.stack([cases.terrain(64, 128, rng).astype(np.float32) for _ in range(4)])
        src = _aligned(tiles.nbytes).view(np.float32).reshape(tiles.shape)
        src[...] = tiles
        slots = _aligned(4 * 1024)
        sizes = np.zeros(4, np.uint32)
        assert L.lerc_amd_encode_tiles_device_slots(h, src.ctypes.data, 6, 128, 64, 4, 0.01, slots.ctypes.data, 1024, sizes.ctypes.data) == 3
        assert L.lerc_amd_encode_tiles_device_slots(h, src.ctypes.data, 6, 128, 64, 4, 0.01, slots.ctypes.data, 1000, sizes.ctypes.data) == 2
    finally:
        L.lerc_amd_destroy(h)


def test_sim_masked_bands_take_the_one_launch_encoder(libs):
    """A band with a validity mask (one value per pixel, 16 bits a pixel or more, any number of rows and columns): its block stream is made
    by the one-launch encoder's masked form -- any subset of a lane's pixels valid, elements placed by their rank among the block's
    valid pixels, blocks without a valid pixel one byte, the masked branch's "same as the value before" count -- straight into
    the band's place behind mask and ranges.  Bytes are the oracle's; the note says which kernels ran; too small a buffer is the
    oracle's status."""
    O, S = libs
    rng = np.random.default_rng(77)
    streamed = 0
    for dt, e in ((np.float32, 0.01), (np.uint16, 0), (np.float64, 0.001)):
        for shape in ((64, 64), (8, 8), (40, 520), (63, 65), (130, 67), (3, 300)):    # (the last three: rows / columns no multiples of 8)
            for style in (0, 1, 3, 5):
                r, c = shape
                x = cases._cast(cases.terrain(r, c, rng, amp=300, base=1000, sigma=2.0), dt) if style % 2 == 0 else cases.mixed_regions(r, c, rng, dt)
                m = np.ones((r, c), np.uint8)
                if style == 0:
                    for _ in range(6):
                        i0, j0 = int(rng.integers(0, r)), int(rng.integers(0, c))
                        m[i0:i0 + int(rng.integers(1, 40)), j0:j0 + int(rng.integers(1, 60))] = 0
                elif style == 1:
                    m = (rng.random((r, c)) > 0.3).astype(np.uint8)
                elif style == 2:
                    m[:, :c // 2] = 0
                elif style == 3:
                    m = (rng.random((r, c)) > 0.97).astype(np.uint8)
                elif style == 4:
                    m[::3, ::5] = 0
                else:
                    m[:] = 0
                    m[r // 2, c // 3] = 1
                    m[0, :] = 1
                if m.all() or not m.any():
                    m[0, 0] ^= 1
                r1, b1 = O.encode(x, e, mask=m)
                r2, b2 = S.encode(x, e, mask=m)
                assert r1 == r2 == 0 and b1 == b2, (np.dtype(dt).name, shape, style)
                streamed += "one-launch encoder" in S.last_note()
                d1, d2 = O.decode(b1), S.decode(b1)
                assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1]) and _same(d1[2], d2[2])
                if style == 0:
                    assert O.encode(x, e, mask=m, buf_size=len(b1) - 1)[0] == S.encode(x, e, mask=m, buf_size=len(b1) - 1)[0] == 3
    assert streamed >= 60


def test_sim_mask_coded_in_pieces(libs):
    """The host codes a large mask in pieces, cut where a run of five or more equal bytes ends (RLE.cpp's encoder starts afresh
    there), by several threads.  LERC_AMD_RLE_PIECE makes the pieces small, so that masks of test size are cut many times -- runs
    longer than 32767 bytes across the cuts included; the blobs are the oracle's (the knob is read once: a process of its own)."""
    import sys
    code = r"""
import sys, os
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, capi, cases
S, O = capi.sim(), capi.oracle()
rng = np.random.default_rng(5)
for it in range(24):
    r, c = int(rng.integers(1, 40)) * 8, int(rng.integers(1, 60)) * 8
    if it %% 3 == 0: r += int(rng.integers(0, 8)); c += int(rng.integers(0, 8))
    if it == 23: r, c = 160, 4096
    x = cases._cast(cases.terrain(r, c, rng, amp=300, base=1000, sigma=2.0), np.uint16)
    m = np.ones((r, c), np.uint8)
    style = it %% 6
    if style == 0:
        for _ in range(8):
            i0, j0 = int(rng.integers(0, r)), int(rng.integers(0, c)); m[i0:i0 + int(rng.integers(1, 60)), j0:j0 + int(rng.integers(1, 200))] = 0
    elif style == 1: m = (rng.random((r, c)) > 0.3).astype(np.uint8)
    elif style == 2: m[:, :c // 2] = 0
    elif style == 3: m = (rng.random((r, c)) > 0.999).astype(np.uint8); m[0, 0] = 1
    elif style == 4: m[r // 3:, :] = 0
    else: m[:] = (np.arange(c)[None, :] // 41 + np.arange(r)[:, None] // 3) %% 2
    if it == 23: m[:] = 1; m[: r // 2 + 3, :] = 0; m[5, 77] = 1
    if m.all() or not m.any(): m[0, 0] ^= 1
    r1, b1 = O.encode(x, 0, mask=m); r2, b2 = S.encode(x, 0, mask=m)
    assert r1 == r2 == 0 and b1 == b2, (it, r, c, style)
    d1, d2 = O.decode(b1), S.decode(b1)    # (the mask's way back: on the host, or -- with the knob -- rle_kernels.hip's decoder)
    assert d1[0] == d2[0] == 0 and np.array_equal(d1[2], d2[2]) and np.array_equal(d1[1].reshape(r, c) * (d1[2].reshape(r, c) != 0), d2[1].reshape(r, c) * (d2[2].reshape(r, c) != 0)), (it, r, c, style)
print("pieces ok")
""" % (capi.ROOT,)
    for piece in ("16", "4096"):
        env = dict(os.environ, LERC_AMD_RLE_PIECE=piece, LERC_AMD_DEVICE_RLE="0")
        out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        assert out.returncode == 0 and b"pieces ok" in out.stdout, out.stdout.decode()[-2000:]
    # ... and the same masks through the device's coder (rle_kernels.hip: every byte decides for itself whether it lies in a
    # run, two scans say where its segment begins and ends) -- which takes masks of 256 KB and more; the knob makes it take all
    env = dict(os.environ, LERC_AMD_DEVICE_RLE="16")
    out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert out.returncode == 0 and b"pieces ok" in out.stdout, out.stdout.decode()[-2000:]


def test_sim_several_bands_with_a_mask_each_decoded_on_the_device(libs):
    """Four bands, each with its own noisy mask, the masks' run-length streams decoded on the device (LERC_AMD_DEVICE_RLE=16): a
    band's tables in the workspace are sized for one band and every band starts where the first one did (codec_decode.cpp) --
    they used to pile up until a band found no room and the call failed on a blob the library's own encoder had written."""
    import sys
    code = r"""
import sys, os
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, capi, cases
S, O = capi.sim(), capi.oracle()
rng = np.random.default_rng(77)
for (nb, r, c, dt, e) in ((16, 256, 400, np.float32, 0.01), (3, 200, 264, np.uint16, 0), (5, 96, 520, np.uint8, 0)):    # (the first one failed)
    x = np.stack([cases._cast(cases.terrain(r, c, rng, amp=300, base=1000, sigma=2.0) + 7 * k, dt) for k in range(nb)])
    m = (rng.random((nb, r, c)) > 0.5).astype(np.uint8)
    r1, b1 = O.encode(x, e, n_bands=nb, mask=m); r2, b2 = S.encode(x, e, n_bands=nb, mask=m)
    assert r1 == r2 == 0 and b1 == b2, (nb, r, c)
    d1, d2 = O.decode(b1, want_masks=nb, n_bands=nb), S.decode(b1, want_masks=nb, n_bands=nb)
    assert d1[0] == d2[0] == 0, (d1[0], d2[0], nb, r, c)
    assert np.array_equal(d1[2], d2[2]), (nb, r, c)
    v = d1[2].reshape(nb, r, c) != 0
    assert np.array_equal(d1[1].reshape(nb, r, c)[v], d2[1].reshape(nb, r, c)[v]), (nb, r, c)
print("bands ok")
""" % (capi.ROOT,)
    for knob in ("16", "0"):
        env = dict(os.environ, LERC_AMD_DEVICE_RLE=knob)
        out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        assert out.returncode == 0 and b"bands ok" in out.stdout, out.stdout.decode()[-2000:]


def _rle_restated(b):
    """RLE::compress (RLE.cpp:123-254) said plainly: in a literal stretch a run opens where five equal bytes start and one more
    byte follows; it takes every byte equal to its first; stretches and runs are cut at 32767; -32768 ends the stream"""
    n, out, i = len(b), bytearray(), 0

    def cnt(v):
        out.extend(int(v & 0xFFFF).to_bytes(2, "little"))
    while i < n:
        lit = i
        while i < n and not (i + 5 < n and b[i] == b[i + 1] == b[i + 2] == b[i + 3] == b[i + 4]):
            i += 1
        while lit < i:
            ln = min(32767, i - lit)
            cnt(ln)
            out.extend(b[lit:lit + ln])
            lit += ln
        if i >= n:
            break
        t = i
        while t + 1 < n and b[t + 1] == b[i]:
            t += 1
        left = t - i + 1
        while left > 0:
            ln = min(32767, left)
            cnt(-ln)
            out.append(b[i])
            left -= ln
        i = t + 1
    cnt(-32768)
    return bytes(out)


def rle_cases(rng):
    out = []
    for n in (1, 2, 5, 6, 7, 15, 16, 17, 31, 33, 100, 1000, 4096, 70000):
        out.append(rng.integers(0, 256, n).astype(np.uint8))                      # noise: one long literal stretch
        out.append(np.zeros(n, np.uint8))                                          # one run
        k = max(1, n // 7 + 1)
        x = np.repeat(rng.integers(0, 3, k).astype(np.uint8) * 127, rng.integers(1, 14, k))[:n]
        out.append(np.concatenate([x, np.zeros(n - len(x), np.uint8)]).astype(np.uint8))    # short runs and literals mixed
        y = np.zeros(n, np.uint8)
        y[rng.integers(0, n, max(1, n // 50))] = rng.integers(1, 256, max(1, n // 50))
        out.append(y)                                                              # runs with single bytes in between
        z = rng.integers(0, 256, n).astype(np.uint8)
        z[n // 3:n // 3 + n // 2] = 0xFF
        out.append(z)
        w = np.full(n, 7, np.uint8)
        w[:max(0, n - 5)] = rng.integers(0, 256, max(0, n - 5))
        out.append(w)                                                              # exactly five equal bytes at the end: no run
    for n in (32767, 32768, 32767 * 2 + 5, 32767 * 3):
        out.append(np.full(n, 0xAA, np.uint8))                                     # runs cut at 32767
        c = (np.arange(n) % 3).astype(np.uint8)
        out.append(c)                                                              # a literal stretch cut at 32767
    return out


def check_device_rle(L, h):
    import ctypes as ct
    L.lerc_amd_mask_rle_device.restype = ct.c_uint
    L.lerc_amd_mask_rle_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_void_p, ct.c_uint, ct.POINTER(ct.c_uint)]
    rng = np.random.default_rng(9)
    for k, b in enumerate(rle_cases(rng)):
        n = len(b)
        src = _aligned(max(n, 16))
        src[:n] = b
        want = _rle_restated(bytes(b))
        out = _aligned(len(want) + 64)
        size = ct.c_uint(0)
        rc = L.lerc_amd_mask_rle_device(h, src.ctypes.data, n, out.ctypes.data, out.size, ct.byref(size))
        assert rc == 0 and out[:size.value].tobytes() == want, (k, n, rc, size.value, len(want))
    src = _aligned(1000)
    src[:] = rng.integers(0, 256, 1000).astype(np.uint8)
    out = _aligned(100)
    assert L.lerc_amd_mask_rle_device(h, src.ctypes.data, 1000, out.ctypes.data, 100, ct.byref(ct.c_uint(0))) == 3    # BufferTooSmall


def _rle_decode_restated(src, n_out):
    """RLE::decompress (RLE.cpp:259-330) said plainly; None for a stream the reference refuses"""
    out, at, left, i = bytearray(n_out), 0, len(src), 0
    while True:
        if left < 2:
            return None
        cnt = int.from_bytes(src[i:i + 2], "little", signed=True)
        i += 2
        left -= 2
        if cnt == -32768:
            return bytes(out)
        n = abs(cnt)
        payload = n if cnt > 0 else 1
        if left < payload + 2 or at + n > n_out:
            return None
        out[at:at + n] = src[i:i + n] if cnt > 0 else bytes([src[i]]) * n
        at += n
        i += payload
        left -= payload


def check_device_rle_decode(L, h, run=None):
    """run(stream, n_out) -> (status, n_out decoded bytes); default: the emulator's, on host memory"""
    import ctypes as ct
    L.lerc_amd_mask_rle_decode_device.restype = ct.c_uint
    L.lerc_amd_mask_rle_decode_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_void_p, ct.c_uint]
    rng = np.random.default_rng(10)

    def run_host(stream, n_out):
        src = _aligned(len(stream) + 16)
        src[:len(stream)] = np.frombuffer(stream, np.uint8)
        out = _aligned(n_out + 64)
        out[:] = 0xA5
        rc = L.lerc_amd_mask_rle_decode_device(h, src.ctypes.data, len(stream), out.ctypes.data, n_out)
        assert (out[n_out:] == 0xA5).all()
        return rc, out[:n_out].tobytes()
    run = run or run_host

    cases_ = rle_cases(rng)
    # masks as rasters make them: rectangles of invalid pixels (several pieces and sub-pieces of stream), and one stream of many MB
    i = np.arange(1200).reshape(-1, 1)
    j = np.arange(4096).reshape(1, -1)
    cases_.append(np.packbits((((i // 97) + (j // 131)) % 10 != 0).astype(np.uint8)))
    cases_.append(np.packbits((rng.random(300000) > 0.03).astype(np.uint8)))
    for k, b in enumerate(cases_):
        stream = _rle_restated(bytes(b))
        rc, got = run(stream, len(b))
        assert rc == 0 and got == bytes(b), (k, len(b), rc)
        if len(b) > 8:    # a stream that holds less than the mask: the rest stays zero
            rc, got = run(stream, len(b) + 37)
            assert rc == 0 and got == bytes(b) + bytes(37), (k, len(b), rc)
            rc, _ = run(stream, len(b) - 1)                      # ... and more: refused
            assert rc == 1, (k, rc)
    # damaged streams: the verdict is the restated decoder's (no end marker, a segment that runs over the end, garbage)
    for k in range(60):
        b = cases_[(7 * k) % len(cases_)]
        stream = bytearray(_rle_restated(bytes(b)))
        if k % 3 == 0:
            stream = stream[:max(2, len(stream) - 1 - int(rng.integers(0, min(40, len(stream) - 1))))]
        elif k % 3 == 1:
            stream[int(rng.integers(0, len(stream)))] ^= 1 << int(rng.integers(0, 8))
        else:
            stream = bytearray(rng.integers(0, 256, int(rng.integers(2, 3000))).astype(np.uint8).tobytes())
        want = _rle_decode_restated(bytes(stream), len(b))
        rc, got = run(bytes(stream), len(b))
        assert (rc == 0) == (want is not None), (k, rc, want is None)
        if want is not None:
            assert got == want, k


def test_sim_device_mask_rle_decode(libs):
    """lerc_amd_mask_rle_decode_device: the way back (rle_kernels.hip: hops by pointer doubling, a chain over 8 KiB pieces, a wave
    per 256 bytes of stream) against RLE::decompress said plainly, incl. damaged streams."""
    import ctypes as ct
    O, S = libs
    L = S.lib
    L.lerc_amd_create.restype = ct.c_void_p
    L.lerc_amd_create.argtypes = [ct.c_void_p]
    L.lerc_amd_destroy.argtypes = [ct.c_void_p]
    h = L.lerc_amd_create(None)
    assert h
    try:
        check_device_rle_decode(L, h)
    finally:
        L.lerc_amd_destroy(h)


def test_sim_device_mask_rle(libs):
    """lerc_amd_mask_rle_device: the run-length coding of validity bits on the device (rle_kernels.hip) against RLE::compress
    said plainly -- noise, single runs, mixtures, runs and stretches longer than 32767, five equal bytes at the very end."""
    import ctypes as ct
    O, S = libs
    L = S.lib
    L.lerc_amd_create.restype = ct.c_void_p
    L.lerc_amd_create.argtypes = [ct.c_void_p]
    L.lerc_amd_destroy.argtypes = [ct.c_void_p]
    h = L.lerc_amd_create(None)
    assert h
    try:
        check_device_rle(L, h)
    finally:
        L.lerc_amd_destroy(h)


def test_sim_damaged_mask_streams_in_front_of_the_huffman_and_one_sweep_kernels(libs):
    """A mask whose run-length stream is damaged, in a band coded by the 8-bit Huffman mode or in one sweep: those kernels take the
    mask's word for which pixels the stream holds.  With the mask decoded on the device the verdict on its stream used to come with
    the call's last wait -- after k_huff_emit had divided a rank by a valid count of zero (found by tools/fuzz_sim_masked.py: SIGFPE
    under the emulator).  The mask is checked against the header's count in front of those kernels now; same verdicts as the oracle's
    on every flipped bit of the mask section, on the host's decoder and (LERC_AMD_DEVICE_RLE=16) the device's."""
    import sys
    code = r"""
import sys, os, struct
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, capi, cases
S, O = capi.sim(), capi.oracle()
rng = np.random.default_rng(87)
n = 0
for dt, e, shape in ((np.int8, 0, (65, 186)), (np.uint8, 0, (40, 96)), (np.float32, 1e-7, (33, 70))):
    r, c = shape
    x = cases.terrain(r, c, rng, amp=50, base=100, sigma=3.0 if dt == np.float32 else 0.3)
    x = cases._cast(x / 8 if np.dtype(dt).itemsize == 1 else x * 1000.123, dt)    # (float: noise no block can quantise -> one sweep)
    m = np.ones((r, c), np.uint8); m[:, : c // 2] = 0; m[r // 2, 3] = 1; m[3:9, c // 2 + 5: c // 2 + 30] = 0
    r1, b1 = O.encode(x, e, mask=m)
    assert r1 == 0
    n_mask = struct.unpack_from("<I", b1, 90)[0]
    assert n_mask > 8
    d1, d2 = O.decode(b1), S.decode(b1)
    assert d1[0] == d2[0] == 0 and np.array_equal(d1[2], d2[2])
    for k in range(60):
        bb = bytearray(b1)
        bb[94 + int(rng.integers(0, n_mask))] ^= 1 << int(rng.integers(0, 8))
        a, b = O.decode(bytes(bb)), S.decode(bytes(bb))
        assert (a[0] == 0) == (b[0] == 0), (np.dtype(dt).name, k, a[0], b[0])
        n += 1
print("masks ok", n)
""" % (capi.ROOT,)
    for knob in ("0", "16"):
        env = dict(os.environ, LERC_AMD_DEVICE_RLE=knob)
        out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
        assert out.returncode == 0 and b"masks ok" in out.stdout, out.stdout.decode()[-2000:]


COUNT_MISMATCH_CODE = r"""
import sys, os, struct
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, capi, cases
P, O, R = getattr(capi, %r)(), capi.oracle(), capi.ref()
checkers = [O] + ([R] if R is not None else [])

def fletcher32(b):
    # Lerc2::ComputeChecksumFletcher32 (Lerc2.cpp:1037-1064) on the bytes behind the checksum field
    a = np.frombuffer(b[: len(b) & ~1], np.uint8).astype(np.uint64)
    w = (a[0::2] << 8) | a[1::2]
    n = len(w)
    s1 = 0xffff + int(w.sum())
    s2 = 0xffff * (n + 1) + int((w * np.arange(n, 0, -1, dtype=np.uint64)).sum())
    if len(b) & 1:
        s1 += b[-1] << 8; s2 += s1
    return ((s2 %% 65535 or 65535) << 16) | (s1 %% 65535 or 65535)

def reseal(bb):
    bb = bytearray(bb)
    struct.pack_into("<I", bb, 10, fletcher32(bytes(bb[14:])))
    return bytes(bb)

rng = np.random.default_rng(87)
n = 0
for dt, e, shape in ((np.int8, 0, (65, 186)), (np.uint8, 0, (40, 96)), (np.float32, 1e-7, (33, 70)), (np.float64, 1e-12, (24, 40))):
    r, c = shape
    x = cases.terrain(r, c, rng, amp=50, base=100, sigma=3.0 if np.dtype(dt).kind == "f" else 0.3)
    x = cases._cast(x / 8 if np.dtype(dt).itemsize == 1 else x * 1000.123, dt)    # (floats: noise no block can quantise -> one sweep)
    m = np.ones((r, c), np.uint8); m[:, : c // 2] = 0; m[r // 2, 3] = 1; m[3:9, c // 2 + 5: c // 2 + 30] = 0
    r1, b1 = O.encode(x, e, mask=m)
    assert r1 == 0 and reseal(b1) == b1, "the test's checksum is not the codec's"
    nv = struct.unpack_from("<i", b1, 26)[0]
    assert nv == int(m.sum())
    tb = np.dtype(dt).itemsize
    n_mask = struct.unpack_from("<I", b1, 90)[0]
    one_sweep = b1[94 + n_mask + 2 * tb] == 1
    assert one_sweep == (np.dtype(dt).kind == "f")
    crafted = []
    for delta in (-1, 1, 1 - nv, 5, -20):    # the header names another count than the mask holds, the stream is whole
        bb = bytearray(b1); struct.pack_into("<i", bb, 26, nv + delta); crafted.append(reseal(bb))
    if one_sweep:
        # the header says ONE valid pixel, the mask holds hundreds, the stream is cut to one pixel: by the header's count it is long
        # enough, by the mask's (Lerc2::ReadDataOneSweep, Lerc2.cpp:1379-1385) it is not -- and the kernel reads by the mask's ranks
        pay = 94 + n_mask + 2 * tb + 1
        bb = bytearray(b1[:pay + tb]); struct.pack_into("<i", bb, 26, 1); struct.pack_into("<i", bb, 34, len(bb)); crafted.append(reseal(bb))
        bb = bytearray(b1[:pay + tb * (nv - 1)]); struct.pack_into("<i", bb, 26, nv - 1); struct.pack_into("<i", bb, 34, len(bb)); crafted.append(reseal(bb))
    for k, bb in enumerate(crafted):
        got = P.decode(bb)
        for L in checkers:
            want = L.decode(bb)
            assert (want[0] == 0) == (got[0] == 0), (np.dtype(dt).name, k, want[0], got[0])
            if want[0] == 0:
                assert np.array_equal(want[1].view(np.uint8), got[1].view(np.uint8)) and np.array_equal(want[2], got[2]), (np.dtype(dt).name, k)
        if one_sweep and k >= 5: assert got[0] != 0
        n += 1
print("counts ok", n)
"""


def test_sim_header_and_mask_disagree_on_the_valid_count(libs):
    """Behind a VALID checksum the header names another number of valid pixels than the mask holds (a crafted blob; round-5 review: with
    the stream cut to the header's count the one-sweep kernel, which reads by the mask's ranks, read past the blob).  The reference asks
    the mask, never the header (Lerc2::ReadDataOneSweep, Lerc2.cpp:1379-1385; DecodeHuffman goes by the mask's bits): same verdicts and
    same pixels as the oracle and the real reference, with the mask decoded by the host and (LERC_AMD_DEVICE_RLE=16) by the device."""
    import sys
    for knob in ("0", "16"):
        env = dict(os.environ, LERC_AMD_DEVICE_RLE=knob)
        out = subprocess.run([sys.executable, "-c", COUNT_MISMATCH_CODE % (capi.ROOT, "sim")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
        assert out.returncode == 0 and b"counts ok" in out.stdout, out.stdout.decode()[-2000:]


def mask_and_stats_cases(rng):
    """float rasters with a mask whose values lie on a grid of 0.1 / 0.01 / 0.5 / whole numbers -- TryRaiseMaxZError raises the
    error bound, or a first row promises it (the candidates are pruned on it, codec_encode.cpp) and a later row does not --,
    NaNs under and beside the mask"""
    out = []
    for dt in (np.float32, np.float64):
        for k, (digits, e) in enumerate(((1, 0.01), (2, 0.001), (0, 0.3), (1, 0.04), (None, 0.01))):
            r, c = 64 + 16 * k, 128
            x = 1000 + 50 * np.sin(np.arange(c)[None, :] / 30.0) + rng.standard_normal((r, c))
            x = np.round(x * 2) / 2 if digits is None else np.round(x, digits)
            x = x.astype(dt)
            m = (rng.random((r, c)) > 0.15).astype(np.uint8)
            m[r // 3:r // 3 + 9, 20:90] = 0
            out.append((f"{np.dtype(dt).name} grid {digits} e {e}", x, e, m))
            y = x.copy()
            y[1:, :] += dt(0.013) * (rng.random((r - 1, c)) > 0.5)        # the first row keeps its promise, the others do not
            out.append((f"{np.dtype(dt).name} grid {digits} e {e}, rows 1.. off the grid", y, e, m))
            z = x.copy()
            z[m == 0] = np.nan                                           # NaN under the mask: nothing changes
            z[5, 7] = np.nan
            m2 = m.copy()
            m2[5, 7] = 1                                                 # ... and one at a valid pixel: it leaves the mask
            out.append((f"{np.dtype(dt).name} grid {digits} e {e}, NaNs", z, e, m2))
    return out


def test_sim_try_raise_with_a_mask(libs):
    """same blobs as the oracle's, whose TryRaiseMaxZError and mask filter are the reference's (a mask's statistics and the first
    row's errors come out of one wait)"""
    O, S = libs
    rng = np.random.default_rng(33)
    raised = 0
    for name, x, e, m in mask_and_stats_cases(rng):
        r1, b1 = O.encode(x, e, mask=m)
        r2, b2 = S.encode(x, e, mask=m)
        assert r1 == r2 and b1 == b2, name
        if r1 == 0:
            d1, d2 = O.decode(b1), S.decode(b1)
            assert d1[0] == d2[0] == 0 and _same(d1[2], d2[2]), name
            raised += int(O.blob_info(b1)[2][2] > e * 1.5)    # (dataRangeArray[2]: the error bound the blob was coded with)
    assert raised >= 4, raised


@pytest.mark.parametrize("knob", ["0", "8", "16", "24"])
def test_sim_block_offsets_by_four_lanes_a_chunk(libs, knob):
    """k_walk_emit_sub: a chunk's block offsets are written by four lanes, three of which start where k_rank_chunks saw a
    candidate's chain enter their KiB.  The first lane checks that it arrives at the same place with the same block index; the
    knobs make it distrust the landings (8), make the landings wrong by a byte (16), or both: same pixels every time.  Masked
    and ragged rasters of every type that takes this path (8 x 8 blocks, one value per pixel), several chunks long."""
    import sys
    env = dict(os.environ, LERC_AMD_TEST_GIVEUP=knob)
    out = subprocess.run([sys.executable, "-c", four_lanes_code("sim")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200)
    assert out.returncode == 0 and b"offsets ok" in out.stdout, out.stdout.decode()[-2000:]


def four_lanes_code(which):
    """the script of test_sim_block_offsets_by_four_lanes_a_chunk (a process of its own: the knob is read once); which: "sim" or
    "product" (the GPU suite runs it on the device)"""
    return r"""
import sys, os
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, capi, cases
S, O = capi.%s(), capi.oracle()
rng = np.random.default_rng(12)
n = 0
for dt, e in ((np.float32, 0.01), (np.uint16, 0), (np.int32, 1), (np.float64, 0.001), (np.uint8, 0), (np.int16, 2)):
    for r, c in ((96, 512), (131, 397)):
        x = cases._cast(cases.terrain(r, c, rng, amp=300, base=1000, sigma=1.5) / (8 if np.dtype(dt).itemsize == 1 else 1), dt)
        for style in range(3):
            m = np.ones((r, c), np.uint8)
            if style == 0:
                i = np.arange(r).reshape(-1, 1); j = np.arange(c).reshape(1, -1)
                m = (((i // 13) + (j // 37)) %% 5 != 0).astype(np.uint8)
            elif style == 1:
                m = (rng.random((r, c)) > 0.1).astype(np.uint8)
            elif (r %% 8 == 0 and c %% 8 == 0):
                continue    # (no mask, whole blocks: the streaming kernels' raster)
            r1, b1 = O.encode(x, e, mask=m)
            assert r1 == 0
            d1, d2 = O.decode(b1), S.decode(b1)
            assert d1[0] == d2[0] == 0 and np.array_equal(d1[2], d2[2]), (np.dtype(dt).name, r, c, style)
            v = d1[2].reshape(r, c) != 0 if d1[2] is not None else np.ones((r, c), bool)
            assert np.array_equal(np.where(v, d1[1].reshape(r, c), 0), np.where(v, d2[1].reshape(r, c), 0)), (np.dtype(dt).name, r, c, style)
            n += 1
            if style == 0 and len(b1) > 9000:    # a damaged copy: the same verdict
                bad = bytearray(b1); bad[len(bad) * 2 // 3] ^= 0x21
                assert (O.decode(bytes(bad))[0] == 0) == (S.decode(bytes(bad))[0] == 0)
print("offsets ok", n)
""" % (capi.ROOT, which)


def test_sim_bit_plane_mode(libs):
    """maxZErr == 777: Lerc2::TryBitPlaneCompression picks the error bound from neighbour XOR statistics
    (Lerc2.cpp:1071-1229) -- all integer types, with a mask, with nDepth > 1, too few pixels, float (refused)."""
    O, S = libs
    rng = np.random.default_rng(21)
    for dt in (np.uint8, np.int16, np.uint16, np.int32):
        x = (rng.integers(0, 60, (100, 120)) * 64 + rng.integers(0, 16, (100, 120))).astype(np.int64)
        if np.dtype(dt).kind == "i":
            x = x - 1500
        x = np.clip(x, np.iinfo(dt).min, np.iinfo(dt).max).astype(dt)
        m = (rng.random(x.shape) > 0.2).astype(np.uint8)
        x3 = np.stack([x, x // 2, x ^ 3], axis=-1).astype(dt)
        for arr, kw in ((x, {}), (x, dict(mask=m)), (x3, dict(n_depth=3))):
            r1, b1 = O.encode(arr, 777, **kw)
            r2, b2 = S.encode(arr, 777, **kw)
            assert r1 == r2 == 0 and b1 == b2, (np.dtype(dt).name, list(kw))
            assert O.blob_info(b1) == S.blob_info(b2)
    small = rng.integers(0, 1000, (40, 40)).astype(np.uint16)
    assert O.encode(small, 777) == S.encode(small, 777)
    f = rng.random((64, 64)).astype(np.float32)
    assert S.encode(f, 777)[0] == O.encode(f, 777)[0] == 1


def test_sim_nodata_values(libs):
    """lerc_encode_4D / lerc_decode_4D with per-band noData values (Lerc.cpp:1241-1552)."""
    O, S = libs
    T = capi.ref() or O
    for name, arr, e, kw in cases.nodata_fuzz_cases(50):
        cases.check_nodata_case(T, S, name, arr, e, kw, _same)


def test_sim_many_values_per_pixel(libs):
    """nDepth of several hundred (hyperspectral cubes): per-depth ranges, tiles, masks as the oracle's"""
    O, S = libs
    for name, arr, e, kw in cases.deep_pixel_cases():
        cases.check_deep_pixel_case(O, S, name, arr, e, kw, _same)


def test_sim_encode_for_older_codec_versions(libs):
    """lerc_encodeForVersion, codec 3..5: header layouts, no ranges before 4, no slice differences before 5,
    raw Huffman only from 4, lossless float as raw blocks, NaN -> mask, no all-integer promotion."""
    O, S = libs
    for name, arr, ver, e, kw in cases.old_codec_cases(60):
        cases.check_old_codec_case(O, S, name, arr, ver, e, kw, _same)


def test_sim_huffman_long_codes_and_many_subsequences(libs):
    """Code words beyond the look-up table, sub-sequences whose warm-up does not catch on (the workgroup chains them in
    LDS), spans assembled in LDS by the packer: blob == oracle blob, decode == input."""
    O, S = libs
    for name, arr, kw in cases.huffman_stress_cases():
        r1, b1 = O.encode(arr, 0, **kw)
        r2, b2 = S.encode(arr, 0, **kw)
        assert r1 == r2 == 0 and b1 == b2, name
        d = S.decode(b1)
        assert d[0] == 0 and np.array_equal(np.asarray(d[1]).reshape(arr.shape), arr), name


def _huff_device_decoder(S):
    """decode(blob, arr, kw) for cases.check_huffman_matrix_case: lerc_amd_decode_device through the emulator on a context with
    the profile on; the sync rounds are its huff_sync launches (one per host round trip of the sync loop)"""
    import ctypes as ct
    L = S.lib
    L.lerc_amd_create.restype = ct.c_void_p
    L.lerc_amd_create.argtypes = [ct.c_void_p]
    L.lerc_amd_destroy.argtypes = [ct.c_void_p]
    L.lerc_amd_last_error.argtypes = [ct.c_void_p]
    L.lerc_amd_last_error.restype = ct.c_char_p
    L.lerc_amd_profile_enable.argtypes = [ct.c_void_p, ct.c_int]
    L.lerc_amd_profile_read.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int]
    L.lerc_amd_decode_device.restype = ct.c_uint
    L.lerc_amd_decode_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int,
                                         ct.c_int, ct.c_uint, ct.c_void_p]

    def decode(blob, arr, kw):
        h = L.lerc_amd_create(None)
        assert h
        try:
            nd = kw.get("n_depth", 1)
            rows, cols = arr.shape[0], arr.shape[1]
            src = _aligned(len(blob), 256)
            src[:] = np.frombuffer(blob, np.uint8)
            out = _aligned(arr.nbytes).view(arr.dtype)
            has_mask = "mask" in kw
            valid = _aligned(rows * cols) if has_mask else None
            L.lerc_amd_profile_enable(h, 1)
            rc = L.lerc_amd_decode_device(h, src.ctypes.data, len(blob), 1 if has_mask else 0, valid.ctypes.data if has_mask else None,
                                          nd, cols, rows, 1, capi.dt_code(arr.dtype), out.ctypes.data)
            buf = ct.create_string_buffer(1 << 16)
            L.lerc_amd_profile_read(h, buf, len(buf), 1)
            rounds = sum(int(ln.split()[2]) for ln in buf.value.decode().splitlines() if ln.split()[0] == "huff_sync")
            return rc, out.copy(), (valid.copy() if has_mask else None), rounds, L.lerc_amd_last_error(h).decode()
        finally:
            L.lerc_amd_destroy(h)
    return decode


def test_sim_huffman_sync_matrix(libs):
    """cases.huffman_matrix_cases on the emulator (16 decoder threads a workgroup, 1 warm-up word): blob == the real reference's,
    decode == input == the reference's decode, and the sync takes at most 2 + ceil(log2(sub-sequences)) rounds -- code books
    whose words all have one length never fall into step on their own.  The stream offsets cover all four byte phases."""
    O, S = libs
    R = capi.ref() or O    # (the oracle only where the real reference was not built)
    dec = _huff_device_decoder(S)
    phases = set()
    for name, arr, kw, mode, kind in cases.huffman_matrix_cases(4):
        mis, _, _ = cases.check_huffman_matrix_case(R, S, dec, name, arr, kw, mode, kind, compute_units=256,
                                                    threads=huffblob.DEC_THREADS_SIM)
        phases.add(mis)
    assert phases == {0, 1, 2, 3}, phases


def test_sim_byte_rasters_priced_by_the_lane_per_block_kernel(libs):
    O, S = libs
    for name, arr, kw in cases.byte_tiling_cases():
        r1, b1 = O.encode(arr, 0, **kw)
        r2, b2 = S.encode(arr, 0, **kw)
        assert r1 == r2 == 0 and b1 == b2, name
        d = S.decode(b1)
        assert d[0] == 0 and np.array_equal(np.asarray(d[1]).reshape(arr.shape), arr), name


def test_sim_lossless_float_against_golden(libs):
    """maxZErr == 0 on float / double (IEM_DeltaDeltaHuffman): predictor and difference-order choices,
    plane coding (Huffman / one value / stored / PackBits), decode by scans -- against the reference's vectors."""
    import hashlib
    import json
    import os
    O, S = libs
    gold = os.path.join(capi.ROOT, "tests", "golden")
    vec = json.load(open(os.path.join(gold, "fpl_vectors.json")))
    cases.check_lossless_float_golden(S, vec, os.path.join(gold, "blobs"), lambda b: hashlib.sha256(bytes(b)).hexdigest())


@pytest.mark.ref
def test_sim_lossless_float_against_reference(libs):
    R = capi.ref()
    if R is None:
        pytest.skip("reference library not built")
    O, S = libs
    for name, arr, kw in cases.lossless_float_cases(40, seed=92):
        cases.check_lossless_float_case(R, S, name, arr, kw, _same)


def test_sim_lossless_float_damaged_blobs(libs):
    """flipped / overwritten bytes and truncation in lossless float blobs: same verdict as the oracle, no out-of-bounds walk
    (the emulator runs the kernels as host code, so a stray access would crash the test)"""
    O, S = libs
    rng = np.random.default_rng(5)
    for name, arr, kw in cases.lossless_float_cases(8, seed=7, max_side=60):
        rc, blob = O.encode(arr, 0, **kw)
        assert rc == 0
        for t in range(12):
            b = bytearray(blob)
            k = int(rng.integers(0, len(b)))
            how = int(rng.integers(0, 3))
            if how == 0:
                b[k] ^= 1 << int(rng.integers(0, 8))
            elif how == 1:
                b[k] = int(rng.integers(0, 256))
            else:
                b = b[:max(20, k)]
            b = bytes(b)
            assert (O.decode(b)[0] == 0) == (S.decode(b)[0] == 0), (name, k, how)


def test_sim_damaged_blobs_of_every_path(libs):
    """no stray access, no endless walk, the oracle's verdict -- whichever kernels the blob goes to"""
    O, S = libs
    for name, blob in cases.damaged_blob_cases(O, 6):
        cases.check_damaged_blob(O, S, name, blob, _same)


def test_sim_streaming_encode_of_several_bands(libs):
    """unmasked multi-band rasters: every band through the streaming kernels, "bands to follow" in each header"""
    O, S = libs
    rng = np.random.default_rng(31)
    for dt, e, shape in ((np.uint16, 0, (3, 16, 512)), (np.float32, 0.01, (2, 24, 200)), (np.float64, 0.001, (4, 8, 64)), (np.int32, 0, (2, 40, 328))):
        x = np.stack([cases._cast(cases.terrain(shape[1], shape[2], rng, amp=300, base=1000 + 50 * b, sigma=1.5), dt) for b in range(shape[0])])
        c0 = S.path_counters()
        assert O.compute_size(x, e, n_bands=shape[0]) == S.compute_size(x, e, n_bands=shape[0])
        r1, b1 = O.encode(x, e, n_bands=shape[0])
        r2, b2 = S.encode(x, e, n_bands=shape[0])
        assert r1 == r2 == 0 and b1 == b2, np.dtype(dt).name
        assert S.path_counters()[0] >= c0[0] + 2, (np.dtype(dt).name, S.last_note())
        d1, d2 = O.decode(b1), S.decode(b1)
        assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1])
    # one band that the streaming kernels hand back (constant): the whole call goes the general way, same bytes
    x = np.stack([cases._cast(cases.terrain(16, 512, rng), np.float32), np.full((16, 512), 2.5, np.float32)])
    assert O.encode(x, 0.01, n_bands=2) == S.encode(x, 0.01, n_bands=2)
    # output buffer too small for the second band
    x = np.stack([cases._cast(cases.terrain(16, 512, rng), np.float32)] * 2)
    rc, size = O.compute_size(x, 0.01, n_bands=2)
    assert S.encode(x, 0.01, n_bands=2, buf_size=size - 10)[0] == O.encode(x, 0.01, n_bands=2, buf_size=size - 10)[0] == 3


def test_sim_lerc1_world(libs):
    """the reference's Lerc1 fixture (testData/world.lerc1, 257 x 257 float, RLE mask, 33 x 33 tiles): info, ranges, pixels
    as float / double / int16, the mask, the refusal when the caller takes no mask, damaged copies"""
    import ctypes as ct
    O, S = libs
    blob = open(os.path.join(capi.ROOT, "tests", "golden", "world.lerc1"), "rb").read()
    assert O.blob_info(blob) == S.blob_info(blob) == (0, [0, 6, 1, 257, 257, 1, 65025, 63518, 1, 1, 0], [-27.458635330200195, 5474.1728515625, 0.1])
    assert O.data_ranges(blob, 1, 1) == S.data_ranges(blob, 1, 1)
    d1, d2 = O.decode(blob), S.decode(blob)
    assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1]) and _same(d1[2], d2[2])    # (pixels that are not valid keep the harness's fill)
    d1, d2 = O.decode(blob, to_double=True), S.decode(blob, to_double=True)
    assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1])
    b = np.frombuffer(blob, np.uint8)
    outs = []
    for L in (O, S):
        out, m = np.full((257, 257), -7, np.int16), np.zeros((257, 257), np.uint8)
        assert L.lib.lerc_decode(b.ctypes.data, len(blob), 1, m.ctypes.data, 1, 257, 257, 1, 2, out.ctypes.data) == 0
        assert L.lib.lerc_decode(b.ctypes.data, len(blob), 0, None, 1, 257, 257, 1, 2, out.ctypes.data) == 1    # has a mask: the caller must take it
        outs.append((out, m))
    assert _same(outs[0][0], outs[1][0]) and _same(outs[0][1], outs[1][1]) and int(outs[1][1].sum()) == 65025
    rng = np.random.default_rng(3)
    for t in range(40):
        x = bytearray(blob)
        k = int(rng.integers(0, len(x)))
        x[k] ^= 1 << int(rng.integers(0, 8))
        if t % 4 == 0:
            x = x[:max(40, k)]
        x = bytes(x)
        g1, g2 = O.decode(x), S.decode(x)    # Lerc1 has no checksum: a flipped payload bit decodes to other pixels in both
        assert (g1[0] == 0) == (g2[0] == 0), (t, k)
        if g1[0] == 0:
            assert _same(g1[1], g2[1]) and _same(g1[2], g2[2]), (t, k)


def test_sim_lerc1_written_blobs(libs):
    """Lerc1 blobs of tests/lerc1_writer.py (masks, remainder tiles, raw / constant / zero / bit-stuffed tiles, int8 / int16 /
    float offsets, several bands): info, ranges, pixels, masks as the oracle's; damaged copies: the oracle's verdict"""
    O, S = libs
    rng = np.random.default_rng(4)
    for name, blob, nb in cases.lerc1_cases():
        cases.check_lerc1_case(O, S, name, blob, nb, _same)
        for t in range(6):
            x = bytearray(blob)
            k = int(rng.integers(0, len(x)))
            x[k] ^= 1 << int(rng.integers(0, 8))
            x = bytes(x[:max(40, k)] if t % 3 == 0 else x)
            g1, g2 = O.decode(x), S.decode(x)
            assert (g1[0] == 0) == (g2[0] == 0), (name, t, k)
            if g1[0] == 0:
                assert _same(g1[1], g2[1]) and _same(g1[2], g2[2]), (name, t, k)


def test_sim_large_mask_helper_thread(libs):
    """A single-band raster whose validity bits make 256 KB and more: the mask's RLE is coded by a helper thread while the
    calling thread launches kernels (codec_encode.cpp: sendBitsHome) -- same blob as the oracle's, and it decodes"""
    O, S = libs
    rng = np.random.default_rng(1)
    r, c = 1460, 1448
    x = cases._cast(cases.terrain(r, c, rng, amp=40, base=100, sigma=1.0), np.uint8)
    m = (rng.random((r, c)) > 0.1).astype(np.uint8)
    m[100:300, 200:900] = 0
    r1, b1 = O.encode(x, 1.0, mask=m)
    r2, b2 = S.encode(x, 1.0, mask=m)
    assert r1 == r2 == 0 and bytes(b1) == bytes(b2)
    d1, d2 = O.decode(b1), S.decode(b1)
    assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1]) and _same(d1[2], d2[2])


def test_sim_poisoned_scratch():
    """The damaged-blob cases once more in a process whose scratch memory is filled with 0xFF before every call
    (LERC_AMD_POISON, codec_common.cpp): a kernel that trusts what nobody wrote -- the block offsets a refused walk
    leaves unwritten, say -- meets 0xFFFFFFFF here instead of the zeros of a fresh allocation.  (On the GPU such a read
    once made a staging loop run away for minutes; the emulator, whose scratch starts zeroed, had not shown it.)"""
    import subprocess
    import sys
    env = dict(os.environ, LERC_AMD_POISON="0xFF")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "damaged or lerc1_world"], env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_sim_mask_bytes_of_an_all_valid_band(libs):
    """nMasks >= 1 on a blob without a mask: 1s everywhere, on the streaming path too (the harness pre-fills 0xCD)."""
    O, S = libs
    rng = np.random.default_rng(41)
    for shape, n_bands in (((16, 1024), 1), ((2, 16, 520), 2), ((33, 47), 1)):
        arr = cases.terrain(*shape[-2:], rng).astype(np.float32)
        if n_bands > 1:
            arr = np.stack([arr + i for i in range(n_bands)])
        rc, blob = O.encode(arr, 0.01, n_bands=n_bands)
        assert rc == 0
        for want in (1, n_bands):
            rc, dec, mask = S.decode(blob, want_masks=want, n_bands=n_bands)
            assert rc == 0 and mask is not None and (mask == 1).all(), (shape, want)
            assert _same(dec, O.decode(blob)[1])


def _async_lib(S):
    import ctypes as ct
    L = S.lib
    L.lerc_amd_create.restype = ct.c_void_p
    L.lerc_amd_create.argtypes = [ct.c_void_p]
    L.lerc_amd_destroy.argtypes = [ct.c_void_p]
    enc = [ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p, ct.c_double]
    L.lerc_amd_encode_device_async.restype = ct.c_uint
    L.lerc_amd_encode_device_async.argtypes = [ct.c_void_p] + enc + [ct.c_void_p, ct.c_uint, ct.POINTER(ct.c_uint)]
    L.lerc_amd_decode_device_async.restype = ct.c_uint
    L.lerc_amd_decode_device_async.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_int,
                                               ct.c_uint, ct.c_void_p, ct.POINTER(ct.c_uint)]
    L.lerc_amd_finish.restype = ct.c_uint
    L.lerc_amd_finish.argtypes = [ct.c_void_p, ct.c_uint, ct.POINTER(ct.c_uint)]
    return L


def test_sim_async_device_api(libs):
    """lerc_amd_encode_device_async / decode_device_async / finish: operations queue up in order; a decode enqueued right
    behind the encode that writes its blob gets the buffer's capacity as size bound; what the device hands back to the
    general path (a constant raster) is repeated at finish time, and so is whatever was enqueued behind it."""
    import ctypes as ct
    O, S = libs
    L = _async_lib(S)
    h = L.lerc_amd_create(None)
    assert h
    rng = np.random.default_rng(8)
    try:
        rasters = [cases.terrain(32, 1024, rng, amp=300, base=1000, sigma=1.5).astype(np.float32),
                   np.full((16, 512), 3.5, np.float32),                                  # constant: the device says "redo"
                   cases._cast(cases.terrain(24, 200, rng, amp=300, base=1000, sigma=1.5), np.uint16),
                   cases.terrain(33, 47, rng).astype(np.float32)]                        # no whole blocks: never a streaming request
        errs = [0.01, 0.01, 0, 0.01]
        keep, tickets = [], []
        for arr, e in zip(rasters, errs):
            src = _aligned(arr.nbytes).view(arr.dtype).reshape(arr.shape)
            src[...] = arr
            blob = _aligned(arr.nbytes + 4096)
            out = _aligned(arr.nbytes).view(arr.dtype).reshape(arr.shape)
            t1, t2 = ct.c_uint(0), ct.c_uint(0)
            rc = L.lerc_amd_encode_device_async(h, src.ctypes.data, capi.dt_code(arr.dtype), 1, arr.shape[1], arr.shape[0], 1, 0, None, float(e),
                                                blob.ctypes.data, blob.size, ct.byref(t1))
            assert rc == 0 and t1.value
            rc = L.lerc_amd_decode_device_async(h, blob.ctypes.data, blob.size, 0, None, 1, arr.shape[1], arr.shape[0], 1, capi.dt_code(arr.dtype),
                                                out.ctypes.data, ct.byref(t2))
            assert rc == 0 and t2.value
            keep.append((src, blob, out))
            tickets.append((t1.value, t2.value))
        for (arr, e, (src, blob, out), (t1, t2)) in zip(rasters, errs, keep, tickets):
            n = ct.c_uint(0)
            assert L.lerc_amd_finish(h, t1, ct.byref(n)) == 0
            r0, b0 = O.encode(arr, e)
            assert r0 == 0 and blob[:n.value].tobytes() == b0
            assert L.lerc_amd_finish(h, t2, ct.byref(n)) == 0
            assert _same(O.decode(b0)[1].reshape(arr.shape), out)
        assert L.lerc_amd_finish(h, tickets[0][0], None) == 2                            # handed out already
        # more operations than result slots: the oldest are completed and dropped, the newest still answer
        arr = rasters[0]
        src, blob, out = keep[0]
        last = ct.c_uint(0)
        for _ in range(80):
            assert L.lerc_amd_encode_device_async(h, src.ctypes.data, 6, 1, arr.shape[1], arr.shape[0], 1, 0, None, 0.01, blob.ctypes.data, blob.size,
                                                  ct.byref(last)) == 0
        n = ct.c_uint(0)
        assert L.lerc_amd_finish(h, last.value, ct.byref(n)) == 0 and blob[:n.value].tobytes() == O.encode(arr, 0.01)[1]
        assert L.lerc_amd_finish(h, 0, None) == 0
    finally:
        L.lerc_amd_destroy(h)


def test_sim_decode_given_a_buffer_full_of_stale_bytes_behind_the_blob(libs):
    """A queued decode is given the buffer's capacity as its size bound, and what lies behind the blob there is whatever the buffer
    held before -- here the worst for the scanning decoder: nothing but bytes that read like block headers (0x8C 0x40 over and over).
    They must not count (they once filled the queue of the blob's last piece: every queued decode went down a tier, silently);
    the scanning decoder serves the call."""
    import ctypes as ct
    O, S = libs
    L = _async_lib(S)
    h = L.lerc_amd_create(None)
    assert h
    L.lerc_amd_decode_forms.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    rng = np.random.default_rng(18)
    try:
        for arr, e in ((cases.terrain(64, 1024, rng, amp=300, base=1000, sigma=1.5).astype(np.float32), 0.01),
                       (cases._cast(cases.terrain(40, 328, rng, amp=300, base=1000, sigma=1.5), np.uint16), 0)):
            r0, b0 = O.encode(arr, e)
            assert r0 == 0
            blob = _aligned(len(b0) + 70000)
            blob[:] = np.tile(np.array([0x8C, 0x40], np.uint8), blob.size // 2 + 1)[:blob.size]
            blob[:len(b0)] = np.frombuffer(b0, np.uint8)
            out = _aligned(arr.nbytes).view(arr.dtype).reshape(arr.shape)
            f0 = (ct.c_ulonglong * 4)(); f1 = (ct.c_ulonglong * 4)()
            L.lerc_amd_decode_forms(h, f0)
            t2 = ct.c_uint(0)
            rc = L.lerc_amd_decode_device_async(h, blob.ctypes.data, blob.size, 0, None, 1, arr.shape[1], arr.shape[0], 1, capi.dt_code(arr.dtype),
                                                out.ctypes.data, ct.byref(t2))
            assert rc == 0 and t2.value
            assert L.lerc_amd_finish(h, t2.value, None) == 0
            assert _same(O.decode(b0)[1].reshape(arr.shape), out)
            L.lerc_amd_decode_forms(h, f1)
            assert f1[3] == f0[3] + 1, ("the scanning decoder did not serve the call", list(f0), list(f1))
    finally:
        L.lerc_amd_destroy(h)


def test_sim_queued_decode_whose_launch_was_sized_by_a_smaller_band(libs):
    """A queued decode is given a capacity, and the scanning decoder's launch is sized by what the context's last band of that shape
    had (+ an eighth, + 64 KiB) instead of by the capacity.  A band that turns out LARGER than that finds too few workgroups: it says so
    (flag 2, nothing decoded), the host forgets the guess and the scanning decoder's other form serves the call with a launch sized by
    the capacity: one launch thrown away, counted -- and nothing keeps the bands behind it off the first form (no early count was
    wrong, no stream was refused): the same large band once more costs no second launch, its launch sized by the large one."""
    import ctypes as ct
    O, S = libs
    L = _async_lib(S)
    h = L.lerc_amd_create(None)
    assert h
    L.lerc_amd_decode_forms.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    L.lerc_amd_decode_refusals.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    rng = np.random.default_rng(31)
    try:
        smooth = cases.terrain(256, 1024, rng, amp=300, base=1000, sigma=0.01).astype(np.float32)
        noisy = (cases.terrain(256, 1024, rng, amp=300, base=1000, sigma=1.5) + rng.normal(0, 40, (256, 1024))).astype(np.float32)
        forms = []
        for arr, e in ((smooth, 0.05), (noisy, 0.0005), (noisy, 0.0005), (smooth, 0.05)):
            r0, b0 = O.encode(arr, e)
            assert r0 == 0
            blob = _aligned(arr.nbytes + 4096)
            blob[:] = 0
            blob[:len(b0)] = np.frombuffer(b0, np.uint8)
            out = _aligned(arr.nbytes).view(arr.dtype).reshape(arr.shape)
            f0 = (ct.c_ulonglong * 4)(); f1 = (ct.c_ulonglong * 4)(); r0_ = (ct.c_ulonglong * 4)(); r1_ = (ct.c_ulonglong * 4)()
            L.lerc_amd_decode_forms(h, f0)
            L.lerc_amd_decode_refusals(h, r0_)
            t2 = ct.c_uint(0)
            rc = L.lerc_amd_decode_device_async(h, blob.ctypes.data, blob.size, 0, None, 1, arr.shape[1], arr.shape[0], 1, capi.dt_code(arr.dtype),
                                                out.ctypes.data, ct.byref(t2))
            assert rc == 0 and t2.value
            assert L.lerc_amd_finish(h, t2.value, None) == 0
            assert _same(O.decode(b0)[1].reshape(arr.shape), out)
            L.lerc_amd_decode_forms(h, f1)
            L.lerc_amd_decode_refusals(h, r1_)
            forms.append(([int(f1[k] - f0[k]) for k in range(4)], len(b0), int(r1_[2] - r0_[2])))
        sizes = [f[1] for f in forms]
        assert sizes[1] > sizes[0] + sizes[0] // 8 + 65536 + 4096, sizes           # (else the test shows nothing)
        assert [f[0] for f in forms] == [[0, 0, 0, 1]] * 4, forms                  # the scanning decoder every time ...
        assert [f[2] for f in forms] == [0, 1, 0, 0], forms                        # ... and one launch thrown away, for the larger band
    finally:
        L.lerc_amd_destroy(h)


def test_sim_queued_verdicts_are_judged_against_their_own_launch(libs):
    """Two queued decodes in flight: a large band of a ragged shape whose launch was sized by a smaller band of that shape (too few
    pieces: it says so), and behind it a band of ANOTHER shape whose launch is larger than either.  The first verdict is judged
    against what its own launch held, not against the launch enqueued last: the guess is forgotten (one launch thrown away, counted),
    and the shape is NOT taken for one the scanning decoder cannot follow -- the same large band once more is served by the scanning
    decoder.  (Judged against the last launch, the band read as "a stream the scan does not follow" and its shape kept off the
    scanning decoder for 16 calls.)"""
    import ctypes as ct
    O, S = libs
    L = _async_lib(S)
    h = L.lerc_amd_create(None)
    assert h
    L.lerc_amd_decode_forms.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    L.lerc_amd_decode_refusals.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]

    def counters():
        f = (ct.c_ulonglong * 4)(); q = (ct.c_ulonglong * 4)()
        L.lerc_amd_decode_forms(h, f); L.lerc_amd_decode_refusals(h, q)
        return list(f), list(q)

    keep = []

    def queue(arr, b0, bound=None):
        blob = _aligned(arr.nbytes + 4096)
        blob[:] = 0
        blob[:len(b0)] = np.frombuffer(b0, np.uint8)
        out = _aligned(arr.nbytes).view(arr.dtype).reshape(arr.shape)
        t = ct.c_uint(0)
        rc = L.lerc_amd_decode_device_async(h, blob.ctypes.data, bound or blob.size, 0, None, 1, arr.shape[1], arr.shape[0], 1, capi.dt_code(arr.dtype),
                                            out.ctypes.data, ct.byref(t))
        assert rc == 0 and t.value
        keep.append((blob, out))
        return t.value, out

    try:
        (smooth, bs), (noisy, bn), (other, bo) = cases.queued_bands_of_two_shapes(O)
        t1, o1 = queue(smooth, bs)
        assert L.lerc_amd_finish(h, t1, None) == 0                       # the size guess for the shape is now small
        f0, q0 = counters()
        t2, o2 = queue(noisy, bn)                                         # sized by the small guess: too few pieces
        t3, o3 = queue(other, bo, len(bo))                                # another shape, a larger launch: in flight behind it
        assert L.lerc_amd_finish(h, t2, None) == 0 and L.lerc_amd_finish(h, t3, None) == 0
        f1, q1 = counters()
        for arr, b0, out in ((smooth, bs, o1), (noisy, bn, o2), (other, bo, o3)):
            assert _same(O.decode(b0)[1].reshape(arr.shape), out), arr.shape
        assert q1[2] == q0[2] + 1, (q0, q1)
        t4, o4 = queue(noisy, bn)
        assert L.lerc_amd_finish(h, t4, None) == 0
        f2, q2 = counters()
        assert _same(O.decode(bn)[1].reshape(noisy.shape), o4)
        assert f2[3] == f1[3] + 1 and f2[2] == f1[2] and q2 == q1, ("the scanning decoder did not serve the shape", f1, f2, q1, q2)
    finally:
        L.lerc_amd_destroy(h)


def test_sim_early_counts_that_the_mending_changes(libs):
    """The scanning decoder's pieces say how many blocks they hold as soon as the survivors are counted (form 4, EARLY).  A raster with
    flat stretches has constant blocks, which the scan does not see and the mending enters: the piece's count changes after it has
    left -- the piece says so, the band is decoded once more by the late form (one launch thrown away, counted), and the next bands
    of the context start with the late form: no more launches thrown away.  Noise keeps to the early form."""
    import ctypes as ct
    O, S = libs
    L = _async_lib(S)
    h = L.lerc_amd_create(None)
    assert h
    L.lerc_amd_decode_forms.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    L.lerc_amd_decode_refusals.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    L.lerc_amd_decode_device.restype = ct.c_uint
    L.lerc_amd_decode_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_uint, ct.c_void_p]
    rng = np.random.default_rng(41)
    try:
        noise = cases.terrain(128, 1024, rng, amp=300, base=1000, sigma=1.5).astype(np.float32)
        flat = noise.copy()
        flat[40:72, 200:264] = 1234.5          # 4 x 8 blocks of one value
        flat[96:104, 512:520] = 777.25
        seen = []
        for arr in (noise, flat, flat, flat, noise):
            r0, b0 = O.encode(arr, 0.01)
            assert r0 == 0
            blob = _aligned(len(b0) + 4096)
            blob[:] = 0
            blob[:len(b0)] = np.frombuffer(b0, np.uint8)
            out = _aligned(arr.nbytes).view(arr.dtype).reshape(arr.shape)
            f0 = (ct.c_ulonglong * 4)(); f1 = (ct.c_ulonglong * 4)(); q0 = (ct.c_ulonglong * 4)(); q1 = (ct.c_ulonglong * 4)()
            L.lerc_amd_decode_forms(h, f0)
            L.lerc_amd_decode_refusals(h, q0)
            rc = L.lerc_amd_decode_device(h, blob.ctypes.data, len(b0), 0, None, 1, arr.shape[1], arr.shape[0], 1, capi.dt_code(arr.dtype), out.ctypes.data)
            assert rc == 0
            assert _same(O.decode(b0)[1].reshape(arr.shape), out)
            L.lerc_amd_decode_forms(h, f1)
            L.lerc_amd_decode_refusals(h, q1)
            seen.append(([int(f1[k] - f0[k]) for k in range(4)], int(q1[2] - q0[2])))
        assert [f for f, _ in seen] == [[0, 0, 0, 1]] * 5, seen          # the scanning decoder every time
        assert [q for _, q in seen] == [0, 1, 0, 0, 0], seen             # the early count was wrong once; the context counts late from there on
    finally:
        L.lerc_amd_destroy(h)


def test_sim_flat_stretches_stay_on_the_scanning_decoder(libs):
    """Rasters with flat stretches -- a lake, the sea, a fill value: runs of constant (2 ... 5 bytes) and all-zero (1 byte) blocks, hundreds
    on end, which the scan does not see -- are the scanning decoder's: the piece's first wave walks a gap run by run, 64 blocks a step,
    and a piece that begins inside a run (no anchor in the bytes in front of it) takes its first block's place from the piece in
    front.  Runs longer than a piece's staged bytes in front, runs that end with the raster's block row, several values (= block lengths),
    the stream's first and last blocks inside a run; 16- and 32-bit integers as well.  One launch is thrown away for the first such band
    of a context (the early count is wrong: the late form mends), none after that."""
    import ctypes as ct
    O, S = libs
    L = _async_lib(S)
    L.lerc_amd_decode_forms.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    L.lerc_amd_decode_refusals.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    L.lerc_amd_decode_device.restype = ct.c_uint
    L.lerc_amd_decode_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_uint, ct.c_void_p]
    rng = np.random.default_rng(43)

    def flats(dt, e):
        x = cases.terrain(96, 2048, rng, amp=300, base=1000, sigma=1.5)
        out = []
        a = x.copy(); a[16:48, 256:1280] = 1017.25; a[64:72, 1536:2048] = 0.0; a[72:80, 0:512] = 1500.0          # 5-byte, 1-byte and short blocks; a run up to the row's end, one from its start
        out.append(a)
        b = x.copy(); b[0:24, 0:1024] = 733.5; b[88:96, 1024:2048] = 12.0                                      # the stream's first and last blocks lie in runs
        out.append(b)
        c = x.copy(); c[8:88, 64:1984] = 250.0                                                                 # mostly flat: runs of 240 blocks, a few noise blocks between
        out.append(c)
        d = x.copy(); d[40:48, :] = 900.0; d[48:56, :] = 0.0                                                   # whole block rows flat: 256 + 256 blocks on end, two values
        out.append(d)
        return [(cases._cast(v, dt), e) for v in out]

    for dt, e in ((np.float32, 0.01), (np.uint16, 0), (np.int32, 0)):
        h = L.lerc_amd_create(None)
        assert h
        try:
            seen = []
            for arr, err in flats(dt, e):
                r0, b0 = O.encode(arr, err)
                assert r0 == 0
                blob = _aligned(len(b0) + 4096)
                blob[:] = 0
                blob[:len(b0)] = np.frombuffer(b0, np.uint8)
                out = _aligned(arr.nbytes).view(arr.dtype).reshape(arr.shape)
                f0 = (ct.c_ulonglong * 4)(); f1 = (ct.c_ulonglong * 4)(); q0 = (ct.c_ulonglong * 4)(); q1 = (ct.c_ulonglong * 4)()
                L.lerc_amd_decode_forms(h, f0)
                L.lerc_amd_decode_refusals(h, q0)
                rc = L.lerc_amd_decode_device(h, blob.ctypes.data, len(b0), 0, None, 1, arr.shape[1], arr.shape[0], 1, capi.dt_code(arr.dtype), out.ctypes.data)
                assert rc == 0
                assert _same(O.decode(b0)[1].reshape(arr.shape), out), (dt, len(seen))
                L.lerc_amd_decode_forms(h, f1)
                L.lerc_amd_decode_refusals(h, q1)
                seen.append(([int(f1[k] - f0[k]) for k in range(4)], int(q1[2] - q0[2])))
            assert [f for f, _ in seen] == [[0, 0, 0, 1]] * 4, (dt, seen)      # the scanning decoder every time
            assert [q for _, q in seen] == [1, 0, 0, 0], (dt, seen)            # the early count was wrong once
        finally:
            L.lerc_amd_destroy(h)


def test_sim_mask_and_statistics_in_one_read(libs):
    """A band with a byte mask (one value a pixel, 16- / 32-bit types, whole words of the bit mask): k_mask_stats makes the bit mask, the
    count of valid pixels and the band's statistics in ONE read of the band (misc_kernels.hip) where no TryRaiseMaxZError candidate
    survives the first row -- the profile names the kernel, the blob is the oracle's.  NaNs under the mask and outside it, rasters
    of whole numbers (the all-integer promotion), candidates that survive (then launchBandStats runs as before)."""
    import ctypes as ct
    O, S = libs
    L = _async_lib(S)
    enc = [ct.c_void_p, ct.c_uint, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_void_p, ct.c_double]
    L.lerc_amd_encode_device.restype = ct.c_uint
    L.lerc_amd_encode_device.argtypes = [ct.c_void_p] + enc + [ct.c_void_p, ct.c_uint, ct.POINTER(ct.c_uint)]
    L.lerc_amd_profile_enable.argtypes = [ct.c_void_p, ct.c_int]
    L.lerc_amd_profile_read.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int]
    rng = np.random.default_rng(51)
    h = L.lerc_amd_create(None)
    assert h
    try:
        cases_ = []
        for dt, e in ((np.float32, 0.01), (np.uint16, 0), (np.int32, 0), (np.int16, 1), (np.uint32, 2)):
            for (r, c) in ((64, 128), (40, 104), (128, 256)):
                x = cases._cast(cases.terrain(r, c, rng, amp=300, base=1000, sigma=2.0), dt)
                m = (rng.random((r, c)) > 0.2).astype(np.uint8)
                m[:8, :16] = 0
                if dt == np.float32:
                    x[5, 7] = np.nan; x[20, 33] = np.nan; x[2, 3] = np.nan      # (under the mask, and not)
                cases_.append((x, m, e, True))
        whole = np.floor(cases.terrain(64, 128, rng, amp=300, base=1000, sigma=2.0)).astype(np.float32)
        cases_.append((whole, (rng.random((64, 128)) > 0.3).astype(np.uint8), 0.5, True))       # all integers
        tenths = (np.round(cases.terrain(64, 128, rng, amp=30, base=100, sigma=2.0) * 10) / 10).astype(np.float32)
        cases_.append((tenths, (rng.random((64, 128)) > 0.3).astype(np.uint8), 0.001, False))   # a candidate may survive the first row: the statistics' own kernel
        for x, m, e, fused in cases_:
            src = _aligned(x.nbytes).view(x.dtype).reshape(x.shape); src[...] = x
            msk = _aligned(m.nbytes).reshape(m.shape); msk[...] = m
            blob = _aligned(x.nbytes + 65536)
            n = ct.c_uint(0)
            L.lerc_amd_profile_enable(h, 1)
            rc = L.lerc_amd_encode_device(h, src.ctypes.data, capi.dt_code(x.dtype), 1, x.shape[1], x.shape[0], 1, 1, msk.ctypes.data, float(e),
                                          blob.ctypes.data, blob.size, ct.byref(n))
            L.lerc_amd_profile_enable(h, 0)
            buf = ct.create_string_buffer(1 << 16)
            L.lerc_amd_profile_read(h, buf, len(buf), 1)
            names = [ln.split()[0] for ln in buf.value.decode().splitlines()]
            r0, b0 = O.encode(x, e, mask=m)
            assert rc == r0 == 0 and blob[:n.value].tobytes() == bytes(b0), (x.dtype, x.shape, e)
            if fused:
                assert "mask_stats" in names and "build_mask" not in names and "band_stats" not in names, (x.dtype, x.shape, names)
            else:
                assert "mask_stats" in names, names
    finally:
        L.lerc_amd_destroy(h)


def test_sim_ragged_rasters_on_the_scanning_decoder(libs):
    """Rasters whose rows / columns are no multiples of 8 (the reference's own benchmark rasters: 4600 x 4300, 3612^2, 1201^2 ...): the scanning
    decoder's RAG instantiation -- the filter also takes the count byte of the last block row's blocks (8 x rows mod 8), the one edge block a
    block row comes in through the mending, a block's size is checked against its place, partial rows are stored pixel by pixel.  Pixels
    = the oracle's, every band served by the scanning decoder; flat stretches and look-up tables
    at the edges; all types."""
    import ctypes as ct
    O, S = libs
    L = _async_lib(S)
    L.lerc_amd_decode_forms.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    L.lerc_amd_decode_refusals.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    L.lerc_amd_decode_device.restype = ct.c_uint
    L.lerc_amd_decode_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_uint, ct.c_void_p]
    rng = np.random.default_rng(61)
    h = L.lerc_amd_create(None)
    assert h
    try:
        n_scan = n_thrown = 0
        for dt, e, (r, c) in ((np.float32, 0.01, (257, 257)), (np.float32, 0.01, (100, 1027)), (np.uint16, 0, (129, 2050)), (np.int32, 0, (64, 1001)),
                              (np.float32, 0.01, (203, 1024)), (np.float64, 0.001, (75, 515)), (np.int16, 1, (333, 517)), (np.uint32, 2, (90, 999)),
                              (np.float32, 0.01, (1001, 131)), (np.uint16, 0, (8, 4099)), (np.float32, 0.1, (15, 3000))):
            x = cases.terrain(r, c, rng, amp=300, base=1000, sigma=1.5)
            if r > 64:
                x[40:56, c - 40:] = 123.0          # flat up to the edge column
                x[r - 12:, 16:200] = 77.0          # and in the last block row
            x[:, 200:232] = np.floor(x[:, 200:232] / 32) * 32       # few distinct values: look-up tables
            x = cases._cast(x, dt)
            r0, b0 = O.encode(x, e)
            assert r0 == 0
            blob = _aligned(len(b0) + 4096)
            blob[:] = 0
            blob[:len(b0)] = np.frombuffer(b0, np.uint8)
            out = _aligned(x.nbytes).view(x.dtype).reshape(x.shape)
            f0 = (ct.c_ulonglong * 4)(); f1 = (ct.c_ulonglong * 4)(); q0 = (ct.c_ulonglong * 4)(); q1 = (ct.c_ulonglong * 4)()
            L.lerc_amd_decode_forms(h, f0); L.lerc_amd_decode_refusals(h, q0)
            rc = L.lerc_amd_decode_device(h, blob.ctypes.data, len(b0), 0, None, 1, c, r, 1, capi.dt_code(x.dtype), out.ctypes.data)
            assert rc == 0
            assert _same(O.decode(b0)[1].reshape(x.shape), out), (np.dtype(dt).name, r, c)
            L.lerc_amd_decode_forms(h, f1); L.lerc_amd_decode_refusals(h, q1)
            served = int(f1[3] - f0[3]) == 1
            n_scan += served
            n_thrown += int(q1[2] - q0[2])
            assert served or r < 16, (np.dtype(dt).name, r, c, [int(f1[k] - f0[k]) for k in range(4)], int(q1[2] - q0[2]))
        # (an edge block that is constant or raw is found by the mending: the piece's early count was wrong, once -- the context counts late from there on)
        assert n_scan >= 9 and n_thrown <= 2, (n_scan, n_thrown)
    finally:
        L.lerc_amd_destroy(h)


def test_sim_masked_bands_are_cut_into_blocks_by_the_scan(libs):
    """A band with a mask (8 x 8 blocks, one value a pixel, 16-bit and wider types): the scanning decoder's first half finds the block
    offsets (tile_fast_decode_scan.hip, MODE 1 -- count bytes of 1 ... 64, one-byte blocks of pixels that are all invalid walked by the
    mending, the blocks behind a piece's end up to the next bit-stuffed pair handed to the piece in front), the general kernels decode
    the pixels.  lerc_amd_decode_forms()[0] counts such bands; damaged copies get the oracle's verdict (the scan hands what it cannot
    follow to the general discovery)."""
    O, S = libs
    rng = np.random.default_rng(25)
    served = 0
    for it, (r, c, dt, e) in enumerate(((256, 400, np.float32, 0.01), (200, 264, np.uint16, 0), (512, 1024, np.float32, 0.01), (300, 300, np.int32, 0),
                                        (128, 2048, np.float64, 0.001), (333, 517, np.float32, 0.1), (96, 4096, np.int16, 1))):
        x = cases._cast(cases.terrain(r, c, rng, amp=300, base=1000, sigma=2.0), dt)
        m = np.ones((r, c), np.uint8)
        if it % 3 == 0:
            for _ in range(8):
                i0, j0 = int(rng.integers(0, r)), int(rng.integers(0, c))
                m[i0:i0 + int(rng.integers(1, 60)), j0:j0 + int(rng.integers(1, 200))] = 0
        elif it % 3 == 1:
            m = (rng.random((r, c)) > 0.3).astype(np.uint8)
        else:
            m[((np.arange(r)[:, None] // 97) + (np.arange(c)[None, :] // 131)) % 10 == 0] = 0
        rc, blob = O.encode(x, e, mask=m)
        assert rc == 0
        f0 = S.decode_forms()
        d1, d2 = O.decode(blob), S.decode(blob)
        f1 = S.decode_forms()
        v = d1[2].reshape(r, c) != 0
        assert d1[0] == d2[0] == 0 and np.array_equal(d1[2], d2[2]) and np.array_equal(d1[1].reshape(r, c)[v], d2[1].reshape(r, c)[v]), (it, r, c)
        served += f1[0] - f0[0]
        for t in range(6):
            bad = bytearray(blob)
            k = int(rng.integers(100, len(bad)))
            bad[k] ^= 1 << int(rng.integers(0, 8))
            g1, g2 = O.decode(bytes(bad)), S.decode(bytes(bad))
            assert (g1[0] == 0) == (g2[0] == 0), (it, t, k, g1[0], g2[0])
    assert served == 7, ("the scan did not serve every masked band", served, S.last_note())


def test_sim_masked_bands_with_runs_and_raw_blocks(libs):
    """What a mask's shape does to a band's block stream, and the scan (MODE 1) has to follow: RUNS of one-byte blocks (blocks without
    a valid pixel) -- found by the flood from the survivors' ends, also where a run is longer than the bytes a piece stages in front of
    its own (the run's first byte there is taken for a block; the piece in front confirms it) or crosses block rows; RAW blocks of one or
    two valid pixels at curved and slanted edges, whose length only the mask knows (the mending tries the counts and wants the blocks
    behind to parse up to a known one, the column signature going on in pairs); a raw block, the run to the next block row's edge, its
    raw block.  Every band here is served by the scan, pixels and masks as the oracle has them."""
    O, S = libs
    rng = np.random.default_rng(7)
    def ellipse(r, c):
        ii, jj = np.mgrid[0:r, 0:c]
        return ((ii - r / 2) ** 2 / (0.45 * r) ** 2 + (jj - c / 2) ** 2 / (0.44 * c) ** 2 < 1).astype(np.uint8)
    def diagonal(r, c):
        ii, jj = np.mgrid[0:r, 0:c]
        return ((ii + jj) % 300 < 200).astype(np.uint8)
    def cols(r, c, j0, j1, rows=None):
        m = np.ones((r, c), np.uint8); m[:, j0:j1] = 0
        if rows: m[rows[0]:rows[1]] = rows[2]
        return m
    todo = (("a third of every row", 64, 4096, np.float32, 0.01, cols(64, 4096, 0, 1365)),
            ("the right half and the left quarter", 64, 4096, np.float32, 0.01, cols(64, 4096, 2048, 4096) & cols(64, 4096, 0, 1024)),
            ("block rows without a pixel", 160, 1024, np.float32, 0.01, cols(160, 1024, 0, 0, (40, 80, 0))),
            ("runs of 350", 32, 8192, np.uint16, 0, cols(32, 8192, 1000, 3800)),
            ("runs of 400, a block row without", 32, 8192, np.uint16, 0, cols(32, 8192, 3000, 6200, (8, 16, 1))),
            ("runs of 650: longer than what a piece stages in front", 32, 8192, np.float32, 0.01, cols(32, 8192, 500, 5700)),
            ("an ellipse", 200, 1600, np.float32, 0.01, ellipse(200, 1600)),
            ("an ellipse, 16 bit", 200, 1600, np.int16, 0, ellipse(200, 1600)),
            ("slanted bands", 200, 1600, np.float32, 0.01, diagonal(200, 1600)),
            ("slanted bands, 32 bit", 200, 1600, np.int32, 0, diagonal(200, 1600)))
    for name, r, c, dt, e, m in todo:
        x = cases._cast(cases.terrain(r, c, rng, amp=300, base=1000, sigma=2.0), dt)
        rc, blob = O.encode(x, e, mask=m)
        assert rc == 0
        f0 = S.decode_forms()
        d1, d2 = O.decode(blob), S.decode(blob)
        f1 = S.decode_forms()
        v = d1[2].reshape(r, c) != 0
        assert d1[0] == d2[0] == 0 and np.array_equal(d1[2], d2[2]) and np.array_equal(d1[1].reshape(r, c)[v], d2[1].reshape(r, c)[v]), name
        assert f1[0] - f0[0] == 1, ("the scan did not serve the band", name, S.last_note())


def test_sim_workgroups_that_give_up_waiting(libs):
    """LERC_AMD_TEST_GIVEUP: every hand-off inside the one-launch encoder and the streaming decoder arrives with a tag nobody
    waits for; the waiters run into their poll limit, say so, and the host repeats the call on the general kernels --
    same bytes, same pixels (the knob is read once: a process of its own).  The GPU suite runs the same on hardware."""
    import subprocess
    import sys
    code = r"""
import sys, os
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, capi, cases
S, O = capi.sim(), capi.oracle()
rng = np.random.default_rng(5)
for dt, e, shape in ((np.float32, 0.01, (128, 1024)), (np.uint16, 0, (256, 512))):    # (blobs of several decoding workgroups)
    x = cases._cast(cases.terrain(shape[0], shape[1], rng, amp=300, base=1000, sigma=2.0), dt)
    c0 = S.path_counters()
    r1, b1 = O.encode(x, e)
    r2, b2 = S.encode(x, e)
    assert r1 == r2 == 0 and b1 == b2, "blob"
    d1, d2 = O.decode(b1), S.decode(b1)
    assert d1[0] == d2[0] == 0 and np.array_equal(d1[1].view(np.uint8), d2[1].view(np.uint8)), "pixels"
    c1 = S.path_counters()
    assert c1[1] > c0[1] and c1[3] > c0[3], (c0, c1)
print("gave up and recovered")
""" % (capi.ROOT,)
    env = dict(os.environ, LERC_AMD_TEST_GIVEUP="3")
    out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0 and b"gave up and recovered" in out.stdout, out.stdout.decode()[-2000:]


@pytest.mark.parametrize("launches,giveup", [("1", "0"), ("1", "2"), ("1", "4"), ("2", "0"), ("2", "2")])
def test_sim_streaming_decoder_in_one_launch_and_in_two(libs, launches, giveup):
    """The streaming decoder is ONE launch (k_fast_decode_one: a workgroup stages 16 chunks, finds their block starts and
    decodes them; what travels between workgroups is a block count per workgroup); LERC_AMD_DECODE_LAUNCHES=2 keeps the
    two-launch form (k_fast_discover + k_fast_decode).  Emulator builds have groups of 2 workgroups, so a blob of a few
    hundred KB takes the cells of its own group and the group totals in front.  Same pixels as the oracle, streaming path
    taken, damaged copies refused like the oracle refuses them; with the hand-offs made to fail (LERC_AMD_TEST_GIVEUP) every
    blob that needs one -- more than one workgroup -- comes back through the general kernels."""
    import subprocess
    import sys
    code = r"""
import sys, os
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, capi, cases
S, O = capi.sim(), capi.oracle()
giveup = os.environ.get("LERC_AMD_TEST_GIVEUP", "0") == "2"    # ("4": every chunk's path is walked a second time, the way a path that is not walk 0 is)
one = os.environ.get("LERC_AMD_DECODE_LAUNCHES") != "2"
rng = np.random.default_rng(12)
for dt, e, shape in ((np.float32, 0.01, (128, 1024)), (np.uint16, 0, (128, 512)), (np.float64, 0.001, (64, 256)), (np.int32, 0, (100, 70)),
                     (np.float32, 0.5, (257, 257)), (np.int16, 0, (8, 8)), (np.float32, 0.01, (256, 1024)), (np.uint16, 0, (512, 768)),
                     (np.int32, 0, (301, 777)), (np.float64, 0.0001, (200, 520))):
    for kind in ("terrain", "mixed"):
        x = cases._cast(cases.terrain(shape[0], shape[1], rng, amp=300, base=1000, sigma=2.0), dt) if kind == "terrain" else cases.mixed_regions(shape[0], shape[1], rng, dt)
        r1, b1 = O.encode(x, e)
        assert r1 == 0
        c0 = S.path_counters()
        d1, d2 = O.decode(b1), S.decode(b1)
        c1 = S.path_counters()
        assert d1[0] == d2[0] == 0 and np.array_equal(d1[1].view(np.uint8), d2[1].view(np.uint8)), ("pixels", shape, kind)
        several = len(b1) > 32768    # (one launch: a blob of one workgroup -- 32 KiB -- waits for nobody)
        if giveup and (several or not one): assert c1[3] > c0[3], (c0, c1, shape)
        if not giveup and kind == "terrain": assert c1[2] > c0[2] and c1[3] == c0[3], (c0, c1, shape, S.last_note())
        for t in range(3):
            y = bytearray(b1)
            k = int(rng.integers(0, len(y)))
            y[k] ^= 1 << int(rng.integers(0, 8))
            d1, d2 = O.decode(bytes(y)), S.decode(bytes(y))
            assert (d1[0] == 0) == (d2[0] == 0), ("status", shape, k)
            if d1[0] == 0:
                assert np.array_equal(d1[1].view(np.uint8), d2[1].view(np.uint8)), ("damaged", shape, k)
print("decoder ok")
""" % (capi.ROOT,)
    env = dict(os.environ, LERC_AMD_DECODE_LAUNCHES=launches, LERC_AMD_TEST_GIVEUP=giveup)
    out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    assert out.returncode == 0 and b"decoder ok" in out.stdout, out.stdout.decode()[-2000:]


def test_sim_ragged_rasters_take_the_streaming_kernels(libs):
    """Rows / columns that are no multiples of 8: the blocks of the last block row / column hold w x h < 64 elements
    (Lerc2.cpp:1504-1519).  The one-launch encoder and the streaming decoder take such rasters (path counters), bytes and
    pixels are the oracle's -- 257 x 257 elevation tiles included, whose one-pixel corner block is always a raw one."""
    O, S = libs
    rng = np.random.default_rng(31)
    for dt, e in ((np.float32, 0.01), (np.uint16, 0), (np.int32, 0), (np.float64, 0.001)):
        for shape in ((9, 9), (17, 23), (63, 65), (100, 70), (257, 257), (3, 700), (64, 1027)):
            for kind in ("terrain", "mixed"):
                x = cases._cast(cases.terrain(shape[0], shape[1], rng, amp=300, base=1000, sigma=2.0), dt) if kind == "terrain" else cases.mixed_regions(shape[0], shape[1], rng, dt)
                c0 = S.path_counters()
                r1, b1 = O.encode(x, e)
                r2, b2 = S.encode(x, e)
                assert r1 == r2 == 0 and b1 == b2, (np.dtype(dt).name, shape, kind)
                d1, d2 = O.decode(b1), S.decode(b1)
                assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1]), (np.dtype(dt).name, shape, kind)
                c1 = S.path_counters()
                if kind == "terrain":
                    assert c1[0] - c0[0] == 2 and c1[2] - c0[2] == 1, (np.dtype(dt).name, shape, c0, c1, S.last_note())    # size query + encode, decode
