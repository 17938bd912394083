"""GPU parity tests (`-m gpu`): the product library liblerc_amd.so, called through its C ABI, against
  * the committed golden vectors (tests/golden, produced by the real reference),
  * the CPU oracle (oracle/liblerc_oracle.so) on the same seeded inputs,
  * the real reference build (oracle/_ref/libLercRef.so) when it travelled to the GPU box,
plus size-independent properties at the full BASELINE sizes.  Bar: byte-identical blobs, bit-identical
decodes; float pixels within MaxZError (+ 1/2 ulp of the f32 result)."""
import ctypes as ct
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import capi
import cases

pytestmark = pytest.mark.gpu

GOLD = os.path.join(capi.ROOT, "tests", "golden")
VEC = json.load(open(os.path.join(GOLD, "ref_vectors.json")))


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.fixture(scope="module")
def P():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    lib = capi.product()
    assert lib is not None, "lerc_amd/csrc/liblerc_amd.so missing -- run __graft_entry__.build()"
    return lib


@pytest.fixture(scope="module")
def O():
    if capi.oracle() is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(capi.ROOT, "oracle")])
    return capi.oracle()


# device features that are not implemented yet are listed here explicitly (and in DESIGN.md)
def _unsupported(name):
    return False    # (the bit plane mode, maxZErr 777, used to be listed here)


_CASES = [c for c in cases.basic_cases() if not _unsupported(c[0])]


@pytest.mark.parametrize("idx", range(len(_CASES)), ids=[c[0] for c in _CASES])
def test_case_matrix_vs_golden_and_oracle(P, O, idx):
    name, arr, kw = _CASES[idx]
    v = VEC[name]
    kw = dict(kw)
    e = kw.pop("max_z_err")
    assert sha(np.ascontiguousarray(arr).tobytes()) == v["input_sha"]
    rc, size = P.compute_size(arr, e, **kw)
    assert (rc, size) == (v["rc_size"], v["size"])
    rc, blob = P.encode(arr, e, **kw)
    assert rc == v["rc"]
    if rc != 0:
        return
    assert len(blob) == v["size"]
    assert sha(blob) == v["blob_sha"], "blob differs from the reference's"
    rc, dec, mask = P.decode(blob)
    assert rc == 0 and sha(dec.tobytes()) == v["dec_sha"]
    assert (sha(mask.tobytes()) if mask is not None else None) == v["mask_sha"]
    assert P.blob_info(blob)[1:] == (v["info"], v["range"])
    # cross-check with the oracle on the same input, both directions
    r2, b2 = O.encode(arr, e, **kw)
    assert r2 == 0 and b2 == blob
    d2 = O.decode(blob)
    assert _same(d2[1], dec) and _same(d2[2], mask)


def test_decode_reference_blobs(P, O):
    names = ["california_400_400_1_float.lerc2", "js_sanity_v5.lerc2"]
    names += [os.path.join("blobs", f) for f in sorted(os.listdir(os.path.join(GOLD, "blobs")))]
    for f in names:
        blob = open(os.path.join(GOLD, f), "rb").read()
        d1, d2 = O.decode(blob), P.decode(blob)
        assert d1[0] == d2[0] == 0, f
        assert _same(d1[1], d2[1]) and _same(d1[2], d2[2]), f
    blob = open(os.path.join(GOLD, "california_400_400_1_float.lerc2"), "rb").read()
    rc, dec, mask = P.decode(blob)
    assert sha(dec.tobytes())[:16] == "61e4aa3ffeeccb06" and int(mask.sum()) == 58515


def test_bluemarble_three_bands(P, O):
    blob = open(os.path.join(GOLD, "bluemarble_256_256_3_byte.lerc2"), "rb").read()
    d1, d2 = O.decode(blob), P.decode(blob)
    assert d1[0] == d2[0] == 0
    assert _same(d1[1], d2[1]) and _same(d1[2], d2[2])


def test_to_double_and_partial_bands(P, O):
    rng = np.random.default_rng(3)
    bands = np.stack([cases.terrain(40, 50, rng, base=1000 + 100 * b) for b in range(3)]).astype(np.float32)
    rc, blob = P.encode(bands, 0.01, n_bands=3)
    assert rc == 0
    a, b = O.decode(blob, to_double=True), P.decode(blob, to_double=True)
    assert a[0] == b[0] == 0 and _same(a[1], b[1])
    a, b = O.decode(blob, n_bands=2), P.decode(blob, n_bands=2)
    assert a[0] == b[0] == 0 and _same(a[1], b[1])


def test_error_codes(P):
    a = np.zeros((4, 4), np.float32)
    assert P.encode(a, -1.0)[0] == 2
    rc, blob = P.encode(a + np.arange(4, dtype=np.float32), 0.01, buf_size=20)
    assert rc == 3 and blob == b""
    n = np.full((8, 8, 2), 1.0, np.float32)
    n[1, 1, 0] = np.nan
    assert P.encode(n, 0.01, n_depth=2)[0] == 4
    blob = bytearray(open(os.path.join(GOLD, "blobs", "mixed-float32.lerc2"), "rb").read())
    blob[len(blob) // 2] ^= 0x40
    assert P.decode(bytes(blob))[0] == 1
    assert P.decode(bytes(blob[:300]))[0] != 0


def test_against_real_reference_fuzz(P):
    R = capi.ref()
    if R is None:
        pytest.skip("oracle/_ref/libLercRef.so did not travel")
    rng = np.random.default_rng(99)
    for it in range(120):
        dt = cases.ALL_DTYPES[rng.integers(2, 8)]    # 8-bit types: covered by the Huffman tests
        r, c = int(rng.integers(1, 200)), int(rng.integers(1, 200))
        nd = int(rng.choice([1, 1, 1, 2, 3]))
        kind = np.dtype(dt).kind
        base = cases.terrain(r, c, rng, amp=float(rng.choice([5, 50, 500])), base=float(rng.choice([0, 100, 1000])),
                             sigma=float(rng.choice([0, 0.3, 3])))
        x = np.stack([base + k for k in range(nd)], axis=-1) if nd > 1 else base
        style = rng.integers(0, 3)
        if style == 1:
            x = np.floor(x / 16) * 16
        if style == 2:
            x = np.round(x, 1)
        x = cases._cast(x, dt)
        e = float(rng.choice([0.001, 0.01, 0.5, 1, 3])) if kind == "f" else float(rng.choice([0, 0, 1, 4]))
        kw = dict(n_depth=nd)
        if rng.random() < 0.3:
            kw["mask"] = (rng.random((r, c)) > rng.random() * 0.6).astype(np.uint8)
        tag = f"fuzz{it} {np.dtype(dt).name} {r}x{c}x{nd} e={e} style={style} mask={'mask' in kw}"
        assert R.compute_size(x, e, **kw) == P.compute_size(x, e, **kw), tag
        r1, b1 = R.encode(x, e, **kw)
        r2, b2 = P.encode(x, e, **kw)
        assert r1 == r2 and b1 == b2, tag
        if r1 == 0:
            d1, d2 = R.decode(b1), P.decode(b1)
            assert d1[0] == d2[0] and _same(d1[1], d2[1]) and _same(d1[2], d2[2]), tag


# ---- full BASELINE sizes, device-pointer API ------------------------------------------------------
def _device_roundtrip(x, max_z_err, streamed=False):
    """streamed: the call must have been served by the streaming kernels alone -- the one-launch encoder, the scanning decoder
    (a silent detour through the general kernels would keep every byte right and show on the bench only)"""
    import torch
    from lerc_amd import api
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)    # same stream as the tensor producers
    out = torch.empty(x.numel() * x.element_size() + (1 << 20), dtype=torch.uint8, device=x.device)
    y = torch.empty_like(x)
    rc, nb = api.encode_device(codec, x, max_z_err, out)
    assert rc == 0, (rc, codec.last_error())
    rc = api.decode_device(codec, out, nb, y)
    assert rc == 0, (rc, codec.last_error())
    torch.cuda.synchronize()
    if streamed:
        assert codec.path_counters() == [1, 0, 1, 0], (codec.path_counters(), codec.last_note())
        assert codec.decode_forms()[3] == 1, (codec.decode_forms(), codec.last_note())
    return out[:nb].cpu().numpy().tobytes(), y


def test_c2_full_size_8192_float32(P, O):
    """BASELINE configs[1]: byte identity with the CPU oracle at full size, error bound, reference decode."""
    import torch
    from lerc_amd import synth
    x = synth.c2_float32(8192, 8192, device="cuda:0")
    blob, y = _device_roundtrip(x, 0.01, streamed=True)
    err = float((y.double() - x.double()).abs().max().item())
    assert err <= 0.01 + 6.2e-5
    xh = x.cpu().numpy()
    rc, b2 = O.encode(xh, 0.01)
    assert rc == 0 and len(b2) == len(blob) and sha(b2) == sha(blob)
    chk = capi.ref() or O
    rc, dec, _ = chk.decode(blob)
    assert rc == 0 and np.array_equal(dec.reshape(8192, 8192), y.cpu().numpy())
    # idempotence: encoding the decoded raster again cannot move any pixel by more than the bound
    blob2, y2 = _device_roundtrip(y, 0.01)
    assert float((y2.double() - y.double()).abs().max().item()) <= 0.01 + 6.2e-5


def test_flat_stretches_stay_on_the_scanning_decoder_at_full_size(P, O):
    """The C2 raster with 15 % of its area flat (rectangles of one value: runs of constant and all-zero blocks, 256 ... 384 on end, in
    every piece of the stream): the scanning decoder's first wave walks the runs, pieces that begin inside one take their first block's
    place from the piece in front.  Blob = the oracle's, pixels = the oracle's decode; the first such band of a context costs one
    launch (its early counts are wrong), the bands behind it none; the same with uint16 (two vectors of blocks a lane less)."""
    import torch
    from lerc_amd import api, synth
    for make, e, n in ((lambda: synth.c2_float32(8192, 8192, device="cuda:0"), 0.01, 8192),
                       (lambda: synth.c3_uint16(4096, 8192, device="cuda:0"), 0, 4096)):
        x = make()
        xv = x if x.dtype == torch.float32 else x.view(torch.int16)    # (the same bits: values below 2^15)
        for (r0, r1, c0, c1, val) in ((512, 2560, 1024, 3584, 1017), (3000, 4096, 4096, 7168, 733), (1000, 2024, 256, 2304, 1500), (3072, 3584, 0, 2048, 0)):
            xv[r0:min(r1, n), c0:c1] = val
        if x.dtype == torch.float32:
            x[512:2560, 1024:3584] += 0.25
        codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
        out = torch.empty(x.numel() * x.element_size() + (1 << 20), dtype=torch.uint8, device=x.device)
        y = torch.empty_like(x)
        rc, nb = api.encode_device(codec, x, e, out)
        assert rc == 0
        xh = x.cpu().numpy()
        rc, b2 = O.encode(xh, e)
        blob = out[:nb].cpu().numpy().tobytes()
        assert rc == 0 and len(b2) == nb and sha(b2) == sha(blob)
        seen = []
        for _ in range(3):
            f0, q0 = codec.decode_forms(), codec.decode_refusals()
            y.zero_()
            rc = api.decode_device(codec, out, nb, y)
            assert rc == 0, codec.last_error()
            torch.cuda.synchronize()
            f1, q1 = codec.decode_forms(), codec.decode_refusals()
            seen.append((f1[3] - f0[3], q1[2] - q0[2]))
            rc, dec, _ = O.decode(blob)
            assert rc == 0 and np.array_equal(dec.reshape(xh.shape), y.cpu().numpy())
        assert seen == [(1, 1), (1, 0), (1, 0)], (seen, codec.last_note())


def test_ragged_rasters_on_the_scanning_decoder_at_full_size(P, O):
    """Rasters whose sides are no multiples of 8 -- the shapes the reference was benchmarked on -- decode on the scanning decoder (its RAG
    instantiation: the edge blocks' count bytes in the filter, a block's size checked against its place, raw corner blocks, partial rows stored
    pixel by pixel): pixels = the oracle's decode of the same blob, the blob = the oracle's, `decode_forms()[3]` counts the band.  8190 x 8190
    float32 (rows at 8-byte alignment), 2049 x 4097 uint16 (odd pitch: pixel stores), 257 x 257 (a one-pixel raw corner), 1201 x 1001 int32."""
    import torch
    from lerc_amd import api, synth
    for shape, dt, e in (((8190, 8190), torch.float32, 0.01), ((2049, 4097), "u16", 0), ((257, 257), torch.float32, 0.01), ((1201, 1001), torch.int32, 0),
                         ((4300, 4600), torch.float32, 0.01)):
        r, c = shape
        x = synth.c2_float32(r + 8, c + 8, device="cuda:0")[:r, :c].contiguous()
        if dt == "u16":
            x = (x * 8).to(torch.int32).to(torch.uint16).contiguous()
        elif dt == torch.int32:
            x = (x * 8).to(torch.int32).contiguous()
        codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
        out = torch.empty(x.numel() * x.element_size() + (1 << 20), dtype=torch.uint8, device=x.device)
        y = torch.zeros_like(x)
        rc, nb = api.encode_device(codec, x, e, out)
        assert rc == 0, codec.last_error()
        f0 = codec.decode_forms()
        rc = api.decode_device(codec, out, nb, y)
        assert rc == 0, codec.last_error()
        torch.cuda.synchronize()
        f1 = codec.decode_forms()
        assert f1[3] == f0[3] + 1, (shape, f0, f1, codec.last_note())
        blob = out[:nb].cpu().numpy().tobytes()
        xh = x.cpu().numpy()
        rc, b2 = O.encode(xh, e)
        assert rc == 0 and len(b2) == nb and sha(b2) == sha(blob), shape
        rc, dec, _ = O.decode(blob)
        assert rc == 0 and np.array_equal(dec.reshape(xh.shape), y.cpu().numpy()), shape


def test_mask_and_statistics_in_one_read_at_full_size(P, O):
    """A masked 8192 x 4096 float32 band (and a uint16 one): the bit mask and the band's statistics come out of one kernel (the profile
    says which), the blob is the oracle's -- NaNs under the mask and beside it."""
    import ctypes as ct
    import torch
    from lerc_amd import api, synth
    for make, e in ((lambda: synth.c2_float32(4096, 8192, device="cuda:0"), 0.01), (lambda: synth.c3_uint16(2048, 8192, device="cuda:0"), 0)):
        x = make()
        r, c = x.shape
        ii = torch.arange(r, device=x.device).view(-1, 1); jj = torch.arange(c, device=x.device).view(1, -1)
        mk = (((ii // 97) + (jj // 131)) % 10 != 0).to(torch.uint8).contiguous()
        if x.dtype == torch.float32:
            x[5, 7] = float("nan"); x[1000, 4000] = float("nan"); x[0, 0] = float("nan")
        codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
        L = codec.lib
        L.lerc_amd_profile_enable.argtypes = [ct.c_void_p, ct.c_int]
        L.lerc_amd_profile_read.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int]
        out = torch.empty(x.numel() * x.element_size() + (1 << 20), dtype=torch.uint8, device=x.device)
        L.lerc_amd_profile_enable(codec.h, 1)
        rc, nb = codec.encode(x.data_ptr(), api._torch_dt_code(x), 1, c, r, 1, e, out.data_ptr(), out.numel(), mk.data_ptr(), 1)
        assert rc == 0, codec.last_error()
        L.lerc_amd_profile_enable(codec.h, 0)
        buf = ct.create_string_buffer(1 << 16)
        L.lerc_amd_profile_read(codec.h, buf, len(buf), 1)
        names = [ln.split()[0] for ln in buf.value.decode().splitlines()]
        assert "mask_stats" in names and "build_mask" not in names and "band_stats" not in names, names
        rc, b2 = O.encode(x.cpu().numpy(), e, mask=mk.cpu().numpy())
        assert rc == 0 and len(b2) == nb and sha(b2) == sha(out[:nb].cpu().numpy().tobytes())


def test_c3_full_size_16384_uint16_lossless(P, O):
    """BASELINE configs[2]: lossless integer path, bit exact round trip, identical to the oracle."""
    import torch
    from lerc_amd import synth
    x = synth.c3_uint16(16384, 16384, device="cuda:0")
    blob, y = _device_roundtrip(x, 0.0, streamed=True)
    assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    xh = x.cpu().numpy()
    rc, b2 = O.encode(xh, 0)
    assert rc == 0 and len(b2) == len(blob) and sha(b2) == sha(blob)


def test_c5_tiles_are_independent_blobs(P, O):
    """BASELINE configs[4] in miniature: 256 x 256 windows of the virtual raster are independent blobs."""
    from lerc_amd import synth
    for (tr, tc) in ((0, 0), (3, 7), (255, 255)):
        t = synth.c5_tile(tr, tc).numpy()
        r1, b1 = P.encode(t, 0.01)
        r2, b2 = O.encode(t, 0.01)
        assert r1 == r2 == 0 and b1 == b2


def test_c5_tile_batch_in_one_call(P, O):
    """BASELINE configs[4]: a rank's share of the mosaic goes through lerc_amd_encode_tiles_device /
    lerc_amd_decode_tiles_device in one call.  Every blob equals the per-tile lerc_encode() blob (oracle on a sample),
    all tiles round-trip within the bound, and tiles the streaming kernels hand back are still right."""
    import torch
    from lerc_amd import api, synth
    dev = torch.device("cuda:0")
    n_side = 16                                                    # 256 tiles = a 4096 x 4096 window of the virtual raster
    big = synth.c2_float32(256 * n_side, 256 * n_side, virt_cols=65536, device=dev)
    tiles = big.reshape(n_side, 256, n_side, 256).permute(0, 2, 1, 3).contiguous().reshape(n_side * n_side, 256, 256)
    tiles[5] = 7.25                                                # a constant tile (ocean): general path inside the batch
    tiles[9] = torch.round(tiles[9])                               # all-integer floats: bIsInt promotion
    n_tiles = tiles.shape[0]
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    arena = torch.empty(tiles.numel() * 4 + n_tiles * 256, dtype=torch.uint8, device=dev)
    rc, offs, sizes, used = api.encode_tiles_device(codec, tiles, 0.01, arena)
    assert rc == 0, (rc, codec.last_error())
    assert (offs % 16 == 0).all() and int(offs.max()) < used <= arena.numel()
    ah = arena[:used].cpu().numpy()
    th = tiles.cpu().numpy()
    for t in (0, 1, 5, 9, 100, n_tiles - 1):
        r1, b1 = O.encode(th[t], 0.01)
        assert r1 == 0 and ah[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() == b1, t
    out = torch.empty_like(tiles)
    rc = api.decode_tiles_device(codec, arena, offs, sizes, out)
    assert rc == 0, (rc, codec.last_error())
    torch.cuda.synchronize()
    assert float((out.double() - tiles.double()).abs().max().item()) <= 0.01 + 6.2e-5
    for t in (0, 5, 9, n_tiles - 1):
        want = O.decode(ah[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes())
        assert np.array_equal(want[1].reshape(256, 256), out[t].cpu().numpy())
    cnt = (ct.c_ulonglong * 4)()
    codec.lib.lerc_amd_path_counters.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
    codec.lib.lerc_amd_path_counters(codec.h, cnt)
    assert cnt[0] == n_tiles - 2 and cnt[2] >= n_tiles - 4, list(cnt)    # the batch really went through the streaming kernels


def test_elevation_tile_batch_257(P, O):
    """A mosaic of 257 x 257 tiles (Esri's elevation tile caches; rows / columns no multiples of 8, tiles 4 bytes off a 16-byte
    grid) in one batched call each way: the ragged forms of the streaming kernels take them (path counters), blobs are the
    per-tile oracle blobs."""
    import torch
    from lerc_amd import api, synth
    dev = torch.device("cuda:0")
    n_tiles = 96
    big = synth.c2_float32(257 * 8, 257 * 12, virt_cols=65536, device=dev)
    tiles = big.reshape(8, 257, 12, 257).permute(0, 2, 1, 3).contiguous().reshape(n_tiles, 257, 257)
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    arena = torch.empty(tiles.numel() * 4 + n_tiles * 256, dtype=torch.uint8, device=dev)
    rc, offs, sizes, used = api.encode_tiles_device(codec, tiles, 0.01, arena)
    assert rc == 0, (rc, codec.last_error())
    ah = arena[:used].cpu().numpy()
    th = tiles.cpu().numpy()
    for t in (0, 1, 50, n_tiles - 1):
        r1, b1 = O.encode(th[t], 0.01)
        assert r1 == 0 and offs[t] % 16 == 0 and ah[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() == b1, t
    out = torch.empty_like(tiles)
    rc = api.decode_tiles_device(codec, arena, offs, sizes, out)
    assert rc == 0, (rc, codec.last_error())
    torch.cuda.synchronize()
    assert float((out.double() - tiles.double()).abs().max().item()) <= 0.01 + 6.2e-5
    for t in (0, 50, n_tiles - 1):
        want = O.decode(ah[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes())
        assert np.array_equal(want[1].reshape(257, 257), out[t].cpu().numpy())
    assert codec.path_counters()[0] == n_tiles and codec.path_counters()[2] == n_tiles, codec.path_counters()


@pytest.mark.parametrize("shape", [(256, 256), (257, 257)])
def test_tile_batches_with_a_slot_per_tile(P, O, shape):
    """lerc_amd_encode_tiles_device_slots: every tile's blob written straight into its slot (t * slotBytes) by the encode kernel --
    no packing pass -- and decoded from there; blobs are the per-tile oracle blobs, both ways on the streaming kernels."""
    import torch
    from lerc_amd import api, synth
    dev = torch.device("cuda:0")
    r, c = shape
    n_tiles = 96
    big = synth.c2_float32(r * 8, c * 12, virt_cols=65536, device=dev)
    tiles = big.reshape(8, r, 12, c).permute(0, 2, 1, 3).contiguous().reshape(n_tiles, r, c)
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    slot = (r * c * 4 // 2 + 4096 + 15) // 16 * 16
    slots = torch.full((n_tiles * slot,), 0xEE, dtype=torch.uint8, device=dev)
    rc, sizes = api.encode_tiles_device_slots(codec, tiles, 0.01, slots, slot)
    assert rc == 0, (rc, codec.last_error())
    sh = slots.cpu().numpy()
    th = tiles.cpu().numpy()
    for t in (0, 1, 50, n_tiles - 1):
        r1, b1 = O.encode(th[t], 0.01)
        assert r1 == 0 and sh[t * slot:t * slot + int(sizes[t])].tobytes() == b1, t
    out = torch.empty_like(tiles)
    rc = api.decode_tiles_device_slots(codec, slots, slot, sizes, out)
    assert rc == 0, (rc, codec.last_error())
    torch.cuda.synchronize()
    for t in (0, 50, n_tiles - 1):
        want = O.decode(sh[t * slot:t * slot + int(sizes[t])].tobytes())
        assert np.array_equal(want[1].reshape(r, c), out[t].cpu().numpy())
    assert codec.path_counters()[0] == n_tiles and codec.path_counters()[2] == n_tiles, codec.path_counters()
    # slots too small for the blobs
    rc, _ = api.encode_tiles_device_slots(codec, tiles, 0.01, slots, 1024)
    assert rc == 3


def test_masked_bands_take_the_one_launch_encoder(P, O):
    """Bands with a validity mask: the block stream comes from the one-launch encoder's masked form (the note says so), written in
    place behind the band's mask and ranges; bytes are the oracle's, for blob-shaped masks, salt-and-pepper masks, masks that
    leave whole block rows empty and a single valid pixel."""
    rng = np.random.default_rng(21)
    for dt, e, shape in ((np.float32, 0.01, (1024, 1536)), (np.uint16, 0, (512, 1024)), (np.float64, 0.001, (256, 512)), (np.int32, 2, (640, 640)),
                         (np.float32, 0.01, (1001, 1203)), (np.uint16, 0, (257, 257)), (np.float64, 0.5, (130, 1027))):    # (the last three: ragged)
        r, c = shape
        x = cases._cast(cases.terrain(r, c, rng, amp=300, base=1000, sigma=2.0), dt)
        for style in range(4):
            m = np.ones((r, c), np.uint8)
            if style == 0:
                for _ in range(12):
                    i0, j0 = int(rng.integers(0, r)), int(rng.integers(0, c))
                    m[i0:i0 + int(rng.integers(1, 200)), j0:j0 + int(rng.integers(1, 300))] = 0
            elif style == 1:
                m = (rng.random((r, c)) > 0.05).astype(np.uint8)
            elif style == 2:
                m[: r // 2] = 0
                m[:, ::7] = 0
            else:
                m[:] = 0
                m[r // 3, c // 5] = 1
                m[r - 1, :] = 1
            r1, b1 = O.encode(x, e, mask=m)
            r2, b2 = P.encode(x, e, mask=m)
            assert r1 == r2 == 0 and b1 == b2, (np.dtype(dt).name, style)
            assert "one-launch encoder" in P.last_note(), P.last_note()
            d1, d2 = O.decode(b1), P.decode(b1)
            assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1]) and _same(d1[2], d2[2])
        assert O.encode(x, e, mask=m, buf_size=len(b1) - 1)[0] == P.encode(x, e, mask=m, buf_size=len(b1) - 1)[0] == 3


def test_masked_bands_are_cut_into_blocks_by_the_scan_on_the_gpu(P, O):
    """The scan's form for bands with a mask (tile_fast_decode_scan.hip, MODE 1) on hardware, at its full piece size: rectangular
    holes, an ellipse (curved edges: raw blocks of one or two pixels, the run to the next block row's edge), slanted bands, columns
    without a pixel (runs longer than what a piece stages in front of its own bytes), block rows without.  Pixels and masks are the
    oracle's, every band is served by the scan (lerc_amd_decode_forms()[0]) and none by a second attempt; damaged copies get the
    oracle's verdict."""
    rng = np.random.default_rng(77)
    r, c = 1024, 4096
    ii, jj = np.mgrid[0:r, 0:c]
    masks = {
        "stripes": (((ii // 97) + (jj // 131)) % 10 != 0).astype(np.uint8),
        "an ellipse": ((ii - r / 2) ** 2 / (0.55 * r) ** 2 + (jj - c / 2) ** 2 / (0.44 * c) ** 2 < 1).astype(np.uint8),    # (cut off above and below: no block row without a pixel)
        "slanted bands": ((ii + jj) % 300 < 200).astype(np.uint8),
        "columns without a pixel": ((jj >= 1200) & (jj < 3900)).astype(np.uint8) ^ 1,
        "a block row without": ((ii % 256) >= 8).astype(np.uint8),
    }
    # (a piece's list holds 2048 blocks: streams of mostly one-byte blocks -- 16-bit data with long runs -- go to the general discovery)
    wide = (np.arange(8192)[None, :] < 1400).astype(np.uint8) * np.ones((256, 1), np.uint8)    # runs of 850: longer than a piece stages in front
    n_refused = 0
    for dt, e in ((np.float32, 0.01), (np.uint16, 0), (np.int32, 0), (np.float64, 0.001)):
        x = cases._cast(cases.terrain(1024, 4096, rng, amp=300, base=1000, sigma=2.0), dt)
        todo = [(name, x, m) for name, m in masks.items() if not (name == "columns without a pixel" and np.dtype(dt).itemsize == 2)]
        if dt == np.float32:
            todo.append(("runs of 850", cases._cast(cases.terrain(256, 8192, rng, amp=300, base=1000, sigma=2.0), dt), wide))
        for name, x, m in todo:
            r, c = m.shape
            r1, b1 = O.encode(x, e, mask=m)
            assert r1 == 0
            f0, c0, q0 = P.decode_forms(), P.path_counters(), P.decode_refusals()
            d1, d2 = O.decode(b1), P.decode(b1)
            f1, c1, q1 = P.decode_forms(), P.path_counters(), P.decode_refusals()
            v = d1[2].reshape(r, c) != 0
            assert d1[0] == d2[0] == 0 and _same(d1[2], d2[2]) and np.array_equal(d1[1].reshape(r, c)[v], d2[1].reshape(r, c)[v]), (np.dtype(dt).name, name)
            # A raw block's length is a guess the decode kernels may refuse (two-byte values leave the chain of blocks behind it more room to
            # come out right twice); the band then goes to the general discovery.  That is a thrown-away pass, so it is COUNTED
            # (lerc_amd_decode_refusals) and bounded: one band of this matrix at most -- 16-bit data under the ellipse's curved edge.
            served, refused, handed_on = f1[0] - f0[0], q1[0] - q0[0], q1[1] - q0[1]
            assert served + refused + handed_on == 1 and handed_on == 0, ("the scan neither served nor refused the band", np.dtype(dt).name, name, P.last_note())
            if refused:
                assert np.dtype(dt).itemsize == 2 and name == "an ellipse" and "refused the scan's block offsets" in P.last_note(), (np.dtype(dt).name, name, P.last_note())
            n_refused += refused
            if dt == np.float32:
                bad = bytearray(b1)
                k = int(rng.integers(len(b1) // 2, len(b1)))
                bad[k] ^= 1 << int(rng.integers(0, 8))
                assert (O.decode(bytes(bad))[0] == 0) == (P.decode(bytes(bad))[0] == 0), (name, k)
    assert n_refused <= 1, n_refused


def test_several_bands_with_a_large_mask_each_decoded_on_the_device(P, O):
    """Three and four bands, every band with a noisy mask of its own that is large enough for the DEVICE's run-length decoder at its default
    threshold (2 M pixels and more a band; round-4 review: a band's workspace tables once started behind the band before's and the second
    large mask found no room -- covered on the emulator with the threshold forced down, and here on the device it was found for).  Blob ==
    oracle's, decode == oracle's, masks and all; one-sweep and tiling bands, float and 16-bit."""
    rng = np.random.default_rng(404)
    for dt, e, bands, (r, c) in ((np.float32, 0.01, 3, (1536, 2048)), (np.uint16, 0, 4, (2048, 1024)), (np.float32, 1e-7, 3, (1024, 2304))):
        x = np.stack([cases._cast(cases.terrain(r, c, rng, amp=200 + 50 * k, base=1000, sigma=2.0), dt) for k in range(bands)])
        m = np.stack([(rng.random((r, c)) > 0.03 + 0.02 * k).astype(np.uint8) for k in range(bands)])
        for k in range(bands):
            m[k, 100 * (k + 1): 100 * (k + 1) + 64, :] = 0
        assert r * c // 8 >= 256 * 1024, "the device's mask coder takes masks from 256 KB"
        r1, b1 = O.encode(x, e, n_bands=bands, mask=m)
        assert r1 == 0
        r2, b2 = P.encode(x, e, n_bands=bands, mask=m)
        assert r2 == 0 and bytes(b2) == bytes(b1), (np.dtype(dt).name, bands, len(b1), len(b2))
        d1 = O.decode(b1, want_masks=bands, n_bands=bands)
        d2 = P.decode(b1, want_masks=bands, n_bands=bands)
        assert d1[0] == d2[0] == 0 and _same(d1[2], d2[2]), (np.dtype(dt).name, bands)
        v = np.asarray(d1[2]).reshape(bands, r, c) != 0
        assert np.array_equal(np.asarray(d1[1]).reshape(bands, r, c)[v], np.asarray(d2[1]).reshape(bands, r, c)[v]), (np.dtype(dt).name, bands)
        assert np.array_equal(v, m != 0)


def test_nodata_values(P, O):
    """lerc_encode_4D / lerc_decode_4D with per-band noData values, differential against the real reference (or the
    oracle): sizes, blobs, decoded pixels, masks and the noData values handed back."""
    T = capi.ref() or O
    for name, arr, e, kw in cases.nodata_fuzz_cases(120):
        cases.check_nodata_case(T, P, name, arr, e, kw, _same)


def test_many_values_per_pixel(P, O):
    """nDepth of several hundred (hyperspectral cubes): blobs, pixels, masks, info and ranges as the oracle's"""
    for name, arr, e, kw in cases.deep_pixel_cases():
        cases.check_deep_pixel_case(O, P, name, arr, e, kw, _same)


def test_encode_for_older_codec_versions(P, O):
    """lerc_encodeForVersion / lerc_computeCompressedSizeForVersion, codec 3..5 (Lerc.cpp:526-624): status, size and
    blob bytes as the oracle's (itself pinned on the real reference by tests/test_oracle_vs_reference.py), and against
    the real reference when it travelled."""
    for name, arr, ver, e, kw in cases.old_codec_cases(200):
        cases.check_old_codec_case(O, P, name, arr, ver, e, kw, _same)
    R = capi.ref()
    if R is not None:
        for name, arr, ver, e, kw in cases.old_codec_cases(100, seed=72):
            cases.check_old_codec_case(R, P, name, arr, ver, e, kw, _same)


def test_lossless_float(P, O):
    """maxZErr == 0 on float / double rasters (Lerc2 IEM_DeltaDeltaHuffman): golden vectors of the real reference, the
    oracle, the real reference itself when it travelled, and rasters large enough for every scan to span many workgroups."""
    vec = json.load(open(os.path.join(GOLD, "fpl_vectors.json")))
    cases.check_lossless_float_golden(P, vec, os.path.join(GOLD, "blobs"), sha)
    for name, arr, kw in cases.lossless_float_cases(150, seed=93, max_side=300):
        cases.check_lossless_float_case(O, P, name, arr, kw, _same)
    rng = np.random.default_rng(8)
    R = capi.ref()
    for dt, shape in ((np.float32, (2048, 3000)), (np.float64, (1500, 1111))):
        x = (cases.terrain(shape[0], shape[1], rng, sigma=0.02) + np.cumsum(rng.standard_normal(shape), axis=1) * 1e-3).astype(dt)
        x[100:400, 200:900] = 7.25
        cases.check_lossless_float_case(O, P, "large-" + np.dtype(dt).name, x, {}, _same)
        if R is not None:
            cases.check_lossless_float_case(R, P, "large-" + np.dtype(dt).name, x, {}, _same)
    if R is not None:
        for name, arr, kw in cases.lossless_float_cases(60, seed=95, max_side=300):
            cases.check_lossless_float_case(R, P, name, arr, kw, _same)


def test_lossless_float_round_trip_full_size(P):
    """8192 x 8192 float32, maxZErr 0: decode(encode(x)) == x bit for bit, and the blob is smaller than the raster."""
    from lerc_amd import synth
    x = synth.c2_float32().numpy()
    rc, blob = P.encode(x, 0)
    assert rc == 0 and len(blob) < x.nbytes
    d = P.decode(blob)
    assert d[0] == 0 and _same(d[1].reshape(x.shape), x)


def test_any_width_takes_the_streaming_kernels(P, O):
    """unmasked rasters of whole 8 x 8 blocks, any width: a workgroup's blocks wrap around block row ends, the last
    workgroup is partly empty -- still the streaming kernels, still the oracle's bytes"""
    rng = np.random.default_rng(12)
    for dt, shape, e in ((np.float32, (4000, 3000), 0.01), (np.uint16, (1000, 1000), 0), (np.float64, (808, 1208), 0.001),
                         (np.int32, (2048, 1032), 0), (np.float32, (8, 8), 0.01), (np.float32, (1600, 8), 0.01)):
        x = cases._cast(cases.terrain(shape[0], shape[1], rng, amp=300, base=1000, sigma=1.5), dt)
        r1, b1 = O.encode(x, e)
        c0 = P.path_counters()
        r2, b2 = P.encode(x, e)
        c1 = P.path_counters()
        assert r1 == r2 == 0 and b1 == b2, (np.dtype(dt).name, shape)
        assert c1[0] > c0[0], (np.dtype(dt).name, shape, P.last_note())
        d1, d2 = O.decode(b1), P.decode(b1)
        assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1])
        if len(b1) > 8192:
            assert P.path_counters()[2] > c1[2], (np.dtype(dt).name, shape, P.last_note())


def test_damaged_blobs_of_every_path(P, O):
    """flipped / overwritten / zeroed bytes and truncation in blobs of every path: the oracle's verdict, no fault on the device"""
    for name, blob in cases.damaged_blob_cases(O, 40):
        cases.check_damaged_blob(O, P, name, blob, _same)


def test_several_bands_take_the_streaming_kernels(P, O):
    rng = np.random.default_rng(32)
    for dt, e, shape in ((np.uint16, 0, (3, 1024, 1024)), (np.float32, 0.01, (2, 1000, 1200)), (np.float64, 0.001, (4, 256, 512))):
        x = np.stack([cases._cast(cases.terrain(shape[1], shape[2], rng, amp=300, base=1000 + 50 * b, sigma=1.5), dt) for b in range(shape[0])])
        c0 = P.path_counters()
        r1, b1 = O.encode(x, e, n_bands=shape[0])
        r2, b2 = P.encode(x, e, n_bands=shape[0])
        assert r1 == r2 == 0 and b1 == b2, np.dtype(dt).name
        assert P.path_counters()[0] >= c0[0] + 2, (np.dtype(dt).name, P.last_note())
        d1, d2 = O.decode(b1), P.decode(b1)
        assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1])


def test_later_bands_do_not_see_the_cells_of_earlier_ones(P, O):
    """Several streamed bands of one decode call share the context's epoch-tagged cells: every band has to come with an
    epoch of its own, or band k + 1 reads what band k left there (block indices, walks, group totals).  Band 0's blob must
    be a multiple of 16 bytes long for band 1 to qualify for the streaming decoder at all, so the raster is searched for."""
    import struct
    rng = np.random.default_rng(77)
    n = 512
    b0 = cases._cast(cases.terrain(n, n, rng, amp=300, base=1000, sigma=1.5), np.uint16)
    b1 = cases._cast(cases.terrain(n, n, rng, amp=30, base=200, sigma=12.0), np.uint16)    # other block sizes, other counts per chunk
    found = 0
    for k in range(64):
        c = b0.copy()
        for q in range(k):    # blocks of small values: one-byte offsets and other widths move the band's size by odd amounts
            c[8 * (q % 5):8 * (q % 5) + 8, 8 * q:8 * q + 8] = rng.integers(10, 10 + 2 ** (1 + q % 6), (8, 8))
        x = np.stack([c, b1, c[::-1].copy()])
        r1, blob = O.encode(x, 0, n_bands=3)
        assert r1 == 0
        if struct.unpack_from("<i", blob, 34)[0] % 16:
            continue
        found += 1
        c0 = P.path_counters()
        d1, d2 = O.decode(blob), P.decode(blob)
        assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1]), k
        assert P.path_counters()[2] > c0[2], P.last_note()
        assert np.array_equal(d2[1].reshape(3, n, n), x)
    assert found >= 2


def test_ragged_rasters_take_the_streaming_kernels(P, O):
    """8190 x 8190 and the 257 x 257 of Esri's elevation tiles (rows / columns no multiples of 8) on the one-launch encoder and
    the streaming decoder: path counters say so, bytes and pixels are the oracle's."""
    rng = np.random.default_rng(41)
    for dt, e, shape in ((np.float32, 0.01, (257, 257)), (np.uint16, 0, (257, 257)), (np.float32, 0.01, (1000, 1201)), (np.int32, 0, (515, 130)),
                         (np.float64, 0.001, (63, 65)), (np.float32, 0.01, (2050, 4099))):
        x = cases._cast(cases.terrain(shape[0], shape[1], rng, amp=300, base=1000, sigma=2.0), dt)
        c0 = P.path_counters()
        r1, b1 = O.encode(x, e)
        r2, b2 = P.encode(x, e)
        assert r1 == r2 == 0 and b1 == b2, (np.dtype(dt).name, shape)
        d1, d2 = O.decode(b1), P.decode(b1)
        assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1]), (np.dtype(dt).name, shape)
        c1 = P.path_counters()
        assert c1[0] - c0[0] == 2 and c1[2] - c0[2] == 1, (np.dtype(dt).name, shape, c0, c1, P.last_note())
    # full size, on the device: decode == what the oracle-checked small cases promise, error bound, re-encode idempotent
    import torch
    from lerc_amd import api, synth
    dev = torch.device("cuda:0")
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    x = synth.c2_float32(8192, 8192, device=dev)[:8190, :8190].contiguous()
    blob = torch.empty(x.numel() * 4 + 4096, dtype=torch.uint8, device=dev)
    y = torch.empty_like(x)
    c0 = codec.path_counters()
    rc, n = api.encode_device(codec, x, 0.01, blob)
    assert rc == 0
    rc = api.decode_device(codec, blob, n, y)
    assert rc == 0
    c1 = codec.path_counters()
    assert c1[0] - c0[0] == 1 and c1[2] - c0[2] == 1, (c0, c1)
    assert float((y.double() - x.double()).abs().max()) <= 0.01 * (1 + 1e-6) + 6.2e-5
    # ... and the bytes: the blob's size is what the size query says, and the general kernels read the same pixels out of it
    rc, need = codec.encode(x.data_ptr(), 6, 1, 8190, 8190, 1, 0.01, 0, 0)    # (no output buffer: the size query)
    assert rc == 0 and need == n
    rc, dec_general, _ = P.decode(blob[:n].cpu().numpy().tobytes())    # host call: stages the blob itself
    assert rc == 0 and bool(np.array_equal(dec_general.reshape(8190, 8190), y.cpu().numpy()))


def test_first_row_errors_are_read_after_they_are_written(P, O):
    """The one-launch encoder's last workgroup takes TryRaiseMaxZError's first-row errors from cells that workgroup 0 writes
    while the launch runs.  On rasters of one residency round the two run side by side, and the last one used to read before
    it had seen the writer arrive (the barrier in fusedFinish): zeros in a fresh context -- the band went to the general
    kernels for nothing, 3 calls in 100 --, in a context that had seen another raster THAT raster's errors -- a band whose
    error bound the reference raises could have kept the requested one.  Fresh contexts must stream every call; a raster on the
    0.1 grid between rasters off it must come out as the oracle's bytes every time."""
    import torch
    from lerc_amd import api, synth
    dev = torch.device("cuda:0")
    x = synth.c2_float32(2048, 4096, device=dev)
    blob = torch.empty(x.numel() * 4 + 4096, dtype=torch.uint8, device=dev)
    y = torch.empty_like(x)
    # (the codecs below run on streams of their own, which are not ordered behind the stream that is still WRITING x: without this wait
    # the first encode once read a raster that was not there yet -- leftovers of another test's blob: NaN, absurd sizes, reason bits
    # 0x61 -- and "fell back" once in six runs of the suite.  The test's race, not the library's.)
    torch.cuda.synchronize()
    fell = 0
    notes = []
    for i in range(200):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            codec = api.DeviceCodec(s.cuda_stream)
            rc, nb = api.encode_device(codec, x, 0.01, blob)
            rc2 = api.decode_device(codec, blob, nb, y)
            c = codec.path_counters()
            f = codec.decode_forms()
            if c[1] != 0 or c[3] != 0 or f[3] != 1: notes.append((i, list(c), list(f), codec.last_note(), codec.last_error()))
            codec.close()
        assert rc == 0 and rc2 == 0, (i, rc, rc2, list(c))
        fell += int(c[1] != 0 or c[3] != 0 or f[3] != 1)
    # (before the barrier: 6 of 200 on average.  None since.  A hand-off that times out while other processes keep the GPU busy
    # sends a call the same way, by design: LERC_AMD_TEST_SHARED_GPU=1 lets two pass -- the driver's run owns its GPU)
    assert fell <= (2 if os.environ.get("LERC_AMD_TEST_SHARED_GPU") else 0), (fell, notes[:4])
    rng = np.random.default_rng(77)
    off = cases.terrain(1024, 2048, rng, amp=300, base=1000, sigma=2.0).astype(np.float32)          # nothing to raise
    on = np.round(cases.terrain(1024, 2048, rng, amp=300, base=1000, sigma=2.0), 1).astype(np.float32)    # every value on the 0.1 grid
    r_off, b_off = O.encode(off, 0.01)
    r_on, b_on = O.encode(on, 0.01)
    assert r_off == r_on == 0 and O.blob_info(b_on)[2][2] > 0.02    # (the reference raises the bound for the second)
    for i in range(60):
        r1, b1 = P.encode(off, 0.01)
        r2, b2 = P.encode(on, 0.01)
        assert r1 == r2 == 0 and b1 == b_off and b2 == b_on, i


def test_workgroups_that_give_up_waiting_fall_back_to_the_general_path():
    """The hand-offs inside the one-launch encoder and the streaming decoder (size cells, aggregator cells, the resolving
    blocks' cells) rely on workgroups starting in index order.  LERC_AMD_TEST_GIVEUP makes every such cell arrive with a tag
    nobody waits for, so every waiter runs into its poll limit: the calls must then come back through the general kernels
    with the reference's bytes -- slower, never wrong, never hanging.  (A process of its own: the knob is read once.)"""
    import subprocess
    import sys
    code = r"""
import sys, os
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, capi, cases
P, O = capi.product(), capi.oracle()
rng = np.random.default_rng(5)
for dt, e in ((np.float32, 0.01), (np.uint16, 0)):
    x = cases._cast(cases.terrain(1024, 1536, rng, amp=300, base=1000, sigma=2.0), dt)
    c0 = P.path_counters()
    r1, b1 = O.encode(x, e)
    r2, b2 = P.encode(x, e)
    assert r1 == r2 == 0 and b1 == b2, "blob"
    d1, d2 = O.decode(b1), P.decode(b1)
    assert d1[0] == d2[0] == 0 and np.array_equal(d1[1].view(np.uint8), d2[1].view(np.uint8)), "pixels"
    c1 = P.path_counters()
    assert c1[1] > c0[1] and c1[3] > c0[3], (c0, c1)    # both went the long way
print("gave up and recovered")
""" % (capi.ROOT,)
    env = dict(os.environ, LERC_AMD_TEST_GIVEUP="3")
    out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0 and b"gave up and recovered" in out.stdout, out.stdout.decode()[-2000:]


@pytest.mark.parametrize("launches,giveup", [("1", "0"), ("1", "2"), ("1", "4"), ("2", "0"), ("2", "2")])
def test_streaming_decoder_in_one_launch_and_in_two(launches, giveup):
    """The streaming decoder is ONE launch (k_fast_decode_one: a workgroup of 512 threads stages 16 chunks of the blob, finds
    their block starts and decodes them; a block count per workgroup is all that travels between workgroups);
    LERC_AMD_DECODE_LAUNCHES=2 keeps the two-launch form.  Same pixels as the oracle, streaming path taken, rasters whose sides
    are no multiples of 8 and damaged blobs included -- and, with the hand-offs made to fail (LERC_AMD_TEST_GIVEUP=2), the general
    path takes over; =4 makes the one-launch decoder walk every chunk's path a second time (what it does for the rare chunk
    whose path is not its first walk)."""
    import subprocess
    import sys
    code = r"""
import sys, os
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, capi, cases
P, O = capi.product(), capi.oracle()
giveup = os.environ.get("LERC_AMD_TEST_GIVEUP", "0") == "2"
one = os.environ.get("LERC_AMD_DECODE_LAUNCHES") != "2"
rng = np.random.default_rng(11)
for dt, e, shape in ((np.float32, 0.01, (2048, 3072)), (np.uint16, 0, (1024, 1536)), (np.float64, 0.001, (512, 1024)), (np.int32, 0, (1001, 777)),
                     (np.float32, 0.5, (257, 257)), (np.int16, 0, (64, 64))):
    x = cases._cast(cases.terrain(shape[0], shape[1], rng, amp=300, base=1000, sigma=2.0), dt)
    r1, b1 = O.encode(x, e)
    assert r1 == 0
    c0 = P.path_counters()
    d1, d2 = O.decode(b1), P.decode(b1)
    c1 = P.path_counters()
    assert d1[0] == d2[0] == 0 and np.array_equal(d1[1].view(np.uint8), d2[1].view(np.uint8)), ("pixels", shape)
    several = len(b1) > 32768    # (one launch: a blob of one workgroup -- 32 KiB -- waits for nobody)
    if giveup and (several or not one): assert c1[3] > c0[3], (c0, c1, shape)
    if not giveup: assert c1[2] > c0[2] and c1[3] == c0[3], (c0, c1, shape, P.last_note())
    for t in range(12):    # damaged copies: same status as the oracle, and the same pixels where it decodes
        y = bytearray(b1)
        k = int(rng.integers(0, len(y)))
        y[k] ^= 1 << int(rng.integers(0, 8))
        d1, d2 = O.decode(bytes(y)), P.decode(bytes(y))
        assert (d1[0] == 0) == (d2[0] == 0), ("status", shape, k)
        if d1[0] == 0:
            assert np.array_equal(d1[1].view(np.uint8), d2[1].view(np.uint8)), ("damaged", shape, k)
print("decoder ok")
""" % (capi.ROOT,)
    env = dict(os.environ, LERC_AMD_DECODE_LAUNCHES=launches, LERC_AMD_TEST_GIVEUP=giveup)
    out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert out.returncode == 0 and b"decoder ok" in out.stdout, out.stdout.decode()[-2000:]


def test_device_mask_rle():
    """the run-length coding of validity bits on the device (rle_kernels.hip), against RLE::compress said plainly: the cases of
    the emulator suite, on device memory"""
    import torch
    import test_sim_kernels as tsk
    from lerc_amd import api
    dev = torch.device("cuda:0")
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    L = codec.lib
    L.lerc_amd_mask_rle_device.restype = ct.c_uint
    L.lerc_amd_mask_rle_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_void_p, ct.c_uint, ct.POINTER(ct.c_uint)]
    rng = np.random.default_rng(9)
    for k, b in enumerate(tsk.rle_cases(rng)):
        n = len(b)
        want = tsk._rle_restated(bytes(b))
        src = torch.zeros(max(n, 16) + 16, dtype=torch.uint8, device=dev)
        src[:n] = torch.from_numpy(b).to(dev)
        out = torch.zeros(len(want) + 64, dtype=torch.uint8, device=dev)
        size = ct.c_uint(0)
        rc = L.lerc_amd_mask_rle_device(codec.h, src.data_ptr(), n, out.data_ptr(), out.numel(), ct.byref(size))
        assert rc == 0 and out[:size.value].cpu().numpy().tobytes() == want, (k, n, rc, size.value, len(want))


def test_try_raise_with_a_mask(P, O):
    """the emulator suite's cases -- TryRaiseMaxZError with a mask, first rows that promise more than the band keeps, NaNs under
    and beside the mask -- byte for byte against the oracle"""
    import test_sim_kernels as tsk
    rng = np.random.default_rng(33)
    for name, x, e, m in tsk.mask_and_stats_cases(rng):
        r1, b1 = O.encode(x, e, mask=m)
        r2, b2 = P.encode(x, e, mask=m)
        assert r1 == r2 and b1 == b2, name
        if r1 == 0:
            d1, d2 = O.decode(b1), P.decode(b1)
            assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1]) and _same(d1[2], d2[2]), name


@pytest.mark.parametrize("knob", ["0", "8", "16"])
def test_block_offsets_by_four_lanes_a_chunk(knob):
    """k_walk_emit_sub on the device: the emulator suite's rasters (masked and ragged, every data type) with the landings
    trusted, distrusted (8) and made wrong by a byte (16) -- same pixels, same verdict on a damaged copy"""
    import sys
    import test_sim_kernels as tsk
    env = dict(os.environ, LERC_AMD_TEST_GIVEUP=knob)
    out = subprocess.run([sys.executable, "-c", tsk.four_lanes_code("product")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0 and b"offsets ok" in out.stdout, out.stdout.decode()[-2000:]


def test_device_mask_rle_decode():
    """the way back (rle_kernels.hip: hops by pointer doubling, a chain over the pieces, a wave per 256 bytes of stream) against
    RLE::decompress said plainly: the cases of the emulator suite incl. the damaged streams, on device memory"""
    import torch
    import test_sim_kernels as tsk
    from lerc_amd import api
    dev = torch.device("cuda:0")
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    L = codec.lib

    def run(stream, n_out):
        src = torch.zeros(len(stream) + 16, dtype=torch.uint8, device=dev)
        src[:len(stream)] = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to(dev)
        out = torch.full((n_out + 64,), 0xA5, dtype=torch.uint8, device=dev)
        rc = L.lerc_amd_mask_rle_decode_device(codec.h, src.data_ptr(), len(stream), out.data_ptr(), n_out)
        got = out.cpu().numpy()
        assert (got[n_out:] == 0xA5).all()
        return rc, got[:n_out].tobytes()
    tsk.check_device_rle_decode(L, codec.h, run)


def test_small_blobs_decode_in_one_launch_every_time():
    """A blob of a few workgroups, decoded again and again: the launch's last workgroup is through microseconds after the
    first one has left the band's parameters for the host -- the verdict on the checksum must not be overtaken by them
    (one writer per byte; it was, once: every decode but the first came back through the two-launch form, silently).  The
    kernels that ran say which form served the calls."""
    import torch
    from lerc_amd import api, synth
    dev = torch.device("cuda:0")
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    L = codec.lib
    L.lerc_amd_profile_enable.argtypes = [ct.c_void_p, ct.c_int]
    L.lerc_amd_profile_read.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int]
    for n in (64, 256, 600, 1024):
        x = synth.c2_float32(n, n, device=dev)
        blob = torch.empty(x.numel() * 4 + 4096, dtype=torch.uint8, device=dev)
        y = torch.empty_like(x)
        rc, nb = api.encode_device(codec, x, 0.01, blob)
        assert rc == 0
        L.lerc_amd_profile_enable(codec.h, 1)
        for rep in range(8):
            assert api.decode_device(codec, blob, nb, y) == 0
        L.lerc_amd_profile_enable(codec.h, 0)
        buf = ct.create_string_buffer(1 << 14)
        L.lerc_amd_profile_read(codec.h, buf, len(buf), 1)
        launches = {ln.split()[0]: int(ln.split()[2]) for ln in buf.value.decode().splitlines()}
        assert launches in ({"fast_decode_scan": 8}, {"fast_decode_one": 8}), (n, launches)    # (one launch a call, and the same form every time)
        assert float((y.double() - x.double()).abs().max().item()) <= 0.01 * (1 + 1e-6) + 6.2e-5


def test_host_threads_call_the_stock_api_at_the_same_time(P, O):
    """The reference's contract (Lerc.cpp:448, :640; Lerc_c_api.h:113): no global state, concurrent calls on different buffers
    are fine.  Eight host threads call lerc_encode / lerc_decode at once -- every data type, a masked raster among them, every
    thread its own context inside the library -- and each gets the oracle's bytes and pixels, again and again."""
    import threading
    rng = np.random.default_rng(77)
    jobs = []
    for k, (dt, e, shape) in enumerate(((np.float32, 0.01, (1024, 1536)), (np.uint16, 0, (1024, 1024)), (np.int32, 0, (777, 1001)),
                                        (np.float64, 0.001, (512, 768)), (np.uint8, 0, (768, 1024)), (np.int16, 0.5, (640, 640)),
                                        (np.float32, 0.1, (1000, 1000)), (np.uint32, 0, (512, 2048)))):
        x = cases._cast(cases.terrain(shape[0], shape[1], rng, amp=300, base=1000, sigma=2.0), dt)
        m = None
        if k == 6:    # a mask with a hole and ragged edges
            m = np.ones(shape, np.uint8)
            m[100:300, 200:700] = 0
            m[::7, ::13] = 0
        r, blob = O.encode(x, e, mask=m)
        assert r == 0
        jobs.append((x, e, m, blob, O.decode(blob)))
    errors = []

    def work(k):
        x, e, m, blob, want = jobs[k]
        try:
            for rep in range(6):
                r, b = P.encode(x, e, mask=m)
                assert r == 0 and b == blob, ("blob", k, rep)
                d = P.decode(blob)
                assert d[0] == 0 and _same(d[1], want[1]) and _same(d[2], want[2]), ("pixels", k, rep)
        except BaseException as ex:    # noqa: BLE001 -- reported by the main thread
            errors.append(repr(ex))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(600)
    assert not errors and not any(t.is_alive() for t in threads), errors[:3]


def test_two_codecs_on_two_streams_at_the_same_time(O):
    """Two DeviceCodec contexts on two HIP streams, their one-launch encoders and decoders in flight together: the hand-offs
    inside a launch (size cells, block-count cells, checksum accumulators) are per context, and a workgroup that waits for
    a cell waits for a workgroup of its OWN launch -- which the other launch's workgroups may delay but not starve.  Bytes
    are the oracle's, pixels within the bound, and no call came back through the general kernels."""
    import torch
    from lerc_amd import api, synth
    dev = torch.device("cuda:0")
    xs = [synth.c2_float32(4096, 4096, row0=4096 * k, device=dev) for k in range(2)]
    want = []
    for x in xs:
        r, b = O.encode(x.cpu().numpy(), 0.01)
        assert r == 0
        want.append(b)
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    codecs = [api.DeviceCodec(st.cuda_stream) for st in streams]
    blobs = [torch.empty(x.numel() * 4 + 4096, dtype=torch.uint8, device=dev) for x in xs]
    outs = [torch.empty_like(x) for x in xs]
    torch.cuda.synchronize()
    tickets = [[], []]
    for rep in range(12):
        for k in range(2):
            rc, t1 = api.encode_device_async(codecs[k], xs[k], 0.01, blobs[k])
            rc2, t2 = api.decode_device_async(codecs[k], blobs[k], blobs[k].numel(), outs[k])
            assert rc == 0 and rc2 == 0, (rc, rc2, codecs[k].last_error())
            tickets[k].append((t1, t2))
        if rep % 4 == 3:
            for k in range(2):
                for t1, t2 in tickets[k]:
                    rc, nb = codecs[k].finish(t1)
                    rc2, _ = codecs[k].finish(t2)
                    assert rc == 0 and rc2 == 0 and nb == len(want[k]), (rc, rc2, nb, len(want[k]), codecs[k].last_error())
                tickets[k] = []
    torch.cuda.synchronize()
    for k in range(2):
        assert blobs[k][:len(want[k])].cpu().numpy().tobytes() == want[k], ("blob", k)
        assert float((outs[k].double() - xs[k].double()).abs().max().item()) <= 0.01 * (1 + 1e-6) + 6.2e-5
        c = codecs[k].path_counters()
        assert c[0] == 12 and c[2] == 12 and c[1] == 0 and c[3] == 0, (k, c, codecs[k].last_note() if hasattr(codecs[k], "last_note") else "")


def test_lerc1_world(P, O):
    """the reference's legacy Lerc1 fixture (decode only): info, ranges, pixels, mask -- and damaged copies"""
    blob = open(os.path.join(GOLD, "world.lerc1"), "rb").read()
    assert P.blob_info(blob) == O.blob_info(blob) == (0, [0, 6, 1, 257, 257, 1, 65025, 63518, 1, 1, 0], [-27.458635330200195, 5474.1728515625, 0.1])
    assert P.data_ranges(blob, 1, 1) == O.data_ranges(blob, 1, 1)
    for kw in ({}, {"to_double": True}):
        d1, d2 = O.decode(blob, **kw), P.decode(blob, **kw)
        assert d1[0] == d2[0] == 0 and _same(d1[1], d2[1]) and _same(d1[2], d2[2])
    m = d2[2].reshape(257, 257).astype(bool)
    assert sha(P.decode(blob)[1].reshape(257, 257)[m].tobytes()) == "74f626d1a4fcf78f1eae5b7cb07f7690a8a0bf76d5d77315b3737a2bae5aae09"
    rng = np.random.default_rng(3)
    for t in range(150):
        x = bytearray(blob)
        k = int(rng.integers(0, len(x)))
        x[k] ^= 1 << int(rng.integers(0, 8))
        if t % 4 == 0:
            x = x[:max(40, k)]
        x = bytes(x)
        g1, g2 = O.decode(x), P.decode(x)
        assert (g1[0] == 0) == (g2[0] == 0), (t, k)
        if g1[0] == 0:
            assert _same(g1[1], g2[1]) and _same(g1[2], g2[2]), (t, k)


def test_lerc1_written_blobs(P, O):
    """Lerc1 blobs of tests/lerc1_writer.py: info, ranges, pixels and masks as the oracle's"""
    for name, blob, nb in cases.lerc1_cases():
        cases.check_lerc1_case(O, P, name, blob, nb, _same)


def test_reference_test_driver_runs_against_the_product():
    """The reference's own caller, src/LercTest/main.cpp, compiled from where it lies (`make -C oracle reftest`, test
    infrastructure under oracle/_ref/) and linked against liblerc_amd.so under the reference's soname libLerc.so.4: its
    encode / decode / getBlobInfo sequences check themselves, the exit code is the number of failed checks != 0."""
    exe = os.path.join(capi.ROOT, "oracle", "_ref", "LercTest_amd")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/LercTest_amd not built (needs /root/reference at build time)")
    csrc = os.path.join(capi.ROOT, "lerc_amd", "csrc")
    link = os.path.join(csrc, "libLerc.so.4")
    if not os.path.exists(link):
        os.symlink("liblerc_amd.so", link)
    out = subprocess.run([exe], cwd=capi.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    tail = out.stdout.decode(errors="replace")[-2000:]
    assert out.returncode == 0, tail
    assert "failed" not in tail.lower(), tail


def test_mask_bytes_of_an_all_valid_band(P, O):
    """lerc_decode with nMasks >= 1 on a blob that stores no mask (all pixels valid): the caller's mask bytes become 1s on
    every path (Lerc.cpp:464-488), including the streaming kernels (the harness pre-fills the mask with 0xCD)."""
    rng = np.random.default_rng(41)
    for shape, n_bands in (((64, 1024), 1), ((2, 40, 520), 2), ((33, 47), 1)):
        arr = cases.terrain(*shape[-2:], rng).astype(np.float32)
        if n_bands > 1:
            arr = np.stack([arr + i for i in range(n_bands)])
        rc, blob = O.encode(arr, 0.01, n_bands=n_bands)
        assert rc == 0
        for want in (1, n_bands):
            rc, dec, mask = P.decode(blob, want_masks=want, n_bands=n_bands)
            assert rc == 0 and mask is not None and mask.shape[0] == want
            assert (mask == 1).all(), (shape, want, np.unique(mask))
            want_dec = O.decode(blob)[1]
            assert _same(dec, want_dec)


def test_c4_full_size_4096_rgb_uint8_huffman(P, O):
    """BASELINE configs[3] at full size: 4096 x 4096 x 3 bytes, lossless -> 8-bit Huffman mode.  Blob == oracle blob,
    decode == input (the self-synchronising Huffman decoder and the multi-level scans depend on the size)."""
    from lerc_amd import synth
    x = synth.c4_rgb_u8().numpy() if hasattr(synth, "c4_rgb_u8") else None
    if x is None:
        pytest.skip("synth.c4_rgb_u8 missing")
    rc, blob = P.encode(x, 0, n_depth=3)
    assert rc == 0
    rc_o, blob_o = O.encode(x, 0, n_depth=3)
    assert rc_o == 0 and len(blob) == len(blob_o) and sha(blob) == sha(blob_o)
    rc, dec, _ = P.decode(blob)
    assert rc == 0 and np.array_equal(dec.reshape(x.shape), x)


def test_huffman_long_codes_and_many_subsequences(P, O):
    """The cases of tests/test_sim_kernels.py's Huffman stress test at four times the edge length, on the device."""
    for name, arr, kw in cases.huffman_stress_cases(scale=4):
        rc, blob = P.encode(arr, 0, **kw)
        rc_o, blob_o = O.encode(arr, 0, **kw)
        assert rc == rc_o == 0 and blob == blob_o, name
        rc, dec, _ = P.decode(blob)
        assert rc == 0 and np.array_equal(dec.reshape(arr.shape), arr), name


def test_byte_rasters_priced_by_the_lane_per_block_kernel(P, O):
    for name, arr, kw in cases.byte_tiling_cases():
        rc, blob = P.encode(arr, 0, **kw)
        rc_o, blob_o = O.encode(arr, 0, **kw)
        assert rc == rc_o == 0 and blob == blob_o, name
        rc, dec, _ = P.decode(blob)
        assert rc == 0 and np.array_equal(dec.reshape(arr.shape), arr), name


def test_queued_device_calls(O):
    """lerc_amd_encode_device_async / lerc_amd_decode_device_async / lerc_amd_finish on device tensors: operations queue up
    on the stream; a decode enqueued right behind the encode that writes its blob gets the buffer's capacity as size bound
    (the grids are sized for that, the stream's true end is read from the header on the device); what the device hands
    back to the general path (a constant raster) is repeated at finish time."""
    import torch
    from lerc_amd import api
    dev = torch.device("cuda:0")
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(8)
    try:
        rasters = [cases.terrain(1024, 2048, rng, amp=300, base=1000, sigma=1.5).astype(np.float32),
                   np.full((64, 512), 3.5, np.float32),                                           # constant: the device says "redo"
                   cases.terrain(264, 1000, rng, amp=300, base=1000, sigma=1.5).astype(np.int32),
                   cases.terrain(2048, 4096, rng, amp=50, base=100, sigma=0.3).astype(np.float32)]
        errs = [0.01, 0.01, 0, 0.001]
        keep, tickets = [], []
        for arr, e in zip(rasters, errs):
            x = torch.from_numpy(arr).to(dev)
            blob = torch.empty(arr.nbytes + 4096, dtype=torch.uint8, device=dev)
            y = torch.empty_like(x)
            rc, t1 = api.encode_device_async(codec, x, e, blob)
            assert rc == 0 and t1
            rc, t2 = api.decode_device_async(codec, blob, blob.numel(), y)
            assert rc == 0 and t2
            keep.append((x, blob, y))
            tickets.append((t1, t2))
        for arr, e, (x, blob, y), (t1, t2) in zip(rasters, errs, keep, tickets):
            rc, n = codec.finish(t1)
            assert rc == 0
            r0, b0 = O.encode(arr, e)
            assert r0 == 0 and blob[:n].cpu().numpy().tobytes() == b0, arr.shape
            rc, _ = codec.finish(t2)
            assert rc == 0
            assert _same(O.decode(b0)[1].reshape(arr.shape), y.cpu().numpy()), arr.shape
    finally:
        codec.close()


def test_queued_verdicts_are_judged_against_their_own_launch(O):
    """tests/test_sim_kernels.py: test_sim_queued_verdicts_are_judged_against_their_own_launch on the device, the same rasters: a band
    whose launch was sized by a smaller band of its shape and, in flight behind it, a band of another shape with a larger launch.  The
    first is judged against its own launch: the size guess is forgotten (one launch thrown away), the shape stays on the scanning
    decoder."""
    import torch
    from lerc_amd import api
    dev = torch.device("cuda:0")
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    keep = []

    def queue(arr, b0, bound=None):
        blob = torch.zeros(arr.nbytes + 4096, dtype=torch.uint8, device=dev)
        blob[:len(b0)] = torch.frombuffer(bytearray(b0), dtype=torch.uint8).to(dev)
        y = torch.empty(arr.shape, dtype=torch.float32, device=dev)
        rc, t = api.decode_device_async(codec, blob, bound or blob.numel(), y)
        assert rc == 0 and t
        keep.append((blob, y))
        return t, y

    try:
        (smooth, bs), (noisy, bn), (other, bo) = cases.queued_bands_of_two_shapes(O)
        t1, y1 = queue(smooth, bs)
        assert codec.finish(t1)[0] == 0                                   # the size guess for the shape is now small
        q0 = codec.decode_refusals()
        t2, y2 = queue(noisy, bn)                                         # sized by the small guess: too few pieces
        t3, y3 = queue(other, bo, len(bo))                                # another shape, a larger launch: in flight behind it
        assert codec.finish(t2)[0] == 0 and codec.finish(t3)[0] == 0
        f1, q1 = codec.decode_forms(), codec.decode_refusals()
        for arr, b0, y in ((smooth, bs, y1), (noisy, bn, y2), (other, bo, y3)):
            assert _same(O.decode(b0)[1].reshape(arr.shape), y.cpu().numpy()), arr.shape
        assert q1[2] == q0[2] + 1, (q0, q1, codec.last_note())
        t4, y4 = queue(noisy, bn)
        assert codec.finish(t4)[0] == 0
        f2, q2 = codec.decode_forms(), codec.decode_refusals()
        assert _same(O.decode(bn)[1].reshape(noisy.shape), y4.cpu().numpy())
        assert f2[3] == f1[3] + 1 and f2[2] == f1[2] and list(q2) == list(q1), ("the scanning decoder did not serve the shape", f1, f2, q1, q2, codec.last_note())
    finally:
        codec.close()


def test_random_sizes_stay_on_the_streaming_kernels():
    """tools/fallback_hunt.py in the suite: a few thousand round trips of rasters of random sizes (rows / columns multiples of 8 and
    not; float32 and int32) on a fresh context and on a warm one.  Synthetic terrain has nothing that sends a band elsewhere: every
    call is served by the streaming kernels -- the hand-offs inside the launches (block counts, span sizes, checksum terms, first-row
    errors) arrive every time, or the note of the call that went another way is printed.  (LERC_AMD_TEST_SHARED_GPU=1: two such
    calls are let pass -- a hand-off that times out under other processes' load falls back by design.)"""
    import time
    import torch
    from lerc_amd import api, synth
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20260928)
    big = synth.c2_float32(2048, 2304, device=dev)
    warm = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    n = 0
    odd = []
    # a batch of 96 tiles of 256 x 256 through the batched calls (a tile per blockIdx.y: every tile's hand-offs in cells of its own), on
    # warm and fresh contexts: one streaming pass each way, no tile elsewhere
    tiles = torch.stack([big[(k // 8) * 128: (k // 8) * 128 + 256, (k % 8) * 256: (k % 8) * 256 + 256] for k in range(96)]).contiguous()
    arena = torch.empty(96 * (256 * 256 * 4 + 4096), dtype=torch.uint8, device=dev)
    tiles_out = torch.empty_like(tiles)

    def batch_round_trip(codec):
        c0, f0 = codec.path_counters(), codec.decode_forms()
        rc, offsets, sizes, used = api.encode_tiles_device(codec, tiles, 0.01, arena)
        assert rc == 0 and used <= arena.numel() and int(sizes.min()) > 70, (rc, codec.last_error())
        rc = api.decode_tiles_device(codec, arena, offsets, sizes, tiles_out)
        c1, f1 = codec.path_counters(), codec.decode_forms()
        assert rc == 0, (rc, codec.last_error())
        assert float((tiles_out.double() - tiles.double()).abs().max()) <= 0.01 * (1 + 1e-6) + 6.2e-5
        if c1[1] != c0[1] or c1[3] != c0[3] or f1[3] != f0[3] + 96:
            odd.append(("96 tiles", [int(b - a) for a, b in zip(c0, c1)], [int(b - a) for a, b in zip(f0, f1)], codec.last_note(), codec.last_error()))

    t0 = time.time()
    while n < 3000 and time.time() - t0 < 150:
        r, c = int(rng.integers(32, 2048)), int(rng.integers(64, 2304))
        if rng.random() < 0.6:
            r -= r % 8
            c -= c % 8
        x = big[:r, :c].contiguous()
        e = 0.01
        kind = rng.random()
        if kind < 0.25:
            x = (x * 8).to(torch.int32).contiguous()
            e = 0
        elif kind < 0.5 and hasattr(torch, "uint16"):
            # (16-bit data: three units a workgroup in the encoder, four times the blocks per byte in the decoder -- the C3 shape's protocols)
            x = (x * 8).to(torch.int32).to(torch.uint16).contiguous()
            e = 0
        if n % 100 == 0:
            batch_round_trip(warm)
            fresh_batch = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
            batch_round_trip(fresh_batch)
            fresh_batch.close()
        blob = torch.empty(x.numel() * x.element_size() + 8192, dtype=torch.uint8, device=dev)
        y = torch.empty_like(x)
        for fresh in (True, False):
            codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream) if fresh else warm
            c0, f0 = codec.path_counters(), codec.decode_forms()
            rc, nb = api.encode_device(codec, x, e, blob)
            rc2 = api.decode_device(codec, blob, nb, y)
            c1, f1 = codec.path_counters(), codec.decode_forms()
            n += 1
            assert rc == 0 and rc2 == 0, (tuple(x.shape), x.dtype, rc, rc2, codec.last_error())
            whole = r % 8 == 0 and c % 8 == 0
            if c1[1] != c0[1] or c1[3] != c0[3] or (whole and f1[3] != f0[3] + 1):
                odd.append((tuple(x.shape), str(x.dtype), "fresh" if fresh else "warm", [int(b - a) for a, b in zip(c0, c1)],
                            [int(b - a) for a, b in zip(f0, f1)], codec.last_note(), codec.last_error()))
            if fresh:
                codec.close()
        if n % 64 == 0:    # (the pixels, now and then: the counters say who served the call, not what it wrote)
            d = (y.to(torch.int32) - x.to(torch.int32)).abs().max().item() if x.dtype == getattr(torch, "uint16", None) else (y.double() - x.double()).abs().max().item()
            assert d <= e * (1 + 1e-6) + (6.2e-5 if e else 0), (tuple(x.shape), d)
    assert len(odd) <= (2 if os.environ.get("LERC_AMD_TEST_SHARED_GPU") else 0), (n, odd[:6])


def test_damaged_mask_in_front_of_the_huffman_kernels(P, O):
    """A byte raster with a mask, coded in the 8-bit Huffman mode, with damaged mask sections: the Huffman kernels take the mask's word
    for the number of valid pixels, so a mask that is not what the header says is refused before they run (it once divided a rank by a
    valid count of zero -- found on the emulator; this is the same on hardware, the mask decoded on the host and on the device)."""
    rng = np.random.default_rng(31)
    r, c = 600, 1000
    x = cases._cast(cases.terrain(r, c, rng, amp=40, base=100, sigma=1.0), np.uint8)
    m = np.ones((r, c), np.uint8)
    m[100:300, 200:900] = 0
    m[rng.random((r, c)) < 0.02] = 0
    rc, blob = O.encode(x, 0, mask=m)
    assert rc == 0
    info = O.blob_info(blob)
    assert info[0] == 0
    d0 = O.decode(blob)
    assert d0[0] == 0
    code = r"""
import sys, os
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, capi
P, O = capi.product(), capi.oracle()
blob = open(sys.argv[1], "rb").read()
rng = np.random.default_rng(5)
hdr = 90 + 4
n_mask = int.from_bytes(blob[90:94], "little")
assert n_mask > 16
bad = 0
for t in range(48):
    x = bytearray(blob)
    k = hdr + int(rng.integers(0, n_mask))
    x[k] ^= 1 << int(rng.integers(0, 8))
    if t %% 6 == 0: x[k:k + 2] = b"\x00\x80"      # an end marker in the middle of the stream
    x = bytes(x)
    g1, g2 = O.decode(x), P.decode(x)
    assert (g1[0] == 0) == (g2[0] == 0), (t, k, g1[0], g2[0])
    bad += int(g1[0] != 0)
g1, g2 = O.decode(blob), P.decode(blob)
assert g1[0] == g2[0] == 0 and np.array_equal(g1[2], g2[2]) and np.array_equal(g1[1][g1[2] != 0], g2[1][g2[2] != 0])
print("masks ok", bad)
""" % (capi.ROOT,)
    import subprocess
    import sys
    import tempfile
    with tempfile.NamedTemporaryFile(suffix=".lerc2", delete=False) as f:
        f.write(blob)
        path = f.name
    try:
        for knob in ("16", "0"):
            env = dict(os.environ, LERC_AMD_DEVICE_RLE=knob)
            out = subprocess.run([sys.executable, "-c", code, path], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
            assert out.returncode == 0 and b"masks ok" in out.stdout, out.stdout.decode()[-2000:]
    finally:
        os.unlink(path)


def test_header_and_mask_disagree_on_the_valid_count(P, O):
    """Crafted blobs with a valid checksum whose header names another number of valid pixels than the mask holds, the one-sweep stream cut
    to the header's count among them (round-5 review: the kernel, which reads by the mask's ranks, read past the blob through the
    device-pointer API).  Verdicts and pixels are the oracle's and the real reference's; the same script runs under the emulator in
    tests/test_sim_kernels.py.  Mask decoded on the host and (LERC_AMD_DEVICE_RLE=16) on the device."""
    import sys
    from test_sim_kernels import COUNT_MISMATCH_CODE
    for knob in ("0", "16"):
        env = dict(os.environ, LERC_AMD_DEVICE_RLE=knob)
        out = subprocess.run([sys.executable, "-c", COUNT_MISMATCH_CODE % (capi.ROOT, "product")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert out.returncode == 0 and b"counts ok" in out.stdout, out.stdout.decode()[-2000:]


def test_blob_gather_over_rccl_in_a_group_of_one(O):
    """The mosaic job's exchange step (lerc_amd/shard.py: gather_arenas_start) on the GPU box: a process group of ONE rank over
    "nccl" -- RCCL -- with the collective steps forced (there is nobody to send to, but the lengths' all-gather runs on RCCL with
    device tensors, the collective's stream is ordered behind the codec's by an event, and the root's own copy and the tables move
    between HBM slices).  What several ranks do differently -- the grouped send / receive batch -- is covered by the gloo tests
    (tests/test_shard_gloo.py); this one shows that RCCL loads and runs here and that the device-side half is in order: the
    mosaic it leaves decodes to the tiles.  (A process of its own: the process group is global state.)"""
    import sys
    code = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np, torch, torch.distributed as dist
from lerc_amd import api, shard, synth
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29531", rank=0, world_size=1, device_id=dev)
assert dist.get_backend() == "nccl"
side = torch.cuda.Stream()
with torch.cuda.stream(side):                         # the codec on a stream of its own: the gather has to be told
    codec = api.DeviceCodec(side.cuda_stream)
    tiles = torch.stack([synth.c5_tile(3, k, device=dev) for k in range(24)])
    arena = torch.empty(tiles.numel() * 4 + (1 << 16), dtype=torch.uint8, device=dev)
    rc, offs, sizes, used = api.encode_tiles_device(codec, tiles, 0.01, arena)
    assert rc == 0
    done = torch.cuda.Event()
    done.record(side)
# the torch.distributed form (what the gloo tests run), then the exchange BELOW Python: lerc_amd_gather_blobs on a communicator made
# with ncclGetUniqueId / ncclCommInitRank through the same librccl -- a message a rank, the per-tile table in front of the arena
os.environ["LERC_AMD_GATHER"] = "torch"
flight = shard.gather_arenas_start(arena, used, offs, sizes, root=0, after=done, force_collective=True)
mosaic, t_off, t_size, bases = flight.finish()
torch.cuda.synchronize()
assert bases == [0] and int(mosaic.numel()) >= int(used)
assert torch.equal(mosaic[:int(used)], arena[:int(used)])
assert [int(v) for v in t_off] == [int(v) for v in offs] and [int(v) for v in t_size] == [int(v) for v in sizes]
os.environ["LERC_AMD_GATHER"] = "c"
need = 16 + 16 * 24
for with_room in (False, True):
    if with_room:      # the arena with room in front of it: the message leaves as it lies
        with torch.cuda.stream(side):
            buf = torch.empty(need + arena.numel(), dtype=torch.uint8, device=dev)
            arena2 = buf[need:]
            rc, offs2, sizes2, used2 = api.encode_tiles_device(codec, tiles, 0.01, arena2)
            assert rc == 0 and used2 == used
            done.record(side)
        flight = shard.gather_arenas_start(arena2, used2, offs2, sizes2, root=0, after=done, force_collective=True, codec=codec, front=buf)
    else:
        flight = shard.gather_arenas_start(arena, used, offs, sizes, root=0, after=done, force_collective=True)
    mosaic, t_off, t_size, bases = flight.finish()
    assert bases == [need] and int(mosaic.numel()) == ((need + int(used) + 15) & ~15), (bases, mosaic.numel(), used)
    # (a batch's tiles lie in the arena in the order of their claims: another encode, another order -- compare with the arena that travelled)
    src_arena, src_offs, src_sizes = (arena2, offs2, sizes2) if with_room else (arena, offs, sizes)
    assert torch.equal(mosaic[need:need + int(used)], src_arena[:int(used)])
    assert [int(v) - need for v in t_off] == [int(v) for v in src_offs] and [int(v) for v in t_size] == [int(v) for v in src_sizes]
    assert sorted(int(v) for v in src_sizes) == sorted(int(v) for v in sizes)
import ctypes as ct
R = shard.rccl_comm(dev)
n_ranks = ct.c_int(0)
assert R.lib.ncclCommCount(R.comm, ct.byref(n_ranks)) == 0 and n_ranks.value == 1
# a root buffer that is too small is refused with BufferTooSmall (3), a communicator that is none with WrongParam (2)
fn = codec.lib.lerc_amd_gather_blobs
small = torch.empty(64, dtype=torch.uint8, device=dev)
assert fn(codec.h, R.comm, 0, arena.data_ptr(), int(used), small.data_ptr(), 64, None, None, R.stream.cuda_stream) == 3
assert fn(codec.h, None, 0, arena.data_ptr(), int(used), small.data_ptr(), 64, None, None, R.stream.cuda_stream) == 2
torch.cuda.synchronize()
out = torch.empty_like(tiles)
with torch.cuda.stream(side):
    side.wait_stream(torch.cuda.current_stream())
    rc = api.decode_tiles_device(codec, mosaic, t_off.numpy().astype(np.uint64), t_size.numpy().astype(np.uint32), out)
    assert rc == 0
torch.cuda.synchronize()
assert float((out.double() - tiles.double()).abs().max().item()) <= 0.01 + 6.2e-5
t = shard.max_over_ranks(1.25, device=dev)
assert t == 1.25
dist.destroy_process_group()
print("rccl ok")
""" % (capi.ROOT,)
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0 and b"rccl ok" in out.stdout, out.stdout.decode()[-3000:]
