"""One call through every per-band stage of the general band path (BandEncoder, CallDecoder): six bands with a mask plane each --
a masked band in tiling mode, the same mask again ("use the previous mask"), another mask over noise (one sweep), a band with every
pixel valid, a band with none, a constant band -- at the smallest shape with interior blocks, edge blocks and a second block row.
uint16 with nDepth 2, and uint8 lossless with nDepth 1 (the masked Huffman plan and the mask-count wait in front of it)."""
import struct

import numpy as np
import pytest
import torch

import capi
from lerc_amd import synth

ROWS, COLS, BANDS = 37, 70, 6


def _raster(dtype, n_depth, seed=4242):
    i, j, idx = synth._grid(ROWS, COLS, 0, 0, COLS, "cpu")
    noise = lambda k: synth._hash32(idx + (seed + k) * 0x10001)
    smooth = lambda k: torch.stack([synth.c3_uint16(ROWS, COLS, seed=seed + 10 * k + d).to(torch.int64) for d in range(n_depth)], -1)
    small = np.dtype(dtype).itemsize == 1
    bands = []
    for b in range(BANDS):
        if b == 2:    # noise: one sweep
            v = torch.stack([noise(50 + d) & (0xFF if small else 0xFFFF) for d in range(n_depth)], -1)
        elif b == 5:
            v = torch.full((ROWS, COLS, n_depth), 77, dtype=torch.int64)
        else:
            v = smooth(b) // 16 if small else smooth(b)
        bands.append(v)
    x = torch.stack(bands).numpy().astype(dtype)
    x = x if n_depth > 1 else x[..., 0]
    m0 = (noise(1) % 10 >= 3).numpy().astype(np.uint8)    # about 30 % invalid
    m2 = (noise(2) % 10 >= 4).numpy().astype(np.uint8)
    masks = np.stack([m0, m0, m2, np.ones_like(m0), np.zeros_like(m0), m2])
    return np.ascontiguousarray(x), np.ascontiguousarray(masks)


def _band_modes(blob, n_depth, item):
    """per band of a codec-6 blob: (mask bytes, 'empty' | 'const' | 'sweep' | 'blocks' | 'huffman'); 8-bit lossless bands carry an
    image-mode byte behind the one-sweep flag: 0 blocks, 1 DeltaHuffman, 2 Huffman"""
    out, at = [], 0
    while at < len(blob):
        assert blob[at:at + 6] == b"Lerc2 " and struct.unpack_from("<i", blob, at + 6)[0] == 6
        num_valid, _, size = struct.unpack_from("<3i", blob, at + 26)
        z_min, z_max = struct.unpack_from("<2d", blob, at + 58)
        n_mask = struct.unpack_from("<i", blob, at + 90)[0]
        p = at + 94 + n_mask
        if num_valid == 0:
            mode = "empty"
        elif z_min == z_max:
            mode = "const"
        else:
            p += 2 * n_depth * item
            mode = "sweep" if blob[p] == 1 else "blocks"
            if mode == "blocks" and item == 1:
                assert blob[p + 1] in (0, 1, 2)
                mode = "huffman" if blob[p + 1] else "blocks"
        out.append((n_mask, mode))
        at += size
    return out


_PARAMS = [pytest.param(np.uint16, 2, id="uint16-depth2"), pytest.param(np.uint8, 1, id="uint8-lossless")]


# (The masks here are 324 bytes, below the size from which a mask is decoded on the device: the decoder counts them on the host.  The
# device-side count in front of the one-sweep and Huffman kernels is crossed by test_sim_several_bands_with_a_mask_each_decoded_on_the_device.)
def _check(lib, dtype, n_depth):
    R = capi.ref() or capi.oracle()
    x, m = _raster(dtype, n_depth)
    kw = dict(n_depth=n_depth, n_bands=BANDS, mask=m)
    rc_r, blob_r = R.encode(x, 0, **kw)
    assert rc_r == 0
    # the reference itself must take the paths this test is about
    modes = _band_modes(blob_r, n_depth, np.dtype(dtype).itemsize)
    coded = "huffman" if np.dtype(dtype).itemsize == 1 else "blocks"    # (8-bit lossless: the Huffman plan over valid pixels must win)
    assert [k for _, k in modes] == [coded, coded, "sweep", coded, "empty", "const"], modes
    assert modes[0][0] > 0 and modes[1][0] == 0 and modes[2][0] > 0 and modes[5][0] > 0, modes    # band 1: "use the previous mask"
    rc, blob = lib.encode(x, 0, **kw)
    assert rc == 0 and blob == blob_r, "blob differs from the reference"
    assert lib.compute_size(x, 0, **kw) == (0, len(blob_r))
    d_r, d = R.decode(blob_r, want_masks=BANDS, n_bands=BANDS), lib.decode(blob_r, want_masks=BANDS, n_bands=BANDS)
    assert d_r[0] == d[0] == 0
    assert np.array_equal(d_r[2], d[2]) and np.array_equal(d[2].reshape(m.shape), m)
    assert np.array_equal(d_r[1], d[1])


@pytest.mark.parametrize("dtype,n_depth", _PARAMS)
def test_sim_every_band_stage(dtype, n_depth):
    S = capi.sim()
    assert S is not None, "tests/_sim/liblerc_amd_sim.so missing -- run __graft_entry__.build()"
    _check(S, dtype, n_depth)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n_depth", _PARAMS)
def test_gpu_every_band_stage(dtype, n_depth):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    P = capi.product()
    assert P is not None, "lerc_amd/csrc/liblerc_amd.so missing -- run __graft_entry__.build()"
    _check(P, dtype, n_depth)
