"""Depth rasters in any layout, windows and tile ranges (the four calls of include/lerc_amd_depth.h that take a depthPitch) on the
MI355X (raster_depth_layouts_common.py), and lerc_amd.api's functions over them on torch views."""
import numpy as np
import pytest

import capi
import raster_depth_layouts_common as C

pytestmark = [pytest.mark.gpu, pytest.mark.ref]


def _libs():
    import torch    # (before the library is loaded: both then share one HIP runtime)
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    P, R = capi.product(), capi.ref()
    assert P is not None, "lerc_amd/csrc/liblerc_amd.so is not built"
    assert R is not None, "oracle/_ref/libLercRef.so did not travel"
    return P, R


@pytest.fixture()
def batch():
    P, _ = _libs()
    B = C.DepthLayouts(P.lib, C.D.GpuMem())
    yield B
    B.close()


@pytest.mark.parametrize("dtype,e,c,lay,with_mask,slotted", C.PARITY, ids=C.PARITY_IDS)
def test_parity_both_ways(batch, dtype, e, c, lay, with_mask, slotted):
    """37 x 45 x C, tiles of 16: four shape classes, ragged last tiles"""
    C.check_parity(batch, _libs()[1], dtype, e, c, lay, with_mask, slotted)


@pytest.mark.parametrize("lay", ["planes", "planes_view", "lines", "gapped"])
@pytest.mark.parametrize("dtype,e,shape", [(np.uint8, 0, (9, 520, 3)), (np.float64, 0.001, (9, 70, 2))], ids=["uint8", "float64"])
def test_rows_longer_than_a_segment(batch, dtype, e, shape, lay):
    """one tile whose rows take two segments of kRtPxSegBytes = 512 bytes an element plane"""
    h, w, c = shape
    C.check_parity(batch, _libs()[1], dtype, e, c, "gapped%d" % (c + 1) if lay == "gapped" else lay, True, False, shape=(h, w), tile=(16, 1024))


@pytest.mark.parametrize("lay", C.layouts_for(3))
@pytest.mark.parametrize("window,n_tiles", C.WINDOWS, ids=["x".join(str(v) for v in w) for w, _ in C.WINDOWS])
def test_window(batch, window, n_tiles, lay):
    C.check_window(batch, _libs()[1], window, n_tiles, lay)


@pytest.mark.parametrize("lay", C.layouts_for(3))
def test_window_with_a_damaged_blob(batch, lay):
    C.check_damaged_blob(batch, _libs()[1], lay)


@pytest.mark.parametrize("lay", C.layouts_for(3))
@pytest.mark.parametrize("rng", C.RANGES, ids=["x".join(str(v) for v in r) for r in C.RANGES])
def test_tile_range(batch, rng, lay):
    C.check_range(batch, _libs()[1], rng, lay)


def test_refused(batch):
    C.check_refused(batch)


def test_header_symbols_are_exported():
    C.check_header(_libs()[0].lib)


def test_python_functions_on_views():
    """lerc_amd.api's four functions on chw.permute(1, 2, 0), rgba[..., :3] and big[a:b, c:d]: no copy, the strides are the pitches"""
    import torch
    from lerc_amd import api
    _, R = _libs()
    Cn = C.content(R, np.float32, 0.01, 3, True)
    h, w, c = Cn.shape
    tile, window, rng = C.TILE, (10, 12, 14, 13), (1, 1, 2, 2)
    ras = torch.from_numpy(np.array(Cn.raster)).cuda()
    valid = torch.from_numpy(np.array(Cn.mask)).cuda()
    chw = ras.permute(2, 0, 1).contiguous()
    rgba = torch.full((h, w, 4), -7.0, dtype=torch.float32, device="cuda")
    rgba[..., :3] = ras
    big = torch.full((h + 6, w + 9, 3), -7.0, dtype=torch.float32, device="cuda")
    big[2:2 + h, 4:4 + w] = ras
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    try:
        n = len(Cn.blobs)
        arena = torch.zeros(n * C.slot_for(tile, c, np.float32), dtype=torch.uint8, device="cuda")

        def blobs_of(offs, sizes, members):
            a = arena.cpu().numpy()
            return {t: a[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() for t in members}

        for name, view in (("chw", chw.permute(1, 2, 0)), ("rgba", rgba[..., :3]), ("big", big[2:2 + h, 4:4 + w])):
            assert tuple(view.shape) == (h, w, c) and (name == "big" or not view.is_contiguous())
            rc, offs, sizes, used = api.encode_raster_tiles_device_depth_strided(codec, view, valid, 0.01, tile, arena)
            assert rc == 0, (name, rc, codec.last_note())
            assert [blobs_of(offs, sizes, range(n))[t] for t in range(n)] == Cn.blobs, name
            members = C.range_tiles(h, w, tile, rng)
            rc, r_offs, r_sizes, used = api.encode_raster_tile_range_device_depth(codec, view, valid, 0.01, tile, rng, arena)
            assert rc == 0 and blobs_of(r_offs, r_sizes, members) == {t: Cn.blobs[t] for t in members}, name
            assert all(int(r_sizes[t]) == 0 for t in range(n) if t not in members)
            # ---- the way back, into a tensor of the same kind
            rc, offs, sizes, used = api.encode_raster_tiles_device_depth_strided(codec, view, valid, 0.01, tile, arena)
            assert rc == 0
            holder = {"chw": torch.full_like(chw, -7.0), "rgba": torch.full_like(rgba, -7.0), "big": torch.full_like(big, -7.0)}[name]
            out = {"chw": lambda t: t.permute(1, 2, 0), "rgba": lambda t: t[..., :3], "big": lambda t: t[2:2 + h, 4:4 + w]}[name](holder)
            valid_out = torch.full_like(valid, 9)
            assert api.decode_raster_tiles_device_depth_strided(codec, arena, offs, sizes, out, valid_out, tile) == 0
            assert C.same_bits(out.cpu().numpy(), Cn.ref_pix) and np.array_equal(valid_out.cpu().numpy(), Cn.ref_valid), name
            rest = holder.clone()
            out_rest = {"chw": lambda t: t.permute(1, 2, 0), "rgba": lambda t: t[..., :3], "big": lambda t: t[2:2 + h, 4:4 + w]}[name](rest)
            out_rest[...] = -7.0
            assert bool((rest == -7.0).all()), "%s: elements beside the view were written" % name
            # ---- a window into a tensor of the same kind
            wh, ww = window[2], window[3]
            if name == "chw":
                w_holder = torch.full((c, wh, ww), -7.0, dtype=torch.float32, device="cuda")
                w_out = w_holder.permute(1, 2, 0)
            elif name == "rgba":
                w_holder = torch.full((wh, ww, 4), -7.0, dtype=torch.float32, device="cuda")
                w_out = w_holder[..., :3]
            else:
                w_holder = torch.full((wh + 3, ww + 5, 3), -7.0, dtype=torch.float32, device="cuda")
                w_out = w_holder[1:1 + wh, 2:2 + ww]
            w_valid = torch.full((wh, ww), 9, dtype=torch.uint8, device="cuda")
            r0 = codec.raster_tiles_counters()
            assert api.decode_raster_window_device_depth(codec, arena, offs, sizes, (h, w), tile, window[:2], w_out, w_valid) == 0
            assert C.delta(r0, codec.raster_tiles_counters()) == [0, 0, len(api.raster_window_tiles(h, w, tile, window)), 0]
            rows, cols = slice(window[0], window[0] + wh), slice(window[1], window[1] + ww)
            assert C.same_bits(w_out.cpu().numpy(), Cn.ref_pix[rows, cols]) and np.array_equal(w_valid.cpu().numpy(), Cn.ref_valid[rows, cols]), name
            if name == "rgba":
                assert bool((w_holder[..., 3] == -7.0).all()), "the alpha channel was written"
        # a view of every second column of [C, H, W] has pixelPitch 2 and depthPitch H * W: refused
        assert api.encode_raster_tiles_device_depth_strided(codec, chw.permute(1, 2, 0)[:, ::2], None, 0.01, tile, arena)[0] == 2
    finally:
        codec.close()
