"""The noData raster calls (lerc_amd_encode_raster_tiles_device_nodata / lerc_amd_decode_raster_window_device_nodata,
include/lerc_amd_nodata.h) on the MI355X (raster_nodata_common.py): every blob against the reference library's lerc_encode of the
numpy slice with the derived mask, byte for byte; every window against np.where(mask, the reference's decode, noData); guard bytes
around the rasters must keep their 0xCD.  Then the Python functions on torch tensors."""
import numpy as np
import pytest

import capi
import raster_nodata_common as ND

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
    B = ND.NoDataBatch(P.lib, ND.GpuMem())
    yield B
    B.close()


VALUES = [(dtype, e, kind) for dtype, e in ND.TYPES for kind in ("inside", "outside", "zero")] + \
         [(dtype, e, kind) for dtype, e in ND.TYPES[6:] for kind in ("nan", "-inf")]


@pytest.mark.parametrize("dtype,e,kind", VALUES, ids=lambda v: v if isinstance(v, str) else (np.dtype(v).name if isinstance(v, type) else None))
def test_types_and_values(batch, dtype, e, kind):
    ND.check_type_and_value(batch, _libs()[1], dtype, e, kind)


def test_negative_zero_matches_zero(batch):
    ND.check_negative_zero(batch, _libs()[1])


def test_no_pixel_matches(batch):
    ND.check_no_pixel_matches(batch, _libs()[1])


def test_a_tile_of_holes_is_an_empty_blob(batch):
    ND.check_one_tile_all_holes(batch, _libs()[1])


def test_nan_holes_stay_inside_the_batch(batch):
    ND.check_nan_holes_stay_inside(batch, _libs()[1])


def test_invalid_values_never_count(batch):
    ND.check_invalid_values_never_count(batch, _libs()[1])


def test_alignment_sweep(batch):
    ND.check_alignment_sweep(batch, _libs()[1])


def test_one_channel_of_an_interleaved_image(batch):
    ND.check_pixel_pitches(batch, _libs()[1])


@pytest.mark.parametrize("rng", ND.RANGES, ids=lambda r: "x".join(str(k) for k in r))
def test_tile_ranges(batch, rng):
    ND.check_range(batch, _libs()[1], rng)


@pytest.mark.parametrize("window,n_tiles", ND.WINDOWS, ids=lambda v: "x".join(str(k) for k in v) if isinstance(v, tuple) else None)
def test_windows(batch, window, n_tiles):
    ND.check_window(batch, _libs()[1], window, n_tiles)


def test_several_chunks_a_class(batch):
    ND.check_chunks(batch, _libs()[1])


def test_range_encode_then_window_decode(batch):
    ND.check_round_trip(batch, _libs()[1])


def test_damaged_blob_inside_and_outside_the_window(batch):
    ND.check_damaged_blob(batch, _libs()[1])


def test_slot_too_small(batch):
    ND.check_slot_too_small(batch, _libs()[1])


def test_boundary(batch):
    ND.check_boundary(batch, _libs()[1])


def test_full_size_tiles_with_nan_holes(batch):
    ND.check_large_tiles(batch, _libs()[1])


def test_python_functions_on_views():
    """through lerc_amd.api: an [H, W] float32 view of a larger tensor with NaN holes, and hwc[..., 1] of a uint16 image with 65535 for
    no data -- blobs equal the masked call's on the derived mask, the way back restores the raster (lossless) or stays within maxZErr with
    the holes back in place, and nothing beside the views is written"""
    import torch
    _, R = _libs()
    from lerc_amd import api
    tile, per_tile = (32, 40), 32 * 40 * 4 + 2048
    rng = np.random.default_rng(29)
    codec = api.DeviceCodec()
    try:
        # a view of a larger float32 tensor, NaN holes
        host = np.array(ND.RT.noisy_float(90, 120)[0])
        host[4:87, 7:108][ND.holes_of(83, 101)] = np.nan
        big = torch.from_numpy(host).cuda()
        view = big[4:87, 7:108]
        arena = torch.zeros(9 * per_tile, dtype=torch.uint8, device="cuda")
        rc, offs, sizes, used = api.encode_raster_tiles_device_nodata(codec, view, float("nan"), 0.01, tile, arena)
        assert rc == 0, (rc, codec.last_error())
        C = ND.judge(R, host[4:87, 7:108].copy(), ND.NAN, 0.01, tile)
        got = arena.cpu().numpy()
        assert [got[int(o):int(o) + int(s)].tobytes() for o, s in zip(offs, sizes)] == C.blobs
        valid = (~torch.isnan(view)).to(torch.uint8)
        arena_m = torch.zeros_like(arena)
        rc, offs_m, sizes_m, _ = api.encode_raster_tile_range_device(codec, view, valid, 0.01, tile, (0, 0, 3, 3), arena_m)
        assert rc == 0 and np.array_equal(sizes, sizes_m)
        got_m = arena_m.cpu().numpy()
        assert all(got[int(o):int(o) + int(s)].tobytes() == got_m[int(om):int(om) + int(s)].tobytes() for o, om, s in zip(offs, offs_m, sizes))
        out_big = torch.full((90, 120), -7.0, dtype=torch.float32, device="cuda")
        out = out_big[4:87, 7:108]
        valid_out = torch.full((83, 101), 9, dtype=torch.uint8, device="cuda")
        assert api.decode_raster_tiles_device_nodata(codec, arena, offs, sizes, out, float("nan"), tile, valid_out) == 0
        torch.cuda.synchronize()
        assert ND.same_pixels(out.cpu().numpy(), C.want) and np.array_equal(valid_out.cpu().numpy(), C.mask)
        around = torch.ones((90, 120), dtype=torch.bool, device="cuda")
        around[4:87, 7:108] = False
        assert bool((out_big[around] == -7.0).all()), "the decode wrote beside the view"
        win = torch.zeros((30, 45), dtype=torch.float32, device="cuda")
        assert api.decode_raster_window_device_nodata(codec, arena, offs, sizes, (83, 101), tile, (40, 50), win, float("nan")) == 0
        torch.cuda.synchronize()
        assert ND.same_pixels(win.cpu().numpy(), C.want[40:70, 50:95])

        # one channel of an interleaved uint16 image, 65535 for no data; a tile range
        img = rng.integers(0, 4000, (83, 101, 3), dtype=np.uint16)
        img[..., 1][ND.holes_of(83, 101, seed=8)] = 65535
        hwc = torch.from_numpy(img.view(np.int16)).cuda()    # (torch has no uint16 everywhere: the bits as int16, noData -1)
        rc, offs, sizes, used = api.encode_raster_tiles_device_nodata(codec, hwc[..., 1], -1, 0, tile, arena, tile_range=(1, 0, 2, 3))
        assert rc == 0, (rc, codec.last_error())
        assert not sizes[:3].any() and sizes[3:].all()
        C = ND.judge(R, img[..., 1].view(np.int16).copy(), -1.0, 0, tile)
        got = arena.cpu().numpy()
        assert [got[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() for t in range(3, 9)] == C.blobs[3:]
        back = torch.full((51, 101, 3), 77, dtype=torch.int16, device="cuda")
        assert api.decode_raster_window_device_nodata(codec, arena, offs, sizes, (83, 101), tile, (32, 0), back[..., 1], -1) == 0
        torch.cuda.synchronize()
        assert torch.equal(back[..., 1], hwc[32:, :, 1]) and bool((back[..., 0] == 77).all()) and bool((back[..., 2] == 77).all())
    finally:
        codec.close()
