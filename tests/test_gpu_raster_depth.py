"""Raster mosaics of depth tiles (lerc_amd_encode_raster_tiles_device_depth / lerc_amd_decode_raster_tiles_device_depth) on the MI355X:
an [H, W, C] raster, or a view of one with padded rows, cut into the grid and coded as blobs of nDepth = C (raster_depth_common.py)."""
import numpy as np
import pytest

import capi
import raster_depth_common as C

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
    B = C.RasterDepth(P.lib, C.D.GpuMem())
    yield B
    B.close()


@pytest.mark.parametrize("view", [False, True])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("dtype,e", [(np.uint16, 0), (np.float32, 0.01)])
def test_four_shape_classes(batch, dtype, e, with_mask, view):
    """70 x 90 x 3, tile 32: interior, right column, bottom row, corner"""
    C.check_raster(batch, _libs()[1], dtype, e, 70, 90, 3, 32, with_mask, view)


@pytest.mark.parametrize("dtype,e", [(np.uint16, 0), (np.float32, 0.01)])
def test_whole_tiles_slotted(batch, dtype, e):
    C.check_raster(batch, _libs()[1], dtype, e, 64, 64, 4, 32, True, False, slotted=True)


def test_refused(batch):
    C.check_refused(batch)


def test_python_wrappers():
    """lerc_amd.api's four depth calls on torch tensors: an [H, W, C] view into a wider tensor (its strides are the pitches), then tiles"""
    import torch
    from lerc_amd import api
    _, R = _libs()
    rng = np.random.default_rng(9)
    h, w, c, tile, e = 70, 90, 3, 32, 0.01
    big_np = np.ascontiguousarray(C.D.tiles_of(rng, 1, h, w + 8, c, np.float32)[0])
    mask_np = C.D.random_blob_mask(rng, 1, h, w)[0]
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    try:
        big = torch.from_numpy(big_np).cuda()
        view = big[:, 5:5 + w]
        valid = torch.from_numpy(mask_np).cuda()
        grid = api.raster_tile_grid(h, w, (tile, tile))
        arena = torch.zeros(len(grid) * (tile * tile * c * 4 + 4096), dtype=torch.uint8, device="cuda")
        rc, offs, sizes, used = api.encode_raster_tiles_device_depth(codec, view, valid, e, (tile, tile), arena)
        assert rc == 0, (rc, codec.last_note())
        a_np = arena.cpu().numpy()
        out = torch.full_like(big, -7.0)
        valid_out = torch.full_like(valid, 9)
        assert api.decode_raster_tiles_device_depth(codec, arena, offs, sizes, out[:, 5:5 + w], valid_out, (tile, tile)) == 0
        out_np, vo_np = out.cpu().numpy(), valid_out.cpu().numpy()
        for t, (y0, y1, x0, x1) in enumerate(grid):
            rect = np.ascontiguousarray(big_np[y0:y1, 5 + x0:5 + x1])
            rc_r, want = R.encode(rect, e, n_depth=c, mask=np.ascontiguousarray(mask_np[y0:y1, x0:x1]))
            assert rc_r == 0 and a_np[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() == want, "tile %d" % t
            rc_r, p_r, m_r = R.decode(want, want_masks=1)
            assert out_np[y0:y1, 5 + x0:5 + x1].tobytes() == p_r.reshape(y1 - y0, x1 - x0, c).tobytes()
            assert np.array_equal(vo_np[y0:y1, x0:x1], m_r.reshape(y1 - y0, x1 - x0))
        assert (out_np[:, :5] == -7.0).all() and (out_np[:, 5 + w:] == -7.0).all(), "elements beside the view were written"
        # a view of every second column has pixelPitch 2 * C: refused
        assert api.encode_raster_tiles_device_depth(codec, big[:, ::2], None, e, (tile, tile), arena)[0] == 2
        # ---- tiles
        t_np = np.ascontiguousarray(C.D.tiles_of(rng, 4, 33, 41, c, np.int32))
        m_np = C.D.masks_of(rng, 4, 33, 41)
        tiles, masks = torch.from_numpy(t_np).cuda(), torch.from_numpy(m_np).cuda()
        rc, offs, sizes, used = api.encode_tiles_device_depth(codec, tiles, masks, 0, arena)
        assert rc == 0, (rc, codec.last_note())
        a_np = arena.cpu().numpy()
        want = C.D.ref_blobs(R, t_np, m_np, 0)
        assert [a_np[int(offs[t]):int(offs[t]) + int(sizes[t])].tobytes() for t in range(4)] == want
        back, vback = torch.zeros_like(tiles), torch.zeros_like(masks)
        assert api.decode_tiles_device_depth(codec, arena, offs, sizes, back, vback) == 0
        assert np.array_equal(vback.cpu().numpy(), m_np)
        assert np.array_equal(back.cpu().numpy()[m_np > 0], t_np[m_np > 0])
        assert codec.tile_batch_counters()[1] == 0 and codec.tile_batch_counters()[3] == 0
    finally:
        codec.close()
