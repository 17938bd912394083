"""The strided raster tile calls (lerc_amd_encode_raster_tiles_device_strided / lerc_amd_decode_raster_tiles_device_strided) on the
MI355X: pixel-interleaved, gapped and line-interleaved rasters cut into a grid of tiles and back (raster_px_common.py).  Every blob is
compared with the reference library's lerc_encode of the numpy slice, byte for byte; pixels and valid bytes with its lerc_decode's;
guards, row padding and the gaps between the pixels must keep their sentinel."""
import numpy as np
import pytest

import capi
import raster_px_common as PX

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
    B = PX.PxBatch(P.lib, PX.RT.M.GpuMem())
    yield B
    B.close()


@pytest.mark.parametrize("case", PX.PARITY, ids=PX.case_id)
def test_parity(batch, case):
    PX.check_parity(batch, _libs()[1], case)


@pytest.mark.parametrize("case", PX.SAME_AS_PLANES, ids=PX.case_id)
def test_same_bytes_as_the_planar_call(batch, case):
    PX.check_same_as_planes(batch, _libs()[1], case)


def test_pixel_pitch_one_is_the_existing_call(batch):
    PX.check_pixel_pitch_one(batch, _libs()[1])


def test_line_interleaved(batch):
    PX.check_line_interleaved(batch, _libs()[1])


def test_chunks(batch):
    PX.check_chunks(batch, _libs()[1])


def test_failing_tile(batch):
    PX.check_failing_tile(batch, _libs()[1])


def test_arguments(batch):
    PX.check_arguments(batch, _libs()[1])


def test_python_interleaved_view():
    """RGB out of a [90, 120, 4] uint8 tensor, hwc[4:87, 7:108, :3].permute(2, 0, 1), through lerc_amd.api without a copy: the round trip
    equals the input, the alpha channel and everything beside the view keep their 0xA5, nine tiles go through the staging buffer each
    way -- and a tensor with dense rows still takes the calls without a pixel pitch"""
    import torch
    _libs()
    from lerc_amd import api
    rng = np.random.default_rng(19)
    big = torch.from_numpy(rng.integers(0, 256, (90, 120, 4), dtype=np.uint8)).cuda()
    view = big[4:87, 7:108, :3].permute(2, 0, 1)
    assert tuple(view.shape) == (3, 83, 101) and view.stride(-1) == 4 and view.stride(0) == 1
    tile = (32, 40)
    codec = api.DeviceCodec()
    try:
        arena = torch.zeros(9 * (3 * (32 * 40 + 1024) + 64), dtype=torch.uint8, device="cuda")
        rc, offsets, sizes, used = api.encode_raster_tiles_device(codec, view, None, 0, tile, arena)
        assert rc == 0, (rc, codec.last_error())
        out_big = torch.full((90, 120, 4), 0xA5, dtype=torch.uint8, device="cuda")
        rc = api.decode_raster_tiles_device(codec, arena, offsets, sizes, out_big[4:87, 7:108, :3].permute(2, 0, 1), None, tile)
        assert rc == 0, (rc, codec.last_error())
        torch.cuda.synchronize()
        assert torch.equal(out_big[4:87, 7:108, :3], big[4:87, 7:108, :3])
        around = torch.ones((90, 120, 4), dtype=torch.bool, device="cuda")
        around[4:87, 7:108, :3] = False
        assert bool((out_big[around] == 0xA5).all()), "the decode wrote beside the view or into the alpha channel"
        assert codec.raster_tiles_counters() == [9, 0, 9, 0]
        # the planar copy of the same view: the same blobs by the calls without a pixel pitch, counted like test_python_view's
        planes = view.contiguous()
        arena2 = torch.zeros_like(arena)
        rc, offsets2, sizes2, used2 = api.encode_raster_tiles_device(codec, planes, None, 0, tile, arena2)
        assert rc == 0 and used2 == used and np.array_equal(sizes2, sizes)
        host, host2 = arena.cpu().numpy(), arena2.cpu().numpy()
        for t in range(9):
            assert np.array_equal(host[int(offsets[t]):int(offsets[t]) + int(sizes[t])], host2[int(offsets2[t]):int(offsets2[t]) + int(sizes2[t])]), t
        back = torch.zeros_like(planes)
        assert api.decode_raster_tiles_device(codec, arena2, offsets2, sizes2, back, None, tile) == 0
        torch.cuda.synchronize()
        assert torch.equal(back, planes)
        assert codec.raster_tiles_counters() == [18, 0, 18, 0]
    finally:
        codec.close()
