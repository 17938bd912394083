"""The window decode and the tile range encode (lerc_amd_decode_raster_window_device / lerc_amd_encode_raster_tiles_device_range) on
the MI355X (raster_window_common.py).  A window's pixels and valid bytes are compared with the slice of the raster the reference
library decodes from the same blobs, and bit for bit with the slice of what lerc_amd_decode_raster_tiles_device writes; a range's blobs
with the reference's lerc_encode of the numpy slices, byte for byte; guards, padding and the gaps between pixels must keep their
sentinel."""
import numpy as np
import pytest

import capi
import raster_window_common as RW

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
    B = RW.WindowBatch(P.lib, RW.RT.M.GpuMem())
    yield B
    B.close()


@pytest.mark.parametrize("window,n_tiles", RW.WINDOWS, ids=lambda v: "x".join(str(k) for k in v) if isinstance(v, tuple) else None)
def test_windows(batch, window, n_tiles):
    RW.check_windows(batch, _libs()[1], window, n_tiles)


def test_window_on_thin_edges(batch):
    RW.check_windows(batch, _libs()[1], *RW.THIN_WINDOW, shape_tile=RW.THIN_EDGES)


@pytest.mark.parametrize("case", RW.CASES, ids=RW.case_id)
def test_types_and_destinations(batch, case):
    RW.check_case(batch, _libs()[1], case)


def test_alignment_sweep(batch):
    RW.check_alignment_sweep(batch, _libs()[1])


def test_only_the_windows_tiles(batch):
    RW.check_only_the_windows_tiles(batch, _libs()[1])


def test_window_chunks(batch):
    RW.check_chunks(batch, _libs()[1])


def test_damaged_blob_inside_and_outside_the_window(batch):
    RW.check_damaged_blob(batch, _libs()[1])


def test_window_arguments(batch):
    RW.check_window_arguments(batch, _libs()[1])


@pytest.mark.parametrize("rng", RW.RANGES, ids=lambda r: "x".join(str(k) for k in r))
def test_tile_ranges(batch, rng):
    RW.check_ranges(batch, _libs()[1], rng)


def test_tile_range_mask_bands_and_pixels(batch):
    RW.check_range_kinds(batch, _libs()[1])


def test_tile_range_in_place(batch):
    RW.check_range_in_place(batch, _libs()[1])


def test_tile_range_arguments(batch):
    RW.check_range_arguments(batch, _libs()[1])


def test_range_encode_then_window_decode(batch):
    RW.check_round_trip(batch, _libs()[1])


def test_python_window_and_range():
    """through lerc_amd.api: two ranks' runs of tile rows of a [3, 83, 101] uint8 view fill one table; a window of it comes back into an
    RGB view of an [h, w, 4] tensor -- the pixels of the raster's slice, the alpha channel and everything beside the view untouched,
    and only the window's tiles are decoded"""
    import torch
    _libs()
    from lerc_amd import api, shard
    rng = np.random.default_rng(23)
    big = torch.from_numpy(rng.integers(0, 256, (3, 90, 120), dtype=np.uint8)).cuda()
    view = big[:, 4:87, 7:108]
    tile, per_tile = (32, 40), 3 * (32 * 40 + 1024) + 64
    codec = api.DeviceCodec()
    try:
        arena = torch.zeros(9 * per_tile, dtype=torch.uint8, device="cuda")
        offsets, sizes, at = np.zeros(9, np.uint64), np.zeros(9, np.uint32), 0
        for rank in range(2):
            first, count = shard.raster_tile_rows(rank, 2, 83, tile[0])
            assert (first, count) == ((0, 2), (2, 1))[rank]
            rc, o, s, used = api.encode_raster_tile_range_device(codec, view, None, 0, tile, (first, 0, count, 3), arena[at:])
            assert rc == 0, (rc, codec.last_error())
            members = [ty * 3 + tx for ty in range(first, first + count) for tx in range(3)]
            assert not s[[t for t in range(9) if t not in members]].any()
            offsets[members], sizes[members] = o[members] + at, s[members]
            at += (used + 15) & ~15
        assert codec.raster_tiles_counters() == [9, 0, 0, 0]
        whole = torch.zeros_like(view)
        assert api.decode_raster_tiles_device(codec, arena, offsets, sizes, whole, None, tile) == 0
        torch.cuda.synchronize()
        assert torch.equal(whole, view)
        window = (17, 23, 50, 60)
        touched = api.raster_window_tiles(83, 101, tile, window)
        assert touched == RW.window_tiles(83, 101, tile, window) == [0, 1, 2, 3, 4, 5, 6, 7, 8]
        assert api.raster_window_tiles(83, 101, tile, (33, 41, 27, 37)) == [4] and api.raster_window_tiles(83, 101, tile, (64, 0, 19, 41)) == [6, 7]
        window = (33, 41, 40, 37)
        touched = api.raster_window_tiles(83, 101, tile, window)
        assert touched == [4, 7]
        dead_off, dead_size = np.full(9, RW.DEAD64, np.uint64), np.full(9, RW.DEAD32, np.uint32)
        dead_off[touched], dead_size[touched] = offsets[touched], sizes[touched]
        out_big = torch.full((50, 60, 4), 0xA5, dtype=torch.uint8, device="cuda")
        out = out_big[5:45, 9:46, :3].permute(2, 0, 1)
        rc = api.decode_raster_window_device(codec, arena, dead_off, dead_size, (83, 101), tile, window[:2], out, None)
        assert rc == 0, (rc, codec.last_error())
        torch.cuda.synchronize()
        assert torch.equal(out, view[:, 33:73, 41:78])
        around = torch.ones((50, 60, 4), dtype=torch.bool, device="cuda")
        around[5:45, 9:46, :3] = False
        assert bool((out_big[around] == 0xA5).all()), "the decode wrote beside the view or into the alpha channel"
        assert codec.raster_tiles_counters() == [9, 0, 9 + 2, 0]
    finally:
        codec.close()
