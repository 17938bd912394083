"""The raster tile calls (lerc_amd_encode_raster_tiles_device / lerc_amd_decode_raster_tiles_device) on the MI355X: a pitched,
misaligned raster cut into a grid of tiles and back (raster_tiles_common.py).  Every blob is compared with the reference library's
lerc_encode of the numpy slice, byte for byte; pixels and valid bytes with its lerc_decode's; padding and guards must keep their
sentinel; and the tiles are counted as done by the tile batches' own launches wherever the tile calls themselves would do so."""
import numpy as np
import pytest

import capi
import raster_tiles_common as RT

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
    B = RT.RasterBatch(P.lib, RT.M.GpuMem())
    yield B
    B.close()


@pytest.mark.parametrize("case", RT.PARITY, ids=RT.parity_id)
def test_parity(batch, case):
    dtype, e, nb, with_mask, shape_tile = case
    RT.check_parity(batch, _libs()[1], dtype, e, nb, with_mask, shape_tile)


def test_is_a_batch(batch):
    RT.check_is_a_batch(batch, _libs()[1])


@pytest.mark.parametrize("case", RT.COUNTERS, ids=lambda c: "%s%s" % ("%dx" % c[2] if c[2] > 1 else "", c[0].__name__))
def test_counters_match_the_tile_calls(batch, case):
    RT.check_counters_match(batch, _libs()[1], *case)


def test_chunks(batch):
    RT.check_chunks(batch, _libs()[1])


def test_in_place(batch):
    RT.check_in_place(batch, _libs()[1])


def test_failing_tile(batch):
    RT.check_failing_tile(batch, _libs()[1])


def test_arguments(batch):
    RT.check_arguments(batch, _libs()[1])


def island_mask(n_rows, n_cols):
    """the island of lerc_amd.synth.island_mask on a rectangle: an ellipse of valid pixels with scattered holes in a band of rows"""
    i = np.arange(n_rows, dtype=np.int64).reshape(-1, 1)
    j = np.arange(n_cols, dtype=np.int64).reshape(1, -1)
    m = ((i - (n_rows - 1) / 2.0) / (0.44 * n_rows)) ** 2 + ((j - (n_cols - 1) / 2.0) / (0.44 * n_cols)) ** 2 < 1.0
    hole = ((i * 2654435761 + j * 40503) % 1009 == 0) & (i >= n_rows // 4) & (i < n_rows // 4 + n_rows // 8)
    return (m & ~hole).astype(np.uint8)


def test_island_1030x1290(batch):
    """30 tiles of 256 x 256 with edges of 6 rows and 10 columns, all valid, partly valid and empty ones: parity, and all 30 by the
    batch's launches each way"""
    from lerc_amd import synth
    R = _libs()[1]
    n_rows, n_cols, tile = 1030, 1290, (256, 256)
    raster = synth.c2_float32(n_rows, n_cols).numpy()[None]
    mask = island_mask(n_rows, n_cols)
    assert len(RT.grid(n_rows, n_cols, tile)) == 30 and sorted(RT.classes(n_rows, n_cols, tile)) == [(6, 10), (6, 256), (256, 10), (256, 256)]
    want = RT.ref_blobs(R, raster, mask, 0.01, tile)
    _, moved = RT.batch_delta(batch, 0, lambda: RT.check_encode(batch, R, raster, mask, 0.01, tile, want=want))
    assert moved == (30, 0), ("tiles left the batch's launches", moved, batch.note())
    RT.check_encode(batch, R, raster, mask, 0.01, tile, slot_bytes=RT.slot_for(raster, tile), want=want)
    (pix, valid), moved = RT.batch_delta(batch, 2, lambda: RT.check_decode(batch, R, want, raster.shape, raster.dtype, tile, True))
    assert moved == (30, 0), ("tiles left the batch's launches", moved, batch.note())
    assert np.array_equal(valid, mask)


def test_python_view():
    """a [3, 83, 101] uint8 view cut out of a larger tensor, through lerc_amd.api: the round trip equals the input, the blobs' headers
    state the sizes of raster_tile_grid, and nothing beside the view is written"""
    import torch
    _libs()
    from lerc_amd import api
    rng = np.random.default_rng(17)
    big = torch.from_numpy(rng.integers(0, 256, (3, 90, 120), dtype=np.uint8)).cuda()
    view = big[:, 4:87, 7:108]
    assert tuple(view.shape) == (3, 83, 101) and not view.is_contiguous()
    tile = (32, 40)
    codec = api.DeviceCodec()
    try:
        arena = torch.zeros(9 * (3 * (32 * 40 + 1024) + 64), dtype=torch.uint8, device="cuda")
        rc, offsets, sizes, used = api.encode_raster_tiles_device(codec, view, None, 0, tile, arena)
        assert rc == 0, (rc, codec.last_error())
        grid = api.raster_tile_grid(83, 101, tile)
        assert grid == RT.grid(83, 101, tile) == codec.raster_tile_grid(83, 101, tile) and len(grid) == len(offsets) == 9
        host = arena.cpu().numpy()
        for t, (r0, r1, c0, c1) in enumerate(grid):
            assert RT.header_shape(host[int(offsets[t]):int(offsets[t]) + int(sizes[t])].tobytes()) == (r1 - r0, c1 - c0), t
        out_big = torch.full((3, 90, 120), 0xA5, dtype=torch.uint8, device="cuda")
        rc = api.decode_raster_tiles_device(codec, arena, offsets, sizes, out_big[:, 4:87, 7:108], None, tile)
        assert rc == 0, (rc, codec.last_error())
        torch.cuda.synchronize()
        assert torch.equal(out_big[:, 4:87, 7:108], view)
        around = torch.ones((3, 90, 120), dtype=torch.bool, device="cuda")
        around[:, 4:87, 7:108] = False
        assert bool((out_big[around] == 0xA5).all()), "the decode wrote beside the view"
        assert codec.raster_tiles_counters() == [9, 0, 9, 0]
    finally:
        codec.close()
