#!/usr/bin/env python3
"""Times the raster tile calls (lerc_amd_encode_raster_tiles_device / lerc_amd_decode_raster_tiles_device) against the tile calls
they are built on, to learn what the staging pass -- k_rt_cut in front of the encode, k_rt_paste behind the decode -- costs.  One
MI355X, everything device resident, float32 (synth.c2_float32) at MaxZError 0.01, tiles of 256 x 256, packed arenas, two rasters:

  8192 x 8192    1024 tiles, one shape class
  8190 x 8190    961 interior tiles and three edge classes (254 columns, 254 rows, the corner)

Three things are timed on each:

  (a) the raster calls on the raster as it lies
  (b) lerc_amd_encode_tiles_device / lerc_amd_decode_tiles_device on the same tiles cut beforehand (the ragged raster: its
      interior class only -- the edge classes are (a)'s alone, so (a) - (b) is an upper bound there)
  (c) a plain device-to-device copy of the raster's bytes: what a pass that reads and writes them costs when nothing is strided

(a) - (b) is the staging's cost.  Target: (a) - (b) <= 2 x (c) on the 8192^2 raster -- rows of 1 KiB instead of one long run, a launch
per chunk, the records' round trip per class; beyond that the cut kernel is not streaming.

Every call is queued on torch's current stream and timed with events around it; warm-up, then the median and the interquartile range
of REPS (21) repetitions.  Prints the numbers (they are recorded in DESIGN.md 8.3); exit status 1 if the target is missed.  Run it under a time limit of its own:
  timeout -k 10 600 python tools/time_raster_tiles.py

`python tools/time_raster_tiles.py interleaved` times the strided calls (lerc_amd_*_raster_tiles_device_strided) on PIXEL-INTERLEAVED
rasters instead: 4096 x 4096 x 3 uint8 lossless and 4096 x 4096 x 4 float32 at 0.01, as [H, W, C] tensors, tiles of 256 x 256:

  (1) the strided call on hwc.permute(2, 0, 1), no copy: k_rt_cut_px / k_rt_paste_px do the transposition
  (2) what a caller did before: permute(2, 0, 1).contiguous() and the planar call; back: the planar call and a copy into [H, W, C]
  (3) the planar call alone on the planar raster of the same bytes: (1) - (3) is what the transposing kernels cost over
      k_rt_cut / k_rt_paste, the rest of the two calls being the same launches

No pass mark (exit status 0): the numbers are recorded in DESIGN.md 8.3.  The kernels' own times come from running this mode under
rocprofv3 --kernel-trace --stats (k_rt_cut_px, k_rt_paste_px against k_rt_cut, k_rt_paste).

`python tools/time_raster_tiles.py window` times lerc_amd_decode_raster_window_device on the 8192 x 8192 raster: windows of one tile,
1/16, 1/4 and the whole of it, each once on tile boundaries and once shifted by (3, 5), against what a caller did before -- the
whole-raster decode and a device copy of the slice.  The shifted whole-raster window (8189 x 8187 from (3, 5)) against the whole-raster
decode is what the clipped paste costs over k_rt_paste.  Every window is checked bit for bit against the slice first.  No pass mark;
the numbers are recorded in DESIGN.md 8.3 and profiles/raster_window_time.txt.

`python tools/time_raster_tiles.py depth [FILE]` times the depth raster calls that take a layout (include/lerc_amd_depth.h) on
8192 x 8192 x 3 uint16 lossless and 4096 x 4096 x 4 float32 at 0.01, tiles of 256 x 256, blobs of nDepth = C:

  (a) lerc_amd_*_raster_tiles_device_depth_strided on chw.permute(1, 2, 0) (planes) and on the C channels of an [H, W, C + 1]
      tensor (gapped pixels: RGB out of RGBA), no copy: k_rtd_cut / k_rtd_paste read and write the raster where it lies
  (b) what a caller did before: view.contiguous() and the packed depth call, the copy inside the timed region; back: the packed
      decode and the copy into the view
  and the window decode into packed pixels against the whole-raster decode and a copy of the slice, for windows of one tile, 1/16,
  1/4 and the whole, with a least-squares line through them: a fixed cost and a cost per thousand tiles.

(a) and (b) alternate inside one loop of REPS; the arenas of (a) and (b) are compared byte for byte before anything is timed, every
window against the slice.  No pass mark: the report says where (a) is slower than (b) or a window slower than the whole decode.  It
goes to FILE (default profiles/raster_depth_layouts_time.txt) and to stdout; the table is recorded in DESIGN.md 8.4.

`python tools/time_raster_tiles.py nodata [FILE]` times the noData raster calls (include/lerc_amd_nodata.h) on 8192 x 8192 float32 at
0.01 with NaN holes and 16384 x 16384 uint16 lossless with 65535 for no data, tiles of 256 x 256, about 10 % holes, both ways:

  (a) lerc_amd_encode_raster_tiles_device_nodata / lerc_amd_decode_raster_window_device_nodata (the whole raster as the window)
  (b) what a caller did before: valid = (raster != noData) (or ~isnan) as a uint8 tensor plus the masked strided encode; back, the
      masked decode plus a fill of noData where the valid bytes say 0 -- the torch operations inside the timed region
  (c) the float raster with its NaN holes through the existing call without a mask (encode only, fewer runs: its tiles go one by one)

(a) and (b) alternate inside one loop of REPS; their arenas are compared byte for byte and their pixels bit for bit (NaN by isnan)
before anything is timed.  No pass mark: the report says where (a) is slower than (b).  It goes to FILE (default
profiles/raster_nodata_time.txt) and to stdout; the table is recorded in DESIGN.md 8.3.
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = int(os.environ.get("REPS", "21"))
TILE = 256
E = 0.01


def interleaved():
    import torch
    from lerc_amd import api, synth
    assert torch.cuda.is_available(), "needs a GPU"
    size, tile = 4096, (TILE, TILE)
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    print("strided raster tile calls on pixel-interleaved rasters -- %s; %d x %d, tiles of %d x %d; median [interquartile range] of %d, ms"
          % (torch.cuda.get_device_name(0), size, size, TILE, TILE, REPS))
    terrain = synth.c2_float32(size, size, device="cuda:0")
    for name, nb, e in (("uint8", 3, 0.0), ("float32", 4, E)):
        chans = [terrain.roll(37 * b, 0).roll(91 * b, 1) + 3.0 * b for b in range(nb)]
        if name == "uint8":
            lo, hi = float(terrain.min()), float(terrain.max())
            chans = [((c - lo) * (255.0 / (hi - lo + 3.0 * nb))).to(torch.uint8) for c in chans]
        hwc = torch.stack(chans, dim=2).contiguous()
        del chans
        view = hwc.permute(2, 0, 1)
        item = hwc.element_size()
        n = len(api.raster_tile_grid(size, size, tile))
        arena = torch.zeros(n * (nb * (TILE * TILE * item + TILE * TILE // 4 + 1024) + 16), dtype=torch.uint8, device="cuda")
        hwc_back = torch.zeros_like(hwc)
        planes = view.contiguous()
        planes_back = torch.zeros_like(planes)
        state = {}

        def enc_1():
            rc, offs, sizes, used = api.encode_raster_tiles_device(codec, view, None, e, tile, arena)
            assert rc == 0, (rc, codec.last_error())
            state["t"] = (offs, sizes, used)

        def dec_1():
            assert api.decode_raster_tiles_device(codec, arena, state["t"][0], state["t"][1], hwc_back.permute(2, 0, 1), None, tile) == 0

        def enc_2():
            rc, offs, sizes, used = api.encode_raster_tiles_device(codec, view.contiguous(), None, e, tile, arena)
            assert rc == 0, (rc, codec.last_error())

        def dec_2():
            assert api.decode_raster_tiles_device(codec, arena, state["t"][0], state["t"][1], planes_back, None, tile) == 0
            hwc_back.copy_(planes_back.permute(1, 2, 0))

        def enc_3():
            rc, offs, sizes, used = api.encode_raster_tiles_device(codec, planes, None, e, tile, arena)
            assert rc == 0, (rc, codec.last_error())

        def dec_3():
            assert api.decode_raster_tiles_device(codec, arena, state["t"][0], state["t"][1], planes_back, None, tile) == 0

        def copy_c():
            hwc_back.copy_(hwc)

        r0 = codec.raster_tiles_counters()
        enc_1()
        dec_1()
        torch.cuda.synchronize()
        r1 = codec.raster_tiles_counters()
        err = float((hwc_back.double() - hwc.double()).abs().max())
        assert err <= e + 1e-4, err
        t = {k: timed_on(torch, f) for k, f in (("e1", enc_1), ("d1", dec_1), ("e2", enc_2), ("d2", dec_2), ("e3", enc_3), ("d3", dec_3), ("c", copy_c))}
        mib = hwc.numel() * item / 2 ** 20
        print("%s x %d (%.0f MiB, %d blob bytes): raster call counters [cut, in place, pasted, in place] %s; max error %.6f"
              % (name, nb, mib, state["t"][2], [int(y - x) for x, y in zip(r0, r1)], err))
        print("  (1) strided call, no copy               encode %8.3f [%6.3f]   decode %8.3f [%6.3f]" % (t["e1"] + t["d1"]))
        print("  (2) contiguous() + planar call / back   encode %8.3f [%6.3f]   decode %8.3f [%6.3f]" % (t["e2"] + t["d2"]))
        print("  (3) planar call on the planar raster    encode %8.3f [%6.3f]   decode %8.3f [%6.3f]" % (t["e3"] + t["d3"]))
        print("  device-to-device copy of the raster     %8.3f [%6.3f]   (%.0f GB/s read + written)" % (t["c"][0], t["c"][1], 2 * mib * 2 ** 20 / t["c"][0] / 1e6))
        print("  (1) - (3), the transposition's price    encode %8.3f   decode %8.3f" % (t["e1"][0] - t["e3"][0], t["d1"][0] - t["d3"][0]))
        print("  (2) - (1), the gain over a planar copy  encode %8.3f   decode %8.3f" % (t["e2"][0] - t["e1"][0], t["d2"][0] - t["d1"][0]))
        del hwc, view, arena, hwc_back, planes, planes_back
        torch.cuda.empty_cache()
    codec.close()
    return 0


def window():
    import torch
    from lerc_amd import api, synth
    assert torch.cuda.is_available(), "needs a GPU"
    size, tile = 8192, (TILE, TILE)
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    print("window decode against the whole-raster decode and a slice -- %s; %d x %d float32 at %.2f, tiles of %d x %d, packed; "
          "median [interquartile range] of %d, ms" % (torch.cuda.get_device_name(0), size, size, E, TILE, TILE, REPS))
    raster = synth.c2_float32(size, size, device="cuda:0")
    n = len(api.raster_tile_grid(size, size, tile))
    arena = torch.zeros(n * (TILE * TILE * 4 + TILE * TILE // 4 + 1024 + 16), dtype=torch.uint8, device="cuda")
    rc, offs, sizes, used = api.encode_raster_tiles_device(codec, raster, None, E, tile, arena)
    assert rc == 0, (rc, codec.last_error())
    back = torch.zeros_like(raster)

    def whole():
        assert api.decode_raster_tiles_device(codec, arena, offs, sizes, back, None, tile) == 0

    whole()
    torch.cuda.synchronize()
    ref = back.clone()
    t_whole = timed_on(torch, whole)
    print("  whole-raster decode (lerc_amd_decode_raster_tiles_device)   %8.3f [%6.3f]" % t_whole)
    print("  window (row0, col0, rows x cols)        tiles   window decode        whole decode + copy of the slice")
    for name, side in (("one tile", TILE), ("1/16", size // 4), ("1/4", size // 2), ("whole", size)):
        for shift in ((0, 0), (3, 5)):
            rows, cols = (side, side) if shift == (0, 0) or side < size else (size - shift[0], size - shift[1])
            r0, c0 = (0 if side == size else TILE * 3) + shift[0], (0 if side == size else TILE * 5) + shift[1]
            out = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
            touched = len(api.raster_window_tiles(size, size, tile, (r0, c0, rows, cols)))

            def win():
                assert api.decode_raster_window_device(codec, arena, offs, sizes, (size, size), tile, (r0, c0), out, None) == 0

            def old():
                assert api.decode_raster_tiles_device(codec, arena, offs, sizes, back, None, tile) == 0
                out.copy_(back[r0:r0 + rows, c0:c0 + cols])

            c_0 = codec.raster_tiles_counters()
            win()
            torch.cuda.synchronize()
            c_1 = codec.raster_tiles_counters()
            assert [int(b - a) for a, b in zip(c_0, c_1)] == [0, 0, touched, 0]
            assert torch.equal(out.view(torch.int32), ref[r0:r0 + rows, c0:c0 + cols].contiguous().view(torch.int32)), "the window is not the slice"
            t_win, t_old = timed_on(torch, win), timed_on(torch, old)
            print("  %-8s (%4d, %4d, %4d x %4d)   %5d   %8.3f [%6.3f]   %8.3f [%6.3f]" % ((name, r0, c0, rows, cols, touched) + t_win + t_old))
            del out
    codec.close()
    return 0


def depth(out_path):
    import torch
    from lerc_amd import api, synth
    assert torch.cuda.is_available(), "needs a GPU"
    tile = (TILE, TILE)
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    say("depth raster calls with a layout against contiguous() + the packed calls -- %s; tiles of %d x %d, packed arenas; the two ways "
        "alternating, median [interquartile range] of %d, ms" % (torch.cuda.get_device_name(0), TILE, TILE, REPS))
    verdicts = []
    for name, size, c, e in (("uint16", 8192, 3, 0.0), ("float32", 4096, 4, E)):
        terrain = synth.c2_float32(size, size, device="cuda:0")
        chans = [terrain.roll(37 * b, 0).roll(91 * b, 1) + 3.0 * b for b in range(c)]
        if name == "uint16":
            lo, hi = float(terrain.min()), float(terrain.max())
            chans = [((ch - lo) * (60000.0 / (hi - lo + 3.0 * c))).to(torch.int32).to(torch.uint16) for ch in chans]
        hwc = torch.stack(chans, dim=2).contiguous()
        del chans, terrain
        item = hwc.element_size()
        mib = hwc.numel() * item / 2 ** 20
        n = len(api.raster_tile_grid(size, size, tile))
        cap = n * (TILE * TILE * c * item + TILE * TILE // 4 + 2048)
        arena_a = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        arena_b = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        hwc_back = torch.zeros_like(hwc)
        say("%s x %d, %d x %d (%.0f MiB), maxZErr %g, %d tiles" % (name, c, size, size, mib, e, n))
        for what in ("planes [C, H, W]", "gapped: %d channels of %d" % (c, c + 1)):
            if what.startswith("planes"):
                holder = hwc.permute(2, 0, 1).contiguous()
                view, holder_back = holder.permute(1, 2, 0), torch.zeros_like(holder)
                view_back = holder_back.permute(1, 2, 0)
            else:
                holder = torch.zeros((size, size, c + 1), dtype=hwc.dtype, device="cuda")
                holder[..., :c] = hwc
                view, holder_back = holder[..., :c], torch.zeros_like(holder)
                view_back = holder_back[..., :c]
            state = {}

            def enc_a():
                rc, offs, sizes, used = api.encode_raster_tiles_device_depth_strided(codec, view, None, e, tile, arena_a)
                assert rc == 0, (rc, codec.last_error())
                state["a"] = (offs, sizes, used)

            def enc_b():
                rc, offs, sizes, used = api.encode_raster_tiles_device_depth(codec, view.contiguous(), None, e, tile, arena_b)
                assert rc == 0, (rc, codec.last_error())
                state["b"] = (offs, sizes, used)

            def dec_a():
                assert api.decode_raster_tiles_device_depth_strided(codec, arena_a, state["a"][0], state["a"][1], view_back, None, tile) == 0

            def dec_b():
                assert api.decode_raster_tiles_device_depth(codec, arena_a, state["a"][0], state["a"][1], hwc_back, None, tile) == 0
                view_back.copy_(hwc_back)

            b0 = codec.tile_batch_counters()
            enc_a()
            b1 = codec.tile_batch_counters()
            enc_b()
            torch.cuda.synchronize()
            used = state["a"][2]
            assert used == state["b"][2] and (state["a"][0] == state["b"][0]).all() and (state["a"][1] == state["b"][1]).all(), "the tables differ"
            assert torch.equal(arena_a[:used], arena_b[:used]), "the blobs differ from the packed call's"
            dec_b()
            torch.cuda.synchronize()
            want = view_back.clone()
            view_back.zero_()
            dec_a()
            torch.cuda.synchronize()
            assert torch.equal(view_back.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), "the decodes differ"
            err = float((view_back.double() - view.double()).abs().max())
            assert err <= e + 1e-4, err
            (ea, eb), (da, db) = timed_pair(torch, enc_a, enc_b), timed_pair(torch, dec_a, dec_b)
            say("  %-28s %d blob bytes, tile batch counters of one encode %s, max error %.6f" % (what, used, [int(y - x) for x, y in zip(b0, b1)], err))
            say("    (a) strided call, no copy            encode %8.3f [%6.3f]   decode %8.3f [%6.3f]" % (ea + da))
            say("    (b) contiguous() + packed call       encode %8.3f [%6.3f]   decode %8.3f [%6.3f]" % (eb + db))
            say("    (b) - (a)                            encode %8.3f            decode %8.3f" % (eb[0] - ea[0], db[0] - da[0]))
            for way, a, b in (("encode", ea, eb), ("decode", da, db)):
                if a[0] > b[0]:
                    verdicts.append("%s x %d, %s, %s: (a) %.3f ms is SLOWER than (b) %.3f ms" % (name, c, what, way, a[0], b[0]))
            del holder, holder_back, view, view_back, want
            torch.cuda.empty_cache()
        # ---- windows of the mosaic into packed pixels
        rc, offs, sizes, used = api.encode_raster_tiles_device_depth(codec, hwc, None, e, tile, arena_a)
        assert rc == 0

        def whole():
            assert api.decode_raster_tiles_device_depth(codec, arena_a, offs, sizes, hwc_back, None, tile) == 0

        whole()
        torch.cuda.synchronize()
        ref = hwc_back.clone()
        say("  window (row0, col0, rows x cols)        tiles   window decode        whole decode + copy of the slice")
        points = []
        for wname, side in (("one tile", TILE), ("1/16", size // 4), ("1/4", size // 2), ("whole", size)):
            r0 = c0 = 0 if side == size else TILE * 3
            out = torch.zeros((side, side, c), dtype=hwc.dtype, device="cuda")
            touched = len(api.raster_window_tiles(size, size, tile, (r0, c0, side, side)))

            def win():
                assert api.decode_raster_window_device_depth(codec, arena_a, offs, sizes, (size, size), tile, (r0, c0), out, None) == 0

            def old():
                assert api.decode_raster_tiles_device_depth(codec, arena_a, offs, sizes, hwc_back, None, tile) == 0
                out.copy_(hwc_back[r0:r0 + side, c0:c0 + side])

            k0 = codec.raster_tiles_counters()
            win()
            torch.cuda.synchronize()
            assert [int(y - x) for x, y in zip(k0, codec.raster_tiles_counters())] == [0, 0, touched, 0]
            assert torch.equal(out.view(torch.uint8), ref[r0:r0 + side, c0:c0 + side].contiguous().view(torch.uint8)), "the window is not the slice"
            t_win, t_old = timed_pair(torch, win, old)
            points.append((touched, t_win[0]))
            say("  %-8s (%4d, %4d, %4d x %4d)   %5d   %8.3f [%6.3f]   %8.3f [%6.3f]" % ((wname, r0, c0, side, side, touched) + t_win + t_old))
            if 2 * touched < n and t_win[0] > t_old[0]:
                verdicts.append("%s x %d, window %s: %.3f ms is SLOWER than the whole decode and a slice, %.3f ms" % (name, c, wname, t_win[0], t_old[0]))
            del out
        mx, my = sum(p[0] for p in points) / len(points), sum(p[1] for p in points) / len(points)
        slope = sum((p[0] - mx) * (p[1] - my) for p in points) / sum((p[0] - mx) ** 2 for p in points)
        say("  window decode ~ %.3f ms + %.3f ms per thousand tiles (least squares through the four windows)" % (my - slope * mx, 1000 * slope))
        del hwc, hwc_back, arena_a, arena_b, ref
        torch.cuda.empty_cache()
    say("expectation: (a) no slower than (b), a window of under half the tiles faster than the whole decode and a slice -- %s"
        % ("met everywhere" if not verdicts else "NOT met:"))
    for v in verdicts:
        say("  " + v)
    codec.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


def nodata(out_path):
    """the noData raster calls (include/lerc_amd_nodata.h) against what a caller did before, see the module's text"""
    import numpy as np
    import torch
    from lerc_amd import api, synth
    assert torch.cuda.is_available(), "needs a GPU"
    tile = (TILE, TILE)
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    say("noData raster calls against a torch-made mask + the masked calls -- %s; tiles of %d x %d, packed arenas, about 10 %% holes; the ways "
        "alternating, median [interquartile range] of %d, ms" % (torch.cuda.get_device_name(0), TILE, TILE, REPS))
    slower = []
    for name, size, e in (("float32", 8192, E), ("uint16", 16384, 0.0)):
        terrain = synth.c2_float32(8192, 8192, device="cuda:0")
        if size > 8192:
            terrain = terrain.repeat(size // 8192, size // 8192) + torch.arange(size, device="cuda", dtype=torch.float32)[:, None] * 0.01
        yy = torch.arange(size, device="cuda", dtype=torch.float32)[:, None]
        xx = torch.arange(size, device="cuda", dtype=torch.float32)[None, :]
        f = torch.sin(yy / 97.0) * torch.cos(xx / 131.0) + 0.5 * torch.sin(yy / 41.0 + xx / 59.0)
        holes = f > torch.quantile(f[::16, ::16].reshape(-1), 0.9)
        del f, yy, xx
        if name == "float32":
            raster, nd = terrain.clone(), float("nan")
            raster[holes] = nd
            bits, nd_bits = raster, None
        else:
            lo, hi = float(terrain.min()), float(terrain.max())
            raster, nd = ((terrain - lo) * (60000.0 / (hi - lo))).to(torch.int32).to(torch.uint16), 65535.0
            bits, nd_bits = raster.view(torch.int16), -1    # (torch compares and fills 16-bit patterns as int16: a view, no copy)
            bits[holes] = nd_bits
        del terrain
        share = float(holes.float().mean())
        del holes
        item = raster.element_size()
        n = len(api.raster_tile_grid(size, size, tile))
        cap = n * (TILE * TILE * item + TILE * TILE // 4 + 2048)
        arena_a = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        arena_b = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        back_a, back_b = torch.zeros_like(raster), torch.zeros_like(raster)
        valid_back = torch.zeros((size, size), dtype=torch.uint8, device="cuda")
        say("%s, %d x %d (%.0f MiB), maxZErr %g, %d tiles, %.1f %% holes, noData %s" % (name, size, size, raster.numel() * item / 2 ** 20, e, n, 100 * share, nd))
        state = {}

        def enc_a():
            rc, offs, sizes, used = api.encode_raster_tiles_device_nodata(codec, raster, nd, e, tile, arena_a)
            assert rc == 0, (rc, codec.last_error())
            state["a"] = (offs, sizes, used)

        def enc_b():
            valid = (~torch.isnan(raster) if nd_bits is None else bits != nd_bits).to(torch.uint8)
            rc, offs, sizes, used = api.encode_raster_tile_range_device(codec, raster, valid, e, tile, (0, 0, size // TILE, size // TILE), arena_b)
            assert rc == 0, (rc, codec.last_error())
            state["b"] = (offs, sizes, used)

        def enc_c():
            rc, offs, sizes, used = api.encode_raster_tile_range_device(codec, raster, None, e, tile, (0, 0, size // TILE, size // TILE), arena_b)
            state["c"] = rc

        def dec_a():
            assert api.decode_raster_tiles_device_nodata(codec, arena_a, state["a"][0], state["a"][1], back_a, nd, tile) == 0

        def dec_b():
            assert api.decode_raster_tiles_device(codec, arena_b, state["b"][0], state["b"][1], back_b, valid_back, tile) == 0
            (back_b if nd_bits is None else back_b.view(torch.int16)).masked_fill_(valid_back == 0, nd if nd_bits is None else nd_bits)

        # blobs and pixels compared before anything is timed
        c0 = codec.tile_batch_counters()
        enc_a()
        c1 = codec.tile_batch_counters()
        enc_b()
        assert np.array_equal(state["a"][0], state["b"][0]) and np.array_equal(state["a"][1], state["b"][1]) and state["a"][2] == state["b"][2]
        assert torch.equal(arena_a[:state["a"][2]], arena_b[:state["b"][2]]), "the blobs of (a) and (b) differ"
        dec_a()
        dec_b()
        torch.cuda.synchronize()
        if nd_bits is None:
            assert torch.equal(torch.isnan(back_a), torch.isnan(back_b)) and torch.equal(torch.isnan(back_a), torch.isnan(raster))
            assert torch.equal(torch.nan_to_num(back_a), torch.nan_to_num(back_b)), "the pixels of (a) and (b) differ"
            assert float((torch.nan_to_num(back_a) - torch.nan_to_num(raster)).abs().max()) <= e + 1e-4    # (float32 rounding beside the bound)
        else:
            assert torch.equal(back_a.view(torch.int16), back_b.view(torch.int16)) and torch.equal(back_a.view(torch.int16), bits)
        say("  (a) tile batch counters of one encode: %d tiles in the batch's launches, %d one by one; %d blob bytes"
            % (c1[0] - c0[0], c1[1] - c0[1], state["a"][2]))
        ways = [("(a) the noData calls", enc_a, dec_a), ("(b) torch mask + masked calls, torch fill", enc_b, dec_b)]
        res = timed_ways(torch, [w[1] for w in ways]), timed_ways(torch, [w[2] for w in ways])
        for k, w in enumerate(ways):
            say("  %-44s encode %8.3f [%6.3f]   decode %8.3f [%6.3f]" % (w[0], res[0][k][0], res[0][k][1], res[1][k][0], res[1][k][1]))
        for which, r in zip(("encode", "decode"), res):
            say("  %s: (a) / (b) = %.3f" % (which, r[0][0] / r[1][0]))
            if r[0][0] > r[1][0]:
                slower.append("%s %s: (a) %.3f ms is slower than (b) %.3f ms" % (name, which, r[0][0], r[1][0]))
        if nd_bits is None:
            c0 = codec.tile_batch_counters()
            enc_c()
            c1 = codec.tile_batch_counters()
            m = timed_ways(torch, [enc_c], reps=max(3, REPS // 4), warm=1)[0]
            say("  %-44s encode %8.3f [%6.3f]   (status %d; %d tiles in the batch's launches, %d one by one; %d runs)"
                % ("(c) NaN holes, the unmasked call", m[0], m[1], state["c"], c1[0] - c0[0], c1[1] - c0[1], max(3, REPS // 4)))
        del raster, bits, arena_a, arena_b, back_a, back_b, valid_back
        torch.cuda.empty_cache()
    say("(a) no slower than (b): %s" % ("everywhere" if not slower else "NOT everywhere:"))
    for v in slower:
        say("  " + v)
    codec.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


def timed_ways(torch, fns, reps=REPS, warm=3):
    """the functions alternating inside one loop -> [(median, interquartile range)] in their order"""
    for _ in range(warm):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [(statistics.median(m), statistics.quantiles(m, n=4)[2] - statistics.quantiles(m, n=4)[0]) for m in ms]


def timed_pair(torch, fa, fb, reps=REPS, warm=3):
    """fa and fb alternating inside one loop -> ((median, interquartile range) of fa, of fb)"""
    for _ in range(warm):
        fa()
        fb()
    ms = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    out = []
    for m in ms:
        q = statistics.quantiles(m, n=4)
        out.append((statistics.median(m), q[2] - q[0]))
    return out[0], out[1]


def timed_on(torch, fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    q = statistics.quantiles(ms, n=4)
    return statistics.median(ms), q[2] - q[0]


def main():
    import numpy as np
    import torch
    from lerc_amd import api, synth
    assert torch.cuda.is_available(), "needs a GPU"

    def timed(fn, reps=REPS, warm=3):
        for _ in range(warm):
            fn()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        q = statistics.quantiles(ms, n=4)
        return statistics.median(ms), q[2] - q[0]

    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    print("raster tile calls against the tile calls -- %s; float32 at %.2f, tiles of %d x %d; median [interquartile range] of %d, ms"
          % (torch.cuda.get_device_name(0), E, TILE, TILE, REPS))
    ok = True
    for size in (8192, 8190):
        raster = synth.c2_float32(size, size, device="cuda:0")
        grid = api.raster_tile_grid(size, size, (TILE, TILE))
        n = len(grid)
        arena = torch.zeros(n * (TILE * TILE * 4 + TILE * TILE // 4 + 1024 + 16), dtype=torch.uint8, device="cuda")
        back = torch.zeros_like(raster)
        state = {}

        def enc_a():
            rc, offs, sizes, used = api.encode_raster_tiles_device(codec, raster, None, E, (TILE, TILE), arena)
            assert rc == 0, (rc, codec.last_error())
            state["a"] = (offs, sizes)

        def dec_a():
            assert api.decode_raster_tiles_device(codec, arena, state["a"][0], state["a"][1], back, None, (TILE, TILE)) == 0

        r0, b0 = codec.raster_tiles_counters(), codec.tile_batch_counters()
        enc_a()
        dec_a()
        torch.cuda.synchronize()
        r1, b1 = codec.raster_tiles_counters(), codec.tile_batch_counters()
        err = float((back.double() - raster.double()).abs().max())
        assert err <= E + 1e-4, err
        a_enc, a_dec = timed(enc_a), timed(dec_a)

        full = size // TILE
        tiles = raster[:full * TILE, :full * TILE].reshape(full, TILE, full, TILE).permute(0, 2, 1, 3).contiguous().reshape(full * full, TILE, TILE)
        tiles_back = torch.zeros_like(tiles)

        def enc_b():
            rc, offs, sizes, used = api.encode_tiles_device(codec, tiles, E, arena)
            assert rc == 0, (rc, codec.last_error())
            state["b"] = (offs, sizes)

        def dec_b():
            assert api.decode_tiles_device(codec, arena, state["b"][0], state["b"][1], tiles_back) == 0

        enc_b()
        dec_b()
        b_enc, b_dec = timed(enc_b), timed(dec_b)

        def copy_c():
            back.copy_(raster)

        c = timed(copy_c)
        print("%d x %d: %d tiles (%d interior); raster call counters [cut, in place, pasted, in place] %s, tile batch counters %s; max error %.6f"
              % (size, size, n, full * full, [int(y - x) for x, y in zip(r0, r1)], [int(y - x) for x, y in zip(b0, b1)], err))
        print("  (a) raster calls            encode %8.3f [%6.3f]   decode %8.3f [%6.3f]" % (a_enc + a_dec))
        print("  (b) tile calls, tiles cut   encode %8.3f [%6.3f]   decode %8.3f [%6.3f]" % (b_enc + b_dec))
        print("  (c) device-to-device copy of %.0f MiB   %8.3f [%6.3f]   (%.0f GB/s read + written)"
              % (raster.numel() * 4 / 2 ** 20, c[0], c[1], 2 * raster.numel() * 4 / c[0] / 1e6))
        for what, a, b in (("encode", a_enc[0], b_enc[0]), ("decode", a_dec[0], b_dec[0])):
            met = a - b <= 2 * c[0]
            print("  %s: (a) - (b) = %7.3f ms = %.2f x (c)%s" % (what, a - b, (a - b) / c[0],
                                                               "   target 2 x (c): %s" % ("met" if met else "NOT met") if size == 8192 else ""))
            if size == 8192:
                ok = ok and met
        del raster, arena, back, tiles, tiles_back
        torch.cuda.empty_cache()
    codec.close()
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1:2] == ["nodata"]:
        sys.exit(nodata(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "raster_nodata_time.txt")))
    if sys.argv[1:2] == ["depth"]:
        sys.exit(depth(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "raster_depth_layouts_time.txt")))
    sys.exit(interleaved() if sys.argv[1:] == ["interleaved"] else window() if sys.argv[1:] == ["window"] else main())
