#!/usr/bin/env python3
"""Times the tile batch calls on tiles of 512 x 512 -- which the batches' own launches take since their size limits rose to 264 192
pixels and 4 352 blocks a tile (tile_batch.h) -- against a library built from the PARENT commit, where the same calls do such tiles
one by one inside (--parent-lib, or PARENT_LIB, loaded through LERC_AMD_LIBRARY).  All device resident, one MI355X, packed arenas.

The 4 096^2 island (synth.island, synth.byte_mosaic under synth.island_mask), nMasks 1, cut two ways in the same run:

  64 tiles of 512^2     new ground: pass line  parent / this build > 1 + 3 s
  256 tiles of 256^2    old ground: pass line  parent / this build >= 1 - 3 s      (s: the larger relative interquartile range)

in six configurations: masked float32 (maxZErr 0.01), masked uint16, masked uint8 (lossless), the byte mosaic with every pixel valid
and no mask pointer (the unmasked 8-bit batch), RGB stacks of three uint8 bands and stacks of four uint16 bands -- the configurations of
tools/time_tiles_masked.py, time_tiles_bytes.py and time_tiles_bands.py.  The time per pixel of the two cuts on this build stands side by side: the
phases that are serial per tile (the mask's run-length coder, the masked un-delta of a delta Huffman tile) get four times longer at 512^2.

Every library is measured in a fresh process of its own (this script with --measure).  Warm-up, then the median and the
interquartile range of REPS (21) repetitions, HIP events around the calls; the counters of one round trip beside them.  Writes
profiles/tiles_large_time.txt.  Run it under a time limit of its own (each of the two measuring
processes has 420 s):  timeout -k 10 900 python tools/time_tiles_large.py --parent-lib ...
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = int(os.environ.get("REPS", "21"))
CONFIGS = ("float32", "uint16", "uint8", "mosaic8", "rgb", "ms4")
LABEL = {"float32": "masked float32, 0.01", "uint16": "masked uint16", "uint8": "masked uint8", "mosaic8": "uint8, every pixel valid", "rgb": "RGB, 3 x uint8", "ms4": "MS4, 4 x uint16"}


def measure():
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
        return {"median": statistics.median(ms), "iqr": q[2] - q[0]}

    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    res = {"device": torch.cuda.get_device_name(0)}
    for tile in (512, 256):
        masks_np = synth.cut_tiles(synth.island_mask(4096), tile)
        byte = synth.byte_mosaic(4096, tile)
        u16, _, _ = synth.island("uint16", 4096, tile)
        f32, _, e32 = synth.island("float32", 4096, tile)
        stacks = {
            "float32": (f32[:, None], e32), "uint16": (u16[:, None], 0), "uint8": (byte[:, None], 0), "mosaic8": (byte[:, None], 0),
            "rgb": (np.stack([byte, 255 - byte, (byte // 2 + 17).astype(np.uint8)], axis=1), 0),
            "ms4": (np.stack([u16, u16 + 100, (u16 // 2).astype(np.uint16), np.roll(u16, 7, axis=2)], axis=1).astype(np.uint16), 0),
        }
        for name in CONFIGS:
            stack_np, e = stacks[name]
            stack_np = np.ascontiguousarray(stack_np)
            n, nb, r, c = stack_np.shape
            item = stack_np.itemsize
            dt = api._dt_code(stack_np.dtype)
            tiles = torch.from_numpy(stack_np.view(np.uint8).copy()).cuda()    # (bytes: torch has no uint16 everywhere)
            valid = torch.from_numpy(masks_np.copy()).cuda()
            arena = torch.zeros(n * ((nb * (r * c * item + r * c // 4 + 1024) + 15) & ~15), dtype=torch.uint8, device="cuda")
            out = torch.zeros(n * nb * r * c * item, dtype=torch.uint8, device="cuda")
            valid_out = torch.zeros((n, r, c), dtype=torch.uint8, device="cuda")
            nm = 0 if name == "mosaic8" else 1    # (no mask: the unmasked 8-bit batch behind the same call)
            state = {}

            def enc():
                rc, offs, sizes, used = codec.encode_tiles_bands(tiles.data_ptr(), dt, c, r, nb, n, nm, valid.data_ptr() if nm else None, e, arena.data_ptr(), arena.numel())
                assert rc == 0, rc
                state["at"] = (offs, sizes)

            def dec():
                offs, sizes = state["at"]
                assert codec.decode_tiles_bands(arena.data_ptr(), offs, sizes, n, c, r, nb, dt, out.data_ptr(), nm, valid_out.data_ptr() if nm else None) == 0

            c0 = codec.tile_batch_counters()
            enc()
            dec()
            c1 = codec.tile_batch_counters()
            got = out.cpu().numpy().view(stack_np.dtype).reshape(stack_np.shape)
            m = np.broadcast_to(masks_np[:, None] > 0, stack_np.shape) if nm else np.ones(stack_np.shape, bool)
            assert not nm or np.array_equal(valid_out.cpu().numpy(), masks_np), "the valid bytes did not come back"
            if e == 0:
                assert np.array_equal(got[m], stack_np[m]), "the round trip is not lossless"
            else:
                # (the bound holds for the double the decoder computes; the float32 it is stored as lies within half an ulp of that)
                assert np.abs(got[m].astype(np.float64) - stack_np[m]).max() <= e + 1e-4, "the round trip misses the error bound"
            res["%s_%d" % (name, tile)] = {"tiles": n, "mpix": n * nb * r * c / 1e6, "counters": [int(c1[i] - c0[i]) for i in range(4)],
                                           "enc": timed(enc), "dec": timed(dec)}
    codec.close()
    print("RESULT " + json.dumps(res))
    return 0


def child(lib):
    env = dict(os.environ)
    env.pop("LERC_AMD_LIBRARY", None)
    if lib:
        env["LERC_AMD_LIBRARY"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure"], env=env, capture_output=True, text=True, timeout=420)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit("the measuring process failed (exit %d): no second try" % p.returncode)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--parent-lib", default=os.environ.get("PARENT_LIB", ""))
    args = ap.parse_args()
    if args.measure:
        return measure()
    assert args.parent_lib and os.path.exists(args.parent_lib), "--parent-lib: liblerc_amd.so built from the parent commit"
    a = child("")
    b = child(os.path.abspath(args.parent_lib))
    lines = ["tile batches on tiles of 512 x 512 -- %s" % a["device"],
             "the 4 096^2 island under its mask, nMasks 1, packed; median [interquartile range] of %d, ms; this build against the parent commit" % REPS]
    ok = True

    def ratio_line(label, fast, slow, faster):
        nonlocal ok
        spread = max(fast["iqr"] / fast["median"], slow["iqr"] / slow["median"])
        ratio = slow["median"] / fast["median"]
        met = ratio > 1 + 3 * spread if faster else ratio >= 1 - 3 * spread
        ok = ok and met
        return "  %-34s %9.3f [%7.3f]   against %9.3f [%7.3f]   ratio %7.2f   pass line 1 %s 3 x %.4f: %s" % (
            label, fast["median"], fast["iqr"], slow["median"], slow["iqr"], ratio, "+" if faster else "-", spread, "met" if met else "NOT met")

    for tile, faster, head in ((512, True, "new ground: 64 tiles of 512 x 512 (the parent does them one by one inside the call)"),
                               (256, False, "old ground: 256 tiles of 256 x 256 (the small forms of the kernels, on both)")):
        lines.append(head)
        for name in CONFIGS:
            ra, rb = a["%s_%d" % (name, tile)], b["%s_%d" % (name, tile)]
            lines.append("%s (%.1f Mpixel): this build %d / %d encoded by the batch's launches / one by one, %d / %d decoded; the parent %d / %d, %d / %d"
                         % ((LABEL[name], ra["mpix"]) + tuple(ra["counters"]) + tuple(rb["counters"])))
            lines.append(ratio_line("encode", ra["enc"], rb["enc"], faster))
            lines.append(ratio_line("decode", ra["dec"], rb["dec"], faster))
    lines.append("this build, ps a pixel (all bands), 512 x 512 beside 256 x 256: what the phases that are serial per tile cost")
    for name in CONFIGS:
        big, small = a["%s_512" % name], a["%s_256" % name]
        lines.append("  %-24s encode %7.3f against %7.3f (x %.2f)   decode %7.3f against %7.3f (x %.2f)" % (
            LABEL[name], big["enc"]["median"] * 1e3 / big["mpix"], small["enc"]["median"] * 1e3 / small["mpix"],
            big["enc"]["median"] / big["mpix"] / (small["enc"]["median"] / small["mpix"]),
            big["dec"]["median"] * 1e3 / big["mpix"], small["dec"]["median"] * 1e3 / small["mpix"],
            big["dec"]["median"] / big["mpix"] / (small["dec"]["median"] / small["mpix"])))
    lines.append("pass lines met: %s" % ("yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text)
    out_dir = os.environ.get("TILES_LARGE_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "tiles_large_time.txt"), "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
