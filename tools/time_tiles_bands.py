#!/usr/bin/env python3
"""Times the band stack tile batch calls (lerc_amd_encode_tiles_device_bands / lerc_amd_decode_tiles_device_bands), all device
resident, on one MI355X, on two mosaics of 256 tiles of 256^2 under the island mask (synth.island_mask: 98 tiles all valid, 76
empty, 82 partial), nMasks = 1:

  RGB     three uint8 bands derived from the byte mosaic (synth.byte_mosaic), lossless
  MS4     four uint16 bands derived from the uint16 island (synth.island), lossless

each (a) through the band stack calls of THIS build and (b) through one lerc_amd_encode_device / lerc_amd_decode_device call per
tile with nBands -- the only way a library built from the PARENT commit can do it (--parent-lib, or PARENT_LIB, loaded through
LERC_AMD_LIBRARY).  (b) is measured on this build and on the parent.  Pass line: per-tile / band stack call > 1 + 3 s, s the larger
relative interquartile range of the two.

The same run repeats the single-band lines of tools/time_tiles_masked.py and tools/time_tiles_bytes.py (the float32 and uint16
islands and the byte island through the _masked calls, the byte mosaic through the unmasked calls; packed) on both libraries: the
existing calls did not pay for the new arguments if parent / this build >= 1 - 3 s.

Every library is measured in a fresh process of its own (this script with --measure).  Warm-up, then the median and the
interquartile range of REPS (21) repetitions, HIP events around the calls.  Writes profiles/tiles_bands_time.txt.  Run it under a time
limit of its own:  timeout -k 10 900 python tools/time_tiles_bands.py --parent-lib ...
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
    have_bands = hasattr(codec.lib, "lerc_amd_encode_tiles_device_bands")
    masks_np = synth.cut_tiles(synth.island_mask(4096), 256)
    res = {"device": torch.cuda.get_device_name(0), "have_bands": have_bands}

    # ---- band stacks
    byte = synth.byte_mosaic(4096, 256)
    rgb = np.stack([byte, 255 - byte, (byte // 2 + 17).astype(np.uint8)], axis=1)
    u16, _, _ = synth.island("uint16", 4096, 256)
    ms4 = np.stack([u16, u16 + 100, (u16 // 2).astype(np.uint16), np.roll(u16, 7, axis=2)], axis=1).astype(np.uint16)
    for name, stack_np in (("rgb", rgb), ("ms4", ms4)):
        n, nb, r, c = stack_np.shape
        item = stack_np.itemsize
        dt = api._dt_code(stack_np.dtype)
        tiles = torch.from_numpy(stack_np.view(np.uint8).copy()).cuda()    # (bytes: torch has no uint16 everywhere)
        valid = torch.from_numpy(masks_np.copy()).cuda()
        slot = (nb * (r * c * item + r * c // 4 + 1024) + 15) & ~15
        arena = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
        out = torch.zeros(n * nb * r * c * item, dtype=torch.uint8, device="cuda")
        valid_out = torch.zeros((n, r, c), dtype=torch.uint8, device="cuda")
        tile_bytes = nb * r * c * item
        state = {}

        def enc_bands():
            rc, offs, sizes, used = codec.encode_tiles_bands(tiles.data_ptr(), dt, c, r, nb, n, 1, valid.data_ptr(), 0, arena.data_ptr(), arena.numel())
            assert rc == 0, rc
            state["bands"] = (offs, sizes)

        def dec_bands():
            offs, sizes = state["bands"]
            assert codec.decode_tiles_bands(arena.data_ptr(), offs, sizes, n, c, r, nb, dt, out.data_ptr(), 1, valid_out.data_ptr()) == 0

        def enc_each():
            sizes = np.zeros(n, np.uint32)
            for t in range(n):
                rc, sizes[t] = codec.encode(tiles.data_ptr() + t * tile_bytes, dt, 1, c, r, nb, 0, arena.data_ptr() + t * slot, slot,
                                            valid.data_ptr() + t * r * c, 1)
                assert rc == 0, rc
            state["each"] = sizes

        def dec_each():
            sizes = state["each"]
            for t in range(n):
                assert codec.decode(arena.data_ptr() + t * slot, int(sizes[t]), dt, 1, c, r, nb, out.data_ptr() + t * tile_bytes,
                                    valid_out.data_ptr() + t * r * c, 1) == 0

        def round_trip_ok():
            got = out.cpu().numpy().view(stack_np.dtype).reshape(stack_np.shape)
            m = np.broadcast_to(masks_np[:, None] > 0, stack_np.shape)
            return np.array_equal(valid_out.cpu().numpy(), masks_np) and np.array_equal(got[m], stack_np[m])

        enc_each()
        dec_each()
        assert round_trip_ok(), "the per-tile round trip is not lossless"
        res[name] = {"tiles": n, "bands": nb, "mpix": n * nb * r * c / 1e6, "enc_each": timed(enc_each), "dec_each": timed(dec_each)}
        if have_bands:
            out.zero_()
            c0 = codec.tile_batch_counters()
            enc_bands()
            dec_bands()
            c1 = codec.tile_batch_counters()
            assert round_trip_ok(), "the band stack round trip is not lossless"
            res[name]["counters"] = [int(c1[i] - c0[i]) for i in range(4)]
            res[name]["enc_bands"] = timed(enc_bands)
            res[name]["dec_bands"] = timed(dec_bands)

    # ---- the single-band lines: the islands and the byte island through the _masked calls, the byte mosaic unmasked; packed
    single = {}
    for name in ("float32", "uint16", "byte_island", "byte_mosaic"):
        if name in ("float32", "uint16"):
            t_np, m_np, e = synth.island(name, 4096, 256)
        else:
            t_np, m_np, e = byte, (masks_np if name == "byte_island" else None), 0
        n, r, c = t_np.shape
        if t_np.dtype == np.uint16 and not hasattr(torch, "uint16"):
            continue
        tiles = torch.from_numpy(t_np.copy()).cuda()
        valid = torch.from_numpy(m_np.copy()).cuda() if m_np is not None else None
        arena = torch.zeros(n * (t_np[0].nbytes + r * c // 4 + 1024), dtype=torch.uint8, device="cuda")
        out = torch.zeros_like(tiles)
        valid_out = torch.zeros((n, r, c), dtype=torch.uint8, device="cuda") if m_np is not None else None
        state = {}

        def enc():
            rc, offs, sizes, used = api.encode_tiles_device_masked(codec, tiles, valid, e, arena)
            assert rc == 0, rc
            state["at"] = (offs, sizes)

        def dec():
            offs, sizes = state["at"]
            assert api.decode_tiles_device_masked(codec, arena, offs, sizes, out, valid_out) == 0

        enc()
        dec()
        single[name] = {"enc": timed(enc), "dec": timed(dec)}
    res["single"] = single
    codec.close()
    print("RESULT " + json.dumps(res))
    return 0


def child(lib):
    env = dict(os.environ)
    env.pop("LERC_AMD_LIBRARY", None)
    if lib:
        env["LERC_AMD_LIBRARY"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure"], env=env, capture_output=True, text=True, timeout=800)
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
    assert a["have_bands"] and not b["have_bands"], "this build has the band stack calls, the parent has not"
    lines = ["band stack tile batches on the island -- %s" % a["device"],
             "256 tiles of 256 x 256 under the island mask, nMasks 1, lossless; median [interquartile range] of %d, ms" % REPS,
             "(a) this build, the band stack calls; (b) this build, one lerc_amd_encode_device / lerc_amd_decode_device call per tile; (c) the parent commit, the same per-tile calls"]
    ok = True

    def ratio_line(label, fast, slow, faster):
        nonlocal ok
        spread = max(fast["iqr"] / fast["median"], slow["iqr"] / slow["median"])
        ratio = slow["median"] / fast["median"]
        met = ratio > 1 + 3 * spread if faster else ratio >= 1 - 3 * spread
        ok = ok and met
        return "  %-34s %9.3f [%7.3f]   against %9.3f [%7.3f]   ratio %7.2f   pass line 1 %s 3 x %.4f: %s" % (
            label, fast["median"], fast["iqr"], slow["median"], slow["iqr"], ratio, "+" if faster else "-", spread, "met" if met else "NOT met")

    for name, label in (("rgb", "RGB, 3 x uint8"), ("ms4", "MS4, 4 x uint16")):
        ra, rb = a[name], b[name]
        lines.append("%s (%.1f Mpixel a band stack mosaic): %d tiles encoded by the batch's launches, %d one by one; %d / %d decoded"
                     % ((label, ra["mpix"]) + tuple(ra["counters"])))
        lines.append(ratio_line("encode, (a) against (b)", ra["enc_bands"], ra["enc_each"], True))
        lines.append(ratio_line("encode, (a) against (c)", ra["enc_bands"], rb["enc_each"], True))
        lines.append(ratio_line("decode, (a) against (b)", ra["dec_bands"], ra["dec_each"], True))
        lines.append(ratio_line("decode, (a) against (c)", ra["dec_bands"], rb["dec_each"], True))
    lines.append("single-band calls, packed: this build against the parent commit (no slower: parent / this build >= 1 - 3 s)")
    for name in a["single"]:
        for way in ("enc", "dec"):
            lines.append(ratio_line("%s %s" % (name, "encode" if way == "enc" else "decode"), a["single"][name][way], b["single"][name][way], False))
    lines.append("pass lines met: %s" % ("yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text)
    out_dir = os.environ.get("TILES_BANDS_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "tiles_bands_time.txt"), "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
