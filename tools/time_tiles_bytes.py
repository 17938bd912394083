#!/usr/bin/env python3
"""Times the 8-bit tile batch calls on the byte mosaic (16 x 16 uint8 tiles of 256^2: channel 0 of the C4 raster, lossless), all
device resident, on one MI355X:

  (a) lerc_amd_encode_tiles_device / _slots and their decoding counterparts of THIS build
  (b) the same calls on a library built from the PARENT commit (--parent-lib, or PARENT_LIB), loaded through LERC_AMD_LIBRARY

and the MASKED case: the byte island -- the same mosaic under synth.island_mask (98 tiles all valid, 76 empty, 82 partial) --
through lerc_amd_encode_tiles_device_masked / lerc_amd_decode_tiles_device_masked, packed.  The parent does every such tile one by one.

each in a fresh process of its own (this script with --measure).  Build the parent with
  git worktree add /some/scratch/parent HEAD~1 && make -C /some/scratch/parent/lerc_amd/csrc

Warm-up, then the median and the interquartile range of REPS (21) repetitions, HIP events around the calls.  The pass lines, with s the
larger relative interquartile range of the two runs: masked, (b) / (a) > 1 + 3 s each way (this build is faster); all valid,
(b) / (a) >= 1 - 3 s (this build is no slower).  Writes
profiles/tiles_bytes_time.txt.  Run it under a time limit of its own:  timeout -k 10 600 python tools/time_tiles_bytes.py --parent-lib ...
"""
import argparse
import ctypes as ct
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

    tiles_np = synth.byte_mosaic(4096, 256)
    n, r, c = tiles_np.shape
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    tiles = torch.from_numpy(tiles_np.copy()).cuda()
    slot = (r * c + r * c // 4 + 1024 + 15) & ~15
    arena = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, r, c), dtype=torch.uint8, device="cuda")
    state = {}

    def enc_packed():
        rc, offs, sizes, used = api.encode_tiles_device(codec, tiles, 0, arena)
        assert rc == 0, rc
        state["packed"] = (offs, sizes)

    def dec_packed():
        offs, sizes = state["packed"]
        assert api.decode_tiles_device(codec, arena, offs, sizes, out) == 0

    def enc_slots():
        rc, sizes = api.encode_tiles_device_slots(codec, tiles, 0, arena, slot)
        assert rc == 0, rc
        state["slots"] = sizes

    def dec_slots():
        assert api.decode_tiles_device_slots(codec, arena, slot, state["slots"], out) == 0

    c0 = codec.tile_batch_counters()
    enc_packed()
    dec_packed()
    c1 = codec.tile_batch_counters()
    assert np.array_equal(out.cpu().numpy(), tiles_np), "the round trip is not lossless"
    res = {"device": torch.cuda.get_device_name(0), "tiles": n, "mpix": n * r * c / 1e6,
           "counters": [int(c1[i] - c0[i]) for i in range(4)],
           "enc_packed": timed(enc_packed), "dec_packed": timed(dec_packed)}
    res["enc_slots"] = timed(enc_slots)
    res["dec_slots"] = timed(dec_slots)

    # ---- the masked case: the byte island
    masks_np = synth.cut_tiles(synth.island_mask(4096), 256)
    valid = torch.from_numpy(masks_np.copy()).cuda()
    valid_out = torch.zeros((n, r, c), dtype=torch.uint8, device="cuda")

    def enc_masked():
        rc, offs, sizes, used = api.encode_tiles_device_masked(codec, tiles, valid, 0, arena)
        assert rc == 0, rc
        state["masked"] = (offs, sizes)

    def dec_masked():
        offs, sizes = state["masked"]
        assert api.decode_tiles_device_masked(codec, arena, offs, sizes, out, valid_out) == 0

    c0 = codec.tile_batch_counters()
    enc_masked()
    dec_masked()
    c1 = codec.tile_batch_counters()
    assert np.array_equal(valid_out.cpu().numpy(), masks_np) and np.array_equal(out.cpu().numpy()[masks_np > 0], tiles_np[masks_np > 0])
    res["masked_counters"] = [int(c1[i] - c0[i]) for i in range(4)]
    res["enc_masked"] = timed(enc_masked)
    res["dec_masked"] = timed(dec_masked)
    codec.lib.lerc_amd_profile_enable.argtypes = [ct.c_void_p, ct.c_int]
    codec.lib.lerc_amd_profile_read.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int]
    codec.lib.lerc_amd_profile_enable(codec.h, 1)
    enc_packed()
    dec_packed()
    enc_masked()
    dec_masked()
    buf = ct.create_string_buffer(8192)
    codec.lib.lerc_amd_profile_read(codec.h, buf, 8192, 1)
    codec.lib.lerc_amd_profile_enable(codec.h, 0)
    res["profile"] = buf.value.decode().splitlines()
    codec.close()
    print("RESULT " + json.dumps(res))
    return 0


def child(lib):
    env = dict(os.environ)
    env.pop("LERC_AMD_LIBRARY", None)
    if lib:
        env["LERC_AMD_LIBRARY"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure"], env=env, capture_output=True, text=True, timeout=540)
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
    lines = ["8-bit tile batches on the byte mosaic -- %s" % a["device"],
             "%d uint8 tiles of 256 x 256, lossless (%.1f Mpixel); median [interquartile range] of %d, ms; (a) this build, (b) the parent commit"
             % (a["tiles"], a["mpix"], REPS)]
    for name, r in (("a", a), ("b", b)):
        lines.append("  (%s) one round trip, all valid: %d tiles encoded by the batch's launches, %d one by one; %d / %d decoded" % ((name,) + tuple(r["counters"])))
        lines.append("  (%s) one round trip, the island: %d tiles encoded by the batch's launches, %d one by one; %d / %d decoded"
                     % ((name,) + tuple(r["masked_counters"])))
    ok = True
    for key, label, faster in (("enc_packed", "encode, packed ", False), ("dec_packed", "decode, packed ", False), ("enc_slots", "encode, slotted", False),
                               ("dec_slots", "decode, slotted", False), ("enc_masked", "encode, island ", True), ("dec_masked", "decode, island ", True)):
        ma, mb = a[key], b[key]
        spread = max(ma["iqr"] / ma["median"], mb["iqr"] / mb["median"])
        ratio = mb["median"] / ma["median"]
        met = ratio > 1 + 3 * spread if faster else ratio >= 1 - 3 * spread
        ok = ok and met
        lines.append("  %s  (a) %9.3f [%7.3f] %9.1f MPix/s   (b) %9.3f [%7.3f] %9.1f MPix/s   (b)/(a) %7.2f   pass line 1 %s 3 x %.4f: %s"
                     % (label, ma["median"], ma["iqr"], a["mpix"] / ma["median"] * 1e3, mb["median"], mb["iqr"], a["mpix"] / mb["median"] * 1e3,
                        ratio, "+" if faster else "-", spread, "met" if met else "NOT met"))
    lines.append("  profile groups of one (a) encode + decode, all valid and island (group, ms, launches):")
    lines += ["    " + ln for ln in a["profile"]]
    lines.append("pass line met: %s" % ("yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text)
    out_dir = os.environ.get("TILES_BYTES_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "tiles_bytes_time.txt"), "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
