#!/usr/bin/env python3
"""Times the masked tile batch calls on the island mosaic (16 x 16 tiles of 256^2 cut from a 4096^2 raster, a disc of valid pixels
minus salt holes; float32 at MaxZError 0.01 and uint16 lossless), all device resident, in one process on one MI355X:

  (a) lerc_amd_encode_tiles_device_masked / lerc_amd_decode_tiles_device_masked
  (b) what a caller had to do without them: lerc_amd_encode_device / lerc_amd_decode_device with nMasks = 1, once per tile,
      on the same context
  (c) for scale: the unmasked batch calls on the same pixels, masks dropped

Median of REPS repetitions after a warm-up with the interquartile range beside it, HIP events around the calls, plus a wall-clock
figure for the whole run.  Writes profiles/tiles_masked_time.txt (or into TILES_MASKED_OUT).  Run it under a time limit of its own:
    timeout -k 10 600 python tools/time_tiles_masked.py [--parent-lib lerc_amd/csrc/_var/parent.so]
--parent-lib: a library built from the parent commit (REV=HEAD~1 tools/build_variant.sh parent).  The script then measures that
library and this build in a fresh child process each (itself with --measure; the parent through LERC_AMD_LIBRARY), writes both sets
of lines, the ratios parent / this build of (a) and the hand-back counts.  The pass line of that comparison: for both kinds and both
directions the ratio exceeds 1 by more than three times the larger relative interquartile range of the two runs.
"""
import ctypes as ct
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = int(os.environ.get("REPS", "21"))


def timed(fn, reps=REPS, warm=2):
    import torch
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


def run(kind, lines, figures):
    import numpy as np
    import torch
    from lerc_amd import api, synth
    tiles_np, masks_np, e = synth.island(kind)
    n, r, c = tiles_np.shape
    item = tiles_np.itemsize
    dt = [np.dtype(t) for t in api._DT_NP].index(tiles_np.dtype)
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    tiles = torch.from_numpy(tiles_np.view(np.uint8).reshape(n, -1).copy()).cuda()
    masks = torch.from_numpy(masks_np.reshape(n, -1).copy()).cuda()
    slot = (r * c * item + r * c // 4 + 1024 + 15) & ~15
    arena = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
    out = torch.zeros(n * r * c * item, dtype=torch.uint8, device="cuda")
    valid = torch.zeros(n * r * c, dtype=torch.uint8, device="cuda")
    state = {}

    def enc_a():
        rc, offs, sizes, used = codec.encode_tiles_masked(tiles.data_ptr(), dt, c, r, n, masks.data_ptr(), e, arena.data_ptr(), arena.numel())
        assert rc == 0, rc
        state["a"] = (offs, sizes)

    def dec_a():
        offs, sizes = state["a"]
        assert codec.decode_tiles_masked(arena.data_ptr(), offs, sizes, n, c, r, dt, out.data_ptr(), valid.data_ptr()) == 0

    def enc_b():
        sizes = np.zeros(n, np.uint32)
        for t in range(n):
            rc, nb = codec.encode(tiles.data_ptr() + t * r * c * item, dt, 1, c, r, 1, e, arena.data_ptr() + t * slot, slot,
                                  d_mask=masks.data_ptr() + t * r * c, n_masks=1)
            assert rc == 0, rc
            sizes[t] = nb
        state["b"] = sizes

    def dec_b():
        sizes = state["b"]
        for t in range(n):
            rc = codec.decode(arena.data_ptr() + t * slot, int(sizes[t]), dt, 1, c, r, 1, out.data_ptr() + t * r * c * item,
                              d_mask=valid.data_ptr() + t * r * c, n_masks=1)
            assert rc == 0, rc

    def enc_c():
        rc, offs, sizes, used = codec.encode_tiles_masked(tiles.data_ptr(), dt, c, r, n, 0, e, arena.data_ptr(), arena.numel())
        assert rc == 0, rc
        state["c"] = (offs, sizes)

    def dec_c():
        offs, sizes = state["c"]
        assert codec.decode_tiles_masked(arena.data_ptr(), offs, sizes, n, c, r, dt, out.data_ptr(), 0) == 0

    c0 = codec.tile_batch_counters()
    enc_a()
    dec_a()
    c1 = codec.tile_batch_counters()
    res = {}
    for name, fe, fd in (("a", enc_a, dec_a), ("b", enc_b, dec_b), ("c", enc_c, dec_c)):
        res[name] = (timed(fe), timed(fd))
    mp = n * r * c / 1e6
    lines.append("%s, %d tiles of %d x %d, MaxZError %g (%.1f Mpixel); median of %d, ms" % (kind, n, r, c, e, mp, REPS))
    lines.append("  one batch: %d tiles encoded by the batch's launches, %d one by one; %d / %d decoded" %
                 (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2], c1[3] - c0[3]))
    iqr = {k: (v[0][1], v[1][1]) for k, v in res.items()}
    res = {k: (v[0][0], v[1][0]) for k, v in res.items()}
    for name, text in (("a", "(a) masked batch calls           "), ("b", "(b) one call per tile, nMasks = 1"), ("c", "(c) unmasked batch, masks dropped")):
        lines.append("  %s encode %8.3f (iqr %.3f)   decode %8.3f (iqr %.3f)" % (text, res[name][0], iqr[name][0], res[name][1], iqr[name][1]))
    lines.append("  (b)/(a): encode %.2f, decode %.2f   (pass line: >= 1.1 each)" % (res["b"][0] / res["a"][0], res["b"][1] / res["a"][1]))
    lines.append("  (a)/(c): encode %.2f, decode %.2f" % (res["a"][0] / res["c"][0], res["a"][1] / res["c"][1]))
    ok = res["b"][0] / res["a"][0] >= 1.1 and res["b"][1] / res["a"][1] >= 1.1
    figures[kind] = {"encode": {"median": res["a"][0], "iqr": iqr["a"][0]}, "decode": {"median": res["a"][1], "iqr": iqr["a"][1]},
                     "single": [c1[1] - c0[1], c1[3] - c0[3]]}
    # where the time of (a) goes, by profile group
    codec.lib.lerc_amd_profile_enable.argtypes = [ct.c_void_p, ct.c_int]
    codec.lib.lerc_amd_profile_read.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int]
    codec.lib.lerc_amd_profile_enable(codec.h, 1)
    enc_a()
    dec_a()
    buf = ct.create_string_buffer(8192)
    codec.lib.lerc_amd_profile_read(codec.h, buf, 8192, 1)
    codec.lib.lerc_amd_profile_enable(codec.h, 0)
    lines.append("  profile groups of one (a) encode + decode (group, ms, launches):")
    for ln in buf.value.decode().splitlines():
        lines.append("    " + ln)
    codec.close()
    return ok


def measure(label):
    """one build, this process -> (lines, figures of (a), (b)/(a) line met)"""
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    t0 = time.time()
    lines = ["masked tile batches on the island mosaic -- %s -- %s" % (torch.cuda.get_device_name(0), label)]
    figures = {}
    ok = True
    for kind in ("float32", "uint16"):
        ok = run(kind, lines, figures) and ok
    lines.append("wall clock of the whole run: %.1f s" % (time.time() - t0))
    lines.append("(b)/(a) line met: %s" % ("yes" if ok else "NO"))
    return lines, figures, ok


def child(label, library):
    env = dict(os.environ)
    if library:
        env["LERC_AMD_LIBRARY"] = os.path.abspath(library)
    else:
        env.pop("LERC_AMD_LIBRARY", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", label], env=env, stdout=subprocess.PIPE, timeout=280, check=True)
    return json.loads(out.stdout.decode().strip().splitlines()[-1])


def main():
    if "--measure" in sys.argv:
        lines, figures, ok = measure(sys.argv[sys.argv.index("--measure") + 1])
        print(json.dumps({"lines": lines, "figures": figures, "ok": ok}))
        return 0
    parent_lib = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else os.environ.get("PARENT_LIB")
    if parent_lib:
        before, after = child("parent commit", parent_lib), child("this build", None)
        lines = before["lines"] + [""] + after["lines"] + ["", "parent / this build, (a) masked batch calls (pass line: ratio > 1 + 3 x the larger relative iqr):"]
        ok = True
        for kind in ("float32", "uint16"):
            for way in ("encode", "decode"):
                p, t = before["figures"][kind][way], after["figures"][kind][way]
                ratio = p["median"] / t["median"]
                rel = max(p["iqr"] / p["median"], t["iqr"] / t["median"])
                met = ratio > 1 + 3 * rel
                ok = ok and met
                lines.append("  %-8s %s: %8.3f / %8.3f = %6.2f   larger relative iqr %.4f   line 1 + 3 x = %.3f   %s"
                             % (kind, way, p["median"], t["median"], ratio, rel, 1 + 3 * rel, "met" if met else "NOT MET"))
            lines.append("  %-8s tiles one by one (encode, decode): parent %s, this build %s" % (kind, before["figures"][kind]["single"], after["figures"][kind]["single"]))
        lines.append("pass line met: %s" % ("yes" if ok else "NO"))
    else:
        lines, _, ok = measure("this build")
    text = "\n".join(lines) + "\n"
    print(text)
    out_dir = os.environ.get("TILES_MASKED_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "tiles_masked_time.txt"), "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
