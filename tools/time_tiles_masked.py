#!/usr/bin/env python3
"""Times the masked tile batch calls on the island mosaic (16 x 16 tiles of 256^2 cut from a 4096^2 raster, a disc of valid pixels
minus salt holes; float32 at MaxZError 0.01 and uint16 lossless), all device resident, in one process on one MI355X:

  (a) lerc_amd_encode_tiles_device_masked / lerc_amd_decode_tiles_device_masked
  (b) what a caller had to do without them: lerc_amd_encode_device / lerc_amd_decode_device with nMasks = 1, once per tile,
      on the same context
  (c) for scale: the unmasked batch calls on the same pixels, masks dropped

Median of REPS repetitions after a warm-up, HIP events around the calls, plus a wall-clock figure for the whole run.  Writes
profiles/tiles_masked_time.txt.  Run it under a time limit of its own:  timeout -k 10 600 python tools/time_tiles_masked.py
"""
import ctypes as ct
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lerc_amd import api, synth    # noqa: E402

REPS = int(os.environ.get("REPS", "21"))


def timed(fn, reps=REPS, warm=2):
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
    return statistics.median(ms)


def run(kind, lines):
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
    lines.append("  (a) masked batch calls            encode %8.3f   decode %8.3f" % res["a"])
    lines.append("  (b) one call per tile, nMasks = 1 encode %8.3f   decode %8.3f" % res["b"])
    lines.append("  (c) unmasked batch, masks dropped encode %8.3f   decode %8.3f" % res["c"])
    lines.append("  (b)/(a): encode %.2f, decode %.2f   (pass line: >= 1.1 each)" % (res["b"][0] / res["a"][0], res["b"][1] / res["a"][1]))
    lines.append("  (a)/(c): encode %.2f, decode %.2f" % (res["a"][0] / res["c"][0], res["a"][1] / res["c"][1]))
    ok = res["b"][0] / res["a"][0] >= 1.1 and res["b"][1] / res["a"][1] >= 1.1
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


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    t0 = time.time()
    lines = ["masked tile batches on the island mosaic -- %s" % torch.cuda.get_device_name(0)]
    ok = True
    for kind in ("float32", "uint16"):
        ok = run(kind, lines) and ok
    lines.append("wall clock of the whole run: %.1f s" % (time.time() - t0))
    lines.append("pass line met: %s" % ("yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text)
    out_dir = os.environ.get("TILES_MASKED_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "tiles_masked_time.txt"), "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
