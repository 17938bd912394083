#!/usr/bin/env python3
"""Times the depth tile batch calls (lerc_amd_encode_tiles_device_depth / lerc_amd_decode_tiles_device_depth, include/lerc_amd_depth.h),
all device resident, on one MI355X, on two mosaics of 256 tiles of 256 x 256, each with the island mask (synth.island_mask: 98 tiles
all valid, 76 empty, 82 partial) and without a mask:

  U16x3   three uint16 values a pixel derived from the uint16 island (synth.island), lossless
  F32x4   four float32 values a pixel derived from the float32 island, maxZErr 0.01

each (a) through the depth calls (lerc_amd.api.encode_tiles_device_depth / decode_tiles_device_depth) and (b) through one
lerc_amd_encode_device / lerc_amd_decode_device call per tile with nDepth -- what a build without the depth calls offers.  Both are
measured in the same process, alternating repetition by repetition; the blobs of (a) and (b) are compared byte for byte before
anything is timed, and the decoded pixels with the source.

Warm-up, then the median and the interquartile range of REPS (21) repetitions, HIP events around the calls.  Behind the timing, with
the library's own profile on, one batch encode and decode per configuration says where the batch's time goes.  Writes
profiles/tiles_depth_time.txt (TILES_DEPTH_OUT names another directory).  Run it under a time limit of its own:
timeout -k 10 600 python tools/time_tiles_depth.py
"""
import ctypes as ct
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = int(os.environ.get("REPS", "21"))


def mosaics():
    """-> [(name, tiles [n, r, c, d], masks uint8 [n, r, c], maxZErr)]"""
    import numpy as np
    from lerc_amd import synth
    u16, masks, _ = synth.island("uint16", 4096, 256)
    f32, _, e = synth.island("float32", 4096, 256)
    u = np.stack([u16, u16 + 100, (u16 // 2).astype(np.uint16)], axis=-1).astype(np.uint16)
    f = np.stack([f32, f32 * 0.5 + 3, np.roll(f32, 7, axis=2), f32 + np.roll(f32, 3, axis=1) * 0.25], axis=-1).astype(np.float32)
    return [("U16x3", np.ascontiguousarray(u), masks, 0.0), ("F32x4", np.ascontiguousarray(f), masks, float(e))]


def alternating(fast, slow, reps=REPS, warm=3):
    """the two in turn, repetition by repetition -> ({median, iqr} of fast, of slow), ms"""
    import torch
    for _ in range(warm):
        fast()
        slow()
    ms = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((fast, slow)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    out = []
    for v in ms:
        q = statistics.quantiles(v, n=4)
        out.append({"median": statistics.median(v), "iqr": q[2] - q[0]})
    return out


def profile_of(codec, fn):
    """the library's own profile of one call of fn -> text"""
    lib = codec.lib
    lib.lerc_amd_profile_enable.argtypes = [ct.c_void_p, ct.c_int]
    lib.lerc_amd_profile_read.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int]
    lib.lerc_amd_profile_read.restype = ct.c_int
    buf = ct.create_string_buffer(1 << 16)
    lib.lerc_amd_profile_enable(codec.h, 1)
    lib.lerc_amd_profile_read(codec.h, buf, len(buf), 1)
    fn()
    n = lib.lerc_amd_profile_read(codec.h, buf, len(buf), 1)
    lib.lerc_amd_profile_enable(codec.h, 0)
    return buf.value.decode(errors="replace") if n > 0 else ""


def main():
    import numpy as np
    import torch
    from lerc_amd import api
    assert torch.cuda.is_available(), "needs a GPU"
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    lines = ["depth tile batches -- %s" % torch.cuda.get_device_name(0),
             "256 tiles of 256 x 256 x nDepth; median [interquartile range] of %d repetitions, ms, the two ways alternating" % REPS,
             "(a) the depth calls; (b) one lerc_amd_encode_device / lerc_amd_decode_device call per tile with nDepth"]
    profiles = []
    for name, t_np, m_np, e in mosaics():
        n, r, c, d = t_np.shape
        item = t_np.itemsize
        dt = api._dt_code(t_np.dtype)
        tiles = torch.from_numpy(t_np).cuda()
        tile_bytes = r * c * d * item
        slot = (tile_bytes + r * c // 4 + 1024 + 15) & ~15
        for with_mask in (True, False):
            valid = torch.from_numpy(m_np.copy()).cuda() if with_mask else None
            arena = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
            arena_each = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
            out = torch.zeros_like(tiles)
            valid_out = torch.zeros((n, r, c), dtype=torch.uint8, device="cuda") if with_mask else None
            state = {}

            def enc_batch():
                rc, offs, sizes, used = api.encode_tiles_device_depth(codec, tiles, valid, e, arena)
                assert rc == 0, (rc, codec.last_note())
                state["batch"] = (offs, sizes)

            def dec_batch():
                offs, sizes = state["batch"]
                assert api.decode_tiles_device_depth(codec, arena, offs, sizes, out, valid_out) == 0

            def enc_each():
                sizes = np.zeros(n, np.uint32)
                for t in range(n):
                    rc, sizes[t] = codec.encode(tiles.data_ptr() + t * tile_bytes, dt, d, c, r, 1, e, arena_each.data_ptr() + t * slot, slot,
                                                valid.data_ptr() + t * r * c if with_mask else 0, 1 if with_mask else 0)
                    assert rc == 0, rc
                state["each"] = sizes

            def dec_each():
                sizes = state["each"]
                for t in range(n):
                    assert codec.decode(arena_each.data_ptr() + t * slot, int(sizes[t]), dt, d, c, r, 1, out.data_ptr() + t * tile_bytes,
                                        valid_out.data_ptr() + t * r * c if with_mask else 0, 1 if with_mask else 0) == 0

            def pixels_ok():
                got = out.cpu().numpy()
                m = np.broadcast_to((m_np > 0)[..., None], t_np.shape) if with_mask else np.ones(t_np.shape, bool)
                err = np.abs(got[m].astype(np.float64) - t_np[m].astype(np.float64)).max() if m.any() else 0.0
                tol = 0.0 if e == 0 else e + 4 * float(np.spacing(np.float32(np.abs(t_np).max())))    # (the bound, in float32 arithmetic)
                return err <= tol and (not with_mask or np.array_equal(valid_out.cpu().numpy(), m_np))

            # ---- the two ways make the same blobs and the same pixels
            c0 = codec.tile_batch_counters()
            enc_batch()
            dec_batch()
            c1 = codec.tile_batch_counters()
            assert pixels_ok(), "the batch's round trip misses the error bound"
            enc_each()
            offs, sizes = state["batch"]
            a_np, b_np = arena.cpu().numpy(), arena_each.cpu().numpy()
            for t in range(n):
                assert int(sizes[t]) == int(state["each"][t]), (t, sizes[t], state["each"][t])
                assert np.array_equal(a_np[int(offs[t]):int(offs[t]) + int(sizes[t])], b_np[t * slot:t * slot + int(sizes[t])]), "tile %d: the blobs differ" % t
            out.zero_()
            dec_each()
            assert pixels_ok(), "the per-tile round trip misses the error bound"
            counters = [int(c1[i] - c0[i]) for i in range(4)]

            eb, ee = alternating(enc_batch, enc_each)
            db, de = alternating(dec_batch, dec_each)
            label = "%s, %s (%.1f Mvalues, %.1f MB of blobs)" % (name, "island mask" if with_mask else "no mask", n * r * c * d / 1e6, float(sizes.sum()) / 1e6)
            lines.append("%s: %d tiles encoded by the batch's launches, %d one by one; %d / %d decoded" % ((label,) + tuple(counters)))
            for way, fast, slow in (("encode", eb, ee), ("decode", db, de)):
                lines.append("  %s  (a) %8.3f [%6.3f]   (b) %9.3f [%7.3f]   (b) / (a) %7.2f" % (way, fast["median"], fast["iqr"], slow["median"], slow["iqr"],
                                                                                              slow["median"] / fast["median"]))
            profiles.append("%s\n-- encode\n%s-- decode\n%s" % (label, profile_of(codec, enc_batch), profile_of(codec, dec_batch)))
    lines.append("")
    lines.append("where the batch's time goes: the library's own profile of one batch call each (profiling on: not the timed runs)")
    lines.extend(profiles)
    codec.close()
    text = "\n".join(lines) + "\n"
    print(text)
    out_dir = os.environ.get("TILES_DEPTH_OUT", os.path.join(ROOT, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "tiles_depth_time.txt"), "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
