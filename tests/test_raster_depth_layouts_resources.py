"""k_rtd_cut / k_rtd_paste (raster_tiles_depth.hip) keep what the layout they share with raster_tiles_px.hip promises: no scratch in
any instantiation -- the vectors they transpose and compact are indexed by unrolled loops only --, and no more LDS a workgroup than
k_rt_cut_px / k_rt_paste_px take, so that two workgroups a CU still fit.  The compiler's own resource remarks are the check, in the
manner of test_tiles_depth_resources.py; no GPU needed.  profiles/raster_depth_layouts_resources.txt keeps the table of the build this
was written against (python tests/test_raster_depth_layouts_resources.py writes it anew)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def remarks(name):
    src = os.path.join(ROOT, "lerc_amd", "csrc", name)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
                        "--cuda-device-only", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"\b(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            seen.setdefault(name, {})[m.group(1).split()[0]] = int(m.group(2))
    return seen


def table():
    """-> (rows [(kernel, VGPRs, scratch, LDS)] of raster_tiles_depth.hip, the largest LDS a workgroup of raster_tiles_px.hip's kernels)"""
    depth, px = remarks("raster_tiles_depth.hip"), remarks("raster_tiles_px.hip")
    yard = max(v["LDS"] for k, v in px.items() if re.search(r"k_rt_(cut|paste)_px", k))
    return [(k, v["VGPRs"], v["ScratchSize"], v["LDS"]) for k, v in sorted(depth.items())], yard


def test_depth_layout_kernels_have_no_scratch_and_the_px_kernels_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    rows, yard = table()
    ours = [r for r in rows if re.search(r"k_rtd_(cut|paste)", r[0])]
    assert len(ours) == 8 and len(rows) == 8, [r[0] for r in rows]    # (cut and paste, an instantiation an element size: 1, 2, 4, 8 bytes)
    assert 0 < yard and 2 * yard <= 160 * 1024
    for name, vgprs, scratch, lds in ours:
        assert scratch == 0, (name, scratch)
        assert 0 < lds <= yard, (name, lds, yard)


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "raster_depth_layouts_resources.txt")
    rows, yard = table()
    with open(out, "w") as f:
        f.write("kernels of raster_tiles_depth.hip, gfx950, -O3: VGPRs, scratch bytes a lane, LDS bytes a workgroup; the largest LDS a workgroup\n"
                "of k_rt_cut_px / k_rt_paste_px (raster_tiles_px.hip), which is their bound: %d\n\n" % yard)
        for name, vgprs, scratch, lds in rows:
            f.write("%-70s VGPRs %3d  scratch %4d  LDS %6d\n" % (name, vgprs, scratch, lds))
    sys.stdout.write(open(out).read())
