"""k_rt_cut_px / k_rt_paste_px (raster_tiles_px.hip) keep what their layout promises: no scratch -- the vectors they transpose are
indexed by unrolled loops only, a dynamic index would put them into scratch memory --, and an LDS buffer small enough for two
workgroups a CU at the least.  The compiler's own resource remarks are the check, in the manner of
test_scanning_decoder_keeps_three_workgroups_a_cu; no GPU needed.  profiles/raster_px_resources.txt keeps the remarks of the build
this was written against."""
import os
import re
import subprocess

import pytest

import capi


def test_px_kernels_have_no_scratch_and_two_workgroups_a_cu():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(capi.ROOT, "lerc_amd", "csrc", "raster_tiles_px.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
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
    px = {k: v for k, v in seen.items() if re.search(r"k_rt_(cut|paste)_px", k)}
    assert len(px) == 8, sorted(seen)    # (cut and paste, an instantiation an element size: 1, 2, 4, 8 bytes)
    for k, v in px.items():
        assert v["ScratchSize"] == 0 and 0 < v["LDS"] and 2 * v["LDS"] <= 160 * 1024, (k, v)
