"""k_rw_paste / k_rw_paste_px (raster_window.hip) keep what the kernels they are modelled on promise: no scratch in any of them, and for
the pixel form an LDS buffer small enough for two workgroups a CU at the least.  The compiler's own resource remarks are the check,
in the manner of test_raster_px_resources.py; no GPU needed.  profiles/raster_window_resources.txt keeps the remarks of the build
this was written against."""
import os
import re
import subprocess

import pytest

import capi


def test_window_kernels_have_no_scratch_and_two_workgroups_a_cu():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(capi.ROOT, "lerc_amd", "csrc", "raster_window.hip")
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
    assert len(seen) == 8 and all("k_rw_paste" in k for k in seen), sorted(seen)    # (two forms, an instantiation an element size)
    px = {k: v for k, v in seen.items() if "k_rw_paste_px" in k}
    assert len(px) == 4, sorted(seen)
    for k, v in seen.items():
        assert v["ScratchSize"] == 0, (k, v)
        if k in px:
            assert 0 < v["LDS"] and 2 * v["LDS"] <= 160 * 1024, (k, v)
        else:
            assert v["LDS"] == 0, (k, v)
