"""k_rtn_cut / k_rtn_paste (raster_nodata.hip) keep what the staging kernels they are modelled on promise: no scratch and no LDS in
any of them, and the file holds the kernels it is meant to hold -- the cut for the three integer patterns (1, 2, 4 bytes, either sign),
float and double, the paste an instantiation an element size.  The compiler's own resource remarks are the check, in the manner of test_raster_window_resources.py; no
GPU needed.  profiles/raster_nodata_resources.txt keeps the remarks of the build this was written against."""
import os
import re
import subprocess

import pytest

import capi


def test_nodata_kernels_have_no_scratch():
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(capi.ROOT, "lerc_amd", "csrc", "raster_nodata.hip")
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
    cut = {k: v for k, v in seen.items() if "k_rtn_cut" in k}
    paste = {k: v for k, v in seen.items() if "k_rtn_paste" in k}
    assert len(seen) == 9 and len(cut) == 5 and len(paste) == 4, sorted(seen)
    for k, v in seen.items():
        assert v["ScratchSize"] == 0 and v["LDS"] == 0, (k, v)
        assert v["VGPRs"] <= 128, (k, v)    # (a bandwidth kernel wants loads in flight: four waves a SIMD at the least, 512 registers / 4)
