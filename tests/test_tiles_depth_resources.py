"""The depth batch's block kernels (k_tdb_blocks, tile_depth_batch.hip) run k_encode_tiles' body (tile_encode.hip) with a tile per
blockIdx.y: they may use no more scratch a lane than k_encode_tiles of the same type, block size and WRITE, and no kernel of the file
more than 64 KiB of LDS a workgroup.  The compiler's own resource remarks are the check, in the manner of test_raster_px_resources.py;
no GPU needed.  profiles/depth_batch_resources.txt keeps the table of the build this was written against (python
tests/test_tiles_depth_resources.py writes it anew)."""
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
    """-> (rows [(kernel, VGPRs, scratch, LDS, k_encode_tiles' scratch or None)], all kernels of tile_depth_batch.hip)"""
    depth, general = remarks("tile_depth_batch.hip"), remarks("tile_encode.hip")
    yard = {}
    for k, v in general.items():
        m = re.search(r"k_encode_tilesI(\w)Li(\d+)ELb([01])E", k)
        if m:
            yard[m.groups()] = v["ScratchSize"]
    rows = []
    for k, v in sorted(depth.items()):
        m = re.search(r"k_tdb_blocksI(\w)Li(\d+)ELb([01])E", k)
        rows.append((k, v["VGPRs"], v["ScratchSize"], v["LDS"], yard[m.groups()] if m else None))
    return rows


def test_block_kernels_match_the_general_encoder_and_fit_the_lds():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    rows = table()
    blocks = [r for r in rows if r[4] is not None]
    assert len(blocks) == 24, [r[0] for r in rows]    # (six types, 8 x 8 and 16 x 16, sizes and bytes)
    assert len(rows) >= 24 + 12 + 12 + 12, len(rows)  # (beside them: preludes, parses, the decoders' block kernels, the small ones)
    for name, vgprs, scratch, lds, yard in rows:
        assert lds <= 64 * 1024, (name, lds)
        if yard is not None:
            assert scratch <= yard, (name, scratch, yard)


if __name__ == "__main__":
    out = os.path.join(ROOT, "profiles", "depth_batch_resources.txt")
    with open(out, "w") as f:
        f.write("kernels of tile_depth_batch.hip, gfx950, -O3: VGPRs, scratch bytes a lane, LDS bytes a workgroup; k_tdb_blocks beside\n"
                "k_encode_tiles of the same type, block size and WRITE (tile_encode.hip), whose scratch is its bound\n\n")
        for name, vgprs, scratch, lds, yard in table():
            f.write("%-110s VGPRs %3d  scratch %4d  LDS %6d%s\n" % (name, vgprs, scratch, lds, "" if yard is None else "  k_encode_tiles scratch %d" % yard))
    sys.stdout.write(open(out).read())
