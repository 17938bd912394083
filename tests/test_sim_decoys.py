"""Block streams seeded with decoy block headers (decoy_common.py), on the emulator build of the real kernel sources: the scanning
decoder's mending (strike path, anchor rule, false chains that tile into the path, table overflow) and the walking tiers behind it,
against the oracle, bit for bit.  The emulator build stages pieces of LERC_SCAN_PIECE = 8 KiB (tile_fast.h, under LERC_SMALL_GROUPS, which
the sim target of lerc_amd/csrc/Makefile sets); the GPU file runs the same plans aimed at the device's 32 KiB."""
import ctypes as ct
import os
import subprocess
import sys

import numpy as np
import pytest

import capi
import decoy_common as D

PIECE = D.scan_piece(emulator=True)


@pytest.fixture(scope="module")
def libs():
    import fcntl
    csrc = os.path.join(capi.ROOT, "lerc_amd", "csrc")
    os.makedirs(os.path.join(capi.ROOT, "tests", "_sim"), exist_ok=True)
    with open(os.path.join(capi.ROOT, "tests", "_sim", ".build.lock"), "w") as lock:    # (pytest-xdist workers: one make at a time)
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", csrc, "sim", "-j8"])
        subprocess.check_call(["make", "-s", "-C", os.path.join(capi.ROOT, "oracle")])
    return capi.oracle(), capi.sim()


def _aligned(n_bytes, align=64):
    raw = np.zeros(n_bytes + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + n_bytes]


class Context:
    """a context of its own on the emulator library (device pointers are host pointers there)"""

    def __init__(self, S):
        L = self.L = S.lib
        L.lerc_amd_create.restype = ct.c_void_p
        L.lerc_amd_create.argtypes = [ct.c_void_p]
        L.lerc_amd_destroy.argtypes = [ct.c_void_p]
        L.lerc_amd_decode_device.restype = ct.c_uint
        L.lerc_amd_decode_device.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_uint, ct.c_int, ct.c_void_p, ct.c_int, ct.c_int, ct.c_int,
                                             ct.c_int, ct.c_uint, ct.c_void_p]
        for f in (L.lerc_amd_path_counters, L.lerc_amd_decode_forms, L.lerc_amd_decode_refusals):
            f.argtypes = [ct.c_void_p, ct.POINTER(ct.c_ulonglong)]
            f.restype = None
        L.lerc_amd_last_note.argtypes = [ct.c_void_p]
        L.lerc_amd_last_note.restype = ct.c_char_p
        self.h = L.lerc_amd_create(None)
        assert self.h

    def _four(self, f):
        out = (ct.c_ulonglong * 4)()
        f(self.h, out)
        return [int(v) for v in out]

    def forms(self):
        return self._four(self.L.lerc_amd_decode_forms)

    def refusals(self):
        return self._four(self.L.lerc_amd_decode_refusals)

    def paths(self):
        return self._four(self.L.lerc_amd_path_counters)

    def note(self):
        return self.L.lerc_amd_last_note(self.h).decode()

    def decode(self, blob, shape, dtype):
        src = _aligned(len(blob) + 4096)
        src[:] = 0
        src[:len(blob)] = np.frombuffer(blob, np.uint8)
        out = _aligned(int(np.prod(shape)) * np.dtype(dtype).itemsize).view(dtype).reshape(shape)
        out.view(np.uint8)[...] = 0xCD
        rc = self.L.lerc_amd_decode_device(self.h, src.ctypes.data, len(blob), 0, None, 1, shape[1], shape[0], 1, capi.dt_code(dtype), out.ctypes.data)
        return rc, out.copy()

    def close(self):
        self.L.lerc_amd_destroy(self.h)


NAMES = D.case_names()
# (masked bands have a tier test of their own)
TIER_NAMES = [n for n in NAMES if not n.startswith("masked")]


@pytest.mark.parametrize("piece", [D.scan_piece(True), D.scan_piece(False)])
def test_decoy_preconditions_at_both_piece_sizes(libs, piece):
    """The model's conditions for every case, aimed at the emulator's piece size and at the device's: the plan's false survivors are
    there, in the piece intended; at most 8 a piece (crowd: more than 64 in one); boundary: the last one in front of a piece's own
    bytes and the first one inside it are neighbours of one chain; the control raster holds none.  The oracle alone, no kernel."""
    O, _ = libs
    for name in NAMES:
        c = D.build_case(O, name, piece)
        assert c.control_model.false_survivors == [] and len(c.model.false_survivors) >= len(c.promised) > 0, name


@pytest.mark.parametrize("name", NAMES)
def test_sim_decoy_pixels(libs, name):
    """blob = the oracle's, pixels = the oracle's, damaged copies (a byte inside a decoy, a byte of a real header beside one) judged alike"""
    O, S = libs
    D.check_decoy_case(O, S, D.build_case(O, name, PIECE))


@pytest.mark.parametrize("name", TIER_NAMES)
def test_sim_decoy_tiers(libs, name):
    """which tier served: see decoy_common.check_tiers"""
    O, S = libs
    other = D.build_case(O, "mid-i32" if name.endswith("u16") else "mid-u16", PIECE)
    D.check_tiers(lambda: Context(S), O, D.build_case(O, name, PIECE), other)


@pytest.mark.parametrize("knob,value", D.KNOBS, ids=[k for k, _ in D.KNOBS])
def test_sim_decoys_on_the_tiers_behind_the_scanning_decoder(libs, knob, value):
    """The walking one-launch decoder (LERC_AMD_DECODE_SCAN=0), discovery + decode in two launches (LERC_AMD_DECODE_LAUNCHES=2) and the
    scanning decoder with late counts (LERC_AMD_SCAN_EARLY=0: no launch thrown away) on every case, the long false chains included:
    the oracle's pixels, the control rasters on the streaming path.  A child process a setting: the knobs are read once."""
    D.run_knob_child("sim", PIECE, knob, value)


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("masked")])
def test_sim_masked_decoy_tiers(libs, name):
    """a masked band seeded with decoys stays with the scan that cuts it into blocks: see decoy_common.check_masked_tiers"""
    O, S = libs
    D.check_masked_tiers(O, S, D.build_case(O, name, PIECE))
