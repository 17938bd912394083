"""Block streams seeded with decoy block headers (decoy_common.py) on the device: the plans of test_sim_decoys.py aimed at the scanning
decoder's 32 KiB pieces -- pixels and blob against the oracle bit for bit, which tier served, and the tiers behind the scanning decoder."""
import subprocess
import os

import numpy as np
import pytest

import capi
import decoy_common as D

pytestmark = pytest.mark.gpu

PIECE = D.scan_piece(emulator=False)
NAMES = D.case_names()
# (masked bands have a tier test of their own)
TIER_NAMES = [n for n in NAMES if not n.startswith("masked")]


@pytest.fixture(scope="module")
def P():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    lib = capi.product()
    assert lib is not None, "lerc_amd/csrc/liblerc_amd.so missing -- run __graft_entry__.build()"
    return lib


@pytest.fixture(scope="module")
def O():
    if capi.oracle() is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(capi.ROOT, "oracle")])
    return capi.oracle()


class Context:
    """a context of its own (lerc_amd_create) on the current stream; blobs and pixels travel through torch tensors"""

    def __init__(self):
        import torch
        from lerc_amd import api
        self.torch = torch
        self.codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)

    def forms(self):
        return self.codec.decode_forms()

    def refusals(self):
        return self.codec.decode_refusals()

    def paths(self):
        return self.codec.path_counters()

    def note(self):
        return self.codec.last_note()

    def decode(self, blob, shape, dtype):
        torch = self.torch
        src = torch.zeros(len(blob) + 4096, dtype=torch.uint8, device="cuda:0")
        src[:len(blob)] = torch.from_numpy(np.frombuffer(blob, np.uint8).copy())
        n_out = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out = torch.full((n_out,), 0xCD, dtype=torch.uint8, device="cuda:0")
        rc = self.codec.decode(src.data_ptr(), len(blob), capi.dt_code(dtype), 1, shape[1], shape[0], 1, out.data_ptr())
        torch.cuda.synchronize()
        return rc, out.cpu().numpy().view(dtype).reshape(shape)

    def close(self):
        self.codec.close()


@pytest.mark.parametrize("name", NAMES)
def test_gpu_decoy_pixels(P, O, name):
    """blob = the oracle's, pixels = the oracle's, damaged copies (a byte inside a decoy, a byte of a real header beside one) judged alike"""
    D.check_decoy_case(O, P, D.build_case(O, name, PIECE))


@pytest.mark.parametrize("name", TIER_NAMES)
def test_gpu_decoy_tiers(P, O, name):
    """which tier served: see decoy_common.check_tiers"""
    other = D.build_case(O, "mid-i32" if name.endswith("u16") else "mid-u16", PIECE)
    D.check_tiers(Context, O, D.build_case(O, name, PIECE), other)


@pytest.mark.parametrize("knob,value", D.KNOBS, ids=[k for k, _ in D.KNOBS])
def test_gpu_decoys_on_the_tiers_behind_the_scanning_decoder(P, O, knob, value):
    """the walking one-launch decoder, discovery + decode in two launches, the scanning decoder with late counts: a child process a setting"""
    D.run_knob_child("product", PIECE, knob, value, timeout=300)


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("masked")])
def test_gpu_masked_decoy_tiers(P, O, name):
    """a masked band seeded with decoys stays with the scan that cuts it into blocks: see decoy_common.check_masked_tiers"""
    D.check_masked_tiers(O, P, D.build_case(O, name, PIECE))
