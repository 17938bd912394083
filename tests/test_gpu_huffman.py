"""The 8-bit Huffman decoder on the device (`-m gpu`): cases.huffman_matrix_cases -- code books whose words all have one
length, which never fall into step on their own, next to self-synchronising ones -- against the real reference build
(oracle/_ref/libLercRef.so; the CPU oracle where that did not travel).  Blob and size query byte-identical, decode == input
== the reference's decode, and the decoder's speculative sync within 2 + ceil(log2(sub-sequences)) host round trips
(exactly one for the self-synchronising content)."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest

import capi
import cases
import huffblob

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs():
    import torch
    from lerc_amd import api
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    if capi.oracle() is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(capi.ROOT, "oracle")])
    P = capi.LercLib(api.library_path())    # (the build the device codec below loads)
    R = capi.ref() or capi.oracle()
    return R, P


def _decoder():
    """decode(blob, arr, kw) for cases.check_huffman_matrix_case: lerc_amd_decode_device on a DeviceCodec with the profile on;
    sync rounds = its huff_sync launches (one per host round trip of the sync loop)"""
    import torch
    from lerc_amd import api
    codec = api.DeviceCodec(torch.cuda.current_stream().cuda_stream)
    L = codec.lib
    L.lerc_amd_profile_enable.argtypes = [ct.c_void_p, ct.c_int]
    L.lerc_amd_profile_read.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int, ct.c_int]

    def decode(blob, arr, kw):
        nd = kw.get("n_depth", 1)
        rows, cols = arr.shape[0], arr.shape[1]
        d_blob = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()    # (an allocation of its own: 256-byte aligned)
        out = torch.full((arr.nbytes,), 0xCD, dtype=torch.uint8, device="cuda")
        mask = torch.full((rows * cols,), 0xCD, dtype=torch.uint8, device="cuda") if "mask" in kw else None
        torch.cuda.synchronize()
        L.lerc_amd_profile_read(codec.h, ct.create_string_buffer(16), 16, 1)
        L.lerc_amd_profile_enable(codec.h, 1)
        rc = codec.decode(d_blob.data_ptr(), len(blob), capi.dt_code(arr.dtype), nd, cols, rows, 1, out.data_ptr(),
                          mask.data_ptr() if mask is not None else 0, 1 if mask is not None else 0)
        torch.cuda.synchronize()
        L.lerc_amd_profile_enable(codec.h, 0)
        buf = ct.create_string_buffer(1 << 16)
        L.lerc_amd_profile_read(codec.h, buf, len(buf), 1)
        rounds = sum(int(ln.split()[2]) for ln in buf.value.decode().splitlines() if ln.split()[0] == "huff_sync")
        dec = out.cpu().numpy().view(arr.dtype)
        return rc, dec, (mask.cpu().numpy() if mask is not None else None), rounds, codec.last_error()
    return decode


def _compute_units():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run(libs, scale, big=False, only=None):
    R, P = libs
    dec = _decoder()
    cu = _compute_units()
    phases = set()
    for name, arr, kw, mode, kind in cases.huffman_matrix_cases(scale, big=big):
        if only is not None and name not in only:
            continue
        mis, _, _ = cases.check_huffman_matrix_case(R, P, dec, name, arr, kw, mode, kind, cu, huffblob.DEC_THREADS_GPU)
        phases.add(mis)
    return phases


@pytest.mark.parametrize("scale", [4, 32])
def test_huffman_sync_matrix(libs, scale):
    """scale 4: streams of one decoder workgroup (256 sub-sequences) or less; scale 32: several workgroups, the chain between
    them.  Stream offsets 0 .. 3 bytes into a word all occur."""
    assert _run(libs, scale) == {0, 1, 2, 3}


def test_huffman_sync_4096_rgb_and_8192_128_values(libs):
    """A 4096^2 x 3 delta raster of 3-bit codes (most of one round of resident workgroups) and an 8192^2 plain raster of 128
    balanced values (7-bit codes, several rounds of resident workgroups)."""
    _run(libs, 1, big=True, only={"delta8-u8-4096x4096x3", "eq7-u8-8192x8192"})


def test_huffman_sync_c4_raster_takes_one_round(libs):
    """The benchmark's C4 raster (4096 x 4096 x 3, self-synchronising): a single sync round."""
    from lerc_amd import synth
    R, P = libs
    x = synth.c4_rgb_u8().numpy()
    rc, blob = P.encode(x, 0, n_depth=3)
    rc_r, blob_r = R.encode(x, 0, n_depth=3)
    assert rc == rc_r == 0 and blob == blob_r
    rc, dec, _, rounds, err = _decoder()(blob, x, dict(n_depth=3))
    print(f"c4: sync rounds {rounds}")
    assert rc == 0, err
    assert np.array_equal(dec.reshape(x.shape), x)
    assert rounds == 1
