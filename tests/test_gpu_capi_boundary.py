"""The C boundary's answers (capi_boundary_common.py) on the MI355X: the same table as on the emulator."""
import pytest

import capi
import capi_boundary_common as CB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch    # (before the library is loaded: both then share one HIP runtime)
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    P = capi.product()
    assert P is not None, "lerc_amd/csrc/liblerc_amd.so is not built"
    e = CB.Env(P.lib, CB.M.GpuMem())
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(CB.SPECS))
def test_boundary(env, name):
    CB.check(env, name)
