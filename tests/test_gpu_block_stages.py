"""The shared block stages on the MI355X: tests/block_stages_common.py, against the oracle."""
import pytest

import capi
import block_stages_common as C
import tiles_masked_common as TM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs():
    import torch    # (before the library is loaded: both then share one HIP runtime)
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    P, R = capi.product(), capi.oracle()
    assert P is not None, "lerc_amd/csrc/liblerc_amd.so is not built"
    assert R is not None, "oracle/liblerc_oracle.so is not built"
    return P, R


@pytest.fixture(scope="module")
def batch(libs):
    B = C.batch_of(libs[0].lib, TM.GpuMem())
    yield B
    B.close()


@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_gpu_block_stages(libs, batch, case):
    C.check_case(libs[0], libs[1], batch, *case)
