"""GPU: the side-queue schedule of the reduction tails' latency levels (tests/tail_side_common.py) on the device, at 2^12 and 2^14 with
the full-size arrangement forced."""
import pytest

import tail_side_common as ts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bn():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__
    __graft_entry__.ensure_built()
    import wasmsnark_amd
    b = wasmsnark_amd.build(device=0)
    assert b.lib.path.endswith("wasmsnark_amd/libwsnark.so")
    yield b
    ts.free_keys()


@pytest.mark.parametrize("logd", [12, 14])
@pytest.mark.parametrize("forced", [False, True])
def test_side_queue_proof_is_the_one_queue_proof(bn, tune, logd, forced):
    ts.check_on_is_off(bn, tune, "gpu", logd, forced)


@pytest.mark.parametrize("logd", [12, 14])
@pytest.mark.parametrize("forced", [False, True])
def test_eight_proofs_back_to_back(bn, tune, logd, forced):
    ts.check_back_to_back(bn, tune, "gpu", logd, forced)


@pytest.mark.parametrize("logd", [12, 14])
def test_rejected_call_between_proofs(bn, tune, logd):
    ts.check_rejected_call(bn, tune, "gpu", logd)


@pytest.mark.parametrize("g", [1, 2])
def test_planted_sums_with_levels_on_the_side_queue(bn, orc, tune, g):
    ts.check_planted_sums(bn, orc, tune, g)
