"""GPU (run with -m gpu on an MI355X): the fused task planner and the plans' alternating counter blocks (msm.hip: msm_plan_fused,
WSNARK_PLAN_FUSED / PLAN_SPAN) on the cases of tests/plan_fused_common.py.  Every plan is compared exactly with the model of
tests/grouping_patterns.py, with the switch on and off, and every build is checked for the words it must leave at zero; three 2^12
proofs back to back on one key are their switch-off proofs, the closed form and the oracle's prover's."""
import pytest

import plan_fused_common as pf

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
    return b


@pytest.fixture(autouse=True)
def _reset(bn):
    yield
    pf.reset(bn)


@pytest.mark.parametrize("span", pf.SPANS)
def test_span_edges(bn, tune, span):
    """span - NB, span, span + NB and 2 span + NB buckets, per-window and flat plans, 4- and 8-byte entries; the plan with the switch
    off holds the same buckets"""
    for cs in pf.span_edge_cases(span):
        pf.same_counts(pf.run(bn, tune, cs, 1, span), pf.run(bn, tune, cs, 0))


@pytest.mark.parametrize("fused", [1, 0])
def test_three_kinds_in_one_plan(bn, tune, fused):
    for cs in pf.kinds_cases():
        for span in (pf.SPANS if fused else (None,)):
            pf.run(bn, tune, cs, fused, span)


@pytest.mark.parametrize("fused", [1, 0])
def test_rebuilds_on_one_lane(bn, tune, fused):
    pf.check_rebuilds(bn, tune, fused)


def test_three_proofs_back_to_back(bn, orc, tune):
    pf.check_proofs(bn, orc, tune, 12)
