"""CPU: the fused task planner and the plans' alternating counter blocks (msm.hip: msm_plan_fused, WSNARK_PLAN_FUSED / PLAN_SPAN) under
the thread emulator, on the cases of tests/plan_fused_common.py.  Every plan is compared exactly with the model of
tests/grouping_patterns.py, with the switch on and off, and every build is checked for the words it must leave at zero.

The emulator runs a grid's workgroups one after the other, so the workgroup that arrives last is always the last of the grid: what
this file checks of the arrival is its arithmetic and that the counter is left at zero; the GPU file runs the same cases with the
workgroups beside each other.  The proofs run at 2^10 here (the emulator is slow), at 2^12 on the device."""
import pytest

import grouping_patterns as gp
import plan_fused_common as pf
from emul_util import emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


@pytest.fixture(autouse=True)
def _reset(bn):
    yield
    pf.reset(bn)


def test_span_edges_are_the_nearest_bucket_counts():
    """no GPU, no emulator: the bucket counts around every span, and every case reaches what it names"""
    for span in pf.SPANS:
        c, counts = pf.span_edges(span)
        NB = 1 << (c - 1)
        assert [nb for nb, _ in counts] == [span - NB, span, span + NB, 2 * span + NB]
        for cs in pf.span_edge_cases(span):
            gp.assert_reaches(cs)
    for cs in pf.kinds_cases():
        gp.assert_reaches(cs)


@pytest.mark.parametrize("span", pf.SPANS)
def test_span_edges(bn, tune, span):
    """span - NB, span, span + NB and 2 span + NB buckets, per-window and flat plans, 4- and 8-byte entries; the plan with the switch
    off holds the same buckets"""
    for cs in pf.span_edge_cases(span):
        on = pf.run(bn, tune, cs, 1, span)
        if span == pf.SPAN_DEFAULT:
            pf.same_counts(on, pf.run(bn, tune, cs, 0))


@pytest.mark.parametrize("fused", [1, 0])
def test_three_kinds_in_one_plan(bn, tune, fused):
    for cs in pf.kinds_cases():
        for span in (pf.SPANS if fused else (None,)):
            pf.run(bn, tune, cs, fused, span)


@pytest.mark.parametrize("fused", [1, 0])
def test_rebuilds_on_one_lane(bn, tune, fused):
    pf.check_rebuilds(bn, tune, fused, big_c=10)


def test_three_proofs_back_to_back(bn, orc, tune):
    pf.check_proofs(bn, orc, tune, 10)
