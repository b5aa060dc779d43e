"""CPU: the staged grouping kernels (msm.hip: presort_scatter_once<uint32_t, true>, presort_bins<uint32_t, true>, WSNARK_PRESORT_STAGE)
under the thread emulator, on the cases of tests/grouping_staged_cases.py: every plan comes back through wsnark_selftest_msm_plan and
is compared exactly with the model of tests/grouping_patterns.py, sums bit for bit with the closed form and the oracle's multiexp.

The emulator is slow, so this file runs the minimum: everything at the flat plan of TABLE_C = 16 (16 rows, 256 bins), two plans of
4096 bins (TABLE_C = 20 with MSM_LO_BITS = 7: a full tile and one more scalar of digit scalars; every entry in a bin of its own) and
one per-window plan of c = 16.  The GPU file runs every case at every geometry."""
import pytest

import grouping_patterns as gp
import grouping_staged_cases as gs
from emul_util import emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


@pytest.fixture(autouse=True)
def _reset(bn):
    yield
    gs.reset(bn)


def test_cases_reach_their_boundaries():
    """the model-level self-checks of every case of both files, with no emulator and no GPU"""
    for geo in gs.GEOS:
        lo = geo[3]
        for cs in gs.one_bin_cases(geo) + gs.own_bin_cases(geo, lo) + gs.last_lane_cases(geo, lo) + gs.cap_cases(geo, lo):
            info = gs.geometry(cs, lo)
            assert cs.reaches(gp.model_stats(cs.scalars, info, cs.mask), info), cs.name
    assert gs.geometry(gs.case("", gs.FLAT20_LO7, [1] * 1000, None), 7)["nbins"] == 4096
    assert gs.geometry(gs.case("", gs.FLAT16, [1], None), 8) == gs.geometry(gs.case("", gs.FLAT16, [1], None))


def test_tile_edges_flat16(bn, orc, tune):
    for cs in gs.tile_edge_cases(gs.FLAT16):
        gs.run_plan(bn, tune, cs)
        if len(cs.scalars) in (63, gs.T + 1):
            gs.run_sum(bn, orc, tune, cs)


def test_4096_bins_of_7_low_bits(bn, orc, tune):
    """the 2^20 key's geometry at small sizes: 13 rows, 4096 bins (TABLE_C = 20, MSM_LO_BITS = 7)"""
    for cs in gs.tile_edge_cases(gs.FLAT20_LO7, sizes=[gs.T + 1]) + gs.own_bin_cases(gs.FLAT20_LO7, 7):
        gs.run_plan(bn, tune, cs, lo_bits=7)


def test_runs_as_long_as_the_stage_and_of_length_one(bn, orc, tune):
    for cs in gs.one_bin_cases(gs.FLAT16) + gs.own_bin_cases(gs.FLAT16, None) + gs.last_lane_cases(gs.FLAT16, None):
        gs.run_plan(bn, tune, cs)
    gs.run_sum(bn, orc, tune, gs.one_bin_cases(gs.FLAT16)[1])


def test_per_window_plan(bn, orc, tune):
    gs.run_plan(bn, tune, gs.last_lane_cases(gs.WIN16, None)[0])


def test_bins_around_cap(bn, orc, tune):
    for cs in gs.cap_cases(gs.FLAT16, None):
        gs.run_plan(bn, tune, cs)


def test_switch_off_against_on(bn, orc, tune):
    for cs in (gs.cap_cases(gs.FLAT16, None)[0], gs.tile_edge_cases(gs.FLAT16, sizes=[gs.T + 1])[0]):
        off, on = (gs.run_plan(bn, tune, cs, stage=st) for st in (0, 1))
        gs.assert_same_plans(off, on, cs.lmax)
    sums = [gs.raw_sum(bn, orc, tune, cs, None, st) for st in (0, 1)]
    assert sums[0] == sums[1] == gp.Points.get(orc, 1).expected(cs.scalars)


def test_entry64_takes_the_unstaged_kernels(bn, orc, tune):
    for cs in gp.size_cases(16, flat=True, entry64=True, sizes=[gs.T + 1]):
        gs.run_plan(bn, tune, cs)
        gs.run_sum(bn, orc, tune, cs)
