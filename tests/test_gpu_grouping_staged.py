"""GPU (run with -m gpu on an MI355X): the staged grouping kernels (msm.hip: presort_scatter_once<uint32_t, true>,
presort_bins<uint32_t, true>, WSNARK_PRESORT_STAGE) on the cases of tests/grouping_staged_cases.py, at every geometry of that file: flat
plans of TABLE_C = 16 (16 rows, 256 bins) and TABLE_C = 20 (13 rows; 2048 bins, and 4096 with MSM_LO_BITS = 7), and the per-window plan
of c = 16.  Every plan comes back through wsnark_selftest_msm_plan and is compared exactly with the model of
tests/grouping_patterns.py; every G1 sum is compared bit for bit with its closed form and the oracle's multiexp."""
import pytest

import grouping_patterns as gp
import grouping_staged_cases as gs

pytestmark = pytest.mark.gpu
GEO = pytest.mark.parametrize("geo", gs.GEOS, ids=[g[0] for g in gs.GEOS])


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
    gs.reset(bn)


def _run(bn, orc, tune, cases, lo):
    for cs in cases:
        gs.run_plan(bn, tune, cs, lo_bits=lo)
        if cs.mask is None:
            gs.run_sum(bn, orc, tune, cs, lo_bits=lo)


@GEO
def test_tile_edges(bn, orc, tune, geo):
    """n = 1, 63, T - 1, T, T + 1, 2 T + 1: random scalars and the digit scalars"""
    _run(bn, orc, tune, gs.tile_edge_cases(geo), geo[3])


@GEO
def test_runs_as_long_as_the_stage_and_of_length_one(bn, orc, tune, geo):
    """one bin takes every entry of a tile; every entry of a tile in a bin of its own; a bin that only the last live lane reaches"""
    _run(bn, orc, tune, gs.one_bin_cases(geo) + gs.own_bin_cases(geo, geo[3]) + gs.last_lane_cases(geo, geo[3]), geo[3])


@GEO
def test_bins_around_cap(bn, orc, tune, geo):
    """bins of CAP - 1, CAP and CAP + 1 entries, a bin of one bucket, empty bins; then the same under a mask"""
    _run(bn, orc, tune, gs.cap_cases(geo, geo[3]), geo[3])


@GEO
def test_switch_off_against_on(bn, orc, tune, geo):
    """equal bounds, equal tasks per length key, equal buckets as multisets; bit-identical sums"""
    lo = geo[3]
    for cs in (gs.cap_cases(geo, lo)[0], gs.tile_edge_cases(geo, sizes=[2 * gs.T + 1])[0], gs.one_bin_cases(geo)[1]):
        off, on = (gs.run_plan(bn, tune, cs, lo_bits=lo, stage=st) for st in (0, 1))
        gs.assert_same_plans(off, on, cs.lmax)
        sums = [gs.raw_sum(bn, orc, tune, cs, lo, st) for st in (0, 1)]
        assert sums[0] == sums[1] == gp.Points.get(orc, 1).expected(cs.scalars), cs.name


@pytest.mark.parametrize("flat", [True, False])
def test_entry64_takes_the_unstaged_kernels(bn, orc, tune, flat):
    for cs in gp.size_cases(16, flat=flat, entry64=True, sizes=[gs.T - 1, gs.T + 1]):
        gs.run_plan(bn, tune, cs)
        gs.run_sum(bn, orc, tune, cs)


def test_proof_of_2_14_constraints(bn, tune):
    """one proof on the synthetic 2^14 circuit with the switch on (and, for the pair, off) equals the closed form"""
    from wasmsnark_amd import synth
    circ = synth.NativeCircuit(bn.lib, 14, n_public=5, seed=1)
    sec, _ = circ.build_sections()
    key = bn.load_key(sections=sec)
    try:
        r, s = bytes(range(32)), bytes(range(32, 64))
        want = circ.expected_proof(r, s)
        for stage in (1, 0):
            tune(bn.lib, "PRESORT_STAGE", stage)
            assert bn.groth16GenProof(circ.witness_bin(), key, r=r, s=s) == want, stage
    finally:
        key.free()
