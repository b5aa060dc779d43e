"""GPU (run with -m gpu on an MI355X): the MSM's grouping pass and task planner (msm.hip: the two digit recodings, presort_count / scan /
scatter / scatter_once / bins, msm_plan_emit / emit_hot, msm_plan_variant) on PLANTED scalars (tests/grouping_patterns.py) that reach
the planner's boundaries by construction, at every geometry: c = 8, 13, 15 (two-pass scatter) and c = 16 (the one-pass scatter every
proof of 2^14 pairs and more takes), each with 8-byte entries too, the window shards (1, 3) and (2, 3), flat table plans of c = 9 and
c = 12, and the masked variants.  Every plan comes back through wsnark_selftest_msm_plan and is compared exactly with the model; every
sum over the oracle's points is compared bit for bit with its closed form and (up to 20 000 pairs) with the oracle's multiexp: G1 for
every case, G2 for every third.

The masked variants' sums run where the product runs them: in a proof on a planted key and witness, against the oracle's prover.

Not covered: the second trip of the hot combine's slice loop needs nt > 256 * 512 tasks in one bucket
(test_msm_full_size_adversarial_closed_forms)."""
import pytest

import grouping_patterns as gp

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


@pytest.mark.parametrize("k,part", [(k, part) for k in range(len(gp.GEOMETRIES)) for part in gp.geometry_parts(k)])
def test_plans_and_sums(bn, orc, tune, k, part):
    cases = gp.geometry_cases(k, part)
    assert cases
    for j, case in enumerate(cases):
        gp.run_plan(bn, tune, case)
        if case.mask is None:
            gp.run_sum(bn, orc, tune, case, 1)
            if j % 3 == k % 3 and len(case.scalars) <= 5000:        # (the oracle's own G2 multiexp takes 7 s at 18 000 pairs)
                gp.run_sum(bn, orc, tune, case, 2)
        for name in ("MSM_C", "TABLE_C", "MSM_LMAX", "MSM_HOT_MIN", "MSM_ENTRY64"):
            bn.lib.tune(name, None)


@pytest.mark.parametrize("mode", ["plain", "table"])
def test_masked_variant_sums_in_a_proof(bn, orc, tune, mode):
    """the sums over the masked variants: a proof on a planted key and witness against the oracle's prover (gp.planted_key_proof) --
    the path where several point sets with hot buckets of their own share one msm_accumulate / msm_combine_all launch"""
    gp.planted_key_proof(bn, orc, tune, mode)


def test_hook_checks_capacities(bn):
    gp.check_hook_capacities(bn)
