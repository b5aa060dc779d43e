"""CPU: the MSM's grouping pass and task planner (msm.hip: the two digit recodings, presort_count / scan / scatter / scatter_once /
bins, msm_plan_emit / emit_hot, msm_plan_variant) under the thread emulator, on PLANTED scalars (tests/grouping_patterns.py) that reach
the planner's boundaries by construction.  Every plan comes back through wsnark_selftest_msm_plan and is compared exactly with the
model -- buckets as multisets, tasks, partial slots, counters, hot slices --, and the sums over the oracle's points are compared bit
for bit with their closed form and with the oracle's multiexp.

The emulator is slow, so every boundary row runs once, at c = 8 (two-pass scatter, presort_scan), with its G1 sum; the other geometries
(c = 13, MSM_ENTRY64, the window shards, the flat table plans of c = 9 and c = 12) run the reduced list, and sums only where they are
small; G2 sums on every third of the smallest cases.  Trimmed against the GPU file, which runs everything everywhere: the sizes
n = 2048, 2049 and 4097 run at no geometry here (1, 63, 1023, 1024, 1025 do at c = 8: both sides of a 1024-scalar tile and of
idx_bits' step at 2^10); c = 16, the one-pass scatter, runs the digit scalars at n = 1025 with no sum (1, 63, 1023 and 1024 are
left to the GPU: a plan of 2048 bins takes 13-25 s each here); c = 13 runs the window-0 rows of the reduced list, a size and the masked
variant, no bin rows; c = 15 does not run.  The masked variants'
sums run in two proofs on a planted key.  Measured on an otherwise idle machine: the whole file in 205 s
(tests/test_emul_tail_patterns.py: 106 s); c = 8 takes 56 s of it, c = 16 24 s, c = 13 18 s, the two proofs 30 s, the self-checks 34 s."""
import random

import pytest

import grouping_patterns as gp
from emul_util import emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


def _run(bn, orc, tune, cases, sum_below, g2_below=0):
    for k, case in enumerate(cases):
        gp.run_plan(bn, tune, case)
        if case.mask is None and len(case.scalars) <= sum_below:
            gp.run_sum(bn, orc, tune, case, 1)
            if k % 3 == 0 and len(case.scalars) <= g2_below:
                gp.run_sum(bn, orc, tune, case, 2)
        for name in ("MSM_C", "TABLE_C", "MSM_LMAX", "MSM_HOT_MIN", "MSM_ENTRY64"):
            bn.lib.tune(name, None)


def test_digits_against_int_arithmetic():
    """digits() from the definition: sum_w d_w 2^(c w) == raw mod r and |d_w| <= NB (NB itself only positive), on the whole scalars
    of every width and 10 000 seeded values"""
    rnd = random.Random(5)
    for c in (8, 9, 12, 13, 15, 16):
        Wall, NB = gp.windows(c), 1 << (c - 1)
        vals = gp.whole_scalars(c) + [2 * gp.R - 1, (1 << 255) - 1, NB, NB + 1, (1 << c) - 1, 1 << c]
        vals += [rnd.randrange(1 << 256) for _ in range(1250)] + [rnd.randrange(gp.R) for _ in range(420)]
        for v in vals:
            ds = gp.digits(v, c, Wall)
            assert len(ds) == Wall and all(-NB < d <= NB for d in ds), (c, v)
            assert sum(d * (1 << (c * w)) for w, d in enumerate(ds)) == v % gp.R, (c, v)


@pytest.mark.parametrize("k", range(len(gp.GEOMETRIES)))
def test_every_case_reaches_its_boundary(k):
    """the model-level self-checks alone (no emulator, no GPU) on every case of every geometry the GPU file runs: each reaches the
    boundary it names.  (The tests below assert the same for every case they run, before they run it: gp.run_plan.)"""
    for part in gp.geometry_parts(k):
        for case in gp.geometry_cases(k, part):
            gp.assert_reaches(case)


def test_c8_every_boundary_row(bn, orc, tune):
    """c = 8: 32 windows, the two-pass scatter and presort_scan; every row of the catalogue, G1 sums of all, G2 sums of the small ones"""
    _run(bn, orc, tune, gp.catalogue(8, masked=True, sizes=[1, 63, 1023, 1024, 1025]), sum_below=20000, g2_below=150)


def test_c13_reduced(bn, orc, tune):
    """c = 13: windows that straddle limb boundaries, 16 bins per window"""
    _run(bn, orc, tune, gp.planner_cases(13, full=False)[:2] + gp.size_cases(13, sizes=[1025]) + gp.masked_cases(13), sum_below=100)


@pytest.mark.parametrize("shard", [(0, 1), (1, 3), (2, 3)])
def test_c8_entry64_and_shards(bn, orc, tune, shard):
    """8-byte grouping entries (MSM_ENTRY64) on the whole scalar; the window shards (1, 3) and (2, 3) with 4-byte entries"""
    _run(bn, orc, tune, gp.catalogue(8, shard=shard, entry64=shard == (0, 1), full=False, sizes=[63, 1025]), sum_below=1100)


@pytest.mark.parametrize("c", [9, 12])
def test_flat_table_plans(bn, orc, tune, c):
    """flat plans (TABLE_C): one bucket set for every window, entries index the table (window n + i); the reduced
    catalogue; the sums through resident points"""
    _run(bn, orc, tune, gp.catalogue(c, flat=True, full=False, sizes=[1, 63, 1024, 1025], masked=True), sum_below=300)


def test_c16_one_pass_scatter_digit_scalars(bn, orc, tune):
    """c = 16: 16 windows, presort_scatter_once (the statically unrolled recoding) -- the digit scalars at n = 1025 (two tiles, the second
    with one scalar); the plan only (2048 bins of 64 emulated threads each)"""
    _run(bn, orc, tune, gp.size_cases(16, sizes=[1025]), sum_below=0)


@pytest.mark.parametrize("mode", ["plain", "table"])
def test_masked_variant_sums_in_a_proof(bn, orc, tune, mode):
    """the sums over the masked variants: a proof on a planted key and witness against the oracle's prover (gp.planted_key_proof)"""
    gp.planted_key_proof(bn, orc, tune, mode)


def test_hook_checks_capacities(bn):
    gp.check_hook_capacities(bn)
