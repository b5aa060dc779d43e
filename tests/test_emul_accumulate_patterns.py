"""CPU: the MSM accumulation kernel (msm.hip: msm_accumulate, accumulate_range) under the thread emulator on caller-written tasks
(tests/accumulate_patterns.py) through wsnark_selftest_msm_accumulate: every entry that equals, cancels or is infinity is planted at
a chosen position of a chosen task, on both curves (G1: the prefetching loop; G2: the other), in launches of 1, 255 and all tasks.
Every sum is compared bit for bit with the oracle's double-and-add of the signed sum of the multiples; the case table's coverage of
the loop's branches is asserted before the library is used."""
import pytest

import accumulate_patterns as ap
from emul_util import emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


@pytest.mark.parametrize("g", [1, 2])
def test_case_table_reaches_every_branch(g):
    T = ap.case_table(g)
    ap.assert_coverage(T)
    assert 256 < len(T.cases) < 1000 and len(T.vals) < 20000


@pytest.mark.parametrize("g", [1, 2])
def test_accumulate_patterns(bn, orc, g):
    ap.assert_coverage(ap.case_table(g))
    T, points, expected = ap.planted(orc, g)
    for n_tasks in (1, 255, len(T.tasks)):
        ap.check_launch(bn, g, T, points, expected, n_tasks)


@pytest.mark.parametrize("g", [1, 2])
def test_accumulate_hook_refuses_bad_arguments(bn, orc, g):
    T, points, expected = ap.planted(orc, g)
    ap.check_error_calls(bn, g, T, points, expected)
