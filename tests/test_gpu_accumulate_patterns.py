"""GPU (run with -m gpu on an MI355X): the MSM accumulation kernel (msm.hip: msm_accumulate, accumulate_range) on caller-written tasks
(tests/accumulate_patterns.py) through wsnark_selftest_msm_accumulate: every entry that equals, cancels or is infinity is planted at
a chosen position of a chosen task, on both curves (G1: the prefetching loop; G2: the other), in launches of 1, 255 and all tasks.
Every sum is compared bit for bit with the oracle's double-and-add of the signed sum of the multiples; the case table's coverage of
the loop's branches is asserted before the device is used."""
import pytest

import accumulate_patterns as ap

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


@pytest.mark.parametrize("g", [1, 2])
def test_accumulate_patterns_on_device(orc, g, request):
    ap.assert_coverage(ap.case_table(g))             # (a condition on the inputs: before the device is used)
    T, points, expected = ap.planted(orc, g)
    bn = request.getfixturevalue("bn")
    for n_tasks in (1, 255, len(T.tasks)):
        ap.check_launch(bn, g, T, points, expected, n_tasks)


@pytest.mark.parametrize("g", [1, 2])
def test_accumulate_hook_refuses_bad_arguments_on_device(bn, orc, g):
    T, points, expected = ap.planted(orc, g)
    ap.check_error_calls(bn, g, T, points, expected)
