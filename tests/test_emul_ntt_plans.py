"""CPU: the transform's digit plans with the pass count forced (NTT_PASSES) on the emulator build of the kernel sources -- four, three
and two passes at sizes the oracle checks in milliseconds, CALC_H on top of them -- and the two plain-integer yardsticks of the GPU
leg (tests/test_gpu_ntt_plans.py) pinned against the oracle.  Cases and checks: tests/ntt_plans_common.py."""
import pytest

import ntt_plans_common as npc
from emul_util import emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


@pytest.mark.parametrize("passes,bits", npc.FORCED_PLANS)
def test_forced_plan_vs_oracle(bn, orc, tune, passes, bits):
    npc.check_forced_plan(bn, orc, tune, passes, bits)


@pytest.mark.parametrize("passes,dom_bits", npc.FORCED_CALC_H)
def test_forced_calc_h_vs_oracle(bn, orc, tune, passes, dom_bits):
    npc.check_forced_calc_h(bn, orc, tune, passes, dom_bits)


def test_switch_unset_and_out_of_range_keep_the_default_plan(bn, tune):
    npc.check_default_plans(bn, (4, 10, 12))
    for f, bits in ((4, 7), (1, 12), (2, 12), (5, 12), (0, 12)):       # 2 f > bits; bits > 10 f; the default itself; no such count
        tune(bn.lib, "NTT_PASSES", f)
        npc.check_default_plans(bn, (bits,))


@pytest.mark.parametrize("bits", [4, 11])
def test_ntt_sparse_yardstick_vs_oracle(orc, bits):
    npc.check_ntt_sparse_pin(orc, bits)


@pytest.mark.parametrize("bits", [3, 8, 10])
def test_calc_h_sparse_yardstick_vs_oracle(orc, bits):
    npc.check_calc_h_sparse_pin(orc, bits)
