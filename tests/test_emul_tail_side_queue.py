"""CPU: the side-queue schedule of the reduction tails' latency levels (tests/tail_side_common.py) under the thread emulator, at 2^10
with the full-size arrangement forced."""
import pytest

import tail_side_common as ts
from emul_util import emul_bn128

LOGD = 10


@pytest.fixture(scope="module")
def bn():
    yield emul_bn128()
    ts.free_keys()


@pytest.mark.parametrize("forced", [False, True])
def test_side_queue_proof_is_the_one_queue_proof(bn, tune, forced):
    ts.check_on_is_off(bn, tune, "emul", LOGD, forced)


def test_eight_proofs_back_to_back(bn, tune):
    ts.check_back_to_back(bn, tune, "emul", LOGD, True)


def test_rejected_call_between_proofs(bn, tune):
    ts.check_rejected_call(bn, tune, "emul", LOGD)


@pytest.mark.parametrize("g", [1, 2])
def test_planted_sums_with_levels_on_the_side_queue(bn, orc, tune, g):
    ts.check_planted_sums(bn, orc, tune, g, splits=(1,))      # (the one-lane kernels: tests/test_emul_tail_patterns.py, and on the device)
