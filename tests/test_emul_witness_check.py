"""The witness check (wsnark_witness_check, wsnark_circuit_load / _witness_check, csrc/witcheck.hip) on the CPU thread emulator: the
kernel SOURCES compiled by g++ (tests/emul).  tests/witness_check_common.py holds the checks and their yardstick (Python integers over
the circuit's rows); tests/test_gpu_witness_check.py runs them again on the device.  2^4 is less than a wavefront, 2^6 exactly one."""
import pytest

import witness_check_common as wc
from emul_util import SO_PATH, emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


@pytest.mark.parametrize("style", ["columns", "rows"])
@pytest.mark.parametrize("log_domain", [4, 6])
def test_good_witnesses_pass(bn, log_domain, style):
    wc.check_good(bn, log_domain, style)


@pytest.mark.parametrize("log_domain", [4, 6])
def test_planted_failures_give_exactly_the_python_set(bn, log_domain):
    wc.check_planted(bn, log_domain)


def test_truncated_lists_and_every_verdict_of_the_hand_built_circuit(bn):
    wc.check_truncation(bn, 6)


def test_unreduced_signals(bn):
    wc.check_unreduced(bn, 6)


def test_a_longer_witness_buffer_is_accepted(bn):
    wc.check_longer_buffer(bn, 4)


def test_errors_leave_the_report_and_the_lists_untouched(bn):
    wc.check_errors(bn, SO_PATH, 4)


def test_one_handle_two_threads(bn):
    wc.check_two_threads(bn, 6)


def test_gen_proof_checks_the_witness_first(bn):
    wc.check_gen_proof(bn, 4)
