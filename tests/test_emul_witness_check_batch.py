"""The batch witness check (wsnark_circuit_witness_check_batch, csrc/witcheck.hip) and groth16GenProofBatch(..., circuit=rc) on the CPU
thread emulator: the kernel SOURCES compiled by g++ (tests/emul).  tests/witness_check_batch_common.py holds the checks and their
yardsticks (Python integers over the circuit's rows, and the single resident call); tests/test_gpu_witness_check_batch.py runs them
again on the device.  2^4 is less than a wavefront -- a witness takes one with idle lanes --, 2^6 exactly one."""
import pytest

import witness_check_batch_common as wb
from emul_util import SO_PATH, emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


@pytest.mark.parametrize("style", ["columns", "rows"])
@pytest.mark.parametrize("count", [1, 2, 5, 65])
@pytest.mark.parametrize("log_domain", [4, 6])
def test_equals_the_single_call_and_python(bn, log_domain, count, style):
    wb.check_equals_single(bn, log_domain, style, count)


@pytest.mark.parametrize("log_domain", [4, 6])
def test_the_pass_size_changes_nothing(bn, log_domain):
    wb.check_geometry(bn, log_domain)


def test_stride_blob_and_sequence(bn):
    wb.check_stride(bn, 6)


def test_the_hand_built_circuit_between_two_zero_witnesses(bn):
    wb.check_hand_built(bn, 6)


def test_unreduced_signals_and_signal_0_per_witness(bn):
    wb.check_unreduced(bn, 6)


def test_errors_leave_everything_untouched(bn):
    wb.check_errors(bn, SO_PATH, 4)


def test_two_threads_one_handle_two_batches(bn):
    wb.check_two_threads(bn, 6)


def test_the_batch_prover_checks_the_witnesses_first(bn):
    wb.check_gen_proof_batch(bn, 6)
