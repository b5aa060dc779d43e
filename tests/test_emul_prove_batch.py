"""The batch prover (wsnark_groth16_prove_batch, csrc/provebatch.hip) on the CPU thread emulator: the kernel SOURCES compiled by g++
(tests/emul).  tests/prove_batch_common.py holds the checks; their yardstick is the single prover on the same handle, byte for byte.
tests/test_gpu_prove_batch.py runs them again on the device.  2^4 is less than a wavefront of points, 2^6 exactly one; a batch of 65 is
one more than a wavefront of proofs in the assembly kernels."""
import pytest

import prove_batch_common as pb
from emul_util import SO_PATH, emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("style", ["columns", "rows"])
@pytest.mark.parametrize("log_domain", [4, 6])
def test_equals_the_single_prover(bn, log_domain, style, count):
    pb.check_equals_single(bn, log_domain, style, count)


def test_equals_the_single_prover_65_proofs(bn):
    pb.check_equals_single(bn, 4, "rows", 65)


def test_the_references_own_proofs(bn):
    pb.check_reference_proofs(bn)


@pytest.mark.parametrize("log_domain", [4, 6])
def test_adversarial_witnesses_in_one_batch(bn, log_domain):
    pb.check_adversarial(bn, log_domain)


def test_boolean_heavy_witness(bn):
    pb.check_boolean_heavy(bn, 6)


@pytest.mark.parametrize("log_domain", [4, 6])
def test_planted_equal_and_opposite_points(bn, log_domain):
    pb.check_planted_points(bn, log_domain)


def test_geometry_and_routing_change_nothing(bn):
    pb.check_geometry(bn, 4)


def test_drawn_blinding(bn):
    pb.check_drawn_blinding(bn, 4)


def test_errors_leave_the_outputs_and_the_report_untouched(bn):
    pb.check_errors(bn, SO_PATH, 4)


def test_two_threads_one_handle(bn):
    pb.check_two_threads(bn, 4)
