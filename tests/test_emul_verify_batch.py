"""The batch verifier (wsnark_groth16_verify_batch, csrc/pairing.hip + fp12.h) on the CPU thread emulator: the kernel SOURCES
compiled by g++ (tests/emul), every status compared with the pinned single-proof host verifier.  The checks themselves are in
tests/verify_batch_common.py; tests/test_gpu_verify_batch.py runs them again on the device.  Batches are kept small: the
emulator runs a wavefront's lanes one after the other (the whole file takes about a minute on one core, half of it the planted
table of verify_batch_common.py section 7)."""
import pytest

import verify_batch_common as vb
from emul_util import SO_PATH, emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


def test_fp12_device_against_host(bn):
    vb.check_fp12(bn, n_random=8)


def test_reference_verifier_vectors_in_one_batch_and_alone(bn):
    vb.check_golden_verify(bn)


@pytest.mark.parametrize("name", ["t3", "t6"])
def test_golden_proofs_in_one_batch(bn, name):
    vb.check_golden_proofs(bn, name)


def test_malformed_proofs_between_valid_neighbours(bn):
    vb.check_mixed_batches(bn, sizes=(1, 2, 63, 65, 131))


def test_key_level_outcomes(bn):
    vb.check_key_level(bn, SO_PATH)


def test_python_argument_errors(bn):
    vb.check_python_argument_errors(bn)


@pytest.mark.parametrize("n_public", [1, 5])
def test_forged_proofs_and_flipped_bits(bn, n_public):
    vb.check_forged(bn, n_public, 24)


def test_mul_base_gives_the_reference_points(bn):
    vb.check_mul_base_against_reference(bn)


@pytest.mark.parametrize("what", ["rows", "alone", "host", "shuffled"])
def test_planted_keys_inputs_and_proofs(bn, what):
    vb.check_planted(bn, what=(what,))


@pytest.mark.parametrize("plain", [1, 2])
def test_planted_with_the_plain_exponents(bn, tune, plain):
    # (each row in one call; the shuffled batches with their neighbours run under both exponents on the device, where they cost nothing)
    vb.check_planted(bn, what=("rows",), plain=plain, tune=tune)
