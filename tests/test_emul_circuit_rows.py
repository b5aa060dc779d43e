"""Circuits in row form (wsnark_circuit_from_rows_size / _from_rows / _load_rows, csrc/circuitrows.hip) on the CPU thread emulator: the
kernel SOURCES compiled by g++ (tests/emul).  tests/circuit_rows_common.py holds the cases, the checks and their yardstick (a plain
Python model of the record streams); tests/test_gpu_circuit_rows.py runs them again on the device.  The end-to-end checks run at 2^6
here (2^4 where a key is set up or a proof made) and at 2^8 there."""
import pytest

import circuit_rows_common as cr
from emul_util import SO_PATH, emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


def test_the_model_on_a_circuit_written_down():
    cr.check_model_itself()


def test_rows_from_constraints_packs_terms_in_order():
    cr.check_rows_from_constraints()


@pytest.mark.parametrize("name", list(cr.CASES))
def test_streams_are_the_models_bytes(bn, name):
    cr.check_case(bn, name)


@pytest.mark.parametrize("name", list(cr.CASES))
def test_resident_circuit_from_rows_is_the_one_from_the_streams(bn, name):
    cr.check_resident(bn, name)


@pytest.mark.parametrize("name", ["ties", "special coefficients", "hot column, the last signal", "C empty, no public rows"])
def test_the_c_entry_point_on_a_struct_written_down(bn, name):
    cr.check_raw_struct(bn, name)


def test_errors_write_nothing(bn):
    cr.check_errors(bn, SO_PATH)


@pytest.mark.parametrize("style", ["columns", "rows"])
def test_synth_circuit_streams_and_row_sums(bn, style):
    cr.check_e2e_streams(bn, 6, style)
    cr.check_e2e_row_sums(bn, 6, style)


@pytest.mark.parametrize("style", ["columns", "rows"])
def test_synth_circuit_setup_key(bn, style):
    cr.check_e2e_setup_key(bn, 4, style)


@pytest.mark.parametrize("style", ["columns", "rows"])
def test_synth_circuit_witness_checks(bn, style):
    cr.check_e2e_witnesses(bn, 6, style)


def test_gen_proof_with_a_circuit_from_rows(bn):
    cr.check_e2e_gen_proof(bn, 4)
