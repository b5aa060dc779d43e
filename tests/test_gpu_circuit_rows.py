"""-m gpu: circuits in row form (wsnark_circuit_from_rows_size / _from_rows / _load_rows, csrc/circuitrows.hip) of the hipcc-built
libwsnark.so on the device.  The cases and checks of tests/test_emul_circuit_rows.py again (tests/circuit_rows_common.py holds them and
their yardstick, a plain Python model of the record streams), and the end-to-end checks at 2^8 with synth.make_circuit in both styles."""
import pytest

import circuit_rows_common as cr

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
    cr.check_errors(bn, bn.lib.path)


@pytest.mark.parametrize("style", ["columns", "rows"])
def test_synth_circuit_streams_and_row_sums(bn, style):
    cr.check_e2e_streams(bn, 8, style)
    cr.check_e2e_row_sums(bn, 8, style)


@pytest.mark.parametrize("style", ["columns", "rows"])
def test_synth_circuit_setup_key(bn, style):
    cr.check_e2e_setup_key(bn, 8, style)


@pytest.mark.parametrize("style", ["columns", "rows"])
def test_synth_circuit_witness_checks(bn, style):
    cr.check_e2e_witnesses(bn, 8, style)


def test_gen_proof_with_a_circuit_from_rows(bn):
    cr.check_e2e_gen_proof(bn, 8)
