"""snarkjs' .zkey in and out and the H basis change (wsnark_g1_h_basis, wsnark_zkey_*, csrc/zkey.hip) on the CPU thread emulator: the
kernel SOURCES compiled by g++ (tests/emul).  tests/zkey_common.py holds the checks and their yardsticks (Python integers, a model
.zkey written from a synthetic circuit's toxic waste, the reference-format golden keys); tests/test_gpu_zkey.py runs them again on the
device at size.  The basis change stays at 2^1 .. 2^7 and keys at 2^3 and 2^6: an emulated lane is a coroutine."""
import pytest

import zkey_common as zk
from emul_util import SO_PATH, emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


def test_identity_in_python_integers():
    zk.check_identity_in_integers()


def test_wtns_format():
    zk.check_wtns_format()


def test_h_basis_is_its_definition_at_every_size(bn):
    zk.check_basis_definition(bn, 7)


@pytest.mark.parametrize("bits", [1, 5])
def test_h_basis_corner_inputs(bn, bits):
    zk.check_basis_corners(bn, bits)


def test_h_basis_per_lane_digits_give_the_same_bytes(bn, tune):
    zk.check_basis_uniform_switch(bn, 7, tune)


def test_h_basis_errors(bn):
    zk.check_basis_errors(bn)


@pytest.mark.parametrize("log_domain,style", [(3, "rows"), (6, "columns")])
def test_import_equals_the_closed_form_and_export_inverts_it(bn, log_domain, style):
    zk.check_import_closed_form(bn, log_domain, style)


def test_import_from_a_mapped_file(bn, tmp_path):
    zk.check_import_from_path(bn, tmp_path)


@pytest.mark.parametrize("name", ["t3", "t6"])
def test_golden_keys_export_and_come_back(bn, name):
    zk.check_golden_key(bn, name)


def test_trial_proof(bn):
    zk.check_trial_proof(bn, 3)


def test_record_order(bn, tune):
    zk.check_record_order(bn, 3, tune)


def test_partition_tile_edges(bn, tune):
    zk.check_tile_edges(bn, tune)


def test_errors_leave_outputs_and_report_untouched(bn):
    zk.check_errors(bn, SO_PATH)
