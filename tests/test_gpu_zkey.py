"""-m gpu: snarkjs' .zkey in and out and the H basis change (wsnark_g1_h_basis, wsnark_zkey_*, csrc/zkey.hip) of the hipcc-built
libwsnark.so on the device.  The checks of tests/test_emul_zkey.py again (tests/zkey_common.py holds them and their yardsticks) at
the sizes where the device kernels take their other paths: 2^7 and 2^8 straddle the switch between one twiddle per wavefront and
per-lane digits, from 2^10 a stage spans more than one 256-lane workgroup."""
import pytest

import zkey_common as zk

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


def test_h_basis_is_its_definition_at_every_size(bn):
    zk.check_basis_definition(bn, 10)


@pytest.mark.parametrize("bits", [1, 6, 10])
def test_h_basis_corner_inputs(bn, bits):
    zk.check_basis_corners(bn, bits)


def test_h_basis_per_lane_digits_give_the_same_bytes(bn, tune):
    zk.check_basis_uniform_switch(bn, 10, tune)


def test_h_basis_errors(bn):
    zk.check_basis_errors(bn)


@pytest.mark.parametrize("log_domain,style", [(3, "rows"), (6, "columns"), (8, "columns")])
def test_import_equals_the_closed_form_and_export_inverts_it(bn, log_domain, style):
    zk.check_import_closed_form(bn, log_domain, style)


def test_import_from_a_mapped_file(bn, tmp_path):
    zk.check_import_from_path(bn, tmp_path)


@pytest.mark.parametrize("name", ["t3", "t6"])
def test_golden_keys_export_and_come_back(bn, name):
    zk.check_golden_key(bn, name)


def test_trial_proof(bn):
    zk.check_trial_proof(bn, 6)


def test_record_order(bn, tune):
    zk.check_record_order(bn, 6, tune)


def test_partition_tile_edges(bn, tune):
    zk.check_tile_edges(bn, tune)


def test_errors_leave_outputs_and_report_untouched(bn):
    zk.check_errors(bn, bn.lib.path)
