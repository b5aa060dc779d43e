"""-m gpu: the key setup from powers of tau (wsnark_g{1,2}_ntt, wsnark_pkey_setup*, csrc/pkeysetup.hip) of the hipcc-built
libwsnark.so on the device.  The checks of tests/test_emul_pkey_setup.py again (tests/pkey_setup_common.py holds them and their
yardsticks) at the sizes where the device kernels take their other paths: from 2^7 a wavefront shares one twiddle in the early
stages, from 2^10 a stage spans more than one 256-lane workgroup."""
import pytest

import pkey_setup_common as ps

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


@pytest.mark.parametrize("g", [1, 2])
def test_group_ntt_is_its_definition(bn, g):
    ps.check_ntt_definition(bn, g)


@pytest.mark.parametrize("g", [1, 2])
def test_group_ntt_every_size(bn, g):
    ps.check_ntt_sizes(bn, g, 11)


def test_group_ntt_agrees_with_the_fr_transform(bn):
    ps.check_ntt_agrees_with_fr(bn, 9)


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("bits", [6, 10])
def test_group_ntt_corner_inputs(bn, g, bits):
    ps.check_ntt_corners(bn, g, bits)


@pytest.mark.parametrize("g", [1, 2])
def test_group_ntt_round_trip(bn, g):
    ps.check_ntt_round_trip(bn, g, 11)


def test_group_ntt_errors(bn):
    ps.check_ntt_errors(bn, bn.lib.path)


# ---- the setup ----
@pytest.mark.parametrize("log_domain,style", [(6, "rows"), (10, "columns")])
def test_new_key_equals_the_closed_form(bn, tune, log_domain, style):
    ps.check_setup_closed_form(bn, tune, log_domain, style, msm_mins=(None, 2, 1 << 20) if log_domain == 6 else (None, 1 << 20))


def test_new_key_with_a_long_column(bn, tune):
    ps.check_setup_long_column(bn, tune, 6)


@pytest.mark.parametrize("log_domain,style", [(6, "columns"), (10, "rows")])
def test_new_key_chains_to_audit_contribution_and_its_check(bn, log_domain, style):
    ps.check_setup_chain(bn, log_domain, style)


def test_the_new_key_proves_and_verifies(bn):
    ps.check_setup_key_works(bn, 6)


def test_bad_powers_are_a_result(bn):
    ps.check_setup_bad_powers(bn, 10)


def test_setup_errors_leave_report_and_outputs_untouched(bn):
    ps.check_setup_errors(bn, 6, bn.lib.path)
