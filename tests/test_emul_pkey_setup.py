"""The key setup from powers of tau (wsnark_g{1,2}_ntt, wsnark_pkey_setup*, csrc/pkeysetup.hip) on the CPU thread emulator: the
kernel SOURCES compiled by g++ (tests/emul).  tests/pkey_setup_common.py holds the checks and their yardsticks (Python integers,
the closed form of a synthetic key under delta = gamma = 1, the audit's classifier); tests/test_gpu_pkey_setup.py runs them again
on the device at size.  Transforms stay at 2^0 .. 2^7 and keys at 2^4 and 2^6: an emulated lane is a coroutine."""
import pytest

import pkey_setup_common as ps
from emul_util import SO_PATH, emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


def test_python_transforms_agree():
    ps.check_python_transforms_agree()


@pytest.mark.parametrize("g", [1, 2])
def test_group_ntt_is_its_definition(bn, g):
    ps.check_ntt_definition(bn, g)


@pytest.mark.parametrize("g", [1, 2])
def test_group_ntt_every_size(bn, g):
    ps.check_ntt_sizes(bn, g, 7)


def test_group_ntt_agrees_with_the_fr_transform(bn):
    ps.check_ntt_agrees_with_fr(bn, 5)


@pytest.mark.parametrize("g", [1, 2])
def test_group_ntt_corner_inputs(bn, g):
    ps.check_ntt_corners(bn, g, 6)


def test_group_ntt_round_trip(bn):
    ps.check_ntt_round_trip(bn, 1, 6)
    ps.check_ntt_round_trip(bn, 2, 4)


def test_group_ntt_errors(bn):
    ps.check_ntt_errors(bn, SO_PATH)


# ---- the setup ----
@pytest.mark.parametrize("log_domain,style", [(4, "rows"), (6, "columns")])
def test_new_key_equals_the_closed_form(bn, tune, log_domain, style):
    # PKSETUP_MSM_MIN = 2 at the small domain only: an emulated MSM call takes half a second
    ps.check_setup_closed_form(bn, tune, log_domain, style, msm_mins=(None, 2, 1 << 20) if log_domain == 4 else (None, 1 << 20))


def test_new_key_with_a_long_column(bn, tune):
    ps.check_setup_long_column(bn, tune, 6)


@pytest.mark.parametrize("log_domain,style", [(4, "columns"), (6, "rows")])
def test_new_key_chains_to_audit_contribution_and_its_check(bn, log_domain, style):
    ps.check_setup_chain(bn, log_domain, style)


def test_the_new_key_proves_and_verifies(bn):
    ps.check_setup_key_works(bn, 4)


def test_bad_powers_are_a_result(bn):
    ps.check_setup_bad_powers(bn, 6)


def test_setup_errors_leave_report_and_outputs_untouched(bn):
    ps.check_setup_errors(bn, 4, SO_PATH)
