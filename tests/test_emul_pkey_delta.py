"""The phase-2 delta contribution (wsnark_g{1,2}_scale_batch, wsnark_pkey_contribute*, wsnark_pkey_delta_verify*,
csrc/pkeydelta.hip) on the CPU thread emulator: the kernel SOURCES compiled by g++ (tests/emul).  tests/pkey_delta_common.py holds
the checks and their yardsticks (Python integers, the closed form of a re-keyed synthetic key, the audit's classifier);
tests/test_gpu_pkey_delta.py runs them again on the device at size.  Keys stay at 2^5 .. 2^7 with PKDELTA_CHUNK = 64, so that
sections span chunks; the emulated relation sums dominate the run time."""
import pytest

import pkey_check_common as pk
import pkey_delta_common as pd
from emul_util import SO_PATH, emul_bn128

CHUNK = 64      # the smallest chunk the library accepts


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


@pytest.fixture(scope="module")
def key7_parts(bn):
    return pk.synth_sections(bn, 7, seed=1)      # the circuit, its toxic waste, the key's sections


@pytest.fixture(scope="module")
def key7(key7_parts):
    return key7_parts[2]


@pytest.fixture(scope="module")
def key5(bn):
    return pk.synth_sections(bn, 5, seed=2)[2]


@pytest.mark.parametrize("g", [1, 2])
def test_scale_batch_against_python_integers(bn, g):
    pd.check_scale_batch(bn, g)


@pytest.mark.parametrize("log_domain", [5, 7])
def test_rekeyed_key_equals_the_closed_form(bn, tmp_path, tune, log_domain):
    pd.check_closed_form(bn, tmp_path, tune, log_domain)


def test_shared_normalisation_gives_the_yardsticks_bytes(bn, key7_parts):
    """The one normalisation, an inversion per workgroup, against Python integers.  The contribution to key7 is the closed form: the
    same key built under delta * d.  70 points of B2 times r - 2 are g2_mul's: a partly filled workgroup passes 1 into the shared
    inversion, and the chain passes through -P."""
    circ, S, key7 = key7_parts
    pd.assert_same_key(bn.contribute_key(sections=key7, d=pd.D_FIXED)[0], pd.closed_form(bn, circ, S, pd.D_FIXED)[0])
    pts = bytes(key7["pointsB2"][:128 * 70])
    assert bn.scale_points(2, pts, pk.R - 2) == pd.expected_scale(2, pts, pk.R - 2)


def test_scale_batch_rejects_bad_points(bn):
    pd.check_scale_batch_rejects_bad_points(bn)


def test_the_new_key_works(bn):
    pd.check_new_key_works(bn)


def test_verify_contribution_accepts_and_rejects(bn, tmp_path):
    pd.check_verify_contribution(bn, tmp_path=tmp_path)


def test_bad_input_points_are_a_result(bn, key7, tmp_path, tune):
    pd.check_bad_inputs(bn, key7, tmp_path, tune, CHUNK)


def test_errors_leave_the_report_untouched(bn, key5, tmp_path):
    pd.check_errors(bn, key5, tmp_path, SO_PATH)


def test_library_drawn_secret(bn, key5):
    pd.check_library_drawn_secret(bn, key5)
