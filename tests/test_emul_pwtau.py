"""Powers of tau (wsnark_g{1,2}_mul_batch, wsnark_powers_contribute, wsnark_powers_check, csrc/pwtau.hip) on the CPU thread emulator:
the kernel SOURCES compiled by g++ (tests/emul).  tests/pwtau_common.py holds the checks and their yardsticks (Python integers,
mul_base on logarithms multiplied in Python, the closed form of a transcript from its toxic waste, the audit's classifier);
tests/test_gpu_pwtau.py runs them again on the device at size.  Transcripts stay at 2^4 (2^6 where an array must span two chunks of
64) and the relation cases run without the point tests where points are not the subject: an emulated MSM call takes about half a
second and an audit runs eight of them per chunk."""
import pytest

import pwtau_common as pw
from emul_util import SO_PATH, emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


@pytest.mark.parametrize("g", [1, 2])
def test_mul_points_against_python_integers(bn, g):
    pw.check_mul_integers(bn, g)


@pytest.mark.parametrize("g", [1, 2])
def test_mul_points_sizes_against_mul_base(bn, g):
    pw.check_mul_sizes(bn, g, (1, 63, 64, 65, 257))      # 257: just above the 256-lane workgroup of both curves


@pytest.mark.parametrize("g", [1, 2])
def test_mul_points_planted_scalars_and_infinities(bn, g):
    pw.check_mul_planted(bn, g)


@pytest.mark.parametrize("g", [1, 2])
def test_mul_points_one_point_many_scalars_and_one_scalar_many_points(bn, g):
    pw.check_mul_wavefront_shapes(bn, g)


def test_mul_points_g2_point_outside_the_subgroup(bn):
    pw.check_mul_outside_subgroup(bn)


@pytest.mark.parametrize("g", [1, 2])
def test_mul_points_both_chains_give_the_same_bytes(bn, g):
    pw.check_mul_modes(bn, g)


def test_mul_points_chunks(bn, tune):
    pw.check_mul_chunks(bn, tune)


def test_mul_points_errors(bn):
    pw.check_mul_errors(bn, SO_PATH)


# ---- the contribution ----
def test_contribution_equals_the_closed_form(bn, tune):
    pw.check_contribution_closed_form(bn, tune, 4)


def test_contribution_spanning_chunks(bn, tune):
    pw.check_contribution_closed_form(bn, tune, 6, chunks=(64,))


def test_contribution_in_place(bn):
    pw.check_contribution_in_place(bn, 4)


def test_two_contributions_equal_one_by_the_products(bn):
    pw.check_contribution_twice(bn, 4)


def test_contribution_with_drawn_secrets(bn):
    pw.check_contribution_drawn_secrets(bn, 4)


def test_contribution_rejects_a_zero_secret(bn):
    pw.check_contribution_zero_secret(bn, 4)


def test_contribution_bad_powers_are_a_result(bn):
    pw.check_contribution_bad_powers(bn, 6)


def test_powers_errors_leave_report_and_outputs_untouched(bn):
    pw.check_powers_errors(bn, 4)


def test_contributed_transcript_passes_the_audit_and_makes_the_closed_form_key(bn):
    pw.check_chain(bn, 4)


# ---- the audit ----
def test_audit_of_a_good_transcript(bn):
    pw.check_audit_good(bn, 4)


def test_audit_one_case_per_relation(bn):
    pw.check_audit_relations(bn, 4, points=False)


def test_audit_at_the_overlap_of_two_chunks(bn, tune):
    pw.check_audit_chunk_overlap(bn, tune, 6, points=False)


def test_audit_counts_a_point_outside_the_subgroup(bn):
    pw.check_audit_outside_subgroup(bn, 4)


def test_audit_seed_and_halves(bn):
    pw.check_audit_seed_and_halves(bn, 4)
