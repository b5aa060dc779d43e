"""-m gpu: powers of tau (wsnark_g{1,2}_mul_batch, wsnark_powers_contribute, wsnark_powers_check, csrc/pwtau.hip) of the hipcc-built
libwsnark.so on the device.  The checks of tests/test_emul_pwtau.py again (tests/pwtau_common.py holds them and their yardsticks)
at the sizes where the device kernel can go wrong: a partial last wavefront (63, 65), a partial last workgroup (255, 257), several
workgroups (1000), arrays that span chunks of 64 and 256 points."""
import pytest

import pwtau_common as pw

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
def test_mul_points_against_python_integers(bn, g):
    pw.check_mul_integers(bn, g)


@pytest.mark.parametrize("g", [1, 2])
def test_mul_points_sizes_against_mul_base(bn, g):
    pw.check_mul_sizes(bn, g, (1, 63, 64, 65, 255, 256, 257, 1000))


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
    pw.check_mul_modes(bn, g, n=300)


def test_mul_points_chunks(bn, tune):
    pw.check_mul_chunks(bn, tune)


def test_mul_points_errors(bn):
    pw.check_mul_errors(bn, bn.lib.path)


# ---- the contribution ----
@pytest.mark.parametrize("log_domain,chunks", [(6, (None,)), (10, (64, 256, None))])
def test_contribution_equals_the_closed_form(bn, tune, log_domain, chunks):
    pw.check_contribution_closed_form(bn, tune, log_domain, chunks)


def test_contribution_in_place(bn):
    pw.check_contribution_in_place(bn, 6)


def test_two_contributions_equal_one_by_the_products(bn):
    pw.check_contribution_twice(bn, 6)


def test_contribution_with_drawn_secrets(bn):
    pw.check_contribution_drawn_secrets(bn, 6)


def test_contribution_rejects_a_zero_secret(bn):
    pw.check_contribution_zero_secret(bn, 6)


def test_contribution_bad_powers_are_a_result(bn):
    pw.check_contribution_bad_powers(bn, 10)


def test_powers_errors_leave_report_and_outputs_untouched(bn):
    pw.check_powers_errors(bn, 6)


@pytest.mark.parametrize("log_domain", [6, 10])
def test_contributed_transcript_passes_the_audit_and_makes_the_closed_form_key(bn, log_domain):
    pw.check_chain(bn, log_domain)


# ---- the audit ----
@pytest.mark.parametrize("log_domain", [6, 10])
def test_audit_of_a_good_transcript(bn, log_domain):
    pw.check_audit_good(bn, log_domain)


def test_audit_one_case_per_relation(bn):
    pw.check_audit_relations(bn, 6, points=True)


def test_audit_at_the_overlap_of_two_chunks(bn, tune):
    pw.check_audit_chunk_overlap(bn, tune, 8, points=True)


def test_audit_counts_a_point_outside_the_subgroup(bn):
    pw.check_audit_outside_subgroup(bn, 6)


def test_audit_seed_and_halves(bn):
    pw.check_audit_seed_and_halves(bn, 6)
