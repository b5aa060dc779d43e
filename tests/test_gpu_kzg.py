"""-m gpu: KZG commitments on powers of tau (wsnark_kzg_*, wsnark_fr_poly_eval, wsnark_fr_poly_divide; csrc/kzg.hip) of the hipcc-built
libwsnark.so on the device.  The checks of tests/test_emul_kzg.py again (tests/kzg_common.py holds them and their yardsticks), the
field side at the tile boundaries of the shipped run length, and a reference string of 2^12 powers: several workgroups in every
kernel of the sums, openings at len = n and len = n - 1 against mul_base and one Python evaluation."""
import pytest

import kzg_common as kz

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


# ---- the field side ----
def test_divide_and_eval_sizes_against_python_integers(bn):
    kz.check_divide_sizes(bn, (1, 2, 3, 63, 64, 65, 255, 256, 257) + kz.tile_sizes(kz.SEG_DEFAULT))


@pytest.mark.parametrize("seg", [1, 3])
def test_divide_at_the_tile_boundaries_of_a_forced_run_length(bn, tune, seg):
    kz.check_divide_forced_seg(bn, tune, seg)


def test_divide_with_more_tiles_than_the_carry_scan_has_lanes(bn, tune):
    tune(bn.lib, "KZG_SEG", 1)
    kz.check_divide_sizes(bn, (256 * 256 + 1,), seed=12)


def test_divide_bytes_do_not_depend_on_the_run_length(bn, tune):
    tune(bn.lib, "KZG_SEG", None)
    kz.check_divide_seg_independent(bn, tune, (1, 2, 255, 257, 769, 1027, 2051))


def test_divide_planted_points_and_polynomials(bn):
    kz.check_divide_planted(bn)


def test_eval_of_several_polynomials_equals_single_calls(bn):
    kz.check_eval_counts(bn)


# ---- the curve side ----
def test_commit_equals_the_closed_form_and_the_multiexp(bn, tune):
    kz.check_commit(bn, tune, 6, multiexp_lens=(1, 2, 15, 16, 63, 64))


def test_commit_of_evaluations_equals_commit_of_coefficients(bn):
    kz.check_commit_evaluations(bn, 6)


def test_open_equals_the_closed_form(bn):
    kz.check_open(bn, 6)


def test_verify_accepts_openings_and_rejects_each_spoilt_part(bn):
    kz.check_verify(bn, 6)


def test_commit_open_verify_on_another_generator(bn):
    kz.check_verify(bn, 6, s=0x123456789ABCDEF0FEDCBA9876543210)


def test_verify_input_points(bn):
    kz.check_verify_inputs(bn)


def test_two_threads_commit_on_one_handle(bn):
    kz.check_threads(bn, 6)


def test_errors_leave_outputs_and_handle_untouched(bn):
    kz.check_errors(bn, 6, bn.lib.path)


def test_srs_load_rejects_bad_powers_with_the_first_index(bn):
    kz.check_srs_load_errors(bn, 6)


# ---- 2^12 powers ----
def test_commit_and_open_on_4096_powers(bn, tune):
    kz.check_commit(bn, tune, 12, multiexp_lens=(4095,))
    kz.check_open(bn, 12)
