"""-m gpu: the phase-2 delta contribution (wsnark_g{1,2}_scale_batch, wsnark_pkey_contribute*, wsnark_pkey_delta_verify*,
csrc/pkeydelta.hip) of the hipcc-built libwsnark.so on the device.  The checks of tests/test_emul_pkey_delta.py again
(tests/pkey_delta_common.py holds them and their yardsticks), then keys of 2^16 and 2^20 constraints against the closed form."""
import pytest

import pkey_check_common as pk
import pkey_delta_common as pd

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


def test_rekeyed_key_2p16_equals_the_closed_form(bn, tmp_path, tune):
    sec, want = pd.native_closed_form(bn, 16, pd.D_FIXED, seed=3)
    pd.check_closed_form_sections(bn, tmp_path, tune, sec, want, pd.D_FIXED, ((64, False), (1000, True), (None, False)))
    # the relation check at size: the re-keyed key is accepted, one replaced C' point and a wrong delta2' are found
    assert bn.verify_contribution(sec, want, check=False)["ok"] is True
    bad = dict(want, pointsC=bytearray(want["pointsC"]))
    fin = pk.finite_indices(bad, "C")
    i, j = fin[len(fin) // 2], fin[-1]
    bad["pointsC"][64 * i:64 * i + 64] = bytes(want["pointsC"][64 * j:64 * j + 64])
    v = bn.verify_contribution(sec, bad, check=False)
    assert v["checks_bad"] == pd.BIT["C"] and v["checks_run"] == 31


def test_rekeyed_key_2p20_equals_the_closed_form(bn, tmp_path, tune):
    sec, want = pd.native_closed_form(bn, 20, pd.D_FIXED, seed=5, style="columns")
    assert len(sec["pointsH"]) // 64 == 1 << 20
    pd.check_closed_form_sections(bn, tmp_path, tune, sec, want, pd.D_FIXED, ((100003, True), (None, False)), with_pkey=False)
    assert bn.check_key(sections=want)["ok"] is True
    assert bn.verify_contribution(sec, want, check=False)["ok"] is True


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
    pd.check_new_key_works(bn, log_domain=7)


def test_verify_contribution_accepts_and_rejects(bn, tmp_path):
    pd.check_verify_contribution(bn, log_domain=6, tmp_path=tmp_path)


def test_bad_input_points_are_a_result(bn, key7, tmp_path, tune):
    pd.check_bad_inputs(bn, key7, tmp_path, tune, 64)


def test_errors_leave_the_report_untouched(bn, key5, tmp_path):
    pd.check_errors(bn, key5, tmp_path, bn.lib.path)


def test_library_drawn_secret(bn, key5):
    pd.check_library_drawn_secret(bn, key5)
