"""The proving-key audit (wsnark_pkey_check*, csrc/pkeycheck.hip) on the CPU thread emulator: the kernel SOURCES compiled by g++
(tests/emul), every count and every first-bad index compared with the pure-Python classifier of tests/pkey_check_common.py, which
holds the checks themselves; tests/test_gpu_pkey_check.py runs them again on the device at size.  Keys are kept to a few hundred
variables: the emulator runs a wavefront's lanes one after the other, and a G2 subgroup chain costs it about a millisecond per
point (the whole file takes a little over a minute on one core; most of it is the emulated relation sums)."""
import pytest

import pkey_check_common as pk
from emul_util import SO_PATH, emul_bn128

CHUNK = 64      # the smallest chunk the library accepts: the 2^7 key then spans three chunks per section


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


@pytest.fixture(scope="module")
def key7(bn):
    return pk.synth_sections(bn, 7, seed=1)[2]


@pytest.fixture(scope="module")
def key5(bn):
    return pk.synth_sections(bn, 5, seed=2)[2]


@pytest.mark.parametrize("log_domain", [5, 6, 7])
def test_valid_keys_pass_through_every_entry_point(bn, tmp_path, log_domain):
    sec = pk.synth_sections(bn, log_domain, seed=log_domain)[2]
    rep = pk.check_valid_key(bn, sec, tmp_path)
    assert rep["A"]["infinity"] + rep["B1"]["infinity"] >= 2        # the last variable occurs in no row


def test_valid_key_with_absent_columns_and_in_chunks(bn, tmp_path, tune):
    """style="rows": ~40 % of the variables occur in no row of A (resp. B), so their key points are infinity."""
    from wasmsnark_amd import synth
    circ = synth.make_circuit(6, n_public=3, seed=8, style="rows")
    sec, _ = synth.build_sections(circ, synth.setup(circ, seed=80), bn.mul_base)
    whole = pk.check_valid_key(bn, sec, tmp_path)
    assert whole["A"]["infinity"] > 5 and whole["B1"]["infinity"] == whole["B2"]["infinity"] > 5
    tune(bn.lib, "PKCHECK_CHUNK", CHUNK)
    assert pk.no_ms(bn.check_key(sections=sec)) == pk.no_ms(whole)


def test_planted_points_one_section_at_a_time_and_several_at_once(bn, key7):
    fin = {s: pk.finite_indices(key7, s) for s in pk.SECTIONS}
    singles = [("A", pk.UNREDUCED), ("A", pk.OFF_CURVE), ("B1", pk.OFF_CURVE), ("B2", pk.UNREDUCED), ("B2", pk.OFF_CURVE), ("B2", pk.OUTSIDE),
               ("C", pk.UNREDUCED), ("H", pk.OFF_CURVE)]
    for k, (name, what) in enumerate(singles):
        # (with the relations for one case per section: the sums are the slow part on the emulator)
        pk.check_planted(bn, key7, [(name, fin[name][5 + 3 * k], what)], relations=what in (pk.OUTSIDE, pk.OFF_CURVE) and name != "B2" or what == pk.OUTSIDE)
    several = [("A", fin["A"][7], pk.OFF_CURVE), ("A", fin["A"][2], pk.UNREDUCED), ("B2", fin["B2"][40], pk.OUTSIDE), ("B2", fin["B2"][41], pk.OFF_CURVE),
               ("B2", fin["B2"][90], pk.UNREDUCED), ("C", fin["C"][11], pk.OFF_CURVE), ("H", fin["H"][100], pk.UNREDUCED), ("H", fin["H"][99], pk.OFF_CURVE)]
    rep, _ = pk.check_planted(bn, key7, several)
    assert [rep[s]["bad"] for s in pk.SECTIONS] == [2, 0, 3, 1, 2]
    assert rep["A"]["first_bad"] == fin["A"][2] and rep["A"]["first_reason"] == pk.UNREDUCED
    assert rep["B2"]["first_bad"] == fin["B2"][40] and rep["B2"]["first_reason"] == pk.OUTSIDE


def test_planted_points_at_the_ends_and_across_chunk_boundaries(bn, key7, tune):
    tune(bn.lib, "PKCHECK_CHUNK", CHUNK)
    for name, plants in pk.boundary_plants(key7, CHUNK):
        rep, _ = pk.check_planted(bn, key7, plants, relations=False)
        assert rep[name]["first_bad"] == plants[0][1]
    # both sides of a boundary at once, with the relations: the sums stop at the chunk that holds the bad point
    fin = pk.finite_indices(key7, "B1")
    below, above = max(i for i in fin if i < CHUNK), min(i for i in fin if i >= CHUNK)
    chunked, bad = pk.check_planted(bn, key7, [("B1", above, pk.OFF_CURVE), ("B1", below, pk.UNREDUCED), ("H", CHUNK - 1, pk.OFF_CURVE), ("H", CHUNK, pk.OFF_CURVE)])
    assert chunked["B1"]["first_bad"] == below and chunked["H"]["first_bad"] == CHUNK - 1
    tune(bn.lib, "PKCHECK_CHUNK", 1 << 18)
    assert pk.no_ms(bn.check_key(sections=bad)) == pk.no_ms(chunked)          # the report does not depend on the chunk size


def test_smallest_applicable_reason(bn, key5):
    pk.check_smallest_reason(bn, key5)


def test_subgroup_tests_agree(bn, key5, tune):
    fin = pk.finite_indices(key5, "B2")
    pk.check_subgroup_tests_agree(bn, key5, tune, [fin[0], fin[7], fin[8], fin[-1]])


def test_fixed_points(bn, key5):
    pk.check_fixed_points(bn, key5, relations_every=False)


def test_pseudo_key_has_good_points_and_no_relation(bn):
    pk.check_pseudo_key(bn)


def test_relations(bn, key5):
    pk.check_relations(bn, key5)


def test_errors_leave_the_report_untouched(bn, key5):
    pk.check_errors(bn, key5, SO_PATH)


def test_an_audit_changes_no_proof(bn):
    pk.check_no_side_effects(bn)


def test_load_key_check_option(bn):
    pk.check_load_key_option(bn)
