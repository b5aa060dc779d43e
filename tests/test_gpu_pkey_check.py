"""-m gpu: the proving-key audit (wsnark_pkey_check*, csrc/pkeycheck.hip) of the hipcc-built libwsnark.so on the device.  The
checks of tests/test_emul_pkey_check.py again (tests/pkey_check_common.py: every count and first-bad index against the pure-Python
classifier), then what only a device can show: keys of 2^16 and 2^20 constraints with seeded planted points, and an audit beside
a proof on another host thread."""
import random
import threading

import pytest

import pkey_check_common as pk

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
def key7(bn):
    return pk.synth_sections(bn, 7, seed=1)[2]


@pytest.fixture(scope="module")
def key16(bn):
    from wasmsnark_amd import synth
    sec = synth.NativeCircuit(bn.lib, 16, n_public=2, seed=3, style="rows").build_sections()[0]
    return pk.mutable(sec)       # (bytearrays, like every other key here; never written)


@pytest.mark.parametrize("log_domain", [5, 6, 7])
def test_valid_keys_pass_through_every_entry_point(bn, tmp_path, log_domain):
    sec = pk.synth_sections(bn, log_domain, seed=log_domain)[2]
    pk.check_valid_key(bn, sec, tmp_path)


def test_valid_key_2p16_with_absent_columns(bn, key16, tmp_path, tune):
    """style="rows": a large share of the variables occurs in no row of A (resp. B): their key points are infinity."""
    whole = pk.check_valid_key(bn, key16, tmp_path, classify_all=False)
    assert whole["A"]["infinity"] > 1000 and whole["B1"]["infinity"] == whole["B2"]["infinity"] > 1000
    for chunk in (64, 1000, 1 << 14):
        tune(bn.lib, "PKCHECK_CHUNK", chunk)
        assert pk.no_ms(bn.check_key(sections=key16)) == pk.no_ms(whole), chunk


def test_valid_key_2p20(bn, tmp_path):
    from wasmsnark_amd import synth
    sec = synth.NativeCircuit(bn.lib, 20, n_public=2, seed=5).build_sections()[0]
    rep = pk.check_valid_key(bn, sec, tmp_path, classify_all=False)
    assert rep["H"]["points"] == 1 << 20
    # three planted points in three sections: the exact report
    bad = pk.mutable(sec)
    fin = {s: pk.finite_indices(bad, s) for s in ("A", "B2", "H")}
    plants = [("A", fin["A"][-1], pk.UNREDUCED), ("B2", fin["B2"][len(fin["B2"]) // 2], pk.OUTSIDE), ("H", fin["H"][(1 << 18) + 1], pk.OFF_CURVE)]
    for p in plants:
        pk.plant(bad, *p)
    got = bn.check_key(sections=bad)
    want = pk.no_ms(rep)
    want["ok"] = False
    for name, i, why in plants:
        want[name] = dict(want[name], bad=1, first_bad=i, first_reason=why)
        assert pk.classify(bad[pk.SEC_KEY[name]][pk.SEC_SIZE[name] * i:pk.SEC_SIZE[name] * (i + 1)]) == why
    want["relations"] = dict(want["relations"], **{"B1~B2": None})
    want["relations_run"] = 3
    assert pk.no_ms(got) == want


def test_planted_points_one_section_at_a_time_and_several_at_once(bn, key7):
    fin = {s: pk.finite_indices(key7, s) for s in pk.SECTIONS}
    singles = [("A", pk.UNREDUCED), ("A", pk.OFF_CURVE), ("B1", pk.UNREDUCED), ("B1", pk.OFF_CURVE), ("B2", pk.UNREDUCED), ("B2", pk.OFF_CURVE),
               ("B2", pk.OUTSIDE), ("C", pk.UNREDUCED), ("C", pk.OFF_CURVE), ("H", pk.UNREDUCED), ("H", pk.OFF_CURVE)]
    for k, (name, what) in enumerate(singles):
        pk.check_planted(bn, key7, [(name, fin[name][5 + 3 * k], what)])
    several = [("A", fin["A"][7], pk.OFF_CURVE), ("A", fin["A"][2], pk.UNREDUCED), ("B2", fin["B2"][40], pk.OUTSIDE), ("B2", fin["B2"][41], pk.OFF_CURVE),
               ("B2", fin["B2"][90], pk.UNREDUCED), ("C", fin["C"][11], pk.OFF_CURVE), ("H", fin["H"][100], pk.UNREDUCED), ("H", fin["H"][99], pk.OFF_CURVE)]
    rep, _ = pk.check_planted(bn, key7, several)
    assert [rep[s]["bad"] for s in pk.SECTIONS] == [2, 0, 3, 1, 2]


def test_planted_points_at_the_ends_and_across_chunk_boundaries(bn, key7, tune):
    chunk = 64
    tune(bn.lib, "PKCHECK_CHUNK", chunk)
    for name, plants in pk.boundary_plants(key7, chunk):
        rep, _ = pk.check_planted(bn, key7, plants)
        assert rep[name]["first_bad"] == plants[0][1]
    fin = pk.finite_indices(key7, "B1")
    below, above = max(i for i in fin if i < chunk), min(i for i in fin if i >= chunk)
    chunked, bad = pk.check_planted(bn, key7, [("B1", above, pk.OFF_CURVE), ("B1", below, pk.UNREDUCED), ("H", chunk - 1, pk.OFF_CURVE), ("H", chunk, pk.OFF_CURVE)])
    assert chunked["B1"]["first_bad"] == below and chunked["H"]["first_bad"] == chunk - 1
    tune(bn.lib, "PKCHECK_CHUNK", 1 << 18)
    assert pk.no_ms(bn.check_key(sections=bad)) == pk.no_ms(chunked)


def test_smallest_applicable_reason(bn, key7):
    pk.check_smallest_reason(bn, key7)


def test_seeded_sample_at_2p16(bn, key16, tune):
    """About 50 planted points per section at seeded random indices: bad[] equals the planted counts; the classifier, run on every
    planted point and on 200 untouched ones per section, agrees with the counts and with first_bad.  The same report from the psi
    subgroup test."""
    rnd = random.Random(2016)
    bad = pk.mutable(key16)
    kinds = {"A": (pk.UNREDUCED, pk.OFF_CURVE, "both"), "B1": (pk.UNREDUCED, pk.OFF_CURVE), "B2": (pk.UNREDUCED, pk.OFF_CURVE, pk.OUTSIDE, pk.OUTSIDE, "both"),
             "C": (pk.OFF_CURVE, pk.UNREDUCED), "H": (pk.OFF_CURVE, pk.UNREDUCED, "both")}
    planted, sample = {}, {}
    for name in pk.SECTIONS:
        fin = pk.finite_indices(bad, name)
        pick = rnd.sample(fin, 250)
        planted[name] = {i: rnd.choice(kinds[name]) for i in pick[:50]}
        sample[name] = pick[50:]
        for i, what in planted[name].items():
            pk.plant(bad, name, i, what)
    rep = bn.check_key(sections=bad)
    clean = bn.check_key(sections=key16, relations=False)
    for name in pk.SECTIONS:
        size, buf = pk.SEC_SIZE[name], bad[pk.SEC_KEY[name]]
        assert rep[name]["bad"] == 50, (name, rep[name])
        inf, nbad, first, reason = pk.expected_section(buf, size, indices=list(planted[name]) + sample[name])
        assert (inf, nbad, first, reason) == (0, 50, rep[name]["first_bad"], rep[name]["first_reason"]), (name, rep[name], (inf, nbad, first, reason))
        for i, what in planted[name].items():        # every planted point, under its smallest applicable reason
            assert pk.classify(buf[size * i:size * i + size]) == (pk.UNREDUCED if what == "both" else what), (name, i, what)
        assert rep[name]["infinity"] == clean[name]["infinity"]
    assert rep["ok"] is False and rep["relations"] == {"beta1~beta2": True, "delta1~delta2": True, "B1~B2": None}
    tune(bn.lib, "PKCHECK_SUBGROUP", 1)
    assert pk.no_ms(bn.check_key(sections=bad)) == pk.no_ms(rep)


def test_subgroup_tests_agree(bn, key7, tune):
    fin = pk.finite_indices(key7, "B2")
    pk.check_subgroup_tests_agree(bn, key7, tune, [fin[0], fin[7], fin[70], fin[-1]])


def test_fixed_points(bn, key7):
    pk.check_fixed_points(bn, key7)


def test_pseudo_key_has_good_points_and_no_relation(bn):
    pk.check_pseudo_key(bn, n_vars=700, n_public=3, domain=512)


def test_relations(bn, key7, key16):
    pk.check_relations(bn, key7)
    pk.check_relations(bn, key16)


def test_errors_leave_the_report_untouched(bn, key7):
    pk.check_errors(bn, key7, bn.lib.path)


def test_an_audit_changes_no_proof(bn):
    pk.check_no_side_effects(bn, log_domain=10)


def test_load_key_check_option(bn):
    pk.check_load_key_option(bn, log_domain=8)


def test_an_audit_beside_a_proof_on_another_thread(bn, key16):
    from wasmsnark_amd import synth
    circ = synth.make_circuit(12, n_public=2, seed=4)
    S = synth.setup(circ, seed=40)
    pkey, _ = synth.build_key(circ, S, bn.mul_base)
    key = bn.load_key(pkey)
    wit = synth.witness_bin(circ)
    r, s = bytes([1]) * 32, bytes([200]) * 32
    proof = bn.groth16GenProof(wit, key, r=r, s=s)
    assert proof == synth.expected_proof(circ, S, r, s, bn.mul_base)
    bad = pk.mutable(key16)
    pk.plant(bad, "B2", pk.finite_indices(bad, "B2")[12345], pk.OUTSIDE)
    ref_good, ref_bad = bn.check_key(sections=key16, seed=bytes(32)), bn.check_key(sections=bad, seed=bytes(32))
    assert ref_good["ok"] is True and ref_bad["B2"]["bad"] == 1
    out = {}

    def prove():
        out["proofs"] = [bn.groth16GenProof(wit, key, r=r, s=s) for _ in range(8)]

    t = threading.Thread(target=prove)
    t.start()
    out["good"], out["bad"] = bn.check_key(sections=key16, seed=bytes(32)), bn.check_key(sections=bad, seed=bytes(32))
    t.join()
    assert pk.no_ms(out["good"]) == pk.no_ms(ref_good) and pk.no_ms(out["bad"]) == pk.no_ms(ref_bad) and out["proofs"] == [proof] * 8
    key.free()
