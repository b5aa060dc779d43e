"""Shared checks of the proving-key audit (wsnark_pkey_check / _check_sections / _check_file, csrc/pkeycheck.hip), run by
tests/test_emul_pkey_check.py on the thread-emulator build of the kernel sources and by tests/test_gpu_pkey_check.py on the device.

The yardstick is never the code under test: `classify()` below decides every point with Python integers -- x == 0 (the loaders'
infinity), every coordinate < Q, the curve equation after leaving Montgomery form, and [r] Q == O by double-and-add over Fq2 --
and `expected_sections()` folds those verdicts into what the report must hold for a section: count of infinities, count of bad
points, the smallest bad index and its smallest applicable reason."""
import ctypes as C
import os
import random
import subprocess
import sys

from bn128_ref import Q, R, RINV, g1_on_curve, g2_on_twist, g2_times_r_is_infinity, le, mont, twist_point_outside_g2

OK, ERR_SIZE, ERR_FORMAT, ERR_ARG, ERR_NOINIT = 0, 1, 2, 4, 5
SECTIONS = ("A", "B1", "B2", "C", "H")
SEC_KEY = {"A": "pointsA", "B1": "pointsB1", "B2": "pointsB2", "C": "pointsC", "H": "pointsH"}
SEC_SIZE = {"A": 64, "B1": 64, "B2": 128, "C": 64, "H": 64}
FIXED = ("alfa1", "beta1", "delta1", "beta2", "delta2")
UNREDUCED, OFF_CURVE, OUTSIDE, INFINITY = "unreduced", "off_curve", "outside_subgroup", "infinity"


# ---- the yardstick (the arithmetic: bn128_ref.py) ----
_memo = {}


def classify(pt):
    """64 (G1) or 128 (G2) bytes of a key point -> None (good), "infinity", or the smallest applicable reason."""
    pt = bytes(pt)
    if pt in _memo:
        return _memo[pt]
    w = [int.from_bytes(pt[i:i + 32], "little") for i in range(0, len(pt), 32)]
    nx = len(w) // 2
    if all(v == 0 for v in w[:nx]):
        res = INFINITY                     # the rest of its bytes is not examined
    elif any(v >= Q for v in w):
        res = UNREDUCED
    else:
        v = [x * RINV % Q for x in w]
        if nx == 1:
            res = None if g1_on_curve(v[0], v[1]) else OFF_CURVE
        else:
            x, y = (v[0], v[1]), (v[2], v[3])
            if not g2_on_twist(x, y):
                res = OFF_CURVE
            else:
                res = None if g2_times_r_is_infinity((x, y)) else OUTSIDE
    _memo[pt] = res
    return res


def expected_section(data, size, indices=None):
    """(infinity count, bad count, first bad index, its reason) of a section by the classifier, over all points or `indices`."""
    n = len(data) // size
    inf = bad = 0
    first = reason = None
    for i in (range(n) if indices is None else sorted(indices)):
        c = classify(data[size * i:size * i + size])
        if c == INFINITY:
            inf += 1
        elif c is not None:
            bad += 1
            if first is None:
                first, reason = i, c
    return inf, bad, first, reason


def assert_sections_match(rep, sec, names=SECTIONS):
    """Every section of the report against the classifier's answer over ALL its points."""
    for name in names:
        inf, bad, first, reason = expected_section(sec[SEC_KEY[name]], SEC_SIZE[name])
        got = rep[name]
        assert got["points"] == len(sec[SEC_KEY[name]]) // SEC_SIZE[name], name
        assert (got["infinity"], got["bad"], got["first_bad"], got["first_reason"]) == (inf, bad, first, reason), (name, got, (inf, bad, first, reason))


# ---- keys ----
def synth_sections(bn, log_domain, n_public=2, seed=1):
    from wasmsnark_amd import synth
    circ = synth.make_circuit(log_domain, n_public=n_public, seed=seed)
    S = synth.setup(circ, seed=seed + 50)
    sec, _ = synth.build_sections(circ, S, bn.mul_base)
    return circ, S, sec


def mutable(sec):
    """A private copy of a sections dict whose point sections and fixed points can be written in place."""
    out = dict(sec)
    for k in list(SEC_KEY.values()) + list(FIXED):
        out[k] = bytearray(sec[k])
    return out


def no_ms(rep):
    return {k: v for k, v in rep.items() if k != "ms"}


def rogue_g2_bytes():
    x, y = twist_point_outside_g2()
    return mont(x[0]) + mont(x[1]) + mont(y[0]) + mont(y[1])


def plant(sec, name, index, what):
    """Spoil point `index` of section `name` in place: what in unreduced, off_curve, outside_subgroup, both (unreduced AND off
    the curve: must be reported as unreduced)."""
    size, buf = SEC_SIZE[name], sec[SEC_KEY[name]]
    o = size * index
    ny = size // 2           # offset of y inside the point
    assert classify(buf[o:o + size]) is None, "plant on a finite valid point"
    if what == UNREDUCED:        # x + q: the same residue, but not a field element's canonical word string
        buf[o:o + 32] = le(int.from_bytes(buf[o:o + 32], "little") + Q)
    elif what == OFF_CURVE:      # the low bit of y
        buf[o + ny] ^= 1
    elif what == "both":
        buf[o + ny] ^= 1
        buf[o + size - 32:o + size] = le(Q + 12345)      # the last word of y
    elif what == OUTSIDE:
        assert name == "B2"
        buf[o:o + 128] = rogue_g2_bytes()
    else:
        raise ValueError(what)


def finite_indices(sec, name):
    size, buf = SEC_SIZE[name], sec[SEC_KEY[name]]
    nx = size // 2
    return [i for i in range(len(buf) // size) if any(buf[size * i:size * i + nx])]


# ---- 1. valid keys, three entry points, two file formats ----
def check_valid_key(bn, sec, tmp_path, expect_infinity=None, classify_all=True):
    from wasmsnark_amd import formats, synth
    rep = bn.check_key(sections=sec)
    assert rep["ok"] is True and rep["relations_run"] == 7 and rep["relations_bad"] == 0
    assert all(v is None for v in rep["fixed"].values()) and all(v is True for v in rep["relations"].values())
    nv, npub, dom = sec["n_vars"], sec["n_public"], sec["domain"]
    assert [rep[s]["points"] for s in SECTIONS] == [nv, nv, nv, nv - npub - 1, dom]
    for name in SECTIONS:
        size, buf = SEC_SIZE[name], sec[SEC_KEY[name]]
        zeros = len(buf) // size - len(finite_indices(sec, name))       # x == 0
        assert rep[name]["infinity"] == zeros and rep[name]["bad"] == 0 and rep[name]["first_bad"] is None, (name, rep[name], zeros)
    if classify_all:
        assert_sections_match(rep, sec)
    if expect_infinity is not None:
        assert expect_infinity(rep)
    want = no_ms(rep)
    assert set(rep["ms"]) == {"points", "relation_sums", "pairings", "total"} and rep["ms"]["total"] >= rep["ms"]["pairings"] > 0
    pkey = synth.sections_to_pkey(sec)
    assert no_ms(bn.check_key(pkey=pkey)) == want
    p_bin, p_box = os.path.join(str(tmp_path), "k.bin"), os.path.join(str(tmp_path), "k.wsnark64")
    with open(p_bin, "wb") as f:
        f.write(pkey)
    formats.write_key_container(sec, p_box)
    assert no_ms(bn.check_key(path=p_bin)) == want
    assert no_ms(bn.check_key(path=p_box)) == want
    return rep


# ---- 2. planted bad points ----
def check_planted(bn, sec, plants, relations=True):
    """plants: [(section, index, what)].  The report must equal the classifier's answer for EVERY section, ok must be 0, and the
    relations whose points are involved must not have been run."""
    bad = mutable(sec)
    for name, index, what in plants:
        plant(bad, name, index, what)
    rep = bn.check_key(sections=bad, relations=relations)
    assert_sections_match(rep, bad)
    hit = {name for name, _, _ in plants}
    for name in SECTIONS:
        assert (rep[name]["bad"] > 0) == (name in hit), (name, rep[name])
    assert rep["ok"] is False
    if relations:
        b_hit = bool(hit & {"B1", "B2"})
        assert rep["relations"]["B1~B2"] is (None if b_hit else True)
        assert rep["relations"]["beta1~beta2"] is True and rep["relations"]["delta1~delta2"] is True
    else:
        assert rep["relations_run"] == 0
    return rep, bad


def boundary_plants(sec, chunk):
    """One plant per position class: index 0, the last index, both sides of the first chunk boundary -- finite points only."""
    out = []
    whats = {"A": UNREDUCED, "B1": OFF_CURVE, "B2": OUTSIDE, "C": OFF_CURVE, "H": UNREDUCED}
    for name in SECTIONS:
        fin = finite_indices(sec, name)
        n = len(sec[SEC_KEY[name]]) // SEC_SIZE[name]
        assert n > chunk, "the key must span several chunks"
        below = max(i for i in fin if i < chunk)
        above = min(i for i in fin if i >= chunk)
        out.append((name, [(name, fin[0], whats[name])]))
        out.append((name, [(name, fin[-1], whats[name])]))
        out.append((name, [(name, below, whats[name])]))
        out.append((name, [(name, above, whats[name])]))
    return out


def check_smallest_reason(bn, sec):
    """One point that is both unreduced and off the curve, in G1 and in G2: reported as unreduced."""
    for name in ("A", "B2"):
        i = finite_indices(sec, name)[3]
        rep, bad = check_planted(bn, sec, [(name, i, "both")], relations=False)
        assert (rep[name]["bad"], rep[name]["first_bad"], rep[name]["first_reason"]) == (1, i, UNREDUCED)
        # and the classifier agrees that the curve equation fails too once the coordinate is reduced
        size = SEC_SIZE[name]
        pt = bytearray(bad[SEC_KEY[name]][size * i:size * i + size])
        pt[size - 32:size] = le(int.from_bytes(pt[size - 32:size], "little") - Q)
        assert classify(pt) == OFF_CURVE


def check_subgroup_tests_agree(bn, sec, tune, indices):
    """The shipped verdict ([r] Q == O) and the psi test (PKCHECK_SUBGROUP=1) on a B2 section with planted points of every kind:
    the same report, and both equal to the classifier's."""
    bad = mutable(sec)
    for i, what in zip(indices, (OUTSIDE, OFF_CURVE, UNREDUCED, OUTSIDE)):
        plant(bad, "B2", i, what)
    r0 = bn.check_key(sections=bad, relations=False)
    tune(bn.lib, "PKCHECK_SUBGROUP", 1)
    r1 = bn.check_key(sections=bad, relations=False)
    tune(bn.lib, "PKCHECK_SUBGROUP", 0)
    assert no_ms(r0) == no_ms(r1)
    assert_sections_match(r0, bad, names=("B2",))
    assert r0["B2"]["bad"] == 4


# ---- 4. fixed points ----
def check_fixed_points(bn, sec, relations_every=True):
    """relations_every=False (the emulator, where the sums are slow): the relations run beside the infinity case of every point only,
    the other cases are audited points-only."""
    for k, name in enumerate(FIXED):
        g2 = name.endswith("2")
        size = 128 if g2 else 64
        cases = [(UNREDUCED, lambda b: b.__setitem__(slice(32, 64), le(int.from_bytes(b[32:64], "little") + Q))),
                 (OFF_CURVE, lambda b: b.__setitem__(size // 2, b[size // 2] ^ 1)),
                 (INFINITY, lambda b: b.__setitem__(slice(0, size // 2), bytes(size // 2)))]
        if g2:
            cases.append((OUTSIDE, lambda b: b.__setitem__(slice(0, 128), rogue_g2_bytes())))
        for why, spoil in cases:
            bad = mutable(sec)
            spoil(bad[name])
            with_rel = relations_every or why == INFINITY
            rep = bn.check_key(sections=bad, relations=with_rel)
            assert rep["fixed"] == {n: (why if n == name else None) for n in FIXED}, (name, why, rep["fixed"])
            assert rep["ok"] is False
            assert all(rep[s]["bad"] == 0 for s in SECTIONS)
            if not with_rel:
                assert rep["relations_run"] == 0
                continue
            # the relation this point belongs to was not run; the others were, and hold
            rel = {"beta1": "beta1~beta2", "beta2": "beta1~beta2", "delta1": "delta1~delta2", "delta2": "delta1~delta2"}.get(name)
            for r, v in rep["relations"].items():
                assert v is (None if r == rel else True), (name, why, rep["relations"])


# ---- 5. relations ----
def check_pseudo_key(bn, n_vars=70, n_public=2, domain=64):
    """Every point a multiple of a generator, nothing related: no bad point, all three relations run and all three violated."""
    from wasmsnark_amd import synth
    pkey = synth.pseudo_key(n_vars, n_public, domain, seed=5, mul_base=bn.mul_base)
    rep = bn.check_key(pkey=pkey)
    assert all(rep[s]["bad"] == 0 for s in SECTIONS) and all(v is None for v in rep["fixed"].values())
    assert rep["relations_run"] == 7 and rep["relations_bad"] == 7 and rep["ok"] is False
    assert rep["B1"]["infinity"] == rep["B2"]["infinity"] == len(range(0, n_vars, 97))


def check_relations(bn, sec):
    """What bit 2 sees and what it cannot see.  Swapping B2_j and B2_k breaks the pairing of logs and is found; swapping BOTH
    (B1_j, B1_k) and (B2_j, B2_k) keeps every pair intact -- a permutation of the signals, which no check of B1 against B2 can
    see: the audit says ok."""
    fin1 = set(finite_indices(sec, "B1"))
    fin = [i for i in finite_indices(sec, "B2") if i in fin1]
    j, k = fin[1], fin[-2]
    b2 = sec["pointsB2"]
    assert b2[128 * j:128 * j + 128] != b2[128 * k:128 * k + 128]

    def swap(buf, size):
        buf[size * j:size * j + size], buf[size * k:size * k + size] = bytes(buf[size * k:size * k + size]), bytes(buf[size * j:size * j + size])

    only_b2 = ("B1~B2",)
    bad = mutable(sec)
    swap(bad["pointsB2"], 128)
    rep = bn.check_key(sections=bad)
    assert rep["relations_run"] == 7 and rep["relations_bad"] == 4 and rep["ok"] is False
    assert all(rep[s]["bad"] == 0 for s in SECTIONS) and [r for r, v in rep["relations"].items() if v is False] == list(only_b2)
    swap(bad["pointsB1"], 64)
    rep = bn.check_key(sections=bad)
    assert rep["ok"] is True and rep["relations_bad"] == 0
    # B2_j = infinity where B1_j is finite
    bad = mutable(sec)
    bad["pointsB2"][128 * j:128 * j + 128] = bytes(128)
    rep = bn.check_key(sections=bad)
    assert rep["relations_run"] == 7 and rep["relations_bad"] == 4 and rep["B2"]["infinity"] == bn.check_key(sections=sec, relations=False)["B2"]["infinity"] + 1
    # delta2 := beta2
    bad = mutable(sec)
    bad["delta2"][:] = bad["beta2"]
    rep = bn.check_key(sections=bad)
    assert rep["relations_run"] == 7 and rep["relations_bad"] == 2 and rep["ok"] is False
    # the verdicts do not depend on the seed
    bad = mutable(sec)
    swap(bad["pointsB2"], 128)
    for seed in (bytes(range(32)), bytes([7]) * 32, None):
        assert bn.check_key(sections=bad, seed=seed)["relations_bad"] == 4
        assert bn.check_key(sections=sec, seed=seed)["ok"] is True
    # points only: no relation runs, and a valid key is ok
    rep = bn.check_key(sections=sec, relations=False)
    assert rep["ok"] is True and rep["relations_run"] == 0 and all(v is None for v in rep["relations"].values())
    # relations only: no point is looked at (counts stay 0), the relations run
    rep = bn.check_key(sections=sec, points=False)
    assert rep["ok"] is True and rep["relations_run"] == 7 and all(rep[s]["infinity"] == 0 and rep[s]["bad"] == 0 for s in SECTIONS)


# ---- 6. errors and no side effects ----
def _raw_report(bn):
    from wasmsnark_amd.bn128 import _KeyReport
    rep = _KeyReport()
    C.memset(C.byref(rep), 0x5A, C.sizeof(rep))
    return rep


def check_errors(bn, sec, so_path):
    from wasmsnark_amd import synth
    from wasmsnark_amd._lib import WsnarkError
    lib = bn.lib
    pkey = synth.sections_to_pkey(sec)
    untouched = bytes(_raw_report(bn))
    for cut in (100, 487, len(pkey) - 1, len(pkey) // 2):
        rep = _raw_report(bn)
        rc = lib.c.wsnark_pkey_check(pkey[:cut], cut, 0, None, C.byref(rep))
        h = C.c_void_p()
        assert rc == lib.c.wsnark_pkey_load(pkey[:cut], cut, C.byref(h)) == ERR_FORMAT, (cut, rc)
        assert bytes(rep) == untouched
    # a short section through the sections entry point: the loader's code
    short = dict(sec, pointsH=bytes(sec["pointsH"])[:-64])
    try:
        bn.check_key(sections=short)
        raise AssertionError("a short section passed")
    except WsnarkError as e:
        assert e.code == ERR_FORMAT
    try:
        bn.load_key(sections=short)
        raise AssertionError("a short section loaded")
    except WsnarkError as e:
        assert e.code == ERR_FORMAT
    # a file that cannot be opened, unknown flag bits
    rep = _raw_report(bn)
    h = C.c_void_p()
    assert lib.c.wsnark_pkey_check_file(b"/nonexistent/key.bin", 0, None, C.byref(rep)) == lib.c.wsnark_pkey_load_file(b"/nonexistent/key.bin", 0, 1, 0, C.byref(h)) == ERR_ARG
    assert lib.c.wsnark_pkey_check(pkey, len(pkey), 8, None, C.byref(rep)) == ERR_ARG
    assert bytes(rep) == untouched
    # before wsnark_init: a fresh process that loads the library and never initialises it
    code = ("import ctypes as C, sys\n"
            "c = C.CDLL(sys.argv[1])\n"
            "rep = (C.c_uint8 * 256)(*([90] * 256))\n"
            "c.wsnark_pkey_check.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p]\n"
            "c.wsnark_pkey_check_file.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p]\n"
            "print(c.wsnark_pkey_check(bytes(600), 600, 0, None, rep), c.wsnark_pkey_check_file(b'x', 0, None, rep), set(rep))\n")
    out = subprocess.run([sys.executable, "-c", code, so_path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == [str(ERR_NOINIT), str(ERR_NOINIT), "{90}"], (out.stdout, out.stderr)


def check_no_side_effects(bn, log_domain=5):
    """The same proof from the same key handle before and after an audit of the same bytes."""
    from wasmsnark_amd import synth
    circ, S, sec = synth_sections(bn, log_domain, seed=9)
    pkey = synth.sections_to_pkey(sec)
    key = bn.load_key(pkey)
    wit = synth.witness_bin(circ)
    r, s = bytes([3]) * 32, bytes([5]) * 32
    before = bn.groth16GenProof(wit, key, r=r, s=s)
    assert bn.check_key(pkey=pkey)["ok"] is True
    assert bn.groth16GenProof(wit, key, r=r, s=s) == before == synth.expected_proof(circ, S, r, s, bn.mul_base)
    key.free()


# ---- 7. the opt-in load ----
def check_load_key_option(bn, log_domain=5):
    import pytest
    from wasmsnark_amd import synth
    from wasmsnark_amd._lib import WsnarkError
    circ, S, sec = synth_sections(bn, log_domain, seed=12)
    bad = mutable(sec)
    i = finite_indices(bad, "B2")[2]
    plant(bad, "B2", i, OUTSIDE)
    good_pkey, bad_pkey = synth.sections_to_pkey(sec), synth.sections_to_pkey(bad)
    with pytest.raises(WsnarkError) as e:
        bn.load_key(bad_pkey, check=True)
    assert "section B2" in str(e.value) and "index %d" % i in str(e.value) and OUTSIDE in str(e.value)
    with pytest.raises(WsnarkError):
        bn.load_key(sections=bad, check=True)
    key = bn.load_key(good_pkey, check=True)
    wit, r, s = synth.witness_bin(circ), bytes([1]) * 32, bytes([2]) * 32
    assert bn.groth16GenProof(wit, key, r=r, s=s) == synth.expected_proof(circ, S, r, s, bn.mul_base)
    key.free()
    # unchanged behaviour: without the option the tampered key loads, and proves (a proof no verifier accepts)
    key = bn.load_key(bad_pkey)
    assert bn.groth16GenProof(wit, key, r=r, s=s)["pi_a"] == synth.expected_proof(circ, S, r, s, bn.mul_base)["pi_a"]
    key.free()
