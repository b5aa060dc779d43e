"""Shared checks of the key-against-circuit check (wsnark_circuit_row_sums, wsnark_pkey_circuit_check*, csrc/pkeycircuit.hip), run by
tests/test_emul_pkey_circuit.py on the thread-emulator build of the kernel sources and by tests/test_gpu_pkey_circuit.py on the device.

The yardstick is never the code under test.  The row sums are compared, every element of all six vectors, with the sums in Python
integers over a hand-built circuit.  Good keys come from three independent makers: the closed form from the toxic waste
(synth.build_sections: every point a fixed-base multiple of a known logarithm), setup_key, and setup_key followed by contribute_key.
Every tamper plants VALID curve points (swaps, doublings through scale_points, points of another setup) and names the whole word
checks_bad it must produce, so nothing depends on the point tests."""
import ctypes as C
import copy
import random
import subprocess
import sys

import pkey_check_common as pk
import pkey_delta_common as pd
import pkey_setup_common as ps
from bn128_ref import R, le
from pkey_check_common import ERR_ARG, ERR_FORMAT, ERR_NOINIT, ERR_SIZE
from wasmsnark_amd import synth

BIT = {"shape_and_streams": 1, "fixed_points": 2, "delta1~delta2": 4, "A": 8, "B1": 16, "B2": 32, "C": 64, "H": 128, "vk_fixed_points": 256,
       "IC": 512}
ALL, ALL_VK = 0xFF, 0x3FF
SEED_A, SEED_B = bytes(range(32)), bytes(range(100, 132))


# ---- 1. the row sums against Python integers ----
def hand_circuit(log_domain, n_vars=40, seed=5):
    """rows[m][i] = [(column, coefficient), ...] for m in A, B, C, in the order the records are written.  Rows 0..4: no term, 1, 2, 3 and 9
    terms; row 5 only columns <= 2, row 6 only columns > 2, row 7 columns on either side of 2 in turn, row 8 with 300 terms; repeated
    (row, column) records and zero coefficients throughout; the rest 0..4 terms."""
    rnd = random.Random(seed)
    domain = 1 << log_domain
    coef = lambda: rnd.choice((0, 1, R - 1, rnd.randrange(R), rnd.randrange(R), rnd.randrange(1, 8)))
    rows = []
    for m in range(3):
        M = [[] for _ in range(domain)]
        for i, k in ((1, 1), (2, 2), (3, 3), (4, 9)):
            M[i] = [(rnd.randrange(n_vars), coef()) for _ in range(k)]
        M[5] = [(rnd.randrange(0, 3), coef()) for _ in range(5)]
        M[6] = [(rnd.randrange(3, n_vars), coef()) for _ in range(6)]
        M[7] = [((rnd.randrange(0, 3) if t % 2 == 0 else rnd.randrange(3, n_vars)), rnd.randrange(1, R)) for t in range(8)]
        M[8] = [(rnd.randrange(n_vars), coef()) for _ in range(300)]
        M[8][17] = M[8][16]                      # a repeated record
        M[8][40] = (M[8][41][0], 0)              # a zero coefficient beside a real one of the same column
        for i in range(9, domain):
            M[i] = [(rnd.randrange(n_vars), coef()) for _ in range(rnd.randrange(0, 5))]
        if m == 2:
            M[domain - 1] = []                   # the last row empty in one matrix
        rows.append(M)
    return rows


def rows_to_blob(M, n_vars):
    cols = [[] for _ in range(n_vars)]
    for i, row in enumerate(M):
        for j, c in row:
            cols[j].append((i, c))
    return ps._records_blob(cols)


def weights_for(n_vars, seed=9):
    rnd = random.Random(seed)
    w = [rnd.randrange(1 << 128) for _ in range(n_vars)]
    # the special values on both sides of nPublic = 2, and at the last signal
    w[0], w[1], w[2], w[3], w[4], w[5], w[n_vars - 1] = 1, R - 1, (1 << 256) - 1, 0, (1 << 256) - 1, R - 1, 1
    return w


def expected_row_sums(rows, w, n_public, domain):
    mont = lambda v: le(v % R * synth.MONT % R)
    pub, prv = b"", b""
    for M in rows:
        for i in range(domain):
            pub += mont(sum(c * w[j] for j, c in M[i] if j <= n_public))
            prv += mont(sum(c * w[j] for j, c in M[i] if j > n_public))
    return pub, prv


def check_row_sums(bn, log_domain, n_vars=40):
    domain = 1 << log_domain
    rows = hand_circuit(log_domain, n_vars)
    assert [len(rows[0][i]) for i in (0, 1, 2, 3, 4, 8)] == [0, 1, 2, 3, 9, 300]
    blobs = [rows_to_blob(M, n_vars) for M in rows]
    w = weights_for(n_vars)
    wb = b"".join(le(v) for v in w)
    for n_public in (0, 2, n_vars - 1):
        circuit = {"n_vars": n_vars, "n_public": n_public, "domain": domain, "polsA": blobs[0], "polsB": blobs[1], "polsC": blobs[2]}
        pub, prv = bn.circuit_row_sums(circuit, wb)
        want_pub, want_prv = expected_row_sums(rows, w, n_public, domain)
        for name, got, want in (("public", pub, want_pub), ("private", prv, want_prv)):
            diff = [(k // domain, k % domain) for k in range(3 * domain) if got[32 * k:32 * k + 32] != want[32 * k:32 * k + 32]]
            assert got == want and len(got) == 96 * domain, (n_public, name, diff[:8])
        if n_public == n_vars - 1:
            assert prv == bytes(96 * domain)
        if n_public == 2:      # row 5 is all public, row 6 all private, row 7 has both halves
            z = bytes(32)
            assert prv[32 * 5:32 * 6] == z and pub[32 * 6:32 * 7] == z and pub[32 * 7:32 * 8] != z and prv[32 * 7:32 * 8] != z


def check_row_sums_errors(bn):
    from wasmsnark_amd.bn128 import _circuit_struct
    circ = synth.make_circuit(4, n_public=2, seed=3)
    blobs = synth.circuit_blobs(circ)
    n, nv = circ.domain, circ.n_vars
    w = bytes(32 * nv)
    out = [(C.c_uint8 * (96 * n))(*([0x5A] * (96 * n))) for _ in range(2)]

    def call(k, weights=w, o0=out[0], o1=out[1]):
        cs, keep = _circuit_struct(k)
        rc = bn.lib.c.wsnark_circuit_row_sums(C.byref(cs), weights, o0, o1)
        assert set(out[0]) == set(out[1]) == {0x5A}
        return rc

    assert call(blobs, weights=None) == ERR_ARG and call(blobs, o0=None) == ERR_ARG and call(blobs, o1=None) == ERR_ARG
    assert bn.lib.c.wsnark_circuit_row_sums(None, w, out[0], out[1]) == ERR_ARG
    assert call(dict(blobs, domain=48)) == ERR_SIZE and call(dict(blobs, domain=1 << 25)) == ERR_SIZE
    assert call(dict(blobs, n_public=nv)) == ERR_FORMAT
    assert call(dict(blobs, polsC=blobs["polsC"][:-1])) == ERR_FORMAT
    cols = [list(col.items()) for col in circ.B]
    cols[nv - 1] = cols[nv - 1] + [(n, 5)]
    assert call(dict(blobs, polsB=ps._records_blob(cols))) == ERR_FORMAT


# ---- 2. good keys ----
_good_memo = {}


def good_keys(bn, log_domain, style):
    """{"toxic": (sections, vk, gamma2's bytes), "setup": ..., "contributed": ...} for the circuit of pkey_setup_common.setup_inputs, made once"""
    key = (id(bn), log_domain, style)
    if key not in _good_memo:
        circ, S, powers, blobs, _ = ps.setup_inputs(bn, log_domain, style)
        assert S.delta != 1 and S.gamma != 1
        sec, (ic, gamma2) = synth.build_sections(circ, S, bn.mul_base)
        out = {"toxic": (sec, synth.vk_from_points(circ.n_public, sec, ic, gamma2), gamma2)}
        new, (ic1, gamma1), rep = bn.setup_key(powers, blobs)
        assert rep["ok"] is True
        vk1 = synth.vk_from_points(circ.n_public, new, ic1, gamma1)
        out["setup"] = (new, vk1, gamma1)
        that, rep = bn.contribute_key(sections=new, d=pd.D_FIXED)
        assert rep["ok"] is True
        out["contributed"] = (that, synth.vk_with_delta2(vk1, that), gamma1)
        _good_memo[key] = out
    return _good_memo[key]


def assert_good(v, with_vk=True):
    want = ALL_VK if with_vk else ALL
    assert v["ok"] is True and v["checks_run"] == want and v["checks_bad"] == 0, v
    assert all(v["checks"][name] is (True if BIT[name] & want else None) for name in BIT), v
    assert set(v["ms"]) == {"matrices", "key_sums", "powers_sums", "pairings", "total"} and v["ms"]["total"] >= v["ms"]["matrices"] > 0


def check_good_key(bn, tmp_path, tune, log_domain, style, which, forms=("sections",), chunks=(None,), seeds=(SEED_A,), no_vk=False):
    """The verdict of a good key: all requested bits run, none bad, whatever the form, the chunk and the seed."""
    circ, S, powers, blobs, _ = ps.setup_inputs(bn, log_domain, style)
    sec, vk, _ = good_keys(bn, log_domain, style)[which]
    if style == "rows":
        assert len(pk.finite_indices(sec, "A")) < circ.n_vars and len(pk.finite_indices(sec, "B2")) < circ.n_vars      # infinity points
    pkey = synth.sections_to_pkey(sec)
    for chunk in chunks:
        if chunk is None:
            bn.lib.tune("PKCIRCUIT_CHUNK", None)
        else:
            tune(bn.lib, "PKCIRCUIT_CHUNK", chunk)
            assert circ.domain > chunk or circ.domain <= 64
        for seed in seeds:
            for form in forms:
                if form == "sections":
                    v = bn.check_key_circuit(powers, blobs, sections=sec, vk=vk, seed=seed)
                elif form == "pkey":
                    v = bn.check_key_circuit(powers, blobs, pkey=pkey, vk=vk, seed=seed)
                else:
                    path = str(tmp_path / ("key_%s.bin" % which))
                    with open(path, "wb") as f:
                        f.write(pkey)
                    v = bn.check_key_circuit(powers, blobs, path=path, vk=vk, seed=seed)
                assert_good(v)
    if no_vk:
        assert_good(bn.check_key_circuit(powers, blobs, sections=sec, vk=None, seed=None), with_vk=False)      # and a seed from the OS


def check_empty_c_section(bn):
    """nVars == nPublic + 1: no private signal, the C section is empty and bit 6 compares two points at infinity"""
    rnd = random.Random(12)
    n, nv = 4, 3
    A = [{0: 3, 1: 5}, {1: 7, 2: 1}, {3: 2}]
    B = [{0: 1}, {2: 9}, {1: 4, 3: 6}]
    Cm = [{0: 11}, {1: 1}, {2: 13, 3: 1}]
    circ = synth.Circuit(nv, nv - 1, n, A, B, Cm, [1, 2, 3])
    S = synth.setup(circ, seed=rnd.randrange(1 << 30))
    sec, (ic, gamma2) = synth.build_sections(circ, S, bn.mul_base)
    assert len(sec["pointsC"]) == 0 and len(ic) == nv
    powers = synth.powers_from_toxic(S, n, bn.mul_base)
    vk = synth.vk_from_points(circ.n_public, sec, ic, gamma2)
    assert_good(bn.check_key_circuit(powers, synth.circuit_blobs(circ), sections=sec, vk=vk, seed=SEED_A))
    swapped = dict(vk, IC=[vk["IC"][1], vk["IC"][0]] + vk["IC"][2:])
    assert bn.check_key_circuit(powers, synth.circuit_blobs(circ), sections=sec, vk=swapped, seed=SEED_A)["checks_bad"] == BIT["IC"]


# ---- 3. tampers ----
def _swap(buf, size, i, j):
    a, b = bytes(buf[size * i:size * i + size]), bytes(buf[size * j:size * j + size])
    assert a != b and any(a[:size // 2]) and any(b[:size // 2])
    buf[size * i:size * i + size], buf[size * j:size * j + size] = b, a


def _doubled(bn, g, buf, size, i):
    p = bytes(buf[size * i:size * i + size])
    assert any(p[:size // 2])
    buf[size * i:size * i + size] = bn.scale_points(g, p, 2)


def _bump_coefficient(circ, name, column):
    """the circuit's record stream `name` with one coefficient of `column` changed"""
    cols = [dict(c) for c in getattr(circ, name[-1])]
    if cols[column]:
        row = sorted(cols[column])[0]
        cols[column][row] = (cols[column][row] + 1) % R
    else:
        cols[column][0] = 1
    return synth._pol_blob(cols)


def tamper_cases(bn, log_domain, style, chunk, only=None):
    """[(name, kwargs of check_key_circuit, expected checks_run, expected checks_bad)] on the contributed key (C and hExps under an unknown
    delta).  Every tampered index sits in the LAST chunk of its section at the given chunk size."""
    circ, S, powers, blobs, _ = ps.setup_inputs(bn, log_domain, style)
    sec, vk, gamma2 = good_keys(bn, log_domain, style)["contributed"]
    other_sec, other_vk, _ = good_keys(bn, log_domain, style)["toxic"]      # another delta and gamma on the same circuit and transcript
    nv, npub, n = circ.n_vars, circ.n_public, circ.domain
    nC = nv - npub - 1
    cases = []

    def add(name, run, bad, sections=None, vk_=vk, powers_=powers, blobs_=blobs):
        if only is None or name in only:
            cases.append((name, {"powers": powers_, "circuit": blobs_, "sections": sections if sections is not None else sec, "vk": vk_}, run, bad))

    def finite_pair(s, name):
        idx = pk.finite_indices(s, name)
        i, j = idx[-1], idx[-2]
        size = pk.SEC_SIZE[name]
        assert s[pk.SEC_KEY[name]][size * i:size * i + size] != s[pk.SEC_KEY[name]][size * j:size * j + size]
        assert i // chunk == (len(s[pk.SEC_KEY[name]]) // size - 1) // chunk or len(idx) < nv, "the tampered index sits in the last chunk"
        return i, j

    m = pk.mutable(sec)
    _swap(m["pointsA"], 64, *finite_pair(sec, "A"))
    add("swap_A", ALL_VK, BIT["A"], m)
    m = pk.mutable(sec)
    both = sorted(set(pk.finite_indices(sec, "B1")) & set(pk.finite_indices(sec, "B2")))
    i, j = both[-1], both[-2]
    _swap(m["pointsB1"], 64, i, j)
    _swap(m["pointsB2"], 128, i, j)
    add("swap_B1_and_B2", ALL_VK, BIT["B1"] | BIT["B2"], m)
    m = pk.mutable(sec)
    _swap(m["pointsB2"], 128, i, j)
    add("swap_B2", ALL_VK, BIT["B2"], m)
    m = pk.mutable(sec)
    _doubled(bn, 1, m["pointsC"], 64, nC - 1)
    add("double_C", ALL_VK, BIT["C"], m)
    m = pk.mutable(sec)
    _doubled(bn, 1, m["pointsH"], 64, n - 1)
    add("double_H", ALL_VK, BIT["H"], m)
    add("swap_IC", ALL_VK, BIT["IC"], vk_=dict(vk, IC=[vk["IC"][1], vk["IC"][0]] + vk["IC"][2:]))
    twice = bn.scale_points(2, gamma2, 2)
    add("double_gamma2", ALL_VK, BIT["IC"], vk_=dict(vk, vk_gamma_2=synth.vk_from_points(npub, sec, [], twice)["vk_gamma_2"]))
    add("vk_delta2_of_another_key", ALL_VK, BIT["vk_fixed_points"], vk_=dict(vk, vk_delta_2=other_vk["vk_delta_2"]))
    m = pk.mutable(sec)
    _doubled(bn, 1, m["delta1"], 64, 0)
    add("double_delta1", ALL_VK & ~(BIT["C"] | BIT["H"]), BIT["delta1~delta2"], m)
    private_col, public_col = nv - 2, 1
    add("polsC_private_column", ALL_VK, BIT["C"], blobs_=dict(blobs, polsC=_bump_coefficient(circ, "polsC", private_col)))
    add("polsC_public_column", ALL_VK, BIT["IC"], blobs_=dict(blobs, polsC=_bump_coefficient(circ, "polsC", public_col)))
    col = max(j for j in range(npub + 1, nv) if circ.A[j])
    bumped = _bump_coefficient(circ, "polsA", col)
    add("polsA_in_the_key_only", ALL_VK, BIT["shape_and_streams"], dict(sec, polsA=bumped))
    add("polsA_in_key_and_circuit", ALL_VK, BIT["A"] | BIT["C"], dict(sec, polsA=bumped), blobs_=dict(blobs, polsA=bumped))
    add("n_public_off_by_one", 1, 1, blobs_=dict(blobs, n_public=npub + 1))
    S2 = copy.copy(S)
    S2.tau = S.tau * 3 % R
    add("another_tau", ALL_VK, BIT["A"] | BIT["B1"] | BIT["B2"] | BIT["C"] | BIT["H"] | BIT["IC"], powers_=synth.powers_from_toxic(S2, n, bn.mul_base))
    S3 = copy.copy(S)
    S3.alpha = S.alpha * 3 % R
    add("another_alpha", ALL_VK, BIT["fixed_points"] | BIT["C"] | BIT["IC"],
        powers_=dict(powers, alpha_tau_g1=synth.powers_from_toxic(S3, n, bn.mul_base)["alpha_tau_g1"]))
    return cases


def check_tampers(bn, tune, log_domain, style, chunk=64, only=None, seed=SEED_B):
    tune(bn.lib, "PKCIRCUIT_CHUNK", chunk)
    cases = tamper_cases(bn, log_domain, style, chunk, only)
    assert cases and (only is None or len(cases) == len(only))
    for name, kw, run, bad in cases:
        v = bn.check_key_circuit(kw["powers"], kw["circuit"], sections=kw["sections"], vk=kw["vk"], seed=seed)
        assert (v["checks_run"], v["checks_bad"], v["ok"]) == (run, bad, False), (name, v)


TAMPERS = ("swap_A", "swap_B1_and_B2", "swap_B2", "double_C", "double_H", "swap_IC", "double_gamma2", "vk_delta2_of_another_key",
           "double_delta1", "polsC_private_column", "polsC_public_column", "polsA_in_the_key_only", "polsA_in_key_and_circuit",
           "n_public_off_by_one", "another_tau", "another_alpha")


# ---- 4. errors ----
def check_errors(bn, log_domain, so_path):
    """What the loaders and the setup reject fails with their code and leaves a pre-filled verdict untouched."""
    from wasmsnark_amd.bn128 import _CircuitVerdict, _circuit_struct, _key_sections, _powers_struct, vk_to_bytes
    circ, S, powers, blobs, _ = ps.setup_inputs(bn, log_domain, "columns")
    sec, vk, _ = good_keys(bn, log_domain, "columns")["toxic"]
    c = bn.lib.c
    nv, npub, n = circ.n_vars, circ.n_public, circ.domain
    untouched = bytes(pd._raw(_CircuitVerdict))
    pkey = synth.sections_to_pkey(sec)
    vkb = vk_to_bytes(vk, npub)

    def call(p=powers, k=blobs, s=sec, vk_=vkb, n_inputs=npub, null=None):
        ps_, keep_p = _powers_struct(p)
        cs, keep_c = _circuit_struct(k)
        ks, keep_k = _key_sections(s)
        v = pd._raw(_CircuitVerdict)
        args = [C.byref(ks), C.byref(ps_), C.byref(cs), vk_, len(vk_) if vk_ else 0, n_inputs, SEED_A, C.byref(v)]
        if null is not None:
            args[null] = None
        rc = c.wsnark_pkey_circuit_check_sections(*args)
        assert bytes(v) == untouched
        return rc

    for name in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1"):      # a short array
        assert call(p=dict(powers, **{name: powers[name][:-64]})) == ERR_FORMAT, name
    for name in ("polsA", "polsB", "polsC"):                               # a truncated stream; a record index = domain
        assert call(k=dict(blobs, **{name: blobs[name][:-1]})) == ERR_FORMAT, name
        cols = [list(col.items()) for col in getattr(circ, name[-1])]
        cols[nv - 1] = cols[nv - 1] + [(n, 5)]
        assert call(k=dict(blobs, **{name: ps._records_blob(cols)})) == ERR_FORMAT, name
    assert call(p=dict(powers, domain=48), k=dict(blobs, domain=48)) == ERR_SIZE                # not a power of two
    assert call(p=dict(powers, domain=1 << 25), k=dict(blobs, domain=1 << 25)) == ERR_SIZE      # > 2^24
    assert call(p=dict(powers, domain=2 * n)) == ERR_SIZE                                       # the two domains differ
    assert call(p=dict(powers, tau_g1=bn.mul_base(1, le(2)) + powers["tau_g1"][64:])) == ERR_FORMAT      # not the generator
    assert call(p=dict(powers, tau_g2=bn.mul_base(2, le(2)) + powers["tau_g2"][128:])) == ERR_FORMAT
    assert call(k=dict(blobs, n_public=nv)) == ERR_FORMAT                                       # nPublic + 1 > nVars
    assert call(s=dict(sec, pointsH=sec["pointsH"][:-64])) == ERR_FORMAT                        # a short section of the key
    assert call(vk_=vkb[:-1]) == ERR_SIZE and call(n_inputs=npub + 1) == ERR_SIZE               # fewer than n_inputs + 1 IC points
    for null in (0, 1, 2, 7):
        assert call(null=null) == ERR_ARG, null
    # the bytes and the file forms: a truncated key, a missing file, a NULL verdict
    ps_, keep_p = _powers_struct(powers)
    cs, keep_c = _circuit_struct(blobs)
    v = pd._raw(_CircuitVerdict)
    tail = (C.byref(ps_), C.byref(cs), vkb, len(vkb), npub, SEED_A)
    assert c.wsnark_pkey_circuit_check(pkey, len(pkey) - 1, *tail, C.byref(v)) == ERR_FORMAT
    assert c.wsnark_pkey_circuit_check(pkey, len(pkey), *tail, None) == ERR_ARG
    assert c.wsnark_pkey_circuit_check_file(b"/nonexistent/key.bin", *tail, C.byref(v)) != 0
    assert c.wsnark_pkey_circuit_check_file(None, *tail, C.byref(v)) == ERR_ARG
    assert bytes(v) == untouched
    # before wsnark_init: a fresh process that loads the library and never initialises it
    code = ("import ctypes as C, sys\n"
            "c = C.CDLL(sys.argv[1])\n"
            "vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64\n"
            "c.wsnark_pkey_circuit_check.argtypes = [vp, sz, vp, vp, vp, sz, u64, vp, vp]\n"
            "c.wsnark_pkey_circuit_check_sections.argtypes = [vp, vp, vp, vp, sz, u64, vp, vp]\n"
            "c.wsnark_pkey_circuit_check_file.argtypes = [C.c_char_p, vp, vp, vp, sz, u64, vp, vp]\n"
            "c.wsnark_circuit_row_sums.argtypes = [vp, vp, vp, vp]\n"
            "v = (C.c_uint8 * 64)(*([90] * 64))\n"
            "print(c.wsnark_pkey_circuit_check(None, 0, None, None, None, 0, 0, None, v),\n"
            "      c.wsnark_pkey_circuit_check_sections(None, None, None, None, 0, 0, None, v),\n"
            "      c.wsnark_pkey_circuit_check_file(b'x', None, None, None, 0, 0, None, v),\n"
            "      c.wsnark_circuit_row_sums(None, None, v, v), set(v))\n")
    res = subprocess.run([sys.executable, "-c", code, so_path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == [str(ERR_NOINIT)] * 4 + ["{90}"], (res.stdout, res.stderr)
