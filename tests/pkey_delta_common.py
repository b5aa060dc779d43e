"""Shared checks of the phase-2 delta contribution (wsnark_g{1,2}_scale_batch, wsnark_pkey_contribute*, wsnark_pkey_delta_verify*,
csrc/pkeydelta.hip), run by tests/test_emul_pkey_delta.py on the thread-emulator build of the kernel sources and by
tests/test_gpu_pkey_delta.py on the device.

The yardstick is never the code under test.  scale_batch is compared with affine double-and-add in plain Python integers
(`g1_mul` / `g2_mul` of bn128_ref.py).  A re-keyed key is compared byte for byte with the closed form: the SAME synthetic key built from
toxic waste whose delta is delta * d, every point a fixed-base multiple of a known logarithm through mul_base -- an independent
kernel that the parity tests pin.  Bad input points are counted by the audit's pure-Python classifier (pkey_check_common)."""
import ctypes as C
import os
import subprocess
import sys

import pkey_check_common as pk
from bn128_ref import Q, R, from_mont, g1_mul, g2_mul, le, mont
from pkey_check_common import ERR_ARG, ERR_FORMAT, ERR_NOINIT, ERR_SIZE

D_FIXED = 0x1D2C3B4A5968778695A4B3C2D1E0F00112233445566778899AABBCCDDEEFF01 % R
BIT = {"unchanged": 1, "delta1~delta2": 2, "C": 4, "H": 8, "delta_changed": 16}


# ---- the yardstick: affine double-and-add in Python integers (bn128_ref.g1_mul / g2_mul) ----
def point_from_bytes(g, b):
    """64 / 128 bytes affine Montgomery -> integers; x == 0 (the loaders' rule) -> None"""
    if g == 1:
        return None if not any(b[:32]) else (from_mont(b[:32]), from_mont(b[32:64]))
    return None if not any(b[:64]) else ((from_mont(b[:32]), from_mont(b[32:64])), (from_mont(b[64:96]), from_mont(b[96:128])))


def point_to_bytes(g, p):
    if p is None:
        return bytes(64 if g == 1 else 128)
    if g == 1:
        return mont(p[0]) + mont(p[1])
    return mont(p[0][0]) + mont(p[0][1]) + mont(p[1][0]) + mont(p[1][1])


_mul_memo = {}


def expected_scale(g, points, k):
    """k * P for every point of `points` by the yardstick.  An input at infinity is copied through byte for byte."""
    sz = 64 if g == 1 else 128
    out = bytearray()
    for o in range(0, len(points), sz):
        b = bytes(points[o:o + sz])
        if point_from_bytes(g, b) is None:
            out += b
            continue
        key = (g, b, k % R)
        if key not in _mul_memo:
            _mul_memo[key] = point_to_bytes(g, (g1_mul if g == 1 else g2_mul)(point_from_bytes(g, b), k % R))
        out += _mul_memo[key]
    return bytes(out)


SCALARS = [1, 2, 3, R - 1, R - 2, (R + 1) // 2, 1 << 253, int("55" * 32, 16) % R, int("AA" * 32, 16) % R,
           ((1 << 200) - 1) << 17,              # a run of 200 one-bits: the recoding's carry chain
           R + 12345,                           # >= r: must equal its residue
           0]                                   # every output infinity


def check_scale_batch(bn, g, distinct=12):
    """Every scalar of the list over a few dozen points -- generator multiples, infinity first and last, one point twice --, then
    the lengths around a wavefront and a workgroup with one scalar."""
    sz = 64 if g == 1 else 128
    logs = [1, 2, 3, 5, R - 1, R - 2, (R + 1) // 2, 0xDEADBEEF] + [pow(7, i + 40, R) for i in range(distinct - 8)]
    base = bn.mul_base(g, b"".join(le(v) for v in logs))
    pts = [base[sz * i:sz * i + sz] for i in range(distinct)]
    # infinity with a non-zero y: "copied through byte for byte" is then visible
    inf = bytes(sz // 2) + bytes([9]) + bytes(sz // 2 - 1)
    batch = inf + b"".join(pts) + pts[4] + pts[4] + b"".join(pts[:distinct // 2]) + inf      # distinct + 2 + distinct / 2 + 2 points
    for k in SCALARS:
        got = bn.scale_points(g, batch, k)
        want = expected_scale(g, batch, k)
        assert got == want, (g, hex(k), [i for i in range(len(batch) // sz) if got[sz * i:sz * i + sz] != want[sz * i:sz * i + sz]])
        if k % R == 0:
            assert got[sz:-sz] == bytes(len(batch) - 2 * sz) and got[:sz] == got[-sz:] == inf
    assert bn.scale_points(g, batch, le(R + 12345)) == expected_scale(g, batch, 12345)      # 32 bytes plain LE, reduced
    k = 0x1234567 * R // 0x7654321 | 1
    for n in (1, 63, 64, 65, 257):
        many = b"".join(pts[(5 * i + i // distinct) % distinct] if i % 31 != 30 else inf for i in range(n))
        assert bn.scale_points(g, many, k) == expected_scale(g, many, k), (g, n)
    # the two additions next to the group order: k = r - 1 ends on -P, k = r - 2 passes through it
    one = pts[0]
    neg = bytearray(expected_scale(g, one, 1))
    assert bytes(neg) == one
    p = point_from_bytes(g, one)
    minus = point_to_bytes(g, (p[0], (Q - p[1]) % Q) if g == 1 else (p[0], ((-p[1][0]) % Q, (-p[1][1]) % Q)))
    assert bn.scale_points(g, one, R - 1) == minus


def check_scale_batch_rejects_bad_points(bn):
    from wasmsnark_amd._lib import WsnarkError
    pts = bytearray(bn.mul_base(1, b"".join(le(v) for v in range(1, 70))))
    pts[64 * 66 + 32] ^= 1
    try:
        bn.scale_points(1, pts, 5)
        raise AssertionError("an off-curve point was scaled")
    except WsnarkError as e:
        assert e.code == ERR_FORMAT and "index 66" in str(e)


# ---- keys ----
def rekeyed(circ, S, d):
    """The toxic waste after a contribution by d."""
    import copy
    S2 = copy.copy(S)
    S2.delta = S.delta * d % R
    return S2


def closed_form(bn, circ, S, d):
    from wasmsnark_amd import synth
    return synth.build_sections(circ, rekeyed(circ, S, d), bn.mul_base)


def with_infinity_in_c(circ, S):
    """The same setup with one private signal's key scalars zeroed (as if it occurred in no constraint): its C point is infinity.
    Only for the byte comparison with the closed form -- such a key no longer matches its own polynomials."""
    import copy
    S2 = copy.copy(S)
    S2.a, S2.b, S2.c = list(S.a), list(S.b), list(S.c)
    s = circ.n_public + 1 + 3
    S2.a[s] = S2.b[s] = S2.c[s] = 0
    return S2


def assert_same_key(got, want):
    for k in want:
        assert (got[k] if isinstance(got[k], int) else bytes(got[k])) == (want[k] if isinstance(want[k], int) else bytes(want[k])), k


def no_ms(d):
    return {k: v for k, v in d.items() if k != "ms"}


# ---- 2. the whole re-keyed key against the closed form, three entry points, two file formats, two chunk sizes ----
def check_closed_form(bn, tmp_path, tune, log_domain, chunks=((64, False), (96, True), (None, False)), seed=3, d=D_FIXED):
    """chunks: (PKDELTA_CHUNK or None for the default, whether neither section's length may be a multiple of it).  hExps has a
    power-of-two length, so no run with chunk 64 or the default 2^18 can end both sections inside a chunk: those two sizes run as
    they are, and one more size that is no power of two carries the not-a-multiple assertion."""
    from wasmsnark_amd import formats, synth
    circ = synth.make_circuit(log_domain, n_public=2, seed=seed)
    S = with_infinity_in_c(circ, synth.setup(circ, seed=seed + 50))
    sec, _ = synth.build_sections(circ, S, bn.mul_base)
    want, _ = closed_form(bn, circ, S, d)
    check_closed_form_sections(bn, tmp_path, tune, sec, want, d, chunks)
    return circ, S, sec, want


def check_closed_form_sections(bn, tmp_path, tune, sec, want, d, chunks, with_pkey=True):
    from wasmsnark_amd import formats, synth
    nC, nH = len(sec["pointsC"]) // 64, len(sec["pointsH"]) // 64
    n_inf = nC - len(pk.finite_indices(sec, "C"))
    assert n_inf >= 1, "the C section must hold an infinity entry"
    assert bytes(want["pointsA"]) == bytes(sec["pointsA"]) and bytes(want["pointsC"]) != bytes(sec["pointsC"]) and want["delta2"] != sec["delta2"]
    reports = []
    for ch, ragged in chunks:
        if ch is not None:
            tune(bn.lib, "PKDELTA_CHUNK", ch)
        else:
            bn.lib.tune("PKDELTA_CHUNK", None)
        if ragged:
            assert nC % ch and nH % ch, "neither section may end on a chunk boundary"
            assert nH > ch or nH <= 64, "hExps must span chunks"
        new, rep = bn.contribute_key(sections=sec, d=le(d))
        assert rep["ok"] is True and rep["C"]["bad"] == rep["H"]["bad"] == 0 and rep["C"]["first_bad"] is None
        assert (rep["C"]["points"], rep["H"]["points"]) == (nC, nH)
        assert rep["C"]["infinity"] == n_inf and rep["H"]["infinity"] == 0
        assert set(rep["ms"]) == {"device", "host", "total"} and rep["ms"]["total"] >= rep["ms"]["device"] > 0
        assert_same_key(new, want)
        reports.append(no_ms(rep))
        if with_pkey:
            new_pkey, rep2 = bn.contribute_key(pkey=synth.sections_to_pkey(sec), d=d)
            assert new_pkey == synth.sections_to_pkey(want) and no_ms(rep2) == no_ms(rep)
        for name, write in (("k.bin", lambda s, p: open(p, "wb").write(synth.sections_to_pkey(s))), ("k.wsnark64", formats.write_key_container)):
            if name == "k.bin" and not with_pkey:
                continue
            p_in, p_out, p_want = (os.path.join(str(tmp_path), t + name) for t in ("in_", "out_", "want_"))
            write(sec, p_in)
            write(want, p_want)
            if os.path.exists(p_out):
                os.unlink(p_out)
            got_path, rep3 = bn.contribute_key(path=p_in, out_path=p_out, d=le(d))
            assert got_path == p_out and no_ms(rep3) == no_ms(rep)
            with open(p_out, "rb") as f, open(p_want, "rb") as g:
                assert f.read() == g.read(), name
            assert bn.key_file_info(p_out)["format"] == bn.key_file_info(p_in)["format"]
    assert all(r == reports[0] for r in reports)


# ---- 3. the new key works ----
def check_new_key_works(bn, log_domain=5, seed=9, d=D_FIXED):
    from wasmsnark_amd import synth
    circ, S, sec = pk.synth_sections(bn, log_domain, seed=seed)
    _, (ic, gamma2) = synth.build_sections(circ, S, bn.mul_base)
    vk_old = synth.vk_from_points(circ.n_public, sec, ic, gamma2)
    wit, pub = synth.witness_bin(circ), synth.public_signals(circ)
    r, s = bytes([3]) * 32, bytes([5]) * 32
    old_handle = bn.load_key(sections=sec)
    before = bn.groth16GenProof(wit, old_handle, r=r, s=s)
    new, rep = bn.contribute_key(sections=sec, d=d)
    assert rep["ok"] is True
    assert bn.check_key(sections=new)["ok"] is True
    S2 = rekeyed(circ, S, d)
    proof = bn.groth16GenProof(wit, synth.sections_to_pkey(new), r=r, s=s)
    assert proof == synth.expected_proof(circ, S2, r, s, bn.mul_base)
    vk_new = synth.vk_with_delta2(vk_old, new)
    assert vk_new == synth.vk_with_delta2(vk_old, synth.sections_to_pkey(new)) == synth.vk_with_delta2(vk_old, new["delta2"])
    assert bn.groth16Verify(vk_new, pub, proof) is True
    assert bn.groth16Verify(vk_old, pub, proof) is False
    # no side effects on a resident handle
    assert bn.groth16GenProof(wit, old_handle, r=r, s=s) == before == synth.expected_proof(circ, S, r, s, bn.mul_base)
    assert bn.groth16Verify(vk_old, pub, before) is True
    old_handle.free()


# ---- 4. verify_contribution ----
def _only_bad(v, *names):
    want = sum(BIT[n] for n in names)
    assert v["checks_bad"] == want and v["ok"] is False, (v, names)


def check_verify_contribution(bn, log_domain=5, seed=4, tmp_path=None):
    from wasmsnark_amd import synth
    from wasmsnark_amd._lib import WsnarkError
    circ, S, sec = pk.synth_sections(bn, log_domain, seed=seed)
    d1, d2 = D_FIXED, pow(5, 77, R)
    new, _ = bn.contribute_key(sections=sec, d=d1)
    newest, _ = bn.contribute_key(sections=new, d=d2)
    seeds = (bytes(range(32)), bytes([7]) * 32, None)
    # accepts: one contribution, and a chain of two checked as old -> newest
    for sd in seeds:
        v = bn.verify_contribution(sec, new, seed=sd)
        assert v["ok"] is True and v["checks_run"] == 31 and v["checks_bad"] == 0 and all(x is True for x in v["checks"].values()), v
    assert bn.verify_contribution(sec, newest, seed=seeds[0])["ok"] is True
    assert bn.verify_contribution(new, newest)["ok"] is True
    assert set(v["ms"]) == {"sums", "pairings", "total"}
    pk_old, pk_new = synth.sections_to_pkey(sec), synth.sections_to_pkey(new)
    assert no_ms(bn.verify_contribution(pk_old, pk_new, seed=seeds[0])) == no_ms(v)
    if tmp_path is not None:
        from wasmsnark_amd import formats
        p_old, p_new = os.path.join(str(tmp_path), "old.bin"), os.path.join(str(tmp_path), "new.wsnark64")
        open(p_old, "wb").write(pk_old)
        formats.write_key_container(new, p_new)
        assert no_ms(bn.verify_contribution(p_old, p_new)) == no_ms(v)

    fin_c, fin_h = pk.finite_indices(new, "C"), pk.finite_indices(new, "H")
    cases = []
    # one C' point replaced by another valid point
    bad = pk.mutable(new)
    bad["pointsC"][64 * fin_c[1]:64 * fin_c[1] + 64] = bytes(new["pointsC"][64 * fin_c[2]:64 * fin_c[2] + 64])
    cases.append((bad, ("C",), 31))
    # two hExps' entries swapped
    bad = pk.mutable(new)
    j, k = fin_h[1], fin_h[-2]
    bad["pointsH"][64 * j:64 * j + 64], bad["pointsH"][64 * k:64 * k + 64] = bytes(new["pointsH"][64 * k:64 * k + 64]), bytes(new["pointsH"][64 * j:64 * j + 64])
    cases.append((bad, ("H",), 31))
    # C scaled by d1^-1 but hExps by d2^-1
    other, _ = bn.contribute_key(sections=sec, d=d2)
    cases.append((dict(new, pointsH=other["pointsH"]), ("H",), 31))
    # delta2' from another d than delta1': bits 2 and 3 not run
    cases.append((dict(new, delta2=other["delta2"]), ("delta1~delta2",), 1 | 2 | 16))
    # one byte of A
    bad = pk.mutable(new)
    bad["pointsA"][64 * 3 + 40] ^= 1
    cases.append((bad, ("unchanged",), 31))
    # one coefficient of polsB
    bad = dict(new, polsB=bytearray(new["polsB"]))
    bad["polsB"][8 + 5] ^= 0x10
    cases.append((bad, ("unchanged",), 31))
    for bad, names, run in cases:
        for sd in (seeds if names == ("C",) else seeds[1:]):
            v = bn.verify_contribution(sec, bad, seed=sd, check=False)
            _only_bad(v, *names)
            assert v["checks_run"] == run, (v, names)
    # another circuit's size: bit 0, and the sums are not run
    circ6, S6, sec6 = pk.synth_sections(bn, log_domain + 1, seed=seed)
    v = bn.verify_contribution(sec, sec6, check=False)
    assert v["checks_bad"] & 1 and not v["checks_run"] & 12 and v["ok"] is False
    # d = 1: bit 4 only
    same, rep = bn.contribute_key(sections=sec, d=1)
    assert rep["ok"] is True
    assert_same_key(same, sec)
    _only_bad(bn.verify_contribution(sec, same), "delta_changed")
    # check=True refuses a new key with an off-curve C' point, with the audit's message
    bad = pk.mutable(new)
    pk.plant(bad, "C", fin_c[4], pk.OFF_CURVE)
    try:
        bn.verify_contribution(sec, bad)
        raise AssertionError("a key with an off-curve point was checked")
    except WsnarkError as e:
        assert "failed its audit" in str(e) and "section C" in str(e) and "index %d" % fin_c[4] in str(e) and pk.OFF_CURVE in str(e)
    # ... and without the audit the same bytes do not fault the check: the sum is meaningless, the bit bad
    assert bn.verify_contribution(sec, bad, check=False)["checks_bad"] & BIT["C"]


# ---- 5. bad inputs and errors ----
def _raw(cls):
    rep = cls()
    C.memset(C.byref(rep), 0x5A, C.sizeof(rep))
    return rep


def expected_bad(sec):
    out = {}
    for name in ("C", "H"):
        inf, bad, first, reason = pk.expected_section(sec[pk.SEC_KEY[name]], 64)
        out[name] = {"points": len(sec[pk.SEC_KEY[name]]) // 64, "infinity": inf, "bad": bad, "first_bad": first, "first_reason": reason}
    return out


def check_bad_inputs(bn, sec, tmp_path, tune, chunk):
    """Unreduced and off-curve points in C and hExps at index 0, the last index and both sides of a chunk boundary: counts, first
    index and reason by the Python classifier; ok = 0; the file variant leaves no output."""
    from wasmsnark_amd import synth
    tune(bn.lib, "PKDELTA_CHUNK", chunk)
    results = []
    for name in ("C", "H"):
        fin = pk.finite_indices(sec, name)
        assert len(sec[pk.SEC_KEY[name]]) // 64 > chunk
        below, above = max(i for i in fin if i < chunk), min(i for i in fin if i >= chunk)
        for plants in ([(fin[0], pk.UNREDUCED)], [(fin[-1], pk.OFF_CURVE)], [(below, pk.OFF_CURVE)], [(above, pk.UNREDUCED)],
                       [(above, pk.OFF_CURVE), (below, pk.UNREDUCED), (fin[-1], pk.UNREDUCED), (fin[0 if name == "H" else 1], pk.OFF_CURVE)]):
            bad = pk.mutable(sec)
            for i, what in plants:
                pk.plant(bad, name, i, what)
            new, rep = bn.contribute_key(sections=bad, d=D_FIXED)
            want = expected_bad(bad)
            assert new is None and rep["ok"] is False and {k: rep[k] for k in ("C", "H")} == want, (name, plants, rep, want)
            assert rep[name]["bad"] == len(plants) and rep[name]["first_bad"] == min(i for i, _ in plants)
            results.append((bad, rep))
    bad, rep = results[-1]
    p_in, p_out = os.path.join(str(tmp_path), "bad.bin"), os.path.join(str(tmp_path), "bad_out.bin")
    open(p_in, "wb").write(synth.sections_to_pkey(bad))
    got, rep_f = bn.contribute_key(path=p_in, out_path=p_out, d=D_FIXED)
    assert got is None and no_ms(rep_f) == no_ms(rep) and not os.path.exists(p_out)
    bn.lib.tune("PKDELTA_CHUNK", None)
    assert no_ms(bn.contribute_key(sections=bad, d=D_FIXED)[1]) == no_ms(rep)      # the report does not depend on the chunk size
    # delta1 at infinity, delta2 off its curve: ok = 0
    for name, spoil in (("delta1", lambda b: b.__setitem__(slice(0, 32), bytes(32))), ("delta2", lambda b: b.__setitem__(64, b[64] ^ 1))):
        bad = pk.mutable(sec)
        spoil(bad[name])
        new, rep = bn.contribute_key(sections=bad, d=D_FIXED)
        assert new is None and rep["ok"] is False and rep["C"]["bad"] == rep["H"]["bad"] == 0


def check_errors(bn, sec, tmp_path, so_path):
    from wasmsnark_amd import synth
    from wasmsnark_amd.bn128 import _DeltaReport, _DeltaVerdict, _key_sections
    lib = bn.lib
    pkey = synth.sections_to_pkey(sec)
    untouched = bytes(_raw(_DeltaReport))
    out = (C.c_uint8 * len(pkey))()
    marker = bytes(out)

    def call(*a):
        rep = _raw(_DeltaReport)
        rc = lib.c.wsnark_pkey_contribute(*a, C.byref(rep))
        assert bytes(rep) == untouched and bytes(out) == marker, a[1:3]
        return rc

    d = le(D_FIXED)
    assert call(pkey, len(pkey), le(0), out, len(pkey)) == ERR_ARG                  # d = 0
    assert call(pkey, len(pkey), le(R), out, len(pkey)) == ERR_ARG                  # d = 0 mod r
    assert call(pkey, len(pkey), d, out, len(pkey) - 1) == ERR_SIZE                 # out_cap < len
    for cut in (100, 487, len(pkey) - 1, len(pkey) // 2):
        assert call(pkey[:cut], cut, d, out, len(pkey)) == ERR_FORMAT               # what the loader rejects, with its code
    # a short section through the sections entry point
    short = dict(sec, pointsH=bytes(sec["pointsH"])[:-64])
    ks, keep = _key_sections(short)
    bufs = [(C.c_uint8 * max(len(sec[k]), 1))() for k in ("pointsC", "pointsH", "delta1", "delta2")]
    rep = _raw(_DeltaReport)
    assert lib.c.wsnark_pkey_contribute_sections(C.byref(ks), d, *bufs, C.byref(rep)) == ERR_FORMAT
    assert bytes(rep) == untouched and all(not any(b) for b in bufs)
    v = _raw(_DeltaVerdict)
    assert lib.c.wsnark_pkey_delta_verify(pkey, len(pkey), pkey[:500], 500, None, C.byref(v)) == ERR_FORMAT
    assert bytes(v) == bytes(_raw(_DeltaVerdict))
    # files: cannot be opened; in and out the same file (by name, and through a link)
    p_in, p_link, p_out = (os.path.join(str(tmp_path), n) for n in ("e.bin", "e_link.bin", "e_out.bin"))
    open(p_in, "wb").write(pkey)
    os.link(p_in, p_link)
    rep = _raw(_DeltaReport)
    f = lambda a, b: lib.c.wsnark_pkey_contribute_file(os.fsencode(a), os.fsencode(b), d, C.byref(rep))
    assert f("/nonexistent/key.bin", p_out) == ERR_ARG and not os.path.exists(p_out)
    assert f(p_in, p_in) == ERR_ARG and f(p_in, p_link) == ERR_ARG
    assert f(p_in, "/nonexistent/dir/out.bin") == ERR_ARG
    assert bytes(rep) == untouched and open(p_in, "rb").read() == pkey
    # before wsnark_init: a fresh process that loads the library and never initialises it
    code = ("import ctypes as C, sys\n"
            "c = C.CDLL(sys.argv[1])\n"
            "rep = (C.c_uint8 * 256)(*([90] * 256))\n"
            "vp, sz = C.c_void_p, C.c_size_t\n"
            "c.wsnark_pkey_contribute.argtypes = [vp, sz, vp, vp, sz, vp]\n"
            "c.wsnark_pkey_contribute_file.argtypes = [C.c_char_p, C.c_char_p, vp, vp]\n"
            "c.wsnark_pkey_delta_verify.argtypes = [vp, sz, vp, sz, vp, vp]\n"
            "c.wsnark_g1_scale_batch.argtypes = [vp, C.c_uint64, vp, vp]\n"
            "k, o = bytes(600), (C.c_uint8 * 600)()\n"
            "print(c.wsnark_pkey_contribute(k, 600, None, o, 600, rep), c.wsnark_pkey_contribute_file(b'x', b'y', None, rep),\n"
            "      c.wsnark_pkey_delta_verify(k, 600, k, 600, None, rep), c.wsnark_g1_scale_batch(k, 1, k, o), set(rep))\n")
    res = subprocess.run([sys.executable, "-c", code, so_path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == [str(ERR_NOINIT)] * 4 + ["{90}"], (res.stdout, res.stderr)


def check_library_drawn_secret(bn, sec):
    """d = None: the library draws d itself.  Two calls give different keys, each is exactly the old key under a new delta."""
    a, ra = bn.contribute_key(sections=sec)
    b, rb = bn.contribute_key(sections=sec)
    assert ra["ok"] and rb["ok"]
    assert a["delta1"] != b["delta1"] and a["pointsC"] != b["pointsC"] and a["pointsH"] != b["pointsH"]
    assert a["delta1"] != sec["delta1"] and a["pointsA"] == sec["pointsA"]
    assert bn.verify_contribution(sec, a)["ok"] is True and bn.verify_contribution(sec, b)["ok"] is True


# ---- keys at size: the closed form from the native generator's key scalars ----
def native_closed_form(bn, log_domain, d, seed, style="rows"):
    """(sections, sections after a contribution by d) of a NativeCircuit key: the logarithm of every key point is known
    (wsnark_synth_key_scalars), so C', hExps', delta1', delta2' are fixed-base multiples through mul_base.  C[3] is made infinity
    on both sides if the circuit gives no infinity entry."""
    from wasmsnark_amd import synth
    nc = synth.NativeCircuit(bn.lib, log_domain, n_public=2, seed=seed, style=style)
    sec = nc.build_sections()[0]
    nv, npub, dom = nc.n_vars, nc.n_public, nc.domain
    nC = nv - npub - 1
    s1 = bytearray(nc.info.n_g1_scalars * 32)
    bn.lib.check(bn.lib.c.wsnark_synth_key_scalars(nc._h, 1, nc._cbuf(s1)))
    val = lambda i: int.from_bytes(s1[32 * i:32 * i + 32], "little")
    delta, dinv = val(2), pow(d, -1, R)
    assert bn.mul_base(1, le(delta)) == bytes(sec["delta1"])
    o = 3 + 2 * nv
    scaled = b"".join(le(val(i) * dinv % R) for i in range(o, o + nC + dom))
    pts = bn.mul_base(1, scaled)
    want = dict(sec, pointsC=bytearray(pts[:64 * nC]), pointsH=pts[64 * nC:], delta1=bn.mul_base(1, le(delta * d % R)),
                delta2=bn.mul_base(2, le(delta * d % R)))
    sec["pointsC"] = bytearray(sec["pointsC"])
    if len(pk.finite_indices(sec, "C")) == nC:
        sec["pointsC"][64 * 3:64 * 4] = want["pointsC"][64 * 3:64 * 4] = bytes(64)
    nc.free()
    return sec, want
