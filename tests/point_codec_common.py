"""Shared checks of the square roots (field.h / field29.h / fp2.h through wsnark_selftest_field ops 18 and 19) and of the compressed
points and proofs (csrc/pointcodec.hip), run by tests/test_emul_point_codec.py on the thread-emulator build of the kernel sources
and by tests/test_gpu_point_codec.py on the device.  The yardstick is Python integers: bn128_ref's fields and curves, and the
encoder / decoder below, written from the statement of the two encodings in include/wsnark.h.  Nothing here shares code with the
library.  NOT checked, here or anywhere: bytes written by arkworks or gnark themselves (none were available)."""
import ctypes as C
import random
import subprocess
import sys

import bn128_ref as ref
from bn128_ref import Q, R
from conftest import load_golden

OK, ERR_SIZE, ERR_ARG, ERR_NOINIT = 0, 1, 4, 5
ST_SQRT, ST_IS_SQUARE = 18, 19
HALF = (Q - 1) // 2
ENCODINGS = ("le", "be")
ENC_ID = {"le": 1, "be": 2}
FF = b"\xff" * 32


# ---- Python integers: roots and signs ----
def fq_sqrt(a):
    r = pow(a, (Q + 1) // 4, Q)
    return r if r * r % Q == a % Q else None


def larger(y):
    return y > HALF


def f2_larger(y):
    return larger(y[1]) if y[1] else larger(y[0])


def f2_neg(y):
    return ((-y[0]) % Q, (-y[1]) % Q)


def f2_sqr(a):
    return ref._f2_mul(a, a)


def f2_sqrt(a):
    """bn128_ref._f2_sqrt, completed for c1 = 0: there its candidate t can be 0, and it answers None for (c, 0) with c a non-square
    of Fq -- which is the square of (0, sqrt(-c)), as -1 is a non-square for q = 3 mod 4.  Every element of Fq is a square in Fq2."""
    if a[1] % Q == 0:
        r = fq_sqrt(a[0] % Q)
        return (r, 0) if r is not None else (0, fq_sqrt((-a[0]) % Q))
    return ref._f2_sqrt(a)


def f2_split_branch(a):
    """Which way the x0^2 = +-t split of the complex method goes for a square a with c1 != 0: '+' or '-'."""
    s = fq_sqrt((a[0] * a[0] + a[1] * a[1]) % Q)
    t = (a[0] + s) * pow(2, -1, Q) % Q
    x0 = pow(t, (Q + 1) // 4, Q)
    return "+" if x0 * x0 % Q == t else "-"


# ---- 1. field roots through the self-test ops ----
def _selftest(lib, which, impl, op, vals):
    """vals: integers (which 0) or pairs (which 2), plain -> the raw output bytes per element"""
    sz = 32 if which == 0 else 64
    a = b"".join(ref.mont(v) if which == 0 else ref.mont(v[0]) + ref.mont(v[1]) for v in vals)
    out = (C.c_uint8 * (len(vals) * sz))()
    rc = lib.c.wsnark_selftest_field(which, impl, op, a, a, out, len(vals))
    assert rc == OK, (which, impl, op, rc, (lib.c.wsnark_last_error() or b"").decode())
    b = bytes(out)
    return [b[i * sz:(i + 1) * sz] for i in range(len(vals))]


def fq_values(seed=1):
    rnd = random.Random(seed)
    edge = [0, 1, 2, 3, 4, Q - 1, HALF, HALF - 1, HALF + 1, HALF - 2, HALF + 2]
    m29 = (1 << 29) - 1
    limb = []                                      # the 2^29 k boundaries, as tests/field29_contracts.py picks them
    for i in range(8):
        limb += [m29 << (29 * i), 1 << (29 * i), (1 << (29 * i)) - 1]
    limb += [sum(m29 << (29 * i) for i in range(8) if i % 2 == par) for par in (0, 1)]
    limb = [v % Q for v in limb]
    squares = [pow(rnd.randrange(Q), 2, Q) for _ in range(200)]
    return edge + limb + squares + [rnd.randrange(Q) for _ in range(200)]


def check_fq_roots(bn, impl):
    vals = fq_values()
    assert fq_sqrt(3) is None and fq_sqrt(Q - 1) is None and fq_sqrt(4) in (2, Q - 2)
    roots, flags = _selftest(bn.lib, 0, impl, ST_SQRT, vals), _selftest(bn.lib, 0, impl, ST_IS_SQUARE, vals)
    n_sq = 0
    for v, rb, fb in zip(vals, roots, flags):
        want = fq_sqrt(v)
        assert int.from_bytes(fb, "little") == (1 if want is not None else 0), v
        if want is None:
            assert rb == FF, v
            continue
        n_sq += 1
        r = ref.from_mont(rb)
        assert int.from_bytes(rb, "little") < Q and r % 2 == 0 and r * r % Q == v and r in (want, Q - want), v
    assert n_sq >= 200 and len(vals) - n_sq >= 50
    # counts around a wavefront's edge, one call each
    for n in (1, 63, 64, 65, 257):
        assert _selftest(bn.lib, 0, impl, ST_SQRT, vals[:n]) == roots[:n], n


def fq2_values(seed=2):
    rnd = random.Random(seed)
    nonsq_norm = next((a, b) for a in range(1, 50) for b in range(1, 50) if fq_sqrt((a * a + b * b) % Q) is None)
    planted = [(0, 0), (4, 0), (3, 0), (0, 4), (0, 3), (Q - 1, 0), (0, Q - 1), nonsq_norm, (1, 1), (HALF, HALF + 1)]
    squares = [f2_sqr((rnd.randrange(Q), rnd.randrange(Q))) for _ in range(200)]
    return planted, squares, [(rnd.randrange(Q), rnd.randrange(Q)) for _ in range(200)]


def check_fq2_roots(bn, impl):
    planted, squares, rand = fq2_values()
    assert ref._f2_sqrt(planted[7]) is None and fq_sqrt(4) is not None and fq_sqrt(3) is None
    branches = {f2_split_branch(a) for a in squares if a[1]}
    assert branches == {"+", "-"}, "both branches of the x0^2 = +-t split must be among the random squares"
    vals = planted + squares + rand
    roots, flags = _selftest(bn.lib, 2, impl, ST_SQRT, vals), _selftest(bn.lib, 2, impl, ST_IS_SQUARE, vals)
    n_none = 0
    for v, rb, fb in zip(vals, roots, flags):
        want = f2_sqrt(v)
        assert want == ref._f2_sqrt(v) or v[1] == 0
        assert int.from_bytes(fb, "little") == (1 if want is not None else 0), v
        if want is None:
            n_none += 1
            assert rb == FF + FF, v
            continue
        if f2_larger(want):
            want = f2_neg(want)
        got = (ref.from_mont(rb[:32]), ref.from_mont(rb[32:]))
        assert got == want and f2_sqr(got) == v, v
    assert n_none >= 50
    assert all(f2_sqrt(v) is not None for v in planted[:7] + squares)
    for n in (1, 63, 64, 65, 257):
        assert _selftest(bn.lib, 2, impl, ST_SQRT, vals[:n]) == roots[:n], n


def check_fr_has_no_root(bn):
    out = (C.c_uint8 * 32)(*([7] * 32))
    for impl in (0, 2):
        for op in (ST_SQRT, ST_IS_SQUARE):
            assert bn.lib.c.wsnark_selftest_field(1, impl, op, ref.mont(4), ref.mont(4), out, 1) == ERR_ARG


# ---- the encodings, from their statement ----
def _flagged(x, enc, flag_larger, inf):
    """32 bytes of x with the two flag bits; x < 2^254"""
    assert 0 <= x < 1 << 254
    if enc == "le":
        b = bytearray(x.to_bytes(32, "little"))
        b[31] |= 0x40 if inf else (0x80 if flag_larger else 0)
    else:
        b = bytearray(x.to_bytes(32, "big"))
        b[0] |= 0x40 if inf else (0xC0 if flag_larger else 0x80)
    return bytes(b)


def enc_g1(pt, enc):
    if pt is None:
        return _flagged(0, enc, False, True)
    return _flagged(pt[0], enc, larger(pt[1]), False)


def enc_g2(pt, enc):
    x, big, inf = ((0, 0), False, True) if pt is None else (pt[0], f2_larger(pt[1]), False)
    if enc == "le":
        return x[0].to_bytes(32, "little") + _flagged(x[1], enc, big, inf)
    return _flagged(x[1], enc, big, inf) + x[0].to_bytes(32, "big")


def enc_point(g, pt, enc):
    return enc_g1(pt, enc) if g == 1 else enc_g2(pt, enc)


def dec_point(g, rec, enc, subgroup=False):
    """(status, point): 0 with a point or None for infinity; 1 malformed, 2 no point, 3 outside the subgroup, all with None"""
    parts = [rec] if g == 1 else [rec[:32], rec[32:]]
    if enc == "be":
        parts = parts[::-1]
    words = [int.from_bytes(p, "little" if enc == "le" else "big") for p in parts]          # c0, c1
    f, words[-1] = words[-1] >> 254, words[-1] & ((1 << 254) - 1)
    if f == (3 if enc == "le" else 0):
        return 1, None
    if f == 1:
        return (1, None) if any(words) else (0, None)
    sign = f == (2 if enc == "le" else 3)
    if any(w >= Q for w in words):
        return 1, None
    if g == 1:
        y = fq_sqrt((words[0] ** 3 + 3) % Q)
        if y is None:
            return 2, None
        return 0, (words[0], y if larger(y) == sign else (Q - y) % Q)
    x = (words[0], words[1])
    y = f2_sqrt(ref._f2_add(ref._f2_mul(ref._f2_mul(x, x), x), ref.B2_TWIST))
    if y is None:
        return 2, None
    if f2_larger(y) != sign:
        y = f2_neg(y)
    if subgroup and not ref.g2_times_r_is_infinity((x, y)):
        return 3, None
    return 0, (x, y)


def key_bytes(g, pt):
    """affine point -> the key format (Montgomery words; infinity: zero bytes)"""
    if pt is None:
        return bytes(64 * g)
    if g == 1:
        return ref.mont(pt[0]) + ref.mont(pt[1])
    return ref.mont(pt[0][0]) + ref.mont(pt[0][1]) + ref.mont(pt[1][0]) + ref.mont(pt[1][1])


_points = {}


def sample_points(g):
    """generators, negatives, infinity, k G for 64 random k (computed once)"""
    if g not in _points:
        rnd = random.Random(40 + g)
        gen = ref.G1 if g == 1 else ref.G2
        neg = (lambda p: (p[0], (Q - p[1]) % Q)) if g == 1 else (lambda p: (p[0], f2_neg(p[1])))
        fb = ref.FixedBase(ref.g1_add if g == 1 else ref.g2_add, gen)
        pts = [gen, neg(gen), None] + [fb.mul(rnd.randrange(1, R)) for _ in range(64)]
        _points[g] = pts
    return _points[g]


# ---- 2. the codec against the yardstick ----
def check_literal_vectors(bn):
    one, two = ref.mont(1), ref.mont(2)
    g1, ng1, inf = one + two, one + ref.mont(Q - 2), bytes(64)
    want = {"le": [b"\x01" + bytes(31), b"\x01" + bytes(30) + b"\x80", bytes(31) + b"\x40"],
            "be": [b"\x80" + bytes(30) + b"\x01", b"\xc0" + bytes(30) + b"\x01", b"\x40" + bytes(31)]}
    for enc in ENCODINGS:
        out, st = bn.compress_points(1, g1 + ng1 + inf, enc)
        assert st == [0, 0, 0] and [out[0:32], out[32:64], out[64:96]] == want[enc], enc
        back, st = bn.decompress_points(1, out, enc)
        assert st == [0, 0, 0] and back == g1 + ng1 + inf


def check_codec(bn, g):
    pts = sample_points(g)
    raw = b"".join(key_bytes(g, p) for p in pts)
    sz = 32 * g
    if g == 2:
        ys = [p[1] for p in pts if p is not None]
        assert any(y[1] > HALF for y in ys) and any(0 < y[1] <= HALF for y in ys)
    # signs at the half: the compressor does not test the curve equation, so any reduced (x, y) shows them.  y.c1 = 0 on G2 is
    # shown the same way; no POINT of the twist with y.c1 = 0 was looked for (the field-level test has (c, 0) values)
    if g == 1:
        edge = [(5, HALF), (5, HALF + 1), (5, HALF - 1), (Q - 1, Q - 1), (7, 1)]
    else:
        edge = [((5, 6), (1, HALF)), ((5, 6), (1, HALF + 1)), ((5, 6), (HALF, 0)), ((5, 6), (HALF + 1, 0)), ((5, 6), (Q - 1, 0)),
                ((0, 6), (HALF + 1, 1)), ((6, 0), (0, Q - 1))]
    for enc in ENCODINGS:
        out, st = bn.compress_points(g, raw, enc)
        assert st == [0] * len(pts)
        assert out == b"".join(enc_point(g, p, enc) for p in pts), enc
        back, st = bn.decompress_points(g, out, enc, subgroup=(g == 2))
        assert st == [0] * len(pts) and back == raw, enc                      # decompress(compress(P)) == P
        again, st = bn.compress_points(g, back, enc)
        assert again == out                                                   # compress(decompress(e)) == e
        assert [dec_point(g, out[i * sz:(i + 1) * sz], enc) for i in range(len(pts))] == [(0, p) for p in pts]
        out, st = bn.compress_points(g, b"".join(key_bytes(g, p) for p in edge), enc)
        assert st == [0] * len(edge) and out == b"".join(enc_point(g, p, enc) for p in edge), enc
    # an unreduced coordinate: status 1 and a zero record, the neighbours untouched
    le = ref.le
    for word in range(2 * g):
        bad = bytearray(key_bytes(g, pts[3]))
        bad[32 * word:32 * word + 32] = le(Q + word)
        out, st = bn.compress_points(g, key_bytes(g, pts[4]) + bytes(bad) + key_bytes(g, pts[5]), "le")
        assert st == [0, 1, 0] and out == enc_point(g, pts[4], "le") + bytes(sz) + enc_point(g, pts[5], "le"), word


# ---- 3. planted bad encodings ----
def _raw_x(g, words, enc, f):
    """a record from raw component values (c0, c1) and the two raw flag bits, no range check"""
    w = list(words)
    w[-1] |= f << 254
    parts = [v.to_bytes(32, "little" if enc == "le" else "big") for v in w]
    return b"".join(parts if enc == "le" else parts[::-1])


def planted_records(g, enc):
    """(label, record, want status without the subgroup test, with it)"""
    fin, fin_big, inf, bad = {"le": (0, 2, 1, 3), "be": (2, 3, 1, 0)}[enc]
    z = (0,) * (g - 1)
    items = [("x = q", _raw_x(g, z + (Q,), enc, fin), 1), ("x = q + 1", _raw_x(g, z + (Q + 1,), enc, fin_big), 1),
             ("x = 2^254 - 1", _raw_x(g, z + ((1 << 254) - 1,), enc, fin), 1),
             ("undefined flags", _raw_x(g, (1,) * g, enc, bad), 1),
             ("infinity and another bit", _raw_x(g, (1,) + z, enc, inf), 1),
             ("infinity and a high bit", _raw_x(g, z + (1 << 200,), enc, inf), 1)]
    if g == 2:
        items.append(("c0 = q", _raw_x(g, (Q, 1), enc, fin), 1))
        for x, has in (((0, 0), False), ((1, 1), False), ((0, 2), False), ((0, 1), True), ((1, 0), True)):
            items.append(("x = %r" % (x,), _raw_x(g, x, enc, fin), 0 if has else 2))
    else:
        for x, has in ((0, False), (4, False), (10, False), (1, True), (2, True), (3, True)):
            items.append(("x = %d" % x, _raw_x(g, (x,), enc, fin_big), 0 if has else 2))
    out = [(label, rec, st, st) for label, rec, st in items]
    if g == 2:
        rogue = ref.twist_point_outside_g2()
        out.append(("outside the subgroup", enc_g2(rogue, enc), 0, 3))
        # (small x: not in the subgroup either, with overwhelming probability; the yardstick decides)
        out = [(l, r, a, b if b else dec_point(2, r, enc, True)[0]) for l, r, a, b in out]
    return out


def _decompress_raw(lib, g, data, enc, flags):
    n = len(data) // (32 * g)
    out, st, bad = (C.c_uint8 * (n * 64 * g))(*([7] * (n * 64 * g))), (C.c_uint8 * n)(*([7] * n)), C.c_uint64(77)
    fn = lib.c.wsnark_g1_decompress if g == 1 else lib.c.wsnark_g2_decompress
    rc = fn(data, n, ENC_ID[enc], flags, out, st, C.byref(bad))
    assert rc == OK, (rc, (lib.c.wsnark_last_error() or b"").decode())
    return bytes(out), list(st), bad.value


def check_planted_points(bn, g):
    """every bad record at index 0, 63, 64 and last of a 130-point call, between valid neighbours: statuses, n_bad, zero outputs,
    and every neighbour as if it were alone"""
    pts = [p for p in sample_points(g) if p is not None]
    base = (pts * 3)[:130]
    sz, psz = 32 * g, 64 * g
    for enc in ENCODINGS:
        good = [enc_point(g, p, enc) for p in base]
        good_out = [key_bytes(g, p) for p in base]
        items = planted_records(g, enc)
        for label, rec, st0, st1 in items:
            s, pt = dec_point(g, rec, enc)
            assert s == st0, (label, enc, s)
            for sub in ((0, 1) if g == 2 and st1 != st0 else (0,)):      # the 254-doubling chain only where it decides
                want_st = st1 if sub else st0
                recs, want = list(good), list(good_out)
                for pos in (0, 63, 64, 129):
                    recs[pos] = rec
                    want[pos] = key_bytes(g, pt) if want_st == 0 else bytes(psz)
                out, st, n_bad = _decompress_raw(bn.lib, g, b"".join(recs), enc, sub)
                assert st == [want_st if i in (0, 63, 64, 129) else 0 for i in range(130)], (label, enc, sub)
                assert n_bad == (4 if want_st else 0) and out == b"".join(want), (label, enc, sub)


# ---- 4. proofs ----
def _proof_points(pr):
    a, b, c = pr["pi_a"], pr["pi_b"], pr["pi_c"]
    return ((int(a[0]), int(a[1])), ((int(b[0][0]), int(b[0][1])), (int(b[1][0]), int(b[1][1]))), (int(c[0]), int(c[1])))


def enc_proof(pr, enc):
    A, B, Cp = _proof_points(pr)
    return enc_g1(A, enc) + enc_g2(B, enc) + enc_g1(Cp, enc)


def _normal(pr):
    """(x, y, 1) of each point, as strings"""
    A, B, Cp = _proof_points(pr)
    s = str
    return {"pi_a": [s(A[0]), s(A[1]), "1"], "pi_b": [[s(B[0][0]), s(B[0][1])], [s(B[1][0]), s(B[1][1])], ["1", "0"]], "pi_c": [s(Cp[0]), s(Cp[1]), "1"]}


def _on_curves(pr):
    A, B, Cp = _proof_points(pr)
    return ref.g1_on_curve(*A) and ref.g1_on_curve(*Cp) and ref.g2_on_twist(*B)


def golden_proofs():
    g = load_golden("proofs.json")
    return [c["proof"] for name in ("t3", "t6") for c in g[name]]


def check_proof_codec(bn):
    proofs = golden_proofs() + [c["proof"] for c in load_golden("verify.json")["cases"]]
    proofs = [p for p in proofs if _on_curves(p)]
    assert len(proofs) >= 6
    for enc in ENCODINGS:
        want = b"".join(enc_proof(p, enc) for p in proofs)
        out, st = bn.compress_proofs(proofs, enc)
        assert st == [1] * len(proofs) and out == want, enc
        back, st = bn.decompress_proofs(want, enc)
        assert st == [1] * len(proofs) and back == [_normal(p) for p in proofs], enc
    # z is ignored by the compressor unless it is unreduced; any unreduced word makes the proof malformed
    p = proofs[0]
    odd = dict(p, pi_a=[p["pi_a"][0], p["pi_a"][1], "0"], pi_c=p["pi_c"][:2] + ["5"])
    bad_z = dict(p, pi_c=p["pi_c"][:2] + [str(Q)])
    bad_y = dict(p, pi_b=[p["pi_b"][0], [p["pi_b"][1][0], str(Q + 3)], p["pi_b"][2]])
    out, st = bn.compress_proofs([p, odd, bad_z, p, bad_y, p], "le")
    e = enc_proof(p, "le")
    assert st == [1, 1, 2, 1, 2, 1] and out == e + e + bytes(128) + e + bytes(128) + e


def planted_proofs(enc, good):
    """(label, 128 bytes, status of the decompressor, status of the verifier) around the valid proof `good`"""
    A, B, Cp = _proof_points(good)
    e = enc_proof(good, enc)
    fin = {"le": 0, "be": 2}[enc]
    flipped = enc_g1((A[0], (Q - A[1]) % Q), enc)
    return [("valid", e, 1, 1),
            ("sign of A flipped", flipped + e[32:], 1, 0),
            ("A.x = 4: no point", _raw_x(1, (4,), enc, fin) + e[32:], 0, 0),
            ("A.x = q", _raw_x(1, (Q,), enc, fin) + e[32:], 2, 2),
            ("C.x = 2^254 - 1", e[:96] + _raw_x(1, ((1 << 254) - 1,), enc, fin), 2, 2),
            ("B outside the subgroup", e[:32] + enc_g2(ref.twist_point_outside_g2(), enc) + e[96:], 1, 0),
            ("B.x = (1, 1): no point", e[:32] + _raw_x(2, (1, 1), enc, fin) + e[96:], 0, 0),
            ("C at infinity", e[:96] + enc_g1(None, enc), 0, 0)]


def _verify_raw(lib, vkb, n_in, inputs_b, proofs_b, enc, dev=None):
    n = len(proofs_b) // 128
    st = (C.c_uint8 * n)(*([7] * n))
    if dev is None:
        rc = lib.c.wsnark_groth16_verify_batch_compressed(vkb, len(vkb), inputs_b if n_in else None, n_in, proofs_b, n, ENC_ID[enc], st)
    else:
        (p_in, k1), (p_pr, k2) = dev(inputs_b), dev(proofs_b)
        rc = lib.c.wsnark_groth16_verify_batch_compressed_dev(vkb, len(vkb), p_in if n_in else None, n_in, p_pr, n, ENC_ID[enc], st, None)
    assert rc == OK, (rc, (lib.c.wsnark_last_error() or b"").decode())
    return list(st)


def check_planted_proofs(bn, dev, batch=130):
    """dev(bytes) -> (device address, keep-alive): how this build puts a buffer where the _dev call reads it"""
    from wasmsnark_amd.bn128 import vk_to_bytes
    import verify_batch_common as vb
    vk, pub = vb._vk("t6")
    gp = load_golden("proofs.json")["t6"]
    n_in = len(pub)
    vkb, ib = vk_to_bytes(vk, n_in), vb._inputs_bytes(pub)
    for enc in ENCODINGS:
        cases = planted_proofs(enc, gp[1]["proof"])
        other = enc_proof(gp[0]["proof"], enc)
        # alone, and what the decompressor says
        for label, rec, dst, vst in cases:
            assert _verify_raw(bn.lib, vkb, n_in, ib, rec, enc) == [vst], (label, enc)
            got, st = bn.decompress_proofs(rec, enc)
            assert st == [dst] and (got[0] is None) == (dst != 1), (label, enc)
        # between valid neighbours, in one batch; the same batch through device pointers
        rnd = random.Random(9)
        pick = list(range(len(cases))) + [0] * (batch - len(cases))
        rnd.shuffle(pick)
        recs = [other if (k == 0 and i % 2) else cases[k][1] for i, k in enumerate(pick)]
        want = [cases[k][3] for k in pick]
        assert _verify_raw(bn.lib, vkb, n_in, ib * batch, b"".join(recs), enc) == want, enc
        if enc == "le":
            assert _verify_raw(bn.lib, vkb, n_in, ib * batch, b"".join(recs), enc, dev=dev) == want
            assert bn.groth16VerifyBatchCompressed(vk, [pub] * 8, recs[:8], enc, return_status=True) == want[:8]
            assert bn.groth16VerifyBatchCompressed(vk, [pub] * 8, b"".join(recs[:8]), enc) == [w == 1 for w in want[:8]]


def check_golden_verify_compressed(bn, enc="le"):
    """the reference verifier's vectors: compressed by the yardstick, verified compressed and uncompressed, against the recorded verdicts"""
    g = load_golden("verify.json")
    vk, cases = g["verification_key"], g["cases"]
    want = [int(bool(c["reference_verdict"])) for c in cases]
    assert sum(want) == 3
    inputs, proofs = [c["inputs"] for c in cases], [c["proof"] for c in cases]
    assert bn.groth16VerifyBatch(vk, inputs, proofs, return_status=True) == want
    assert bn.groth16VerifyBatchCompressed(vk, inputs, [enc_proof(p, enc) for p in proofs], enc, return_status=True) == want


def check_golden_proofs_compressed(bn):
    import verify_batch_common as vb
    for name in ("t3", "t6"):
        vk, pub = vb._vk(name)
        inputs, proofs, want = [], [], []
        for c in load_golden("proofs.json")[name]:
            inputs += [pub, [str((int(pub[0]) + 1) % R)] + pub[1:]]
            proofs += [c["proof"], c["proof"]]
            want += [True, False]
        assert bn.groth16VerifyBatch(vk, inputs, proofs) == want
        for enc in ENCODINGS:
            data, st = bn.compress_proofs(proofs, enc)
            assert st == [1] * len(proofs)
            assert bn.groth16VerifyBatchCompressed(vk, inputs, data, enc) == want, (name, enc)


# ---- 5. errors: the outputs are untouched ----
def check_errors(bn, so_path):
    import pytest
    from wasmsnark_amd.bn128 import vk_to_bytes
    import verify_batch_common as vb
    lib = bn.lib
    c = lib.c
    vk, pub = vb._vk("t6")
    n_in = len(pub)
    vkb, ib = vk_to_bytes(vk, n_in), vb._inputs_bytes(pub)
    e = enc_proof(load_golden("proofs.json")["t6"][0]["proof"], "le")
    pt, rec = key_bytes(1, ref.G1), enc_g1(ref.G1, "le")
    pt2, rec2 = key_bytes(2, ref.G2), enc_g2(ref.G2, "le")

    def fresh(n):
        return (C.c_uint8 * n)(*([7] * n))

    def untouched(*bufs):
        return all(bytes(b) == b"\x07" * len(b) for b in bufs)

    for enc_id in (0, 3, -1):                                            # unknown encodings
        out, st, bad = fresh(128), fresh(1), C.c_uint64(77)
        assert c.wsnark_g1_compress(pt, 1, enc_id, out, st, C.byref(bad)) == ERR_ARG
        assert c.wsnark_g2_compress(pt2, 1, enc_id, out, st, C.byref(bad)) == ERR_ARG
        assert c.wsnark_g1_decompress(rec, 1, enc_id, 0, out, st, C.byref(bad)) == ERR_ARG
        assert c.wsnark_g2_decompress(rec2, 1, enc_id, 0, out, st, C.byref(bad)) == ERR_ARG
        big = fresh(384)
        assert c.wsnark_proof_compress(bytes(384), 1, enc_id, out, st) == ERR_ARG
        assert c.wsnark_proof_decompress(e, 1, enc_id, big, st) == ERR_ARG
        assert c.wsnark_groth16_verify_batch_compressed(vkb, len(vkb), ib, n_in, e, 1, enc_id, st) == ERR_ARG
        assert c.wsnark_groth16_verify_batch_compressed_dev(vkb, len(vkb), ib, n_in, e, 1, enc_id, st, None) == ERR_ARG
        assert untouched(out, st, big) and bad.value == 77
    out, st, bad = fresh(128), fresh(1), C.c_uint64(77)
    assert c.wsnark_g1_decompress(rec, 1, 1, 2, out, st, C.byref(bad)) == ERR_ARG            # an undefined flag
    # NULL pointers
    assert c.wsnark_g1_compress(None, 1, 1, out, st, C.byref(bad)) == ERR_ARG
    assert c.wsnark_g1_compress(pt, 1, 1, None, st, C.byref(bad)) == ERR_ARG
    assert c.wsnark_g1_compress(pt, 1, 1, out, None, C.byref(bad)) == ERR_ARG
    assert c.wsnark_g1_compress(pt, 1, 1, out, st, None) == ERR_ARG
    assert c.wsnark_g2_decompress(None, 1, 1, 0, out, st, C.byref(bad)) == ERR_ARG
    assert c.wsnark_g2_decompress(rec2, 1, 1, 0, out, None, C.byref(bad)) == ERR_ARG
    assert c.wsnark_proof_compress(None, 1, 1, out, st) == ERR_ARG and c.wsnark_proof_compress(bytes(384), 1, 1, out, None) == ERR_ARG
    assert c.wsnark_proof_decompress(e, 1, 1, None, st) == ERR_ARG
    assert c.wsnark_groth16_verify_batch_compressed(None, len(vkb), ib, n_in, e, 1, 1, st) == ERR_ARG
    assert c.wsnark_groth16_verify_batch_compressed(vkb, len(vkb), None, n_in, e, 1, 1, st) == ERR_ARG
    assert c.wsnark_groth16_verify_batch_compressed(vkb, len(vkb), ib, n_in, None, 1, 1, st) == ERR_ARG
    assert c.wsnark_groth16_verify_batch_compressed(vkb, len(vkb), ib, n_in, e, 1, 1, None) == ERR_ARG
    assert untouched(out, st) and bad.value == 77
    # n == 0: nothing is touched, not even the pointers
    assert c.wsnark_g1_compress(None, 0, 1, None, None, None) == OK and c.wsnark_g2_decompress(None, 0, 9, 0, None, None, None) == OK
    assert c.wsnark_proof_compress(None, 0, 1, None, None) == OK and c.wsnark_proof_decompress(None, 0, 1, None, None) == OK
    assert c.wsnark_groth16_verify_batch_compressed(None, 0, None, 0, None, 0, 1, None) == OK
    assert bn.compress_points(1, b"", "le") == (b"", []) and bn.decompress_proofs(b"", "be") == ([], [])
    assert bn.groth16VerifyBatchCompressed(vk, [], b"", "le") == []
    # count > 2^24, a key with too few IC points, an unreduced key coordinate
    assert c.wsnark_groth16_verify_batch_compressed(vkb, len(vkb), ib, n_in, e, (1 << 24) + 1, 1, st) == ERR_SIZE
    assert c.wsnark_groth16_verify_batch_compressed(vkb, len(vkb) - 64, ib, n_in, e, 1, 1, st) == ERR_SIZE
    bad_vk = vk_to_bytes(dict(vk, vk_alfa_1=[str(Q + 1), vk["vk_alfa_1"][1], "1"]), n_in)
    assert c.wsnark_groth16_verify_batch_compressed(bad_vk, len(bad_vk), ib, n_in, e, 1, 1, st) == vb.ERR_FORMAT
    assert untouched(st)
    # the Python layer
    with pytest.raises(ValueError):
        bn.compress_points(1, pt, "xx")
    with pytest.raises(ValueError):
        bn.decompress_points(2, rec, "le")                               # 32 bytes are no G2 record
    with pytest.raises(ValueError):
        bn.groth16VerifyBatchCompressed(vk, [pub], e + e, "le")
    # before wsnark_init: a fresh process that loads the library and never initialises it
    code = ("import ctypes as C, sys\n"
            "c = C.CDLL(sys.argv[1])\n"
            "st, out, bad = (C.c_uint8 * 1)(7), (C.c_uint8 * 384)(), C.c_uint64(77)\n"
            "u = C.c_uint64\n"
            "rcs = [c.wsnark_g1_compress(bytes(64), u(1), 1, out, st, C.byref(bad)), c.wsnark_g2_decompress(bytes(64), u(1), 1, 0, out, st, C.byref(bad)),\n"
            "       c.wsnark_proof_compress(bytes(384), u(1), 1, out, st), c.wsnark_proof_decompress(bytes(128), u(1), 1, out, st),\n"
            "       c.wsnark_groth16_verify_batch_compressed(bytes(512), C.c_size_t(512), None, u(0), bytes(128), u(1), 1, st)]\n"
            "print(*rcs, st[0], bad.value)\n")
    res = subprocess.run([sys.executable, "-c", code, so_path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == [str(ERR_NOINIT)] * 5 + ["7", "77"], (res.stdout, res.stderr)


def check_chunked_stream(bn, tune, g=1):
    """the staging loop with more than one chunk (CODEC_CHUNK at its smallest, 64 points): 130 points in three chunks"""
    pts = (sample_points(g) * 2)[:130]
    raw = b"".join(key_bytes(g, p) for p in pts)
    want = bn.compress_points(g, raw, "be")
    tune(bn.lib, "CODEC_CHUNK", 64)
    assert bn.compress_points(g, raw, "be") == want
    assert bn.decompress_points(g, want[0], "be") == (raw, [0] * 130)
