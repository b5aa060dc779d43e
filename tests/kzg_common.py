"""Shared checks of the KZG calls (wsnark_kzg_srs_load, wsnark_kzg_commit, wsnark_kzg_open, wsnark_kzg_verify, wsnark_fr_poly_eval,
wsnark_fr_poly_divide; csrc/kzg.hip), run by tests/test_emul_kzg.py on the thread-emulator build of the kernel sources and by
tests/test_gpu_kzg.py on the device.

The yardstick is never the code under test.  The field side is compared with Python integers: y = f(z) mod r, q by the recurrence,
and q(X)(X - z) + y == f(X) coefficient by coefficient.  The curve side runs on a reference string written down from a KNOWN tau
(synth.powers_from_toxic): a commitment must be mul_base((s f(tau)) mod r) -- an independent kernel that the parity tests pin -- and
the normalised g1_multiexp over the same points; a proof must be mul_base of the Python quotient at tau.  What wsnark_kzg_verify must
say about a spoilt opening is worked out from the LOGARITHMS the test wrote the points down from (verdict_of below) and written down
in each case, never read off the library."""
import ctypes as C
import random
import subprocess
import sys
import threading
import types

from bn128_ref import Q, R
from wasmsnark_amd import synth
from wasmsnark_amd.bn128 import G1_GEN, G2_GEN

ERR_SIZE, ERR_FORMAT, ERR_ARG, ERR_NOINIT = 1, 2, 4, 5
SEG_DEFAULT = 4                    # the shipped run length (csrc/kzg.hip: KZ_SEG_DEFAULT); a tile is 256 runs
PAD_PCT_DEFAULT = 50               # the shipped switch between the prefix sum and the padded table sum (csrc/kzg.hip: kz_pad)
TAU = 0x1D2C3B4A5968778695A4B3C2D1E0F00112233445566778899AABBCCDDEEFF01 % R
TOP = (1 << 256) - 1


def le(v):
    return int(v).to_bytes(32, "little")


def poly_bytes(f):
    return b"".join(le(c) for c in f)


def ints(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def py_eval(f, z):
    acc = 0
    for c in reversed(f):
        acc = (acc * z + c) % R
    return acc


def py_divide(f, z):
    """(q, y) by the recurrence q[len-2] = f[len-1], q[k-1] = f[k] + z q[k], y = f[0] + z q[0]"""
    z %= R
    q = [0] * (len(f) - 1)
    acc = 0
    for k in range(len(f) - 1, 0, -1):
        acc = (f[k] + z * acc) % R
        q[k - 1] = acc
    return q, (f[0] + z * acc) % R


def tile_sizes(seg):
    t = 256 * seg
    return (t - 1, t, t + 1, 2 * t + 3)


def random_poly(rnd, n):
    """any 256-bit value per coefficient, the planted ones among them"""
    f = [rnd.randrange(1 << 256) for _ in range(n)]
    for i in range(3, n, 17):
        f[i] = (0, R - 1, R, TOP)[(i // 17) % 4]
    return f


# ---- the field side ----
def check_divide(bn, f, z):
    q, y = bn.poly_divide(poly_bytes(f), z)
    wq, wy = py_divide(f, z)
    assert y == le(wy), (len(f), z)
    assert q == poly_bytes(wq), (len(f), z, next(i for i, (a, b) in enumerate(zip(ints(q), wq)) if a != b))
    assert bn.poly_eval(poly_bytes(f), z) == le(wy)
    # q(X)(X - z) + y == f(X), coefficient by coefficient, from the library's own bytes
    got, zz = ints(q), z % R
    for k in range(len(f)):
        c = ((got[k - 1] if k >= 1 else 0) - zz * (got[k] if k < len(got) else 0) + (wy if k == 0 else 0)) % R
        assert c == f[k] % R, (len(f), k)
    return q, y


def check_divide_sizes(bn, sizes, seed=7):
    rnd = random.Random(seed)
    for n in sizes:
        check_divide(bn, random_poly(rnd, n), rnd.randrange(1 << 256))


def check_divide_forced_seg(bn, tune, seg, extra=()):
    tune(bn.lib, "KZG_SEG", seg)
    check_divide_sizes(bn, tile_sizes(seg) + tuple(extra), seed=10 + seg)


def check_divide_seg_independent(bn, tune, sizes):
    """the bytes of q and y across SEG in {1, 3, default}"""
    rnd = random.Random(21)
    cases = [(random_poly(rnd, n), rnd.randrange(R)) for n in sizes]
    got = []
    for seg in (1, 3, None):
        bn.lib.tune("KZG_SEG", seg)
        got.append([bn.poly_divide(poly_bytes(f), z) for f, z in cases])
    assert got[0] == got[1] == got[2]
    for (f, z), (q, y) in zip(cases, got[2]):
        wq, wy = py_divide(f, z)
        assert q == poly_bytes(wq) and y == le(wy)


def check_divide_planted(bn, n=300):
    rnd = random.Random(33)
    f = random_poly(rnd, n)
    for z in (0, 1, R - 1, R, TOP):
        check_divide(bn, f, z)
    z = rnd.randrange(R)
    q, y = check_divide(bn, [0] * n, z)
    assert set(q) == {0} and y == le(0)
    q, y = check_divide(bn, [0] * (n - 1) + [5], z)                      # only the top coefficient
    assert ints(q) == [5 * pow(z, n - 2 - k, R) % R for k in range(n - 1)] and y == le(5 * pow(z, n - 1, R))
    g = [rnd.randrange(R) for _ in range(n - 1)]                         # f = (X - z) g: y = 0 and q = g exactly
    f = [((g[k - 1] if k >= 1 else 0) - z * (g[k] if k < n - 1 else 0)) % R for k in range(n)]
    q, y = check_divide(bn, f, z)
    assert ints(q) == g and y == le(0)
    q, y = check_divide(bn, [TOP] + [0] * (n - 1), z)                    # a constant at len > 1
    assert set(q) == {0} and y == le(TOP % R)


def check_eval_counts(bn, n=300):
    rnd = random.Random(44)
    polys = [random_poly(rnd, n) for _ in range(5)]
    z = rnd.randrange(1 << 256)
    for count in (1, 2, 5):
        got = bn.poly_eval([poly_bytes(f) for f in polys[:count]], z)
        assert got == [bn.poly_eval(poly_bytes(f), z) for f in polys[:count]] == [le(py_eval(f, z % R)) for f in polys[:count]]


# ---- the curve side: a reference string from a known tau ----
_srs_memo = {}


def srs_of(bn, log_n, s=1):
    """tau_g1[k] = s tau^k G1 for k < n = 2^log_n (the tau_g1 array of synth.powers_from_toxic's transcript for the domain n / 2, times
    s through mul_base when s != 1), g2 | tau g2, and the resident handle"""
    key = (id(bn), log_n, s)
    if key not in _srs_memo:
        n = 1 << log_n
        toxic = types.SimpleNamespace(tau=TAU, alpha=3, beta=5)
        if s == 1 and n >= 4:
            P = synth.powers_from_toxic(toxic, n // 2, bn.mul_base)
            tau_g1, g2_pair = P["tau_g1"], P["tau_g2"][:256]
        else:
            tau_g1 = bn.mul_base(1, poly_bytes([s * pow(TAU, k, R) % R for k in range(n)]))
            g2_pair = bn.mul_base(2, poly_bytes([1, TAU]))
        assert len(tau_g1) == 64 * n and g2_pair[:128] == G2_GEN
        _srs_memo[key] = (tau_g1, g2_pair, bn.load_srs(tau_g1))
    return _srs_memo[key]


def point_of(bn, log):
    return bn.mul_base(1, le(log % R))


def want_commit(bn, f, s=1):
    return point_of(bn, s * py_eval(f, TAU))


def normalised(jac96):
    return bytes(64) if jac96[64:96] == bytes(32) else jac96[:64]


def check_commit(bn, tune, log_n, multiexp_lens=()):
    tau_g1, _, srs = srs_of(bn, log_n)
    n = 1 << log_n
    assert srs.info()["n"] == n and srs.info()["bytes"] >= 64 * n
    rnd = random.Random(55)
    below = (PAD_PCT_DEFAULT * n + 99) // 100 - 1          # the last len of the prefix sum; below + 1 is the first padded one
    for ln in sorted({1, 2, below, below + 1, n - 1, n}):
        f = random_poly(rnd, ln)
        got = srs.commit(poly_bytes(f))
        assert got == want_commit(bn, f), ln
        if ln in multiexp_lens:
            assert got == normalised(bn.g1_multiexp(poly_bytes(f), tau_g1[:64 * ln])), ln
    # the two sums of a shorter polynomial: same bytes whichever the switch picks
    f = random_poly(rnd, n // 2)
    got = []
    for pct in (0, 101):
        tune(bn.lib, "KZG_PAD_PCT", pct)
        got.append(srs.commit(poly_bytes(f)))
    assert got[0] == got[1] == want_commit(bn, f)
    bn.lib.tune("KZG_PAD_PCT", None)
    # three at once, a zero polynomial among them
    polys = [random_poly(rnd, n - 1), [0] * (n - 1), random_poly(rnd, n - 1)]
    got = srs.commit([poly_bytes(f) for f in polys])
    assert got == [srs.commit(poly_bytes(f)) for f in polys] == [want_commit(bn, f) for f in polys] and got[1] == bytes(64)


def check_commit_evaluations(bn, log_n):
    """form 1: the evaluations bn.fft gives of f must commit to what f commits to"""
    _, _, srs = srs_of(bn, log_n)
    rnd = random.Random(66)
    for ln in (1 << log_n, 1 << (log_n - 1), 1):
        f = [rnd.randrange(R) for _ in range(ln)]
        ev = bn.fromMontgomeryN(bn.fft(bn.toMontgomeryN(poly_bytes(f)))) if ln > 1 else poly_bytes(f)
        assert srs.commit(ev, form=1) == srs.commit(poly_bytes(f)) == want_commit(bn, f), ln


def want_open(bn, polys, z, gamma, s=1):
    """(ys, proof) in closed form: F = sum gamma^i f_i, q from the Python division, pi = (s q(tau)) G"""
    F = [sum(pow(gamma, i, R) * f[k] for i, f in enumerate(polys)) % R for k in range(len(polys[0]))]
    q, _ = py_divide(F, z)
    return [le(py_eval(f, z % R)) for f in polys], point_of(bn, s * py_eval(q, TAU))


def check_open(bn, log_n, lens=None):
    _, _, srs = srs_of(bn, log_n)
    n = 1 << log_n
    rnd = random.Random(77)
    for ln in lens or (n, n - 1):
        f = random_poly(rnd, ln)
        for z in (rnd.randrange(1 << 256), 0, TAU):
            assert srs.open(poly_bytes(f), z) == want_open(bn, [f], z, 0), (ln, z)
    ys, proof = srs.open(poly_bytes([9] + [0] * (n - 1)), 12345)          # a constant: the proof is infinity
    assert ys == [le(9)] and proof == bytes(64)
    ys, proof = srs.open(le(TOP), 7)                                      # len == 1
    assert ys == [le(TOP % R)] and proof == bytes(64)
    polys = [random_poly(rnd, n - 3) for _ in range(3)]
    z, gamma = rnd.randrange(R), rnd.randrange(1 << 256)
    assert srs.open([poly_bytes(f) for f in polys], z, gamma) == want_open(bn, polys, z, gamma % R)


def verdict_of(c_logs, ys, z, gamma, pi_log, s=1, g2_log=1, tau_g2_log=TAU):
    """e(C - y g1 + z pi, g2) == e(pi, tau g2) in the exponent: logarithms to the standard generators"""
    c = sum(pow(gamma, i, R) * ci for i, ci in enumerate(c_logs)) % R
    y = sum(pow(gamma, i, R) * yi for i, yi in enumerate(ys)) % R
    return (c - y * s + z * pi_log) * g2_log % R == pi_log * tau_g2_log % R


def check_verify(bn, log_n, s=1):
    """what open produced is accepted; each spoilt part on its own is rejected.  s != 1: a commitment generator s G"""
    tau_g1, g2_pair, srs = srs_of(bn, log_n, s)
    n = 1 << log_n
    g1 = tau_g1[:64]
    rnd = random.Random(88 + s)
    polys = [[rnd.randrange(R) for _ in range(n)] for _ in range(3)]
    z, gamma = rnd.randrange(R), rnd.randrange(R)
    for count in (1, 3):
        fs = polys[:count]
        gm = gamma if count > 1 else None
        ys, proof = srs.open([poly_bytes(f) for f in fs], z, gm)
        cs = srs.commit([poly_bytes(f) for f in fs])
        assert (ys, proof) == want_open(bn, fs, z, gamma if count > 1 else 0, s) and cs == [want_commit(bn, f, s) for f in fs]
        c_logs, y_ints = [s * py_eval(f, TAU) % R for f in fs], [py_eval(f, z) for f in fs]
        F = [sum(pow(gamma if count > 1 else 0, i, R) * f[k] for i, f in enumerate(fs)) % R for k in range(n)]
        pi_log = s * py_eval(py_divide(F, z)[0], TAU) % R
        g = gamma if count > 1 else 0
        assert verdict_of(c_logs, y_ints, z, g, pi_log, s) is True
        assert bn.kzg_verify(g1, g2_pair, cs, z, ys, proof, gm) is True
        # y + 1
        assert verdict_of(c_logs, [y_ints[0] + 1] + y_ints[1:], z, g, pi_log, s) is False
        assert bn.kzg_verify(g1, g2_pair, cs, z, [le((y_ints[0] + 1) % R)] + ys[1:], proof, gm) is False
        # z + 1
        assert verdict_of(c_logs, y_ints, z + 1, g, pi_log, s) is False
        assert bn.kzg_verify(g1, g2_pair, cs, (z + 1) % R, ys, proof, gm) is False
        # pi replaced by 2 pi
        assert verdict_of(c_logs, y_ints, z, g, 2 * pi_log, s) is False
        assert bn.kzg_verify(g1, g2_pair, cs, z, ys, point_of(bn, 2 * pi_log), gm) is False
        # one C_i replaced
        assert verdict_of(c_logs[:-1] + [c_logs[-1] + 1], y_ints, z, g, pi_log, s) is False
        assert bn.kzg_verify(g1, g2_pair, cs[:-1] + [point_of(bn, c_logs[-1] + 1)], z, ys, proof, gm) is False
        # tau g2 replaced by 2 tau g2
        assert verdict_of(c_logs, y_ints, z, g, pi_log, s, tau_g2_log=2 * TAU) is False
        assert bn.kzg_verify(g1, g2_pair[:128] + bn.mul_base(2, le(2 * TAU % R)), cs, z, ys, proof, gm) is False
        if count > 1:      # a wrong gamma
            assert verdict_of(c_logs, y_ints, z, gamma + 1, pi_log, s) is False
            assert bn.kzg_verify(g1, g2_pair, cs, z, ys, proof, (gamma + 1) % R) is False
    # pi at infinity: a constant polynomial; C at infinity: the zero polynomial
    for const in (11, 0):
        f = [const] + [0] * (n - 1)
        ys, proof = srs.open(poly_bytes(f), z)
        c = srs.commit(poly_bytes(f))
        assert proof == bytes(64) and c == point_of(bn, s * const) and verdict_of([s * const], [const], z, 0, 0, s) is True
        assert bn.kzg_verify(g1, g2_pair, c, z, ys, proof) is True
        assert verdict_of([s * const], [const + 1], z, 0, 0, s) is False
        assert bn.kzg_verify(g1, g2_pair, c, z, le(const + 1), proof) is False


def check_verify_inputs(bn):
    """unreduced coordinates are WSNARK_ERR_FORMAT; points off the curve or outside the subgroup are a verdict"""
    from wasmsnark_amd._lib import WsnarkError
    g2_pair = bn.mul_base(2, poly_bytes([1, TAU]))
    c, pi = point_of(bn, 5), bytes(64)                 # the constant 5: y = 5, proof infinity
    assert bn.kzg_verify(G1_GEN, g2_pair, c, 3, le(5), pi) is True
    unreduced = le(int.from_bytes(c[:32], "little") + Q) + c[32:]
    for args in ((unreduced, g2_pair, c, pi), (G1_GEN, g2_pair, unreduced, pi), (G1_GEN, g2_pair, c, unreduced),
                 (G1_GEN, le(int.from_bytes(g2_pair[:32], "little") + Q) + g2_pair[32:], c, pi)):
        try:
            bn.kzg_verify(args[0], args[1], args[2], 3, le(5), args[3])
            raise AssertionError("an unreduced coordinate was accepted")
        except WsnarkError as e:
            assert e.code == ERR_FORMAT
    off = c[:32] + le((int.from_bytes(c[32:], "little") + 1) % Q)
    assert bn.kzg_verify(G1_GEN, g2_pair, off, 3, le(5), pi) is False
    assert bn.kzg_verify(G1_GEN, g2_pair, c, 3, le(5), off) is False
    assert bn.kzg_verify(off, g2_pair, c, 3, le(5), pi) is False
    assert bn.kzg_verify(bytes(64), g2_pair, c, 3, le(5), pi) is False                  # g1 at infinity is no generator
    off2 = g2_pair[:128] + g2_pair[128:224] + le((int.from_bytes(g2_pair[224:], "little") + 1) % Q)
    assert bn.kzg_verify(G1_GEN, off2, c, 3, le(5), pi) is False
    # a point of the twist outside the order-r subgroup, as tau g2 and as g2
    import pkey_check_common as pk
    rogue = pk.rogue_g2_bytes()
    assert pk.classify(rogue) == pk.OUTSIDE
    assert bn.kzg_verify(G1_GEN, g2_pair[:128] + rogue, c, 3, le(5), pi) is False
    assert bn.kzg_verify(G1_GEN, rogue + g2_pair[128:], c, 3, le(5), pi) is False


def check_threads(bn, log_n):
    _, _, srs = srs_of(bn, log_n)
    rnd = random.Random(99)
    polys = [poly_bytes(random_poly(rnd, (1 << log_n) - i)) for i in range(2)]
    want = [srs.commit(p) for p in polys]
    got = [None, None]

    def run(i):
        got[i] = [srs.commit(polys[i]) for _ in range(3)]
    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert got == [[w] * 3 for w in want]


# ---- errors ----
def check_errors(bn, log_n, so_path):
    tau_g1, g2_pair, srs = srs_of(bn, log_n)
    c, h, n = bn.lib.c, srs._h, 1 << log_n
    rnd = random.Random(111)
    f = poly_bytes(random_poly(rnd, n))
    before = srs.commit(f)
    z, gm = le(5), le(6)
    sent = lambda k: (C.c_uint8 * k)(*([90] * k))
    out, ys, proof, q, valid = sent(64 * 3), sent(32 * 3), sent(64), sent(32 * n), C.c_int(-7)
    big = (1 << 24) + 1
    rows = [
        # NULL pointers, a NULL handle
        (c.wsnark_kzg_commit(None, f, n, 1, 0, out), ERR_ARG), (c.wsnark_kzg_commit(h, None, n, 1, 0, out), ERR_ARG),
        (c.wsnark_kzg_commit(h, f, n, 1, 0, None), ERR_ARG), (c.wsnark_kzg_commit(h, f, n, 1, 2, out), ERR_ARG),
        (c.wsnark_kzg_commit_dev(None, f, n, 1, 0, out, None), ERR_ARG),
        (c.wsnark_kzg_open(None, f, n, 1, z, None, ys, proof), ERR_ARG), (c.wsnark_kzg_open(h, None, n, 1, z, None, ys, proof), ERR_ARG),
        (c.wsnark_kzg_open(h, f, n, 1, None, None, ys, proof), ERR_ARG), (c.wsnark_kzg_open(h, f, n, 1, z, None, None, proof), ERR_ARG),
        (c.wsnark_kzg_open(h, f, n, 1, z, None, ys, None), ERR_ARG), (c.wsnark_kzg_open(h, f, n // 2, 2, z, None, ys, proof), ERR_ARG),
        (c.wsnark_kzg_open_dev(None, f, n, 1, z, None, ys, proof, None), ERR_ARG),
        (c.wsnark_fr_poly_eval(None, n, 1, z, ys), ERR_ARG), (c.wsnark_fr_poly_eval(f, n, 1, None, ys), ERR_ARG),
        (c.wsnark_fr_poly_eval(f, n, 1, z, None), ERR_ARG),
        (c.wsnark_fr_poly_divide(None, n, z, q, ys), ERR_ARG), (c.wsnark_fr_poly_divide(f, n, None, q, ys), ERR_ARG),
        (c.wsnark_fr_poly_divide(f, n, z, None, ys), ERR_ARG), (c.wsnark_fr_poly_divide(f, n, z, q, None), ERR_ARG),
        (c.wsnark_fr_poly_divide_dev(None, n, z, q, ys, None), ERR_ARG),
        (c.wsnark_kzg_srs_load(None, n, C.byref(C.c_void_p())), ERR_ARG), (c.wsnark_kzg_srs_load(tau_g1, n, None), ERR_ARG),
        (c.wsnark_kzg_srs_info(None, None, None), ERR_ARG),
        (c.wsnark_kzg_verify(None, g2_pair, before, 1, z, None, ys, before, C.byref(valid)), ERR_ARG),
        (c.wsnark_kzg_verify(G1_GEN, g2_pair, before, 2, z, None, ys, before, C.byref(valid)), ERR_ARG),
        (c.wsnark_kzg_verify(G1_GEN, g2_pair, before, 1, z, None, ys, before, None), ERR_ARG),
        # sizes
        (c.wsnark_kzg_commit(h, f, 0, 1, 0, out), ERR_SIZE), (c.wsnark_kzg_commit(h, f, n + 1, 1, 0, out), ERR_SIZE),
        (c.wsnark_kzg_commit(h, f, big, 1, 0, out), ERR_SIZE), (c.wsnark_kzg_commit(h, f, n - 1, 1, 1, out), ERR_SIZE),
        (c.wsnark_kzg_open(h, f, 0, 1, z, gm, ys, proof), ERR_SIZE), (c.wsnark_kzg_open(h, f, n + 1, 1, z, gm, ys, proof), ERR_SIZE),
        (c.wsnark_kzg_open(h, f, big, 1, z, gm, ys, proof), ERR_SIZE),
        (c.wsnark_fr_poly_eval(f, 0, 1, z, ys), ERR_SIZE), (c.wsnark_fr_poly_eval(f, big, 1, z, ys), ERR_SIZE),
        (c.wsnark_fr_poly_divide(f, 0, z, q, ys), ERR_SIZE), (c.wsnark_fr_poly_divide(f, big, z, q, ys), ERR_SIZE),
        (c.wsnark_kzg_srs_load(tau_g1, 0, C.byref(C.c_void_p())), ERR_SIZE), (c.wsnark_kzg_srs_load(tau_g1, big, C.byref(C.c_void_p())), ERR_SIZE),
        # count == 0 touches nothing
        (c.wsnark_kzg_commit(h, None, n, 0, 0, None), 0), (c.wsnark_kzg_open(h, None, n, 0, None, None, None, None), 0),
        (c.wsnark_fr_poly_eval(None, n, 0, None, None), 0), (c.wsnark_kzg_verify(None, None, None, 0, None, None, None, None, None), 0),
        (c.wsnark_kzg_commit(h, f, n, 0, 0, out), 0), (c.wsnark_kzg_open(h, f, n, 0, z, gm, ys, proof), 0),
    ]
    for i, (got, want) in enumerate(rows):
        assert got == want, (i, got, want)
    assert set(out) == set(ys) == set(proof) == set(q) == {90} and valid.value == -7
    c.wsnark_kzg_srs_free(None)
    assert srs.commit(f) == before and srs.info()["n"] == n             # the handle is as it was
    # before wsnark_init: a fresh process that loads the library and never initialises it; the check alone needs no context
    code = ("import ctypes as C, sys\n"
            "c = C.CDLL(sys.argv[1])\n"
            "vp, u64 = C.c_void_p, C.c_uint64\n"
            "c.wsnark_kzg_srs_load.argtypes = [vp, u64, vp]\n"
            "c.wsnark_fr_poly_eval.argtypes = [vp, u64, u64, vp, vp]\n"
            "c.wsnark_fr_poly_divide.argtypes = [vp, u64, vp, vp, vp]\n"
            "c.wsnark_fr_poly_divide_dev.argtypes = [vp, u64, vp, vp, vp, vp]\n"
            "c.wsnark_kzg_commit.argtypes = [vp, vp, u64, u64, C.c_int, vp]\n"
            "c.wsnark_kzg_commit_dev.argtypes = [vp, vp, u64, u64, C.c_int, vp, vp]\n"
            "c.wsnark_kzg_open.argtypes = [vp, vp, u64, u64, vp, vp, vp, vp]\n"
            "c.wsnark_kzg_open_dev.argtypes = [vp, vp, u64, u64, vp, vp, vp, vp, vp]\n"
            "c.wsnark_kzg_verify.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp]\n"
            "b, h, v = bytes(256), C.c_void_p(), C.c_int(-1)\n"
            "fake = C.c_void_p(8)\n"
            "rcs = [c.wsnark_kzg_srs_load(b, 2, C.byref(h)), c.wsnark_fr_poly_eval(b, 2, 1, b, b), c.wsnark_fr_poly_divide(b, 2, b, b, b),\n"
            "       c.wsnark_fr_poly_divide_dev(b, 2, b, b, b, None), c.wsnark_kzg_commit(fake, b, 2, 1, 0, b),\n"
            "       c.wsnark_kzg_commit_dev(fake, b, 2, 1, 0, b, None), c.wsnark_kzg_open(fake, b, 2, 1, b, b, b, b),\n"
            "       c.wsnark_kzg_open_dev(fake, b, 2, 1, b, b, b, b, None)]\n"
            "g1, g2 = bytes.fromhex(sys.argv[2]), bytes.fromhex(sys.argv[3])\n"
            "rc = c.wsnark_kzg_verify(g1, g2 + g2, bytes(64), 1, b, None, bytes(32), bytes(64), C.byref(v))\n"
            "print(rcs, rc, v.value)\n")
    res = subprocess.run([sys.executable, "-c", code, so_path, G1_GEN.hex(), G2_GEN.hex()], capture_output=True, text=True, timeout=120)
    # (the zero polynomial: C and pi at infinity, y = 0 -- accepted under any pair of G2 points)
    assert res.stdout.strip() == "%s 0 1" % ([ERR_NOINIT] * 8), (res.stdout, res.stderr)


def check_srs_load_errors(bn, log_n):
    from wasmsnark_amd._lib import WsnarkError
    tau_g1, _, _ = srs_of(bn, log_n)
    n = 1 << log_n
    off, unred, inf = bytearray(tau_g1), bytearray(tau_g1), bytearray(tau_g1)
    off[64 * (n - 2) + 32] ^= 1
    unred[64 * 3:64 * 3 + 32] = le(int.from_bytes(tau_g1[64 * 3:64 * 3 + 32], "little") + Q)
    inf[64 * 5:64 * 5 + 32] = bytes(32)
    both = bytearray(inf)
    both[64 * 9 + 32] ^= 1                                                # an infinity at 5 BEFORE an off-curve point at 9
    for bad, index, why in ((off, n - 2, "off the curve"), (unred, 3, "unreduced"), (inf, 5, "at infinity"), (both, 5, "at infinity")):
        try:
            bn.load_srs(bytes(bad))
            raise AssertionError("a bad power was loaded")
        except WsnarkError as e:
            assert e.code == ERR_FORMAT and "index %d " % index in str(e) and why in str(e), str(e)
