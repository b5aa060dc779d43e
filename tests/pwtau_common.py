"""Shared checks of powers of tau (wsnark_g{1,2}_mul_batch, wsnark_powers_contribute, wsnark_powers_check, csrc/pwtau.hip), run by
tests/test_emul_pwtau.py on the thread-emulator build of the kernel sources and by tests/test_gpu_pwtau.py on the device.

The yardstick is never the code under test.  mul_points is compared (a) at tiny sizes with affine double-and-add in Python integers
(bn128_ref) and (b) at every size with mul_base applied to the product of the logarithms, computed in Python -- an independent kernel
that the parity tests pin.  A contributed transcript is compared byte for byte with the closed form: synth.powers_from_toxic of the
toxic waste with tau, alpha, beta multiplied in Python (synth.contributed_toxic).  Bad powers are counted by the audit's pure-Python
classifier (pkey_check_common).  What the audit's relations must say about a spoilt transcript is worked out from the LOGARITHMS the
test wrote it down from (relations_expected below, and each case's own literal), never read off the library."""
import ctypes as C
import random
import subprocess
import sys

import pkey_check_common as pk
import pkey_delta_common as pd
import pkey_setup_common as ps
from bn128_ref import Q, R, g1_mul, g2_mul, le
from pkey_check_common import ERR_ARG, ERR_FORMAT, ERR_NOINIT, ERR_SIZE
from wasmsnark_amd import synth

WIN = 4                                      # the shipped window width (csrc/pwtau.hip: PW_WIN)
ARRAYS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1")
T_FIXED = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F00123456789ABCDEFFEDCBA987654321 % R
A_FIXED = 0x2468ACE013579BDF02468ACE13579BDFFDB97531ECA86420FDB97531ECA8642 % R
B_FIXED = (R - 5) // 3


def size_of(g):
    return 64 if g == 1 else 128


def inf9(g):
    """infinity by the loaders' rule (x == 0) with a non-zero y: "copied through byte for byte" is then visible"""
    sz = size_of(g)
    return bytes(sz // 2) + bytes([9]) + bytes(sz // 2 - 1)


def scalars_bytes(ks):
    return b"".join(int(k).to_bytes(32, "little") for k in ks)


def want_products(bn, g, logs, ks):
    """(s_i k_i) G through mul_base; a product that is 0 mod r is infinity: zero bytes"""
    return ps.points_of_logs(bn, g, [s * k % R for s, k in zip(logs, ks)])


# ---- 1. mul_points ----
def check_mul_integers(bn, g):
    """n = 1 .. 8 against g1_mul / g2_mul in affine Python integers"""
    mul = g1_mul if g == 1 else g2_mul
    sz = size_of(g)
    rnd = random.Random(40 + g)
    logs = [rnd.randrange(1, R) for _ in range(8)]
    ks = [rnd.randrange(R), R - 1, 1, 0, (1 << 256) - 1, R + 7, rnd.randrange(1 << 128), rnd.randrange(R)]
    pts = ps.points_of_logs(bn, g, logs)
    want = b"".join(pd.point_to_bytes(g, mul(pd.point_from_bytes(g, pts[sz * i:sz * i + sz]), ks[i] % R)) for i in range(8))
    for n in range(1, 9):
        got = bn.mul_points(g, pts[:sz * n], scalars_bytes(ks[:n]))
        assert got == want[:sz * n], (g, n, ps.differing(g, got, want[:sz * n]))


_sizes_memo = {}


def check_mul_sizes(bn, g, sizes):
    """Points s_i G times scalars k_i against mul_base((s_i k_i) mod r): the sizes at which a partial last wavefront or workgroup
    meets the shared inversion.  The reference is computed once for the largest size; every size is a prefix of it."""
    sz = size_of(g)
    top = max(sizes)
    key = (id(bn), g, top)
    if key not in _sizes_memo:
        rnd = random.Random(50 + g)
        logs = [rnd.randrange(1, R) for _ in range(top)]
        ks = [rnd.randrange(1 << 256) for _ in range(top)]      # any 256-bit value: reduced mod r
        for i in range(7, top, 29):
            ks[i] = (0, R, 1, R - 1)[(i // 29) % 4]
        _sizes_memo[key] = (ps.points_of_logs(bn, g, logs), scalars_bytes(ks), want_products(bn, g, logs, ks))
    pts, sc, want = _sizes_memo[key]
    for n in sizes:
        got = bn.mul_points(g, pts[:sz * n], sc[:32 * n])
        assert got == want[:sz * n], (g, n, ps.differing(g, got, want[:sz * n]))


def planted_scalars():
    """0, 1, 2, 3, the neighbours of r and of 2^256, 2^k and 2^k - 1 at every boundary of the 4-bit windows, and the scalars whose
    signed windows carry: 0x2FF..F (< r: every window below the top one is 15, so a carry enters each of them and the last one ends in
    the top window, bits 252..255, which holds 2 and becomes 3 -- for a scalar below r < 2^254 that window is at most 3 + 1 and nothing
    ever leaves it), 0x099..9 (every digit -7 with a carry, then -6), 0x088..8 (every window exactly 8: the largest digit that does
    NOT carry), and r - 1 (= -1: the chain ends on -P)."""
    ks = [0, 1, 2, 3, R - 1, R - 2, (R + 1) // 2, R, R + 1, (1 << 256) - 1, int("2" + "F" * 63, 16), int("09" + "9" * 62, 16),
          int("08" + "8" * 62, 16), int("2" + "8" * 63, 16), int("1" + "7" * 63, 16)]
    for j in range(1, 256 // WIN):
        ks += [1 << (WIN * j), (1 << (WIN * j)) - 1]
    ks += [(1 << 253), (1 << 253) - 1, (1 << 254) - 1, (1 << 255), 9 << 248, 8 << 248]
    return ks


def check_mul_planted(bn, g):
    """Every planted scalar on its own point, infinity inputs in both encodings among them: each copied through."""
    sz = size_of(g)
    ks = planted_scalars()
    assert int("2" + "F" * 63, 16) < R
    rnd = random.Random(60 + g)
    logs = [rnd.randrange(1, R) for _ in ks]
    pts = bytearray(ps.points_of_logs(bn, g, logs))
    want = bytearray(want_products(bn, g, logs, ks))
    for i, enc in ((5, bytes(sz)), (20, inf9(g)), (len(ks) - 1, inf9(g))):
        pts[sz * i:sz * i + sz] = enc
        want[sz * i:sz * i + sz] = enc
    got = bn.mul_points(g, pts, scalars_bytes(ks))
    assert got == bytes(want), (g, [hex(ks[i]) for i in ps.differing(g, got, bytes(want))])
    # a scalar that reduces to 0 gives infinity: zero bytes
    for i, k in enumerate(ks):
        if k % R == 0 and i not in (5, 20, len(ks) - 1):
            assert got[sz * i:sz * i + sz] == bytes(sz)
    # all infinity
    assert bn.mul_points(g, inf9(g) * 3 + bytes(sz), scalars_bytes([5, 0, R - 1, 7])) == inf9(g) * 3 + bytes(sz)


def check_mul_wavefront_shapes(bn, g):
    """A wavefront in which every lane has the same point and a different scalar; one in which every lane has the same scalar and a
    different point -- which must equal scale_points."""
    sz = size_of(g)
    rnd = random.Random(70 + g)
    s = rnd.randrange(1, R)
    ks = [rnd.randrange(R) for _ in range(64)]
    one = ps.points_of_logs(bn, g, [s])
    assert bn.mul_points(g, one * 64, scalars_bytes(ks)) == want_products(bn, g, [s] * 64, ks)
    logs = [rnd.randrange(1, R) for _ in range(64)]
    k = rnd.randrange(R)
    pts = ps.points_of_logs(bn, g, logs)
    got = bn.mul_points(g, pts, scalars_bytes([k] * 64))
    assert got == want_products(bn, g, logs, [k] * 64)
    assert got == bn.scale_points(g, pts, k)


def check_mul_outside_subgroup(bn):
    """A G2 point on the twist but outside the order-r subgroup with a handful of scalars below r, against g2_mul in integers: no
    error -- the subgroup test is not this call's -- and (k mod r) Q is what the integers give for k < r."""
    rogue = pk.rogue_g2_bytes()
    assert pk.classify(rogue) == pk.OUTSIDE
    Qp = pd.point_from_bytes(2, rogue)
    ks = [1, 2, 3, 8, 9, 16, R - 1, R - 2, (R + 1) // 2, int("2" + "F" * 63, 16), 0x123456789ABCDEF << 190]
    want = b"".join(pd.point_to_bytes(2, g2_mul(Qp, k)) for k in ks)
    got = bn.mul_points(2, rogue * len(ks), scalars_bytes(ks))
    assert got == want, ps.differing(2, got, want)


def check_mul_modes(bn, g, n=130):
    """The planted scalars, then random 256-bit ones, on random points with one infinity among them: the bytes of the yardstick"""
    sz = size_of(g)
    ks = planted_scalars()[:n]
    rnd = random.Random(80 + g)
    ks += [rnd.randrange(1 << 256) for _ in range(n - len(ks))]
    logs = [rnd.randrange(1, R) for _ in range(n)]
    pts = bytearray(ps.points_of_logs(bn, g, logs))
    want = bytearray(want_products(bn, g, logs, ks))
    pts[sz * 11:sz * 12] = want[sz * 11:sz * 12] = inf9(g)
    got = bn.mul_points(g, pts, scalars_bytes(ks))
    assert got == bytes(want), (g, ps.differing(g, got, bytes(want)))


def check_mul_chunks(bn, tune, n=150):
    """PWTAU_CHUNK = 64: three chunks give the bytes of one; a bad point in the LAST chunk leaves out untouched"""
    rnd = random.Random(90)
    logs = [rnd.randrange(1, R) for _ in range(n)]
    ks = [rnd.randrange(R) for _ in range(n)]
    pts = ps.points_of_logs(bn, 1, logs)
    want = want_products(bn, 1, logs, ks)
    tune(bn.lib, "PWTAU_CHUNK", 64)
    assert bn.mul_points(1, pts, scalars_bytes(ks)) == want
    bad = bytearray(pts)
    bad[64 * (n - 2) + 32] ^= 1
    out = (C.c_uint8 * len(bad))(*([90] * len(bad)))
    rc = bn.lib.c.wsnark_g1_mul_batch((C.c_uint8 * len(bad)).from_buffer(bad), scalars_bytes(ks), n, out)
    assert rc == ERR_FORMAT and set(out) == {90}
    assert "index %d" % (n - 2) in bn.lib.c.wsnark_last_error().decode()


def check_mul_errors(bn, so_path):
    from wasmsnark_amd._lib import WsnarkError
    c = bn.lib.c
    pts = bytearray(ps.points_of_logs(bn, 1, list(range(1, 129))))
    sc = scalars_bytes(range(3, 131))
    out = (C.c_uint8 * (128 * 128))(*([90] * (128 * 128)))
    buf = (C.c_uint8 * len(pts)).from_buffer(pts)
    for fn in (c.wsnark_g1_mul_batch, c.wsnark_g2_mul_batch):
        assert fn(buf, sc, 0, out) == 0 and fn(None, None, 0, None) == 0                     # n == 0 touches nothing
        assert fn(buf, sc, (1 << 24) + 1, out) == ERR_SIZE and fn(buf, sc, 1 << 40, out) == ERR_SIZE
        assert fn(None, sc, 4, out) == ERR_ARG and fn(buf, None, 4, out) == ERR_ARG and fn(buf, sc, 4, None) == ERR_ARG
    assert set(out) == {90}
    for index in (0, 66, 127):
        bad = bytearray(pts)
        bad[64 * index + 32] ^= 1
        try:
            bn.mul_points(1, bad, sc)
            raise AssertionError("an off-curve point was multiplied")
        except WsnarkError as e:
            assert e.code == ERR_FORMAT and "index %d" % index in str(e) and "1 point(s)" in str(e), str(e)
    bad = bytearray(pts)
    bad[64 * 9:64 * 9 + 32] = le(int.from_bytes(pts[64 * 9:64 * 9 + 32], "little") + Q)      # unreduced
    bad[64 * 70 + 32] ^= 1
    rc = c.wsnark_g1_mul_batch((C.c_uint8 * len(bad)).from_buffer(bad), sc, 128, out)
    msg = c.wsnark_last_error().decode()
    assert rc == ERR_FORMAT and "index 9" in msg and "2 point(s)" in msg and set(out) == {90}, msg
    # a G2 point off its curve
    p2 = bytearray(ps.points_of_logs(bn, 2, [5, 6, 7]))
    p2[128 * 2 + 64] ^= 1
    try:
        bn.mul_points(2, p2, sc[:96])
        raise AssertionError("an off-curve G2 point was multiplied")
    except WsnarkError as e:
        assert e.code == ERR_FORMAT and "index 2" in str(e)
    # before wsnark_init: a fresh process that loads the library and never initialises it
    code = ("import ctypes as C, sys\n"
            "c = C.CDLL(sys.argv[1])\n"
            "vp = C.c_void_p\n"
            "c.wsnark_g1_mul_batch.argtypes = c.wsnark_g2_mul_batch.argtypes = [vp, vp, C.c_uint64, vp]\n"
            "c.wsnark_powers_contribute.argtypes = [vp] * 10\n"
            "c.wsnark_powers_check.argtypes = [vp, C.c_uint32, vp, vp]\n"
            "k, o = bytes(256), (C.c_uint8 * 256)(*([90] * 256))\n"
            "print(c.wsnark_g1_mul_batch(k, k, 2, o), c.wsnark_g2_mul_batch(k, k, 1, o), c.wsnark_powers_contribute(*([None] * 9), o),\n"
            "      c.wsnark_powers_check(None, 0, None, o), set(o))\n")
    res = subprocess.run([sys.executable, "-c", code, so_path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == [str(ERR_NOINIT)] * 4 + ["{90}"], (res.stdout, res.stderr)


# ---- 2. the contribution ----
_tr_memo = {}


def transcript(bn, log_domain, seed=3):
    """(circuit, toxic waste, powers) of a synthetic transcript, built once"""
    key = (id(bn), log_domain, seed)
    if key not in _tr_memo:
        circ = synth.make_circuit(log_domain, n_public=2, seed=seed)
        S = synth.setup(circ, seed=seed + 50)
        _tr_memo[key] = (circ, S, synth.powers_from_toxic(S, circ.domain, bn.mul_base))
    return _tr_memo[key]


def assert_same_powers(got, want):
    assert got["domain"] == want["domain"]
    for name in ARRAYS + ("beta_g2",):
        size = 128 if name.endswith("g2") else 64
        assert bytes(got[name]) == bytes(want[name]), (name, ps.differing(size // 64, bytes(got[name]), bytes(want[name])))


def assert_good_contribution_report(rep, n):
    assert rep["ok"] is True and rep["beta_g2"] is None and rep["relations_run"] == 0 and rep["relations_bad"] == 0
    for name in ARRAYS:
        assert rep[name] == {"points": n * (2 if name == "tau_g1" else 1), "infinity": 0, "bad": 0, "first_bad": None, "first_reason": None}
    assert set(rep["ms"]) == {"device", "host", "total"} and rep["ms"]["total"] >= rep["ms"]["device"] > 0


def check_contribution_closed_form(bn, tune, log_domain, chunks=(None,)):
    """contribute_powers(powers_from_toxic(S), t, a, b) == powers_from_toxic(contributed_toxic(S, t, a, b)), all five parts, for every
    PWTAU_CHUNK of `chunks` (None: the default): a wrong global exponent base shows only when an array spans chunks."""
    circ, S, powers = transcript(bn, log_domain)
    want = synth.powers_from_toxic(synth.contributed_toxic(S, T_FIXED, A_FIXED, B_FIXED), circ.domain, bn.mul_base)
    assert want["tau_g1"] != powers["tau_g1"] and want["beta_g2"] != powers["beta_g2"]
    for chunk in chunks:
        if chunk is None:
            bn.lib.tune("PWTAU_CHUNK", None)
        else:
            tune(bn.lib, "PWTAU_CHUNK", chunk)
        new, rep = bn.contribute_powers(powers, T_FIXED, A_FIXED, B_FIXED)
        assert_good_contribution_report(rep, circ.domain)
        assert_same_powers(new, want)
    return new


def _powers_call(bn, powers, secrets, outs, rep):
    from wasmsnark_amd.bn128 import _powers_struct
    p, keep = _powers_struct(powers)
    return bn.lib.c.wsnark_powers_contribute(C.byref(p), *secrets, *outs, C.byref(rep))


def check_contribution_in_place(bn, log_domain):
    """Every output pointer equal to its input: the same bytes"""
    from wasmsnark_amd.bn128 import _PowersReport
    circ, S, powers = transcript(bn, log_domain)
    want = synth.powers_from_toxic(synth.contributed_toxic(S, T_FIXED, A_FIXED, B_FIXED), circ.domain, bn.mul_base)
    mine = {k: (bytearray(v) if k != "domain" else v) for k, v in powers.items()}
    bufs = [(C.c_uint8 * len(mine[k])).from_buffer(mine[k]) for k in ARRAYS + ("beta_g2",)]
    rep = _PowersReport()
    assert _powers_call(bn, mine, [le(T_FIXED), le(A_FIXED), le(B_FIXED)], bufs, rep) == 0 and rep.ok == 1
    assert_same_powers(mine, want)


def check_contribution_twice(bn, log_domain):
    """Two contributions in a row equal one by the products"""
    circ, S, powers = transcript(bn, log_domain)
    t2, a2, b2 = 0xABCDEF0123456789 << 100, R - 2, 3
    first, rep = bn.contribute_powers(powers, T_FIXED, A_FIXED, B_FIXED)
    second, rep2 = bn.contribute_powers(first, t2, a2, b2)
    both, rep3 = bn.contribute_powers(powers, T_FIXED * t2 % R, A_FIXED * a2 % R, B_FIXED * b2 % R)
    assert rep["ok"] and rep2["ok"] and rep3["ok"]
    assert_same_powers(second, both)
    # 32 bytes plain LE at or above r are reduced
    again, _ = bn.contribute_powers(powers, le(T_FIXED + R), le(A_FIXED), le(B_FIXED))
    assert_same_powers(again, first)


def check_contribution_drawn_secrets(bn, log_domain):
    """NULL secrets are drawn from the OS: the result is a transcript (check_powers) and differs from the input and from a second draw"""
    circ, S, powers = transcript(bn, log_domain)
    one, rep = bn.contribute_powers(powers)
    two, rep2 = bn.contribute_powers(powers)
    assert rep["ok"] and rep2["ok"]
    for name in ARRAYS:
        skip = (128 if name == "tau_g2" else 64) if name.startswith("tau") else 0      # tau_g1[0], tau_g2[0] stay the generators
        assert one[name][skip:] != powers[name][skip:] and one[name][skip:] != two[name][skip:] and one[name][:skip] == powers[name][:skip]
    assert one["beta_g2"] != powers["beta_g2"]
    chk = bn.check_powers(one)
    assert chk["ok"] is True and chk["relations_run"] == 63, chk


def check_contribution_zero_secret(bn, log_domain):
    from wasmsnark_amd._lib import WsnarkError
    circ, S, powers = transcript(bn, log_domain)
    for secrets in ((0, 5, 5), (5, R, 5), (5, 5, le(R)), (le(0), 5, 5)):
        try:
            bn.contribute_powers(powers, *secrets)
            raise AssertionError("a zero secret was accepted")
        except WsnarkError as e:
            assert e.code == ERR_ARG and "0 mod r" in str(e), str(e)


_PLANT_AS = {"tau_g1": "A", "alpha_tau_g1": "A", "beta_tau_g1": "A", "tau_g2": "B2"}      # pkey_check_common.plant's section names


def _plant(powers, name, index, what):
    sec = {pk.SEC_KEY[_PLANT_AS[name]]: powers[name]}
    pk.plant(sec, _PLANT_AS[name], index, what)


def check_contribution_bad_powers(bn, log_domain):
    """The plan of pkey_setup_common.check_setup_bad_powers: an unreduced and an off-curve point at index 1, the last index, both
    sides of every 64 / 256 boundary the array has and (tau_g1) of the boundary between its halves, in each array: counts, first index
    and reason by the Python classifier.  A planted infinity, in either encoding, is counted and gives ok False."""
    circ, S, powers = transcript(bn, log_domain)
    n = circ.domain
    for name in ARRAYS:
        size = 128 if name == "tau_g2" else 64
        count = len(powers[name]) // size
        spots = [1, count - 1] + [i for b in (64, 256, n) if b < count for i in (b - 1, b)]
        plans = [[(i, (pk.UNREDUCED, pk.OFF_CURVE)[k % 2])] for k, i in enumerate(spots)]
        plans.append([(i, (pk.OFF_CURVE, pk.UNREDUCED)[k % 2]) for k, i in enumerate(sorted(set(spots), reverse=True))])
        for plants in plans:
            bad = dict(powers)
            bad[name] = bytearray(powers[name])
            for i, what in plants:
                _plant(bad, name, i, what)
            new, rep = bn.contribute_powers(bad, T_FIXED, A_FIXED, B_FIXED)
            idx = sorted(set(i for i, _ in plants))
            inf, nbad, first, reason = pk.expected_section(bad[name], size, indices=idx)
            assert new is None and rep["ok"] is False
            assert rep[name] == {"points": count, "infinity": 0, "bad": nbad, "first_bad": first, "first_reason": reason}, (name, plants, rep[name])
            assert nbad == len(idx) and first == idx[0] and inf == 0
            for other in ARRAYS:
                assert other == name or rep[other]["bad"] == 0
        for enc in (bytes(size), inf9(size // 64)):
            bad = dict(powers)
            bad[name] = bytearray(powers[name])
            bad[name][size * (count - 2):size * (count - 1)] = enc
            new, rep = bn.contribute_powers(bad, T_FIXED, A_FIXED, B_FIXED)
            assert new is None and rep["ok"] is False
            assert rep[name] == {"points": count, "infinity": 1, "bad": 0, "first_bad": None, "first_reason": None}, (name, rep[name])
    # a beta_g2 off its curve
    bad = dict(powers, beta_g2=bytearray(powers["beta_g2"]))
    bad["beta_g2"][64] ^= 1
    new, rep = bn.contribute_powers(bad, T_FIXED, A_FIXED, B_FIXED)
    assert new is None and rep["ok"] is False and rep["beta_g2"] == pk.OFF_CURVE and rep["tau_g1"]["bad"] == 0


def check_powers_errors(bn, log_domain):
    """What the loaders reject fails with the loader's code, a pre-filled report and the output buffers untouched -- for the
    contribution and for the audit."""
    from wasmsnark_amd.bn128 import _PowersReport, _powers_struct
    circ, S, powers = transcript(bn, log_domain)
    n = circ.domain
    c = bn.lib.c
    untouched = bytes(pd._raw(_PowersReport))
    bufs = [(C.c_uint8 * sz)() for sz in (128 * n, 128 * n, 64 * n, 64 * n, 128)]
    secrets = [le(T_FIXED), le(A_FIXED), le(B_FIXED)]

    def call(p):
        rep = pd._raw(_PowersReport)
        rc = _powers_call(bn, p, secrets, bufs, rep)
        ps_, keep = _powers_struct(p)
        rep2 = pd._raw(_PowersReport)
        rc2 = c.wsnark_powers_check(C.byref(ps_), 0, None, C.byref(rep2))
        assert bytes(rep) == bytes(rep2) == untouched and all(not any(b) for b in bufs)
        assert rc == rc2
        return rc

    for name in ARRAYS:      # a short array
        assert call(dict(powers, **{name: powers[name][:-64]})) == ERR_FORMAT, name
    assert call(dict(powers, tau_g1=powers["tau_g1"][:64 * n])) == ERR_FORMAT      # n entries where 2n are needed
    assert call(dict(powers, domain=48)) == ERR_SIZE                              # not a power of two
    assert call(dict(powers, domain=1)) == ERR_SIZE
    assert call(dict(powers, domain=1 << 25)) == ERR_SIZE                         # > 2^24
    # NULL pointers
    p, keep = _powers_struct(powers)
    rep = pd._raw(_PowersReport)
    for k in range(5):
        outs = list(bufs)
        outs[k] = None
        assert c.wsnark_powers_contribute(C.byref(p), *secrets, *outs, C.byref(rep)) == ERR_ARG
    assert c.wsnark_powers_contribute(None, *secrets, *bufs, C.byref(rep)) == ERR_ARG
    assert c.wsnark_powers_contribute(C.byref(p), *secrets, *bufs, None) == ERR_ARG
    assert c.wsnark_powers_check(None, 0, None, C.byref(rep)) == ERR_ARG and c.wsnark_powers_check(C.byref(p), 0, None, None) == ERR_ARG
    assert c.wsnark_powers_check(C.byref(p), 4, None, C.byref(rep)) == ERR_ARG      # an unknown flag
    p.tau_g2 = None
    assert c.wsnark_powers_contribute(C.byref(p), *secrets, *bufs, C.byref(rep)) == ERR_ARG
    assert bytes(rep) == untouched and all(not any(b) for b in bufs)


def check_chain(bn, log_domain):
    """The contributed transcript passes the audit, and setup_key on it is the closed form of the contributed toxic waste under
    delta = gamma = 1."""
    circ, S, powers = transcript(bn, log_domain)
    new, rep = bn.contribute_powers(powers, T_FIXED, A_FIXED, B_FIXED)
    assert rep["ok"] is True
    chk = bn.check_powers(new)
    assert chk["ok"] is True and chk["relations_run"] == 63 and chk["relations_bad"] == 0, chk
    key, (ic, gamma2), rep2 = bn.setup_key(new, synth.circuit_blobs(circ))
    assert rep2["ok"] is True
    S2 = ps.delta_gamma_one(synth.contributed_toxic(S, T_FIXED, A_FIXED, B_FIXED, circ))
    want, (want_ic, _) = synth.build_sections(circ, S2, bn.mul_base)
    pd.assert_same_key(key, want)
    assert ic == want_ic


# ---- 3. the audit ----
TAU2 = 0x5EC0DD7A05EC0DD7A05EC0DD7A0 % R          # a second tau
BETA2 = 0xBE7A2BE7A2BE7A2 % R                     # a second beta


def logs_of(S, n):
    """The logarithms synth.powers_from_toxic writes a transcript down from"""
    tp = [pow(S.tau, k, R) for k in range(2 * n)]
    return {"tau_g1": tp, "tau_g2": tp[:n], "alpha_tau_g1": [S.alpha * t % R for t in tp[:n]], "beta_tau_g1": [S.beta * t % R for t in tp[:n]],
            "beta_g2": S.beta}


def powers_of_logs(bn, n, L):
    return {"domain": n, "tau_g1": ps.points_of_logs(bn, 1, L["tau_g1"]), "tau_g2": ps.points_of_logs(bn, 2, L["tau_g2"]),
            "alpha_tau_g1": ps.points_of_logs(bn, 1, L["alpha_tau_g1"]), "beta_tau_g1": ps.points_of_logs(bn, 1, L["beta_tau_g1"]),
            "beta_g2": ps.points_of_logs(bn, 2, [L["beta_g2"]])}


def relations_expected(L):
    """relations_bad from the logarithms alone: a relation of the header holds (for every rho but 2^-128 of them) iff it holds term
    by term.  With T = the logarithm of tau_g2[1]:
      bit 0: l1[0] == 1 and l2[0] == 1;  bit 1: l1[k + 1] == T l1[k];  bit 2: l2[k + 1] == l1[1] l2[k];
      bit 3, 4: la[k + 1] == T la[k], lb[k + 1] == T lb[k];  bit 5: lb[0] == the logarithm of beta_g2."""
    l1, l2, la, lb = L["tau_g1"], L["tau_g2"], L["alpha_tau_g1"], L["beta_tau_g1"]
    T = l2[1]
    chain = lambda v, f: all(v[k + 1] % R == f * v[k] % R for k in range(len(v) - 1))
    bad = 0 if l1[0] == 1 and l2[0] == 1 else 1
    bad |= 0 if chain(l1, T) else 2
    bad |= 0 if chain(l2, l1[1]) else 4
    bad |= 0 if chain(la, T) else 8
    bad |= 0 if chain(lb, T) else 16
    bad |= 0 if lb[0] % R == L["beta_g2"] % R else 32
    return bad


def relation_cases(S, n):
    """(name, logarithms, relations_bad) of the spoilt transcripts.  Every replacement is another multiple of the generator: on the
    curve, in the subgroup, invisible to the point tests.  The literals, worked out by hand from the six relations:
      tau_g1[k] replaced, k = n and k = 2n - 1: only tau_g1's own chain names these entries: bit 1 -> 2.
      tau_g1[1] replaced: bit 1 (terms k = 0 and k = 1), and bit 2, whose G1 argument IS tau_g1[1] -> 2 | 4 = 6.
      tau_g1[5] and [6] swapped: bit 1 -> 2.      tau_g1's upper half from a second tau: the chain breaks at k = n - 1 -> 2.
      tau_g2[3] replaced: only tau_g2's own chain (T2 is entry 1, untouched) -> 4.
      tau_g2 from a second tau: T2 = tau' G2 now.  Bit 1: tau_g1 still steps by tau, not tau' -> bad.  Bit 2: tau_g1[1] = tau G1 but
        tau_g2 steps by tau' -> bad.  Bits 3 and 4 step by tau against T2 = tau' as well -> 2 | 4 | 8 | 16 = 30: every chain hangs on T2.
      alpha_tau_g1[2] replaced -> 8.      beta_tau_g1[2] replaced -> 16.      beta_tau_g1[0] replaced: its chain AND bit 5 -> 16 | 32 = 48.
      beta_g2 from a second beta -> 32.
      tau_g1[0] = 2G: bit 0, and bit 1's term k = 0 (tau_g1[1] = tau G1 is not tau x 2G) -> 1 | 2 = 3.
      alpha_tau_g1 scaled as a whole by one constant: a valid transcript under another alpha -> 0, and ok."""
    base = logs_of(S, n)

    def edit(f):
        L = {k: (list(v) if isinstance(v, list) else v) for k, v in base.items()}
        f(L)
        return L

    def put(name, k, v):
        return lambda L: L[name].__setitem__(k, v)

    def swap(L):
        L["tau_g1"][5], L["tau_g1"][6] = L["tau_g1"][6], L["tau_g1"][5]

    def upper(L):
        L["tau_g1"][n:] = [pow(TAU2, k, R) for k in range(n, 2 * n)]

    def second_tau2(L):
        L["tau_g2"] = [pow(TAU2, k, R) for k in range(n)]

    def scaled(L):
        L["alpha_tau_g1"] = [v * 0xC0FFEE % R for v in L["alpha_tau_g1"]]

    return [("tau_g1[1]", edit(put("tau_g1", 1, 0xD00D)), 6), ("tau_g1[n]", edit(put("tau_g1", n, 0xD00D)), 2),
            ("tau_g1[2n-1]", edit(put("tau_g1", 2 * n - 1, 0xD00D)), 2), ("swap", edit(swap), 2), ("upper half", edit(upper), 2),
            ("tau_g2[3]", edit(put("tau_g2", 3, 0xD00D)), 4), ("second tau in G2", edit(second_tau2), 30),
            ("alpha_tau_g1[2]", edit(put("alpha_tau_g1", 2, 0xD00D)), 8), ("beta_tau_g1[2]", edit(put("beta_tau_g1", 2, 0xD00D)), 16),
            ("beta_tau_g1[0]", edit(put("beta_tau_g1", 0, 0xD00D)), 48), ("beta_g2", edit(lambda L: L.__setitem__("beta_g2", BETA2)), 32),
            ("tau_g1[0] = 2G", edit(put("tau_g1", 0, 2)), 3), ("alpha scaled", edit(scaled), 0)]


def check_audit_good(bn, log_domain):
    circ, S, powers = transcript(bn, log_domain)
    n = circ.domain
    rep = bn.check_powers(powers)
    assert rep["ok"] is True and rep["relations_run"] == 63 and rep["relations_bad"] == 0 and rep["beta_g2"] is None, rep
    assert all(v is True for v in rep["relations"].values())
    for name in ARRAYS:
        assert rep[name] == {"points": n * (2 if name == "tau_g1" else 1), "infinity": 0, "bad": 0, "first_bad": None, "first_reason": None}
    assert set(rep["ms"]) == {"points", "relation_sums", "pairings", "total"}
    assert relations_expected(logs_of(S, n)) == 0


def check_audit_relations(bn, log_domain, points):
    """One spoilt transcript per case of relation_cases: relations_bad is the case's literal and what the logarithms say; every
    relation ran; ok only for the rescaled alpha array."""
    circ, S, _ = transcript(bn, log_domain)
    n = circ.domain
    for name, L, want in relation_cases(S, n):
        assert relations_expected(L) == want, (name, relations_expected(L), want)
        rep = bn.check_powers(powers_of_logs(bn, n, L), points=points)
        assert rep["relations_run"] == 63 and rep["relations_bad"] == want, (name, rep["relations_bad"], want)
        assert rep["ok"] is (want == 0), name
        assert all(rep[a]["bad"] == 0 and rep[a]["infinity"] == 0 for a in ARRAYS)


def check_audit_chunk_overlap(bn, tune, log_domain, points):
    """PWTAU_CHUNK = 64: a replaced power exactly at index 64 (the k + 1 of chunk 0's last term and the k of chunk 1's first) and at
    index 63, in tau_g1 -> bit 1 alone; the good transcript still passes with the chunks in place."""
    circ, S, powers = transcript(bn, log_domain)
    n = circ.domain
    assert 2 * n > 64
    tune(bn.lib, "PWTAU_CHUNK", 64)
    rep = bn.check_powers(powers, points=points)
    assert rep["ok"] is True and rep["relations_run"] == 63, rep
    for k in (64, 63):
        L = logs_of(S, n)
        L["tau_g1"][k] = 0xD00D
        assert relations_expected(L) == 2
        rep = bn.check_powers(powers_of_logs(bn, n, L), points=points)
        assert rep["relations_run"] == 63 and rep["relations_bad"] == 2 and rep["ok"] is False, (k, rep)
        # ... and a term the two neighbours hide from each other: entry k times c and entry k + 1 times c leave term k alone, but not
        # the terms k - 1 and k + 1
        L = logs_of(S, n)
        L["tau_g1"][k] = L["tau_g1"][k] * 3 % R
        L["tau_g1"][k + 1] = L["tau_g1"][k + 1] * 3 % R
        rep = bn.check_powers(powers_of_logs(bn, n, L), points=points)
        assert rep["relations_bad"] == 2 == relations_expected(L), (k, rep)


def check_audit_outside_subgroup(bn, log_domain):
    """A tau_g2 point outside the order-r subgroup: counted with reason outside_subgroup; bit 2 is not run; ok False"""
    circ, S, powers = transcript(bn, log_domain)
    bad = dict(powers, tau_g2=bytearray(powers["tau_g2"]))
    _plant(bad, "tau_g2", 3, pk.OUTSIDE)
    rep = bn.check_powers(bad)
    assert rep["tau_g2"] == {"points": circ.domain, "infinity": 0, "bad": 1, "first_bad": 3, "first_reason": pk.OUTSIDE}, rep["tau_g2"]
    assert rep["relations_run"] == 63 & ~4 and rep["relations"]["tau_g2"] is None and rep["relations_bad"] == 0 and rep["ok"] is False, rep
    # an off-curve alpha power and an infinity in beta_tau_g1: counted, their own bits not run
    bad = dict(powers, alpha_tau_g1=bytearray(powers["alpha_tau_g1"]), beta_tau_g1=bytearray(powers["beta_tau_g1"]))
    _plant(bad, "alpha_tau_g1", circ.domain - 1, pk.OFF_CURVE)
    bad["beta_tau_g1"][64 * 2:64 * 3] = inf9(1)
    rep = bn.check_powers(bad)
    assert (rep["alpha_tau_g1"]["bad"], rep["alpha_tau_g1"]["first_bad"], rep["alpha_tau_g1"]["first_reason"]) == (1, circ.domain - 1, pk.OFF_CURVE)
    assert rep["beta_tau_g1"]["infinity"] == 1 and rep["beta_tau_g1"]["bad"] == 0
    assert rep["relations_run"] == 63 & ~(8 | 16) and rep["relations_bad"] == 0 and rep["ok"] is False, rep


def check_audit_seed_and_halves(bn, log_domain):
    """A fixed seed gives the same report twice and seed=None works; points=False and relations=False each run only their half"""
    circ, S, powers = transcript(bn, log_domain)
    L = logs_of(S, circ.domain)
    L["alpha_tau_g1"][2] = 0xD00D
    spoilt = powers_of_logs(bn, circ.domain, L)
    seed = bytes(range(32))
    a, b = bn.check_powers(spoilt, seed=seed, points=False), bn.check_powers(spoilt, seed=seed, points=False)
    assert pd.no_ms(a) == pd.no_ms(b) and a["relations_bad"] == 8
    assert bn.check_powers(spoilt, seed=None, points=False)["relations_bad"] == 8
    # relations only
    rep = bn.check_powers(powers, points=False)
    assert rep["ok"] is True and rep["relations_run"] == 63 and rep["ms"]["relation_sums"] > 0
    # points only: the spoilt relation goes unseen, nothing of the relations runs
    rep = bn.check_powers(spoilt, relations=False)
    assert rep["ok"] is True and rep["relations_run"] == 0 and rep["relations_bad"] == 0 and rep["ms"]["relation_sums"] == 0
    assert all(v is None for v in rep["relations"].values())
    bad = dict(powers, tau_g1=bytearray(powers["tau_g1"]))
    _plant(bad, "tau_g1", 7, pk.UNREDUCED)
    rep = bn.check_powers(bad, relations=False)
    assert rep["ok"] is False and (rep["tau_g1"]["bad"], rep["tau_g1"]["first_bad"], rep["tau_g1"]["first_reason"]) == (1, 7, pk.UNREDUCED)
    # beta_g2 off its curve: named, bit 5 not run
    bad = dict(powers, beta_g2=bytearray(powers["beta_g2"]))
    bad["beta_g2"][64] ^= 1
    rep = bn.check_powers(bad)
    assert rep["beta_g2"] == pk.OFF_CURVE and rep["relations_run"] == 31 and rep["ok"] is False
