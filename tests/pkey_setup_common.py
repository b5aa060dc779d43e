"""Shared checks of the key setup from powers of tau (wsnark_g{1,2}_ntt, wsnark_pkey_setup*, csrc/pkeysetup.hip), run by
tests/test_emul_pkey_setup.py on the thread-emulator build of the kernel sources and by tests/test_gpu_pkey_setup.py on the device.

The yardstick is never the code under test.  The group transform is compared (a) at tiny sizes with its definition, sum_k w^(ik) P_k,
in affine Python integers (bn128_ref), and (b) at every size with the transform of the points' LOGARITHMS done in Python integers,
carried back to the group by mul_base -- an independent kernel that the parity tests pin.  A new key is compared byte for byte with
the closed form: the synthetic key built from the toxic waste with delta = gamma = 1 (synth.build_sections).  Bad powers are counted
by the audit's pure-Python classifier (pkey_check_common)."""
import ctypes as C
import copy
import random
import subprocess
import sys

import pkey_check_common as pk
import pkey_delta_common as pd
from bn128_ref import Q, R, g1_add, g1_mul, g2_add, g2_mul, le, mont
from pkey_check_common import ERR_ARG, ERR_FORMAT, ERR_NOINIT, ERR_SIZE
from wasmsnark_amd import synth


# ---- the yardstick of the transform: Python integers ----
def ntt_direct(s, inverse):
    """The definition: out[i] = sum_k w_n^(+-ik) s[k] (times 1/n for the inverse), w_n the root wsnark_fr_ntt uses."""
    n = len(s)
    w = synth.root_of_unity(n.bit_length() - 1) if n > 1 else 1
    if inverse:
        w = pow(w, -1, R)
    pw = [pow(w, e, R) for e in range(n)]
    out = [sum(pw[i * k % n] * s[k] for k in range(n)) % R for i in range(n)]
    return [x * pow(n, -1, R) % R for x in out] if inverse else out


def _ntt_rec(s, w):
    n = len(s)
    if n == 1:
        return list(s)
    e, o = _ntt_rec(s[0::2], w * w % R), _ntt_rec(s[1::2], w * w % R)
    out, t = [0] * n, 1
    for j in range(n // 2):
        x = t * o[j] % R
        out[j], out[j + n // 2] = (e[j] + x) % R, (e[j] - x) % R
        t = t * w % R
    return out


_ntt_memo = {}


def ntt_logs(s, inverse):
    """The same values as ntt_direct by the radix-2 recursion (exact integers; check_python_transforms_agree holds the two
    together), computed once per input."""
    key = (tuple(s), bool(inverse))
    if key not in _ntt_memo:
        n = len(s)
        w = synth.root_of_unity(n.bit_length() - 1) if n > 1 else 1
        out = _ntt_rec(list(s), pow(w, -1, R) if inverse else w)
        _ntt_memo[key] = [x * pow(n, -1, R) % R for x in out] if inverse else out
    return _ntt_memo[key]


def check_python_transforms_agree():
    rnd = random.Random(11)
    for bits in range(0, 6):
        s = [rnd.randrange(R) for _ in range(1 << bits)]
        for inv in (False, True):
            assert ntt_logs(s, inv) == ntt_direct(s, inv)


def points_of_logs(bn, g, logs):
    """s_k G through mul_base; log 0 is infinity: zero bytes"""
    sz = 64 if g == 1 else 128
    pts = bn.mul_base(g, b"".join(le(v % R) for v in logs))
    return b"".join(bytes(sz) if logs[i] % R == 0 else pts[sz * i:sz * i + sz] for i in range(len(logs)))


def differing(g, got, want):
    sz = 64 if g == 1 else 128
    return [i for i in range(len(want) // sz) if got[sz * i:sz * i + sz] != want[sz * i:sz * i + sz]][:8]


def logs_for(bits, seed=5):
    """2^bits logarithms: random, a few zero (infinity inputs), a repeated value"""
    rnd = random.Random(seed * 100 + bits)
    s = [rnd.randrange(1, R) for _ in range(1 << bits)]
    for i in range(3, len(s), 17):
        s[i] = 0
    if len(s) >= 8:
        s[5] = s[4]
    return s


# ---- 1. the transform ----
def check_ntt_definition(bn, g):
    """n = 1, 2, 4, 8 against sum_k w^(ik) P_k in affine integers"""
    add, mul = (g1_add, g1_mul) if g == 1 else (g2_add, g2_mul)
    for bits in range(0, 4):
        n = 1 << bits
        logs = [(7 * k + 3) * pow(5, k, R) % R for k in range(n)]
        if n == 8:
            logs[6] = 0
        data = points_of_logs(bn, g, logs)
        sz = len(data) // n
        P = [pd.point_from_bytes(g, data[sz * k:sz * k + sz]) for k in range(n)]
        for inverse in (False, True):
            w = synth.root_of_unity(bits) if n > 1 else 1
            if inverse:
                w = pow(w, -1, R)
            want = b""
            for i in range(n):
                acc = None
                for k in range(n):
                    f = pow(w, i * k, R) * (pow(n, -1, R) if inverse else 1) % R
                    acc = add(acc, mul(P[k], f) if P[k] is not None else None)
                want += pd.point_to_bytes(g, acc)
            got = bn.group_ntt(g, data, inverse)
            assert got == want, (g, n, inverse, differing(g, got, want))


def check_ntt_sizes(bn, g, max_bits):
    """Every size 2^0 .. 2^max_bits, both directions: the bytes are mul_base(NTT(logs)); the Fr transform of the same logs agrees."""
    for bits in range(0, max_bits + 1):
        logs = logs_for(bits)
        data = points_of_logs(bn, g, logs)
        for inverse in (False, True):
            t = ntt_logs(logs, inverse)
            want = points_of_logs(bn, g, t)
            got = bn.group_ntt(g, data, inverse)
            assert got == want, (g, bits, inverse, differing(g, got, want))


def check_ntt_agrees_with_fr(bn, bits):
    """wsnark_fr_ntt(odd = 0) on the logarithms gives the logarithms of wsnark_g1_ntt's points: one convention for both."""
    logs = logs_for(bits, seed=8)
    data = points_of_logs(bn, 1, logs)
    for inverse in (False, True):
        fr = bn.fromMontgomeryN(bn.fft(bn.toMontgomeryN(b"".join(le(v) for v in logs)), 0, inverse))
        fr_logs = [int.from_bytes(fr[32 * i:32 * i + 32], "little") for i in range(len(logs))]
        assert fr_logs == ntt_logs(logs, inverse)
        assert bn.group_ntt(1, data, inverse) == points_of_logs(bn, 1, fr_logs)


def cancelling_logs(bits, sub_bits, seed=21):
    """Logarithms for which the stage of span 2^sub_bits meets P = -w Q in one butterfly and P = +w Q in another: the size-2^sub_bits
    transform of the stride class c = 1 (elements 1 + k n/2^sub_bits: what that stage finishes) has a zero at index j0 (< half: the
    P + T half) and at index half + j1 (the P - T half).  Returns (logs, that sub-transform)."""
    rnd = random.Random(seed + bits)
    n, m2 = 1 << bits, 1 << sub_bits
    s = [rnd.randrange(1, R) for _ in range(n)]
    V = [rnd.randrange(1, R) for _ in range(m2)]
    V[3] = 0
    V[m2 // 2 + 1] = 0
    v = ntt_logs(V, True)
    stride = n // m2
    for k in range(m2):
        s[1 + k * stride] = v[k]
    return s, V


def check_ntt_corners(bn, g, bits):
    sz = 64 if g == 1 else 128
    n = 1 << bits
    one = points_of_logs(bn, g, [0xC0FFEE])
    inf9 = bytes(sz // 2) + bytes([9]) + bytes(sz // 2 - 1)      # infinity by the loaders' rule, with a non-zero y
    # all points equal: every first-stage butterfly is a doubling and a cancellation
    got = bn.group_ntt(g, one * n, False)
    assert got == points_of_logs(bn, g, [0xC0FFEE * n % R] + [0] * (n - 1))
    assert bn.group_ntt(g, one * n, True) == one + bytes(sz * (n - 1))
    # a single finite point among infinities (both encodings): all copies, times powers of w
    for pos in (0, 5, n - 1):
        logs = [0] * n
        logs[pos] = 0xC0FFEE
        data = bytearray(points_of_logs(bn, g, logs))
        data[sz * ((pos + 1) % n):sz * ((pos + 1) % n) + sz] = inf9
        for inverse in (False, True):
            got = bn.group_ntt(g, data, inverse)
            want = points_of_logs(bn, g, ntt_logs(logs, inverse))
            assert got == want, (g, bits, pos, inverse, differing(g, got, want))
    # all infinity
    assert bn.group_ntt(g, bytes(sz * n), False) == bytes(sz * n) == bn.group_ntt(g, inf9 * n, True)
    # P = -w Q and P = +w Q in a middle stage
    sub_bits = bits // 2 + 1
    logs, V = cancelling_logs(bits, sub_bits)
    stride = n >> sub_bits
    assert ntt_direct([logs[1 + k * stride] for k in range(1 << sub_bits)], False) == V and V.count(0) == 2 and 1 < sub_bits < bits
    got = bn.group_ntt(g, points_of_logs(bn, g, logs), False)
    want = points_of_logs(bn, g, ntt_logs(logs, False))
    assert got == want, (g, bits, differing(g, got, want))


def check_ntt_round_trip(bn, g, bits):
    data = points_of_logs(bn, g, logs_for(bits, seed=9))
    for first in (False, True):
        assert bn.group_ntt(g, bn.group_ntt(g, data, first), not first) == data


def check_ntt_errors(bn, so_path):
    from wasmsnark_amd._lib import WsnarkError
    c = bn.lib.c
    pts = bytearray(points_of_logs(bn, 1, list(range(1, 129))))
    out = (C.c_uint8 * len(pts))()
    buf = (C.c_uint8 * len(pts)).from_buffer(pts)
    for fn, per in ((c.wsnark_g1_ntt, 64), (c.wsnark_g2_ntt, 128)):
        for n in (0, 3, 1 << 25, (1 << 24) + 1, 96):
            assert fn(buf, n, 0, out) == ERR_SIZE, n
        assert fn(None, 4, 0, out) == ERR_ARG and fn(buf, 4, 1, None) == ERR_ARG
    assert not any(out)
    for index in (0, 66, 127):
        bad = bytearray(pts)
        bad[64 * index + 32] ^= 1
        try:
            bn.group_ntt(1, bad, False)
            raise AssertionError("an off-curve point was transformed")
        except WsnarkError as e:
            assert e.code == ERR_FORMAT and "index %d" % index in str(e), str(e)
    bad = bytearray(pts)
    bad[64 * 9:64 * 9 + 32] = le(int.from_bytes(pts[64 * 9:64 * 9 + 32], "little") + Q)      # unreduced
    bad[64 * 70 + 32] ^= 1
    try:
        bn.group_ntt(1, bad, True)
        raise AssertionError("an unreduced point was transformed")
    except WsnarkError as e:
        assert e.code == ERR_FORMAT and "index 9" in str(e) and "2 point(s)" in str(e), str(e)
    # before wsnark_init: a fresh process that loads the library and never initialises it
    code = ("import ctypes as C, sys\n"
            "c = C.CDLL(sys.argv[1])\n"
            "vp = C.c_void_p\n"
            "c.wsnark_g1_ntt.argtypes = c.wsnark_g2_ntt.argtypes = [vp, C.c_uint64, C.c_int, vp]\n"
            "k, o = bytes(256), (C.c_uint8 * 256)(*([90] * 256))\n"
            "print(c.wsnark_g1_ntt(k, 2, 0, o), c.wsnark_g2_ntt(k, 2, 1, o), set(o))\n")
    res = subprocess.run([sys.executable, "-c", code, so_path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == [str(ERR_NOINIT)] * 2 + ["{90}"], (res.stdout, res.stderr)


# ---- 2. the setup: the closed form ----
def no_ms(d):
    return {k: v for k, v in d.items() if k != "ms"}


def delta_gamma_one(S):
    S1 = copy.copy(S)
    S1.delta = S1.gamma = 1
    return S1


_inputs_memo = {}


def setup_inputs(bn, log_domain, style, seed=3):
    """(circuit, toxic waste, powers, circuit blobs, the closed form under delta = gamma = 1: (sections, (IC, gamma2))), built once"""
    key = (id(bn), log_domain, style, seed)
    if key not in _inputs_memo:
        circ = synth.make_circuit(log_domain, n_public=2, seed=seed, style=style)
        S = synth.setup(circ, seed=seed + 50)
        _inputs_memo[key] = (circ, S, synth.powers_from_toxic(S, circ.domain, bn.mul_base), synth.circuit_blobs(circ),
                             synth.build_sections(circ, delta_gamma_one(S), bn.mul_base))
    return _inputs_memo[key]


def assert_good_report(rep, domain):
    assert rep["ok"] is True and rep["beta_g2"] is None
    for name in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1"):
        assert rep[name] == {"points": domain * (2 if name == "tau_g1" else 1), "infinity": 0, "bad": 0, "first_bad": None, "first_reason": None}
    assert set(rep["ms"]) == {"transforms", "column_sums", "hexps", "total"} and rep["ms"]["total"] >= rep["ms"]["transforms"] > 0


def check_setup_closed_form(bn, tune, log_domain, style, msm_mins=(None, 1 << 20)):
    """setup_key == synth.build_sections under delta = gamma = 1, byte for byte: five sections, five fixed points, both record streams,
    IC; both output forms; the same bytes for every PKSETUP_MSM_MIN of msm_mins (None: the default)."""
    circ, S, powers, blobs, (want, (ic, gamma2)) = setup_inputs(bn, log_domain, style)
    if style == "rows":
        assert len(pk.finite_indices(want, "A")) < circ.n_vars and len(pk.finite_indices(want, "B2")) < circ.n_vars      # infinity points
    columns = []
    for mm in msm_mins:
        if mm is None:
            bn.lib.tune("PKSETUP_MSM_MIN", None)
        else:
            tune(bn.lib, "PKSETUP_MSM_MIN", mm)
        key, vk_parts, rep = bn.setup_key(powers, blobs)
        assert_good_report(rep, circ.domain)
        pd.assert_same_key(key, want)
        assert set(key) == set(want)
        assert vk_parts == (ic, gamma2)
        columns.append(rep["msm_columns"])
    longest = max(len(a) + len(b) + len(c) for a, b, c in zip(circ.A, circ.B, circ.C))
    for mm, got in zip(msm_mins, columns):
        if mm is not None and mm >= longest:
            assert got == 0
        if mm == 2:
            assert got > 0
    pkey, vk_parts, rep = bn.setup_key(powers, blobs, pkey=True)
    assert pkey == synth.sections_to_pkey(want) and vk_parts == (ic, gamma2) and rep["ok"] is True
    return key


def _records_blob(cols):
    """the record streams' format from per-signal LISTS of (index, coefficient): indices may repeat, coefficients may be zero"""
    import struct
    out = bytearray()
    for col in cols:
        out += struct.pack("<I", len(col))
        for idx, coef in col:
            out += struct.pack("<I", idx) + le(coef * synth.MONT % R)
    return bytes(out)


def fat_column(col, domain, records, rnd):
    """The same column as `records` or more records: every coefficient split into parts that add up to it, pairs that cancel on
    other rows, and zero coefficients."""
    out = []
    for idx, coef in col.items():
        parts = [rnd.randrange(R) for _ in range(3)]
        out += [(idx, p) for p in parts] + [(idx, (coef - sum(parts)) % R)]
    while len(out) < records:
        idx, x = rnd.randrange(domain), rnd.randrange(1, R)
        out += [(idx, x), (rnd.randrange(domain), 0), (idx, R - x)]
    rnd.shuffle(out)
    return out


def check_setup_long_column(bn, tune, log_domain, records=300):
    """Signal 0 with >= 300 records in A and in B (repeated indices, zeros): by default such a column goes through the MSM, with the
    switch off a lane walks it; the points are those of the plain circuit either way.  Bytes only: the streams in the key are the
    fat ones."""
    circ, S, powers, blobs, (want, (ic, gamma2)) = setup_inputs(bn, log_domain, "columns")
    rnd = random.Random(77)
    fat = dict(blobs)
    for name, cols in (("polsA", circ.A), ("polsB", circ.B)):
        lists = [list(c.items()) for c in cols]
        lists[0] = fat_column(cols[0], circ.domain, records, rnd)
        assert len(lists[0]) >= records
        fat[name] = _records_blob(lists)
    assert _records_blob([list(c.items()) for c in circ.A]) == blobs["polsA"]
    want = dict(want, polsA=fat["polsA"], polsB=fat["polsB"])
    for mm, columns in ((None, 4), (0, 0)):      # A_0, B1_0, K_0 and B2_0
        if mm is None:
            bn.lib.tune("PKSETUP_MSM_MIN", None)
        else:
            tune(bn.lib, "PKSETUP_MSM_MIN", mm)
        key, vk_parts, rep = bn.setup_key(powers, fat)
        assert rep["ok"] is True and rep["msm_columns"] == columns
        pd.assert_same_key(key, want)
        assert vk_parts == (ic, gamma2)


# ---- 3. the chain to the existing features, and a proof ----
def check_setup_chain(bn, log_domain, style="columns"):
    circ, S, powers, blobs, _ = setup_inputs(bn, log_domain, style)
    new, (ic, gamma2), rep = bn.setup_key(powers, blobs)
    assert rep["ok"] is True
    assert bn.check_key(sections=new)["ok"] is True
    that, rep2 = bn.contribute_key(sections=new, d=S.delta)
    assert rep2["ok"] is True
    pd.assert_same_key(that, synth.build_sections(circ, S, bn.mul_base)[0])
    assert bn.verify_contribution(new, that)["ok"] is True


def check_setup_key_works(bn, log_domain):
    circ, S, powers, blobs, _ = setup_inputs(bn, log_domain, "columns")
    new, (ic, gamma2), rep = bn.setup_key(powers, blobs)
    wit, pub = synth.witness_bin(circ), synth.public_signals(circ)
    r, s = bytes([3]) * 32, bytes([5]) * 32
    proof = bn.groth16GenProof(wit, synth.sections_to_pkey(new), r=r, s=s)
    assert proof == synth.expected_proof(circ, delta_gamma_one(S), r, s, bn.mul_base)
    from wasmsnark_amd.bn128 import G2_GEN
    assert gamma2 == G2_GEN
    vk = synth.vk_from_points(circ.n_public, new, ic, gamma2)
    assert bn.groth16Verify(vk, pub, proof) is True
    swapped = [ic[1], ic[0]] + ic[2:]
    assert bn.groth16Verify(synth.vk_from_points(circ.n_public, new, swapped, gamma2), pub, proof) is False


# ---- 4. bad powers are a result ----
_PLANT_AS = {"tau_g1": "A", "alpha_tau_g1": "A", "beta_tau_g1": "A", "tau_g2": "B2"}      # pkey_check_common.plant's section names


def _plant(powers, name, index, what):
    sec = {pk.SEC_KEY[_PLANT_AS[name]]: powers[name]}
    pk.plant(sec, _PLANT_AS[name], index, what)


def check_setup_bad_powers(bn, log_domain):
    """An unreduced and an off-curve point at index 1, the last index, both sides of every 64 / 256 boundary the array has and (tau_g1)
    of the boundary between its two halves, in each of the four arrays: counts, first index and reason by the Python classifier."""
    circ, S, powers, blobs, _ = setup_inputs(bn, log_domain, "columns")
    n = circ.domain
    for name in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1"):
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
            key, vk_parts, rep = bn.setup_key(bad, blobs)
            idx = sorted(set(i for i, _ in plants))
            inf, nbad, first, reason = pk.expected_section(bad[name], size, indices=idx)
            assert key is None and vk_parts is None and rep["ok"] is False
            assert rep[name] == {"points": count, "infinity": 0, "bad": nbad, "first_bad": first, "first_reason": reason}, (name, plants, rep[name])
            assert nbad == len(idx) and first == idx[0] and inf == 0
            for other in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1"):
                assert other == name or rep[other]["bad"] == 0
    # a beta_g2 off its curve
    bad = dict(powers, beta_g2=bytearray(powers["beta_g2"]))
    bad["beta_g2"][64] ^= 1
    key, _, rep = bn.setup_key(bad, blobs)
    assert key is None and rep["ok"] is False and rep["beta_g2"] == pk.OFF_CURVE and rep["tau_g1"]["bad"] == 0


# ---- 5. errors ----
def check_setup_errors(bn, log_domain, so_path):
    """What the loaders reject fails with the loader's code, a pre-filled report and the output buffers untouched."""
    from wasmsnark_amd.bn128 import _SetupReport, _circuit_struct, _powers_struct
    circ, S, powers, blobs, _ = setup_inputs(bn, log_domain, "columns")
    c = bn.lib.c
    nv, npub, n = circ.n_vars, circ.n_public, circ.domain
    untouched = bytes(pd._raw(_SetupReport))
    sizes = (64 * nv, 64 * nv, 128 * nv, 64 * (nv - npub - 1), 64 * n, 64, 64, 64, 128, 128, 64 * (npub + 1))
    bufs = [(C.c_uint8 * sz)() for sz in sizes]
    big = (C.c_uint8 * (1 << 20))()

    def call(p, k):
        ps, keep_p = _powers_struct(p)
        cs, keep_c = _circuit_struct(k)
        rep = pd._raw(_SetupReport)
        rc = c.wsnark_pkey_setup(C.byref(ps), C.byref(cs), *bufs, C.byref(rep))
        rep2 = pd._raw(_SetupReport)
        ln = C.c_size_t(12345)
        rc2 = c.wsnark_pkey_setup_pkey(C.byref(ps), C.byref(cs), big, len(big), C.byref(ln), bufs[10], C.byref(rep2))
        assert bytes(rep) == bytes(rep2) == untouched and all(not any(b) for b in bufs) and not any(big) and ln.value == 12345
        assert rc == rc2
        return rc

    for name in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1"):      # a short array
        assert call(dict(powers, **{name: powers[name][:-64]}), blobs) == ERR_FORMAT, name
    assert call(dict(powers, tau_g1=powers["tau_g1"][:64 * n]), blobs) == ERR_FORMAT      # n entries where 2n are needed
    for name in ("polsA", "polsB", "polsC"):                               # a record index = domain; a truncated stream
        cols = [list(col.items()) for col in getattr(circ, name[-1])]
        cols[nv - 1] = cols[nv - 1] + [(n, 5)]
        assert call(powers, dict(blobs, **{name: _records_blob(cols)})) == ERR_FORMAT, name
        assert call(powers, dict(blobs, **{name: blobs[name][:-1]})) == ERR_FORMAT, name
    assert call(dict(powers, domain=48), dict(blobs, domain=48)) == ERR_SIZE                  # not a power of two
    assert call(dict(powers, domain=1 << 25), dict(blobs, domain=1 << 25)) == ERR_SIZE        # > 2^24
    assert call(dict(powers, domain=2 * n), blobs) == ERR_SIZE                                # the two domains differ
    two = bn.mul_base(1, le(2)) + powers["tau_g1"][64:]
    assert call(dict(powers, tau_g1=two), blobs) == ERR_FORMAT                                # tau_g1[0] is not the generator
    assert call(dict(powers, tau_g2=bn.mul_base(2, le(2)) + powers["tau_g2"][128:]), blobs) == ERR_FORMAT
    assert call(powers, dict(blobs, n_public=nv)) == ERR_FORMAT                               # nPublic + 1 > nVars
    assert call(powers, dict(blobs, n_public=nv - 1, n_vars=0)) == ERR_FORMAT
    # a buffer smaller than the key
    ps, keep_p = _powers_struct(powers)
    cs, keep_c = _circuit_struct(blobs)
    need = C.c_size_t()
    assert c.wsnark_pkey_setup_size(C.byref(cs), C.byref(need)) == 0
    assert need.value == len(synth.sections_to_pkey(setup_inputs(bn, log_domain, "columns")[4][0]))
    rep = pd._raw(_SetupReport)
    assert c.wsnark_pkey_setup_pkey(C.byref(ps), C.byref(cs), big, need.value - 1, None, bufs[10], C.byref(rep)) == ERR_SIZE
    assert bytes(rep) == untouched and not any(big)
    # before wsnark_init
    code = ("import ctypes as C, sys\n"
            "c = C.CDLL(sys.argv[1])\n"
            "vp = C.c_void_p\n"
            "c.wsnark_pkey_setup.argtypes = [vp] * 14\n"
            "c.wsnark_pkey_setup_pkey.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, vp]\n"
            "rep = (C.c_uint8 * 256)(*([90] * 256))\n"
            "print(c.wsnark_pkey_setup(*([None] * 13), rep), c.wsnark_pkey_setup_pkey(None, None, None, 0, None, None, rep), set(rep))\n")
    res = subprocess.run([sys.executable, "-c", code, so_path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == [str(ERR_NOINIT)] * 2 + ["{90}"], (res.stdout, res.stderr)
