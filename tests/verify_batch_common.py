"""Shared checks of the batch verifier (wsnark_groth16_verify_batch, csrc/pairing.hip) and of its Fp12 self-test hook, run by
tests/test_emul_verify_batch.py on the thread-emulator build of the kernel sources and by tests/test_gpu_verify_batch.py on the
device.  The judge everywhere is the pinned single-proof HOST verifier (wsnark_groth16_verify): status[i] of a batch must be
what that call says about proof i (1 valid, 0 invalid, 2 = it returns WSNARK_ERR_FORMAT because of the proof).

Also here, and NOT in the product: the forger.  With the toxic waste of a synthetic setup (wasmsnark_amd/synth.py) a VALID
proof for ANY public input vector x costs three fixed-base multiplications and no proving: pick a, b, set
c = (a b - alpha beta - sum_i x_i (beta a_i + alpha b_i + c_i)) / delta, A = a G1, B = b G2, C = c G1.

Section 7 has a second forger and another judge: PlantedForger builds the KEY from chosen discrete logarithms too, with
bn128_ref's Python points, so a status is an integer predicate and no verifier's answer; its fixed table plants the values that
uniform inputs never produce (IC sums that double, cancel or pass through infinity, key points at infinity, B equal to a key point)."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import bn128_ref as ref
from bn128_ref import Q, R, twist_point_outside_g2
from conftest import GOLDEN, ROOT, load_golden

OK, ERR_SIZE, ERR_FORMAT, ERR_NOINIT = 0, 1, 2, 5


# ---- the two calls, raw ----
def _inputs_bytes(inputs):
    return b"".join(int(v).to_bytes(32, "little") for v in inputs)


def host_status(lib, vkb, n_in, inputs_b, proof_b):
    """What the single host call says: 1 / 0, or 2 when it returns WSNARK_ERR_FORMAT."""
    v = C.c_int(0)
    rc = lib.c.wsnark_groth16_verify(vkb, len(vkb), inputs_b if n_in else None, n_in, proof_b, C.byref(v))
    if rc == ERR_FORMAT:
        return 2
    assert rc == OK, rc
    return v.value


def batch_status(lib, vkb, n_in, inputs_b, proofs_b, expect_rc=OK):
    n = len(proofs_b) // 384
    st = (C.c_uint8 * max(n, 1))(*([7] * max(n, 1)))
    rc = lib.c.wsnark_groth16_verify_batch(vkb, len(vkb), inputs_b if n_in else None, n_in, proofs_b, n, st)
    assert rc == expect_rc, (rc, (lib.c.wsnark_last_error() or b"").decode())
    return list(st)[:n]


def _vk(name):
    return json.load(open(os.path.join(GOLDEN, "keys", name + ".vk.json"))), json.load(open(os.path.join(GOLDEN, "keys", name + ".public.json")))


# ---- 1. Fp12 ----
def _f12_bytes(coeffs):
    assert len(coeffs) == 12
    return b"".join((c % Q).to_bytes(32, "little") for c in coeffs)


def _fp12(lib, impl, op, a, b=None):
    n = len(a) // 384
    out = (C.c_uint8 * (n * 384))()
    rc = lib.c.wsnark_selftest_fp12(impl, op, a, b if b is not None else a, out, n)
    assert rc == OK, (impl, op, rc, (lib.c.wsnark_last_error() or b"").decode())
    return bytes(out)


def fp12_elements(n_random, seed=11):
    rnd = random.Random(seed)
    rand = [[rnd.randrange(Q) for _ in range(12)] for _ in range(n_random)]
    edge = [[0] * 12, [1] + [0] * 11, [Q - 1] + [0] * 11, [rnd.randrange(Q), rnd.randrange(Q)] + [0] * 10, [Q - 1] * 12]
    return rand, edge


def check_fp12(bn, n_random=8):
    """ops 0-5, device (impl 0) against host (impl 2), on random elements and the edge grid; op 4 == op 5 on both; op 4 of a^r is 1."""
    lib = bn.lib
    rand, edge = fp12_elements(n_random)
    elems = rand + edge
    a = b"".join(_f12_bytes(e) for e in elems)
    b = b"".join(_f12_bytes(e) for e in elems[3:] + elems[:3])
    for op in range(6):
        aa, bb = a, b
        if op == 2:     # 1 / 0 is not defined
            keep = [i for i, e in enumerate(elems) if any(e)]
            aa = b"".join(a[384 * i:384 * i + 384] for i in keep)
            bb = aa
        dev, host = _fp12(lib, 0, op, aa, bb), _fp12(lib, 2, op, aa, bb)
        n = len(aa) // 384
        for i in range(n):
            assert dev[384 * i:384 * i + 384] == host[384 * i:384 * i + 384], ("op", op, "element", i)
    ra = b"".join(_f12_bytes(e) for e in rand)
    assert len(rand) >= 8
    e4 = _fp12(lib, 0, 4, ra)
    assert e4 == _fp12(lib, 0, 5, ra) == _fp12(lib, 2, 4, ra) == _fp12(lib, 2, 5, ra)
    # a^r by square-and-multiply on the host Fp12 (ops 0 / 1, impl 2); its final exponentiation is a^(p^12 - 1) = 1
    x = _f12_bytes(rand[0])
    acc = x
    for bit in bin(R)[3:]:
        acc = _fp12(lib, 2, 1, acc)
        if bit == "1":
            acc = _fp12(lib, 2, 0, acc, x)
    one = _f12_bytes([1] + [0] * 11)
    assert acc != one
    assert _fp12(lib, 0, 4, acc) == one and _fp12(lib, 0, 5, acc) == one


# ---- 2. the reference's own verifier data ----
def check_golden_verify(bn):
    from wasmsnark_amd.bn128 import proof_to_bytes, vk_to_bytes
    g = load_golden("verify.json")
    vk, cases = g["verification_key"], g["cases"]
    assert len(cases) == 18 and sum(c["reference_verdict"] for c in cases) == 3
    n_in = len(cases[0]["inputs"])
    assert n_in == 58 and all(len(c["inputs"]) == n_in for c in cases)
    vkb = vk_to_bytes(vk, n_in)
    want = [int(bool(c["reference_verdict"])) for c in cases]
    got = batch_status(bn.lib, vkb, n_in, b"".join(_inputs_bytes(c["inputs"]) for c in cases), b"".join(proof_to_bytes(c["proof"]) for c in cases))
    assert got == want
    for c, w in zip(cases, want):
        assert batch_status(bn.lib, vkb, n_in, _inputs_bytes(c["inputs"]), proof_to_bytes(c["proof"])) == [w], (c["proof_file"], c["label"])
    # the Python entry point, over the same cases
    assert bn.groth16VerifyBatch(vk, [c["inputs"] for c in cases], [c["proof"] for c in cases]) == [bool(w) for w in want]
    assert bn.groth16VerifyBatch(vk, [c["inputs"] for c in cases], [c["proof"] for c in cases], return_status=True) == want


# ---- 3. the golden proofs of the two synthetic keys ----
def check_golden_proofs(bn, name):
    vk, pub = _vk(name)
    inputs, proofs, want = [], [], []
    for c in load_golden("proofs.json")[name]:
        assert c["reference_verifies"] and c["reference_rejects_wrong_public"]
        inputs += [pub, [str((int(pub[0]) + 1) % R)] + pub[1:], pub]
        proofs += [c["proof"], c["proof"], dict(c["proof"], pi_a=c["proof"]["pi_c"])]
        want += [True, False, False]
    assert len(proofs) >= 3
    assert bn.groth16VerifyBatch(vk, inputs, proofs) == want


# ---- 4. malformed points between valid neighbours ----
def rogue_g2_json():
    """bn128_ref's twist point outside the order-r subgroup, as the coordinates of a proof or key JSON."""
    x, y = twist_point_outside_g2()
    return [[str(x[0]), str(x[1])], [str(y[0]), str(y[1])], ["1", "0"]]


def malformed_cases(good, good2, pub):
    """(label, inputs, proof) on the t6 key: the cases of test_verify.py::test_malformed_points_are_invalid_not_paired and friends."""
    bump = lambda p: [p[0], str((int(p[1]) + 1) % Q), p[2]]
    b = good["pi_b"]
    return [
        ("valid", pub, good),
        ("valid other proof", pub, good2),
        ("pi_a off the curve", pub, dict(good, pi_a=bump(good["pi_a"]))),
        ("pi_c off the curve", pub, dict(good, pi_c=bump(good["pi_c"]))),
        ("pi_b off the twist", pub, dict(good, pi_b=[b[0], [b[1][0], str((int(b[1][1]) + 1) % Q)], b[2]])),
        ("pi_b outside the subgroup", pub, dict(good, pi_b=rogue_g2_json())),
        ("z coordinates 0 and 5", pub, dict(good, pi_a=[good["pi_a"][0], good["pi_a"][1], "0"], pi_c=good["pi_c"][:2] + ["5"])),
        ("proof at infinity", pub, {"pi_a": ["0", "1", "0"], "pi_b": [["0", "0"], ["1", "0"], ["0", "0"]], "pi_c": ["0", "1", "0"]}),
        ("an input >= r", [str(R + 1)] + pub[1:], good),
        ("an input = r", pub[:-1] + [str(R)], good),
        ("coordinate >= q in pi_a", pub, dict(good, pi_a=[str(Q + 5), good["pi_a"][1], "1"])),
        ("coordinate = q in pi_b", pub, dict(good, pi_b=[b[0], [str(Q), b[1][1]], b[2]])),
        ("z coordinate >= q in pi_c", pub, dict(good, pi_c=good["pi_c"][:2] + [str(Q + 1)])),
        ("wrong public input", [str((int(pub[0]) + 1) % R)] + pub[1:], good),
    ]


def check_mixed_batches(bn, sizes=(1, 2, 63, 65, 131), seed=5):
    from wasmsnark_amd.bn128 import proof_to_bytes, vk_to_bytes
    lib = bn.lib
    vk, pub = _vk("t6")
    gp = load_golden("proofs.json")["t6"]
    cases = malformed_cases(gp[1]["proof"], gp[0]["proof"], pub)
    n_in = len(pub)
    vkb = vk_to_bytes(vk, n_in)
    enc = [(_inputs_bytes(i), proof_to_bytes(p)) for _, i, p in cases]
    single = [host_status(lib, vkb, n_in, ib, pb) for ib, pb in enc]        # the judge, once per distinct proof
    by_label = dict(zip((c[0] for c in cases), single))
    assert by_label["valid"] == 1 and by_label["valid other proof"] == 1 and by_label["z coordinates 0 and 5"] == 1
    assert by_label["coordinate >= q in pi_a"] == 2 and by_label["coordinate = q in pi_b"] == 2 and by_label["z coordinate >= q in pi_c"] == 2
    assert all(by_label[c[0]] == 0 for c in cases if by_label[c[0]] not in (1, 2)) and sorted(set(single)) == [0, 1, 2]
    rnd = random.Random(seed)
    for n in sizes:
        # every case once where the size allows, the rest half valid proofs, half random cases; a seeded random order
        if n >= len(cases):
            pick = list(range(len(cases))) + [rnd.randrange(2) if j % 2 else rnd.randrange(len(cases)) for j in range(n - len(cases))]
        else:
            pick = [rnd.randrange(len(cases)) for _ in range(n)]
        rnd.shuffle(pick)
        got = batch_status(lib, vkb, n_in, b"".join(enc[k][0] for k in pick), b"".join(enc[k][1] for k in pick))
        want = [single[k] for k in pick]
        assert got == want, (n, [(cases[k][0], g, w) for k, g, w in zip(pick, got, want) if g != w])


# ---- 5. what the key alone decides ----
def check_key_level(bn, so_path):
    from wasmsnark_amd.bn128 import proof_to_bytes, vk_to_bytes
    lib = bn.lib
    vk, pub = _vk("t6")
    gp = load_golden("proofs.json")["t6"]
    good = [gp[0]["proof"], gp[1]["proof"], gp[0]["proof"]]
    n_in = len(pub)
    ib, pb = _inputs_bytes(pub) * 3, b"".join(proof_to_bytes(p) for p in good)
    assert batch_status(lib, vk_to_bytes(vk, n_in), n_in, ib, pb) == [1, 1, 1]
    bump = lambda p: [p[0], str((int(p[1]) + 1) % Q), p[2]]
    rogue = rogue_g2_json()
    bad_keys = [dict(vk, vk_alfa_1=bump(vk["vk_alfa_1"])), dict(vk, vk_gamma_2=rogue), dict(vk, vk_delta_2=rogue),
                dict(vk, IC=[bump(vk["IC"][0])] + vk["IC"][1:]), dict(vk, IC=vk["IC"][:-1] + [bump(vk["IC"][-1])])]
    for k in bad_keys:
        kb = vk_to_bytes(k, n_in)
        assert batch_status(lib, kb, n_in, ib, pb) == [0, 0, 0]
        assert [host_status(lib, kb, n_in, _inputs_bytes(pub), proof_to_bytes(p)) for p in good] == [0, 0, 0]
    # an unreduced key coordinate: WSNARK_ERR_FORMAT for the call, nothing written
    for k in (dict(vk, vk_alfa_1=[str(Q + 1), vk["vk_alfa_1"][1], "1"]), dict(vk, IC=vk["IC"][:-1] + [[str(Q), "2", "1"]])):
        assert batch_status(lib, vk_to_bytes(k, n_in), n_in, ib, pb, expect_rc=ERR_FORMAT) == [7, 7, 7]
    # the input count cannot wrap the size check (the four values of test_verify.py::test_input_count_cannot_wrap_the_size_check)
    vkb = bytes(512)
    for n_inputs in (1 << 58, (1 << 58) - 1, (1 << 64) - 1, 2):
        st = (C.c_uint8 * 1)(7)
        rc = lib.c.wsnark_groth16_verify_batch(vkb, len(vkb), bytes(64), C.c_uint64(n_inputs), bytes(384), 1, st)
        assert rc == ERR_SIZE and st[0] == 7, n_inputs
    st = (C.c_uint8 * 1)(7)
    assert lib.c.wsnark_groth16_verify_batch(vk_to_bytes(vk, n_in), 448 + 64 * (n_in + 1), ib, n_in, pb, (1 << 24) + 1, st) == ERR_SIZE and st[0] == 7
    # count = 0 touches nothing (not even its pointers)
    assert lib.c.wsnark_groth16_verify_batch(None, 0, None, 0, None, 0, None) == OK
    assert bn.groth16VerifyBatch(vk, [], []) == []
    # before wsnark_init: a fresh process that loads the library and never initialises it
    code = ("import ctypes as C, sys\n"
            "c = C.CDLL(sys.argv[1])\n"
            "st = (C.c_uint8 * 1)(7)\n"
            "rc = c.wsnark_groth16_verify_batch(bytes(512), C.c_size_t(512), None, C.c_uint64(0), bytes(384), C.c_uint64(1), st)\n"
            "print(rc, st[0])\n")
    out = subprocess.run([sys.executable, "-c", code, so_path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == [str(ERR_NOINIT), "7"], (out.stdout, out.stderr)


def check_python_argument_errors(bn):
    import pytest
    vk, pub = _vk("t6")
    good = load_golden("proofs.json")["t6"][0]["proof"]
    with pytest.raises(ValueError):
        bn.groth16VerifyBatch(vk, [pub, pub[:-1]], [good, good])            # input vectors of two lengths
    with pytest.raises(ValueError):
        bn.groth16VerifyBatch(vk, [pub], [good, good])
    # an input outside [0, 2^256) makes that proof False without reaching the library; its neighbours are unaffected
    assert bn.groth16VerifyBatch(vk, [pub, [str(1 << 256)] + pub[1:], ["-1"] + pub[1:], pub], [good] * 4) == [True, False, False, True]


# ---- 6. forged proofs from known toxic waste ----
class Forger:
    """A synthetic setup with known toxic waste, its snarkjs verification key, and valid proofs for any public inputs."""

    def __init__(self, bn, n_public, seed=3, log_domain=4):
        from wasmsnark_amd import synth
        self.bn, self.n_public = bn, n_public
        circ = synth.make_circuit(log_domain, n_public=n_public, seed=seed)
        self.S = S = synth.setup(circ, seed=seed + 100)
        sec, (ic, gamma2) = synth.build_sections(circ, S, bn.mul_base)
        self.vk = synth.vk_from_points(n_public, sec, ic, gamma2)
        self.k = [(S.beta * S.a[s] + S.alpha * S.b[s] + S.c[s]) % R for s in range(n_public + 1)]
        self.rnd = random.Random(seed + 1000)

    def vk_bytes(self):
        from wasmsnark_amd.bn128 import vk_to_bytes
        return vk_to_bytes(self.vk, self.n_public)

    def forge(self, n):
        """n valid proofs with distinct random public inputs: (inputs bytes (n x n_public x 32), proofs bytes (n x 384))."""
        rinv = pow(1 << 256, Q - 2, Q)
        S, rnd = self.S, self.rnd
        xs = [[rnd.randrange(R) for _ in range(self.n_public)] for _ in range(n)]
        ab = [(rnd.randrange(1, R), rnd.randrange(1, R)) for _ in range(n)]
        dinv = pow(S.delta, R - 2, R)
        cs = [((a * b - S.alpha * S.beta - sum(x * k for x, k in zip([1] + x_, self.k))) * dinv) % R for (a, b), x_ in zip(ab, xs)]
        le = lambda v: int(v).to_bytes(32, "little")
        g1 = self.bn.mul_base(1, b"".join(le(a) for a, _ in ab) + b"".join(le(c) for c in cs))
        g2 = self.bn.mul_base(2, b"".join(le(b) for _, b in ab))
        plain = lambda bs: le(int.from_bytes(bs, "little") * rinv % Q)         # Montgomery affine bytes -> plain
        one, zero = le(1), le(0)
        proofs = bytearray()
        for i in range(n):
            A, Cp, B = g1[64 * i:64 * i + 64], g1[64 * (n + i):64 * (n + i) + 64], g2[128 * i:128 * i + 128]
            proofs += plain(A[:32]) + plain(A[32:]) + one
            proofs += b"".join(plain(B[32 * j:32 * j + 32]) for j in range(4)) + one + zero
            proofs += plain(Cp[:32]) + plain(Cp[32:]) + one
        return b"".join(le(v) for x_ in xs for v in x_), bytes(proofs)


COORD_WORDS = (0, 1, 3, 4, 5, 6, 9, 10)      # the eight x / y coordinates of a 384-byte proof record (z words: 2, 7, 8, 11)


def tamper(proofs_b, which, rnd):
    """One random bit of one random x / y coordinate flipped in each proof of `which`; returns (bytes, {index: status by construction})."""
    p = bytearray(proofs_b)
    want = {}
    for i in which:
        w, bit = rnd.choice(COORD_WORDS), rnd.randrange(256)
        off = 384 * i + 32 * w
        v = int.from_bytes(p[off:off + 32], "little") ^ (1 << bit)
        p[off:off + 32] = v.to_bytes(32, "little")
        want[i] = 2 if v >= Q else 0          # a changed coordinate is another point, or none: never valid
    return bytes(p), want


def check_forged(bn, n_public, n, seed=3):
    lib = bn.lib
    F = Forger(bn, n_public, seed=seed)
    vkb = F.vk_bytes()
    ib, pb = F.forge(n)
    # the forger itself, once against the pinned host verifier
    assert host_status(lib, vkb, n_public, ib[:32 * n_public], pb[:384]) == 1
    assert batch_status(lib, vkb, n_public, ib, pb) == [1] * n
    rnd = random.Random(seed + 7)
    which = sorted(rnd.sample(range(n), n // 3))
    tp, want = tamper(pb, which, rnd)
    got = batch_status(lib, vkb, n_public, ib, tp)
    for i in range(n):
        if i in want:
            single = host_status(lib, vkb, n_public, ib[32 * n_public * i:32 * n_public * (i + 1)], tp[384 * i:384 * i + 384])
            assert got[i] == single == want[i], (i, got[i], single, want[i])
        else:
            assert got[i] == 1, i


# ---- 7. planted keys, inputs and proofs: every status is an integer predicate ----
_fixed, _points = {}, {}


def _mul_gen(g, k):
    """(k mod r) * generator of G1 (g = 1) or G2 (g = 2) in bn128_ref's affine integers, None for infinity; kept per scalar."""
    k %= R
    if (g, k) not in _points:
        if g not in _fixed:
            _fixed[g] = ref.FixedBase(ref.g1_add, ref.G1) if g == 1 else ref.FixedBase(ref.g2_add, ref.G2)
        _points[g, k] = _fixed[g].mul(k)
    return _points[g, k]


def _g1_plain(p):
    return bytes(64) if p is None else ref.le(p[0]) + ref.le(p[1])


def _g2_plain(p):
    return bytes(128) if p is None else ref.le(p[0][0]) + ref.le(p[0][1]) + ref.le(p[1][0]) + ref.le(p[1][1])


class PlantedForger:
    """A verification key from chosen discrete logarithms, no circuit: alfa1 = alpha G1, beta2 = beta G2, gamma2 = gamma G2,
    delta2 = delta G2, IC[i] = kappa[i] G1; a zero scalar is the point at infinity, (0, 0) in the key.  The proof
    (a G1, b G2, c G1) for inputs x then has status 1 iff  a b == alpha beta + gamma sum_i x_i kappa[i] + c delta (mod r),
    x_0 = 1, and a, b, c are non-zero mod r (a zero proof point has no encoding: (0, 0) is off the curve); 0 otherwise.
    Points come from bn128_ref alone.  gamma2_point replaces gamma2 by a twist point outside G2: then every status is 0."""

    def __init__(self, alpha, beta, gamma, delta, kappa, gamma2_point=None):
        self.alpha, self.beta, self.gamma, self.delta, self.kappa = alpha % R, beta % R, gamma % R, delta % R, [k % R for k in kappa]
        self.n_public = len(kappa) - 1
        self.key_ok = gamma2_point is None
        self.gamma2 = _mul_gen(2, gamma) if gamma2_point is None else gamma2_point

    def vk_bytes(self):
        return (_g1_plain(_mul_gen(1, self.alpha)) + _g2_plain(_mul_gen(2, self.beta)) + _g2_plain(self.gamma2)
                + _g2_plain(_mul_gen(2, self.delta)) + b"".join(_g1_plain(_mul_gen(1, k)) for k in self.kappa))

    def ic(self, x):
        assert len(x) == self.n_public and all(0 <= v < R for v in x)
        return sum(v * k for v, k in zip([1] + list(x), self.kappa)) % R

    def status(self, x, a, b, c):
        if not self.key_ok or a % R == 0 or b % R == 0 or c % R == 0:
            return 0
        return int((a * b - self.alpha * self.beta - self.gamma * self.ic(x) - c * self.delta) % R == 0)

    def solve_c(self, x, a, b):
        return (a * b - self.alpha * self.beta - self.gamma * self.ic(x)) * pow(self.delta, -1, R) % R

    def solve_b(self, x, a, c):
        return (self.alpha * self.beta + self.gamma * self.ic(x) + c * self.delta) * pow(a, -1, R) % R

    @staticmethod
    def proof(a, b, c, B=None):
        """The 384 bytes Forger.forge writes: plain little-endian, z words 1, (1, 0), 1."""
        one, zero = ref.le(1), ref.le(0)
        return (_g1_plain(_mul_gen(1, a)) + one + _g2_plain(_mul_gen(2, b) if B is None else B) + one + zero
                + _g1_plain(_mul_gen(1, c)) + one)

    def neighbours(self, n, rnd):
        """n proofs that the predicate accepts (on a sound key), for random inputs: Case tuples like the table's."""
        out = []
        for _ in range(n):
            x, a, c = tuple(rnd.randrange(R) for _ in range(self.n_public)), rnd.randrange(1, R), rnd.randrange(1, R)
            b = self.solve_b(x, a, c)
            assert b and self.status(x, a, b, c) == int(self.key_ok)
            out.append(("valid neighbour", x, self.proof(a, b, c), int(self.key_ok)))
        return out


PLANTED_VALID = 35        # how many proofs of the table below have status 1
PLANTED_SOUND_KEYS = 15   # its keys, less the three whose gamma2 is outside G2 (on those every status is 0)


def _build_planted_table():
    rnd = random.Random(20260)
    nz = lambda: rnd.randrange(1, R)
    k0, k1 = nz(), nz()
    rows = []

    def key(kappa, **fixed):
        p = {n: nz() for n in ("alpha", "beta", "gamma", "delta")}
        p.update(fixed)
        return PlantedForger(p["alpha"], p["beta"], p["gamma"], p["delta"], kappa)

    def case(F, label, x, a, b, c, want):
        """One proof with its status as the table states it, which the integer predicate must give too."""
        assert F.status(x, a, b, c) == want, (label, x)
        return dict(label=label, x=tuple(x), a=a, b=b, c=c, want=want, proof=F.proof(a, b, c))

    def valid(F, x, label="valid"):
        a, b = nz(), nz()
        c = F.solve_c(x, a, b)
        assert c
        return case(F, "%s x=%s" % (label, _short(x)), x, a, b, c, 1)

    def c_plus_1(F, v):
        return case(F, v["label"] + ", c+1", v["x"], v["a"], v["b"], (v["c"] + 1) % R, 0)

    def x1_plus_1(F, v):
        return case(F, v["label"] + ", x_1+1", ((v["x"][0] + 1) % R,) + v["x"][1:], v["a"], v["b"], v["c"], 0)

    def row(name, F, cases):
        rows.append((name, F, cases))

    # -- IC(x): the joint double-and-add chain of verify_prepare_kernel (and the per-input chains of verify.hip).  In the comments
    #    "acc" is the chain's accumulator, bits are taken from the top, inputs within a bit in order, IC[0] is added last
    F = key([k0, -k0, k1])
    v = [valid(F, (1, 0)),      # acc = IC[1] = -IC[0] at the close: the closing madd cancels, IC(x) is infinity (ic_is_inf, no gamma lines)
         valid(F, (1, 5)),      # IC[0] + IC[1] cancel in the sum only: every addition is the generic one, IC(x) = 5 IC[2]
         valid(F, (0, 0))]      # acc is infinity through all 254 doublings: the closing madd copies IC[0]
    row("IC[1] = -IC[0]", F, v + [x1_plus_1(F, v[0])])
    F = key([k0, k0, k1])
    v = [valid(F, (1, 0)),      # acc = IC[1] = IC[0], still affine (zz = 1), at the close: the closing madd doubles
         valid(F, (2, 0)),      # acc = 2 IC[0]: the generic addition next to it
         valid(F, (R - 1, 0)),  # acc = -IC[0] with zz != 1 at the close: the closing madd cancels, IC(x) is infinity; input r - 1
         valid(F, (R - 2, 0))]  # acc = -2 IC[0]: generic again
    row("IC[1] = IC[0]", F, v + [c_plus_1(F, v[0])])
    F = key([k0, k1, 2 * k1])
    v = [valid(F, (2, 1)),              # bit 1 copies IC[1], bit 0 doubles it and adds IC[2] = 2 IC[1]: madd doubles, acc with zz != 1
         valid(F, (6, 1)),              # acc = 6 IC[1] meets IC[2]: generic
         valid(F, (R - 1, R - 1)),      # both inputs r - 1: 2 x 253 set bits
         valid(F, (1 << 253, 1))]       # the top bit of the chain: IC[1] copied at bit 253, then 253 doublings
    row("IC[2] = 2 IC[1]", F, v + [x1_plus_1(F, v[0])])
    F = key([k0, k1, -2 * k1])
    v = [valid(F, (2, 1)),      # at bit 0 acc = 2 IC[1] meets IC[2] = -2 IC[1]: infinity, then the closing madd copies IC[0]
         valid(F, (6, 3)),      # 3 IC[1] - 2 IC[1] at bit 1 (generic), doubled, cancelled by IC[2] at bit 0
         valid(F, (5, 2))]      # infinity at bit 1, doubled as infinity at bit 0, then IC[1] copied into it: the chain goes on
    row("IC[2] = -2 IC[1]", F, v + [c_plus_1(F, v[1])])
    F = key([k0, k1, k1])
    v = [valid(F, (1, 1)),      # bit 0 copies IC[1], then adds IC[2] = IC[1] in the same bit: madd doubles an affine acc
         valid(F, (3, 3)),      # the same at bit 1, then 4 IC[1] + IC[1] + IC[1]: generic
         valid(F, (1, 2))]
    row("IC[2] = IC[1]", F, v + [x1_plus_1(F, v[0])])
    F = key([0, k1, 0])         # IC points at infinity (a public signal in no constraint): ic_inf[0], ic_inf[2]
    v = [valid(F, (1, 7)),      # the set bits of x_2 and the closing addition are skipped
         valid(F, (0, 9)),      # nothing is ever added: IC(x) is infinity
         valid(F, (R - 1, 1))]
    row("IC[0] = IC[2] = O", F, v + [x1_plus_1(F, v[1])])
    F = key([k0])               # n_inputs == 0 (inputs == NULL): IC(x) = IC[0]
    v = [valid(F, ())]
    row("no inputs", F, v + [c_plus_1(F, v[0])])
    F = key([0])                # ... and IC[0] at infinity as well: IC(x) is infinity
    v = [valid(F, ())]
    row("no inputs, IC[0] = O", F, v + [c_plus_1(F, v[0])])

    # -- the proof side, on one key with random kappa
    F = base = key([nz(), nz(), nz()])
    x = (nz(), nz())
    v = valid(F, x)
    a, b, c = v["a"], v["b"], v["c"]
    c0 = nz()
    row("random key", F, [
        v, c_plus_1(F, v), x1_plus_1(F, v),
        case(F, "(-A, B)", x, -a % R, b, c, 0),
        case(F, "(-A, -B)", x, -a % R, -b % R, c, 1),         # e(-A, -B) = e(A, B)
        case(F, "a b = alpha beta + gamma IC(x), C = (0, 0)", x, a, F.solve_b(x, a, 0), 0, 0)])      # c = 0 has no encoding
    c = F.solve_c(x, F.alpha, F.beta)       # (= -gamma IC(x) / delta)
    v = case(F, "(A, B) = (alfa1, beta2)", x, F.alpha, F.beta, c, 1)
    row("random key, the key's own pair as (A, B)", F, [v, case(F, "(A, B) = (-alfa1, beta2)", x, -F.alpha % R, F.beta, c, 0), c_plus_1(F, v)])
    a = nz()
    v = [case(F, "B = gamma2", x, a, F.gamma, F.solve_c(x, a, F.gamma), 1),      # B's Miller lines are gamma2's stored ones
         case(F, "B = delta2", x, a, F.delta, F.solve_c(x, a, F.delta), 1)]
    row("random key, B a key point", F, v + [c_plus_1(F, v[0])])

    # -- prepare_key.  A key point at infinity pairs to 1 here, which is what the predicate says with a zero scalar.  The reference
    #    checks no point: its verdict on such keys is an accident of its Miller loop (see include/wsnark.h), may differ, and is
    #    no yardstick for these rows, so tests/golden/ has no reference fixtures for them
    F = key([nz(), nz(), nz()], gamma=(g := nz()), delta=g)       # gamma2 == delta2: the two stored line sets are equal
    v = valid(F, x)
    row("delta2 = gamma2", F, [v, case(F, "c = 1", x, v["a"], v["b"], 1, 0), x1_plus_1(F, v)])
    F = key([nz(), nz(), nz()], gamma=0)        # gamma2 at infinity: gamma_on false, steps from delta2; the inputs do not matter
    a = nz()
    b = F.solve_b(x, a, 3)                       # (= (alpha beta + 3 delta) / a)
    row("gamma2 = O", F, [case(F, "c = 3", x, a, b, 3, 1), case(F, "c = 3, other inputs", ((x[0] + 1) % R, 0), a, b, 3, 1), case(F, "c = 4", x, a, b, 4, 0)])
    F = key([nz(), nz(), nz()], delta=0)        # delta2 at infinity: delta_on false; C does not matter
    a = nz()
    b = F.solve_b(x, a, c0)                      # (= (alpha beta + gamma IC(x)) / a)
    v = case(F, "any c", x, a, b, c0, 1)
    row("delta2 = O", F, [v, case(F, "another c", x, a, b, nz(), 1), x1_plus_1(F, v)])
    F = key([nz(), nz(), nz()], alpha=0)        # alfa1 at infinity: the key's own Miller value is 1
    v = valid(F, x)
    row("alfa1 = O", F, [v, c_plus_1(F, v)])
    F = key([nz(), nz(), nz()], beta=0)         # beta2 at infinity: the same
    v = valid(F, x)
    row("beta2 = O", F, [v, c_plus_1(F, v)])
    F = key([nz(), nz(), nz()], gamma=0, delta=0)       # no stored lines at all: e(A, B) = e(alfa1, beta2) is the whole check
    a = nz()
    b = F.solve_b(x, a, c0)
    row("gamma2 = delta2 = O", F, [case(F, "a b = alpha beta", x, a, b, c0, 1), case(F, "b+1", x, a, (b + 1) % R, c0, 0)])

    # -- twist points outside G2 whose order is a small factor of the cofactor 2q - r: on the twist, not killed by r
    good = rows[8][2][0], rows[8][2][4]          # two proofs that the random key accepts
    assert all(g["want"] == 1 for g in good) and rows[8][1] is base
    rogue_b = []
    for d in (10069, 5864401, 10069 * 5864401):
        pt = ref.twist_point_of_order(d, rnd)
        assert not ref.g2_times_r_is_infinity(pt)
        g = good[0]
        rogue_b.append(dict(label="B of order %d" % d, x=g["x"], want=0, proof=PlantedForger.proof(g["a"], 1, g["c"], B=pt)))
        F = PlantedForger(base.alpha, base.beta, base.gamma, base.delta, base.kappa, gamma2_point=pt)
        row("gamma2 of order %d" % d, F, [dict(g, want=0) for g in good])      # key_ok false: every status 0
    row("random key, B outside G2", base, rogue_b)
    return rows


def _short(x):
    return "(%s)" % ", ".join(str(v) if v < 1000 else "r-%d" % (R - v) if R - v < 1000 else "2^%d" % (v.bit_length() - 1) if v & (v - 1) == 0 else "..." for v in x)


_planted = None


def planted_table():
    """[(row name, its PlantedForger, [case, ...])], built once; a case has label, x, proof (384 bytes) and want."""
    global _planted
    if _planted is None:
        _planted = _build_planted_table()
        n = sum(len(cases) for _, _, cases in _planted)
        assert n == 66 and sum(c["want"] for _, _, cases in _planted for c in cases) == PLANTED_VALID
    return _planted


def planted_keys():
    """The table by key: [(PlantedForger, every case of its rows)]."""
    keys = []
    for _, F, cases in planted_table():
        for k in keys:
            if k[0] is F:
                k[1].extend(cases)
                break
        else:
            keys.append((F, list(cases)))
    return keys


def _case_inputs(cases):
    return b"".join(_inputs_bytes(c["x"]) for c in cases)


def check_planted_host(lib):
    """The table through the single-proof host verifier (wsnark_groth16_verify) alone."""
    got = want = 0
    for name, F, cases in planted_table():
        vkb = F.vk_bytes()
        for c in cases:
            st = host_status(lib, vkb, F.n_public, _inputs_bytes(c["x"]), c["proof"])
            assert st == c["want"], (name, c["label"], st)
            got, want = got + st, want + c["want"]
    assert got == want == PLANTED_VALID


def shuffled_key_batches(seed=31, n_neighbours=3):
    """Per key every case of its rows and n_neighbours valid proofs for random inputs, in a seeded random order."""
    rnd = random.Random(seed)
    out = []
    for F, cases in planted_keys():
        mixed = [dict(label=n[0], x=n[1], proof=n[2], want=n[3]) for n in F.neighbours(n_neighbours, rnd)] + cases
        rnd.shuffle(mixed)
        out.append((F, mixed))
    return out


def check_planted(bn, what=("rows", "alone", "host", "shuffled"), plain=None, tune=None):
    """The planted table on the batch verifier: each row in one call ("rows"), each proof in a call of its own ("alone"), the
    host verifier ("host"), and per key all its rows between valid neighbours in one shuffled batch ("shuffled").  plain: with
    VERIFY_PLAIN_EXP set to it through the tune fixture."""
    lib = bn.lib
    if plain is not None:
        tune(lib, "VERIFY_PLAIN_EXP", plain)
    table = planted_table()
    ones = 0
    if "rows" in what:
        for name, F, cases in table:
            got = batch_status(lib, F.vk_bytes(), F.n_public, _case_inputs(cases), b"".join(c["proof"] for c in cases))
            assert got == [c["want"] for c in cases], (name, [(c["label"], g) for c, g in zip(cases, got) if g != c["want"]])
            ones += sum(got)
        assert ones == PLANTED_VALID
    if "alone" in what:
        ones = 0
        for name, F, cases in table:
            vkb = F.vk_bytes()
            for c in cases:
                got = batch_status(lib, vkb, F.n_public, _inputs_bytes(c["x"]), c["proof"])
                assert got == [c["want"]], (name, c["label"], got)
                ones += got[0]
        assert ones == PLANTED_VALID
    if "host" in what:
        check_planted_host(lib)
    if "shuffled" in what:
        ones = 0
        batches = shuffled_key_batches()
        for F, mixed in batches:
            assert len(mixed) < 64
            got = batch_status(lib, F.vk_bytes(), F.n_public, _case_inputs(mixed), b"".join(c["proof"] for c in mixed))
            assert got == [c["want"] for c in mixed], [(c["label"], g) for c, g in zip(mixed, got) if g != c["want"]]
            ones += sum(got)
        assert ones == PLANTED_VALID + 3 * PLANTED_SOUND_KEYS and len(batches) == PLANTED_SOUND_KEYS + 3


def check_mul_base_against_reference(bn):
    """Forger's points come from bn.mul_base, PlantedForger's from bn128_ref: the same bytes on a handful of scalars, 0 included."""
    rnd = random.Random(8)
    ks = [0, 1, 2, R - 1, rnd.randrange(R), rnd.randrange(R)]
    sc = b"".join(ref.le(k) for k in ks)
    g1, g2 = bn.mul_base(1, sc), bn.mul_base(2, sc)
    for i, k in enumerate(ks):
        p1, p2 = ref.g1_mul(ref.G1, k), ref.g2_mul(ref.G2, k)
        assert p1 == _mul_gen(1, k) and p2 == _mul_gen(2, k)          # (the table's fixed-base shortcut is bn128_ref's double-and-add)
        assert g1[64 * i:64 * i + 64] == (bytes(64) if p1 is None else ref.mont(p1[0]) + ref.mont(p1[1])), k
        assert g2[128 * i:128 * i + 128] == (bytes(128) if p2 is None else b"".join(ref.mont(v) for v in p2[0] + p2[1])), k
