"""The contracts of the radix-2^29 lazy field (wasmsnark_amd/csrc/field29.h, and the stacked forms of fp2.h) as a table, and the checks
that run it through wsnark_selftest_field29 -- raw limbs in, raw limbs out, one lane per case.

Shared by tests/test_emul_field29_contracts.py (CPU: the C bodies under the thread emulator and on the host) and
tests/test_gpu_field29_contracts.py (-m gpu: the generated v_mad_u64_u32 chains of mad_chain.h on an MI355X).

One row per op.  For every operand the row gives the bound multiple k (value < k p, or <= k p where the form is closed, e.g. neg_weak's
(0, 2p]) -- taken from the function's comment AND from the widest operand a call site passes (ntt.hip's butterflies, curve.h's
madd_wide / madd_fast / mmadd_fast, fp2.h's mul / sqr / mulsub2); where the two differ the call site is the contract.  For the result it
gives the residue as a plain Python-integer expression, the interval, and -- where the function's comment defines the value itself
(every borrow chain and fold does) -- the exact value.  Every result must have limbs 0..7 below 2^29, and a result below 4p (what
the transforms and the point tables pack next) a top limb below 2^24.

Nothing here is compared against another implementation of the project: all expectations are integer arithmetic mod p.

    python tests/field29_contracts.py        prints the number of cases per row"""
import functools
import itertools
import random
import zlib

import numpy as np

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
PRIMES = {0: Q, 1: R}
FNAME = {0: "Fq", 1: "Fr"}
M29 = (1 << 29) - 1
RADIX = 1 << 261                      # the internal Montgomery radix: 9 limbs of 29 bits
N_RANDOM = 256
N_SAMPLE = 512


# ---------------------------------------------------------------------------------------------------------------- limbs
def limbs(v):
    """nine limbs of v: 29 bits each, the top one takes the rest"""
    assert 0 <= v < 1 << (232 + 32)
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def words(v):
    """eight 32-bit words of a 256-bit v, and a ninth that the library must ignore"""
    assert 0 <= v < 1 << 256
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0xDEADBEEF]


def value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def value_words(l):
    return sum(int(x) << (32 * i) for i, x in enumerate(l[:8]))


# ------------------------------------------------------------------------------------------------------------- operands
class T:
    """a tight operand: value in [0, k p) -- (0, ...) with nonzero, ... k p] with closed -- limbs 0..7 below 2^29"""
    def __init__(self, k, closed=False, nonzero=False, extra=None):
        self.k, self.closed, self.nonzero, self.extra = k, closed, nonzero, extra

    def top(self, p):
        return self.k * p + (1 if self.closed else 0)          # exclusive

    def maxlimb(self, p):
        """the largest admissible value whose limbs 0..7 are all 2^29 - 1"""
        return (((self.top(p) >> 232) - 1) << 232) | ((1 << 232) - 1)

    def maxval(self, p):
        return self.top(p) - 1

    def grid(self, p):
        k, hi = self.k, self.top(p)
        g = {0, 1, p - 1, p, p + 1, k * p - 1, k * p - 2, k * p}
        for j in range(1, k):
            g |= {j * p - 1, j * p, j * p + 1}
        g.add(self.maxlimb(p))
        for i in range(8):
            g.add(M29 << (29 * i))                             # one saturated limb
        g.add(((hi - 1) >> 232) << 232)                        # the top limb alone, as large as the bound lets it be
        for par in (0, 1):                                     # alternating saturated / zero limbs, without and with the largest top limb
            low = sum(M29 << (29 * i) for i in range(8) if i % 2 == par)
            g.add(low)
            g.add(low + (((hi - 1 - low) >> 232) << 232))
        x = pow(3, 0x1234567, p)                               # one residue in every representative
        for j in range(k):
            g.add(j * p + x)
        if self.extra:
            g |= set(self.extra(p))
        return sorted(v for v in g if (1 if self.nonzero else 0) <= v < hi)

    def rand(self, p, rnd):
        return rnd.randrange(1 if self.nonzero else 0, self.top(p))

    enc = staticmethod(limbs)


class W:
    """a raw 256-bit operand in the stored form: eight 32-bit words"""
    def top(self, p):
        return 1 << 256

    def maxlimb(self, p):
        return (1 << 256) - 1

    maxval = maxlimb

    def grid(self, p):
        g = set(T(5).grid(p)) | {5 * p, 5 * p + 1, (1 << 256) - 1, (1 << 256) - 2, 1 << 255}
        for i in range(8):
            g.add(0xFFFFFFFF << (32 * i))
        # what shares its low word (two words, seven words) with p and is not p: packed_is_zero's second test must reject it
        g |= {p & 0xFFFFFFFF, p & ((1 << 64) - 1), p & ((1 << 224) - 1), p + (1 << 32), p + (1 << 64), p ^ (1 << 200), p | (1 << 255)}
        return sorted(v for v in g if 0 <= v < 1 << 256)

    def rand(self, p, rnd):
        return rnd.randrange(1 << 256)

    enc = staticmethod(words)


def _near_multiples(kmax):
    """values that share limb 0 with some j p and differ above it: the cheap filter of the zero tests passes, the exact test must reject"""
    def f(p):
        out = set()
        for j in range(1, kmax + 1):
            jp = j * p
            out |= {jp & M29, jp + (1 << 29), jp - (1 << 29), jp + (1 << 232), jp - (1 << 232), jp ^ (1 << (29 * 3 + 5)), jp ^ (1 << (29 * 7 + 28)),
                    jp & ((1 << 232) - 1), (jp & M29) | ((jp >> 232) << 232)}
        return out
    return f


# -------------------------------------------------------------------------------------------------------------- results
class Res:
    """one element of a result: residue(p, v) mod p, lo p <(=) value <(=) hi p, exact(p, v) where the comment defines the value"""
    def __init__(self, residue, hi, lo_open=False, hi_closed=False, exact=None):
        self.residue, self.hi, self.lo_open, self.hi_closed, self.exact = residue, hi, lo_open, hi_closed, exact


def strict(residue, exact=None):
    return Res(residue, 2, exact=exact)


RINV = {p: pow(RADIX, -1, p) for p in (Q, R)}


def mont(x, p):
    return x * RINV[p] % p


class Row:
    def __init__(self, name, op, opnds, res, kind="elem", ext=False, note=""):
        self.name, self.op, self.opnds, self.kind, self.ext, self.note = name, op, opnds, kind, ext, note
        self.res = res if isinstance(res, (list, tuple)) else [res]


# the ops of include/wsnark.h (WSNARK_F29_*)
(MUL, SQR, MUL_INL, MUL2ADD, MUL2ADD_INL, MUL4ADD, MULSUB2, ADD, SUB, NEG, SUB_WEAK, SUB_WEAK4, SUB_WEAK8, NEG_WEAK, NEG_WEAK4, ADD_NR,
 ADD_LAZY_MUL, FOLD8, FOLD16, FOLD4TO2, COND_SUB_2P, NARROW, CANONICAL, X3_WIDE, SUB_WIDE, IS_ZERO, IS_ZERO_WEAK, IS_ZERO_WIDE,
 MAYBE_ZERO_WEAK, MAYBE_ZERO_WIDE, PACK_UNPACK, PACKED_IS_ZERO, TO_INTERNAL, FROM_INTERNAL, DBL, EQ, FP2_MUL, FP2_SQR, FP2_MULSUB2) = range(39)

_prod2 = lambda p, v: mont(v[0] * v[1], p)
_mul2add = lambda p, v: mont(v[0] * v[1] + v[2] * v[3], p)
_mulsub2 = lambda p, v: mont(v[0] * v[1] - v[2] * v[3], p)
_mul4add = lambda p, v: mont(v[0] * v[1] + v[2] * v[3] + v[4] * v[5] + v[6] * v[7], p)

ROWS = [
    # ---- products: result in [0, 2p), tight.  (a b + m p) / 2^261 < p (1 + ka kb p / 2^261) and p / 2^261 < 2^-7.4: below 2p while
    # ka kb <= 100.  Call sites: ntt.hip multiplies sub_weak8 results (< 16p) by twiddles (< 2p); curve.h multiplies and squares
    # sub_wide results (< 10p); fp2.h's sqr multiplies two values below 8p.
    Row("mul_16p_2p", MUL, [T(16), T(2)], strict(_prod2), note="ntt.hip: mul(sub_weak8(s0, s1), w)"),
    Row("mul_10p_10p", MUL, [T(10), T(10)], strict(_prod2), note="curve.h: mul(P, PP), P = sub_wide(...); both slots at the wide bound"),
    Row("mul_inl_16p_2p", MUL_INL, [T(16), T(2)], strict(_prod2)),
    Row("mul_inl_10p_10p", MUL_INL, [T(10), T(10)], strict(_prod2), note="Field29I::mul in the tails' madd_wide; fp2.h sqr: 8p x 8p"),
    Row("sqr_10p", SQR, [T(10)], strict(lambda p, v: mont(v[0] * v[0], p)), note="curve.h: sqr(P), P = sub_wide(...)"),
    Row("add_lazy_mul", ADD_LAZY_MUL, [T(4), T(4), T(8)], strict(lambda p, v: mont((v[0] + v[1]) * v[2], p)),
        note="fp2.h sqr: mul_inl(add_lazy(a0, a1), sub_weak4(a0, a1)) with weak components: a carry-free sum below 8p, limbs below 2^30"),
    Row("mul2add_curve", MUL2ADD, [T(4), T(10), T(2, closed=True), T(2)], strict(_mul2add),
        note="curve.h: mulsub2(R, sub_wide(Q, X3), y, PPP) = mul2add(R < 4p, < 10p, neg_weak(y) <= 2p, PPP)"),
    Row("mul2add_fp2", MUL2ADD, [T(4), T(2), T(4), T(2, closed=True)], strict(_mul2add), note="fp2.h mul: a0 b0 + a1 (2p - b1)"),
    Row("mul2add_inl_curve", MUL2ADD_INL, [T(4), T(10), T(2, closed=True), T(2)], strict(_mul2add)),
    Row("mul2add_inl_fp2", MUL2ADD_INL, [T(4), T(2), T(4), T(2, closed=True)], strict(_mul2add)),
    Row("mulsub2", MULSUB2, [T(4), T(10), T(2), T(2)], strict(_mulsub2), note="curve.h madd_wide: mulsub2(R, sub_wide(Q, X3), acc.y, PPP)"),
    Row("mul4add", MUL4ADD, [T(4), T(4), T(4), T(4, closed=True), T(2, closed=True), T(2), T(2, closed=True), T(2)], strict(_mul4add),
        note="fp2.h mulsub2: weak components (< 4p) and neg_weak4 / neg_weak results (<= 4p, <= 2p): 40 p^2, 45 terms per column"),
    # ---- strict sums and differences
    Row("add", ADD, [T(2), T(2)], strict(lambda p, v: v[0] + v[1], exact=lambda p, v: (v[0] + v[1]) % (2 * p))),
    Row("dbl", DBL, [T(2)], strict(lambda p, v: 2 * v[0], exact=lambda p, v: 2 * v[0] % (2 * p))),
    Row("sub", SUB, [T(2), T(2)], strict(lambda p, v: v[0] - v[1], exact=lambda p, v: (v[0] - v[1]) % (2 * p))),
    Row("neg", NEG, [T(2)], strict(lambda p, v: -v[0], exact=lambda p, v: 2 * p - v[0] if v[0] else 0)),
    # ---- uncorrected differences: the value itself is defined
    Row("sub_weak", SUB_WEAK, [T(2), T(2)], Res(lambda p, v: v[0] - v[1], 4, lo_open=True, exact=lambda p, v: v[0] - v[1] + 2 * p)),
    Row("sub_weak4", SUB_WEAK4, [T(4), T(4)], Res(lambda p, v: v[0] - v[1], 8, lo_open=True, exact=lambda p, v: v[0] - v[1] + 4 * p)),
    Row("sub_weak8", SUB_WEAK8, [T(8), T(8)], Res(lambda p, v: v[0] - v[1], 16, lo_open=True, exact=lambda p, v: v[0] - v[1] + 8 * p)),
    Row("neg_weak", NEG_WEAK, [T(2)], Res(lambda p, v: -v[0], 2, lo_open=True, hi_closed=True, exact=lambda p, v: 2 * p - v[0])),
    Row("neg_weak4", NEG_WEAK4, [T(4)], Res(lambda p, v: -v[0], 4, lo_open=True, hi_closed=True, exact=lambda p, v: 4 * p - v[0])),
    Row("add_nr", ADD_NR, [T(8), T(8)], Res(lambda p, v: v[0] + v[1], 16, exact=lambda p, v: v[0] + v[1]),
        note="ntt.hip: add_nr(s0, s1) with s0, s1 = sums of two tile values (< 8p each)"),
    Row("x3_wide", X3_WIDE, [T(2), T(2), T(2)], Res(lambda p, v: v[0] - v[1] - 2 * v[2], 8, lo_open=True, exact=lambda p, v: v[0] - v[1] - 2 * v[2] + 6 * p)),
    Row("sub_wide", SUB_WIDE, [T(2), T(8)], Res(lambda p, v: v[0] - v[1], 10, lo_open=True, exact=lambda p, v: v[0] - v[1] + 8 * p)),
    # ---- folds: r = s - k p if s >= k p else s, so the value is s mod (the target bound)
    Row("fold8", FOLD8, [T(8)], Res(lambda p, v: v[0], 4, exact=lambda p, v: v[0] % (4 * p))),
    Row("fold16", FOLD16, [T(16)], Res(lambda p, v: v[0], 4, exact=lambda p, v: v[0] % (4 * p))),
    Row("fold4to2", FOLD4TO2, [T(4)], Res(lambda p, v: v[0], 2, exact=lambda p, v: v[0] % (2 * p))),
    Row("cond_sub_2p", COND_SUB_2P, [T(4)], Res(lambda p, v: v[0], 2, exact=lambda p, v: v[0] % (2 * p))),
    Row("narrow", NARROW, [T(8)], Res(lambda p, v: v[0], 2, exact=lambda p, v: v[0] % (2 * p))),
    Row("canonical", CANONICAL, [T(2)], Res(lambda p, v: v[0], 1, exact=lambda p, v: v[0] % p)),
    # ---- predicates (None = no assertion: the cheap necessary tests may say yes to anything)
    Row("is_zero", IS_ZERO, [T(2, extra=_near_multiples(1))], lambda p, v: v[0] in (0, p), kind="pred"),
    Row("is_zero_weak", IS_ZERO_WEAK, [T(4, nonzero=True, extra=_near_multiples(3))], lambda p, v: v[0] in (p, 2 * p, 3 * p), kind="pred"),
    Row("is_zero_wide", IS_ZERO_WIDE, [T(10, nonzero=True, extra=_near_multiples(9))], lambda p, v: v[0] % p == 0, kind="pred"),
    Row("maybe_zero_weak", MAYBE_ZERO_WEAK, [T(4, extra=_near_multiples(3))], lambda p, v: True if v[0] % p == 0 else None, kind="pred"),
    Row("maybe_zero_wide", MAYBE_ZERO_WIDE, [T(10, extra=_near_multiples(9))], lambda p, v: True if v[0] % p == 0 else None, kind="pred"),
    Row("eq", EQ, [T(2), T(2)], lambda p, v: (v[0] - v[1]) % p == 0, kind="pred"),
    Row("packed_is_zero", PACKED_IS_ZERO, [W()], lambda p, v: v[0] in (0, p), kind="pred"),
    # ---- the stored form
    Row("pack_unpack", PACK_UNPACK, [W()], Res(None, None, exact=lambda p, v: v[0]), kind="words"),
    Row("to_internal", TO_INTERNAL, [W()], strict(lambda p, v: 32 * v[0]), note="x 2^266 / 2^261 for any 256-bit x (< 5.3p)"),
    Row("from_internal", FROM_INTERNAL, [T(2)], Res(None, None, exact=lambda p, v: v[0] * pow(32, -1, p) % p), kind="words"),
    # ---- Fp2T<Fq29> as the G2 formulas stack the forms: (c0, c1) per operand
    Row("fp2_mul", FP2_MUL, [T(4), T(4), T(2), T(2)],
        [strict(lambda p, v: mont(v[0] * v[2] - v[1] * v[3], p)), strict(lambda p, v: mont(v[0] * v[3] + v[1] * v[2], p))], ext=True,
        note="first operand: components of a sub_weak result; second strict"),
    Row("fp2_sqr", FP2_SQR, [T(4), T(4)],
        [strict(lambda p, v: mont(v[0] * v[0] - v[1] * v[1], p)), strict(lambda p, v: mont(2 * v[0] * v[1], p))], ext=True,
        note="a carry-free sum of two weak components (< 8p, limbs < 2^30) times a sub_weak4 result (< 8p)"),
    Row("fp2_mulsub2", FP2_MULSUB2, [T(4), T(4), T(4), T(4), T(2), T(2), T(2), T(2)],
        [strict(lambda p, v: mont(v[0] * v[2] - v[1] * v[3] - (v[4] * v[6] - v[5] * v[7]), p)),
         strict(lambda p, v: mont(v[0] * v[3] + v[1] * v[2] - (v[4] * v[7] + v[5] * v[6]), p))], ext=True,
        note="a, b weak (< 4p per component); c, d strict: mul4add with neg_weak4 / neg_weak operands"),
]
ROW = {r.name: r for r in ROWS}
# Public functions of Field29 without a row of their own, and why:
#   cond_sub_kp, maybe_kp   reached with every k they are called with through fold8 / fold16 / narrow and maybe_zero_weak / _wide
#   add_lazy                its result is valid inside a product only: row add_lazy_mul
#   cneg                    neg or the identity, chosen by the caller's flag
#   inv                     ~380 mul / sqr on strict values: the reference's inverse vectors run it (WSNARK_ST_INVERSE)
#   unpack, pack            row pack_unpack; from_words / zero / one / p_limb / kp_limb / p0_inv29 are compile-time constants, every
#                           row depends on them
#   keep                    an empty asm statement that pins registers: no value changes
STRICT_ROWS = ["add", "dbl", "sub", "neg", "fold4to2", "cond_sub_2p", "narrow", "mul_16p_2p", "sqr_10p", "mulsub2", "to_internal"]


def rows_for(which, impl):
    return [r.name for r in ROWS if not (r.ext and (which != 0 or impl == 3))]


# ---------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def cases(which, name):
    """(operand values per case, the launch's input array): built once per field and row, shared by every implementation"""
    row, p = ROW[name], PRIMES[which]
    rnd = random.Random(zlib.crc32(("%d/%s" % (which, name)).encode()))
    ops = row.opnds
    grids = [o.grid(p) for o in ops]
    rand_case = lambda: tuple(o.rand(p, rnd) for o in ops)
    cs = []
    full = 1
    for g in grids:
        full *= len(g)
    if len(ops) <= 2 or full <= 12000:
        cs += list(itertools.product(*grids))                                   # the full grid (x grid (x grid))
    if len(ops) > 2:
        cs.append(tuple(o.maxlimb(p) for o in ops))                             # all maximal: every limb 0..7 saturated
        cs.append(tuple(o.maxval(p) for o in ops))                              # ... and every value at its bound
        for i in range(len(ops)):                                               # each operand maximal, the rest random
            for m in (ops[i].maxlimb(p), ops[i].maxval(p)):
                for _ in range(4):
                    c = list(rand_case())
                    c[i] = m
                    cs.append(tuple(c))
        cs += [tuple(rnd.choice(g) for g in grids) for _ in range(N_SAMPLE)]    # a seeded sample of grid combinations
    if name == "add_lazy_mul":                                                  # every carry-free sum of two grid values, c cycling through its grid
        cs += [(a, b, grids[2][i % len(grids[2])]) for i, (a, b) in enumerate(itertools.product(grids[0], grids[1]))]
    cs += [rand_case() for _ in range(N_RANDOM)]
    arr = np.array([sum((o.enc(v) for o, v in zip(ops, c)), []) for c in cs], dtype=np.uint32)
    return cs, arr


def run(bn, which, impl, op, arr, out_words):
    n = arr.shape[0]
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    out = np.full((n, out_words), 0xA5A5A5A5, dtype=np.uint32)
    bn.lib.check(bn.lib.c.wsnark_selftest_field29(which, impl, op, arr.ctypes.data, out.ctypes.data, n))
    return out


def _fail(row, which, impl, what, c, got):
    return "%s (%s, impl %d): %s\n  operands: %s\n  result limbs: %s" % (row.name, FNAME[which], impl, what, [hex(x) for x in c], [hex(int(x)) for x in got])


def check_row(bn, which, impl, name):
    """runs one row and checks every case; returns the raw output (the GPU leg compares implementations limb for limb)"""
    row, p = ROW[name], PRIMES[which]
    cs, arr = cases(which, name)
    nres = len(row.res)
    out = run(bn, which, impl, row.op, arr, 9 * nres)
    if row.kind == "pred":
        f = row.res[0]
        for c, o in zip(cs, out.tolist()):
            want = f(p, c)
            assert o[0] in (0, 1) and not any(o[1:]), _fail(row, which, impl, "a predicate writes 0 or 1 in limb 0", c, o)
            assert want is None or bool(o[0]) == want, _fail(row, which, impl, "expected %s" % want, c, o)
        return out
    for c, o in zip(cs, out.tolist()):
        for j, r in enumerate(row.res):
            l = o[9 * j: 9 * j + 9]
            if row.kind == "words":
                assert value_words(l) == r.exact(p, c) and int(l[8]) == 0, _fail(row, which, impl, "stored form: expected 0x%x" % r.exact(p, c), c, l)
                continue
            v = value(l)
            assert (v - r.residue(p, c)) % p == 0, _fail(row, which, impl, "wrong residue (element %d)" % j, c, l)
            lo_ok = v > 0 if r.lo_open else v >= 0
            hi_ok = v <= r.hi * p if r.hi_closed else v < r.hi * p
            assert lo_ok and hi_ok, _fail(row, which, impl, "value / p = %.4f outside its interval (bound %d p)" % (v / p, r.hi), c, l)
            assert all(int(x) <= M29 for x in l[:8]), _fail(row, which, impl, "a limb of 2^29 or more", c, l)
            if r.hi <= 4 and not r.hi_closed:
                assert int(l[8]) < 1 << 24, _fail(row, which, impl, "top limb of 2^24 or more in a value that is packed next", c, l)
            if r.exact is not None:
                assert v == r.exact(p, c), _fail(row, which, impl, "expected the value 0x%x" % r.exact(p, c), c, l)
    return out


def check_zero_representatives(bn, which, impl):
    """is_zero on what the strict functions really return: true exactly where the residue is zero.  Sums and differences over the grid
    land on BOTH representatives of zero (a + b = 2p -> 0, a + b = p or 3p -> p; a - b = 0 -> 0, a - b = +-p -> p)."""
    p = PRIMES[which]
    for name in STRICT_ROWS:
        row = ROW[name]
        cs, arr = cases(which, name)
        out = run(bn, which, impl, row.op, arr, 9)
        flags = run(bn, which, impl, IS_ZERO, out, 9)
        seen = set()
        for c, o, f in zip(cs, out.tolist(), flags.tolist()):
            zero = row.res[0].residue(p, c) % p == 0
            assert bool(f[0]) == zero, _fail(row, which, impl, "is_zero of the result says %d" % f[0], c, o)
            if zero:
                seen.add(value(o))
        assert seen <= {0, p} and (name not in ("add", "sub") or seen == {0, p}), (name, seen)


def check_argument_errors(bn):
    one = np.zeros((1, 72), dtype=np.uint32)
    for which, impl, op in ((2, 0, MUL), (-1, 0, MUL), (0, 1, MUL), (0, 4, MUL), (0, 0, 39), (0, 0, -1), (1, 3, MUL), (1, 0, FP2_MUL), (0, 3, FP2_SQR)):
        out = np.zeros((1, 18), dtype=np.uint32)
        assert bn.lib.c.wsnark_selftest_field29(which, impl, op, one.ctypes.data, out.ctypes.data, 1) == 4, (which, impl, op)     # WSNARK_ERR_ARG
    assert bn.lib.c.wsnark_selftest_field29(0, 0, MUL, None, None, 1) == 4
    assert bn.lib.c.wsnark_selftest_field29(0, 0, MUL, None, None, 0) == 0


if __name__ == "__main__":
    for r in ROWS:
        print("%-20s op %2d  operands %-28s cases: Fq %6d%s" % (r.name, r.op, "x".join("W" if isinstance(o, W) else "%dp%s" % (o.k, "]" if o.closed else "") for o in r.opnds),
                                                              len(cases(0, r.name)[0]), "" if r.ext else "  Fr %6d" % len(cases(1, r.name)[0])))
    print("total: Fq %d, Fr %d" % (sum(len(cases(0, r.name)[0]) for r in ROWS), sum(len(cases(1, r.name)[0]) for r in ROWS if not r.ext)))
