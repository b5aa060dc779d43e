"""The accumulation loop's two straight-path mixed additions (csrc/curve.h: madd_fast on an XYZZ sum, mmadd_fast on a sum that is still
an affine point) through wsnark_selftest_curve ops 12 - 15, one step of the loop's fast half per lane, on every curve that has them:
the accumulation kernels' curves (impl 0), the saturated and the host curve (1, 2) and the inlined-product G1 (3).  Generic pairs:
the step accepts and the sum is Python-integer affine addition (tests/bn128_ref.py).  Planted corners -- q at infinity, p = q with
z = 1, p = q with another z, p = -q --: it refuses and the accumulator comes back bit for bit.  The corners sit between generic
pairs in ONE launch, so neighbouring lanes decide differently.  The refusal is a necessary test, not an exact one: a generic pair
the cheap test happens to flag may come back either way; such pairs are counted, and the fixed seeds have none.  On the CPU thread
emulator and (-m gpu) on the device."""
import random

import pytest

import bn128_ref as ref
from primitives_common import st_curve

BACKENDS = ["emul", pytest.param("gpu", marks=pytest.mark.gpu)]
Q, R = ref.Q, ref.R
IMPLS = {1: (0, 1, 2, 3), 2: (0, 1, 2)}
KINDS = ("generic", "q at infinity", "p = q, z = 1", "p = q, another z", "p = -q")
KINDS_AFFINE = ("generic", "q at infinity", "p = q, z = 1", "p = -q")          # mmadd_fast: p is an affine point

_bns = {}


def _bn(backend):
    if backend not in _bns:
        if backend == "emul":
            from emul_util import emul_bn128
            _bns[backend] = emul_bn128()
        else:
            import torch
            assert torch.cuda.is_available(), "GPU tests need a GPU"
            import __graft_entry__
            __graft_entry__.ensure_built()
            import wasmsnark_amd
            _bns[backend] = wasmsnark_amd.build(device=0)
    return _bns[backend]


# field elements as tuples of g components (Fq: one; Fq2 = Fq[u] / (u^2 + 1): two), plain integers
def _mul(a, b):
    if len(a) == 1:
        return (a[0] * b[0] % Q,)
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def _enc(a):
    return b"".join(ref.mont(v) for v in a)


def _el(g, v):
    return (v,) if g == 1 else tuple(v)


def _affine_bytes(g, pt):
    """the affine point (plain integers) as the triple (x, y, 1)"""
    return _enc(_el(g, pt[0])) + _enc(_el(g, pt[1])) + _enc((1,) + (0,) * (g - 1))


def _jac_bytes(g, pt, z):
    """the same point as (x z^2, y z^3, z)"""
    zz = _mul(z, z)
    return _enc(_mul(_el(g, pt[0]), zz)) + _enc(_mul(_el(g, pt[1]), _mul(zz, z))) + _enc(z)


def _neg(g, pt):
    return (pt[0], (Q - pt[1]) % Q if g == 1 else tuple((Q - c) % Q for c in pt[1]))


_points = {}


def _walk(g, count):
    """count distinct points a G + i b G, i = 0 .. (one affine addition each, Python integers)"""
    if g not in _points or len(_points[g]) < count:
        rnd = random.Random(777 + g)
        add, gen = (ref.g1_add, ref.G1) if g == 1 else (ref.g2_add, ref.G2)
        pt, step = ref.times(add, gen, rnd.randrange(1, R)), ref.times(add, gen, rnd.randrange(1, R))
        out = []
        for _ in range(count):
            out.append(pt)
            pt = add(pt, step)
        _points[g] = out
    return _points[g][:count]


def _vectors(g, n, seed, kinds):
    """n operand pairs cycling through the kinds (every corner sits between generic pairs): p and q as the hook takes them, the kind
    of each, and p and p + q as normalised triples by Python-integer arithmetic"""
    rnd = random.Random(seed)
    add = ref.g1_add if g == 1 else ref.g2_add
    pts = _walk(g, 2 * n)
    z = lambda: tuple(rnd.randrange(1, Q) for _ in range(g))
    unit = (1,) + (0,) * (g - 1)
    every_z = len(kinds) == len(KINDS)
    inf = bytes(32 * g) + _enc(unit) + bytes(32 * g)                                   # (0, 1, 0)
    P, Qs, ks, p_aff, sums = [], [], [], [], []
    for i in range(n):
        kind = kinds[0] if i % 2 == 0 else kinds[1 + (i // 2) % (len(kinds) - 1)]
        a, b = pts[2 * i], pts[2 * i + 1]
        zp = z() if every_z and kind != "p = q, z = 1" else unit
        if kind == "q at infinity":
            q, b = inf, None
        elif kind in ("p = q, z = 1", "p = q, another z"):
            q, b = _affine_bytes(g, a), a
        elif kind == "p = -q":
            b = _neg(g, a)
            q = _affine_bytes(g, b)
        else:
            q = _affine_bytes(g, b)
        P.append(_jac_bytes(g, a, zp)); Qs.append(q); ks.append(kind)
        p_aff.append(_affine_bytes(g, a))
        s = add(a, b)
        sums.append(inf if s is None else _affine_bytes(g, s))
    return P, Qs, ks, p_aff, sums


def _check(bn, g, impl, ops, kinds, n, seed):
    P, Qs, ks, p_aff, sums = _vectors(g, n, seed, kinds)
    assert all(sum(1 for k in ks if k == kind) >= 10 for kind in kinds)
    zero = st_curve(bn, g, impl, 3, [Qs[1]], [Qs[1]])[0]                       # infinity as this ABI writes it: (0, 1, 0)
    assert ks[1] == "q at infinity" and zero == Qs[1]
    assert st_curve(bn, g, impl, 3, P, P) == p_aff                             # (the operands are what the arithmetic above says)
    acc = st_curve(bn, g, impl, ops[0], P, Qs)                                  # the accumulator after the step
    flag = st_curve(bn, g, impl, ops[1], P, Qs)                                 # q where it accepted, infinity where it refused
    flagged = 0
    for i, kind in enumerate(ks):
        if kind == "generic":
            if flag[i] == zero:                                                 # the necessary test may flag a generic pair ...
                flagged += 1
                assert acc[i] == p_aff[i], (i, kind, "refused, and the accumulator changed")
            else:
                assert flag[i] == Qs[i], (i, kind)
                assert acc[i] == sums[i], (i, kind)
        else:
            assert flag[i] == zero, (i, kind, "accepted")
            assert acc[i] == p_aff[i], (i, kind, "the accumulator changed")
    assert flagged == 0, "%d generic pairs were refused: pick another seed" % flagged      # ... and these seeds have none
    # the corners alone, all lanes of a launch refusing, and the generic pairs alone, all accepting
    for want_generic in (False, True):
        idx = [i for i, k in enumerate(ks) if (k == "generic") == want_generic]
        sp, sq = [P[i] for i in idx], [Qs[i] for i in idx]
        assert st_curve(bn, g, impl, ops[0], sp, sq) == [sums[i] if want_generic else p_aff[i] for i in idx]
        assert st_curve(bn, g, impl, ops[1], sp, sq) == [Qs[i] if want_generic else zero for i in idx]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("g,impl", [(g, i) for g in (1, 2) for i in IMPLS[g]])
def test_madd_fast_step(backend, g, impl):
    """ops 12 / 13: an XYZZ sum with any z"""
    _check(_bn(backend), g, impl, (12, 13), KINDS, 201 if g == 1 else 101, 300 * g + impl)       # odd: the last lane alone in its tail


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("g,impl", [(g, i) for g in (1, 2) for i in IMPLS[g]])
def test_mmadd_fast_step(backend, g, impl):
    """ops 14 / 15: the sum is an affine point"""
    _check(_bn(backend), g, impl, (14, 15), KINDS_AFFINE, 201 if g == 1 else 101, 500 * g + impl)


@pytest.mark.parametrize("backend", BACKENDS)
def test_fast_step_arguments(backend):
    """ops 12 - 15 on a curve without these functions, mmadd_fast with a p that is not affine, an op past the list: WSNARK_ERR_ARG"""
    import ctypes as C
    bn = _bn(backend)
    for g in (1, 2):
        P, Qs, *_ = _vectors(g, 4, 9, KINDS)
        sz = len(P[0])
        out = (C.c_uint8 * (4 * sz))()
        call = lambda impl, op, p: bn.lib.c.wsnark_selftest_curve(g, impl, op, b"".join(p), b"".join(Qs), out, 4)
        affine = [st_curve(bn, g, 2, 3, [p], [p])[0] for p in P]
        for op in (12, 13, 14, 15):
            assert call(0, op, affine) == 0
            assert call(4 if g == 2 else 5, op, affine) == 4
            assert call(6 if g == 2 else 4, op, affine) == 4
        for op in (14, 15):
            assert call(0, op, P) == 4                                         # z != 1
            assert call(0, op, affine[:3] + [Qs[1]]) == 4                      # p at infinity: z = 0
        assert call(0, 16, affine) == 4 and call(0, 9, affine) == 4
