"""The reduction tail's straight-path addition (csrc/curve.h and csrc/curve_pair.h: add_fast) against the full addition add(), through
wsnark_selftest_curve ops 10 / 11, on every curve that has it: the one-lane curves msm_chunks runs on (G1: impl 3; G2 on lane pairs:
impl 4), the accumulation kernels' curves, the saturated and the host curve, and the two lane-split curves of msm_chunks2 (G1 on two
lanes: impl 5; G2 on four: impl 6).  Random finite pairs with non-unit z: it must accept and give add()'s sum.  Planted corners --
either operand at infinity, P = Q (the same z and another one), P = -Q --: it must refuse and leave the accumulator as it was.  The
corners sit between generic pairs in ONE launch, so neighbouring lanes / lane pairs / quads decide differently.  On the CPU thread
emulator and (-m gpu) on the device."""
import random

import pytest

from primitives_common import st_curve

BACKENDS = ["emul", pytest.param("gpu", marks=pytest.mark.gpu)]
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % Q
IMPLS = {1: (0, 1, 2, 3, 5), 2: (0, 1, 2, 4, 6)}
KINDS = ("generic", "p at infinity", "q at infinity", "both at infinity", "p = q", "p = q, another z", "p = -q")

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


def _dec(b):
    """Montgomery bytes -> Montgomery integers, kept as they are: x_mont * z (z plain) is the Montgomery form of x z"""
    return tuple(int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32))


def _enc(a):
    return b"".join(int(v).to_bytes(32, "little") for v in a)


def _jac(aff, z):
    """the affine point (Montgomery bytes x | y) as the Jacobian triple (x z^2, y z^3, z) for a plain z != 0"""
    h = len(aff) // 2
    x, y = _dec(aff[:h]), _dec(aff[h:])
    zz = _mul(z, z)
    zm = tuple(v * MONT % Q for v in z)
    return _enc(_mul(x, zz)) + _enc(_mul(y, _mul(zz, z))) + _enc(zm)


def _neg(jac):
    t = len(jac) // 3
    return jac[:t] + _enc(tuple((Q - v) % Q for v in _dec(jac[t:2 * t]))) + jac[2 * t:]


def _vectors(bn, g, n, seed):
    """n operand pairs cycling through KINDS (so that every corner sits between generic pairs), with the kind of each"""
    rnd = random.Random(seed)
    sz = 64 if g == 1 else 128
    pts = bn.mul_base(g, b"".join(rnd.randrange(1, R).to_bytes(32, "little") for _ in range(2 * n)))
    aff = [pts[i * sz:(i + 1) * sz] for i in range(2 * n)]
    z = lambda: tuple(rnd.randrange(1, Q) for _ in range(g))
    inf = bytes(32 * g) + (1).to_bytes(32, "little") + bytes(32 * (g - 1)) + bytes(32 * g)      # (0, anything, 0)
    P, Qs, kinds = [], [], []
    for i in range(n):
        kind = KINDS[0] if i % 2 == 0 else KINDS[1 + (i // 2) % (len(KINDS) - 1)]
        p, q = _jac(aff[2 * i], z()), _jac(aff[2 * i + 1], z())
        if kind == "p at infinity":
            p = inf
        elif kind == "q at infinity":
            q = inf
        elif kind == "both at infinity":
            p = q = inf
        elif kind == "p = q":
            q = p
        elif kind == "p = q, another z":
            q = _jac(aff[2 * i], z())
        elif kind == "p = -q":
            q = _neg(_jac(aff[2 * i], z()))
        P.append(p); Qs.append(q); kinds.append(kind)
    return P, Qs, kinds


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("g,impl", [(g, i) for g in (1, 2) for i in IMPLS[g]])
def test_add_fast_against_add(backend, g, impl):
    bn = _bn(backend)
    n = 601 if g == 1 else 301                    # odd: the last vector's lanes alone in their wavefront's tail
    P, Qs, kinds = _vectors(bn, g, n, 100 * g + impl)
    assert all(sum(1 for k in kinds if k == kind) >= (40 if g == 1 else 20) for kind in KINDS)
    zero = bytes(32 * g) + (1).to_bytes(32, "little") + bytes(32 * (g - 1)) + bytes(32 * g)
    zero = st_curve(bn, g, impl, 3, [zero], [zero])[0]                      # infinity as this ABI writes it: (0, 1, 0)
    full = st_curve(bn, g, impl, 0, P, Qs)                                  # add()
    p_norm = st_curve(bn, g, impl, 3, P, P)
    q_norm = st_curve(bn, g, impl, 3, Qs, Qs)
    acc = st_curve(bn, g, impl, 10, P, Qs)                                   # the accumulator after add_fast
    flag = st_curve(bn, g, impl, 11, P, Qs)                                 # q where it accepted, infinity where it refused
    for i, kind in enumerate(kinds):
        if kind == "generic":
            assert flag[i] == q_norm[i] != zero, (i, kind, "refused")
            assert acc[i] == full[i], (i, kind)
        else:
            assert flag[i] == zero, (i, kind, "accepted")
            assert acc[i] == p_norm[i], (i, kind, "the accumulator changed")
    # the corners alone, all lanes of a launch refusing, and the generic pairs alone, all accepting
    for want_generic in (False, True):
        idx = [i for i, k in enumerate(kinds) if (k == "generic") == want_generic]
        sp, sq = [P[i] for i in idx], [Qs[i] for i in idx]
        assert st_curve(bn, g, impl, 10, sp, sq) == [full[i] if want_generic else p_norm[i] for i in idx]
        assert st_curve(bn, g, impl, 11, sp, sq) == [q_norm[i] if want_generic else zero for i in idx]
