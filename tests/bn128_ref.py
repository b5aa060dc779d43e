"""The pure-Python reference of the tests: BN128 in Python integers.  Fq and Fq2 = Fq[u]/(u^2 + 1), affine addition with every
case on G1 (y^2 = x^3 + 3) and on the twist (y^2 = x^3 + 3/(9 + u)), double-and-add, and the helpers between integers and the
32-byte little-endian Montgomery words of a key.  The yardstick of test_verify.py and of the *_common.py modules; it shares no
code with the library."""

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = 1 << 256
RINV = pow(MONT, Q - 2, Q)
G1 = (1, 2)
G2 = ((10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634),
      (8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531))


# ---- Fq2: pairs (c0, c1) = c0 + c1 u ----
def _f2_add(a, b):
    return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)


def _f2_sub(a, b):
    return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)


def _f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def _f2_inv(a):
    n = pow((a[0] * a[0] + a[1] * a[1]) % Q, -1, Q)
    return (a[0] * n % Q, (-a[1]) * n % Q)


def _f2_sqrt(a):
    """sqrt in Fq[u]/(u^2 + 1), q = 3 mod 4 (complex method); None if a is not a square."""
    if a == (0, 0):
        return (0, 0)
    norm = (a[0] * a[0] + a[1] * a[1]) % Q
    s = pow(norm, (Q + 1) // 4, Q)
    if s * s % Q != norm:
        return None
    half = pow(2, Q - 2, Q)
    for sign in (1, -1):
        t = (a[0] + sign * s) * half % Q
        x0 = pow(t, (Q + 1) // 4, Q)
        if x0 * x0 % Q == t and x0:
            x1 = a[1] * pow(2 * x0 % Q, Q - 2, Q) % Q
            if _f2_mul((x0, x1), (x0, x1)) == (a[0] % Q, a[1] % Q):
                return (x0, x1)
    return None


B2_TWIST = _f2_mul((3, 0), _f2_inv((9, 1)))


# ---- the two curves: affine points as tuples, None is the point at infinity ----
def g1_add(p, q):
    """Affine addition on y^2 = x^3 + 3 with every case."""
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % Q == 0:
            return None
        lam = 3 * p[0] * p[0] * pow(2 * p[1], -1, Q) % Q
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, Q) % Q
    x = (lam * lam - p[0] - q[0]) % Q
    return (x, (lam * (p[0] - x) - p[1]) % Q)


def g2_add(p, q):
    """Affine addition on the twist with every case."""
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if _f2_add(p[1], q[1]) == (0, 0):
            return None
        lam = _f2_mul(_f2_mul((3, 0), _f2_mul(p[0], p[0])), _f2_inv(_f2_mul((2, 0), p[1])))
    else:
        lam = _f2_mul(_f2_sub(q[1], p[1]), _f2_inv(_f2_sub(q[0], p[0])))
    x = _f2_sub(_f2_sub(_f2_mul(lam, lam), p[0]), q[0])
    return (x, _f2_sub(_f2_mul(lam, _f2_sub(p[0], x)), p[1]))


def times(add, pt, k):
    """k * pt by double-and-add, most significant bit first; k = 0 gives infinity."""
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, pt)
    return acc


def g1_mul(pt, k):
    return times(g1_add, pt, k)


def g2_mul(pt, k):
    return times(g2_add, pt, k)


class FixedBase:
    """k * pt for many k: the doublings 2^i pt once, then one addition per set bit of k (the same affine additions as times)."""

    def __init__(self, add, pt, bits=254):
        self.add, self.pow2 = add, [pt]
        for _ in range(bits - 1):
            self.pow2.append(add(self.pow2[-1], self.pow2[-1]))

    def mul(self, k):
        assert 0 <= k < 1 << len(self.pow2)
        acc = None
        for i, p in enumerate(self.pow2):
            if (k >> i) & 1:
                acc = self.add(acc, p)
        return acc


def g2_times_r_is_infinity(pt):
    return g2_mul(pt, R) is None


def g1_on_curve(x, y):
    return y * y % Q == (x ** 3 + 3) % Q


def g2_on_twist(x, y):
    return _f2_mul(y, y) == _f2_add(_f2_mul(_f2_mul(x, x), x), B2_TWIST)


def twist_point_outside_g2():
    """(x, y) on the twist y^2 = x^3 + 3/(9 + u), almost surely not in the order-r subgroup (the cofactor is ~2^254)."""
    k = 1
    while True:
        x = (k, 7 * k + 1)
        y = _f2_sqrt(_f2_add(_f2_mul(_f2_mul(x, x), x), B2_TWIST))
        if y is not None:
            return x, y
        k += 1


def random_twist_point(rnd):
    """A point of the whole twist group E'(Fq2) (order r (2q - r)) with x drawn from `rnd`; the y of the two that _f2_sqrt gives."""
    while True:
        x = (rnd.randrange(Q), rnd.randrange(Q))
        y = _f2_sqrt(_f2_add(_f2_mul(_f2_mul(x, x), x), B2_TWIST))
        if y is not None and y != (0, 0):
            return x, y


def twist_point_of_order(d, rnd):
    """A twist point of exact order d, d a product of distinct primes of the cofactor 2q - r = 10069 * 5864401 * ...: the
    multiple r (2q - r) / d of a random twist point, drawn again until no proper divisor of d kills it."""
    n = R * (2 * Q - R)
    assert n % d == 0
    primes = [p for p in (10069, 5864401) if d % p == 0]
    assert primes and d == (primes[0] if len(primes) == 1 else primes[0] * primes[1])
    while True:
        pt = g2_mul(random_twist_point(rnd), n // d)
        if pt is not None and all(g2_mul(pt, d // p) is not None for p in primes):
            assert g2_mul(pt, d) is None and g2_on_twist(*pt)
            return pt


# ---- integers <-> the 32-byte little-endian words of a key (Montgomery form, 2^256) ----
def le(v):
    return int(v).to_bytes(32, "little")


def mont(v):
    return le(int(v) * MONT % Q)


def from_mont(b):
    return int.from_bytes(b, "little") * RINV % Q
