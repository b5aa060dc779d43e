"""The transform's digit plans (csrc/ntt.hip: 1 to 4 passes, the pass count a function of the size) with the pass count FORCED on small
inputs through the NTT_PASSES switch, so that the four-pass code -- the middle-digit reversal, the per-pass twiddle tables, CALC_H's
product on load and its combining store -- meets the oracle bit for bit; and two yardsticks in plain Python integers for the sizes
the oracle cannot reach: single outputs of a transform of planted values, and of CALC_H on a few non-zero rows, from the definition.

Shared by tests/test_emul_ntt_plans.py (CPU: the kernel sources under the thread emulator) and tests/test_gpu_ntt_plans.py (-m gpu).
Everything is exact integer arithmetic."""
import random
import struct

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
W28 = pow(5, (R - 1) >> 28, R)            # the transform's root of order 2^28 (src/build_fft.js:29-47)
MONT_INV = pow(1 << 256, R - 2, R)

# (passes, bits): digits bits / passes, the remainder on the leading ones -- (3,3,2,2) and (4,4,3,3) have unequal MIDDLE digits
FORCED_PLANS = [(4, 8), (4, 10), (4, 13), (4, 14), (3, 6), (3, 8), (3, 10), (2, 4), (2, 7), (2, 10)]
EXTREME_BITS = (10, 14)                   # these sizes also run the extreme patterns and the NTT_GLOBAL_TW=1 schedule
FORCED_CALC_H = [(p, d) for d in (8, 10, 12) for p in (2, 3, 4)]


def plan_digits(bits, passes):
    return [bits // passes + (1 if d < bits % passes else 0) for d in range(passes)]


def default_passes(bits):
    return 1 if bits <= 10 else 2 if bits <= 16 else 3 if bits <= 24 else 4


def root(bits):
    """w of order 2^bits."""
    return pow(W28, 1 << (28 - bits), R)


def le(v):
    return int(v).to_bytes(32, "little")


def _rand_fr(seed, n):
    rnd = random.Random(seed)
    return b"".join(rnd.randrange(R).to_bytes(32, "little") for _ in range(n))


class launches:
    """Kernel launch counts of the calls inside the block, from wsnark_timing_report."""

    def __init__(self, lib):
        self.lib = lib
        self.counts = {}

    def __enter__(self):
        self.lib.c.wsnark_timing_enable(1)
        self.lib.c.wsnark_timing_reset()
        return self

    def __exit__(self, *a):
        self.counts = {k: v[1] for k, v in self.lib.timing_report().items()}
        self.lib.c.wsnark_timing_reset()
        self.lib.c.wsnark_timing_enable(0)

    def passes(self):
        return (self.counts.get("ntt_pass", 0), self.counts.get("ntt_pass_last", 0))


def extreme_patterns(n):
    top, zero, one = le(R - 1), le(0), le(1)
    return [top * n, b"".join(top if (i & 1) else zero for i in range(n)), b"".join(top if i < n // 2 else one for i in range(n))]


def _all_variants_vs_oracle(bn, orc, x, n, tag):
    for odd in (0, 1):
        assert bn.fft(x, odd) == orc.fft(x, n, odd), tag + (odd, "forward")
        assert bn.ifft(x, odd) == orc.fft(x, n, odd, inverse=True), tag + (odd, "inverse")


def check_forced_plan(bn, orc, tune, passes, bits):
    """A transform of 2^bits in `passes` digit passes: forward and inverse, odd 0 and 1, against the oracle -- and the launch counts
    prove that the forced plan, not the default one, ran."""
    n = 1 << bits
    assert passes != default_passes(bits)
    tune(bn.lib, "NTT_PASSES", passes)
    x = orc.to_mont_n(_rand_fr(100 * passes + bits, n))
    with launches(bn.lib) as L:
        got = bn.fft(x, 0)
    assert L.passes() == (passes - 1, 1), (L.counts, plan_digits(bits, passes))
    assert got == orc.fft(x, n, 0)
    _all_variants_vs_oracle(bn, orc, x, n, (passes, bits, "random"))
    if bits in EXTREME_BITS:
        pats = extreme_patterns(n)
        for i, p in enumerate(pats):
            _all_variants_vs_oracle(bn, orc, p, n, (passes, bits, "extreme", i))
        tune(bn.lib, "NTT_GLOBAL_TW", 1)        # the passes' small twiddles from the global table instead of the LDS copy
        with launches(bn.lib) as L:
            _all_variants_vs_oracle(bn, orc, x, n, (passes, bits, "random, global twiddles"))
        assert L.passes() == (4 * (passes - 1), 4), L.counts
        for i, p in enumerate(pats):
            _all_variants_vs_oracle(bn, orc, p, n, (passes, bits, "extreme, global twiddles", i))


def check_default_plans(bn, sizes=(12,)):
    """The switch unset: the pass count is the size's own."""
    for bits in sizes:
        x = _rand_fr(bits, 1 << bits)
        with launches(bn.lib) as L:
            bn.fft(x, 0)
        assert L.passes() == (default_passes(bits) - 1, 1), (bits, L.counts)


# ------------------------------------------------------------------ CALC_H
def pols_bytes(per_signal):
    """per_signal: for every signal its list of (row, coefficient) records, in the key's column-major format."""
    out = bytearray()
    for recs in per_signal:
        out += struct.pack("<I", len(recs))
        for row, c in recs:
            out += struct.pack("<I", row) + le(c)
    return bytes(out)


def row_evals(signals, per_signal):
    """Row evaluations {row: sum of coefficient x signal}: plain signals, coefficients stored in the Montgomery form."""
    ev = {}
    for s, recs in zip(signals, per_signal):
        for row, c in recs:
            ev[row] = (ev.get(row, 0) + c * MONT_INV % R * s) % R
    return {k: v for k, v in ev.items() if v}


def random_pols(rnd, n_signals, dom, dense_rows=300):
    """The random sparse matrix of test_calc_h_vs_oracle (0-3 records per signal) and one signal with `dense_rows` records, repeated
    rows among them (a row's records of ONE signal add up like any others)."""
    per = []
    for s in range(n_signals - 1):
        per.append([(idx, rnd.randrange(R)) for idx in rnd.sample(range(dom), rnd.randrange(0, 4))])
    rows = [rnd.randrange(dom) for _ in range(dense_rows - 20)]
    rows += rows[:20]
    per.insert(rnd.randrange(n_signals), [(r, rnd.randrange(R)) for r in rows])
    return per


def check_forced_calc_h(bn, orc, tune, passes, dom_bits):
    """CALC_H on a domain of 2^dom_bits with its six transforms (four launches as batches of two) in `passes` passes, against the
    oracle: the product on load (pass-0 table x 2^10), the batch of two, the combining store of the last pass."""
    dom = 1 << dom_bits
    rnd = random.Random(1000 * passes + dom_bits)
    n_sig = 3 * dom // 4
    sig = b"".join(le(rnd.randrange(R)) for _ in range(n_sig))
    A, B = pols_bytes(random_pols(rnd, n_sig, dom)), pols_bytes(random_pols(rnd, n_sig, dom))
    want = orc.calc_h(sig, A, B, n_sig, dom)
    assert want[-32:] == bytes(32) and any(want)
    tune(bn.lib, "NTT_PASSES", passes)
    for batch, runs in ((1, 4), (0, 6)):            # transforms a and b as one batch of two, or one after the other
        tune(bn.lib, "CALCH_BATCH", batch)
        with launches(bn.lib) as L:
            got = bn.calcH(sig, A, B, n_sig, dom)
        assert L.passes() == (runs * (passes - 1), runs), (batch, L.counts)
        assert got == want, (passes, dom_bits, batch)


# ------------------------------------------------------------------ yardsticks in plain integers
def ntt_sparse(bits, x, odd, inverse, ks):
    """Outputs ks of the transform of the vector {position: value} (zero elsewhere), from the definition:
         forward  X[k] = sum_j x_j g^(odd j) w^(j k)
         inverse  X[k] = (1/n) sum_j x_j g^(odd j) w^(-j k)        (the inverse keeps the FORWARD coset factor)
       w of order n = 2^bits, g of order 2n.  Values are whatever representatives the caller uses (the transform is linear, so
       Montgomery forms go in and come out)."""
    n = 1 << bits
    w = root(bits)
    if inverse:
        w = pow(w, R - 2, R)
    g = root(bits + 1) if odd else 1
    terms = [(j, v * pow(g, j, R) % R) for j, v in sorted(x.items())]
    scale = pow(n, R - 2, R) if inverse else 1
    return [sum(c * pow(w, j * k % n, R) for j, c in terms) * scale % R for k in ks]


def calc_h_sparse(bits, a_ev, b_ev, ts):
    """CALC_H's outputs h[t], t in ts: coefficient n + t of A(x) B(x), where A and B are the polynomials of degree < n = 2^bits with
    A(w^k) = a_ev[k], B(w^l) = b_ev[l] (zero on the other rows).  With the Lagrange basis L_k = (1/n) sum_m w^(-k m) x^m:
         h[t] = n^-2 sum_{k,l} a_k b_l w^(-l t) G(k, l, t),    G = sum_{m = t+1}^{n-1} rho^m,  rho = w^(l - k)
              G = n - 1 - t                      (k == l)
              G = (1 - rho^(t+1)) / (rho - 1)    (otherwise: rho^n = 1)"""
    n = 1 << bits
    w = root(bits)
    wi = pow(w, R - 2, R)
    n2 = pow(n * n, R - 2, R)
    pairs = []
    for k, al in sorted(a_ev.items()):
        for l, be in sorted(b_ev.items()):
            c = al * be % R * n2 % R
            if k == l:
                pairs.append((l, c, None))
            else:
                rho = pow(w, (l - k) % n, R)
                pairs.append((l, c * pow(rho - 1, R - 2, R) % R, (l - k) % n))
    out = []
    for t in ts:
        acc = 0
        for l, c, dlk in pairs:
            G = (n - 1 - t) if dlk is None else 1 - pow(w, dlk * (t + 1) % n, R)
            acc += c * pow(wi, l * t % n, R) % R * G
        out.append(acc % R)
    return out


def check_ntt_sparse_pin(orc, bits):
    """ntt_sparse at every k against the oracle: planted values in an otherwise zero vector, and (2^4) a dense one."""
    n = 1 << bits
    rnd = random.Random(7 + bits)
    pos = sorted({0, 1, n // 2, n - 1} | {rnd.randrange(n) for _ in range(n if bits <= 4 else 6)})
    x = {j: rnd.randrange(R) for j in pos}
    buf = b"".join(le(x.get(j, 0)) for j in range(n))
    for odd in (0, 1):
        for inverse in (False, True):
            want = orc.fft(buf, n, odd, inverse=inverse)
            got = ntt_sparse(bits, x, odd, inverse, range(n))
            assert b"".join(le(v) for v in got) == want, (bits, odd, inverse)


def calc_h_pin_case(bits, seed):
    """5 rows per matrix: two signals meet in one row of A (and of B), one row is shared by A and B; rows 0 and n - 1 among them."""
    n = 1 << bits
    rnd = random.Random(seed)
    free = rnd.sample(range(1, n - 1), 6) if n > 8 else [1, 2, 3, 4, 5, 6]
    rows_a = [0, free[0], free[1], free[2], n - 1]
    rows_b = [free[2], free[3], free[4], free[5], n - 1 if n <= 8 else 0]
    n_sig = 6
    sig = [rnd.randrange(R) for _ in range(n_sig)]
    pa = [[(rows_a[i], rnd.randrange(R))] for i in range(5)] + [[(rows_a[1], rnd.randrange(R))]]     # signal 5 meets signal 1
    pb = [[(rows_b[i], rnd.randrange(R))] for i in range(5)] + [[(rows_b[3], rnd.randrange(R))]]
    return sig, pa, pb


def check_calc_h_sparse_pin(orc, bits):
    n = 1 << bits
    sig, pa, pb = calc_h_pin_case(bits, 50 + bits)
    a_ev, b_ev = row_evals(sig, pa), row_evals(sig, pb)
    assert len(a_ev) == 5 and len(b_ev) == 5 and set(a_ev) & set(b_ev)
    want = orc.calc_h(b"".join(le(s) for s in sig), pols_bytes(pa), pols_bytes(pb), len(sig), n)
    got = calc_h_sparse(bits, a_ev, b_ev, range(n))
    assert b"".join(le(v) for v in got) == want, bits
    assert got[n - 1] == 0 and any(got)


# ------------------------------------------------------------------ sample points for the real sizes
def planted_positions(bits, rnd):
    """0, 1, n/2, n - 1; one position with a single set bit inside every digit of the size's own plan; two random ones."""
    n = 1 << bits
    pos = [0, 1, n // 2, n - 1]
    hi = bits
    for k in plan_digits(bits, default_passes(bits)):      # digit 0 is the most significant part of the input index
        lo = hi - k
        pos.append(1 << (lo + k // 2))
        hi = lo
    pos += [rnd.randrange(n), rnd.randrange(n)]
    return sorted(set(pos))


def sample_indices(bits, rnd, count=4096, plus_minus=False):
    """0, 1, n/2, n - 1, every 2^j and 2^j - 1 (plus_minus: 2^j + 1 as well, and n - 2), seeded random indices up to `count`."""
    n = 1 << bits
    s = {0, 1, n // 2, n - 1}
    for j in range(bits + 1):
        s |= {v for v in ((1 << j) - 1, 1 << j) if 0 <= v < n}
        if plus_minus:
            s |= {v for v in ((1 << j) + 1,) if v < n}
    if plus_minus:
        s.add(n - 2)
    while len(s) < count:
        s.add(rnd.randrange(n))
    return sorted(s)
