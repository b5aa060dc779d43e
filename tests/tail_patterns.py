"""Planted bucket sums for the MSM reduction tail (msm.hip: msm_chunks, msm_chunks2, msm_tree, msm_rows and the host's Horner chain
in msm_finish_t).  Shared by tests/test_emul_tail_patterns.py (CPU: the kernel sources under the thread emulator) and
tests/test_gpu_tail_patterns.py (-m gpu: the device code on an MI355X).

A scalar s with 1 <= s <= NB = 2^(c-1) is recoded into the single digit s of window 0 with no carry (for_each_digit), so the pair
(P, b + 1) puts P into bucket b of window 0 and into nothing else -- on table plans too, where window 0 is table row 0, i.e. the
points themselves.  A test therefore chooses every bucket sum B_b = q_b G of the bucket set the tail reduces, and the sum of the
MSM is (sum_b (b + 1) q_b mod r) G: the closed form, computed with the oracle's double-and-add (never with mul_base).

The patterns plant what random sums essentially never show the tail's full additions: equal operands (the doubling branch),
opposite operands (the result is infinity) and infinity operands, in every chain of the tail, at chosen positions, in neighbouring
chunks (adjacent lanes, lane pairs, lane quads) at the same step."""
import random
from collections import namedtuple

from conftest import load_golden

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583

EMPTY = None          # a bucket target: no entry at all
CANCEL = "cancel"     # entries that sum to infinity: P and -P with the same scalar, or an x = 0 point (a target of 0 is planted so)

RUN_DBL, RUN_INF, ACC_DBL, ACC_INF = "run + B doubles", "run + B cancels", "acc + run doubles", "acc + run cancels"
SUM_DBL, SUM_INF = "sum + A doubles", "sum + A cancels"
CHAIN_KINDS = (RUN_DBL, RUN_INF, ACC_DBL, ACC_INF, None)     # None: a generic addition

Geometry = namedtuple("Geometry", "c flat NB tNB tP m1 J1 m2 m J logJ nsum reduce")


def tail_geometry(c, flat, chunk=None, tail_bits=None, tail_l2=None, l2_default=4):
    """The reduction tail's geometry as msm_plan_begin (msm.hip) derives it from the window width c, the plan kind (flat: a table plan,
    ONE bucket set; else per-window plans, one group per window) and the switches MSM_CHUNK / TAIL_BITS / TAIL_L2 (None: unset)."""
    NB = 1 << (c - 1)
    big = NB >= (1 << 18)
    ch = 4 if (flat and not big) else 8
    if chunk in (2, 4, 8, 16, 32):
        ch = chunk
    tbits = (15 if big else 11) if flat else 31
    if tail_bits is not None and 3 <= tail_bits <= 20:
        tbits = tail_bits
    tNB = NB if (tbits >= 31 or NB < (1 << tbits)) else 1 << tbits
    tP = NB // tNB
    if tP > 256:
        tP, tNB = 256, NB // 256
    m1 = min(tNB, ch)
    J1 = tNB // m1
    l2 = tail_l2 if tail_l2 is not None else (l2_default if flat and NB >= (1 << 17) else 1)
    m2 = l2 if (l2 in (2, 4, 8) and flat and tP > 1 and J1 >= 8 * l2) else 1
    J = J1 // m2
    logJ = (J - 1).bit_length()
    nsum = logJ + 1 + (1 if (flat or tP > 1) else 0) + (1 if m2 > 1 else 0)
    return Geometry(c, flat, NB, tNB, tP, m1, J1, m2, m1 * m2, J, logJ, nsum, tP > 1)


def expected_kernels(geo):
    """the tail kernels a sum of this geometry launches (the names of the library's per-kernel timing)"""
    k = {"msm_chunks", "msm_tree"}
    if geo.m2 > 1:
        k.add("msm_chunks2")
    if geo.reduce:
        k.add("msm_rows")
    return k


# ------------------------------------------------------------------ solved chains
def solve_chain(m, want, rnd, acc_last=True):
    """Values v_{m-1} .. v_0 (mod r, 0 = infinity) of one running-sum chain -- run += v_i; acc += run, for i from m - 1 down to 0
    (msm_chunks over a chunk's buckets; msm_chunks2's S' / W chain over its chunk sums, whose acc step stops at i = 1: acc_last
    False) -- such that step i takes the branch want(i) wherever the state allows it (want(i) = None, or a branch the state cannot
    take -- the run is infinity before the first entry --: a random generic value).  Returns (v indexed by i, {i: branch taken})."""
    v = [0] * m
    run = acc = 0
    got = {}
    for i in range(m - 1, -1, -1):
        kind = want(i)
        has_acc = acc_last or i > 0
        x = None
        if kind == RUN_DBL and run:
            x = run
        elif kind == RUN_INF and run:
            x = (-run) % R
        elif kind == ACC_DBL and has_acc and acc:
            x = (acc - run) % R           # the new run equals acc
        elif kind == ACC_INF and has_acc and acc:
            x = (-acc - run) % R          # the new run is -acc
        if x is None:
            x, kind = rnd.randrange(1, R), None
        v[i] = x
        if kind:
            got[i] = kind
        run = (run + x) % R
        if has_acc:
            acc = (acc + run) % R
    return v, got


def check_chain(v, acc_last=True):
    """the branches the chain's additions take, recomputed from the values alone: {(i, 'run' | 'acc'): 'dbl' | 'inf' | 'generic' |
    'operand at infinity'}"""
    def kind(a, b):
        if a == 0 or b == 0:
            return "operand at infinity"
        return "dbl" if a == b else "inf" if (a + b) % R == 0 else "generic"
    out = {}
    run = acc = 0
    for i in range(len(v) - 1, -1, -1):
        out[(i, "run")] = kind(run, v[i])
        run = (run + v[i]) % R
        if acc_last or i > 0:
            out[(i, "acc")] = kind(acc, run)
            acc = (acc + run) % R
    return out


def solve_sum(m, want, rnd):
    """msm_chunks2's A' chain: a = v_0; a += v_i for i = 1 .. m - 1; want(i) in (SUM_DBL, SUM_INF, None)."""
    v, tot, got = [0] * m, 0, {}
    for i in range(m):
        kind = want(i) if i else None
        x = None
        if kind == SUM_DBL and tot:
            x = tot
        elif kind == SUM_INF and tot:
            x = (-tot) % R
        if x is None:
            x, kind = rnd.randrange(1, R), None
        v[i] = x
        if kind:
            got[i] = kind
        tot = (tot + x) % R
    return v, got


def chunk_with_sums(m1, S, A, rnd):
    """bucket values q_0 .. q_{m1-1} of one msm_chunks chunk whose pair is (S = sum q_i, A = sum (i + 1) q_i): random above i = 1"""
    assert m1 >= 2
    q = [0, 0] + [rnd.randrange(1, R) for _ in range(m1 - 2)]
    s = (S - sum(q)) % R
    a = (A - sum((i + 1) * x for i, x in enumerate(q))) % R
    q[1] = (a - s) % R
    q[0] = (2 * s - a) % R
    return q


# ------------------------------------------------------------------ patterns (targets of the NB buckets of window 0 / the table's set)
def uniform(geo, rnd):
    """every bucket Q: equal operands in the second step of every running sum, at every LDS level of the trees, in the two halves of
    the unmasked rows, in msm_rows"""
    return [rnd.randrange(1, R)] * geo.NB


def alternating(geo, rnd):
    """+Q, -Q, ...: the running sums cancel to infinity inside a chain and go on"""
    q = rnd.randrange(1, R)
    return [q if b % 2 == 0 else R - q for b in range(geo.NB)]


def mirrored(geo, rnd):
    """the second half of every piece is the negation of its first: the chunk pairs of the tree's upper half cancel the lower half's
    (the half merge of the unmasked rows adds P + (-P), the masked rows' chains end on P + (-P))"""
    t = []
    h = geo.tNB // 2
    for v in range(geo.tP):
        lo = [rnd.randrange(1, R) for _ in range(h)]
        t += lo + [R - x for x in lo]
    return t


def mirrored_pieces(geo, rnd):
    """pieces tP/2 .. tP - 1 are the negations of pieces 0 .. tP/2 - 1: msm_rows adds P + (-P)"""
    assert geo.tP >= 2
    half = [rnd.randrange(1, R) for _ in range(geo.NB // 2)]
    return half + [R - x for x in half]


def _branches(v, acc_last=True):
    """{(branch, i)} of the doublings and cancellations a running-sum chain over the values v really meets (recomputed from the
    values alone, not from what the solver aimed at)"""
    out = set()
    for (i, step), k in check_chain(v, acc_last).items():
        if k in ("dbl", "inf"):
            out.add(({("run", "dbl"): RUN_DBL, ("run", "inf"): RUN_INF, ("acc", "dbl"): ACC_DBL, ("acc", "inf"): ACC_INF}[(step, k)], i))
    return out


def solved_chunks(geo, rnd):
    """every msm_chunks chain solved for the four branches: chunk j takes branch CHAIN_KINDS[(j - i) % 5] at step i, so that every
    branch sits at every position (the first step with a run, i = m - 2, down to the last, i = 0) and neighbouring chunks -- adjacent
    lanes / lane pairs -- take different branches at the same step.  Returns (targets, {(branch, i)})."""
    t, seen = [], set()
    for j in range(geo.NB // geo.m1):
        q, _ = solve_chain(geo.m1, lambda i: CHAIN_KINDS[(j - i) % 5], rnd)
        t += q
        seen |= _branches(q)
    return t, seen


def solved_chunks2(geo, rnd):
    """msm_chunks2's chains solved: the S' / W chain over the m2 chunk sums S_j of a group and the A' chain over their A_j, group k
    taking branch CHAIN_KINDS[(k - i) % 5] (S' / W) and (SUM_DBL, SUM_INF, None)[(k + i) % 3] (A') at position i -- neighbouring
    groups sit on neighbouring lane pairs / quads; the chunks themselves are solved for their (S_j, A_j).  Returns (targets,
    {(branch, i)})."""
    assert geo.m2 > 1
    t, seen = [], set()
    for k in range(geo.NB // (geo.m1 * geo.m2)):
        S, _ = solve_chain(geo.m2, lambda i: CHAIN_KINDS[(k - i) % 5], rnd, acc_last=False)
        A, _ = solve_sum(geo.m2, lambda i: (SUM_DBL, SUM_INF, None)[(k + i) % 3], rnd)
        for i in range(geo.m2):
            t += chunk_with_sums(geo.m1, S[i], A[i], rnd)
        seen |= _branches(S, acc_last=False)
        tot = A[0]
        for i in range(1, geo.m2):
            if A[i] == tot:
                seen.add((SUM_DBL, i))
            elif (A[i] + tot) % R == 0:
                seen.add((SUM_INF, i))
            tot = (tot + A[i]) % R
    return t, seen


def sparse_cancelled(geo, rnd, filled=False):
    """only the top (i = m - 1) or the bottom (i = 0) bucket of each chunk holds entries, alternately; they cancel (filled: every other
    one holds a value instead).  Run after a dense sum of the same geometry, so that the empty buckets' slots hold stale points."""
    t = [EMPTY] * geo.NB
    for j in range(geo.NB // geo.m1):
        b = j * geo.m1 + (geo.m1 - 1 if j % 2 == 0 else 0)
        t[b] = rnd.randrange(1, R) if (filled and j % 4 < 2) else CANCEL
    return t


def dense(geo, rnd):
    return [rnd.randrange(1, R) for _ in range(geo.NB)]


# ------------------------------------------------------------------ planting
def closed_form(targets):
    e = 0
    for b, q in enumerate(targets):
        if isinstance(q, int):
            e += (b + 1) * q
    return e % R


class Planter:
    """(scalars, points, expected) for bucket targets.  Points come from bn.mul_base (one batch per planting; -P with y negated on
    the host); expected from the oracle's double-and-add of the closed form."""

    def __init__(self, bn, orc, g, seed=0):
        self.bn, self.orc, self.g = bn, orc, g
        self.sz = 64 if g == 1 else 128
        self.gen = bytes.fromhex(load_golden("groups.json")["g%d" % g]["gen"])
        self.rnd = random.Random(seed)

    def neg(self, pt):
        out = bytearray(pt)
        h = self.sz // 2
        for o in range(h, self.sz, 32):
            y = int.from_bytes(pt[o:o + 32], "little")
            out[o:o + 32] = ((Q - y) % Q).to_bytes(32, "little")
        return bytes(out)

    def expected(self, e):
        return self.orc.g_affine(self.g, self.orc.g_times_scalar(self.g, self.gen, e.to_bytes(32, "little")))

    def plant(self, targets, shuffle=True):
        """targets[b]: an int q (the bucket sums to q G; 0 is planted as CANCEL), EMPTY or CANCEL.  Returns (scalars, points, expected,
        number of pairs); the pairs in a seeded random order (shuffle) or bucket by bucket."""
        rnd = self.rnd
        pairs = []                                     # (bucket, key): key = (k, negate) or "inf"
        cancel_k = rnd.randrange(1, R)
        for b, q in enumerate(targets):
            if q is EMPTY:
                continue
            if q == CANCEL or q == 0:
                if b % 3 == 2:
                    pairs.append((b, "inf"))                                  # an x = 0 point
                else:
                    k = cancel_k if b % 3 == 0 else rnd.randrange(1, R)
                    pairs += [(b, (k, False)), (b, (k, True))]               # P and -P with the same scalar
                continue
            k = min(q, R - q)
            pairs.append((b, (k, k != q)))
        if shuffle:
            rnd.shuffle(pairs)
        ks = sorted({key[0] for _, key in pairs if key != "inf"})
        pts = self.bn.mul_base(self.g, b"".join(k.to_bytes(32, "little") for k in ks)) if ks else b""
        at = {k: pts[i * self.sz:(i + 1) * self.sz] for i, k in enumerate(ks)}
        negs = {}
        inf = bytes(self.sz)
        out = []
        for _, key in pairs:
            if key == "inf":
                out.append(inf)
            elif key[1]:
                if key[0] not in negs:
                    negs[key[0]] = self.neg(at[key[0]])
                out.append(negs[key[0]])
            else:
                out.append(at[key[0]])
        scalars = b"".join((b + 1).to_bytes(32, "little") for b, _ in pairs)
        return scalars, b"".join(out), self.expected(closed_form(targets)), len(pairs)


def catalogue(geo, rnd):
    """[(name, targets, planted branches or None)] of every pattern that applies to the geometry (the sparse cases are separate:
    they need a dense sum before them)"""
    cases = [("uniform", uniform(geo, rnd), None), ("alternating", alternating(geo, rnd), None), ("mirrored", mirrored(geo, rnd), None)]
    if geo.tP >= 2:
        cases.append(("mirrored pieces", mirrored_pieces(geo, rnd), None))
    t, seen = solved_chunks(geo, rnd)
    cases.append(("solved chunks", t, seen))
    if geo.m2 > 1:
        t, seen = solved_chunks2(geo, rnd)
        cases.append(("solved chunks2", t, seen))
    return cases


def assert_branches_planted(geo, name, seen):
    """the solved chains really hold every branch at the first position that can take it and at the last one (a chain's first
    step only meets an operand at infinity: the run starts there)"""
    if name == "solved chunks":
        m = geo.m1
        for kind in (RUN_DBL, RUN_INF, ACC_DBL, ACC_INF):
            assert (kind, m - 2) in seen and (kind, 0) in seen, (name, kind, sorted(seen))
    elif name == "solved chunks2":
        m = geo.m2
        for kind in (RUN_DBL, RUN_INF):
            assert (kind, m - 2) in seen and (kind, 0) in seen, (name, kind, sorted(seen))
        if m > 2:                                      # (W's last step is at i = 1: with two chunk pairs it only starts the chain)
            for kind in (ACC_DBL, ACC_INF):
                assert (kind, m - 2) in seen and (kind, 1) in seen, (name, kind, sorted(seen))
        for kind in (SUM_DBL, SUM_INF):
            assert (kind, 1) in seen and (kind, m - 1) in seen, (name, kind, sorted(seen))


class Timing:
    """which kernels a call launched: the library's per-kernel timing (names of every launch)"""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.lib.c.wsnark_timing_enable(1)
        self.lib.c.wsnark_timing_reset()
        return self

    def kernels(self):
        return {k for k in self.lib.timing_report() if k.startswith("msm_chunks") or k in ("msm_tree", "msm_rows")}

    def __exit__(self, *a):
        self.lib.c.wsnark_timing_reset()
        self.lib.c.wsnark_timing_enable(0)


# ------------------------------------------------------------------ mul_base (fixedbase.hip) against the oracle
def mul_base_scalars(rnd, n_random):
    """edge scalars of a 256-bit double-and-add (0, 1, 2, r - 1, r, r + 1, 2^255, 2^256 - 1, long runs of ones and of zeros, single
    top bits) and n_random seeded values below 2^256, as 32-byte little-endian words"""
    top = (1 << 256) - 1
    edge = [0, 1, 2, 3, R - 1, R, R + 1, 2 * R, 5 * R, 5 * R + 7, 1 << 255, top, top - 1, (1 << 255) - 1]
    for k in (1, 8, 63, 64, 65, 127, 128, 200, 251, 252, 253, 254):
        edge += [1 << k, (1 << k) - 1, top ^ ((1 << k) - 1), top >> k]
    for w in (1, 4, 8, 16, 32, 64):                    # alternating runs of w ones and w zeros, both phases
        pat = int(("1" * w + "0" * w) * (256 // (2 * w) + 1), 2) & top
        edge += [pat, pat ^ top]
    vals = edge + [rnd.randrange(1 << 256) for _ in range(n_random // 2)] + [rnd.randrange(R) for _ in range(n_random - n_random // 2)]
    return b"".join(v.to_bytes(32, "little") for v in vals)


def oracle_mul_base(orc, g, scalars):
    """affine k G from the oracle (x = 0 for infinity): the layout bn.mul_base returns"""
    sz = 64 if g == 1 else 128
    gen = bytes.fromhex(load_golden("groups.json")["g%d" % g]["gen"])
    out = []
    for i in range(0, len(scalars), 32):
        p = orc.g_affine(g, orc.g_times_scalar(g, gen, scalars[i:i + 32]))
        out.append(bytes(sz) if orc.g_is_zero(g, p) else p[:sz])
    return b"".join(out)
