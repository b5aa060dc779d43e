"""A reference model of the MSM's grouping pass and task planner (msm.hip: for_each_digit and its unrolled copy in presort_scatter_once,
presort_count / scan / scatter / bins, msm_plan_emit / emit_hot), planted scalars that reach every hard boundary of the planner by
construction, and an exact comparison of what the kernels wrote (wsnark_selftest_msm_plan, bn.msm_plan) with the model.  Shared by
tests/test_emul_grouping_patterns.py (CPU: the kernel sources under the thread emulator) and tests/test_gpu_grouping_patterns.py
(-m gpu: the device code on an MI355X).

A scalar built from chosen signed digits, s = sum_w d_w 2^(c w) with every |d_w| <= NB = 2^(c-1) and 0 <= s < r, is recoded into exactly
those digits (the recoding is unique), so a load list (window, digit, sign, count) chooses the length of every bucket.  A negative
digit -d at window w needs s >= 0, so the planter puts a +1 into window w + 1 behind it (its bucket's load is part of the model like any
other); the top window takes no negative digit.

What the model fixes is what the accumulation and the combine rely on: the multiset of entries of every bucket, tasks that tile the
buckets in runs of at most lmax, one partial slot per task of a split bucket, consecutive slots per bucket, longest-first order by
the length key.  It does NOT fix the order of entries inside a bucket, the order of tasks of equal key, which of a split bucket's
consecutive slots takes which of its runs, the order of the MultiBucket / HotBucket records or which hot bucket gets which slice
base: the kernels hand those out with atomics, and nothing downstream reads them.

Not reached here: the second trip of the hot combine's slice loop needs nt > 256 * 512 tasks in one bucket; that stays with
test_msm_full_size_adversarial_closed_forms (tests/test_gpu_parity.py)."""
import random
from collections import Counter, namedtuple

from conftest import load_golden

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
PARTIAL_FLAG = 0x80000000
HOT_MIN, HOT_SLICE, WAVE_COMBINE_MIN, PRESORT_ONCE_W, PRESORT_MAX_BINS, PRESORT_MAX_LO = 1024, 512, 17, 16, 4096, 10


def le32(v):
    return v.to_bytes(32, "little")


def windows(c):
    return -(-255 // c)


def digits(raw, c, Wall):
    """The signed c-bit digits of raw mod r, least significant window first: the balanced remainder of each step, except that the
    remainder NB itself stays positive (so every digit is in [-(NB - 1), NB]); sum_w d_w 2^(c w) == raw mod r."""
    s, NB, out = raw % R, 1 << (c - 1), []
    for _ in range(Wall):
        if s == 0:                                    # nothing left: the remaining digits are zero
            out += [0] * (Wall - len(out))
            break
        d = s % (1 << c)
        if d > NB:
            d -= 1 << c
        s = (s - d) >> c
        out.append(d)
    assert s == 0, "the windows do not hold the scalar"
    return out


def len_key(length, lmax):
    return min(255, max(1, -(-length * 255 // lmax)))


def owned(info):
    return [w for w in range(info["Wall"]) if w >= info["w_off"] and (w - info["w_off"]) % info["w_stride"] == 0]


def plan_geometry(n, c, flat=False, shard=(0, 1), lmax=None, hot_min=None, entry64=False):
    """The info words a plan of n scalars must echo, from the window width, the plan kind, the shard and the forced switches (MSM_LMAX,
    MSM_HOT_MIN, MSM_ENTRY64), as msm_plan_begin / msm_plan_finish derive them.  Sizes of the tests only: 4-byte entries always fit."""
    assert lmax is not None, "the cases force MSM_LMAX"
    Wall, NB = windows(c), 1 << (c - 1)
    off, stride = shard
    W = (Wall - off + stride - 1) // stride if off < Wall else 0
    Wb = 1 if flat else W
    lo = min(8, c - 1)
    while Wb * (NB >> lo) > PRESORT_MAX_BINS and lo < c - 1 and lo < PRESORT_MAX_LO:
        lo += 1
    while flat and (NB >> lo) < 2048 and lo > 7:
        lo -= 1
    idx_bits = max(1, ((Wall * n if flat else n) - 1).bit_length())
    assert idx_bits + 1 + lo <= 32
    nbins = Wb * (NB >> lo)
    bthr = min(1024, max(64, (n * W // nbins // 8 + 63) // 64 * 64))
    return {"c": c, "Wall": Wall, "W": W, "w_off": off, "w_stride": stride, "NB": NB, "nbuckets": NB if flat else W * NB, "flat": int(flat),
            "lmax": lmax, "hot_min": hot_min or HOT_MIN, "lo_bits": lo, "idx_bits": idx_bits, "nbins": nbins, "e32": int(not entry64),
            "once": int(Wall <= PRESORT_ONCE_W), "bthr": bthr, "n": n}


def expected_buckets(scalars, info, mask=None):
    """{bucket: Counter of index | sign << 31} for the scalars (ints) under the plan's geometry: per-window plans put digit d of owned
    window k (local index) into bucket k NB + |d| - 1 with entry index i; flat plans put every owned window's digit into bucket |d| - 1
    with entry index window n + i.  Pairs with mask[i] == 0 are left out."""
    c, Wall, NB, n, flat = info["c"], info["Wall"], info["NB"], len(scalars), info["flat"]
    own = owned(info)
    out = {}
    for i, s in enumerate(scalars):
        if mask is not None and not mask[i]:
            continue
        ds = digits(s, c, Wall)
        for k, w in enumerate(own):
            d = ds[w]
            if d:
                b = (abs(d) - 1) if flat else k * NB + abs(d) - 1
                e = ((w * n + i) if flat else i) | ((1 << 31) if d < 0 else 0)
                out.setdefault(b, Counter())[e] += 1
    return out


def model_stats(scalars, info, mask=None):
    """what the planner must count, from the model alone: {bucket: load}, {bucket: tasks}, and the bins' loads"""
    want = expected_buckets(scalars, info, mask)
    loads = {b: sum(cn.values()) for b, cn in want.items()}
    nts = {b: -(-v // info["lmax"]) for b, v in loads.items()}
    bins = Counter()
    for b, v in loads.items():
        bins[b >> info["lo_bits"]] += v
    return {"loads": loads, "nts": nts, "bins": bins, "want": want}


def check_plan(dump, scalars, mask=None, st=None):
    """Everything bn.msm_plan returned against the model; exact.  Returns the model's statistics (st: those of model_stats for the
    same scalars, info words and mask, when the caller has them already)."""
    info = dump["info"]
    lmax, hot_min, nb = info["lmax"], info["hot_min"], info["nbuckets"]
    st = st or model_stats(scalars, info, mask)
    want, loads, nts = st["want"], st["loads"], st["nts"]
    bstart, bend, vals = dump["bstart"], dump["bend"], dump["vals"]
    assert len(bstart) == len(bend) == nb and len(vals) == info["nvals"]
    # 1. every bucket holds its multiset; the ranges are disjoint and hold every entry
    assert all(s <= e <= len(vals) for s, e in zip(bstart, bend)), "a bucket range out of order or past the end"
    assert {b for b, (s, e) in enumerate(zip(bstart, bend)) if s != e} == set(want), "the non-empty buckets (an empty one has bstart == bend)"
    ranges = []
    for b in want:
        s, e = bstart[b], bend[b]
        assert Counter(vals[s:e]) == want[b], ("bucket contents", b, sorted(vals[s:e])[:8], sorted(want[b].elements())[:8])
        ranges.append((s, e))
    ranges.sort()
    assert all(ranges[i][1] <= ranges[i + 1][0] for i in range(len(ranges) - 1)), "bucket ranges overlap"
    total = sum(loads.values())
    assert sum(e - s for s, e in ranges) == total
    if mask is None:
        assert len(vals) == total and (not ranges or (ranges[0][0] == 0 and all(ranges[i][1] == ranges[i + 1][0] for i in range(len(ranges) - 1))))
    # 4. the task array: counters[3] entries, every one of a non-empty bucket, no longer than lmax, longest key first
    tasks = dump["tasks"]
    assert len(tasks) == info["tasks"] == sum(nts.values()), ("task count", len(tasks), info["tasks"], sum(nts.values()))
    keys = [len_key(t[2], lmax) for t in tasks]
    assert all(1 <= t[2] <= lmax for t in tasks), "a task longer than lmax, or empty"
    assert all(keys[i] >= keys[i + 1] for i in range(len(keys) - 1)), "tasks are not ordered longest key first"
    plain = {}
    partial = {}
    for dst, s, ln in tasks:
        if dst & PARTIAL_FLAG:
            assert (dst & ~PARTIAL_FLAG) not in partial, ("a partial slot used twice", dst & ~PARTIAL_FLAG)
            partial[dst & ~PARTIAL_FLAG] = (s, ln)
        else:
            assert dst not in plain, ("two tasks write one bucket", dst)
            plain[dst] = (s, ln)
    # 2. plain tasks: exactly the buckets of 1 .. lmax entries, each over its whole range
    assert plain == {b: (bstart[b], v) for b, v in loads.items() if v <= lmax}, "plain tasks"
    # 3. split buckets: nt tasks tiling the range, on consecutive slots of one MultiBucket / HotBucket record
    assert sorted(partial) == list(range(info["partial_slots"])), "partial slots are not a permutation of 0 .. counters[0] - 1"
    assert info["partial_slots"] == sum(v for v in nts.values() if v > 1)
    recs = {}
    for b, fp, nt in dump["multi"]:
        assert b not in recs and nt < hot_min, ("multi record", b, nt)
        recs[b] = (fp, nt)
    slices = []
    for b, fp, nt, task_base, rem_index, s, rem, slice_base in dump["hot"]:
        assert b not in recs and nt >= hot_min, ("hot record", b, nt)
        recs[b] = (fp, nt)
        assert s == bstart[b] and rem == loads[b] - (nt - 1) * lmax, ("hot record range", b)
        assert sorted(tasks[task_base + k] for k in range(nt - 1)) == [(PARTIAL_FLAG | (fp + k), s + k * lmax, lmax) for k in range(nt - 1)]
        assert tasks[rem_index] == (PARTIAL_FLAG | (fp + nt - 1), s + (nt - 1) * lmax, rem)
        slices.append((slice_base, slice_base + -(-nt // HOT_SLICE)))
    assert set(recs) == {b for b, v in nts.items() if v > 1}, "records of the split buckets"
    for b, (fp, nt) in recs.items():
        assert nt == nts[b], ("tasks of a split bucket", b, nt, nts[b])
        runs = [(bstart[b] + k * lmax, lmax) for k in range(nt - 1)] + [(bstart[b] + (nt - 1) * lmax, loads[b] - (nt - 1) * lmax)]
        assert sorted(partial[fp + k] for k in range(nt)) == runs, ("runs of a split bucket", b)
    # 5. the counters, and the hot buckets' slices
    assert info["multi_buckets"] == len(dump["multi"]) == sum(1 for v in nts.values() if 1 < v < hot_min)
    assert info["hot_buckets"] == len(dump["hot"]) == sum(1 for v in nts.values() if v >= hot_min)
    assert info["hot_slices"] == sum(-(-v // HOT_SLICE) for v in nts.values() if v >= hot_min)
    slices.sort()
    assert [s for s, _ in slices] == ([0] + [e for _, e in slices[:-1]] if slices else []) and (not slices or slices[-1][1] == info["hot_slices"]), ("hot slices", slices)
    return st


# ------------------------------------------------------------------ planting
def whole_scalars(c):
    """scalars taken verbatim: the ends of the range and of the reduction, a carry through every window, NB and NB + 1 everywhere (over
    all windows: reduced mod r first; and over all but the top one: the digits as written)"""
    Wall, NB = windows(c), 1 << (c - 1)
    rep = lambda d: sum(d << (c * w) for w in range(Wall)) & ((1 << 256) - 1)
    low = lambda d: sum(d << (c * w) for w in range(Wall - 1))      # the same below r (the top window stays clear): no reduction first
    return [0, 1, R - 1, R, R + 1, (1 << 256) - 1, rep((1 << c) - 1), rep(NB), rep(NB + 1), low((1 << c) - 1), low(NB), low(NB + 1)]


def top_digit_max(c):
    """the largest digit the top window takes while the scalar stays below r whatever the lower windows hold"""
    return (R >> (c * (windows(c) - 1))) - 1


def plant(c, loads, rnd, filler=(), whole=(), n=None, shuffle=True):
    """Scalars (ints) for a load list [(window, digit, negative, count)]: `count` scalars whose digit at `window` is +-digit (negative:
    with the +1 in the next window that keeps the scalar positive), every window of `filler` that the load leaves alone holding a
    random positive digit; then the scalars of `whole` verbatim; then random scalars below 2^256 up to n pairs.  Every built scalar is
    checked against digits()."""
    Wall, NB = windows(c), 1 << (c - 1)
    out = []
    for w, d, neg, count in loads:
        assert 1 <= d <= NB and 0 <= w < Wall and (not neg or (w + 1 < Wall and d < NB)), (w, d, neg)
        for _ in range(count):
            vec = [0] * Wall
            vec[w] = -d if neg else d
            if neg:
                vec[w + 1] = 1
            for fw in filler:
                if fw != w and not (neg and fw == w + 1) and fw != w + 1:
                    vec[fw] = rnd.randrange(1, (min(NB, top_digit_max(c)) if fw == Wall - 1 else NB) + 1)
            s = sum(v << (c * k) if v >= 0 else -((-v) << (c * k)) for k, v in enumerate(vec))
            assert 0 <= s < R and digits(s, c, Wall) == vec, (w, d, neg)
            out.append(s)
    if shuffle:
        rnd.shuffle(out)
    out += list(whole)
    while n is not None and len(out) < n:
        out.append(rnd.randrange(1 << 256))
    assert n is None or len(out) == n, (len(out), n)
    return out


class Points:
    """k_i G for the pairs of every case, from the oracle: P_0 = k_0 G by its double-and-add, P_i = P_{i-1} + D by its addition
    (D = kd G), so k_i = k_0 + i kd mod r.  Made once per curve and grown on demand; never changed afterwards."""
    _sets = {}

    def __init__(self, orc, g):
        self.orc, self.g, self.sz = orc, g, 64 if g == 1 else 128
        self.gen = bytes.fromhex(load_golden("groups.json")["g%d" % g]["gen"])
        rnd = random.Random(4242 + g)
        self.k0, self.kd = rnd.randrange(1, R), rnd.randrange(1, R)
        self.d = orc.g_times_scalar(g, self.gen, le32(self.kd))
        self.cur = orc.g_times_scalar(g, self.gen, le32(self.k0))
        self.pts = bytearray()
        self.count = 0

    @classmethod
    def get(cls, orc, g):
        if g not in cls._sets:
            cls._sets[g] = cls(orc, g)
        return cls._sets[g]

    def k(self, i):
        return (self.k0 + i * self.kd) % R

    def first(self, n):
        while self.count < n:
            a = self.orc.g_affine(self.g, self.cur)
            assert not self.orc.g_is_zero(self.g, a)
            self.pts += a[:self.sz]
            self.cur = self.orc.g_add(self.g, self.cur, self.d)
            self.count += 1
        return bytes(self.pts[:n * self.sz])

    def expected(self, scalars, mask=None):
        """(sum s_i k_i mod r) G, affine, by the oracle's double-and-add"""
        e = sum(s * self.k(i) for i, s in enumerate(scalars) if mask is None or mask[i]) % R
        return self.orc.g_affine(self.g, self.orc.g_times_scalar(self.g, self.gen, le32(e)))


def oracle_sum(orc, g, scalars, pts):
    n = len(scalars)
    return orc.g_affine(g, orc.multiexp(g, "multiexp2" if g == 1 else "multiexp", b"".join(le32(s) for s in scalars), pts, n))


# ------------------------------------------------------------------ the catalogue
# A case: the switches it forces, its scalars, and `reaches`: the boundary it targets as a predicate on the MODEL's statistics
# (model_stats: no GPU, no emulator), asserted by assert_reaches before anything runs.
Case = namedtuple("Case", "name c flat lmax hot_min entry64 shard scalars mask reaches")


def _case(name, c, lmax, scalars, reaches, flat=False, hot_min=None, entry64=False, shard=(0, 1), mask=None):
    return Case(name, c, flat, lmax, hot_min, entry64, shard, scalars, mask, reaches)


def case_info(case):
    return plan_geometry(len(case.scalars), case.c, case.flat, case.shard, case.lmax, case.hot_min, case.entry64)


def assert_reaches(case):
    """the model-level self-check: the case reaches the boundary it names.  A failure fails the test; no case is dropped for it."""
    info = case_info(case)
    st = model_stats(case.scalars, info, case.mask)
    assert case.reaches(st, info), (case.name, "does not reach its boundary")
    return st


def has_loads(*lens):
    return lambda st, info: set(lens) <= set(st["loads"].values())


def has_nts(*nts):
    return lambda st, info: set(nts) <= set(st["nts"].values())


def load_rows(c, L, lens, window, first_digit=2, neg_every=3):
    """buckets of the given lengths at consecutive digits of one window, from first_digit on (length 0: the digit stays empty); every
    neg_every-th bucket holds negative digits where the window allows it.  Digit 1 is left to the +1 that follows a negative digit
    (flat plans: every window's digit 1 shares one bucket)."""
    Wall, NB = windows(c), 1 << (c - 1)
    rows = []
    for j, ln in enumerate(lens):
        d = first_digit + j
        neg = neg_every and j % neg_every == neg_every - 1 and window + 1 < Wall and d < NB
        if ln:
            rows.append((window, d, bool(neg), ln))
    return rows


def lengths_small(L):
    return [0, 1, 2, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1]


def planner_cases(c, flat=False, shard=(0, 1), entry64=False, full=True, seed=0):
    """The planner's boundaries at one geometry.  full: every row of the issue's list, in window 0 with the other windows empty, then in
    the top owned and a middle owned window with random filler in the rest (the L = 1000 rows of 18 002 pairs and the hot rows of up to
    14 334 without filler; the hot rows in the first and the middle window); else the reduced list (small lengths, WAVE_COMBINE_MIN,
    HOT_MIN forced to 8, the whole scalars) in window 0 and in the top owned window."""
    rnd = random.Random(1000 * c + seed)
    Wall, NB = windows(c), 1 << (c - 1)
    own = [w for w in range(Wall) if w >= shard[0] and (w - shard[0]) % shard[1] == 0]
    tmax = min(NB, top_digit_max(c))
    kw = dict(flat=flat, shard=shard, entry64=entry64)
    tag = "c=%d%s%s%s" % (c, " flat" if flat else "", " shard=%d/%d" % shard if shard != (0, 1) else "", " e64" if entry64 else "")
    cases = []
    # (flat plans: every window shares the one bucket set, so filler would add to the planted buckets and the top window has too few
    #  digits below r; their second place is a middle window with the rest empty -- what changes is the entry index, window n + i)
    places = [("first owned window, rest empty", own[0], ())]
    if flat:
        places += [("middle window, rest empty", own[len(own) // 2], ())]
    elif full:
        places += [("top owned window, filler", own[-1], range(Wall)), ("middle owned window, filler", own[len(own) // 2], range(Wall))]
    else:
        places += [("top owned window, filler", own[-1], range(Wall))]
    for where, w, filler in places:
        top = w == Wall - 1
        # in the top window only the digits 1 .. tmax exist: rows are cut to what fits (the first-window run holds every row)
        def fit(lens):
            return lens if not top else lens[:tmax - 1]
        L = 4
        nts_wave = [16, 17, 18, 64, 65]
        lens = fit(lengths_small(L) + [nt * L - 1 for nt in nts_wave])
        sc = plant(c, load_rows(c, L, lens, w), rnd, filler=filler)
        want_l = [x for x in lens if x]
        want_nt = [nt for nt in nts_wave if nt * L - 1 in lens]
        cases.append(_case("%s, L=4: lengths 0..2L+1 and nt 16/17/18/64/65, %s" % (tag, where), c, L, sc,
                           (lambda wl, wn: lambda st, info: has_loads(*wl)(st, info) and has_nts(*wn)(st, info))(want_l, want_nt), **kw))
        lens = fit([7 * L, 8 * L - 3, 9 * L, L + 1, 1])
        sc = plant(c, load_rows(c, L, lens, w, neg_every=2), rnd, filler=filler)
        cases.append(_case("%s, L=4 HOT_MIN=8: nt 7/8/9, %s" % (tag, where), c, L, sc, has_nts(*[-(-x // L) for x in lens]), hot_min=8, **kw))
        if not full:
            continue
        L = 1000
        rems = [1, 3, 4, 996, 997, 1000]
        lens = fit(rems + [2 * L + x for x in rems])
        sc = plant(c, load_rows(c, L, lens, w, neg_every=5), rnd)          # (18 002 pairs: the other windows stay empty)
        keys = {len_key(x, L) for x in rems}
        assert {1, 255} <= keys and len_key(996, L) == 254 and len_key(997, L) == 255 and len_key(3, L) == 1 and len_key(4, L) == 2
        cases.append(_case("%s, L=1000: remainders 1/3/4/996/997/1000 alone and behind two full tasks, %s" % (tag, where.replace(", filler", ", rest empty")), c, L, sc,
                           has_loads(*lens), **kw))
    # the hot rows: in the first owned window, then in a middle owned window, the other windows empty (about 4 100 pairs per bucket
    # of the HOT_MIN-unset row: no filler)
    for where, w in ([("first owned window", own[0]), ("middle owned window", own[len(own) // 2])] if full else []):
        L = 4
        sc = plant(c, load_rows(c, L, [1023 * L, 1024 * L - 1, 1025 * L - 2], w, neg_every=2), rnd)
        cases.append(_case("%s, L=4 HOT_MIN unset: nt 1023/1024/1025, %s" % (tag, where), c, L, sc, has_nts(1023, 1024, 1025), **kw))
        nts = [511, 512, 513, 1024, 1025]
        sc = plant(c, load_rows(c, L, [nt * L - (j % L) for j, nt in enumerate(nts)], w, neg_every=2), rnd)
        cases.append(_case("%s, L=4 HOT_MIN=2: slice edges nt 511/512/513/1024/1025, %s" % (tag, where), c, L, sc, has_nts(*nts), hot_min=2, **kw))
        nts = [513, 2, 1025, 600]
        sc = plant(c, load_rows(c, L, [nt * L - (j % L) for j, nt in enumerate(nts)], w, first_digit=3, neg_every=0), rnd)
        cases.append(_case("%s, L=4 HOT_MIN=2: four hot buckets nt 513/2/1025/600 (slices 2, 1, 3, 2), %s" % (tag, where), c, L, sc,
                           lambda st, info: sorted(st["nts"].values()) == [2, 513, 600, 1025] and
                           sum(-(-v // HOT_SLICE) for v in st["nts"].values()) == 8, hot_min=2, **kw))
    return cases


def bin_cases(c, flat=False, shard=(0, 1), entry64=False, seed=0):
    """the coarse bins and the per-bin counting sort: every bucket of a bin with one entry, one bin / one bucket holding everything, the
    two-round loop of presort_bins at 4 bthr - 1 / 4 bthr / 4 bthr + 1 entries, a partly filled last wavefront with all lanes on one
    key and with every lane on its own key"""
    rnd = random.Random(77 * c + seed)
    Wall, NB = windows(c), 1 << (c - 1)
    own = [w for w in range(Wall) if w >= shard[0] and (w - shard[0]) % shard[1] == 0]
    kw = dict(flat=flat, shard=shard, entry64=entry64)
    tag = "c=%d%s%s" % (c, " flat" if flat else "", " e64" if entry64 else "")
    L = 4
    geo = plan_geometry(1, c, flat, shard, L)
    lo, SUB, HB = geo["lo_bits"], 1 << geo["lo_bits"], NB >> geo["lo_bits"]
    w0, w1 = own[0], own[min(1, len(own) - 1)]
    hi = HB - 1                                            # the bin of the top bucket bits
    dig = lambda hi_, lo_: (hi_ << lo) + lo_ + 1
    cases = []
    # every bucket of one bin with exactly one entry (and nothing else in that bin)
    sc = plant(c, [(w0, dig(hi, t), False, 1) for t in range(SUB)], rnd)
    cases.append(_case("%s: every bucket of one bin holds one entry" % tag, c, L, sc,
                       lambda st, info: sum(1 for b, v in st["loads"].items() if v == 1) >= (1 << info["lo_bits"]) and max(st["bins"].values()) == 1 << info["lo_bits"], **kw))
    # one bin holds every entry, the low bits spread
    sc = plant(c, [(w0, dig(hi, rnd.randrange(SUB)), False, 1) for _ in range(1500)], rnd)
    cases.append(_case("%s: one bin holds every entry" % tag, c, L, sc, lambda st, info: len(st["bins"]) == 1 and len(st["loads"]) > 1, **kw))
    # one bucket holds every entry
    sc = plant(c, [(w0, dig(hi, SUB - 1), False, 1500)], rnd)
    cases.append(_case("%s: one bucket holds every entry" % tag, c, L, sc, lambda st, info: list(st["loads"].values()) == [1500], **kw))
    # 4 bthr - 1 / 4 bthr / 4 bthr + 1 entries in ONE bin that holds the whole plan (a case each): the loop of presort_bins takes one
    # round up to 4 bthr entries and two from there on.  bthr follows from the plan's size (msm_plan_finish), so the smallest bthr is
    # taken at which a plan of 4 bthr - 1 .. 4 bthr + 1 single-digit scalars gets that very bthr.
    bthr = next(t for t in range(64, 1025, 64) if all(plan_geometry(4 * t + dl, c, flat, shard, L)["bthr"] == t for dl in (-1, 0, 1)))
    for dl in (-1, 0, 1):
        sc = plant(c, [(w0, dig(hi, j % SUB), False, 1) for j in range(4 * bthr + dl)], rnd)
        cases.append(_case("%s: a bin of 4 bthr %+d entries (bthr = %d)" % (tag, dl, bthr), c, L, sc,
                           (lambda t, dl_: lambda st, info: info["bthr"] == t and list(st["bins"].values()) == [4 * t + dl_])(bthr, dl), **kw))
    # a bin whose last wavefront is partly filled: 64 + 37 entries, all on one key (one bin), every lane on its own key (another bin:
    # 101 distinct buckets), and a full wavefront's worth of one key followed by distinct keys
    assert SUB >= 101, "a bin has fewer than 101 buckets: the every-lane-its-own-key row does not fit"
    a, b_ = (w0, hi), (w1, 0) if w1 != w0 else (w0, 0)
    loads = [(a[0], dig(a[1], 5), False, 101)] + [(b_[0], dig(b_[1], t), False, 1) for t in range(101)]
    sc = plant(c, loads, rnd)
    cases.append(_case("%s: partly filled last wavefront, one key / every lane its own key" % tag, c, L, sc,
                       lambda st, info: sorted(st["bins"].values()) == [101, 101] and 101 in st["loads"].values() and
                       sum(1 for v in st["loads"].values() if v == 1) == 101, **kw))
    return cases


SIZES = [1, 63, 1023, 1024, 1025, 2048, 2049, 4097]


def size_cases(c, flat=False, shard=(0, 1), entry64=False, sizes=SIZES, seed=0):
    """n pairs of whole and random scalars (the digit scalars), the LAST pair with a negative digit in the first owned window: its entry
    has the largest index with the sign bit right above it (idx_bits at n = 2^k and 2^k + 1), in the last, partly filled tile"""
    rnd = random.Random(31 * c + seed)
    Wall, NB = windows(c), 1 << (c - 1)
    w0 = shard[0]
    cases = []
    for n in sizes:
        whole = whole_scalars(c)[:max(0, n - 1)]
        last = plant(c, [(w0, 2 if NB > 2 else 1, NB > 2, 1)], rnd)
        sc = plant(c, [], rnd, whole=whole, n=n - 1) + last
        k = max(1, (n * (Wall if flat else 1) - 1).bit_length())
        top_entry = ((w0 * n if flat else 0) + n - 1) | (1 << 31)
        cases.append(_case("c=%d%s%s%s: n=%d" % (c, " flat" if flat else "", " shard=%d/%d" % shard if shard != (0, 1) else "", " e64" if entry64 else "", n),
                           c, 4, sc, (lambda n_, k_, e_: lambda st, info: info["idx_bits"] == k_ and info["n"] == n_ and
                                      any(e_ in cn for cn in st["want"].values()))(n, k, top_entry),
                           flat=flat, shard=shard, entry64=entry64))
    return cases


def masked_scalars(c, seed=0):
    """the scalars of the masked cases: window 0 holds two hot buckets of 10 L entries (digits 2 and 3; HOT_MIN = 2, L = 4) and buckets of
    3 L + 1, L, 1 and 2 L + 1; then the whole scalars and 200 random ones"""
    rnd = random.Random(555 + c + seed)
    L = 4
    loads = load_rows(c, L, [10 * L, 10 * L, 3 * L + 1, L, 1, 2 * L + 1], 0, first_digit=2, neg_every=3)
    sc = plant(c, loads, rnd, whole=whole_scalars(c), shuffle=True)
    return plant(c, [], rnd, whole=sc, n=len(sc) + 200)


def planted_mask(sc, c, flat, phase, gone, shrunk, L=4):
    """mask[i] = 0 for every third pair (i % 3 == phase), for every pair that touches the bucket of digit `gone` and for all but L + 1
    of the pairs that touch the bucket of digit `shrunk` (window 0; flat plans: any window).  Returns (mask, pairs kept on `shrunk`)."""
    Wall = windows(c)
    touches = lambda s_, d: any(abs(x) == d for x in digits(s_, c, Wall)) if flat else abs(digits(s_, c, Wall)[0]) == d
    mask = bytearray(0 if i % 3 == phase else 1 for i in range(len(sc)))
    kept = 0
    for i, s_ in enumerate(sc):
        if touches(s_, gone):
            mask[i] = 0
        elif touches(s_, shrunk):
            mask[i] = 1 if kept < L + 1 else 0
            kept += mask[i]
    return bytes(mask), kept


def mask_reaches(sc, mask, kept, gone, shrunk, flat, L=4):
    """the boundary a planted mask targets, on the model: the bucket of `gone` was hot and is empty, the bucket of `shrunk` keeps
    exactly L + 1 pairs (per-window plans: L + 1 entries, two tasks; flat plans hold a pair's every window, so at least that) and is
    still hot, and at least a third of the pairs is gone"""
    def reaches(st, info):
        plain = model_stats(sc, info)
        bg, bs = gone - 1, shrunk - 1                         # window 0 (flat: the one bucket set)
        return plain["nts"][bg] >= 2 and bg not in st["loads"] and kept == L + 1 and st["loads"][bs] >= L + 1 and \
            (flat or st["loads"][bs] == L + 1) and plain["nts"][bs] > st["nts"][bs] >= 2 and sum(1 for m in mask if not m) >= len(sc) // 3
    return reaches


def masked_cases(c, flat=False, seed=0):
    """a plan's masked variant (msm_plan_variant: the per-bin sort in its masked form).  The mask removes every third pair, every pair
    of one hot bucket and all but L + 1 pairs of another (HOT_MIN = 2, L = 4)."""
    sc = masked_scalars(c, seed)
    mask, kept = planted_mask(sc, c, flat, 0, 2, 3)
    return [_case("c=%d%s: masked variant" % (c, " flat" if flat else ""), c, 4, sc, mask_reaches(sc, mask, kept, 2, 3, flat), flat=flat,
                  hot_min=2, mask=mask)]


def catalogue(c, flat=False, shard=(0, 1), entry64=False, full=True, sizes=SIZES, bins=True, masked=False):
    """the cases of one geometry: the planner's rows (full: every row; else the reduced list), the bins' rows, the digit scalars at
    the sizes, the masked variant"""
    cases = planner_cases(c, flat, shard, entry64, full)
    if bins:
        cases += bin_cases(c, flat, shard, entry64)
    cases += size_cases(c, flat, shard, entry64, sizes)
    if masked:
        cases += masked_cases(c, flat)
    return cases


# the geometries of the GPU file: (c, flat, entry64, shard, the whole catalogue or the reduced one)
GEOMETRIES = [(8, False, False, (0, 1), True), (16, False, False, (0, 1), True), (13, False, False, (0, 1), False), (15, False, False, (0, 1), False),
              (8, False, True, (0, 1), False), (13, False, True, (0, 1), False), (15, False, True, (0, 1), False), (16, False, True, (0, 1), False),
              (16, False, False, (1, 3), False), (16, False, False, (2, 3), False), (13, False, False, (1, 3), False), (13, False, False, (2, 3), False),
              (9, True, False, (0, 1), True), (12, True, False, (0, 1), False)]


def geometry_parts(k):
    """a geometry's cases in parts of a few seconds each: the planner's rows place by place (three cases each), the hot rows window by
    window, then the bins, the sizes and the masked variant"""
    c, flat, entry64, shard, full = GEOMETRIES[k]
    places = (2 if flat else 3) if full else 1
    return ["place %d" % p for p in range(places)] + (["hot rows 0", "hot rows 1"] if full else []) + ["bins and sizes"]


def geometry_cases(k, part):
    c, flat, entry64, shard, full = GEOMETRIES[k]
    if part == "bins and sizes":
        cases = bin_cases(c, flat, shard, entry64) + size_cases(c, flat, shard, entry64)
        return cases + (masked_cases(c, flat) if shard == (0, 1) and not entry64 else [])
    cases = planner_cases(c, flat, shard, entry64, full)
    if not full:
        return cases
    places = 2 if flat else 3
    assert len(cases) == 3 * places + 6
    at = 3 * places + 3 * int(part[-1]) if part.startswith("hot rows") else 3 * int(part[-1])
    return cases[at:at + 3]


# ------------------------------------------------------------------ running a case
def apply_switches(bn, tune, case):
    tune(bn.lib, "TABLE_C" if case.flat else "MSM_C", case.c)
    tune(bn.lib, "MSM_LMAX", case.lmax)
    if case.hot_min:
        tune(bn.lib, "MSM_HOT_MIN", case.hot_min)
    if case.entry64:
        tune(bn.lib, "MSM_ENTRY64", 1)


def run_plan(bn, tune, case):
    """the model-level self-check, then the plan of the case's scalars through the hook against the model"""
    st = assert_reaches(case)
    apply_switches(bn, tune, case)
    raw = b"".join(le32(s) for s in case.scalars)
    want = case_info(case)
    entries = len(case.scalars) * want["W"]                  # one entry per pair and owned window at most; a task per entry and bucket
    dump = bn.msm_plan(raw, table_c=case.c if case.flat else 0, shard=case.shard, mask=case.mask,
                       capacity=(want["nbuckets"], entries, entries + want["nbuckets"]))
    got = {k: dump["info"][k] for k in want}
    assert got == want, ("info words", case.name, got, want)
    check_plan(dump, case.scalars, case.mask, st)
    return dump


def run_sum(bn, orc, tune, case, g):
    """the case's sum over the oracle's points k_i G against the closed form (and the oracle's multiexp up to 20 000 pairs): bit for bit.
    Per-window plans through g1_multiexp / g2_multiexp (with the case's shard), flat plans through resident points.  (Masked cases
    have no sum of their own here: only the prover builds a variant -- planted_key_proof.)"""
    assert case.mask is None
    apply_switches(bn, tune, case)
    P = Points.get(orc, g)
    n = len(case.scalars)
    pts = P.first(n)
    raw = b"".join(le32(s) for s in case.scalars)
    if case.flat:
        h = bn.load_points(g, pts)
        try:
            assert h.table["c"] == case.c
            got = h.multiexp(raw)
        finally:
            h.free()
        want_scalars = case.scalars
    else:
        msm = bn.g1_multiexp if g == 1 else bn.g2_multiexp
        got = msm(raw, pts, shard=case.shard if case.shard != (0, 1) else None)
        # a shard's partial sum: the owned windows' digits at their weights
        info = case_info(case)
        want_scalars = case.scalars
        if case.shard != (0, 1):
            own = owned(info)
            part = lambda ds: sum((abs(ds[w]) << (case.c * w)) * (1 if ds[w] >= 0 else -1) for w in own) % R
            want_scalars = [part(digits(s_, case.c, info["Wall"])) for s_ in case.scalars]
    assert got == P.expected(want_scalars), ("sum against the closed form", case.name, g)
    if n <= 20000 and case.shard == (0, 1):
        assert got == oracle_sum(orc, g, case.scalars, pts), ("sum against the oracle's multiexp", case.name, g)


def planted_key_proof(bn, orc, tune, mode):
    """The masked variants' SUMS: a proof on a small key whose pointsA are at infinity where mask A is 0 and whose pointsB1 / pointsB2
    are at infinity where mask B is 0, on a witness that carries the planted scalars of the masked cases; PROVE_SPARSE = 2 makes the
    prover run the A sum and the B1 / B2 sums on the plan's variants (msm_plan_variant), MSM_LMAX = 4 and MSM_HOT_MIN = 2 make digits 2
    and 3 of window 0 hot buckets.  Mask A empties the bucket of digit 2 and leaves L + 1 pairs of digit 3's; mask B the other way
    round; the C sum runs on the plain plan, where both are whole -- so the G1 sets that share one msm_accumulate / msm_combine_all
    launch (blockIdx.y) each bring hot buckets of their own, different from set to set.  mode "plain": per-window plans of c = 8 on the
    key's plain sections; "table": flat plans of c = 9 on the fixed-base tables.  The key is a pseudo key (every point k G for seeded
    k, by the oracle's double-and-add): a proof is a pure function of (witness, key, r, s), and the oracle's prover is the reference."""
    import struct
    from wasmsnark_amd import synth
    import tail_patterns as tp
    flat, c = (True, 9) if mode == "table" else (False, 8)
    sc = [v % R for v in masked_scalars(c)]
    nv = len(sc)
    maskA, keptA = planted_mask(sc, c, flat, 0, 2, 3)
    maskB, keptB = planted_mask(sc, c, flat, 1, 3, 2)
    info = plan_geometry(nv, c, flat, (0, 1), 4, 2)
    for mask, kept, gone, shrunk in ((maskA, keptA, 2, 3), (maskB, keptB, 3, 2)):
        st = model_stats(sc, info, mask)
        assert mask_reaches(sc, mask, kept, gone, shrunk, flat)(st, info), ("the planted mask does not reach its boundary", mode, gone)
        assert sum(1 for v in st["nts"].values() if v >= 2) >= 2, "a variant without two hot buckets"
    assert sum(1 for v in model_stats(sc, info)["nts"].values() if v >= 2) >= 3
    key = bytearray(synth.pseudo_key(nv, 2, 512, 77, lambda g, scalars: tp.oracle_mul_base(orc, g, scalars)))
    pA, pB1, pB2 = struct.unpack("<10I", key[:40])[5:8]
    for i in range(nv):                                       # (pseudo_key's own infinity points stay: x == 0 whatever y is)
        if not maskA[i]:
            key[pA + 64 * i:pA + 64 * i + 32] = bytes(32)
        if not maskB[i]:
            key[pB1 + 64 * i:pB1 + 64 * i + 32] = bytes(32)
            key[pB2 + 128 * i:pB2 + 128 * i + 64] = bytes(64)
    key, wit = bytes(key), b"".join(le32(v) for v in sc)
    tune(bn.lib, "KEY_TABLE", 1 if flat else 0)
    tune(bn.lib, "TABLE_C" if flat else "MSM_C", c)
    tune(bn.lib, "MSM_LMAX", 4)
    tune(bn.lib, "MSM_HOT_MIN", 2)
    tune(bn.lib, "PROVE_SPARSE", 2)
    k = bn.load_key(key)
    try:
        assert (k.table["rows_w"] > 1) == flat and (not flat or k.table["c_w"] == c)
        for r, s_ in ((bytes(32), bytes(32)), (bytes(range(1, 33)), bytes(range(101, 133)))):
            bn.lib.c.wsnark_timing_enable(1)
            bn.lib.c.wsnark_timing_reset()
            try:
                got = bn.groth16GenProof(wit, k, r=r, s=s_)
                sorts = bn.lib.timing_report().get("msm_presort_bins", (0, 0))[1]
            finally:
                bn.lib.c.wsnark_timing_reset()
                bn.lib.c.wsnark_timing_enable(0)
            assert sorts >= 4, ("the per-bin sort ran %d times: the witness plan, its two variants and the H plan make four" % sorts)
            assert got == orc.groth16_prove(wit, key, r, s_, workers=8), (mode, "proof against the oracle's prover")
    finally:
        k.free()


def check_hook_capacities(bn):
    """the hook writes nothing past a capacity: an array that is too small fails the call with WSNARK_ERR_SIZE and stays untouched; a
    plan of no pair, and a shard that owns no window, return all-zero info words"""
    import ctypes as C
    sc = b"".join(le32(v) for v in range(1, 41))
    info = (C.c_uint32 * 24)()
    fn = bn.lib.c.wsnark_selftest_msm_plan
    assert fn(sc, 40, 0, 0, 1, None, info, None, None, 0, None, 0, None, 0, None, 0, None, 0) == 0
    w = dict(zip(bn.MSM_PLAN_INFO, info[:]))
    assert w["n"] == 40 and w["nvals"] >= 40 and w["tasks"] >= 1
    guard = (C.c_uint32 * 8)(*([0xDEADBEEF] * 8))
    assert fn(sc, 40, 0, 0, 1, None, info, None, None, 0, guard, w["nvals"] - 1, None, 0, None, 0, None, 0) == 1       # WSNARK_ERR_SIZE
    assert fn(sc, 40, 0, 0, 1, None, info, None, None, 0, None, 0, guard, w["tasks"] - 1, None, 0, None, 0) == 1
    assert fn(sc, 40, 0, 0, 1, None, info, guard, guard, w["nbuckets"] - 1, None, 0, None, 0, None, 0, None, 0) == 1
    assert list(guard) == [0xDEADBEEF] * 8
    assert fn(sc, 40, 0, 1, 0, None, info, None, None, 0, None, 0, None, 0, None, 0, None, 0) == 4                     # WSNARK_ERR_ARG
    assert fn(None, 0, 0, 0, 1, None, info, None, None, 0, None, 0, None, 0, None, 0, None, 0) == 0 and not any(info)
    assert fn(sc, 40, 0, 300, 301, None, info, None, None, 0, None, 0, None, 0, None, 0, None, 0) == 0 and not any(info)
    d = bn.msm_plan(sc)                                      # the binding's two calls: sizes, then arrays
    assert d["info"]["n"] == 40 and len(d["vals"]) == d["info"]["nvals"] == w["nvals"] and len(d["tasks"]) == w["tasks"]
