"""Cases for the staged grouping kernels (msm.hip: presort_scatter_once<uint32_t, true>, presort_bins<uint32_t, true>; the switch
WSNARK_PRESORT_STAGE), on top of tests/grouping_patterns.py: its model, its planting and its comparison are used unchanged.  Shared by
tests/test_emul_grouping_staged.py (CPU emulator) and tests/test_gpu_grouping_staged.py (-m gpu).

The staged scatter sorts the T = 1024 scalars' entries of a workgroup by bin in an LDS stage of 16 rows x 1024 entries and writes the
stage out position by position; the staged per-bin sort keeps a bin of at most CAP = 4096 entries in LDS (PRESORT_BINS_CAP) and leaves
a larger one to the two loops over global memory.  What can go wrong there and nowhere else: a run as long as the stage, runs of
length one, a partly filled tile, a bin that only the last live lane reaches, bins just below, at and above CAP, entries dropped by a
variant's mask inside the staged path.

Geometries: flat plans of TABLE_C = 16 (16 rows, 256 bins of 7 low bits) and TABLE_C = 20 (13 rows; 2048 bins of 8 low bits, and with
the test-only switch MSM_LO_BITS = 7 the 4096 bins of 7 low bits that a 2^20 key's plans have), and the per-window plan of c = 16
(16 x 128 bins)."""
import random
from collections import Counter

import grouping_patterns as gp

T = 1024          # scalars per workgroup of presort_scatter_once
CAP = 4096        # msm.hip: PRESORT_BINS_CAP
SWITCHES = ("MSM_C", "TABLE_C", "MSM_LMAX", "MSM_HOT_MIN", "MSM_ENTRY64", "MSM_LO_BITS", "PRESORT_STAGE")
TILE_SIZES = [1, 63, T - 1, T, T + 1, 2 * T + 1]

# (name, c, flat, MSM_LO_BITS or None)
FLAT16, FLAT20, FLAT20_LO7, WIN16 = ("flat c=16", 16, True, None), ("flat c=20", 20, True, None), ("flat c=20 lo=7", 20, True, 7), ("c=16", 16, False, None)
GEOS = [FLAT16, FLAT20, FLAT20_LO7, WIN16]


def geometry(case, lo_bits=None):
    """the info words of a case's plan: gp.plan_geometry, and under MSM_LO_BITS the same derivation from that many low bits (msm_plan_begin)"""
    info = gp.case_info(case)
    if lo_bits is None:
        return info
    NB, Wb, lo = info["NB"], (1 if case.flat else info["W"]), min(lo_bits, case.c - 1)
    while Wb * (NB >> lo) > gp.PRESORT_MAX_BINS and lo < case.c - 1 and lo < gp.PRESORT_MAX_LO:
        lo += 1
    while case.flat and (NB >> lo) < 2048 and lo > 7:
        lo -= 1
    assert info["idx_bits"] + 1 + lo <= 32
    nbins = Wb * (NB >> lo)
    bthr = min(1024, max(64, (info["n"] * info["W"] // nbins // 8 + 63) // 64 * 64))
    return dict(info, lo_bits=lo, nbins=nbins, bthr=bthr)


def from_digits(c, vec):
    """the scalar with the given (positive) digits, checked against the model's recoding"""
    s = sum(d << (c * w) for w, d in enumerate(vec))
    assert 0 <= s < gp.R and gp.digits(s, c, gp.windows(c)) == list(vec)
    return s


def case(name, geo, scalars, reaches, lmax=4, mask=None, entry64=False):
    _, c, flat, _ = geo
    return gp.Case("%s: %s" % (geo[0], name), c, flat, lmax, None, entry64, (0, 1), scalars, mask, reaches)


def tile_edge_cases(geo, sizes=TILE_SIZES):
    """n = 1, 63, T - 1, T, T + 1, 2 T + 1 pairs of gp's digit scalars (NB, NB + 1, carries through every window, values >= r) and random ones"""
    _, c, flat, _ = geo
    return [cs._replace(name="%s: %s" % (geo[0], cs.name)) for cs in gp.size_cases(c, flat=flat, sizes=sizes)]


def one_bin_cases(geo):
    """every scalar of a full tile (and of a full tile and one more) has the same digit in every row: on a flat plan ONE bin and one
    bucket take every entry, a run as long as the stage (16 x 1024 entries at 16 rows); on the per-window plan one run of 1024 per row"""
    _, c, flat, _ = geo
    Wall = gp.windows(c)
    s = from_digits(c, [5] * Wall)
    want = 1 if flat else Wall
    return [case("one digit in every row, n = %d" % n, geo, [s] * n,
                 (lambda n_: lambda st, info: len(st["bins"]) == want and set(st["bins"].values()) == {n_ * Wall // want})(n)) for n in (T, T + 1)]


def own_bin_cases(geo, lo_bits):
    """the opposite: every entry of the (partly filled) tile in a bin of its own, runs of length one.  The top row stays empty (its
    digits end below r's top bits, too few bins)."""
    _, c, flat, _ = geo
    Wall = gp.windows(c)
    lo = geometry(case("", geo, [1], None), lo_bits)["lo_bits"]
    HB = (1 << (c - 1)) >> lo
    rows = Wall - 1
    n = HB // rows if flat else HB
    rnd = random.Random(c)
    sc = []
    for i in range(n):
        # flat: one bucket set, bin = digit's high bits, so pair i takes the bins i rows .. i rows + rows - 1; per window: row k has bins of its own
        vec = [(((i * rows + w) if flat else i) << lo) + rnd.randrange(1 << lo) + 1 for w in range(rows)] + [0]
        sc.append(from_digits(c, vec))
    return [case("every entry in a bin of its own, n = %d" % n, geo, sc, lambda st, info: set(st["bins"].values()) == {1} and len(st["bins"]) == n * rows)]


def last_lane_cases(geo, lo_bits):
    """a full tile and a partly filled one of 64 + 63 scalars, every scalar with digit 3 in the first row alone -- but the last pair, the
    last live lane of the last wavefront: its digit lies in the top bin, which nothing else reaches.  And the same in a single partly
    filled tile."""
    _, c, flat, _ = geo
    Wall = gp.windows(c)
    top = 1 << (c - 1)                                   # digit NB: the top bin's last bucket
    out = []
    for n in (T + 127, 127):
        sc = [from_digits(c, [3] + [0] * (Wall - 1))] * (n - 1) + [from_digits(c, [top] + [0] * (Wall - 1))]
        out.append(case("a bin reached by the last live lane alone, n = %d" % n, geo, sc,
                        (lambda n_: lambda st, info: sorted(st["bins"].items()) == [(0, n_ - 1), ((info["NB"] >> info["lo_bits"]) - 1, 1)])(n)))
    return out


def cap_scalars(geo, lo_bits, seed=0):
    """one digit per scalar, all in the first row: bins of CAP - 1, CAP and CAP + 1 entries with the low bits spread, a bin of 500 entries
    in one bucket, the bins between and behind them empty"""
    _, c, flat, _ = geo
    rnd = random.Random(900 + c + seed)
    lo = geometry(case("", geo, [1], None), lo_bits)["lo_bits"]
    dig = lambda hi, lo_: (hi << lo) + lo_ + 1
    loads = [(0, dig(hi, rnd.randrange(1 << lo)), False, 1) for hi, cnt in ((1, CAP - 1), (2, CAP), (4, CAP + 1)) for _ in range(cnt)]
    loads += [(0, dig(6, 9), False, 500)]
    return gp.plant(c, loads, rnd)


def cap_cases(geo, lo_bits):
    """presort_bins around CAP, plain and as a masked variant: the mask drops every third pair and every pair of bucket (2, 0 .. 3), so
    entries are dropped inside the staged path (the bins of CAP - 1 and CAP entries) and inside the loops (the bin of CAP + 1)"""
    _, c, flat, _ = geo
    sc = cap_scalars(geo, lo_bits)
    lo = geometry(case("", geo, [1], None), lo_bits)["lo_bits"]
    want = {1: CAP - 1, 2: CAP, 4: CAP + 1, 6: 500}
    plain = case("bins of CAP - 1, CAP, CAP + 1 entries, one bucket of 500, empty bins", geo, sc,
                 lambda st, info: dict(st["bins"]) == want and st["loads"][(6 << info["lo_bits"]) + 9] == 500)
    gone = {(2 << lo) + t + 1 for t in range(4)}
    mask = bytes(0 if i % 3 == 0 or gp.digits(s, c, gp.windows(c))[0] in gone else 1 for i, s in enumerate(sc))
    masked = case("the same under a mask", geo, sc,
                  lambda st, info: all(0 < st["bins"][b] < want[b] for b in want) and not any((2 << info["lo_bits"]) + t in st["loads"] for t in range(4)),
                  mask=mask)
    return [plain, masked]


def run_plan(bn, tune, cs, lo_bits=None, stage=1):
    """gp.run_plan with the two switches of this file: the model-level self-check, the plan through the hook, the info words, check_plan"""
    want = geometry(cs, lo_bits)
    st = gp.model_stats(cs.scalars, want, cs.mask)
    assert cs.reaches(st, want), (cs.name, "does not reach its boundary")
    gp.apply_switches(bn, tune, cs)
    tune(bn.lib, "PRESORT_STAGE", stage)
    if lo_bits is not None:
        tune(bn.lib, "MSM_LO_BITS", lo_bits)
    entries = len(cs.scalars) * want["W"]
    dump = bn.msm_plan(b"".join(gp.le32(s) for s in cs.scalars), table_c=cs.c if cs.flat else 0, shard=cs.shard, mask=cs.mask,
                       capacity=(want["nbuckets"], entries, entries + want["nbuckets"]))
    got = {k: dump["info"][k] for k in want}
    assert got == want, ("info words", cs.name, got, want)
    gp.check_plan(dump, cs.scalars, cs.mask, st)
    return dump


def run_sum(bn, orc, tune, cs, lo_bits=None, stage=1, g=1):
    """gp.run_sum under the two switches: the sum against the closed form and the oracle"""
    tune(bn.lib, "PRESORT_STAGE", stage)
    if lo_bits is not None:
        tune(bn.lib, "MSM_LO_BITS", lo_bits)
    gp.run_sum(bn, orc, tune, cs, g)


def raw_sum(bn, orc, tune, cs, lo_bits, stage, g=1):
    """the sum's bytes, as gp.run_sum obtains them"""
    gp.apply_switches(bn, tune, cs)
    tune(bn.lib, "PRESORT_STAGE", stage)
    if lo_bits is not None:
        tune(bn.lib, "MSM_LO_BITS", lo_bits)
    n = len(cs.scalars)
    pts = gp.Points.get(orc, g).first(n)
    raw = b"".join(gp.le32(s) for s in cs.scalars)
    if not cs.flat:
        return (bn.g1_multiexp if g == 1 else bn.g2_multiexp)(raw, pts)
    h = bn.load_points(g, pts)
    try:
        assert h.table["c"] == cs.c
        return h.multiexp(raw)
    finally:
        h.free()


def assert_same_plans(off, on, lmax):
    """switch off against switch on: equal bucket bounds, equal tasks as sets per length key (a split bucket's tasks without their
    slot numbers: the planner hands those out with atomics in either setting), equal buckets as multisets"""
    assert off["info"] == on["info"]
    assert off["bstart"] == on["bstart"] and off["bend"] == on["bend"]
    by_key = lambda d: {k: sorted((dst if not dst & gp.PARTIAL_FLAG else gp.PARTIAL_FLAG, s, ln) for dst, s, ln in d["tasks"] if gp.len_key(ln, lmax) == k)
                        for k in {gp.len_key(t[2], lmax) for t in d["tasks"]}}
    assert by_key(off) == by_key(on)
    for b, (s, e) in enumerate(zip(off["bstart"], off["bend"])):
        if s != e:
            assert Counter(off["vals"][s:e]) == Counter(on["vals"][s:e]), ("bucket", b)


def reset(bn):
    for name in SWITCHES:
        bn.lib.tune(name, None)
