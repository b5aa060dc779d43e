"""The fused task planner and the plans' alternating counter blocks (msm.hip: msm_plan_fused, plan_counters_begin / _done, the bin words
presort_bins clears; WSNARK_PLAN_FUSED, WSNARK_PLAN_SPAN).  Shared by tests/test_emul_plan_fused.py (CPU: the sources under the thread
emulator) and tests/test_gpu_plan_fused.py (-m gpu: the device).

Every plan comes back through bn.msm_plan and is compared exactly with the model of tests/grouping_patterns.py (check_plan), with the
switch on and off.  After every build the hook's word 23 must be zero: it counts the words a build has to leave at zero and did not --
the planner's arrival counter, the slot's other header block, and (fused builds) the bin counts and cursors.  It is read by a second,
sizes-only call of the hook with the same inputs, which is one more rebuild of the slot; its other 23 words must repeat the first call's.

What the issue's list cannot mean literally, and what stands here instead:
  * bucket counts of span - 1, span + 1 and 2 span + 1 do not exist: a plan has W 2^(c-1) buckets (flat: 2^(c-1)), a multiple of
    NB = 2^(c-1) >= 8.  span_edges() finds the smallest c at which window shards give span - NB, span, span + NB and 2 span + NB buckets,
    and every such plan carries planted loads in the buckets on both sides of every span boundary, in bucket 0 and in the last bucket
    the recoding can reach.  Flat plans reach span and 2 span only.
  * MSM_HOT_MIN = 2 leaves no multi bucket (a bucket cut into two tasks is hot already).  The three-kinds case runs at HOT_MIN = 2 as
    asked (plain and hot) and at HOT_MIN = 4 (plain, multi and hot in one plan).
  * no call of the C ABI leaves a build between msm_plan_begin and msm_plan_finish unless the device fails; the hook does it on request
    (PLAN_HOOK_ABANDON: begin and the histogram, then an error return).
  * a closed form exists for the satisfying witness only.  The boolean-heavy witness of the proofs is compared with the oracle's prover
    and with the switch-off proof, the uniform one with the closed form and the switch-off proof."""
import ctypes as C
import random

import grouping_patterns as gp

SPANS = (1024, 2048, 4096)          # the instantiations msm_plan_fused is launched at (PLAN_SPAN; any other value: the default)
SPAN_DEFAULT = 1024
L = 4                                # MSM_LMAX of every case
SWITCHES = ("MSM_C", "TABLE_C", "MSM_LMAX", "MSM_HOT_MIN", "MSM_ENTRY64", "PLAN_FUSED", "PLAN_SPAN", "PLAN_HOOK_ABANDON")


def reset(bn):
    for name in SWITCHES:
        bn.lib.tune(name, None)


def shards_by_buckets(c):
    """{bucket count: (rank, world)} of the per-window plans of width c: the first shard that owns W windows, W 2^(c-1) buckets"""
    Wall, NB, out = gp.windows(c), 1 << (c - 1), {}
    for world in range(1, Wall + 1):
        for rank in range(world):
            W = (Wall - rank + world - 1) // world
            out.setdefault(W * NB, (rank, world))
    return out


def span_edges(span):
    """(c, [(buckets, shard)]) at the smallest window width that reaches span - NB, span, span + NB and 2 span + NB buckets"""
    for c in range(4, 17):
        NB, by = 1 << (c - 1), shards_by_buckets(c)
        want = [span - NB, span, span + NB, 2 * span + NB]
        if all(w in by for w in want):
            return c, [(w, by[w]) for w in want]
    raise AssertionError("no window width reaches the four bucket counts around span %d" % span)


def bucket_row(c, flat, shard, b, count):
    """the load row that puts `count` entries into bucket b; None where the recoding cannot (a digit the top window does not take)"""
    NB, Wall = 1 << (c - 1), gp.windows(c)
    k, d = (0, b + 1) if flat else (b // NB, b % NB + 1)
    w = shard[0] + k * shard[1]
    if w == Wall - 1 and d > gp.top_digit_max(c):
        return None
    return (w, d, False, count)


def edge_case(name, c, nbuckets, span, flat=False, shard=(0, 1), entry64=False, hot_min=4, seed=0, fill=200):
    """planted loads of every kind (1, L: plain; L + 1, 3 L: multi at HOT_MIN = 4; 4 L + 1, 9 L: hot) in the buckets on both sides of
    every span boundary, in bucket 0 and in the last reachable bucket (hot), then `fill` random scalars"""
    rnd = random.Random(span * 31 + c + seed)
    edges = sorted({b for m in range(span, nbuckets + 1, span) for b in (m - 2, m - 1, m, m + 1) if 0 <= b < nbuckets} | {0, 1, nbuckets - 2})
    counts = [1, L + 1, 4 * L + 1, L, 3 * L, 9 * L]
    rows, planted = [], {}
    for j, b in enumerate(edges):
        row = bucket_row(c, flat, shard, b, counts[j % len(counts)])
        if row:
            rows.append(row)
            planted[b] = counts[j % len(counts)]
    last = next(b for b in range(nbuckets - 1, -1, -1) if bucket_row(c, flat, shard, b, 1))
    rows.append(bucket_row(c, flat, shard, last, 5 * L + 2))
    planted[last] = 5 * L + 2
    sc = gp.plant(c, rows, rnd, n=sum(r[3] for r in rows) + fill)

    def reaches(st, info):
        return info["nbuckets"] == nbuckets and all(st["loads"].get(b, 0) >= v for b, v in planted.items()) and \
            st["nts"][last] >= hot_min and {1} <= set(st["nts"].values()) and \
            (hot_min == 2 or any(1 < v < hot_min for v in st["nts"].values())) and \
            len({b // span for b, v in st["nts"].items() if v >= hot_min}) == -(-nbuckets // span)      # a hot bucket in every workgroup
    return gp._case(name, c, L, sc, reaches, flat=flat, hot_min=hot_min, entry64=entry64, shard=shard)


def span_edge_cases(span):
    """the four per-window bucket counts around `span` (the third with 8-byte entries), and flat plans of span and 2 span buckets (the
    second with 8-byte entries)"""
    c, counts = span_edges(span)
    cases = [edge_case("span %d: c=%d shard=%d/%d, %d buckets%s" % (span, c, sh[0], sh[1], nb, " e64" if j == 2 else ""), c, nb, span,
                       shard=sh, entry64=j == 2) for j, (nb, sh) in enumerate(counts)]
    for j, mult in enumerate((1, 2)):
        cf = (mult * span).bit_length()                      # NB = 2^(cf - 1) = mult * span
        cases.append(edge_case("span %d: flat c=%d, %d buckets%s" % (span, cf, mult * span, " e64" if j else ""), cf, mult * span, span,
                               flat=True, entry64=bool(j), fill=60))
    return cases


def kinds_cases():
    """plain, multi and hot buckets in one plan of three workgroups at PLAN_SPAN = 1024 (2 304 buckets), a hot bucket in each and one as
    the last bucket: at MSM_HOT_MIN = 2 (as the issue words it: plain and hot) and at 4 (all three kinds)"""
    c, counts = span_edges(1024)
    nb, sh = counts[3]
    return [edge_case("kinds: c=%d, %d buckets, HOT_MIN=%d" % (c, nb, hm), c, nb, 1024, shard=sh, hot_min=hm, seed=hm) for hm in (2, 4)]


def plain_case(c, n, seed, shard=(0, 1), flat=False, entry64=False, name=None):
    """n random scalars, HOT_MIN unset: no hot bucket"""
    rnd = random.Random(seed)
    sc = gp.plant(c, [], rnd, n=n)
    return gp._case(name or "random: c=%d n=%d" % (c, n), c, L, sc, lambda st, info: max(st["nts"].values()) < gp.HOT_MIN,
                    flat=flat, shard=shard, entry64=entry64)


def masked_case(c, seed=0):
    return gp.masked_cases(c, seed=seed)[0]


# ------------------------------------------------------------------ running
def left_words(bn, case, dump):
    """the hook's word 23 after one more build with the same inputs (sizes only); its other words repeat the first call's"""
    raw = b"".join(gp.le32(s) for s in case.scalars)
    info = (C.c_uint32 * 24)()
    rc = bn.lib.c.wsnark_selftest_msm_plan(raw, len(case.scalars), case.c if case.flat else 0, case.shard[0], case.shard[1], case.mask, info,
                                           None, None, 0, None, 0, None, 0, None, 0, None, 0)
    assert rc == 0, (case.name, rc)
    assert dict(zip(bn.MSM_PLAN_INFO, info[:])) == dump["info"], ("the rebuild's info words", case.name)
    return info[23]


def run(bn, tune, case, fused, span=None):
    """one build of the case against the model, then one more for the words a build leaves at zero"""
    bn.lib.tune("PLAN_FUSED", fused)
    bn.lib.tune("PLAN_SPAN", span)
    try:
        dump = gp.run_plan(bn, tune, case)
        assert left_words(bn, case, dump) == 0, ("words not left at zero", case.name, fused, span)
    finally:
        reset(bn)
    return dump


def abandon(bn, tune, case, fused):
    """begin and the histogram of the case's plan, then an error return (PLAN_HOOK_ABANDON)"""
    from wasmsnark_amd._lib import WsnarkError
    bn.lib.tune("PLAN_FUSED", fused)
    bn.lib.tune("PLAN_HOOK_ABANDON", 1)
    try:
        gp.apply_switches(bn, tune, case)
        try:
            bn.msm_plan(b"".join(gp.le32(s) for s in case.scalars), table_c=case.c if case.flat else 0, shard=case.shard)
        except WsnarkError:
            pass
        else:
            raise AssertionError("the abandoned build returned a plan")
    finally:
        reset(bn)


def check_rebuilds(bn, tune, fused, big_c=11):
    """rebuilds of ONE plan slot (the hook builds on the lane's slot 0, its variant on slot 2), each checked against the model and for
    the words it leaves at zero: hot / none / hot; many bins / few / many; 8-byte entries / 4-byte; a plan, its masked variant, the
    plan again with other scalars; an abandoned build, then a good one; a call that fails before anything is queued, then a good one;
    the switch flipped between builds"""
    hot = kinds_cases()[1]
    steps = [hot, plain_case(hot.c, 300, 1, shard=hot.shard), hot,
             plain_case(big_c, 300, 2), plain_case(7, 300, 3), plain_case(big_c, 300, 4),
             plain_case(8, 200, 5, entry64=True), plain_case(8, 200, 6),
             plain_case(8, len(masked_case(8).scalars), 7), masked_case(8), plain_case(8, 250, 8)]
    for cs in steps:
        run(bn, tune, cs, fused, 1024)
    abandon(bn, tune, plain_case(8, 200, 9), fused)
    run(bn, tune, plain_case(8, 200, 10), fused)
    abandon(bn, tune, hot, fused)
    run(bn, tune, hot, fused, 1024)
    info = (C.c_uint32 * 24)()
    assert bn.lib.c.wsnark_selftest_msm_plan(b"\1" * 32, 1, 0, 1, 0, None, info, None, None, 0, None, 0, None, 0, None, 0, None, 0) == 4      # WSNARK_ERR_ARG
    run(bn, tune, hot, fused, 1024)
    for f in (1 - fused, fused, 1 - fused, fused):
        run(bn, tune, hot if f == fused else plain_case(8, 200, 11), f, 1024)


def same_counts(a, b):
    """two dumps of one case agree in everything the model fixes beyond check_plan: the info words and the bucket bounds"""
    assert a["info"] == b["info"] and a["bstart"] == b["bstart"] and a["bend"] == b["bend"]


# ------------------------------------------------------------------ proofs
R32, S32 = bytes(range(5, 37)), bytes(range(70, 102))


def check_proofs(bn, orc, tune, logd):
    """three proofs back to back on one key at the full-size arrangement (PROVE_FULL_SIZE = 1): uniform, boolean-heavy, uniform.  Each
    is its switch-off proof; the uniform one is the closed form, the boolean-heavy one the oracle's prover's."""
    from wasmsnark_amd import synth
    circ = synth.NativeCircuit(bn.lib, logd, n_public=3, seed=33, style="rows")
    pkey, _ = circ.build_key()
    uniform = circ.witness_bin()
    rnd = random.Random(logd)
    heavy = bytearray(uniform)
    for i in range(1, circ.n_vars):
        if i % 8:                                             # 87.5 % of the signals 0 / 1
            heavy[32 * i:32 * i + 32] = gp.le32(rnd.randrange(2))
    heavy = bytes(heavy)
    tune(bn.lib, "PROVE_FULL_SIZE", 1)
    key = bn.load_key(pkey)
    try:
        wits = (uniform, heavy, uniform)
        bn.lib.tune("PLAN_FUSED", 0)
        off = [bn.groth16GenProof(w, key, r=R32, s=S32) for w in wits]
        bn.lib.tune("PLAN_FUSED", 1)
        on = [bn.groth16GenProof(w, key, r=R32, s=S32) for w in wits]
        assert on == off
        assert on[0] == on[2] == circ.expected_proof(R32, S32), "the uniform witness's proof against the closed form"
        assert on[1] == orc.groth16_prove(heavy, pkey, R32, S32, workers=8), "the boolean-heavy witness's proof against the oracle's prover"
        assert on[1] != on[0]
    finally:
        bn.lib.tune("PLAN_FUSED", None)
        key.free()
        circ.free()
