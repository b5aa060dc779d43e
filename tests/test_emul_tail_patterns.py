"""CPU: the MSM reduction tail (msm_chunks, msm_chunks2, msm_tree, msm_rows, the host's Horner chain) under the thread emulator, fed
PLANTED bucket sums (tests/tail_patterns.py) that make its full additions meet equal, opposite and infinity operands -- at every
chunk / piece geometry the switches MSM_C / TABLE_C, MSM_CHUNK, TAIL_BITS, TAIL_L2, TAIL_PAIR_G1 / TAIL_QUAD_G2 select.  Every sum
is compared bit for bit with its closed form and with the oracle's multiexp; every case checks, through the library's per-kernel
timing, that the kernels it targets ran."""
import random

import pytest

import tail_patterns as tp
from emul_util import emul_bn128

SPLIT = ("TAIL_PAIR_G1", "TAIL_QUAD_G2")


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


def _oracle(orc, g, sc, pts, n):
    return orc.g_affine(g, orc.multiexp(g, "multiexp2" if g == 1 else "multiexp", sc, pts, n))


def _set_split(bn, tune, split):
    for name in SPLIT:
        tune(bn.lib, name, split)


# (c, MSM_CHUNK, TAIL_BITS): chunks of 2 .. 32 buckets; one piece per window (TAIL_BITS unset) or 4 / 8 pieces (msm_rows runs).
# Window 0 is the only non-empty one; its buckets are the targets.
PER_WINDOW = [(6, 2, None), (7, 4, 4), (8, None, None), (8, 2, 4), (9, 16, 6), (10, 32, None)]


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("k", range(len(PER_WINDOW)))
def test_per_window_tail_patterns(bn, orc, tune, g, k):
    c, chunk, bits = PER_WINDOW[k]
    split = (k + g) % 2            # each curve: the lane-split tail (1) and the one-lane tail (0), with and without pieces
    geo = tp.tail_geometry(c, False, chunk, bits)
    tune(bn.lib, "MSM_C", c)
    if chunk:
        tune(bn.lib, "MSM_CHUNK", chunk)
    if bits:
        tune(bn.lib, "TAIL_BITS", bits)
    _set_split(bn, tune, split)
    rnd = random.Random(1000 * g + k)
    pl = tp.Planter(bn, orc, g, seed=k)
    msm = bn.g1_multiexp if g == 1 else bn.g2_multiexp
    cases = tp.catalogue(geo, rnd)
    cases += [("dense", tp.dense(geo, rnd), None), ("sparse cancelled", tp.sparse_cancelled(geo, rnd), None),
              ("dense", tp.dense(geo, rnd), None), ("sparse filled", tp.sparse_cancelled(geo, rnd, filled=True), None)]
    for name, targets, seen in cases:
        if seen is not None:
            tp.assert_branches_planted(geo, name, seen)
        sc, pts, want, n = pl.plant(targets)
        with tp.Timing(bn.lib) as t:
            got = msm(sc, pts)
            assert t.kernels() == tp.expected_kernels(geo), (name, geo)
        assert got == want, (name, geo, split)
        assert got == _oracle(orc, g, sc, pts, n), (name, geo, split)
    assert geo.reduce == (bits is not None)


# Table plans: points made resident (bn.load_points) with TABLE_C = 9 -- one set of 256 buckets cut by TAIL_BITS = 7 into two
# pieces of 128, chunks of 2 --, the second chunk level off (TAIL_L2 = 1) or folding 2 / 4 / 8 chunk pairs (msm_chunks2).  One point
# set per curve holds the entries of every pattern; a pattern's scalars leave the others' pairs at zero.
TABLE = dict(c=9, chunk=2, bits=7)
TABLE_RUNS = [(1, 1), (2, 0), (4, 1), (8, 0), (8, 1)]          # (TAIL_L2, lane-split tail)


@pytest.mark.parametrize("g", [1, 2])
def test_table_plan_tail_patterns(bn, orc, tune, g):
    tune(bn.lib, "TABLE_C", TABLE["c"])
    tune(bn.lib, "MSM_CHUNK", TABLE["chunk"])
    tune(bn.lib, "TAIL_BITS", TABLE["bits"])
    rnd = random.Random(77 + g)
    pl = tp.Planter(bn, orc, g, seed=g)
    runs = []                                       # (geometry, lane-split tail, pattern, planted); each sparse sum right after a dense one
    for l2, split in TABLE_RUNS:
        geo = tp.tail_geometry(TABLE["c"], True, TABLE["chunk"], TABLE["bits"], l2)
        assert geo.tP == 2 and geo.m2 == l2
        cases = tp.catalogue(geo, rnd) if split or l2 == 1 else [c for c in tp.catalogue(geo, rnd) if c[0] == "solved chunks2"]
        cases += [("dense", tp.dense(geo, rnd), None), ("sparse cancelled", tp.sparse_cancelled(geo, rnd), None)]
        for name, targets, seen in cases:
            if seen is not None:
                tp.assert_branches_planted(geo, name, seen)
            runs.append((geo, split, name, pl.plant(targets)))
    pts = b"".join(p[1] for *_, p in runs)
    n = sum(p[3] for *_, p in runs)
    h = bn.load_points(g, pts)
    assert h.table["c"] == TABLE["c"]
    try:
        off = 0
        for geo, split, name, (sc, _, want, cnt) in runs:
            full = bytes(32 * off) + sc + bytes(32 * (n - off - cnt))
            off += cnt
            tune(bn.lib, "TAIL_L2", geo.m2)
            _set_split(bn, tune, split)
            with tp.Timing(bn.lib) as t:
                got = h.multiexp(full)
                assert t.kernels() == tp.expected_kernels(geo), (name, geo)
            assert got == want, (name, geo, split)
            if name != "dense":
                assert got == _oracle(orc, g, full, pts, n), (name, geo, split)
    finally:
        h.free()


@pytest.mark.parametrize("g", [1, 2])
def test_mul_base_matches_oracle(bn, orc, g):
    """mul_base_kernel (fixedbase.hip) against the oracle's double-and-add on the edge scalars and seeded random ones"""
    sc = tp.mul_base_scalars(random.Random(9 + g), 300)
    assert (len(sc) // 32) % 256 != 0
    assert bn.mul_base(g, sc) == tp.oracle_mul_base(orc, g, sc)
