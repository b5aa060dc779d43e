"""GPU (run with -m gpu on an MI355X): the MSM reduction tail (msm_chunks, msm_chunks2, msm_tree, msm_rows, the host's Horner chain) at
full-size geometries, fed PLANTED bucket sums (tests/tail_patterns.py) that make its full additions meet equal, opposite and
infinity operands: a per-window plan at c = 16 (one piece, or eight pieces folded by msm_rows) and resident bases of 2^18 and 2^20
points at their default table width (msm_chunks2 runs from 2^17 buckets on), on the lane-split and the one-lane tail curves.
Every sum is compared bit for bit with its closed form (the oracle's double-and-add); every case checks, through the library's
per-kernel timing, that the kernels it targets ran.  And mul_base_kernel (fixedbase.hip) against the oracle on the device."""
import random

import pytest

import tail_patterns as tp

pytestmark = pytest.mark.gpu
SPLIT = ("TAIL_PAIR_G1", "TAIL_QUAD_G2")


@pytest.fixture(scope="module")
def bn():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__
    __graft_entry__.ensure_built()
    import wasmsnark_amd
    b = wasmsnark_amd.build(device=0)
    assert b.lib.path.endswith("wasmsnark_amd/libwsnark.so")
    return b


def _set_split(bn, tune, split):
    for name in SPLIT:
        tune(bn.lib, name, split)


@pytest.mark.parametrize("g,split,bits", [(1, 1, None), (1, 0, 12), (2, 1, 12), (2, 0, None)])
def test_per_window_c16_tail_patterns(bn, orc, tune, g, split, bits):
    """window 0 of a c = 16 plan (2^15 buckets, chunks of 8): one piece, or TAIL_BITS = 12 -- eight pieces of 4096 buckets"""
    geo = tp.tail_geometry(16, False, None, bits)
    tune(bn.lib, "MSM_C", 16)
    if bits:
        tune(bn.lib, "TAIL_BITS", bits)
    _set_split(bn, tune, split)
    rnd = random.Random(16 * g + split)
    pl = tp.Planter(bn, orc, g, seed=g)
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


# (curve, log2 points, lane-split tail, patterns): the default table width -- c = 18 (2^17 buckets, 64 pieces of 2^11, chunks of 4,
# msm_chunks2 folding 4) and c = 20 (2^19 buckets, 16 pieces of 2^15, chunks of 8, msm_chunks2 folding 4); the one-lane tail curves
# on the patterns that reach the second chunk level, the trees' half merge and msm_rows.
FULL = ("uniform", "alternating", "mirrored", "mirrored pieces", "solved chunks", "solved chunks2", "sparse")
ONE_LANE = ("uniform", "mirrored", "mirrored pieces", "solved chunks2")
TABLE_CASES = [(g, logn, split, FULL if split else ONE_LANE) for logn in (18, 20) for g in (1, 2) for split in (1, 0)]


@pytest.mark.parametrize("k", range(len(TABLE_CASES)))
def test_resident_bases_tail_patterns(bn, orc, tune, k):
    g, logn, split, names = TABLE_CASES[k]
    n = 1 << logn
    _set_split(bn, tune, split)
    rnd = random.Random(100 + k)
    pl = tp.Planter(bn, orc, g, seed=k)
    sz = pl.sz

    def table_geo(h):
        c = h.table["c"]
        assert c == logn                                # the default width at 2^18 and 2^20
        return tp.tail_geometry(c, True)

    def run(h, geo, name, planted, off, total):
        sc, _, want, cnt = planted
        full = bytes(32 * off) + sc + bytes(32 * (total - off - cnt))
        with tp.Timing(bn.lib) as t:
            got = h.multiexp(full)
            assert t.kernels() == tp.expected_kernels(geo), (name, geo)
        assert got == want, (name, geo, split)

    geo = tp.tail_geometry(logn, True)                  # (each load checks that its table has this width)
    assert geo.m2 == 4 and geo.reduce
    by_name = {"uniform": tp.uniform, "alternating": tp.alternating, "mirrored": tp.mirrored, "mirrored pieces": tp.mirrored_pieces,
               "solved chunks": lambda geo, rnd: tp.solved_chunks(geo, rnd), "solved chunks2": lambda geo, rnd: tp.solved_chunks2(geo, rnd)}
    for name in names:
        if name == "sparse":
            # a dense sum, then the sparse one on the same lane and geometry: ONE point set holds both
            dense = pl.plant(tp.dense(geo, rnd), shuffle=False)
            sparse = pl.plant(tp.sparse_cancelled(geo, rnd), shuffle=False)
            pts = dense[1] + sparse[1]
            pts += pts[:sz] * (n - dense[3] - sparse[3])
            h = bn.load_points(g, pts)
            try:
                assert table_geo(h) == geo
                run(h, geo, "dense", dense, 0, n)
                run(h, geo, "sparse cancelled", sparse, dense[3], n)
            finally:
                h.free()
            continue
        made = by_name[name](geo, rnd)
        targets, seen = made if isinstance(made, tuple) else (made, None)
        if seen is not None:
            tp.assert_branches_planted(geo, name, seen)
        planted = pl.plant(targets, shuffle=False)
        pts = planted[1] + planted[1][:sz] * (n - planted[3])
        h = bn.load_points(g, pts)
        try:
            assert table_geo(h) == geo
            run(h, geo, name, planted, 0, n)
        finally:
            h.free()


@pytest.mark.parametrize("g", [1, 2])
def test_mul_base_matches_oracle_on_device(bn, orc, g):
    """mul_base_kernel against the oracle's double-and-add: 0, 1, 2, r - 1, r, r + 1, 2^255, 2^256 - 1, runs of ones and zeros and
    1000 seeded values -- a count that leaves the last workgroup partial"""
    sc = tp.mul_base_scalars(random.Random(70 + g), 1000)
    assert (len(sc) // 32) % 256 != 0
    assert bn.mul_base(g, sc) == tp.oracle_mul_base(orc, g, sc)
