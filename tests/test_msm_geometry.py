"""CPU: the geometry the MSM's host driver decides for a plan (msm.hip: msm_plan_geometry, read through
wsnark_selftest_msm_geometry) -- the sum's shape, the grouping pass, the reduction tail -- on the smallest inputs on each side of every
rule, the production shapes (the 2^20 table plan: c = 20, 16 pieces of 2^15 buckets, chunks of 8, a second chunk level of 4), the shards,
the error returns and one row per switch the geometry reads.

Every row is compared (i) word for word with tests/golden/msm_geometry.json and (ii) with the two Python models the kernel tests are
built on, grouping_patterns.plan_geometry and tail_patterns.tail_geometry, on the fields those model (lmax is an input of the first
model: it comes from the fixture, so the rules that choose it are pinned by (i) alone).  The fixture was recorded from the commit
BEFORE msm_plan_geometry existed: msm_plan_begin's own arithmetic, dumped right after it ran, with its reservations skipped; never
from the code under test.  The hook is pure host arithmetic; the emulator library is only what carries it on a machine without a GPU."""
import pytest

import grouping_patterns as gp
import tail_patterns as tp
from conftest import load_golden
from emul_util import emul_bn128

AUTO = "auto"          # table_c: the width msm_table_window gives n pairs
OK, ERR_SIZE, ERR_ARG = 0, 1, 4

SIZES = [1, 15, 16, 1 << 10, (1 << 16) - 1, 1 << 16, 1 << 17, (1 << 20) - 1, 1 << 20, 5 * (1 << 18) - 1, 5 * (1 << 18), 1 << 22, 1 << 24]


def _rows():
    """name -> (n, table_c, shard, {switch: value})"""
    rows = {}
    for n in SIZES:
        rows["n%d_windows" % n] = (n, 0, (0, 1), {})
        rows["n%d_table" % n] = (n, AUTO, (0, 1), {})
    # forced shapes
    rows["narrow_table_c16_at_2^20"] = (1 << 20, 16, (0, 1), {})               # the by_tasks cap on lmax (2^19 tasks)
    for n in (1 << 15, 1 << 17, 1 << 20):                                       # exactly 2^16 buckets: lmax = 16 -- unless it is 16 or less already (2^15)
        rows["table_c17_n%d" % n] = (n, 17, (0, 1), {})
    rows["table_c12_n2048"] = (2048, 12, (0, 1), {})                            # 2^11 buckets under 45 056 entries: below the lmin = 8 rule
    rows["table_c12_n4096"] = (4096, 12, (0, 1), {})                            # ... under 90 112 entries: the rule
    # shards
    for name, n, tc in (("n1024_windows", 1 << 10, 0), ("n2^20_windows", 1 << 20, 0), ("n2^20_table", 1 << 20, AUTO)):
        rows[name + "_shard_3_8"] = (n, tc, (3, 8), {})
    rows["n2^20_table_shard_owns_no_window"] = (1 << 20, AUTO, (30, 32), {})
    rows["n0"] = (0, 0, (0, 1), {})
    # errors
    rows["err_n2^28_windows"] = (1 << 28, 0, (0, 1), {})                        # n W reaches 2^32
    rows["err_n2^28_table"] = (1 << 28, AUTO, (0, 1), {})                       # table rows x n reaches 2^31
    rows["err_n_above_2^28"] = ((1 << 28) + 1, 0, (0, 1), {})
    rows["err_world_0"] = (1 << 10, 0, (0, 0), {})
    rows["err_table_c23"] = (1 << 10, 23, (0, 1), {})
    # one row per switch, at the smallest n where it changes a field
    rows["MSM_C"] = (1, 0, (0, 1), {"MSM_C": 5})
    rows["MSM_CHUNK"] = (1, 0, (0, 1), {"MSM_CHUNK": 2})
    rows["TAIL_BITS"] = (20, AUTO, (0, 1), {"TAIL_BITS": 3})                    # c = 5: the first bucket set larger than 2^3
    rows["TAIL_L2"] = (5120, AUTO, (0, 1), {"TAIL_L2": 2})                      # c = 13: the first table plan cut into pieces
    rows["MSM_LMAX"] = (1, 0, (0, 1), {"MSM_LMAX": 4})
    rows["MSM_HOT_MIN"] = (1, 0, (0, 1), {"MSM_HOT_MIN": 2})
    rows["MSM_LO_BITS"] = (1, 0, (0, 1), {"MSM_LO_BITS": 1})
    rows["MSM_ENTRY64"] = (1, 0, (0, 1), {"MSM_ENTRY64": 1})
    rows["TABLE_C"] = (1, AUTO, (0, 1), {"TABLE_C": 12})                        # (read by msm_table_window)
    return rows


ROWS = _rows()
EXPECTED_RC = {"err_n2^28_windows": ERR_SIZE, "err_n2^28_table": ERR_SIZE, "err_n_above_2^28": ERR_SIZE, "err_world_0": ERR_ARG, "err_table_c23": ERR_ARG}
ALL_ZERO = set(EXPECTED_RC) | {"n0", "n2^20_table_shard_owns_no_window"}


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


@pytest.fixture(scope="module")
def golden():
    return load_golden("msm_geometry.json")["rows"]


def geometry(bn, tune, name):
    n, tc, shard, switches = ROWS[name]
    for k, v in switches.items():
        tune(bn.lib, k, v)
    return bn.msm_geometry(n, bn.MSM_TABLE_C_AUTO if tc == AUTO else tc, shard)


def test_fixture_holds_exactly_these_rows(golden):
    assert set(golden) == set(ROWS)
    assert all(len(r["words"]) == 34 for r in golden.values())


@pytest.mark.parametrize("name", list(ROWS))
def test_geometry_row(bn, tune, golden, name):
    n, tc, shard, switches = ROWS[name]
    rc, w = geometry(bn, tune, name)
    want = dict(zip(bn.MSM_GEOMETRY, golden[name]["words"]))
    # (i) the fixture
    assert rc == golden[name]["rc"] == EXPECTED_RC.get(name, OK)
    assert w == want, {k: (w[k], want[k]) for k in w if w[k] != want[k]}
    if name in ALL_ZERO:
        assert not any(w.values())
        return
    flat = tc != 0
    assert (w["n"], w["flat"], w["w_off"], w["w_stride"]) == (n, int(flat), shard[0], shard[1])
    # (ii) the tail's model: every field it has
    geo = tp.tail_geometry(w["c"], flat, chunk=switches.get("MSM_CHUNK"), tail_bits=switches.get("TAIL_BITS"), tail_l2=switches.get("TAIL_L2"))
    assert geo == tp.Geometry(w["c"], flat, *(w[k] for k in tp.Geometry._fields[2:-1]), bool(w["reduce"]))
    # ... and the planner's, where it applies: it models neither MSM_LO_BITS nor the low bits given up for entries that no longer fit
    # in 4 bytes (its docstring: "sizes of the tests only"), i.e. up to 23 index bits
    if "MSM_LO_BITS" not in switches and ((w["Wall"] if flat else 1) * n - 1).bit_length() <= 23:
        model = gp.plan_geometry(n, w["c"], flat, shard, lmax=want["lmax"], hot_min=switches.get("MSM_HOT_MIN"), entry64="MSM_ENTRY64" in switches)
        skip = ("once", "bthr")          # (msm_plan_finish's: not geometry)
        assert {k: w[k] for k in model if k not in skip} == {k: v for k, v in model.items() if k not in skip}
    # what neither model has, from the definitions
    assert w["tW"] == w["groups"] * w["tP"] and w["groups"] == (1 if flat else w["W"]) and w["tP"] * w["tNB"] == w["NB"]
    assert w["nrows"] == (w["logJ"] + 1 + (w["tP"] - 1).bit_length() + (w["m2"] > 1) if w["reduce"] else w["nsum"])
    assert w["hot_cap"] == n * w["W"] // w["lmax"] + w["nbuckets"] + 16
    assert (w["HB"], w["tile"], w["thr"], w["ps_valid"], w["bthr"]) == (w["NB"] >> w["lo_bits"], 1024, 1024, 1, 0)


@pytest.mark.parametrize("name", [k for k, v in ROWS.items() if v[3]])
def test_switch_row_changes_a_field(bn, tune, name):
    """a switch row is worth its place only if the switch decides something at that size"""
    n, tc, shard, _ = ROWS[name]
    plain = bn.msm_geometry(n, bn.MSM_TABLE_C_AUTO if tc == AUTO else tc, shard)
    assert geometry(bn, tune, name) != plain


def test_production_shape(bn, golden):
    """the 2^20 table plan as DESIGN.md describes it, read from the fixture: c = 20, 13 table rows, 16 pieces of 2^15 buckets, chunks
    of 8 with a second level of 4, 4096 bins of 7 low bits, 4-byte entries, tasks of at most 52 entries (twice the mean load of 26)"""
    w = dict(zip(bn.MSM_GEOMETRY, golden["n%d_table" % (1 << 20)]["words"]))
    assert (w["c"], w["Wall"], w["tP"], w["tNB"], w["m1"], w["m2"]) == (20, 13, 16, 1 << 15, 8, 4)
    assert (w["lo_bits"], w["nbins"], w["e32"], w["lmax"]) == (7, 4096, 1, 52)
