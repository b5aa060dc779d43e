"""Caller-written tasks for the MSM accumulation kernel (msm.hip: msm_accumulate / accumulate_range), run through
wsnark_selftest_msm_accumulate.  Shared by tests/test_emul_accumulate_patterns.py (CPU: the kernel sources under the thread emulator)
and tests/test_gpu_accumulate_patterns.py (-m gpu: the device code on an MI355X).

Every point of the table is k G with a known k -- 64 random multiples, the planted sums and their negatives, all made by the oracle's
double-and-add (never by mul_base) --, so a task's sum is (sum of +-k mod r) G by the oracle, or infinity, and the comparison is bit
for bit after normalisation.  To make entry j EQUAL (or OPPOSITE) to the running sum the table holds the affine point of
sum_{i<j} +-k_i, or its negative: the device meets it with an XYZZ accumulator whose zz is not 1 and whose X is wide.  Each planted
corner is reached both ways: stored as P with sign bit 0, and stored as -P with sign bit 1.

model() is the loop's control flow restated on the k values alone (equal / opposite = exact equality mod r): it names the branch
every entry takes, and assert_coverage() checks that the case table reaches every branch where the issue of a wrong loop would show --
a condition on the INPUTS, checked before the device is used."""
import random
from collections import namedtuple

from conftest import load_golden

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617

# the branch an entry takes.  Fast loop: the first entry starts the sum; the second goes through mmadd_fast; later ones through madd_fast
START = "START"
MMADD_OK, MMADD_REFUSED_DBL, MMADD_REFUSED_INF, ENTRY1_INFINITY = "MMADD_OK", "MMADD_REFUSED_DBL", "MMADD_REFUSED_INF", "ENTRY1_INFINITY"
FAST_OK, FAST_REFUSED_DBL, FAST_REFUSED_INF, FAST_BREAK_INFINITY = "FAST_OK", "FAST_REFUSED_DBL", "FAST_REFUSED_INF", "FAST_BREAK_INFINITY"
# generic loop (madd_wide), from the entry that made the lane leave the fast loop to the task's end
GEN_ADD, GEN_DBL, GEN_CANCEL, GEN_SKIP, GEN_COPY = "GEN_ADD", "GEN_DBL", "GEN_CANCEL", "GEN_SKIP", "GEN_COPY"
BRANCHES = (START, MMADD_OK, MMADD_REFUSED_DBL, MMADD_REFUSED_INF, ENTRY1_INFINITY, FAST_OK, FAST_REFUSED_DBL, FAST_REFUSED_INF,
            FAST_BREAK_INFINITY, GEN_ADD, GEN_DBL, GEN_CANCEL, GEN_SKIP, GEN_COPY)
REFUSALS = (MMADD_REFUSED_DBL, MMADD_REFUSED_INF, FAST_REFUSED_DBL, FAST_REFUSED_INF)
LEAVES = REFUSALS + (ENTRY1_INFINITY, FAST_BREAK_INFINITY)          # what makes a lane leave the fast loop
STRAIGHT = (START, MMADD_OK, FAST_OK)                               # a control takes nothing else

Entry = namedtuple("Entry", "k sign")        # the table's point k G (k = 0: the all-zero record, infinity) and the sign bit of its word
Case = namedtuple("Case", "name entries want")   # want: {position: branch} the case is there for, or None: a control


def value(e):
    """what the entry adds, mod r; None for infinity"""
    return None if e.k == 0 else (R - e.k if e.sign else e.k)


def model(entries):
    """accumulate_range's control flow on the k values: (labels, total) -- labels[i] the branches entry i takes, in order (the entry
    that makes the lane leave the fast loop is met again by the generic loop: two names); total = the sum mod r, 0 for infinity.
    After a refusal by mmadd_fast the fast loop offers entry 1 to madd_fast once more, which refuses for the same reason (the same
    difference of x): no name of its own."""
    v = [value(e) for e in entries]
    n = len(v)
    labels = [[] for _ in v]
    acc = k = 0
    if n and v[0] is not None:
        acc, k = v[0], 1
        labels[0].append(START)
        if n > 1:
            if v[1] is None:
                labels[1].append(ENTRY1_INFINITY)
            elif v[1] == acc:
                labels[1].append(MMADD_REFUSED_DBL)
            elif (v[1] + acc) % R == 0:
                labels[1].append(MMADD_REFUSED_INF)
            else:
                labels[1].append(MMADD_OK)
                acc, k = (acc + v[1]) % R, 2
        while k >= 2 and k < n:
            if v[k] is None:
                labels[k].append(FAST_BREAK_INFINITY)
                break
            if v[k] == acc:
                labels[k].append(FAST_REFUSED_DBL)
                break
            if (v[k] + acc) % R == 0:
                labels[k].append(FAST_REFUSED_INF)
                break
            labels[k].append(FAST_OK)
            acc = (acc + v[k]) % R
            k += 1
    for i in range(k, n):
        if v[i] is None:
            labels[i].append(GEN_SKIP)
        elif acc == 0:
            labels[i].append(GEN_COPY)
            acc = v[i]
        elif v[i] == acc:
            labels[i].append(GEN_DBL)
            acc = 2 * acc % R
        elif (v[i] + acc) % R == 0:
            labels[i].append(GEN_CANCEL)
            acc = 0
        else:
            labels[i].append(GEN_ADD)
            acc = (acc + v[i]) % R
    return labels, acc


# ------------------------------------------------------------------ scripted tasks
# A script is a string of steps: r = a random multiple of the table with a random sign bit; E / e = an entry EQUAL to the running sum,
# stored as P with sign bit 0 (E) or as -P with sign bit 1 (e); O / o = OPPOSITE to the running sum, the same two ways; I / i = the
# infinity record with sign bit 0 / 1.  E, e, O, o while the sum is infinity have nothing to aim at and are not written.
def scripted(script, randoms, rnd):
    out, acc, last = [], 0, None
    for step in script:
        if step == "r":
            k = rnd.choice(randoms)
            while k == last:                                    # (two neighbours on one table point would be a corner of their own)
                k = rnd.choice(randoms)
            e = Entry(k, rnd.randrange(2))
            last = k
        elif step in "Ii":
            e = Entry(0, 0 if step == "I" else 1)
        else:
            assert step in "EeOo" and acc != 0, (script, step)
            want = acc if step in "Ee" else R - acc
            e = Entry(want, 0) if step in "EO" else Entry(R - want, 1)
            last = e.k
        out.append(e)
        v = value(e)
        if v is not None:
            acc = (acc + v) % R
    return out


def _corner_script(L, j, step):
    return "r" * j + step + "r" * (L - 1 - j)


CONTROL_LENGTHS = (0, 1, 2, 3, 4, 5, 8, 33, 70)
SINGLE = {2: (1,), 3: (1, 2), 4: (1, 2, 3), 5: (1, 2, 3, 4), 8: (1, 2, 3, 4, 5, 6, 7), 33: (1, 2, 3, 16, 31, 32)}
WAVE_SAME = (6, 3)            # (length, position): a wavefront of 64 tasks that all leave the fast loop at entry 3
WAVE_SPREAD = 65              # a wavefront whose lane i leaves at entry i + 1 of 65
Table = namedtuple("Table", "ks vals tasks cases same_at spread_at aliases")


def _want(step, j):
    first = {"E": MMADD_REFUSED_DBL, "e": MMADD_REFUSED_DBL, "O": MMADD_REFUSED_INF, "o": MMADD_REFUSED_INF, "I": ENTRY1_INFINITY, "i": ENTRY1_INFINITY}
    later = {"E": FAST_REFUSED_DBL, "e": FAST_REFUSED_DBL, "O": FAST_REFUSED_INF, "o": FAST_REFUSED_INF, "I": FAST_BREAK_INFINITY, "i": FAST_BREAK_INFINITY}
    return {j: (first if j == 1 else later)[step]}


_tables = {}


def case_table(g):
    """The case table of curve g (the k values only: no point is computed here), its coverage asserted.  ks: the table's multiples
    (ks[0] = 0: the infinity record); vals: the words; tasks: [(start, len)]; cases[t]: the Case of task t."""
    if g in _tables:
        return _tables[g]
    rnd = random.Random(4100 + g)
    randoms = [rnd.randrange(1, R) for _ in range(64)]
    corners, controls = [], []

    def control(L, name=None):
        if L == 1 and name == "infinity":
            return Case("one entry, infinity", [Entry(0, 0)], {0: GEN_SKIP})
        return Case("control: %d entries" % L, scripted("r" * L, randoms, rnd), None)

    controls = [control(L) for L in CONTROL_LENGTHS] + [control(1, "infinity")]
    # single corners: one seeded prefix per (L, j), met by all six steps
    for L, positions in SINGLE.items():
        for j in positions:
            seed = rnd.randrange(1 << 30)
            for step in "EeOoIi":
                corners.append(Case("L=%d j=%d %s" % (L, j, step), scripted(_corner_script(L, j, step), randoms, random.Random(seed)), _want(step, j)))
    # entry 0 at infinity: the whole task runs generic
    for name, script, want in (
            ("entry 0 at infinity", "Irrr", {0: GEN_SKIP, 1: GEN_COPY, 2: GEN_ADD}),
            ("entries 0 and 1 at infinity", "iIrr", {0: GEN_SKIP, 1: GEN_SKIP, 2: GEN_COPY}),
            ("every entry at infinity", "IiIi", {0: GEN_SKIP, 3: GEN_SKIP}),
            ("entry 0 at infinity, then P, P", "IrEr", {2: GEN_DBL}),
            ("entry 0 at infinity, then P, -P, Q", "iror", {2: GEN_CANCEL, 3: GEN_COPY}),
            # after leaving the fast loop: the generic loop adds, doubles, cancels, skips an infinity, copies, adds again, ends finite
            ("[P, -P]", "ro", {1: MMADD_REFUSED_INF}),
            ("[P, -P] by the sign bit", "rO", {1: MMADD_REFUSED_INF}),
            ("[P, -P, Q]", "ror", {1: MMADD_REFUSED_INF, 2: GEN_COPY}),
            ("[P, P, -2P, Q, Q]", "rEorE", {1: MMADD_REFUSED_DBL, 2: GEN_CANCEL, 3: GEN_COPY, 4: GEN_DBL}),
            ("[P, P, -2P, Q, Q] by the sign bit", "reOre", {1: MMADD_REFUSED_DBL, 2: GEN_CANCEL, 3: GEN_COPY, 4: GEN_DBL}),
            ("generic tour after a doubling at 3", "rrrEIreOrr", {3: FAST_REFUSED_DBL, 4: GEN_SKIP, 5: GEN_ADD, 6: GEN_DBL, 7: GEN_CANCEL, 8: GEN_COPY, 9: GEN_ADD}),
            ("generic tour after a cancellation at 2", "rrorrEiorO", {2: FAST_REFUSED_INF, 3: GEN_COPY, 4: GEN_ADD, 5: GEN_DBL, 6: GEN_SKIP, 7: GEN_CANCEL, 8: GEN_COPY, 9: GEN_CANCEL}),
            ("generic tour after an infinity at 4", "rrrrirEOrrr", {4: FAST_BREAK_INFINITY, 5: GEN_ADD, 6: GEN_DBL, 7: GEN_CANCEL, 8: GEN_COPY, 9: GEN_ADD}),
            ("generic tour after entry 1 at infinity", "rIreorr", {1: ENTRY1_INFINITY, 2: GEN_ADD, 3: GEN_DBL, 4: GEN_CANCEL, 5: GEN_COPY, 6: GEN_ADD})):
        corners.append(Case(name, scripted(script, randoms, rnd), want))
    # section 1: corner, corner, control, ... (corners beside controls and beside each other, on even and on odd tasks -- buckets and
    # partial slots), filled up to whole wavefronts with controls
    lengths = [2, 3, 4, 5, 8, 33, 7, 2, 12, 3]
    cases, c = [], 0
    for i, corner in enumerate(corners):
        cases.append(corner)
        if i % 2 == 1:
            cases.append(controls[c] if c < len(controls) else control(lengths[c % len(lengths)]))
            c += 1
    while c < len(controls) or len(cases) % 64:
        cases.append(controls[c] if c < len(controls) else control(lengths[c % len(lengths)]))
        c += 1
    # section 2: one wavefront, every lane leaves at the same position (the steps alternate)
    same_at = len(cases)
    L, j = WAVE_SAME
    for i in range(64):
        step = "EeOoIi"[i % 6]
        cases.append(Case("same position, lane %d: L=%d j=%d %s" % (i, L, j, step), scripted(_corner_script(L, j, step), randoms, rnd), _want(step, j)))
    # section 3: one wavefront, lane i leaves at position i + 1
    spread_at = len(cases)
    for i in range(64):
        step = "EoIeOi"[i % 6]
        cases.append(Case("spread, lane %d: L=%d j=%d %s" % (i, WAVE_SPREAD, i + 1, step),
                          scripted(_corner_script(WAVE_SPREAD, i + 1, step), randoms, rnd), _want(step, i + 1)))
    for L in (5, 2, 9):
        cases.append(control(L))
    # the words, task after task
    vals, tasks, index, ks = [], [], {0: 0}, [0]
    for case in cases:
        tasks.append((len(vals), len(case.entries)))
        for e in case.entries:
            if e.k not in index:
                index[e.k] = len(ks)
                ks.append(e.k)
            vals.append(index[e.k] | (e.sign << 31))
    # section 4: tasks over the ranges of earlier ones -- a corner's range again (one with an odd, non-zero start), a control's, and
    # the tail of a corner's range from its entry 1 on (another first entry over the same words)
    aliases = []
    odd = next(t for t, case in enumerate(cases) if case.want and tasks[t][0] % 2 == 1 and tasks[t][1] >= 4)
    even = next(t for t, case in enumerate(cases) if case.want is None and tasks[t][0] and tasks[t][0] % 2 == 0 and tasks[t][1] >= 3)
    tail = next(t for t, case in enumerate(cases) if case.want and tasks[t][0] % 2 == 0 and tasks[t][1] == 8 and 3 in case.want and case.entries[3].k)
    for t, skip in ((odd, 0), (even, 0), (tail, 1), (spread_at + 40, 0)):
        aliases.append((len(cases), t))
        cases.append(Case("the range of task %d from its entry %d on" % (t, skip), cases[t].entries[skip:], None if skip else cases[t].want))
        tasks.append((tasks[t][0] + skip, tasks[t][1] - skip))
    while len(cases) <= 256 or len(cases) % 256 == 0:
        cases.append(control(3))
        tasks.append((len(vals), 3))
        for e in cases[-1].entries:
            vals.append(index[e.k] | (e.sign << 31))
    T = Table(ks, vals, tasks, cases, same_at, spread_at, aliases)
    assert_coverage(T)
    _tables[g] = T
    return T


def assert_coverage(T):
    """The case table reaches every branch, and the refusals where a wrong loop would show: a condition on the inputs."""
    seen = set()                       # (branch, position, sign bit, length)
    after = set()                      # generic branches met at or after the entry that left the fast loop
    for t, case in enumerate(T.cases):
        labels, _ = model(case.entries)
        flat = [b for l in labels for b in l]
        if case.want is None:
            assert all(b in STRAIGHT for b in flat), ("a control meets a corner", t, case.name, flat)
        else:
            for pos, b in case.want.items():
                assert b in labels[pos], ("the case misses what it is there for", t, case.name, pos, b, labels[pos])
        left = False
        for pos, (e, l) in enumerate(zip(case.entries, labels)):
            for b in l:
                seen.add((b, pos, e.sign, len(case.entries)))
                left = left or b in REFUSALS
                if left and b in (GEN_ADD, GEN_DBL, GEN_CANCEL, GEN_COPY):
                    after.add(b)
    names = {b for b, *_ in seen}
    assert names == set(BRANCHES), sorted(set(BRANCHES) - names)
    for b in REFUSALS:
        for sign in (0, 1):
            assert any(x[0] == b and x[2] == sign for x in seen), (b, "sign bit", sign)
    for b in (FAST_REFUSED_DBL, FAST_REFUSED_INF):
        for sign in (0, 1):
            assert any(x[0] == b and x[1] == 2 and x[2] == sign for x in seen), (b, "position 2", sign)
            assert any(x[0] == b and x[1] == 3 and x[2] == sign for x in seen), (b, "position 3", sign)
            assert any(x[0] == b and x[1] == x[3] - 1 and x[1] >= 2 and x[2] == sign for x in seen), (b, "the last entry", sign)
            assert any(x[0] == b and x[1] >= 31 and x[2] == sign for x in seen), (b, "position >= 31", sign)
    assert after == {GEN_ADD, GEN_DBL, GEN_CANCEL, GEN_COPY}, after
    # the lane neighbourhoods: a wavefront that leaves at one position, one whose lanes all leave at different positions
    assert T.same_at % 64 == 0 and T.spread_at % 64 == 0

    def leaves(t):
        labels, _ = model(T.cases[t].entries)
        return [pos for pos, l in enumerate(labels) if any(b in LEAVES for b in l)][:1]

    assert {tuple(leaves(t)) for t in range(T.same_at, T.same_at + 64)} == {(WAVE_SAME[1],)}
    assert sorted(leaves(t)[0] for t in range(T.spread_at, T.spread_at + 64)) == list(range(1, 65))
    # corners on buckets (even tasks) and on partial slots (odd tasks); launch sizes; shared ranges
    for parity in (0, 1):
        assert any(case.want and t % 2 == parity for t, case in enumerate(T.cases))
    assert len(T.cases) > 256 and len(T.cases) % 256 and T.cases[0].want
    assert any(T.tasks[t] == T.tasks[src] and T.tasks[t][0] % 2 == 1 for t, src in T.aliases)
    assert any(T.tasks[t][0] == T.tasks[src][0] + 1 for t, src in T.aliases)
    assert all(s + n <= len(T.vals) for s, n in T.tasks) and all((w & 0x7FFFFFFF) < len(T.ks) for w in T.vals)


# ------------------------------------------------------------------ points and expected sums: the oracle's double-and-add
_planted = {}


def planted(orc, g):
    """(table, points, expected): points = the table's affine points as the MSM entry points take them; expected[t] = the normalised
    sum of task t.  Computed once per curve and shared."""
    if g in _planted:
        return _planted[g]
    T = case_table(g)
    sz = 64 if g == 1 else 128
    gen = bytes.fromhex(load_golden("groups.json")["g%d" % g]["gen"])
    zero = orc.g_affine(g, orc.g_zero(g))
    mult = {0: zero}

    def times(k):
        if k not in mult:
            if R - k in mult:
                mult[k] = orc.g_affine(g, orc.g_neg(g, mult[R - k]))
            else:
                mult[k] = orc.g_affine(g, orc.g_times_scalar(g, gen, k.to_bytes(32, "little")))
        return mult[k]

    points = b"".join(bytes(sz) if k == 0 else times(k)[:sz] for k in T.ks)
    expected = [times(model(case.entries)[1]) for case in T.cases]
    _planted[g] = (T, points, expected)
    return _planted[g]


def describe(T, t):
    """task t for an assertion message: its name, length and the branch of every entry that is not on the straight path"""
    labels, total = model(T.cases[t].entries)
    odd = {pos: l for pos, l in enumerate(labels) if any(b not in STRAIGHT for b in l)}
    return "task %d (%s, %s), %d entries from word %d, sum %s; branches %r" % (
        t, T.cases[t].name, "partial slot" if t % 2 else "bucket", T.tasks[t][1], T.tasks[t][0], "infinity" if total == 0 else "finite", odd)


def check_launch(bn, g, T, points, expected, n_tasks):
    """the first n_tasks tasks in one launch, every sum bit for bit"""
    got = bn.selftest_msm_accumulate(g, points, T.vals, T.tasks[:n_tasks])
    assert len(got) == n_tasks
    bad = [t for t in range(n_tasks) if got[t] != expected[t]]
    assert not bad, "G%d, a launch of %d tasks: %d wrong sums, tasks %r; the first: %s" % (
        g, n_tasks, len(bad), bad[:64], "; ".join(describe(T, t) for t in bad[:4]))


def check_error_calls(bn, g, T, points, expected):
    """bad arguments are refused before anything is launched (WSNARK_ERR_ARG), `out` stays as it was, and a good call afterwards works"""
    import ctypes as C

    import pytest

    from wasmsnark_amd import WsnarkError
    osz = 96 if g == 1 else 192
    n = 5
    fill = bytes([0x5A]) * (n * osz)
    bad_calls = [
        ("an index past n_points", g, T.vals[:7] + [len(T.ks)] + T.vals[8:], T.tasks[:n]),
        ("an index past n_points, sign bit set", g, T.vals[:7] + [len(T.ks) | (1 << 31)] + T.vals[8:], T.tasks[:n]),
        ("start + len past n_vals", g, T.vals, T.tasks[:n - 1] + [(len(T.vals) - 2, 3)]),
        ("start past n_vals, len 0", g, T.vals, T.tasks[:n - 1] + [(len(T.vals) + 1, 0)]),
        ("start + len wraps 2^32", g, T.vals, T.tasks[:n - 1] + [(0xFFFFFFFF, 2)]),
        ("g = 3", 3, T.vals, T.tasks[:n]),
        ("g = 0", 0, T.vals, T.tasks[:n]),
        ("more than 2^16 tasks", g, T.vals, T.tasks[:n] + [(0, 0)] * (1 << 16)),
    ]
    for name, gg, vals, tasks in bad_calls:
        out = (C.c_uint8 * (n * osz)).from_buffer_copy(fill)
        with pytest.raises(WsnarkError) as err:
            bn.selftest_msm_accumulate(gg, points, vals, tasks, out=out)
        assert err.value.code == 4, (name, err.value)
        assert bytes(out) == fill, (name, "out was written")
        assert bn.selftest_msm_accumulate(g, points, T.vals, T.tasks[:n]) == expected[:n], ("the call after", name)
