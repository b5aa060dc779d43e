"""The reduction tails' latency levels on the lane's third queue (prove.hip: PROVE_TAIL_SIDE, PROVE_FULL_SIZE; msm.hip:
msm_launch_tail_chunks / msm_launch_tail_levels).  Shared by tests/test_emul_tail_side_queue.py (CPU: the sources under the thread
emulator, 2^10) and tests/test_gpu_tail_side_queue.py (-m gpu: 2^12 and 2^14 on the device).

No kernel's arithmetic depends on the queue it runs on, so every check is an equality of bytes: the proof with the switch on is the
proof with it off and the closed form; proofs back to back on one lane, which reuse the launch slots' chunk sums, tree halves, rows
and pinned sums, are each their own switch-off proof; a stand-alone sum with planted bucket sums (tests/tail_patterns.py) whose
levels run on the third queue is the oracle's."""
import random

import tail_patterns as tp
from wasmsnark_amd import synth
from wasmsnark_amd._lib import WsnarkError

R32, S32 = bytes(range(5, 37)), bytes(range(70, 102))
# forced tail geometry per table window c: (MSM_CHUNK, TAIL_BITS, TAIL_L2) -- at least two pieces per bucket set (msm_rows runs), the
# second chunk level on (msm_chunks2 runs); None: the geometry the library chooses at that size
FORCED = {10: (2, 7, 4), 12: (4, 9, 2), 14: (4, 11, 2)}

_keys = {}


def native(bn, tag, logd):
    """(witness, another witness, resident key, closed-form proof of the first) of the library's generator, one per backend and size.
    The other witness is the first with every eighth signal replaced: the prover checks no constraint, its proof is only ever compared
    with a proof of the same bytes."""
    k = (tag, logd)
    if k not in _keys:
        circ = synth.NativeCircuit(bn.lib, logd, n_public=3, seed=21, style="rows")
        sec, _ = circ.build_sections()
        wit = circ.witness_bin()
        rnd = random.Random(logd)
        other = bytearray(wit)
        for i in range(3, circ.n_vars, 8):
            other[32 * i:32 * i + 32] = rnd.randrange(synth.R).to_bytes(32, "little")
        _keys[k] = (wit, bytes(other), bn.load_key(sections=sec), circ.expected_proof(R32, S32))
    return _keys[k]


def free_keys():
    for _, _, key, _ in _keys.values():
        key.free()
    _keys.clear()


def force(bn, tune, logd, forced):
    """the full-size arrangement at this size, on two queues; `forced`: the small tail geometry of FORCED"""
    tune(bn.lib, "PROVE_FULL_SIZE", 1)
    if forced:
        chunk, bits, l2 = FORCED[logd]
        geo = tp.tail_geometry(logd, True, chunk, bits, l2)
        assert geo.tP >= 2 and geo.m2 > 1, geo
        tune(bn.lib, "MSM_CHUNK", chunk)
        tune(bn.lib, "TAIL_BITS", bits)
        tune(bn.lib, "TAIL_L2", l2)


def prove(bn, wit, key, side):
    bn.lib.tune("PROVE_TAIL_SIDE", side)
    try:
        return bn.groth16GenProof(wit, key, r=R32, s=S32)
    finally:
        bn.lib.tune("PROVE_TAIL_SIDE", None)


def check_on_is_off(bn, tune, tag, logd, forced):
    wit, _, key, want = native(bn, tag, logd)
    assert key.table["c_w"] == key.table["c_h"] == logd
    force(bn, tune, logd, forced)
    off = prove(bn, wit, key, 0)
    for side in (1, None):                 # on wherever a third queue exists; the default
        on = prove(bn, wit, key, side)
        assert on == off, (side, logd, forced)
    assert off == want, (logd, forced)
    # the small arrangement (B2 already on the third queue): the batched G1 tail's levels behind it
    tune(bn.lib, "PROVE_FULL_SIZE", 0)
    assert prove(bn, wit, key, 1) == want, ("small arrangement", logd, forced)
    # one queue: the switch has nothing to move
    tune(bn.lib, "PROVE_OVERLAP", 0)
    assert prove(bn, wit, key, 1) == want, ("one queue", logd, forced)


def check_back_to_back(bn, tune, tag, logd, forced):
    """eight proofs on one lane, two witnesses in alternation: a slot buffer rewritten before the side queue has read it would put
    one witness's sums into the other's proof"""
    wit, other, key, want = native(bn, tag, logd)
    force(bn, tune, logd, forced)
    ref = [prove(bn, w, key, 0) for w in (wit, other)]
    assert ref[0] == want and ref[1] != want
    tune(bn.lib, "PROVE_TAIL_SIDE", 1)
    got = [bn.groth16GenProof((wit, other)[i % 2], key, r=R32, s=S32) for i in range(8)]
    for i, p in enumerate(got):
        assert p == ref[i % 2], (i, logd, forced)


def check_rejected_call(bn, tune, tag, logd):
    """a witness one signal short is rejected between two proofs; the proof after it is right"""
    wit, other, key, want = native(bn, tag, logd)
    force(bn, tune, logd, True)
    tune(bn.lib, "PROVE_TAIL_SIDE", 1)
    assert bn.groth16GenProof(wit, key, r=R32, s=S32) == want
    try:
        bn.groth16GenProof(wit[:-32], key, r=R32, s=S32)
    except (WsnarkError, ValueError):
        pass
    else:
        raise AssertionError("a short witness was accepted")
    assert bn.groth16GenProof(wit, key, r=R32, s=S32) == want
    off = prove(bn, other, key, 0)
    assert bn.groth16GenProof(other, key, r=R32, s=S32) == off


# Stand-alone sums over resident points: TABLE_C = 9 -- one set of 256 buckets cut by TAIL_BITS = 7 into two pieces of 128, chunks of
# 2 --, the second chunk level off (TAIL_L2 = 1) or folding 2 / 8 chunk pairs.  One point set per curve holds the pairs of every
# pattern (2^12 and more); a pattern's scalars leave the others' pairs at zero.
TABLE = dict(c=9, chunk=2, bits=7)


def check_planted_sums(bn, orc, tune, g, splits=(1, 0)):
    """splits: the lane-split level kernels (1) and the one-lane ones (0)"""
    tune(bn.lib, "TABLE_C", TABLE["c"])
    tune(bn.lib, "MSM_CHUNK", TABLE["chunk"])
    tune(bn.lib, "TAIL_BITS", TABLE["bits"])
    rnd = random.Random(400 + g)
    pl = tp.Planter(bn, orc, g, seed=40 + g)
    runs = []
    for l2 in (1, 2, 8):
        geo = tp.tail_geometry(TABLE["c"], True, TABLE["chunk"], TABLE["bits"], l2)
        assert geo.tP == 2 and geo.m2 == l2
        cases = tp.catalogue(geo, rnd) + [("dense", tp.dense(geo, rnd), None), ("sparse cancelled", tp.sparse_cancelled(geo, rnd), None)]
        for name, targets, seen in cases:
            if seen is not None:
                tp.assert_branches_planted(geo, name, seen)
            runs.append((geo, name, pl.plant(targets)))
    pts = b"".join(p[1] for *_, p in runs)
    n = sum(p[3] for *_, p in runs)
    assert n >= 1 << 12
    h = bn.load_points(g, pts)
    assert h.table["c"] == TABLE["c"]
    try:
        off = 0
        for geo, name, (sc, _, want, cnt) in runs:
            full = bytes(32 * off) + sc + bytes(32 * (n - off - cnt))
            off += cnt
            tune(bn.lib, "TAIL_L2", geo.m2)
            for split in splits:
                for name_ in ("TAIL_PAIR_G1", "TAIL_QUAD_G2"):
                    tune(bn.lib, name_, split)
                tune(bn.lib, "PROVE_TAIL_SIDE", 1)
                with tp.Timing(bn.lib) as t:
                    got = h.multiexp(full)
                    assert t.kernels() == tp.expected_kernels(geo), (name, geo)
                assert got == want, (name, geo, split)
                if split == splits[0]:
                    tune(bn.lib, "PROVE_TAIL_SIDE", 0)
                    assert h.multiexp(full) == want, (name, geo, "side off")
                    if name != "dense":
                        assert got == orc.g_affine(g, orc.multiexp(g, "multiexp2" if g == 1 else "multiexp", full, pts, n)), (name, geo)
    finally:
        h.free()
