"""ONE reduction tail for the prover's C and H sums (prove.hip: PROVE_CH_TAIL; msm.hip: msm_chunks<DUAL>, msm_g1_launch_tail_merged).
pi_c only uses C + H, so the merged tail adds H's buckets to C's bucket by bucket and reduces the sum once.  Every case proves with
the switch forced on and compares the proof with the closed form and with the proof the same key gives with the switch off --
under tail geometries forced small (at least two pieces per bucket set, the second chunk level off and on), on two queues and on
one, with buckets that are empty in one plan and not in the other, and on a key whose two plans have different windows, where the
merge must decline.  The same cases run on the CPU thread emulator and (-m gpu) on the device."""
import random

import pytest

import tail_patterns as tp
from wasmsnark_amd import synth

BACKENDS = ["emul", pytest.param("gpu", marks=pytest.mark.gpu)]
R32, S32 = bytes(range(9, 41)), bytes(range(60, 92))
TAIL = ("msm_chunks", "msm_chunks2", "msm_tree", "msm_rows")
# forced tail geometry per table window c: (MSM_CHUNK, TAIL_BITS, TAIL_L2 when the second chunk level is on)
SMALL = {6: (2, 4, None), 10: (2, 7, 4), 12: (4, 9, 2)}

_bns, _keys = {}, {}


def _bn(backend):
    if backend not in _bns:
        if backend == "emul":
            from emul_util import emul_bn128
            _bns[backend] = emul_bn128()
        else:
            import torch
            assert torch.cuda.is_available(), "GPU tests need a GPU"
            import __graft_entry__
            __graft_entry__.ensure_built()
            import wasmsnark_amd
            _bns[backend] = wasmsnark_amd.build(device=0)
            assert _bns[backend].lib.path.endswith("wasmsnark_amd/libwsnark.so")
    return _bns[backend]


@pytest.fixture(scope="module", autouse=True)
def _free_keys():
    yield
    for _, _, key, _ in _keys.values():
        key.free()
    _keys.clear()


def _native(backend, logd, style, table_c=None):
    """(circuit, witness, resident key, closed-form proof) of the library's generator, one per module"""
    k = (backend, logd, style, table_c)
    if k not in _keys:
        bn = _bn(backend)
        circ = synth.NativeCircuit(bn.lib, logd, n_public=3, seed=8, style=style)
        sec, _ = circ.build_sections()
        bn.lib.tune("TABLE_C", table_c)          # (the tables are built by the load)
        try:
            key = bn.load_key(sections=sec)
        finally:
            bn.lib.tune("TABLE_C", None)
        _keys[k] = (circ, circ.witness_bin(), key, circ.expected_proof(R32, S32))
    return _keys[k]


def _linear_circuit(log_domain, pad, seed):
    """Every row is (sum of earlier variables) * 1 = a fresh variable: B w is the constant polynomial 1 and A w - C w vanishes on the
    whole domain, so h = 0 -- every bucket of the H plan is EMPTY while C's are not.  `pad` unused variables behind the real ones
    (columns empty in A, B and C: their key points are infinity) move n_vars, and with it the window of the witness's tables."""
    rnd = random.Random(seed)
    domain = 1 << log_domain
    n_free = 4
    n_vars = 1 + n_free + domain + pad
    w = [1] + [rnd.randrange(1, synth.R) for _ in range(n_free)] + [0] * (domain + pad)
    A, B, Cm = ([dict() for _ in range(n_vars)] for _ in range(3))
    for c in range(domain):
        out = 1 + n_free + c
        tot = 0
        for s in rnd.sample(range(out), 2):
            A[s][c] = cf = rnd.randrange(1, synth.R)
            tot += cf * w[s]
        B[0][c] = 1
        Cm[out][c] = 1
        w[out] = tot % synth.R
    for i in range(1 + n_free + domain, n_vars):
        w[i] = rnd.randrange(1, synth.R)
    return synth.Circuit(n_vars, 2, domain, A, B, Cm, w)


def _python(backend, name):
    """keys of circuits written down here (wasmsnark_amd/synth.py: the Python generator and its closed form)"""
    k = (backend, name)
    if k not in _keys:
        bn = _bn(backend)
        if name == "h is zero":
            circ = _linear_circuit(6, 0, 31)
        elif name == "two windows":
            base = synth.make_circuit(6, n_public=2, seed=12, style="columns")
            pad = 30                                                       # 96 variables: window 7 for the witness, 6 for the 64 of h
            rnd = random.Random(5)
            circ = synth.Circuit(base.n_vars + pad, base.n_public, base.domain, base.A + [dict() for _ in range(pad)],
                                 base.B + [dict() for _ in range(pad)], base.C + [dict() for _ in range(pad)],
                                 base.witness + [rnd.randrange(1, synth.R) for _ in range(pad)])
        else:
            raise KeyError(name)
        S = synth.setup(circ, seed=9)
        pkey, _ = synth.build_key(circ, S, bn.mul_base)
        _keys[k] = (circ, synth.witness_bin(circ), bn.load_key(pkey), synth.expected_proof(circ, S, R32, S32, bn.mul_base))
    return _keys[k]


def _tail_launches(bn):
    return {k: v[1] for k, v in bn.lib.timing_report().items() if k in TAIL}


def _prove(bn, tune, wit, key, switch):
    tune(bn.lib, "PROVE_CH_TAIL", switch)
    with tp.Timing(bn.lib):
        proof = bn.groth16GenProof(wit, key, r=R32, s=S32)
        return proof, _tail_launches(bn)


def _check(bn, tune, wit, key, want, c, l2_on, overlap, merges=True):
    """off / on under one forced geometry.  On ONE queue the tails are a launch each (B2; A with B1; C; H), so the merge shows in the
    per-kernel launch counts; on the small arrangement's three queues C leaves the batched tail of A and B1 for H's: the count stays."""
    chunk, bits, l2 = SMALL[c]
    l2 = l2 if l2_on else 1
    geo = tp.tail_geometry(c, True, chunk, bits, l2)
    assert geo.tP >= 2 and (geo.m2 > 1) == bool(l2_on), geo
    tune(bn.lib, "MSM_CHUNK", chunk)
    tune(bn.lib, "TAIL_BITS", bits)
    tune(bn.lib, "TAIL_L2", l2)
    tune(bn.lib, "PROVE_OVERLAP", overlap)
    off, n_off = _prove(bn, tune, wit, key, 0)
    on, n_on = _prove(bn, tune, wit, key, 1)
    assert off == want, ("switch off", geo)
    assert on == want, ("switch on", geo)
    assert on == off
    assert set(n_on) == tp.expected_kernels(geo) == set(n_off), (n_on, n_off, geo)
    if overlap == 0:
        assert set(n_off.values()) == {4}, n_off
        assert set(n_on.values()) == ({3} if merges else {4}), n_on
    else:
        assert set(n_off.values()) == {3} and set(n_on.values()) == {3}, (n_off, n_on)


# (log2 constraints, style, second chunk level, PROVE_OVERLAP).  2^10: every style with both chunk levels on both schedules; 2^12
# (whose keys take the emulator most of a minute to make): one case per style, so that every value of the two switches is taken
CASES = [(10, style, l2_on, overlap) for style in ("columns", "rows", "boolean") for l2_on, overlap in ((False, None), (True, 0), (True, None), (False, 0))]
CASES += [(12, "columns", True, None), (12, "rows", False, 0), (12, "boolean", True, 0)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("logd,style,l2_on,overlap", CASES)
def test_merged_tail_proofs(backend, tune, logd, style, l2_on, overlap):
    bn = _bn(backend)
    circ, wit, key, want = _native(backend, logd, style)
    assert key.table["c_w"] == key.table["c_h"] == logd
    _check(bn, tune, wit, key, want, logd, l2_on, overlap)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("l2_on,overlap", [(False, 0), (True, None)])
def test_buckets_empty_in_c_only(backend, tune, l2_on, overlap):
    """boolean style, 2^10, tables of window 12: the ~127 witness values that are not 0 / 1 put ~2800 entries into C's 2048 buckets
    (about a quarter stay empty: e^-1.4), h puts 22 x 1024 into H's (11 per bucket)"""
    bn = _bn(backend)
    circ, wit, key, want = _native(backend, 10, "boolean", table_c=12)
    assert key.table["c_w"] == key.table["c_h"] == 12
    _check(bn, tune, wit, key, want, 12, l2_on, overlap)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("overlap", [0, None])
def test_buckets_empty_in_h_only(backend, tune, overlap):
    """h = 0: the H plan has pairs and no entry at all, C's buckets are full"""
    bn = _bn(backend)
    circ, wit, key, want = _python(backend, "h is zero")
    assert key.table["c_w"] == key.table["c_h"] == 6
    _check(bn, tune, wit, key, want, 6, False, overlap)


@pytest.mark.parametrize("backend", BACKENDS)
def test_two_windows_decline(backend, tune):
    """96 variables against a domain of 64: the witness's tables have window 7, h's window 6 -- two tail geometries, two tails"""
    bn = _bn(backend)
    circ, wit, key, want = _python(backend, "two windows")
    assert (key.table["c_w"], key.table["c_h"]) == (7, 6)
    tune(bn.lib, "PROVE_OVERLAP", 0)
    for switch in (0, 1, None):
        proof, n = _prove(bn, tune, wit, key, switch)
        assert proof == want, switch
        assert n["msm_chunks"] == 4 and n["msm_tree"] == 4, (switch, n)
    tune(bn.lib, "PROVE_OVERLAP", None)
    proof, n = _prove(bn, tune, wit, key, 1)
    assert proof == want and n["msm_chunks"] == 3, n
