"""Shared checks of the batch witness check (wsnark_circuit_witness_check_batch[_dev], csrc/witcheck.hip: lc_check_batch_kernel,
witness_facts_batch_kernel, mask_gather_batch_kernel, lc_row_values_batch_kernel) and of groth16GenProofBatch(..., circuit=rc), run
by tests/test_emul_witness_check_batch.py on the thread-emulator build of the kernel sources and by
tests/test_gpu_witness_check_batch.py on the device.

Two yardsticks, neither of them the code under test: witness_check_common.py's py_check (Python integers over the circuit's rows) and
the single resident call (wsnark_circuit_witness_check) on the SAME handle with the same cap: verdict i and witness i's lists are
field for field what it reports for witness i.

Good witnesses of one circuit: new free values, then synth.make_circuit's rows evaluated in order -- the output of row c is
w[1 + N_FREE + c] -- and py_check agrees that each is good.  Witness i of a batch then breaks its OWN row (7 i + 3) mod n_cons, so that
a mask or an accumulator read at another witness's offset shows."""
import ctypes as C
import random
import subprocess
import sys
import threading

import pkey_delta_common as pd
import witness_check_common as wc
from bn128_ref import R
from pkey_check_common import ERR_ARG, ERR_NOINIT, ERR_SIZE
from wasmsnark_amd import synth
from wasmsnark_amd.bn128 import _WitnessBatchReport, _WitnessVerdict

NONE, N_PUBLIC, N_FREE, TOP = wc.NONE, wc.N_PUBLIC, wc.N_FREE, wc.TOP
FIELDS = ("bad", "first_bad", "unreduced", "first_unreduced", "listed", "one_ok", "ok")
FILL = 0x5A


class chunked:
    """WITCHECK_BATCH_CHUNK for the duration of a block (None: the default)"""

    def __init__(self, bn, chunk):
        self.bn, self.chunk = bn, chunk

    def __enter__(self):
        self.bn.lib.tune("WITCHECK_BATCH_CHUNK", self.chunk)

    def __exit__(self, *exc):
        self.bn.lib.tune("WITCHECK_BATCH_CHUNK", None)


# ---- witnesses ----
_memo = {}


def good_witness(log_domain, style, k):
    """the k-th good witness of synth_case(log_domain, style): k = 0 is the circuit's own, the others have new free values"""
    key = ("good", log_domain, style, k)
    if key not in _memo:
        circ, blobs, rows3 = wc.synth_case(log_domain, style)
        if k == 0:
            w = list(circ.witness)
        else:
            rnd = random.Random(1000 * log_domain + k)
            w = [0] * circ.n_vars
            w[0] = 1
            for i in range(1, 1 + N_FREE):
                w[i] = rnd.randrange(1, R)
            dot = lambda row: sum(c * w[j] for j, c in row) % R
            for c in range(circ.domain - N_PUBLIC - 1):
                w[1 + N_FREE + c] = dot(rows3[0][c]) * dot(rows3[1][c]) % R
            assert w != list(circ.witness)
        want = wc.py_check(rows3, w, N_PUBLIC)
        assert want["ok"] == 1 and want["bad"] == 0, (log_domain, style, k)
        _memo[key] = w
    return list(_memo[key])


def batch_case(log_domain, style, count, good=None):
    """count witnesses: witness i is good_witness(i) with the output of its own row (7 i + 3) mod n_cons changed, except witness 0,
    the last one and one in the middle (or the set `good`), which stay good.  -> ([witness], [py_check of it])"""
    key = ("batch", log_domain, style, count, None if good is None else tuple(sorted(good)))
    if key not in _memo:
        circ, blobs, rows3 = wc.synth_case(log_domain, style)
        n_cons = circ.domain - N_PUBLIC - 1
        keep = {0, count // 2, count - 1} if good is None else set(good)
        wits, wants = [], []
        for i in range(count):
            w = good_witness(log_domain, style, i % 7)      # (seven distinct good witnesses are plenty: the planted row differs)
            if i not in keep:
                row = (7 * i + 3) % n_cons
                w[1 + N_FREE + row] = (w[1 + N_FREE + row] + 1) % R
            want = wc.py_check(rows3, w, N_PUBLIC)
            if i in keep:
                assert want["ok"] == 1
            else:
                assert want["bad"] >= 1 and (7 * i + 3) % n_cons in want["bad_rows"] and want["ok"] == 0
            wits.append(w)
            wants.append(want)
        _memo[key] = (wits, wants)
    return _memo[key]


# ---- comparing ----
def assert_verdict(got, want, single, cap, where):
    """one witness's dict against py_check's and against the single resident call's report (same cap)"""
    listed = min(want["bad"], cap)
    for name in FIELDS:
        expect = listed if name == "listed" else want[name]
        assert got[name] == expect, (where, name, got[name], expect)
        if single is not None:
            assert got[name] == single[name], (where, "single", name, got[name], single[name])
    assert got["bad_rows"] == want["bad_rows"][:listed] and got["bad_values"] == want["bad_values"][:listed], (where, got["bad_rows"])
    if single is not None:
        assert got["bad_rows"] == single["bad_rows"] and got["bad_values"] == single["bad_values"], (where, "single lists")
    assert "rows" not in got and "ms" not in got


def assert_batch(rc, wits, wants, cap, got, rep, where, singles=True):
    assert len(got) == len(wits), where
    for i, (w, want) in enumerate(zip(wits, wants)):
        single = rc.check_witness(wc.wbytes(w), max_rows=cap) if singles else None
        assert_verdict(got[i], want, single, cap, (where, i))
    not_ok = [i for i, want in enumerate(wants) if not want["ok"]]
    assert rep["count"] == len(wits) and rep["rows"] == rc.domain and rep["good"] == len(wits) - len(not_ok), (where, rep)
    assert rep["first_not_ok"] == (not_ok[0] if not_ok else NONE) and 1 <= rep["chunk"] <= len(wits), (where, rep)
    assert set(rep["ms"]) == {"matrices", "device", "total"} and rep["ms"]["matrices"] == 0 and rep["ms"]["total"] >= rep["ms"]["device"] > 0, rep


def c_batch(bn, h, blob, stride, count, cap, dev=False, stream=None, verdicts=True, lists=True, null_rep=False, room=None):
    """the C call on buffers pre-filled with 0x5A: (code, verdict bytes, rows, values, report) as left behind; room: witnesses the
    buffers have room for when that is not `count` (calls that must be refused before anything is written)"""
    n = max(count if room is None else room, 1)
    ver = (C.c_uint8 * (48 * n))(*([FILL] * (48 * n)))
    rows = (C.c_uint64 * (n * max(cap, 1)))(*([int.from_bytes(bytes([FILL]) * 8, "little")] * (n * max(cap, 1))))
    vals = (C.c_uint8 * (96 * n * max(cap, 1)))(*([FILL] * (96 * n * max(cap, 1))))
    rep = pd._raw(_WitnessBatchReport)
    args = [h, blob, stride, count, ver if verdicts else None, rows if lists else None, vals if lists else None, cap, None if null_rep else C.byref(rep)]
    c = bn.lib.c
    code = c.wsnark_circuit_witness_check_batch_dev(*args, stream) if dev else c.wsnark_circuit_witness_check_batch(*args)
    return code, bytes(ver), list(rows), bytes(vals), rep


# ---- 1. equals the single call and Python ----
def check_equals_single(bn, log_domain, style, count):
    circ, blobs, rows3 = wc.synth_case(log_domain, style)
    wits, wants = batch_case(log_domain, style, count)
    rc = bn.load_circuit(blobs)
    try:
        for cap in (0, 1, circ.domain):
            rep = {}
            got = rc.check_witnesses([wc.wbytes(w) for w in wits], max_rows=cap, report=rep)
            assert_batch(rc, wits, wants, cap, got, rep, (log_domain, style, count, cap), singles=(count <= 5 or cap == 1))
            if count == 1:      # a batch of one BAD witness (the library hands a batch of one to the single call)
                two, want2 = batch_case(log_domain, style, 2, good={0})
                rep = {}
                got = rc.check_witnesses(wc.wbytes(two[1]), max_rows=cap, report=rep)
                assert_batch(rc, two[1:], want2[1:], cap, got, rep, (log_domain, style, "one bad", cap))
    finally:
        rc.free()


# ---- 2. geometry: the pass size changes nothing ----
def check_geometry(bn, log_domain):
    circ, blobs, rows3 = wc.synth_case(log_domain)
    wits, wants = batch_case(log_domain, "columns", 5, good={0, 3, 4})      # bad: 1 | 2 on the two sides of chunk 2's first boundary
    blob = b"".join(wc.wbytes(w) for w in wits)
    rc = bn.load_circuit(blobs)
    try:
        results = []
        for chunk, ran in ((1, 1), (2, 2), (None, 5), (3, 3), (64, 5)):
            rep = {}
            with chunked(bn, chunk):
                got = rc.check_witnesses(blob, max_rows=circ.domain, report=rep)
            assert rep["chunk"] == ran, (chunk, rep)
            assert_batch(rc, wits, wants, circ.domain, got, rep, ("chunk", chunk), singles=(chunk is None))
            results.append(got)
        assert all(r == results[0] for r in results)
    finally:
        rc.free()


# ---- 3. stride ----
def check_stride(bn, log_domain=6):
    circ, blobs, rows3 = wc.synth_case(log_domain)
    wits, wants = batch_case(log_domain, "columns", 5)
    nv, cap = circ.n_vars, 4
    packed = [wc.wbytes(w) for w in wits]
    rc = bn.load_circuit(blobs)
    try:
        rep_blob, rep_seq, rep_long = {}, {}, {}
        from_blob = rc.check_witnesses(b"".join(packed), max_rows=cap, report=rep_blob)
        from_seq = rc.check_witnesses(packed, max_rows=cap, report=rep_seq)
        from_long = rc.check_witnesses([w + b"\xff" * 64 for w in packed], max_rows=cap, report=rep_long)      # only nVars signals are read
        assert from_blob == from_seq == from_long
        assert_batch(rc, wits, wants, cap, from_blob, rep_blob, "blob")
        # the C call with the witnesses nVars x 32 + 64 bytes apart and 0xFF between them, under every pass size
        stride = 32 * nv + 64
        strided = b"".join(w + b"\xff" * 64 for w in packed)
        for chunk in (None, 2):
            with chunked(bn, chunk):
                code, ver, rows, vals, rep = c_batch(bn, rc._h, strided, stride, 5, cap)
            assert code == 0 and rep.count == 5 and rep.chunk == (5 if chunk is None else 2)
            for i, got in enumerate(from_blob):
                v = _WitnessVerdict.from_buffer_copy(ver[48 * i:48 * i + 48])
                assert tuple(getattr(v, f) for f in FIELDS) == tuple(got[f] for f in FIELDS), (chunk, i)
                assert rows[i * cap:i * cap + got["listed"]] == got["bad_rows"], (chunk, i)
    finally:
        rc.free()


# ---- 4. the hand-built circuit between two all-zero witnesses: truncation, list offsets, entries beyond `listed` ----
def check_hand_built(bn, log_domain=6):
    circuit, rows3, w = wc.hand_case(log_domain)
    domain, nv = circuit["domain"], circuit["n_vars"]
    zero = [0] * nv
    wits = [zero, w, zero]
    wants = [wc.py_check(rows3, x, N_PUBLIC) for x in wits]
    assert wants[0]["one_ok"] == 0 and wants[0]["ok"] == 0 and wants[0]["bad"] == 0 and wants[2] == wants[0]
    assert wants[1]["bad"] > domain // 2 and 8 in wants[1]["bad_rows"] and wants[1]["unreduced"] == 2 and wants[1]["one_ok"] == 1
    blob = b"".join(wc.wbytes(x) for x in wits)
    rc = bn.load_circuit(circuit)
    try:
        for cap in (0, 1, 5, domain):
            for chunk in (None, 1):
                rep = {}
                with chunked(bn, chunk):
                    got = rc.check_witnesses(blob, max_rows=cap, report=rep)
                assert_batch(rc, wits, wants, cap, got, rep, ("hand", cap, chunk), singles=(chunk is None))
                assert rep["good"] == 0 and rep["first_not_ok"] == 0
            if cap == 0:
                continue
            # the lists as the C call leaves them: witness 1's entries start at cap, everything else is as it was
            code, ver, rows, vals, rep = c_batch(bn, rc._h, blob, 32 * nv, 3, cap)
            listed = min(wants[1]["bad"], cap)
            fill64 = int.from_bytes(bytes([FILL]) * 8, "little")
            assert code == 0 and rows[cap:cap + listed] == wants[1]["bad_rows"][:listed]
            assert set(rows[:cap]) == {fill64} and set(rows[2 * cap:]) == {fill64} and set(rows[cap + listed:2 * cap]) <= {fill64}
            val = lambda k: int.from_bytes(vals[32 * k:32 * k + 32], "little")
            assert [(val(3 * (cap + j)), val(3 * (cap + j) + 1), val(3 * (cap + j) + 2)) for j in range(listed)] == wants[1]["bad_values"][:listed]
            assert set(vals[:96 * cap]) == {FILL} and set(vals[96 * 2 * cap:]) == {FILL} and set(vals[96 * (cap + listed):96 * 2 * cap]) <= {FILL}
    finally:
        rc.free()


# ---- 5. unreduced signals and w[0] != 1, per witness ----
def check_unreduced(bn, log_domain=6):
    circ, blobs, rows3 = wc.synth_case(log_domain)
    nv = circ.n_vars
    private = [N_PUBLIC + 1, N_PUBLIC + 2, nv // 2, nv - 1]
    w = list(circ.witness)
    for k, v in enumerate(private):      # w + r, and the largest multiple that still fits 256 bits
        w[v] += (TOP - w[v]) // R * R if k == 2 else R
        assert R <= w[v] <= TOP
    w2 = list(w)
    w2[nv - 1] = TOP       # reduces to another value: the last row is bad
    w3 = list(circ.witness)
    w3[1] += R
    w4 = list(circ.witness)
    w4[0] = 2
    wits = [w, w2, w3, w4]
    fixed = [dict(bad=0, ok=1, unreduced=len(private), first_unreduced=N_PUBLIC + 1),
             dict(ok=0, unreduced=len(private), first_bad=circ.domain - N_PUBLIC - 2),
             dict(bad=0, ok=0, unreduced=1, first_unreduced=1), dict(one_ok=0, ok=0, unreduced=0)]
    wants = [wc.py_check(rows3, x, N_PUBLIC) for x in wits]
    for want, fx in zip(wants, fixed):
        assert all(want[k] == x for k, x in fx.items()), (want, fx)
    rc = bn.load_circuit(blobs)
    try:
        for chunk in (None, 1, 3):
            rep = {}
            with chunked(bn, chunk):
                got = rc.check_witnesses([wc.wbytes(x) for x in wits], max_rows=circ.domain, report=rep)
            assert_batch(rc, wits, wants, circ.domain, got, rep, ("unreduced", chunk), singles=(chunk is None))
            assert rep["good"] == 1 and rep["first_not_ok"] == 1
    finally:
        rc.free()


# ---- 6. errors leave everything untouched ----
def check_errors(bn, so_path, log_domain=4):
    circ, blobs, rows3 = wc.synth_case(log_domain)
    nv = circ.n_vars
    wit = wc.wbytes(circ.witness) * 2
    untouched = bytes(pd._raw(_WitnessBatchReport))
    rc = bn.load_circuit(blobs)

    def call(h=rc._h, w=wit, stride=32 * nv, count=2, cap=4, dev=False, **kw):
        code, ver, rows, vals, rep = c_batch(bn, h, w, stride, count, cap, dev=dev, **kw)
        assert set(ver) == {FILL} and set(vals) == {FILL} and all(x == int.from_bytes(bytes([FILL]) * 8, "little") for x in rows), code
        assert bytes(rep) == untouched, code
        return code

    try:
        for dev in (False, True):
            assert call(h=None, dev=dev) == ERR_ARG and call(w=None, dev=dev) == ERR_ARG and call(verdicts=False, dev=dev) == ERR_ARG
            assert call(lists=False, dev=dev) == ERR_ARG and call(lists=False, cap=1, dev=dev) == ERR_ARG      # cap > 0 without lists
            assert call(stride=32 * nv - 1, dev=dev) == ERR_SIZE and call(stride=0, dev=dev) == ERR_SIZE
            assert call(count=(1 << 16) + 1, room=2, dev=dev) == ERR_SIZE
            assert call(count=0, dev=dev) == 0 and call(count=0, w=None, verdicts=False, lists=False, dev=dev) == 0      # touches nothing
        # a device batch that is not 16-byte aligned (pointer or stride) is refused before anything reads it
        aligned = (C.c_uint8 * (len(wit) + 64))()
        base = (C.addressof(aligned) + 15) & ~15
        assert call(w=C.c_void_p(base + 8), dev=True) == ERR_ARG and call(w=C.c_void_p(base + 1), dev=True) == ERR_ARG
        assert call(w=C.c_void_p(base), stride=32 * nv + 8, dev=True) == ERR_ARG
        # cap == 0: both lists may be NULL; the report may be NULL
        code, ver, rows, vals, rep = c_batch(bn, rc._h, wit, 32 * nv, 2, 0, lists=False)
        assert code == 0 and rep.good == 2 and rep.first_not_ok == NONE and all(_WitnessVerdict.from_buffer_copy(ver[48 * i:48 * i + 48]).ok == 1 for i in range(2))
        code, ver, rows, vals, rep = c_batch(bn, rc._h, wit, 32 * nv, 2, 4, null_rep=True)
        assert code == 0 and _WitnessVerdict.from_buffer_copy(ver[48:96]).ok == 1 and bytes(rep) == untouched
        assert rc.check_witnesses([]) == [] and rc.check_witnesses(b"") == []
        for bad_input in (wit[:-1], [wit[:32 * nv - 1]]):
            try:
                rc.check_witnesses(bad_input)
            except ValueError:
                pass
            else:
                raise AssertionError("a short witness was accepted")
    finally:
        rc.free()
    # before wsnark_init: a fresh process that loads the library and never initialises it
    code = ("import ctypes as C, sys\n"
            "c = C.CDLL(sys.argv[1])\n"
            "vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64\n"
            "c.wsnark_circuit_witness_check_batch.argtypes = [vp, vp, sz, u64, vp, vp, vp, u64, vp]\n"
            "c.wsnark_circuit_witness_check_batch_dev.argtypes = [vp, vp, sz, u64, vp, vp, vp, u64, vp, vp]\n"
            "v = (C.c_uint8 * 768)(*([90] * 768))\n"
            "print(c.wsnark_circuit_witness_check_batch(v, v, 32, 2, v, v, v, 1, v),\n"
            "      c.wsnark_circuit_witness_check_batch_dev(v, v, 32, 2, v, v, v, 1, v, None),\n"
            "      c.wsnark_circuit_witness_check_batch(None, v, 32, 0, v, v, v, 1, v), set(v))\n")
    res = subprocess.run([sys.executable, "-c", code, so_path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == [str(ERR_NOINIT)] * 3 + ["{90}"], (res.stdout, res.stderr)


# ---- 7. two threads, one handle, two different batches ----
def check_two_threads(bn, log_domain=6, repeats=4):
    circ, blobs, rows3 = wc.synth_case(log_domain)
    jobs = [batch_case(log_domain, "columns", 5), batch_case(log_domain, "columns", 3, good={1})]
    rc = bn.load_circuit(blobs)
    got, errors = [[], []], []

    def work(k):
        try:
            for _ in range(repeats):
                rep = {}
                got[k].append((rc.check_witnesses([wc.wbytes(w) for w in jobs[k][0]], max_rows=circ.domain, report=rep), rep))
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    try:
        assert not errors, errors
        for k in range(2):
            assert len(got[k]) == repeats
            for res, rep in got[k]:
                assert_batch(rc, jobs[k][0], jobs[k][1], circ.domain, res, rep, ("thread", k), singles=False)
        assert_batch(rc, jobs[1][0], jobs[1][1], circ.domain, got[1][0][0], got[1][0][1], "thread 1 against the single call")
    finally:
        rc.free()


# ---- 8. the witnesses already on the device (device only) ----
def check_dev_variant(bn, log_domain):
    import torch
    circ, blobs, rows3 = wc.synth_case(log_domain)
    wits, wants = batch_case(log_domain, "columns", 5)
    nv, cap = circ.n_vars, circ.domain
    rc = bn.load_circuit(blobs)
    try:
        host = rc.check_witnesses([wc.wbytes(w) for w in wits], max_rows=cap)
        for pad in (0, 48):      # packed, and a stride larger than nVars x 32: the bytes between two witnesses are never read
            stride = 32 * nv + pad
            src = torch.frombuffer(bytearray(b"".join(wc.wbytes(w) + b"\xff" * pad for w in wits)), dtype=torch.uint8)
            d_w = src.cuda()
            torch.cuda.synchronize()
            for chunk in (None, 2):
                rep = {}
                with chunked(bn, chunk):
                    got = rc.check_witnesses_dev(d_w.data_ptr(), stride, 5, max_rows=cap, report=rep)
                assert got == host and rep["chunk"] == (5 if chunk is None else 2), (pad, chunk)
                assert_batch(rc, wits, wants, cap, got, rep, ("device, the lane's queue", pad, chunk), singles=False)
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                d_w2 = src.to("cuda", non_blocking=True)
                rep = {}
                got = rc.check_witnesses_dev(d_w2.data_ptr(), stride, 5, max_rows=cap, report=rep, stream=st.cuda_stream)
            assert got == host
            assert_batch(rc, wits, wants, cap, got, rep, ("device, a torch stream", pad), singles=(pad == 0))
    finally:
        rc.free()


# ---- 9. groth16GenProofBatch(..., circuit=rc) ----
class routed:
    """the batch prover's routing switches for the duration of a block"""

    def __init__(self, bn, **kw):
        self.bn, self.kw = bn, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.bn.lib.tune(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.bn.lib.tune(k, None)


def check_gen_proof_batch(bn, log_domain=6, dev=False):
    circ, blobs, rows3 = wc.synth_case(log_domain)
    pkey, vk = synth.build_key(circ, synth.setup(circ, seed=11), bn.mul_base)
    key = bn.load_key(pkey)
    rc = bn.load_circuit(blobs)
    other = bn.load_circuit(wc.synth_case(log_domain + 1)[1])
    wits, wants = batch_case(log_domain, "columns", 5, good={0, 2, 3})      # the second and the last are bad
    good = [0, 2, 3]
    packed = [wc.wbytes(w) for w in wits]
    rnd = random.Random(9)
    rs = [bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(5)]
    ss = [bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(5)]
    stride = 32 * circ.n_vars

    def prove(which, **kw):
        r, s = [rs[i] for i in which], [ss[i] for i in which]
        if not dev:
            return bn.groth16GenProofBatch([packed[i] for i in which], key, r=r, s=s, **kw)
        import torch
        d_w = torch.frombuffer(bytearray(b"".join(packed[i] for i in which)), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        return bn.groth16GenProofBatch_dev(d_w.data_ptr(), stride, len(which), key, r=r, s=s, **kw)

    try:
        for sw, batched in (({"BATCH_MIN": 1, "BATCH_MAX_DOMAIN": 1 << 16}, True), ({"BATCH_MIN": 1 << 20}, False)):      # the batch kernels; the loop route
            with routed(bn, **sw):
                plain = prove(good)
                rep = {}
                proofs, used = prove(range(5), circuit=rc, return_blinding=True, report=rep)
                assert [proofs[i] for i in good] == plain and proofs[1] is None and proofs[4] is None, batched
                assert used == [(rs[i], ss[i]) if i in good else None for i in range(5)]
                assert rep["count"] == 3 and rep["batched"] == (3 if batched else 0), rep
                for i, want in enumerate(wants):
                    assert_verdict(rep["verdicts"][i], want, rc.check_witness(packed[i], max_rows=1), 1, ("guard", i))
                # all bad: nothing is proved
                r1 = {}
                assert prove([1, 4], circuit=rc, report=r1) == [None, None] and r1["count"] == 0 and [v["ok"] for v in r1["verdicts"]] == [0, 0]
                if not batched:
                    continue
                # without circuit= nothing changes: the bad witnesses still prove
                assert all(p is not None for p in prove([1, 4]))
                if not dev:      # blinding drawn by the library: one pair per good witness, none for a bad one
                    drawn, pairs = bn.groth16GenProofBatch(packed, key, circuit=rc, return_blinding=True)
                    assert [p is None for p in pairs] == [False, True, False, False, True] and len({p for p in pairs if p}) == 3
                    assert [d is None for d in drawn] == [p is None for p in pairs]
                    assert bn.groth16Verify(vk, _public(wits[3]), drawn[3])
            for i, p in zip(good, plain):      # each good witness has public inputs of its own
                assert bn.groth16Verify(vk, _public(wits[i]), p)
        for kw in ({}, {"report": {}}):
            try:
                prove(range(5), circuit=other, **kw)
            except ValueError as e:
                assert "is not the key's" in str(e), e
            else:
                raise AssertionError("a circuit of another shape was accepted")
    finally:
        for h in (rc, other, key):
            h.free()


def _public(w):
    return [str(v) for v in w[1:1 + N_PUBLIC]]
