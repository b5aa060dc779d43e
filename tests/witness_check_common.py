"""Shared checks of the witness check (wsnark_witness_check, wsnark_circuit_load / _witness_check / _witness_check_dev,
csrc/witcheck.hip), run by tests/test_emul_witness_check.py on the thread-emulator build of the kernel sources and by
tests/test_gpu_witness_check.py on the device.

The yardstick is Python integers, never the library: the circuit's columns are transposed to rows and (sum A)(sum B) - sum C mod r is
evaluated per row.  Good witnesses are synth.make_circuit's own; bad ones change one signal of a good one, or are
pkey_circuit_common.weights_for over its hand-built circuit (a 300-term row, zero coefficients, repeated records, an empty last row),
where nearly every row is bad.  Every check runs on the one-shot call and on a resident circuit."""
import ctypes as C
import subprocess
import sys
import threading

import pkey_circuit_common as pc
import pkey_delta_common as pd
import pkey_setup_common as ps
from bn128_ref import R, le
from pkey_check_common import ERR_ARG, ERR_FORMAT, ERR_NOINIT, ERR_SIZE
from wasmsnark_amd import synth

NONE = (1 << 64) - 1
TOP = (1 << 256) - 1
N_PUBLIC = 2
N_FREE = N_PUBLIC + 2       # synth.make_circuit: the output variable of row c is 1 + N_FREE + c


# ---- the yardstick ----
def columns_to_rows(cols, domain):
    rows = [[] for _ in range(domain)]
    for j, col in enumerate(cols):
        for i, coef in col.items():
            rows[i].append((j, coef))
    return rows


def py_check(rows3, w, n_public):
    """what the report and the full lists must say for witness w (any 256-bit values) over rows3 = rows of A, B, C"""
    wr = [v % R for v in w]
    dot = lambda row: sum(c * wr[j] for j, c in row) % R
    abc = [(dot(a), dot(b), dot(c)) for a, b, c in zip(*rows3)]
    bad = [i for i, (a, b, c) in enumerate(abc) if (a * b - c) % R]
    big = [j for j, v in enumerate(w) if v >= R]
    return {"rows": len(abc), "bad": len(bad), "first_bad": bad[0] if bad else NONE, "unreduced": len(big),
            "first_unreduced": big[0] if big else NONE, "one_ok": int(w[0] == 1),
            "ok": int(not bad and w[0] == 1 and not any(j <= n_public for j in big)),
            "bad_rows": bad, "bad_values": [abc[i] for i in bad]}


def wbytes(w):
    return b"".join(le(v) for v in w)


_memo = {}


def synth_case(log_domain, style="columns"):
    """(circuit, its blobs, its rows) of synth.make_circuit, made once; Python agrees that its witness is good"""
    key = (log_domain, style)
    if key not in _memo:
        circ = synth.make_circuit(log_domain, n_public=N_PUBLIC, seed=3, style=style)
        rows3 = [columns_to_rows(m, circ.domain) for m in (circ.A, circ.B, circ.C)]
        assert py_check(rows3, circ.witness, N_PUBLIC)["bad"] == 0
        _memo[key] = (circ, synth.circuit_blobs(circ), rows3)
    return _memo[key]


def hand_case(log_domain, n_vars=40):
    key = ("hand", log_domain)
    if key not in _memo:
        rows3 = pc.hand_circuit(log_domain, n_vars)
        blobs = [pc.rows_to_blob(M, n_vars) for M in rows3]
        circuit = {"n_vars": n_vars, "n_public": N_PUBLIC, "domain": 1 << log_domain, "polsA": blobs[0], "polsB": blobs[1], "polsC": blobs[2]}
        _memo[key] = (circuit, rows3, pc.weights_for(n_vars))
    return _memo[key]


class both_calls:
    """the one-shot call and the resident one as [(name, fn(witness bytes, max_rows) -> report)]; the handle is freed on exit"""

    def __init__(self, bn, blobs):
        self.bn, self.blobs = bn, blobs

    def __enter__(self):
        self.rc = self.bn.load_circuit(self.blobs)
        return [("one-shot", lambda w, cap: self.bn.check_witness(self.blobs, w, max_rows=cap)),
                ("resident", lambda w, cap: self.rc.check_witness(w, max_rows=cap))]

    def __exit__(self, *exc):
        self.rc.free()


def assert_report(got, want, cap, where):
    """every field of the report and both lists against py_check's, for a list of at most `cap` rows"""
    for name in ("rows", "bad", "first_bad", "unreduced", "first_unreduced", "one_ok", "ok"):
        assert got[name] == want[name], (where, name, got[name], want[name])
    listed = min(want["bad"], cap)
    assert got["listed"] == listed and got["bad_rows"] == want["bad_rows"][:listed], (where, got["bad_rows"], want["bad_rows"][:listed])
    assert got["bad_values"] == want["bad_values"][:listed], where
    assert set(got["ms"]) == {"matrices", "device", "total"} and got["ms"]["total"] >= got["ms"]["device"] > 0, (where, got["ms"])


# ---- 1. good witnesses pass ----
def check_good(bn, log_domain, style):
    circ, blobs, rows3 = synth_case(log_domain, style)
    want = py_check(rows3, circ.witness, N_PUBLIC)
    assert want["ok"] == 1 and want["first_bad"] == NONE and want["unreduced"] == 0
    with both_calls(bn, blobs) as calls:
        for name, call in calls:
            got = call(wbytes(circ.witness), 16)
            assert_report(got, want, 16, name)
            assert (got["ok"], got["bad"], got["first_bad"], got["listed"], got["one_ok"], got["unreduced"]) == (1, 0, NONE, 0, 1, 0)
            assert got["rows"] == circ.domain and got["bad_rows"] == [] and got["bad_values"] == []
            assert (got["ms"]["matrices"] > 0) == (name == "one-shot")
        rc = bn.load_circuit(blobs)
        inf = rc.info()
        nnz = tuple(sum(len(col) for col in m) for m in (circ.A, circ.B, circ.C))
        assert (inf["n_vars"], inf["n_public"], inf["domain"], inf["nnz"]) == (circ.n_vars, N_PUBLIC, circ.domain, nnz), inf
        assert (rc.n_vars, rc.n_public, rc.domain) == (circ.n_vars, N_PUBLIC, circ.domain)
        assert inf["bytes"] >= 36 * sum(nnz) + 3 * 4 * (circ.domain + 1)      # col + coef per record, row_ptr per matrix
        rc.free()
        rc.free()      # twice is harmless


# ---- 2. planted failures give exactly the Python set ----
def planted_signals(log_domain):
    """output variables of row 0, 63, 64 and the last real row where the circuit has them, and at 2^10 one row per workgroup"""
    n_cons = (1 << log_domain) - N_PUBLIC - 1
    rows = {0, n_cons - 1} | {c for c in (63, 64) if c < n_cons}
    if log_domain >= 10:
        rows |= {100, 300, 600, 900}
    return [1 + N_FREE + c for c in sorted(rows)]


def check_planted(bn, log_domain):
    circ, blobs, rows3 = synth_case(log_domain)
    with both_calls(bn, blobs) as calls:
        for v in planted_signals(log_domain):
            w = list(circ.witness)
            w[v] = (w[v] + 1) % R
            want = py_check(rows3, w, N_PUBLIC)
            assert want["bad"] >= 1 and (v - 1 - N_FREE) in want["bad_rows"], v      # its own row at least
            for name, call in calls:
                assert_report(call(wbytes(w), want["bad"] + 3), want, want["bad"] + 3, (name, v))
        # several at once: the count is a sum over wavefronts, the first index a minimum
        w = list(circ.witness)
        for v in planted_signals(log_domain):
            w[v] = (w[v] + 1) % R
        want = py_check(rows3, w, N_PUBLIC)
        assert want["bad"] >= len(planted_signals(log_domain))
        for name, call in calls:
            assert_report(call(wbytes(w), circ.domain), want, circ.domain, (name, "all"))


# ---- 3. truncation, and every row's verdict on the hand-built circuit ----
def check_truncation(bn, log_domain=6):
    circuit, rows3, w = hand_case(log_domain)
    domain = circuit["domain"]
    want = py_check(rows3, w, N_PUBLIC)
    assert want["bad"] > domain // 2 and 8 in want["bad_rows"] and len(rows3[0][8]) == 300      # nearly every row, the long one included
    assert want["unreduced"] == 2 and want["first_unreduced"] == 2 and want["one_ok"] == 1      # weights_for plants 2^256 - 1 twice
    with both_calls(bn, circuit) as calls:
        for name, call in calls:
            for cap in (0, 1, 5, domain):
                got = call(wbytes(w), cap)
                assert_report(got, want, cap, (name, cap))
                assert got["listed"] == min(want["bad"], cap)
            verdicts = [i in set(got["bad_rows"]) for i in range(domain)]      # cap = domain: every row's verdict
            assert verdicts == [i in set(want["bad_rows"]) for i in range(domain)], name


# ---- 4. unreduced signals ----
def check_unreduced(bn, log_domain=6):
    circ, blobs, rows3 = synth_case(log_domain)
    nv = circ.n_vars
    private = [N_PUBLIC + 1, N_PUBLIC + 2, nv // 2, nv - 1]
    cases = []
    w = list(circ.witness)
    for k, v in enumerate(private):      # w + r, and the largest multiple that still fits 256 bits
        w[v] += (TOP - w[v]) // R * R if k == 2 else R
        assert R <= w[v] <= TOP
    cases.append(("private + r", w, dict(bad=0, ok=1, unreduced=len(private), first_unreduced=N_PUBLIC + 1)))
    w2 = list(w)
    w2[nv - 1] = TOP       # reduces to another value: the last row is bad, as Python's reduction says
    cases.append(("2^256 - 1", w2, dict(ok=0, unreduced=len(private), first_bad=circ.domain - N_PUBLIC - 2)))
    w3 = list(circ.witness)
    w3[1] += R
    cases.append(("public + r", w3, dict(bad=0, ok=0, unreduced=1, first_unreduced=1)))
    w4 = list(circ.witness)
    w4[0] = 2
    cases.append(("w[0] = 2", w4, dict(one_ok=0, ok=0, unreduced=0)))
    with both_calls(bn, blobs) as calls:
        for what, wit, fixed in cases:
            want = py_check(rows3, wit, N_PUBLIC)
            assert all(want[k] == x for k, x in fixed.items()), (what, want)
            for name, call in calls:
                assert_report(call(wbytes(wit), circ.domain), want, circ.domain, (name, what))


# ---- 5. a longer witness buffer ----
def check_longer_buffer(bn, log_domain=4):
    circ, blobs, rows3 = synth_case(log_domain)
    w = list(circ.witness)
    w[circ.n_vars - 1] = (w[circ.n_vars - 1] + 1) % R
    with both_calls(bn, blobs) as calls:
        for wit in (circ.witness, w):
            want = py_check(rows3, wit, N_PUBLIC)
            for name, call in calls:
                assert_report(call(wbytes(wit) + b"\xff" * 64, 4), want, 4, name)


# ---- 6. errors leave the report and the lists untouched ----
def check_errors(bn, so_path, log_domain=4):
    from wasmsnark_amd.bn128 import _WitnessReport, _circuit_struct
    circ, blobs, rows3 = synth_case(log_domain)
    c = bn.lib.c
    nv, n = circ.n_vars, circ.domain
    wit = wbytes(circ.witness)
    untouched = bytes(pd._raw(_WitnessReport))
    rows = (C.c_uint64 * 4)(*([0x5A5A5A5A5A5A5A5A] * 4))
    vals = (C.c_uint8 * (96 * 4))(*([0x5A] * (96 * 4)))
    rc = bn.load_circuit(blobs)

    def clean(rep):
        assert bytes(rep) == untouched and set(rows) == {0x5A5A5A5A5A5A5A5A} and set(vals) == {0x5A}

    def one_shot(k=blobs, w=wit, w_len=None, r=rows, v=vals, cap=4, null_circuit=False, null_rep=False):
        cs, keep = _circuit_struct(k)
        rep = pd._raw(_WitnessReport)
        code = c.wsnark_witness_check(None if null_circuit else C.byref(cs), w, len(wit) if w_len is None else w_len, r, v, cap,
                                      None if null_rep else C.byref(rep))
        clean(rep)
        return code

    def resident(h=rc._h, w=wit, w_len=None, r=rows, v=vals, cap=4, null_rep=False, dev=False):
        rep = pd._raw(_WitnessReport)
        args = [h, w, len(wit) if w_len is None else w_len, r, v, cap, None if null_rep else C.byref(rep)]
        code = c.wsnark_circuit_witness_check_dev(*args, None) if dev else c.wsnark_circuit_witness_check(*args)
        clean(rep)
        return code

    for call in (one_shot, resident):
        assert call(w_len=32 * nv - 1) == ERR_SIZE and call(w_len=0) == ERR_SIZE
        assert call(w=None) == ERR_ARG and call(null_rep=True) == ERR_ARG
        assert call(r=None) == ERR_ARG and call(v=None) == ERR_ARG and call(r=None, v=None, cap=1) == ERR_ARG
    assert one_shot(null_circuit=True) == ERR_ARG and resident(h=None) == ERR_ARG and resident(h=None, dev=True) == ERR_ARG
    assert resident(w=None, dev=True) == ERR_ARG and resident(w_len=32 * nv - 1, dev=True) == ERR_SIZE
    aligned = (C.c_uint8 * (len(wit) + 32))()      # a device witness that is not 16-byte aligned is refused before anything reads it
    base = (C.addressof(aligned) + 15) & ~15
    assert resident(w=C.c_void_p(base + 8), dev=True) == ERR_ARG and resident(w=C.c_void_p(base + 1), dev=True) == ERR_ARG
    assert c.wsnark_circuit_info(None, None, None, None, None, None) == ERR_ARG
    assert c.wsnark_circuit_info(rc._h, None, None, None, None, None) == 0      # any out pointer may be NULL
    # what wsnark_circuit_row_sums rejects of a circuit, with its codes: by the one-shot call and by the load
    cols = [list(col.items()) for col in circ.C]
    cols[nv - 1] = cols[nv - 1] + [(n, 5)]
    bad_circuits = [(dict(blobs, polsC=ps._records_blob(cols)), ERR_FORMAT), (dict(blobs, polsC=blobs["polsC"][:-1]), ERR_FORMAT),
                    (dict(blobs, polsA=blobs["polsA"][:-1]), ERR_FORMAT), (dict(blobs, n_public=nv), ERR_FORMAT),
                    (dict(blobs, domain=48), ERR_SIZE), (dict(blobs, domain=1 << 25), ERR_SIZE)]
    for k, code in bad_circuits:
        assert one_shot(k=k) == code, (k["domain"], k["n_public"], code)
        cs, keep = _circuit_struct(k)
        h = C.c_void_p()
        assert c.wsnark_circuit_load(C.byref(cs), C.byref(h)) == code and not h
    assert c.wsnark_circuit_load(None, C.byref(C.c_void_p())) == ERR_ARG
    cs, keep = _circuit_struct(blobs)
    assert c.wsnark_circuit_load(C.byref(cs), None) == ERR_ARG
    # cap == 0: both lists may be NULL
    rep = _WitnessReport()
    assert c.wsnark_circuit_witness_check(rc._h, wit, len(wit), None, None, 0, C.byref(rep)) == 0 and rep.ok == 1
    rep = _WitnessReport()
    assert c.wsnark_witness_check(C.byref(cs), wit, len(wit), None, None, 0, C.byref(rep)) == 0 and rep.ok == 1
    c.wsnark_circuit_free(None)
    rc.free()
    # before wsnark_init: a fresh process that loads the library and never initialises it
    code = ("import ctypes as C, sys\n"
            "c = C.CDLL(sys.argv[1])\n"
            "vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64\n"
            "c.wsnark_circuit_load.argtypes = [vp, vp]\n"
            "c.wsnark_circuit_free.argtypes = [vp]\n"
            "c.wsnark_circuit_free.restype = None\n"
            "c.wsnark_witness_check.argtypes = [vp, vp, sz, vp, vp, u64, vp]\n"
            "c.wsnark_circuit_witness_check.argtypes = [vp, vp, sz, vp, vp, u64, vp]\n"
            "c.wsnark_circuit_witness_check_dev.argtypes = [vp, vp, sz, vp, vp, u64, vp, vp]\n"
            "v = (C.c_uint8 * 96)(*([90] * 96))\n"
            "h = C.c_void_p()\n"
            "c.wsnark_circuit_free(None)\n"
            "print(c.wsnark_circuit_load(v, C.byref(h)), c.wsnark_witness_check(v, v, 96, None, None, 0, v),\n"
            "      c.wsnark_circuit_witness_check(None, v, 96, None, None, 0, v),\n"
            "      c.wsnark_circuit_witness_check_dev(None, v, 96, None, None, 0, v, None), set(v), h.value)\n")
    res = subprocess.run([sys.executable, "-c", code, so_path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == [str(ERR_NOINIT)] * 4 + ["{90}", "None"], (res.stdout, res.stderr)


# ---- 7. one handle, two threads ----
def check_two_threads(bn, log_domain=6, repeats=8):
    circ, blobs, rows3 = synth_case(log_domain)
    bad = list(circ.witness)
    bad[1 + N_FREE + 7] = (bad[1 + N_FREE + 7] + 1) % R
    wits = [circ.witness, bad]
    wants = [py_check(rows3, w, N_PUBLIC) for w in wits]
    assert wants[0]["ok"] == 1 and wants[1]["bad"] >= 1
    rc = bn.load_circuit(blobs)
    got, errors = [[], []], []

    def work(k):
        try:
            for _ in range(repeats):
                got[k].append(rc.check_witness(wbytes(wits[k]), max_rows=circ.domain))
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    rc.free()
    assert not errors, errors
    for k in range(2):
        assert len(got[k]) == repeats
        for rep in got[k]:
            assert_report(rep, wants[k], circ.domain, ("thread", k))


# ---- 8. the witness already on the device (device only) ----
def check_dev_variant(bn, log_domain):
    import torch
    circ, blobs, rows3 = synth_case(log_domain)
    bad = list(circ.witness)
    for v in planted_signals(log_domain):
        bad[v] = (bad[v] + 1) % R
    rc = bn.load_circuit(blobs)
    for wit in (circ.witness, bad):
        want = py_check(rows3, wit, N_PUBLIC)
        host = rc.check_witness(wbytes(wit), max_rows=circ.domain)
        assert_report(host, want, circ.domain, "host")
        src = torch.frombuffer(bytearray(wbytes(wit)), dtype=torch.uint8)
        d_w = src.cuda()
        torch.cuda.synchronize()
        assert_report(rc.check_witness_dev(d_w.data_ptr(), d_w.numel(), max_rows=circ.domain), want, circ.domain, "device, the lane's queue")
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d_w2 = src.to("cuda", non_blocking=True)
            got = rc.check_witness_dev(d_w2.data_ptr(), d_w2.numel(), max_rows=circ.domain, stream=st.cuda_stream)
        assert_report(got, want, circ.domain, "device, a torch stream")
        for name in ("bad_rows", "bad_values", "bad", "first_bad", "ok"):
            assert got[name] == host[name]
    rc.free()


# ---- 9. groth16GenProof(..., circuit=rc) ----
def check_gen_proof(bn, log_domain, dev=False):
    circ, blobs, rows3 = synth_case(log_domain)
    pkey, vk = synth.build_key(circ, synth.setup(circ, seed=11), bn.mul_base)
    key = bn.load_key(pkey)
    rc = bn.load_circuit(blobs)
    other = bn.load_circuit(synth_case(log_domain + 1)[1])
    r, s = bytes(range(1, 33)), bytes(range(40, 72))
    good = wbytes(circ.witness)
    w = list(circ.witness)
    v = 1 + N_FREE + 3
    w[v] = (w[v] + 1) % R
    want = py_check(rows3, w, N_PUBLIC)
    assert want["first_bad"] == 3
    text = "constraint 3: (A.w)(B.w) != C.w: a=%d, b=%d, c=%d" % want["bad_values"][0]

    def prove(wit, **kw):
        if not dev:
            return bn.groth16GenProof(wit, key, r=r, s=s, **kw)
        import torch
        d_w = torch.frombuffer(bytearray(wit), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        return bn.groth16GenProof_dev(d_w.data_ptr(), d_w.numel(), key, r=r, s=s, **kw)

    plain = prove(good)
    assert prove(good, circuit=rc) == plain and bn.groth16Verify(vk, synth.public_signals(circ), plain)
    for wit, circuit, needle in ((wbytes(w), rc, text), (good, other, "is not the key's"), (wbytes(w), other, "is not the key's")):
        try:
            prove(wit, circuit=circuit)
        except ValueError as e:
            assert needle in str(e), (needle, str(e))
        else:
            raise AssertionError("no ValueError: " + needle)
    if not dev:      # proving_key.bin bytes instead of a handle: the same, and the temporary key is freed either way
        assert bn.groth16GenProof(good, pkey, r=r, s=s, circuit=rc) == plain
    assert prove(wbytes(w)) != plain      # without a circuit nothing changes: a bad witness still proves
    for h in (rc, other, key):
        h.free()
