"""Shared checks of the batch prover (wsnark_groth16_prove_batch[_dev], csrc/provebatch.hip), run by tests/test_emul_prove_batch.py on
the thread-emulator build of the kernel sources and by tests/test_gpu_prove_batch.py on the device.

The yardstick everywhere is the single prover (wsnark_groth16_prove) on the SAME handle with the same r_i, s_i: proof i of a batch is
byte for byte what it writes (the bindings turn the 384 bytes into decimal strings one to one, so equal proofs are equal bytes).  A
witness need not satisfy the circuit for that: most witnesses are plain random bytes, values >= r included.  The reference's own
recorded proofs (tests/golden/proofs.json, unreduced.json) pin the batch path to the reference directly.

The routing switches are set by every check that wants the batch kernels (BATCH_MIN = 1, BATCH_MAX_DOMAIN = 2^16) and forgotten
afterwards, so no check depends on the shipped defaults; the report's `batched` says which path ran."""
import base64
import ctypes as C
import json
import os
import random
import subprocess
import sys
import threading

import pkey_delta_common as pd
from bn128_ref import R
from pkey_check_common import ERR_ARG, ERR_NOINIT, ERR_SIZE
from wasmsnark_amd import synth
from wasmsnark_amd.bn128 import _ProveBatchReport

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOP = (1 << 256) - 1
SWITCHES = ("BATCH_MIN", "BATCH_MAX_DOMAIN", "BATCH_CHUNK", "BATCH_WINDOW", "BATCH_STACK")
WINDOWS = (4, 5, 6, 7, 8)      # every width provebatch.hip accepts


class tuned:
    """the routing / geometry switches for the duration of a block; batch path unless told otherwise"""

    def __init__(self, bn, **kw):
        self.bn = bn
        self.kw = dict({"BATCH_MIN": 1, "BATCH_MAX_DOMAIN": 1 << 16}, **kw)

    def __enter__(self):
        for k, v in self.kw.items():
            self.bn.lib.tune(k, v)

    def __exit__(self, *exc):
        for k in SWITCHES:
            self.bn.lib.tune(k, None)


def rand_bytes(rnd, n):
    return bytes(rnd.getrandbits(8) for _ in range(n))


def wbytes(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


_memo = {}


def key_case(bn, log_domain, style="columns"):
    """(circuit, resident key, vk) of a synthetic key, made once per process and library"""
    k = (id(bn), log_domain, style)
    if k not in _memo:
        if style == "boolean":
            nc = synth.NativeCircuit(bn.lib, log_domain, n_public=2, seed=5, style="boolean")
            pkey, vk = nc.build_key()
            circ = type("BoolCircuit", (), {"n_vars": nc.n_vars, "n_public": nc.n_public, "domain": nc.domain,
                                            "witness_bytes": nc.witness_bin(), "public": nc.public_signals()})
        else:
            c = synth.make_circuit(log_domain, n_public=2, seed=3, style=style)
            pkey, vk = synth.build_key(c, synth.setup(c, seed=11), bn.mul_base)
            circ = type("Circuit", (), {"n_vars": c.n_vars, "n_public": c.n_public, "domain": c.domain,
                                        "witness_bytes": synth.witness_bin(c), "public": synth.public_signals(c)})
        _memo[k] = (circ, bn.load_key(pkey), vk)
    return _memo[k]


def single(bn, key, wits, rs, ss):
    return [bn.groth16GenProof(w, key, r=r, s=s) for w, r, s in zip(wits, rs, ss)]


def batch(bn, key, wits, rs, ss, want_batched=True, **switches):
    """the batch call under the given switches; the report must say which path ran"""
    rep = {}
    with tuned(bn, **switches):
        got, used = bn.groth16GenProofBatch(wits, key, r=rs, s=ss, return_blinding=True, report=rep)
    assert rep["count"] == len(wits) and rep["batched"] == (len(wits) if want_batched else 0), rep
    assert rep["window_bits"] == switches.get("BATCH_WINDOW", 8) and 1 <= rep["chunk"] <= max(len(wits), 1), rep
    assert rep["ms"]["total"] > 0 and set(rep["ms"]) == {"upload", "calc_h", "sums", "assembly", "total"}, rep
    if rs is not None and ss is not None:
        assert used == list(zip(rs, ss))
    return got


def blindings(rnd, count):
    return [rand_bytes(rnd, 32) for _ in range(count)], [rand_bytes(rnd, 32) for _ in range(count)]


# ---- 1. equals the single prover ----
def check_equals_single(bn, log_domain, style, count):
    circ, key, vk = key_case(bn, log_domain, style)
    rnd = random.Random(1000 * log_domain + count)
    wits = [circ.witness_bytes] + [rand_bytes(rnd, 32 * circ.n_vars) for _ in range(count - 1)]
    rs, ss = blindings(rnd, count)
    want = single(bn, key, wits, rs, ss)
    assert batch(bn, key, wits, rs, ss) == want
    if count <= 3:      # the witnesses back to back in one buffer: the same call
        rep = {}
        with tuned(bn):
            assert bn.groth16GenProofBatch(b"".join(wits), key, r=b"".join(rs), s=b"".join(ss), report=rep) == want
        assert rep["batched"] == count
    assert bn.groth16Verify(vk, circ.public, want[0])


# ---- 2. the reference's own proofs ----
def check_reference_proofs(bn):
    proofs = json.load(open(os.path.join(GOLDEN, "proofs.json")))
    U = json.load(open(os.path.join(GOLDEN, "unreduced.json")))
    rd = lambda name, ext: open(os.path.join(GOLDEN, "keys", name + ext), "rb").read()
    for name in ("t3", "t6"):
        key = bn.load_key(rd(name, ".pkey.bin"))
        cases = proofs[name]
        rs, ss = [bytes.fromhex(c["r"]) for c in cases], [bytes.fromhex(c["s"]) for c in cases]
        want = [c["proof"] for c in cases]
        witnesses = [rd(name, ".witness.bin")]
        if name == U["key"]:
            witnesses.append(base64.b64decode(U["witness_lifted"]))      # every value lifted by a multiple of r: the same proofs
        for wit in witnesses:
            assert batch(bn, key, [wit] * len(cases), rs, ss) == want, name
        key.free()


# ---- 3. adversarial witnesses, mixed into one batch with a random one ----
def check_adversarial(bn, log_domain):
    circ, key, vk = key_case(bn, log_domain, "rows")
    nv = circ.n_vars
    rnd = random.Random(77 + log_domain)
    one_hot = [0] * nv
    one_hot[nv // 2] = rnd.getrandbits(256)
    wits = [wbytes([0] * nv), wbytes([1] * nv), wbytes([TOP] * nv), wbytes(one_hot), rand_bytes(rnd, 32 * nv)]
    rs, ss = blindings(rnd, len(wits))
    rs[0] = ss[0] = bytes(32)      # all zero with r = s = 0: every sum is infinity
    want = single(bn, key, wits, rs, ss)
    assert batch(bn, key, wits, rs, ss) == want
    assert want[0]["pi_c"] == ["0", "1", "0"]      # ... and infinity prints as (0, 1, 0)


def check_boolean_heavy(bn, log_domain):
    circ, key, vk = key_case(bn, log_domain, "boolean")
    rnd = random.Random(91 + log_domain)
    wits = [circ.witness_bytes, rand_bytes(rnd, 32 * circ.n_vars), circ.witness_bytes]
    rs, ss = blindings(rnd, len(wits))
    want = single(bn, key, wits, rs, ss)
    assert batch(bn, key, wits, rs, ss) == want
    assert bn.groth16Verify(vk, circ.public, want[0])


# ---- 4. planted points ----
def check_planted_points(bn, log_domain):
    """Neighbouring signals hold equal points (A) and opposite points (C) and the witnesses are equal on them: in every window one
    bucket meets P + P or P + (-P), inside a piece or between two.  B1 and B2 are infinity throughout."""
    c = synth.make_circuit(log_domain, n_public=2, seed=3)
    sec, _ = synth.build_sections(c, synth.setup(c, seed=11), bn.mul_base)
    nv, nc = c.n_vars, c.n_vars - c.n_public - 1
    rnd = random.Random(13)
    logs = [rnd.randrange(1, R) for _ in range(nv)]
    a_logs = [logs[i - i % 2] for i in range(nv)]                                              # (P, P), (Q, Q), ...
    c_logs = [logs[i - i % 2] if i % 2 == 0 else R - logs[i - 1] for i in range(nv)][c.n_public + 1:]      # (P, -P), ... by SIGNAL index
    cat = lambda xs: b"".join(x.to_bytes(32, "little") for x in xs)
    planted = dict(sec, pointsA=bn.mul_base(1, cat(a_logs)), pointsC=bn.mul_base(1, cat(c_logs[:nc])),
                   pointsB1=bytes(64 * nv), pointsB2=bytes(128 * nv))
    key = bn.load_key(sections=planted)
    wits = []
    for _ in range(3):
        vals = [rnd.getrandbits(256) for _ in range(nv)]
        wits.append(wbytes([vals[i - i % 2] for i in range(nv)]))
    wits.append(wbytes([3] * nv))      # every entry of window 0 in ONE bucket, cut into pieces: the pairs meet between pieces too
    rs, ss = blindings(rnd, len(wits))
    want = single(bn, key, wits, rs, ss)
    assert batch(bn, key, wits, rs, ss) == want
    assert batch(bn, key, wits, rs, ss, BATCH_WINDOW=4) == want
    key.free()


# ---- 5. geometry and routing change nothing ----
def check_geometry(bn, log_domain):
    circ, key, vk = key_case(bn, log_domain, "rows")
    rnd = random.Random(5 + log_domain)
    wits = [circ.witness_bytes] + [rand_bytes(rnd, 32 * circ.n_vars) for _ in range(4)]
    rs, ss = blindings(rnd, 5)
    want = single(bn, key, wits, rs, ss)
    assert batch(bn, key, wits, rs, ss) == want
    assert batch(bn, key, wits, rs, ss, BATCH_CHUNK=2) == want
    for c in WINDOWS:
        assert batch(bn, key, wits, rs, ss, BATCH_WINDOW=c, BATCH_CHUNK=3) == want, c
    assert batch(bn, key, wits, rs, ss, want_batched=False, BATCH_MAX_DOMAIN=circ.domain // 2) == want
    assert batch(bn, key, wits, rs, ss, want_batched=False, BATCH_MIN=6) == want
    for c in (3, 9):      # a width the kernels do not have is refused, not rounded
        try:
            batch(bn, key, wits, rs, ss, BATCH_WINDOW=c)
        except Exception as e:      # noqa: BLE001
            assert getattr(e, "code", None) == ERR_ARG, e
        else:
            raise AssertionError("BATCH_WINDOW=%d accepted" % c)


# ---- 6. drawn blinding ----
def check_drawn_blinding(bn, log_domain):
    circ, key, vk = key_case(bn, log_domain, "columns")
    rnd = random.Random(6)
    wits = [circ.witness_bytes] * 3 + [rand_bytes(rnd, 32 * circ.n_vars)]
    fixed_s = [rand_bytes(rnd, 32) for _ in wits]
    for want_batched, sw in ((True, {}), (False, {"BATCH_MIN": 5})):
        rep = {}
        with tuned(bn, **sw):
            proofs, used = bn.groth16GenProofBatch(wits, key, return_blinding=True, report=rep)
            proofs2, used2 = bn.groth16GenProofBatch(wits, key, s=fixed_s, return_blinding=True)
        assert rep["batched"] == (len(wits) if want_batched else 0)
        flat = [v for pair in used for v in pair]
        assert len(set(flat)) == 2 * len(wits) and all(len(v) == 32 and v != bytes(32) for v in flat)      # one independent draw per proof
        assert [p[1] for p in used2] == fixed_s and len({p[0] for p in used2} | {p[0] for p in used}) == 2 * len(wits)
        assert single(bn, key, wits, [p[0] for p in used], [p[1] for p in used]) == proofs
        assert single(bn, key, wits, [p[0] for p in used2], fixed_s) == proofs2
        assert bn.groth16VerifyBatch(vk, [circ.public] * 4, proofs) == [True, True, True, False]
        assert all(bn.groth16Verify(vk, circ.public, p) for p in proofs[:3])


# ---- 7. errors leave the outputs and the report untouched ----
def check_errors(bn, so_path, log_domain=4):
    circ, key, vk = key_case(bn, log_domain, "columns")
    c = bn.lib.c
    nv = circ.n_vars
    wit = circ.witness_bytes * 2
    r32 = bytes(range(64))

    def call(h=key._h, w=wit, stride=32 * nv, count=2, dev=False, want=None):
        out, rs, rep = (C.c_uint8 * 768)(*([90] * 768)), (C.c_uint8 * 128)(*([90] * 128)), pd._raw(_ProveBatchReport)
        before = bytes(rep)
        args = [h, w, stride, count, r32, r32, out, rs, C.byref(rep)]
        code = c.wsnark_groth16_prove_batch_dev(*args, None) if dev else c.wsnark_groth16_prove_batch(*args)
        if want != "written":
            assert set(out) == {90} and set(rs) == {90} and bytes(rep) == before, code
        return code

    with tuned(bn):
        for dev in (False, True):
            assert call(h=None, dev=dev) == ERR_ARG and call(w=None, dev=dev) == ERR_ARG
            assert call(stride=32 * nv - 1, dev=dev) == ERR_SIZE and call(stride=0, dev=dev) == ERR_SIZE
            assert call(count=(1 << 16) + 1, dev=dev) == ERR_SIZE
            assert call(count=0, dev=dev) == 0 and call(count=0, w=None, dev=dev) == 0      # touches nothing
        rep = _ProveBatchReport()
        assert c.wsnark_groth16_prove_batch(key._h, wit, 32 * nv, 2, r32, r32, None, None, C.byref(rep)) == ERR_ARG and rep.count == 0
        # a device witness that is not 16-byte aligned (pointer or stride) is refused before anything reads it
        assert call(w=C.c_void_p(C.addressof(C.create_string_buffer(64)) | 8), dev=True) == ERR_ARG
        assert call(stride=32 * nv + 8, dev=True) == ERR_ARG
        # out_rs64s and the report may be NULL
        out = (C.c_uint8 * 768)()
        assert c.wsnark_groth16_prove_batch(key._h, wit, 32 * nv, 2, r32, r32, out, None, None) == 0
        from wasmsnark_amd.bn128 import proof_to_bytes
        half = len(wit) // 2
        want = single(bn, key, [wit[:half], wit[half:]], [r32[:32], r32[32:]], [r32[:32], r32[32:]])
        assert bytes(out) == b"".join(proof_to_bytes(p) for p in want)
    # a points shard is refused whichever path the call would take
    from wasmsnark_amd import formats
    sec = formats.pkey_bin_to_sections(open(os.path.join(GOLDEN, "keys", "t3.pkey.bin"), "rb").read())
    w3 = open(os.path.join(GOLDEN, "keys", "t3.witness.bin"), "rb").read()
    # ... and so is a handle whose hExps slice is interleaved (the distributed CALC_H's layout), even at a world of one
    for shard in (bn.load_key(sections=sec, shard=(0, 2)), bn.load_key(sections=sec, shard=(0, 1), h_interleave_log=1)):
        for sw in ({}, {"BATCH_MIN": 9}):
            with tuned(bn, **sw):
                assert call(h=shard._h, w=w3 * 2, stride=len(w3)) == ERR_ARG
        shard.free()
    # before wsnark_init: a fresh process that loads the library and never initialises it
    code = ("import ctypes as C, sys\n"
            "c = C.CDLL(sys.argv[1])\n"
            "vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64\n"
            "c.wsnark_groth16_prove_batch.argtypes = [vp, vp, sz, u64, vp, vp, vp, vp, vp]\n"
            "c.wsnark_groth16_prove_batch_dev.argtypes = [vp, vp, sz, u64, vp, vp, vp, vp, vp, vp]\n"
            "v = (C.c_uint8 * 768)(*([90] * 768))\n"
            "print(c.wsnark_groth16_prove_batch(v, v, 32, 2, None, None, v, v, v),\n"
            "      c.wsnark_groth16_prove_batch_dev(v, v, 32, 2, None, None, v, v, v, None),\n"
            "      c.wsnark_groth16_prove_batch(None, v, 32, 0, None, None, v, v, v), set(v))\n")
    res = subprocess.run([sys.executable, "-c", code, so_path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == [str(ERR_NOINIT)] * 3 + ["{90}"], (res.stdout, res.stderr)


# ---- 8. two threads, one handle ----
def check_two_threads(bn, log_domain=6, repeats=3):
    circ, key, vk = key_case(bn, log_domain, "columns")
    rnd = random.Random(8)
    jobs = []
    for count in (3, 4):
        wits = [circ.witness_bytes] + [rand_bytes(rnd, 32 * circ.n_vars) for _ in range(count - 1)]
        rs, ss = blindings(rnd, count)
        jobs.append((wits, rs, ss, single(bn, key, wits, rs, ss)))
    got, errors = [[], []], []

    def work(k):
        try:
            for _ in range(repeats):
                rep = {}
                got[k].append((bn.groth16GenProofBatch(jobs[k][0], key, r=jobs[k][1], s=jobs[k][2], report=rep), rep["batched"]))
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    with tuned(bn):
        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not errors, errors
    for k in range(2):
        assert got[k] == [(jobs[k][3], len(jobs[k][0]))] * repeats, k


# ---- 9. the witnesses already on the device (device only) ----
def check_dev_variant(bn, log_domain):
    import torch
    circ, key, vk = key_case(bn, log_domain, "rows")
    rnd = random.Random(9 + log_domain)
    nv, count = circ.n_vars, 3
    wits = [circ.witness_bytes] + [rand_bytes(rnd, 32 * nv) for _ in range(count - 1)]
    rs, ss = blindings(rnd, count)
    want = single(bn, key, wits, rs, ss)
    for pad in (0, 48):      # packed, and a stride larger than nVars*32: the bytes between two witnesses are never read
        stride = 32 * nv + pad
        blob = b"".join(w + b"\xff" * pad for w in wits)
        src = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
        d_w = src.cuda()
        torch.cuda.synchronize()
        for sw, want_batched in (({}, True), ({"BATCH_MIN": 4}, False)):
            rep = {}
            with tuned(bn, **sw):
                got = bn.groth16GenProofBatch_dev(d_w.data_ptr(), stride, count, key, r=rs, s=ss, report=rep)
            assert got == want and rep["batched"] == (count if want_batched else 0), (pad, sw)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            d_w2 = src.to("cuda", non_blocking=True)
            with tuned(bn):
                got, used = bn.groth16GenProofBatch_dev(d_w2.data_ptr(), stride, count, key, r=rs, s=ss, return_blinding=True, stream=st.cuda_stream)
        assert got == want and used == list(zip(rs, ss)), pad
