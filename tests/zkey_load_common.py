"""Shared checks of a snarkjs .zkey loaded straight into a resident proving key (wsnark_pkey_load_zkey, wsnark_pkey_load_zkey_file,
Bn128.load_zkey; csrc/zkey.hip: zkey_load), run by tests/test_emul_zkey_load.py on the thread-emulator build of the kernel sources and
by tests/test_gpu_zkey_load.py on the device.

The yardsticks are independent of the new code: the model .zkey that zkey_common.model() writes from a synthetic circuit's toxic waste,
synth.expected_proof (the proof's closed form) and the unchanged two-step path load_key(import_zkey(z)[0]).  Two handles are compared
through what a user can see of them: their numbers, and the BYTES of proofs under fixed blinding values -- of the circuit's witness
and of a witness of raw 256-bit values, some >= r: a missing or wrong entry of a resident matrix changes A.w at its row with
probability 1 - 1/r, and pi_c with it."""
import ctypes as C
import os
import random
import struct
import subprocess
import sys

import zkey_common as zk
from bn128_ref import R, le
from zkey_common import ERR_ARG, ERR_FORMAT, ERR_NOINIT, ERR_SIZE
from wasmsnark_amd import formats, synth
from wasmsnark_amd._lib import WsnarkError

R32 = le(0x1234567 * 0x89ABCDEF + (1 << 200))
S32 = le((1 << 255) + 0xFEEDFACE)                 # (>= r: reduced by the prover)


def raw_witness(n_vars, seed):
    """n_vars raw 256-bit values with the constant 1 in front; every fifth one >= r"""
    rnd = random.Random(seed)
    vals = [1] + [rnd.randrange(R, 1 << 256) if i % 5 == 0 else rnd.randrange(R) for i in range(1, n_vars)]
    return b"".join(le(v) for v in vals)


def two_step(bn, z, report=None, wait_tables=True):
    pkey, vk = bn.import_zkey(z, report=report)
    return bn.load_key(pkey, wait_tables=wait_tables), vk


def same_numbers(a, b):
    assert (a.n_vars, a.n_public, a.domain) == (b.n_vars, b.n_public, b.domain)
    assert a.table == b.table and a.shard == b.shard, (a.table, b.table, a.shard, b.shard)


def same_proofs(bn, a, b, witnesses):
    for i, w in enumerate(witnesses):
        pa, pb = bn.groth16GenProof(w, a, r=R32, s=S32), bn.groth16GenProof(w, b, r=R32, s=S32)
        assert pa == pb, ("witness %d" % i, pa, pb)


# ---- 1. the closed form ----
def check_closed_form(bn, log_domain, style, tmp_path):
    circ, S, parts, (want_pkey, want_vk) = zk.model(bn, log_domain, style)
    wit = synth.witness_bin(circ)
    want = synth.expected_proof(circ, S, R32, S32, bn.mul_base)
    z = zk.zkey_bytes(parts)
    path = os.path.join(str(tmp_path), "model_%d.zkey" % log_domain)
    with open(path, "wb") as f:      # snarkjs' section order, an unknown section among them: sections are found by type
        f.write(zk.zkey_bytes(zk.put(parts, 77, b"unknown"), order=zk.SNARKJS_ORDER[:4] + (77,) + zk.SNARKJS_ORDER[4:]))
    recs = zk.circuit_records(circ)
    for how in ("bytes", "file"):
        rep = {}
        key, vk = bn.load_zkey(z, report=rep) if how == "bytes" else bn.load_zkey(path=path, report=rep)
        try:
            assert vk == want_vk and key.vk == want_vk, how
            assert (key.n_vars, key.n_public, key.domain) == (circ.n_vars, circ.n_public, circ.domain)
            assert key.shard["rank"] == 0 and key.shard["world"] == 1 and key.shard["n_signals"] == circ.n_vars and key.shard["n_hexps"] == circ.domain
            proof = bn.groth16GenProof(wit, key, r=R32, s=S32)
            assert proof == want, (how, proof, want)
            assert bn.groth16Verify(vk, synth.public_signals(circ), proof) is True
            assert rep["records"] == (sum(r[0] == 0 for r in recs), sum(r[0] == 1 for r in recs))
            assert rep["unreduced"] == (0, 0) and rep["zero"] == (0, 0) and rep["sorted"] is True
            assert rep["H"] == {"points": circ.domain, "infinity": 0, "bad": 0, "first_bad": None, "first_reason": None}
            assert rep["ms"]["download"] == 0 and rep["ms"]["total"] >= rep["ms"]["h_basis"] > 0
        finally:
            key.free()
    # the drop-in call with the file's bytes as the key
    assert bn.groth16GenProof(wit, z, r=R32, s=S32) == want


# ---- 2. the same handle as the two-step path ----
def check_same_handle(bn, log_domain, style):
    circ, S, parts, _ = zk.model(bn, log_domain, style)
    z = zk.zkey_bytes(parts)
    wit, raw = synth.witness_bin(circ), raw_witness(circ.n_vars, 41)
    ref, vk_ref = two_step(bn, z)
    key, vk = bn.load_zkey(z)
    late, _ = bn.load_zkey(z, wait_tables=False)
    try:
        assert vk == vk_ref
        same_numbers(key, ref)
        same_numbers(late, ref)
        same_proofs(bn, key, ref, [wit, raw])
        # one call of four witnesses
        four = [wit, raw, raw_witness(circ.n_vars, 42), wit]
        rs, ss = [le(1000 + i) for i in range(4)], [le(2000 + i) for i in range(4)]
        assert bn.groth16GenProofBatch(four, key, r=rs, s=ss) == bn.groth16GenProofBatch(four, ref, r=rs, s=ss)
        # before the tables are waited for and after
        first = bn.groth16GenProof(raw, late, r=R32, s=S32)
        late.wait_tables()
        assert first == bn.groth16GenProof(raw, late, r=R32, s=S32) == bn.groth16GenProof(raw, ref, r=R32, s=S32)
        assert set(key.load_ms) == set(ref.load_ms) and key.load_ms["total"] > 0
    finally:
        for k in (ref, key, late):
            k.free()


# ---- 3. record order and corners ----
def record_lists(circ):
    """zkey_common.check_record_order's lists, and two whose records all sit in one row"""
    nv, n = circ.n_vars, circ.domain
    base = zk.circuit_records(circ)
    rnd = random.Random(19)
    recs = list(base)
    for k in range(12):
        m, c, s, v = base[rnd.randrange(len(base))]
        recs += [(m, c, s, rnd.randrange(R)), (m, c, s, 0), (m, c, s, R + k, "raw"), (m, rnd.randrange(n), s, R, "raw")]
    recs += [(1, n - 1, nv - 1, (1 << 256) - 1, "raw")]
    rnd.shuffle(recs)
    one = [r for r in base if r[0] == 0] + list(reversed([r for r in base if r[0] == 1]))
    lists = [("shuffled", recs, False), ("one matrix out of order", one, False), ("stably sorted", sorted(recs, key=lambda r: r[1]), True)]
    for keep in (0, 1, None):
        lists.append(("only matrix %s" % keep, [r for r in base if r[0] == keep], True))
    for row in (0, n - 1):
        lists.append(("all in row %d" % row, [(m, row, s, rnd.randrange(1, R)) for s in range(nv) for m in (0, 1)] + [(0, row, 1, 7), (1, row, 1, 0)], True))
    return lists


def check_record_order(bn, log_domain, tune, tile):
    """tile: ROWS_TILE, None = the default"""
    circ, S, parts, _ = zk.model(bn, log_domain, "rows")
    witnesses = [synth.witness_bin(circ), raw_witness(circ.n_vars, 43)]
    if tile:
        tune(bn.lib, "ROWS_TILE", tile)
    for name, recs, is_sorted in record_lists(circ):
        z = zk.zkey_bytes(zk.with_records(parts, recs))
        rep_ref, rep = {}, {}
        ref, _ = two_step(bn, z, report=rep_ref)
        key, _ = bn.load_zkey(z, report=rep)
        try:
            same_numbers(key, ref)
            same_proofs(bn, key, ref, witnesses)
            for field in ("records", "unreduced", "zero", "sorted"):
                assert rep[field] == rep_ref[field], (name, tile, field, rep[field], rep_ref[field])
            _, unreduced, zero = zk.streams_of(recs, circ.n_vars)
            assert rep["unreduced"] == unreduced and rep["zero"] == zero and rep["sorted"] is is_sorted, (name, tile, rep)
        finally:
            ref.free()
            key.free()


# ---- 4. tile edges ----
def check_tile_edges(bn, tune, tile):
    circ, S, parts, _ = zk.model(bn, 3, "rows")
    nv, n = circ.n_vars, circ.domain
    rnd = random.Random(23)
    pool = [(rnd.randrange(2), rnd.randrange(n), rnd.randrange(nv), rnd.randrange(1, R)) for _ in range(2049)]
    witnesses = [raw_witness(nv, 44)]
    tune(bn.lib, "ROWS_TILE", tile)
    for count in (255, 256, 257, 2047, 2048, 2049):
        z = zk.zkey_bytes(zk.with_records(parts, pool[:count]))
        ref, _ = two_step(bn, z)
        key, _ = bn.load_zkey(z)
        try:
            same_proofs(bn, key, ref, witnesses)
        finally:
            ref.free()
            key.free()


# ---- 5. H corners ----
def check_h_corners(bn, log_domain):
    circ, S, parts, _ = zk.model(bn, log_domain, "rows")
    n = circ.domain
    witnesses = [synth.witness_bin(circ), raw_witness(circ.n_vars, 45)]
    for where in ((0,), (n - 1,), (0, n - 1)):
        h = bytearray(parts[9])
        for i in where:
            h[64 * i:64 * i + 64] = bytes(64)
        z = zk.zkey_bytes(zk.put(parts, 9, bytes(h)))
        rep = {}
        ref, _ = two_step(bn, z)
        key, _ = bn.load_zkey(z, report=rep)
        try:
            assert rep["H"]["infinity"] == len(where) and rep["H"]["bad"] == 0 and rep["H"]["points"] == n, rep
            same_proofs(bn, key, ref, witnesses)
        finally:
            ref.free()
            key.free()
    for index in (0, n - 1):
        h = bytearray(parts[9])
        h[64 * index + 32] ^= 1
        try:
            bn.load_zkey(zk.zkey_bytes(zk.put(parts, 9, bytes(h))))
            raise AssertionError("an off-curve H point was loaded")
        except WsnarkError as e:
            assert e.code == ERR_FORMAT and ("index %d" % index) in str(e), str(e)


# ---- 6. errors leave everything untouched ----
def malformed_files(bn):
    """zkey_common.check_errors' malformed files: (file, code, words of the message)"""
    circ, S, parts, _ = zk.model(bn, 3, "rows")
    nv, n = circ.n_vars, circ.domain
    good = zk.zkey_bytes(parts)
    head = parts[2]
    patch = lambda off, b: head[:off] + b + head[off + len(b):]
    put, zb = zk.put, zk.zkey_bytes
    out = [(zb(parts, magic=b"zkex"), ERR_FORMAT, ("magic",)), (zb(parts, version=2), ERR_FORMAT, ("version",))]
    for proto, word in ((2, "PLONK"), (10, "FFLONK"), (0, "protocol")):
        out.append((zb(put(parts, 1, struct.pack("<I", proto))), ERR_FORMAT, ("protocol", word)))
    out += [(zb(put(parts, 2, patch(0, struct.pack("<I", 48)))), ERR_FORMAT, ("n8q",)),
            (zb(put(parts, 2, patch(36, struct.pack("<I", 31)))), ERR_FORMAT, ("n8r",)),
            (zb(put(parts, 2, patch(4, le(R)))), ERR_FORMAT, ("q is not",)),
            (zb(put(parts, 2, patch(40, le(zk.Q)))), ERR_FORMAT, ("r is not",)),
            (zb(put(parts, 2, patch(76, struct.pack("<I", nv)))), ERR_FORMAT, ("nPublic + 1 > nVars",))]
    for dom in (12, 1, 1 << 25):
        out.append((zb(put(parts, 2, patch(80, struct.pack("<I", dom)))), ERR_SIZE, ("domainSize",)))
    for t in range(3, 10):
        out.append((zb(put(parts, t, parts[t] + bytes(4))), ERR_FORMAT, ("section %d" % t, "size")))
        out.append((zb(put(parts, t, parts[t][:-4])), ERR_FORMAT, ("section %d" % t, "size")))
    out.append((zb(put(parts, 2, head + bytes(4))), ERR_FORMAT, ("section 2", "size")))
    for cut in (0, 3, 11, 20, len(good) // 2, len(good) - 1):
        out.append((good[:cut], ERR_FORMAT, ("truncated",)))
    for t in range(1, 10):
        out.append((zb(parts, order=[x for x in sorted(parts) if x != t]), ERR_FORMAT, ("section %d" % t, "missing")))
    dup = dict(parts)
    dup[(5, "again")] = parts[5]
    out.append((zb(dup, order=sorted(parts) + [(5, "again")]), ERR_FORMAT, ("section 5", "twice")))
    recs = zk.circuit_records(circ)
    k = len(recs) // 2
    plant = lambda rec: zk.with_records(parts, recs[:k] + [rec] + recs[k + 1:])
    out.append((zb(plant((2, 0, 0, 1))), ERR_FORMAT, ("matrix > 1",)))
    out.append((zb(plant((0, 0, nv, 1))), ERR_FORMAT, ("signal >= nVars", "record %d" % k)))
    out.append((zb(plant((1, n, 0, 1))), ERR_FORMAT, ("constraint >= domainSize", "record %d" % k)))
    for index in (0, n - 1):
        h = bytearray(parts[9])
        h[64 * index + 32] ^= 1
        out.append((zb(put(parts, 9, bytes(h))), ERR_FORMAT, ("of H", "index %d" % index)))
    return out


def check_errors(bn, so_path, tmp_path):
    from wasmsnark_amd.bn128 import _ZkeyReport
    circ, S, parts, (want_pkey, want_vk) = zk.model(bn, 3, "rows")
    c = bn.lib.c
    vk_len = 448 + 64 * (circ.n_public + 1)
    fresh = lambda size: (C.c_uint8 * size)(*([0x5A] * size))
    sentinel = 0x5A5A5A5A5A50
    path = os.path.join(str(tmp_path), "bad.zkey")

    def both(z, vk_cap=vk_len):
        """(code, message) of the two entry points on z; the handle, the vk and the report must be as they were"""
        got = []
        for how in ("bytes", "file"):
            h, vk, rep = C.c_void_p(sentinel), fresh(vk_len), fresh(C.sizeof(_ZkeyReport))
            if how == "file":
                with open(path, "wb") as f:
                    f.write(z)
                rc = c.wsnark_pkey_load_zkey_file(os.fsencode(path), C.byref(h), vk, vk_cap, rep)
            else:
                rc = c.wsnark_pkey_load_zkey(z, len(z), C.byref(h), vk, vk_cap, rep)
            got.append((rc, c.wsnark_last_error().decode()))
            assert rc != 0, how
            assert h.value == sentinel and set(vk) == {0x5A} and set(rep) == {0x5A}, how
        return got

    for z, code, words in malformed_files(bn):
        z = bytes(z)
        big, vk, rep = fresh(len(want_pkey) + 64), fresh(vk_len), fresh(C.sizeof(_ZkeyReport))
        rc = c.wsnark_zkey_import(z, len(z), big, len(want_pkey), None, vk, vk_len, rep)
        msg = c.wsnark_last_error().decode()
        assert rc == code and all(w in msg for w in words), (rc, code, words, msg)      # (the yardstick itself)
        for rc2, msg2 in both(z):
            assert rc2 == code and msg2 == msg, (words, rc2, msg2, msg)
        # ... and through the Python mirror, bytes and path: the same code and text (nothing in front of the load walks the records)
        for kw in ({"zkey": z}, {"path": path}):
            try:
                bn.load_zkey(**kw)[0].free()
                raise AssertionError("a malformed file was loaded: " + repr(words))
            except WsnarkError as e:
                assert e.code == code and msg in str(e), (words, kw.keys(), str(e), msg)
        # the verification key's length alone: the container's errors with the same texts; what only section 4's records or the H
        # points tell is not its business
        ln = C.c_size_t(4242)
        rc3 = c.wsnark_zkey_vk_len(z, len(z), C.byref(ln))
        rc4 = c.wsnark_zkey_vk_len_file(os.fsencode(path), C.byref(ln))
        if any(w in ("matrix > 1", "signal >= nVars", "constraint >= domainSize", "of H") for w in words):
            assert rc3 == rc4 == 0 and ln.value == vk_len, words
        else:
            assert rc3 == rc4 == code and c.wsnark_last_error().decode() == msg and ln.value == 4242, (words, rc3, rc4)
    good = zk.zkey_bytes(parts)
    assert [rc for rc, _ in both(good, vk_cap=vk_len - 1)] == [ERR_SIZE, ERR_SIZE]
    # a file that is not there; NULL arguments
    h, vk, rep = C.c_void_p(sentinel), fresh(vk_len), fresh(C.sizeof(_ZkeyReport))
    assert c.wsnark_pkey_load_zkey_file(os.fsencode(os.path.join(str(tmp_path), "missing.zkey")), C.byref(h), vk, vk_len, rep) == ERR_ARG
    assert "cannot open" in c.wsnark_last_error().decode()
    assert c.wsnark_pkey_load_zkey_file(None, C.byref(h), vk, vk_len, rep) == ERR_ARG
    assert c.wsnark_pkey_load_zkey(None, len(good), C.byref(h), vk, vk_len, rep) == ERR_ARG
    assert c.wsnark_pkey_load_zkey(good, len(good), None, vk, vk_len, rep) == ERR_ARG
    assert c.wsnark_pkey_load_zkey(good, len(good), C.byref(h), None, vk_len, rep) == ERR_ARG
    assert h.value == sentinel and set(vk) == {0x5A} and set(rep) == {0x5A}
    # the verification key and the report are optional
    h = C.c_void_p()
    assert c.wsnark_pkey_load_zkey(good, len(good), C.byref(h), None, 0, None) == 0 and h.value
    c.wsnark_pkey_free(h)
    # before wsnark_init, in a fresh process
    with open(path, "wb") as f:
        f.write(good)
    code = ("import ctypes as C, sys\n"
            "c = C.CDLL(sys.argv[1])\n"
            "z = open(sys.argv[2], 'rb').read()\n"
            "vp, sz = C.c_void_p, C.c_size_t\n"
            "c.wsnark_pkey_load_zkey.argtypes = [vp, sz, C.POINTER(vp), vp, sz, vp]\n"
            "c.wsnark_pkey_load_zkey_file.argtypes = [C.c_char_p, C.POINTER(vp), vp, sz, vp]\n"
            "o = (C.c_uint8 * 4096)(*([90] * 4096))\n"
            "h = vp(77)\n"
            "print(c.wsnark_pkey_load_zkey(z, len(z), C.byref(h), o, 4096, o), c.wsnark_pkey_load_zkey_file(sys.argv[2].encode(), C.byref(h), o, 4096, o),\n"
            "      set(o), h.value)\n")
    res = subprocess.run([sys.executable, "-c", code, so_path, path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == [str(ERR_NOINIT)] * 2 + ["{90}", "77"], (res.stdout, res.stderr)


# ---- 7. the trial proof ----
def check_trial_proof(bn, log_domain):
    circ, S, parts, (want_pkey, want_vk) = zk.model(bn, log_domain, "rows")
    wtns = formats.witness_bin_to_wtns(synth.witness_bin(circ))
    key, vk = bn.load_zkey(zk.zkey_bytes(parts), wtns=wtns)
    key.free()
    assert vk == want_vk
    wrong_root = zk.put(parts, 9, zk.zkey_parts(bn, circ, S, inverse_root=True)[9])
    wrong_coef = zk.with_records(parts, zk.circuit_records(circ), shift=1)
    for name, bad in (("H under w_2n^-1", wrong_root), ("coefficients as c R", wrong_coef)):
        key, vk = bn.load_zkey(zk.zkey_bytes(bad))                   # (it parses: only the proof tells)
        key.free()
        assert vk == want_vk
        try:
            bn.load_zkey(zk.zkey_bytes(bad), wtns=wtns)
            raise AssertionError("the trial proof passed on a file with " + name)
        except ValueError as e:
            assert "trial proof" in str(e)
    bad_wtns = bytearray(wtns)
    bad_wtns[-32] ^= 1
    try:
        bn.load_zkey(zk.zkey_bytes(parts), wtns=bytes(bad_wtns))
        raise AssertionError("the trial proof passed on a wrong witness")
    except ValueError:
        pass


# ---- 8. the golden keys ----
def check_golden_key(bn, name):
    meta, pkey, wit, vk, proofs = zk.golden(name)
    key, vk2 = bn.load_zkey(bn.export_zkey(pkey=pkey, vk=vk))
    try:
        assert {k: v for k, v in vk.items() if k in vk2} == vk2
        for case in proofs[:2]:
            assert bn.groth16GenProof(wit, key, r=bytes.fromhex(case["r"]), s=bytes.fromhex(case["s"])) == case["proof"]
    finally:
        key.free()
