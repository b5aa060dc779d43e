"""Shared checks of snarkjs' .zkey in and out and of the H basis change (wsnark_g1_h_basis, wsnark_zkey_*, csrc/zkey.hip), run by
tests/test_emul_zkey.py on the thread-emulator build of the kernel sources and by tests/test_gpu_zkey.py on the device.

The yardsticks do not come from the library.  The basis change is compared with its definition in Python integers (the transform of
pkey_setup_common on the points' LOGARITHMS, the twist w_2n^k on top), carried back to the group by mul_base -- an independent kernel
that the parity tests pin.  A .zkey is written here, by model_zkey, from a synthetic circuit's toxic waste: N_i = L^{2n}_{2i+1}(tau) /
delta as integers, coefficients as c R^2, records in snarkjs' order -- a second implementation of the format of README.md's "zkey"
section that never calls the library's writer.  Its import must be synth.build_key's closed form byte for byte.  The reference-format
golden keys of tests/golden/keys anchor the opposite direction.

One deviation from "import == synth.build_key(circ, S)": synth's "columns" circuits hold a column's records in the order the
generator drew them, not by constraint, and a key's streams are by contract ascending in the constraint.  The closed form is
therefore built from the same circuit with every column dict sorted by constraint (sorted_circuit): same matrices, same points."""
import ctypes as C
import copy
import json
import os
import random
import struct
import subprocess
import sys

import pkey_setup_common as ps
from bn128_ref import Q, R, le
from pkey_check_common import ERR_ARG, ERR_FORMAT, ERR_NOINIT, ERR_SIZE
from wasmsnark_amd import formats, synth
from wasmsnark_amd._lib import WsnarkError

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MONT = 1 << 256
SNARKJS_ORDER = (1, 2, 4, 3, 9, 8, 5, 6, 7, 10)      # not numeric: sections are found by type


# ---- the basis change in Python integers ----
def to_monomial(N):
    """hExps_k = (-2 w_2n^k) sum_i w_n^(ik) N_i"""
    n = len(N)
    w2 = synth.root_of_unity(n.bit_length())
    t = ps.ntt_logs(N, False)
    return [(-2 * pow(w2, k, R) * t[k]) % R for k in range(n)]


def to_lagrange(h):
    """N_i = n^-1 sum_k w_n^(-ik) (-2 w_2n^k)^-1 h_k"""
    n = len(h)
    w2 = synth.root_of_unity(n.bit_length())
    return ps.ntt_logs([h[k] * pow(-2 * pow(w2, k, R), -1, R) % R for k in range(n)], True)


def closed_forms(tau, delta, bits, inverse_root=False):
    """(N_i, hExps_k) of one tau and delta: L^{2n}_{2i+1}(tau) / delta and tau^k (tau^n - 1) / delta.  inverse_root: the odd points
    taken under w_2n^-1 -- what a writer with the other root convention would store."""
    n = 1 << bits
    L2, _ = synth.lagrange_at(tau, bits + 1)
    dinv = pow(delta, -1, R)
    N = [L2[(-(2 * i + 1)) % (2 * n) if inverse_root else 2 * i + 1] * dinv % R for i in range(n)]
    z = (pow(tau, n, R) - 1) * dinv % R
    return N, [pow(tau, k, R) * z % R for k in range(n)]


def check_identity_in_integers():
    """The two formulas against the closed forms, and against the transform's definition, for n = 2 .. 32"""
    rnd = random.Random(5)
    for bits in range(1, 6):
        N, h = closed_forms(rnd.randrange(2, R), rnd.randrange(2, R), bits)
        assert to_monomial(N) == h and to_lagrange(h) == N
        n, w, w2 = 1 << bits, synth.root_of_unity(bits), synth.root_of_unity(bits + 1)
        x = [rnd.randrange(R) for _ in range(n)]
        assert to_monomial(x) == [(-2 * pow(w2, k, R) * sum(pow(w, i * k, R) * x[i] for i in range(n))) % R for k in range(n)]
        assert to_lagrange(to_monomial(x)) == x
        assert w2 * w2 % R == w


# ---- 1. wsnark_g1_h_basis ----
def check_basis_definition(bn, max_bits):
    for bits in range(1, max_bits + 1):
        logs = ps.logs_for(bits, seed=31)
        data = ps.points_of_logs(bn, 1, logs)
        for lag, model in ((False, to_monomial), (True, to_lagrange)):
            want = ps.points_of_logs(bn, 1, model(logs))
            got = bn.h_basis(data, to_lagrange=lag)
            assert got == want, (bits, lag, ps.differing(1, got, want))
            assert bn.h_basis(got, to_lagrange=not lag) == ps.points_of_logs(bn, 1, logs), (bits, lag)


def check_basis_corners(bn, bits):
    n = 1 << bits
    inf9 = bytes(32) + bytes([9]) + bytes(31)      # infinity by the loaders' rule, with a non-zero y
    for lag in (False, True):
        model = to_lagrange if lag else to_monomial
        assert bn.h_basis(bytes(64 * n), to_lagrange=lag) == bytes(64 * n) == bn.h_basis(inf9 * n, to_lagrange=lag)
        for pos in (0, n - 1, n // 2 + 1 if n > 2 else 1):
            logs = [0] * n
            logs[pos] = 0xC0FFEE
            data = bytearray(ps.points_of_logs(bn, 1, logs))
            data[64 * ((pos + 1) % n):64 * ((pos + 1) % n) + 64] = inf9
            got, want = bn.h_basis(data, to_lagrange=lag), ps.points_of_logs(bn, 1, model(logs))
            assert got == want, (bits, lag, pos, ps.differing(1, got, want))
        logs = [0xC0FFEE] * n                       # a constant array
        got, want = bn.h_basis(ps.points_of_logs(bn, 1, logs), to_lagrange=lag), ps.points_of_logs(bn, 1, model(logs))
        assert got == want, (bits, lag, ps.differing(1, got, want))
        # chosen outputs at infinity: the input is the integer model's preimage of an array with zeros
        rnd = random.Random(77 + bits)
        target = [rnd.randrange(1, R) for _ in range(n)]
        for i in (0, n - 1, n // 3):
            target[i] = 0
        pre = (to_monomial if lag else to_lagrange)(target)
        assert model(pre) == target
        got = bn.h_basis(ps.points_of_logs(bn, 1, pre), to_lagrange=lag)
        assert got == ps.points_of_logs(bn, 1, target), (bits, lag)
        assert got[:64] == bytes(64) and got[64 * (n - 1):] == bytes(64)


def check_basis_uniform_switch(bn, bits, tune):
    logs = ps.logs_for(bits, seed=32)
    data = ps.points_of_logs(bn, 1, logs)
    want = [ps.points_of_logs(bn, 1, to_monomial(logs)), ps.points_of_logs(bn, 1, to_lagrange(logs))]
    for lag in (False, True):
        assert bn.h_basis(data, to_lagrange=lag) == want[lag], lag


def check_basis_errors(bn):
    c = bn.lib.c
    pts = bytearray(ps.points_of_logs(bn, 1, list(range(1, 65))))
    out = (C.c_uint8 * len(pts))(*([0x5A] * len(pts)))
    buf = (C.c_uint8 * len(pts)).from_buffer(pts)
    for n in (0, 1, 3, 48, (1 << 24) + 1, 1 << 25):
        assert c.wsnark_g1_h_basis(buf, n, 0, out) == ERR_SIZE, n
    assert c.wsnark_g1_h_basis(None, 4, 0, out) == ERR_ARG and c.wsnark_g1_h_basis(buf, 4, 1, None) == ERR_ARG
    for index, lag in ((0, 0), (37, 1), (63, 0), (63, 1)):
        bad = bytearray(pts)
        bad[64 * index + 32] ^= 1
        b = (C.c_uint8 * len(bad)).from_buffer(bad)
        assert c.wsnark_g1_h_basis(b, 64, lag, out) == ERR_FORMAT
        assert ("index %d" % index) in c.wsnark_last_error().decode(), c.wsnark_last_error()
    bad = bytearray(pts)
    bad[64 * 9:64 * 9 + 32] = le(int.from_bytes(pts[64 * 9:64 * 9 + 32], "little") + Q)      # unreduced
    b = (C.c_uint8 * len(bad)).from_buffer(bad)
    assert c.wsnark_g1_h_basis(b, 64, 1, out) == ERR_FORMAT and "index 9" in c.wsnark_last_error().decode()
    assert set(out) == {0x5A}


# ---- the model writer ----
def sorted_circuit(circ):
    """the same circuit with every column's records by ascending constraint: the order a key's streams have by contract"""
    c2 = copy.copy(circ)
    c2.A, c2.B, c2.C = ([dict(sorted(col.items())) for col in m] for m in (circ.A, circ.B, circ.C))
    return c2


def circuit_records(circ):
    """Section 4 in snarkjs' order: constraint by constraint, matrix 0's terms by ascending signal, then matrix 1's; the value is the
    plain coefficient (zkey_bytes writes it as c R^2)"""
    rows = [([], []) for _ in range(circ.domain)]
    for m, cols in enumerate((circ.A, circ.B)):
        for s, col in enumerate(cols):
            for c, coef in col.items():
                rows[c][m].append((s, coef))
    return [(m, c, s, coef) for c in range(circ.domain) for m in (0, 1) for s, coef in sorted(rows[c][m])]


def record_bytes(records, shift=2):
    """(matrix, constraint, signal, c) -> the 44-byte records with c R^shift mod r; an entry with a fifth element is written raw"""
    out = bytearray()
    for rec in records:
        m, c, s, v = rec[:4]
        out += struct.pack("<III", m, c, s) + le(v if len(rec) > 4 else v * pow(MONT, shift, R) % R)
    return bytes(out)


def zkey_parts(bn, circ, S, inverse_root=False):
    """The ten sections of the model file as a dict {type: payload}, from the toxic waste"""
    nv, npub, n = circ.n_vars, circ.n_public, circ.domain
    bits = n.bit_length() - 1
    dinv, ginv = pow(S.delta, -1, R), pow(S.gamma, -1, R)
    kc = [(S.beta * S.a[s] + S.alpha * S.b[s] + S.c[s]) % R for s in range(nv)]
    N, _ = closed_forms(S.tau, S.delta, bits, inverse_root)
    P1 = lambda logs: ps.points_of_logs(bn, 1, logs)
    P2 = lambda logs: ps.points_of_logs(bn, 2, logs)
    head = (struct.pack("<I", 32) + le(Q) + struct.pack("<I", 32) + le(R) + struct.pack("<III", nv, npub, n)
            + P1([S.alpha, S.beta]) + P2([S.beta, S.gamma]) + P1([S.delta]) + P2([S.delta]))
    recs = circuit_records(circ)
    return {1: struct.pack("<I", 1), 2: head, 3: P1([kc[s] * ginv % R for s in range(npub + 1)]),
            4: struct.pack("<I", len(recs)) + record_bytes(recs), 5: P1(S.a), 6: P1(S.b), 7: P2(S.b),
            8: P1([kc[s] * dinv % R for s in range(npub + 1, nv)]), 9: P1(N), 10: bytes(64) + struct.pack("<I", 0)}


def zkey_bytes(parts, order=None, version=1, magic=b"zkey"):
    order = list(order if order is not None else sorted(parts))
    out = magic + struct.pack("<II", version, len(order))
    for t in order:
        out += struct.pack("<IQ", t if isinstance(t, int) else t[0], len(parts[t])) + parts[t]
    return out


def put(parts, t, payload):
    out = dict(parts)
    out[t] = payload
    return out


def with_records(parts, records, shift=2):
    return put(parts, 4, struct.pack("<I", len(records)) + record_bytes(records, shift))


_model_memo = {}


def model(bn, log_domain, style, seed=3, n_public=2):
    """(circuit with sorted columns, toxic waste, the model file's sections, the closed form: (proving_key.bin, vk)), built once"""
    key = (id(bn), log_domain, style, seed, n_public)
    if key not in _model_memo:
        circ = sorted_circuit(synth.make_circuit(log_domain, n_public=n_public, seed=seed, style=style))
        S = synth.setup(circ, seed=seed + 50)
        _model_memo[key] = (circ, S, zkey_parts(bn, circ, S), synth.build_key(circ, S, bn.mul_base))
    return _model_memo[key]


def streams_of(records, n_vars):
    """The two column streams the contract asks of a record list: per matrix, the records stably sorted by constraint, then every
    signal's in that order; the value with one Montgomery factor taken off.  Also the counts of the report."""
    rinv = pow(MONT, -1, R)
    out, unreduced, zero = [], [0, 0], [0, 0]
    for m in (0, 1):
        mine = sorted([r for r in records if r[0] == m], key=lambda r: r[1])      # (stable)
        cols = [[] for _ in range(n_vars)]
        for rec in mine:
            v = rec[3] if len(rec) > 4 else rec[3] * MONT * MONT % R
            unreduced[m] += v >= R
            zero[m] += v % R == 0
            cols[rec[2]].append((rec[1], v * rinv % R))
        blob = bytearray()
        for col in cols:
            blob += struct.pack("<I", len(col))
            for c, v in col:
                blob += struct.pack("<I", c) + le(v)
        out.append(bytes(blob))
    return out, tuple(unreduced), tuple(zero)


def pkey_streams(pkey):
    h = struct.unpack_from("<10I", pkey)
    return pkey[h[3]:h[4]], pkey[h[4]:h[5]]


# ---- 2. import equals the closed form ----
def check_import_closed_form(bn, log_domain, style):
    circ, S, parts, (want_pkey, want_vk) = model(bn, log_domain, style)
    z = zkey_bytes(parts)
    info = bn.zkey_info(z)
    recs = circuit_records(circ)
    assert info == {"n_vars": circ.n_vars, "n_public": circ.n_public, "domain": circ.domain, "n_coeffs": len(recs),
                    "records": (sum(r[0] == 0 for r in recs), sum(r[0] == 1 for r in recs)), "n_contributions": 0,
                    "pkey_len": len(want_pkey), "vk_len": 448 + 64 * (circ.n_public + 1)}
    rep = {}
    pkey, vk = bn.import_zkey(z, report=rep)
    assert pkey == want_pkey, [i for i in range(0, len(want_pkey), 4) if pkey[i:i + 4] != want_pkey[i:i + 4]][:8]
    assert vk == want_vk
    assert rep["records"] == info["records"] and rep["unreduced"] == (0, 0) and rep["zero"] == (0, 0) and rep["sorted"] is True
    assert rep["H"] == {"points": circ.domain, "infinity": 0, "bad": 0, "first_bad": None, "first_reason": None}
    assert set(rep["ms"]) == {"upload", "coefficients", "h_basis", "download", "total"} and rep["ms"]["total"] >= rep["ms"]["h_basis"] > 0
    # hExps including k = n - 1, which no proof reads
    hoff = struct.unpack_from("<10I", pkey)[9]
    _, h = closed_forms(S.tau, S.delta, log_domain)
    assert pkey[hoff + 64 * (circ.domain - 1):hoff + 64 * circ.domain] == ps.points_of_logs(bn, 1, h[-1:])
    # the sections form, the non-numeric section order and an unknown section type give the same key
    sec, vk2 = bn.import_zkey(zkey_bytes(put(parts, 77, b"unknown"), order=SNARKJS_ORDER[:4] + (77,) + SNARKJS_ORDER[4:]), sections=True)
    assert synth.sections_to_pkey(sec) == want_pkey and vk2 == want_vk
    # export is the inverse, byte for byte
    rep = {}
    assert bn.export_zkey(pkey=pkey, vk=vk, report=rep) == z
    assert bn.export_zkey(sections=sec, vk=vk) == z and rep["records"] == info["records"] and rep["H"]["bad"] == 0


def check_import_from_path(bn, tmp_path):
    circ, S, parts, (want_pkey, want_vk) = model(bn, 3, "rows")
    path = os.path.join(str(tmp_path), "model.zkey")
    with open(path, "wb") as f:
        f.write(zkey_bytes(parts, order=SNARKJS_ORDER))
    assert bn.zkey_info(path=path)["n_coeffs"] == len(circuit_records(circ))
    assert bn.import_zkey(path=path) == (want_pkey, want_vk)


# ---- 3. the golden keys ----
def golden(name):
    with open(os.path.join(GOLDEN, "keys", name + ".meta.json")) as f:
        meta = json.load(f)
    rd = lambda ext: open(os.path.join(GOLDEN, "keys", name + ext), "rb").read()
    with open(os.path.join(GOLDEN, "keys", name + ".vk.json")) as f:
        vk = json.load(f)
    with open(os.path.join(GOLDEN, "proofs.json")) as f:
        proofs = json.load(f)[name]
    return meta, rd(".pkey.bin"), rd(".witness.bin"), vk, proofs


def check_golden_key(bn, name):
    meta, pkey, wit, vk, proofs = golden(name)
    circ = synth.make_circuit(meta["log_domain"], n_public=meta["n_public"], seed=meta["circuit_seed"], style="rows")
    S = synth.setup(circ, seed=meta["setup_seed"])
    z = bn.export_zkey(pkey=pkey, vk=vk)
    info = bn.zkey_info(z)
    assert (info["n_vars"], info["n_public"], info["domain"], info["pkey_len"]) == (circ.n_vars, circ.n_public, circ.domain, len(pkey))
    # the H section is the closed form N_i; the whole file is the model writer's
    N, _ = closed_forms(S.tau, S.delta, meta["log_domain"])
    assert z[-(12 + 68) - 64 * circ.domain:-(12 + 68)] == ps.points_of_logs(bn, 1, N)
    assert z == zkey_bytes(zkey_parts(bn, circ, S))
    back, vk2 = bn.import_zkey(z)
    assert back == pkey and {k: v for k, v in vk.items() if k in vk2} == vk2
    # the golden witness as .wtns proves on the re-imported key to the golden key's bytes, and the proof verifies
    wtns = formats.witness_bin_to_wtns(wit)
    assert formats.wtns_to_witness_bin(wtns) == wit
    r, s = bytes.fromhex(proofs[0]["r"]), bytes.fromhex(proofs[0]["s"])
    proof = bn.groth16GenProof(formats.wtns_to_witness_bin(wtns), back, r=r, s=s)
    assert proof == proofs[0]["proof"] == bn.groth16GenProof(wit, pkey, r=r, s=s)
    assert bn.groth16Verify(vk2, synth.public_signals(circ), proof) is True


# ---- 4. the trial proof ----
def check_trial_proof(bn, log_domain):
    circ, S, parts, (want_pkey, want_vk) = model(bn, log_domain, "rows")
    wtns = formats.witness_bin_to_wtns(synth.witness_bin(circ))
    assert bn.import_zkey(zkey_bytes(parts), wtns=wtns) == (want_pkey, want_vk)
    sec, _ = bn.import_zkey(zkey_bytes(parts), wtns=wtns, sections=True)
    assert synth.sections_to_pkey(sec) == want_pkey
    wrong_root = put(parts, 9, zkey_parts(bn, circ, S, inverse_root=True)[9])
    wrong_coef = with_records(parts, circuit_records(circ), shift=1)
    for name, bad in (("H under w_2n^-1", wrong_root), ("coefficients as c R", wrong_coef)):
        assert bn.import_zkey(zkey_bytes(bad))[1] == want_vk      # (it parses: only the proof tells)
        try:
            bn.import_zkey(zkey_bytes(bad), wtns=wtns)
            raise AssertionError("the trial proof passed on a file with " + name)
        except ValueError as e:
            assert "trial proof" in str(e)
    bad_wtns = bytearray(wtns)
    bad_wtns[-32] ^= 1                                              # another witness: not one of this circuit
    try:
        bn.import_zkey(zkey_bytes(parts), wtns=bytes(bad_wtns))
        raise AssertionError("the trial proof passed on a wrong witness")
    except ValueError:
        pass


# ---- 5. record order ----
def _import_streams(bn, parts, records, rep=None):
    pkey, _ = bn.import_zkey(zkey_bytes(with_records(parts, records)), report=rep)
    return pkey_streams(pkey)


def check_record_order(bn, log_domain, tune):
    circ, S, parts, _ = model(bn, log_domain, "rows")
    nv, n = circ.n_vars, circ.domain
    base = circuit_records(circ)
    rnd = random.Random(19)
    # shuffled across constraints, with duplicates of (matrix, constraint, signal), zero values and values >= r
    recs = list(base)
    for k in range(12):
        m, c, s, v = base[rnd.randrange(len(base))]
        recs += [(m, c, s, rnd.randrange(R)), (m, c, s, 0), (m, c, s, R + k, "raw"), (m, rnd.randrange(n), s, R, "raw")]
    recs += [(1, n - 1, nv - 1, (1 << 256) - 1, "raw")]
    rnd.shuffle(recs)
    want, unreduced, zero = streams_of(recs, nv)
    for tile in (None, 256):
        if tile:
            tune(bn.lib, "ROWS_TILE", tile)
        rep = {}
        assert list(_import_streams(bn, parts, recs, rep)) == want, tile
        assert rep["sorted"] is False and rep["unreduced"] == unreduced and rep["zero"] == zero and min(unreduced) > 0 and min(zero) > 0
        assert rep["records"] == (sum(r[0] == 0 for r in recs), sum(r[0] == 1 for r in recs))
    # only ONE matrix out of order; the stably sorted file gives the same streams and says so
    one = [r for r in base if r[0] == 0] + list(reversed([r for r in base if r[0] == 1]))
    rep = {}
    assert list(_import_streams(bn, parts, one, rep)) == streams_of(one, nv)[0] and rep["sorted"] is False
    rep = {}
    assert list(_import_streams(bn, parts, sorted(recs, key=lambda r: r[1]), rep)) == want and rep["sorted"] is True
    # a matrix without records; no records at all
    for keep in (0, 1, None):
        only = [r for r in base if r[0] == keep]
        rep = {}
        assert list(_import_streams(bn, parts, only, rep)) == streams_of(only, nv)[0]
        assert rep["records"] == (len(only) if keep == 0 else 0, len(only) if keep == 1 else 0)


def check_tile_edges(bn, tune):
    """255 .. 257 and 2047 .. 2049 records under ROWS_TILE 256 and 2048: the partition's and the sort's tile edges"""
    circ, S, parts, _ = model(bn, 3, "rows")
    nv, n = circ.n_vars, circ.domain
    rnd = random.Random(23)
    pool = [(rnd.randrange(2), rnd.randrange(n), rnd.randrange(nv), rnd.randrange(1, R)) for _ in range(2049)]
    for tile in (256, 2048):
        tune(bn.lib, "ROWS_TILE", tile)
        for count in (255, 256, 257, 2047, 2048, 2049):
            recs = pool[:count]
            want = streams_of(recs, nv)[0]
            assert list(_import_streams(bn, parts, recs)) == want, (tile, count)
            srt = sorted(recs, key=lambda r: r[1])
            assert list(_import_streams(bn, parts, srt)) == want, (tile, count, "sorted")


# ---- 6. the container and the errors ----
_OUT_SIZES = lambda nv, npub, n, la, lb: (la, lb, 64 * nv, 64 * nv, 128 * nv, 64 * (nv - npub - 1), 64 * n, 64, 64, 64, 128, 128)


def check_errors(bn, so_path):
    from wasmsnark_amd.bn128 import _ZkeyReport
    circ, S, parts, (want_pkey, want_vk) = model(bn, 3, "rows")
    c = bn.lib.c
    nv, npub, n = circ.n_vars, circ.n_public, circ.domain
    la, lb = (len(x) for x in pkey_streams(want_pkey))
    sizes = _OUT_SIZES(nv, npub, n, la, lb)
    guard = 64
    fresh = lambda size: (C.c_uint8 * (size + 2 * guard))(*([0x5A] * (size + 2 * guard)))
    vk_len = 448 + 64 * (npub + 1)

    def call(z, code, *words):
        z = bytes(z)
        bufs = [fresh(sz) for sz in sizes]
        ptrs = (C.c_void_p * 12)(*[C.addressof(b) + guard for b in bufs])
        caps = (C.c_uint64 * 12)(*sizes)
        vk, big, rep, rep2 = fresh(vk_len), fresh(len(want_pkey)), fresh(C.sizeof(_ZkeyReport)), fresh(C.sizeof(_ZkeyReport))
        ln = C.c_size_t(12345)
        rc = c.wsnark_zkey_import_sections(z, len(z), ptrs, caps, C.addressof(vk) + guard, vk_len, C.addressof(rep) + guard)
        msg = c.wsnark_last_error().decode()
        rc2 = c.wsnark_zkey_import(z, len(z), C.addressof(big) + guard, len(want_pkey), C.byref(ln), C.addressof(vk) + guard, vk_len,
                                   C.addressof(rep2) + guard)
        assert rc == rc2 == code, (rc, rc2, code, words, msg)
        for w in words:
            assert w in msg, (w, msg)
        assert all(set(b) == {0x5A} for b in bufs + [vk, big, rep, rep2]) and ln.value == 12345, words
        info = fresh(56)
        assert c.wsnark_zkey_info(z, len(z), C.addressof(info) + guard) == code and set(info) == {0x5A}

    good = zkey_bytes(parts)
    head = parts[2]
    patch = lambda off, b: head[:off] + b + head[off + len(b):]
    call(zkey_bytes(parts, magic=b"zkex"), ERR_FORMAT, "magic")
    call(zkey_bytes(parts, version=2), ERR_FORMAT, "version")
    for proto, word in ((2, "PLONK"), (10, "FFLONK"), (0, "protocol")):
        call(zkey_bytes(put(parts, 1, struct.pack("<I", proto))), ERR_FORMAT, "protocol", word)
    call(zkey_bytes(put(parts, 2, patch(0, struct.pack("<I", 48)))), ERR_FORMAT, "n8q")
    call(zkey_bytes(put(parts, 2, patch(36, struct.pack("<I", 31)))), ERR_FORMAT, "n8r")
    call(zkey_bytes(put(parts, 2, patch(4, le(R)))), ERR_FORMAT, "q is not")
    call(zkey_bytes(put(parts, 2, patch(40, le(Q)))), ERR_FORMAT, "r is not")
    call(zkey_bytes(put(parts, 2, patch(76, struct.pack("<I", nv)))), ERR_FORMAT, "nPublic + 1 > nVars")
    for dom in (12, 1, 1 << 25):
        call(zkey_bytes(put(parts, 2, patch(80, struct.pack("<I", dom)))), ERR_SIZE, "domainSize")
    for t in range(3, 10):
        call(zkey_bytes(put(parts, t, parts[t] + bytes(4))), ERR_FORMAT, "section %d" % t, "size")
        call(zkey_bytes(put(parts, t, parts[t][:-4])), ERR_FORMAT, "section %d" % t, "size")
    call(zkey_bytes(put(parts, 2, head + bytes(4))), ERR_FORMAT, "section 2", "size")
    for cut in (3, 11, 20, len(good) // 2, len(good) - 1):
        call(good[:cut], ERR_FORMAT, "truncated")
    for t in range(1, 10):                                          # a missing and a doubled section
        call(zkey_bytes(parts, order=[x for x in sorted(parts) if x != t]), ERR_FORMAT, "section %d" % t, "missing")
    dup = dict(parts)
    dup[(5, "again")] = parts[5]
    call(zkey_bytes(dup, order=sorted(parts) + [(5, "again")]), ERR_FORMAT, "section 5", "twice")
    recs = circuit_records(circ)
    k = len(recs) // 2
    plant = lambda rec: with_records(parts, recs[:k] + [rec] + recs[k + 1:])
    call(zkey_bytes(plant((2, 0, 0, 1))), ERR_FORMAT, "matrix > 1")
    # (the next two only the device finds: wsnark_zkey_info accepts them)
    for rec, word in (((0, 0, nv, 1), "signal >= nVars"), ((1, n, 0, 1), "constraint >= domainSize")):
        z = zkey_bytes(plant(rec))
        bufs = [fresh(sz) for sz in sizes]
        ptrs = (C.c_void_p * 12)(*[C.addressof(b) + guard for b in bufs])
        vk, rep = fresh(vk_len), fresh(C.sizeof(_ZkeyReport))
        rc = c.wsnark_zkey_import_sections(z, len(z), ptrs, (C.c_uint64 * 12)(*sizes), C.addressof(vk) + guard, vk_len, C.addressof(rep) + guard)
        msg = c.wsnark_last_error().decode()
        assert rc == ERR_FORMAT and word in msg and ("record %d" % k) in msg, msg
        assert all(set(b) == {0x5A} for b in bufs + [vk, rep])
    # a bad H point: its index
    for index in (0, n - 1):
        h = bytearray(parts[9])
        h[64 * index + 32] ^= 1
        z = zkey_bytes(put(parts, 9, bytes(h)))
        try:
            bn.import_zkey(z)
            raise AssertionError("an off-curve H point was imported")
        except WsnarkError as e:
            assert e.code == ERR_FORMAT and ("index %d" % index) in str(e), str(e)
    bad_key = bytearray(want_pkey)
    bad_key[struct.unpack_from("<10I", want_pkey)[9] + 64 * 5 + 32] ^= 1
    try:
        bn.export_zkey(pkey=bytes(bad_key), vk=want_vk)
        raise AssertionError("an off-curve hExps point was exported")
    except WsnarkError as e:
        assert e.code == ERR_FORMAT and "index 5" in str(e), str(e)
    # capacities
    bufs = [fresh(sz) for sz in sizes]
    vk, rep = fresh(vk_len), fresh(C.sizeof(_ZkeyReport))
    for short in (0, 6, 11):
        caps = (C.c_uint64 * 12)(*[sz - (1 if i == short else 0) for i, sz in enumerate(sizes)])
        ptrs = (C.c_void_p * 12)(*[C.addressof(b) + guard for b in bufs])
        assert c.wsnark_zkey_import_sections(good, len(good), ptrs, caps, C.addressof(vk) + guard, vk_len, C.addressof(rep) + guard) == ERR_SIZE
    big = fresh(len(want_pkey))
    assert c.wsnark_zkey_import(good, len(good), C.addressof(big) + guard, len(want_pkey) - 1, None, C.addressof(vk) + guard, vk_len,
                                C.addressof(rep) + guard) == ERR_SIZE
    assert c.wsnark_zkey_import(good, len(good), C.addressof(big) + guard, len(want_pkey), None, C.addressof(vk) + guard, vk_len - 1,
                                C.addressof(rep) + guard) == ERR_SIZE
    assert all(set(b) == {0x5A} for b in bufs + [vk, rep, big])
    out = fresh(len(good))
    vkb = __import__("wasmsnark_amd").bn128.vk_to_bytes(want_vk, npub)
    ln = C.c_size_t(777)
    assert c.wsnark_zkey_export(want_pkey, len(want_pkey), None, 0, npub, C.addressof(out) + guard, len(good), C.byref(ln), C.addressof(rep) + guard) == ERR_ARG
    assert c.wsnark_zkey_export(want_pkey, len(want_pkey), vkb, len(vkb), npub, C.addressof(out) + guard, len(good) - 1, C.byref(ln),
                                C.addressof(rep) + guard) == ERR_SIZE
    assert c.wsnark_zkey_export(want_pkey, len(want_pkey), vkb, len(vkb), npub + 1, C.addressof(out) + guard, len(good), C.byref(ln),
                                C.addressof(rep) + guard) == ERR_ARG
    assert set(out) == set(rep) == {0x5A} and ln.value == 777
    need = C.c_size_t()
    assert c.wsnark_zkey_export_size(nv, npub, n, (la - 4 * nv) // 36, (lb - 4 * nv) // 36, C.byref(need)) == 0 and need.value == len(good)
    # before wsnark_init: every device entry point refuses, wsnark_zkey_info works
    code = ("import ctypes as C, sys\n"
            "c = C.CDLL(sys.argv[1])\n"
            "z = bytes.fromhex(sys.argv[2])\n"
            "vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64\n"
            "c.wsnark_g1_h_basis.argtypes = [vp, u64, C.c_int, vp]\n"
            "c.wsnark_zkey_info.argtypes = [vp, sz, vp]\n"
            "c.wsnark_zkey_import.argtypes = [vp, sz, vp, sz, vp, vp, sz, vp]\n"
            "c.wsnark_zkey_import_sections.argtypes = [vp, sz, vp, vp, vp, sz, vp]\n"
            "c.wsnark_zkey_export.argtypes = [vp, sz, vp, sz, u64, vp, sz, vp, vp]\n"
            "c.wsnark_zkey_export_sections.argtypes = [vp, vp, sz, u64, vp, sz, vp, vp]\n"
            "o = (C.c_uint8 * 4096)(*([90] * 4096))\n"
            "info = (C.c_uint32 * 14)()\n"
            "print(c.wsnark_g1_h_basis(o, 2, 0, o), c.wsnark_zkey_import(z, len(z), o, 4096, None, o, 4096, o),\n"
            "      c.wsnark_zkey_import_sections(z, len(z), o, o, o, 4096, o), c.wsnark_zkey_export(o, 4096, o, 4096, 1, o, 4096, None, o),\n"
            "      c.wsnark_zkey_export_sections(o, o, 4096, 1, o, 4096, None, o), set(o), c.wsnark_zkey_info(z, len(z), info), info[0], info[2])\n")
    res = subprocess.run([sys.executable, "-c", code, so_path, good.hex()], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.split() == [str(ERR_NOINIT)] * 5 + ["{90}", "0", str(nv), str(n)], (res.stdout, res.stderr)


def check_wtns_format():
    wit = b"".join(le(v) for v in (1, 5, R - 1, 7))
    w = formats.witness_bin_to_wtns(wit)
    assert w[:12] == b"wtns" + struct.pack("<II", 2, 2) and len(w) == 12 + 12 + 40 + 12 + 128 and formats.wtns_to_witness_bin(w) == wit
    swapped = w[:12] + w[12 + 52:] + w[12:12 + 52]                   # section 2 first: found by type
    assert formats.wtns_to_witness_bin(swapped) == wit
    for bad in (b"wtnx" + w[4:], w[:4] + struct.pack("<I", 1) + w[8:], w[:-1], w[:24] + struct.pack("<I", 31) + w[28:],
                w[:28] + le(Q) + w[60:]):
        try:
            formats.wtns_to_witness_bin(bad)
            raise AssertionError("a malformed .wtns was read")
        except formats.FormatError:
            pass
