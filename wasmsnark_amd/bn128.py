"""Host-side mirror of the reference's JS API for the prove path, over the C ABI.

Mirrors /root/reference src/bn128.js (class Bn128, `build()`), main_bn128.js
(window.groth16GenProof) and README.md:28-30 (genZKSnarkProof): same names, same argument
meaning (byte buffers in the reference's layouts), same return shapes (Jacobian-Montgomery
byte strings for the multiexps, plain-form h for calcH, an object of decimal strings for
proofs).  The Node.js drop-in (wasmsnark_amd/js) binds the same C ABI through N-API; this
Python mirror exists so the parity tests read like the reference's own tests.
"""
import ctypes as C
import os
import struct
import weakref

from . import _lib


_Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583


def _mont(v):
    return ((v << 256) % _Q).to_bytes(32, "little")


# generators (src/bn128/build_bn128.js:59-90), affine Montgomery
G1_GEN = _mont(1) + _mont(2)
G2_GEN = (_mont(10857046999023057135944570762232829481370756359578518086990519993285655852781)
          + _mont(11559732032986387107991004021392285783925812861821192530917403151452391805634)
          + _mont(8495653923123431417604973247489272438418190587263600148770280649306958101930)
          + _mont(4082367875863433681332203403145435568316851327593401208105741076214120093531))


def _buf(b):
    """Private mutable copy (for entry points that work in place)."""
    if isinstance(b, (bytes, bytearray, memoryview)):
        b = bytes(b)
        return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b if len(b) else b"\0"), len(b)
    raise TypeError("expected a bytes-like object (the reference takes ArrayBuffers)")


def _ro(b):
    """Read-only input without a copy: the C side borrows the caller's bytes for the duration of the call
    (a 2^20-pair MSM input is 96 MB; copying it in Python cost more than the MSM)."""
    if isinstance(b, bytes):
        return (C.c_char_p(b) if len(b) else C.c_char_p(b"\0")), len(b)
    if isinstance(b, bytearray):
        return ((C.c_uint8 * len(b)).from_buffer(b) if len(b) else C.c_char_p(b"\0")), len(b)
    if isinstance(b, memoryview):
        return _ro(b.obj if isinstance(b.obj, (bytes, bytearray)) and b.nbytes == len(b.obj) else bytes(b))
    raise TypeError("expected a bytes-like object (the reference takes ArrayBuffers)")


class _KeySections(C.Structure):   # wsnark_key_sections_t
    _fields_ = [("n_vars", C.c_uint32), ("n_public", C.c_uint32), ("domain", C.c_uint32),
                ("alfa1", C.c_void_p), ("beta1", C.c_void_p), ("delta1", C.c_void_p),
                ("beta2", C.c_void_p), ("delta2", C.c_void_p),
                ("polsA", C.c_void_p), ("polsA_len", C.c_uint64), ("polsB", C.c_void_p), ("polsB_len", C.c_uint64),
                ("pointsA", C.c_void_p), ("pointsA_len", C.c_uint64), ("pointsB1", C.c_void_p), ("pointsB1_len", C.c_uint64),
                ("pointsB2", C.c_void_p), ("pointsB2_len", C.c_uint64), ("pointsC", C.c_void_p), ("pointsC_len", C.c_uint64),
                ("pointsH", C.c_void_p), ("pointsH_len", C.c_uint64)]


class _KeyReport(C.Structure):     # wsnark_pkey_report_t
    _fields_ = [("points", C.c_uint64 * 5), ("infinity", C.c_uint64 * 5), ("bad", C.c_uint64 * 5), ("first_bad", C.c_uint64 * 5),
                ("first_reason", C.c_uint32 * 5), ("fixed_reason", C.c_uint32 * 5),
                ("relations_run", C.c_uint32), ("relations_bad", C.c_uint32), ("ok", C.c_uint32), ("ms", C.c_double * 4)]


KEY_SECTIONS = ("A", "B1", "B2", "C", "H")                                  # report order (WSNARK_PK_A ..)
KEY_FIXED = ("alfa1", "beta1", "delta1", "beta2", "delta2")
KEY_RELATIONS = ("beta1~beta2", "delta1~delta2", "B1~B2")                   # bits 0, 1, 2
KEY_REASONS = {0: None, 1: "unreduced", 2: "off_curve", 3: "outside_subgroup", 4: "infinity"}


def _report_dict(r):
    """wsnark_pkey_report_t as a plain dict: per-section dicts keyed "A", "B1", "B2", "C", "H", then fixed, relations, ok, ms."""
    out = {}
    for k, name in enumerate(KEY_SECTIONS):
        bad = int(r.bad[k])
        out[name] = {"points": int(r.points[k]), "infinity": int(r.infinity[k]), "bad": bad,
                     "first_bad": int(r.first_bad[k]) if bad else None, "first_reason": KEY_REASONS[r.first_reason[k]] if bad else None}
    out["fixed"] = {name: KEY_REASONS[r.fixed_reason[k]] for k, name in enumerate(KEY_FIXED)}
    out["relations"] = {name: (None if not (r.relations_run >> k) & 1 else not (r.relations_bad >> k) & 1)
                        for k, name in enumerate(KEY_RELATIONS)}       # None: not run; True: holds; False: violated
    out["relations_run"], out["relations_bad"] = int(r.relations_run), int(r.relations_bad)
    out["ok"] = bool(r.ok)
    out["ms"] = {"points": r.ms[0], "relation_sums": r.ms[1], "pairings": r.ms[2], "total": r.ms[3]}
    return out


class _ZkeyInfo(C.Structure):      # wsnark_zkey_info_t
    _fields_ = [("n_vars", C.c_uint32), ("n_public", C.c_uint32), ("domain", C.c_uint32), ("n_coeffs", C.c_uint32),
                ("records", C.c_uint64 * 2), ("n_contributions", C.c_uint32), ("reserved", C.c_uint32),
                ("pkey_len", C.c_uint64), ("vk_len", C.c_uint64)]


class _ZkeyReport(C.Structure):    # wsnark_zkey_report_t
    _fields_ = [("records", C.c_uint64 * 2), ("unreduced", C.c_uint64 * 2), ("zero", C.c_uint64 * 2),
                ("sorted", C.c_uint32), ("reserved", C.c_uint32),
                ("h_points", C.c_uint64), ("h_infinity", C.c_uint64), ("h_bad", C.c_uint64), ("h_first_bad", C.c_uint64),
                ("h_first_reason", C.c_uint32), ("reserved2", C.c_uint32), ("ms", C.c_double * 5)]


def _zkey_report_dict(r):
    bad = int(r.h_bad)
    return {"records": (int(r.records[0]), int(r.records[1])), "unreduced": (int(r.unreduced[0]), int(r.unreduced[1])),
            "zero": (int(r.zero[0]), int(r.zero[1])), "sorted": bool(r.sorted),
            "H": {"points": int(r.h_points), "infinity": int(r.h_infinity), "bad": bad,
                  "first_bad": int(r.h_first_bad) if bad else None, "first_reason": KEY_REASONS[r.h_first_reason] if bad else None},
            "ms": {"upload": r.ms[0], "coefficients": r.ms[1], "h_basis": r.ms[2], "download": r.ms[3], "total": r.ms[4]}}


def vk_from_bytes(b, n_public):
    """The inverse of vk_to_bytes: wsnark_groth16_verify's layout -> the reference's verification key object."""
    d = lambda o: str(int.from_bytes(b[o:o + 32], "little"))
    g1 = lambda o: [d(o), d(o + 32), "1"]
    g2 = lambda o: [[d(o), d(o + 32)], [d(o + 64), d(o + 96)], ["1", "0"]]
    return {"protocol": "groth", "nPublic": n_public, "vk_alfa_1": g1(0), "vk_beta_2": g2(64), "vk_gamma_2": g2(192),
            "vk_delta_2": g2(320), "IC": [g1(448 + 64 * i) for i in range(n_public + 1)]}


_ZKEY_OUTPUTS = ("polsA", "polsB", "pointsA", "pointsB1", "pointsB2", "pointsC", "pointsH", "alfa1", "beta1", "delta1", "beta2", "delta2")


class _DeltaReport(C.Structure):   # wsnark_pkey_delta_report_t
    _fields_ = [("points", C.c_uint64 * 2), ("infinity", C.c_uint64 * 2), ("bad", C.c_uint64 * 2), ("first_bad", C.c_uint64 * 2),
                ("first_reason", C.c_uint32 * 2), ("ok", C.c_uint32), ("ms", C.c_double * 3)]


class _DeltaVerdict(C.Structure):  # wsnark_pkey_delta_verdict_t
    _fields_ = [("checks_run", C.c_uint32), ("checks_bad", C.c_uint32), ("ok", C.c_uint32), ("ms", C.c_double * 3)]


class _CircuitVerdict(C.Structure):  # wsnark_pkey_circuit_verdict_t
    _fields_ = [("checks_run", C.c_uint32), ("checks_bad", C.c_uint32), ("ok", C.c_uint32), ("reserved", C.c_uint32), ("ms", C.c_double * 5)]


class _Powers(C.Structure):        # wsnark_powers_t
    _fields_ = [("domain", C.c_uint32), ("tau_g1", C.c_void_p), ("tau_g1_len", C.c_uint64), ("tau_g2", C.c_void_p), ("tau_g2_len", C.c_uint64),
                ("alpha_tau_g1", C.c_void_p), ("alpha_tau_g1_len", C.c_uint64), ("beta_tau_g1", C.c_void_p), ("beta_tau_g1_len", C.c_uint64),
                ("beta_g2", C.c_void_p)]


class _Circuit(C.Structure):       # wsnark_circuit_t
    _fields_ = [("n_vars", C.c_uint32), ("n_public", C.c_uint32), ("domain", C.c_uint32),
                ("polsA", C.c_void_p), ("polsA_len", C.c_uint64), ("polsB", C.c_void_p), ("polsB_len", C.c_uint64),
                ("polsC", C.c_void_p), ("polsC_len", C.c_uint64)]


class _SetupReport(C.Structure):   # wsnark_pkey_setup_report_t
    _fields_ = [("points", C.c_uint64 * 4), ("infinity", C.c_uint64 * 4), ("bad", C.c_uint64 * 4), ("first_bad", C.c_uint64 * 4),
                ("first_reason", C.c_uint32 * 4), ("beta2_reason", C.c_uint32), ("ok", C.c_uint32), ("msm_columns", C.c_uint32),
                ("reserved", C.c_uint32), ("ms", C.c_double * 4)]


POWERS_ARRAYS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1")         # report order (WSNARK_PW_TAU_G1 ..)


def _setup_report_dict(r):
    out = {}
    for k, name in enumerate(POWERS_ARRAYS):
        bad = int(r.bad[k])
        out[name] = {"points": int(r.points[k]), "infinity": int(r.infinity[k]), "bad": bad,
                     "first_bad": int(r.first_bad[k]) if bad else None, "first_reason": KEY_REASONS[r.first_reason[k]] if bad else None}
    out["beta_g2"] = KEY_REASONS[r.beta2_reason]
    out["ok"] = bool(r.ok)
    out["msm_columns"] = int(r.msm_columns)
    out["ms"] = {"transforms": r.ms[0], "column_sums": r.ms[1], "hexps": r.ms[2], "total": r.ms[3]}
    return out


class _PowersReport(C.Structure):  # wsnark_powers_report_t
    _fields_ = [("points", C.c_uint64 * 4), ("infinity", C.c_uint64 * 4), ("bad", C.c_uint64 * 4), ("first_bad", C.c_uint64 * 4),
                ("first_reason", C.c_uint32 * 4), ("beta2_reason", C.c_uint32), ("relations_run", C.c_uint32), ("relations_bad", C.c_uint32),
                ("ok", C.c_uint32), ("ms", C.c_double * 4)]


# bits 0..5 of wsnark_powers_report_t.relations_run / relations_bad
POWERS_RELATIONS = ("generators", "tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")


def _powers_report_dict(r, ms_names):
    out = {}
    for k, name in enumerate(POWERS_ARRAYS):
        bad = int(r.bad[k])
        out[name] = {"points": int(r.points[k]), "infinity": int(r.infinity[k]), "bad": bad,
                     "first_bad": int(r.first_bad[k]) if bad else None, "first_reason": KEY_REASONS[r.first_reason[k]] if bad else None}
    out["beta_g2"] = KEY_REASONS[r.beta2_reason]
    out["relations"] = {name: (None if not (r.relations_run >> k) & 1 else not (r.relations_bad >> k) & 1)
                        for k, name in enumerate(POWERS_RELATIONS)}       # None: not run; True: holds; False: violated
    out["relations_run"], out["relations_bad"] = int(r.relations_run), int(r.relations_bad)
    out["ok"] = bool(r.ok)
    out["ms"] = {name: r.ms[k] for k, name in ms_names}
    return out


def _secret32(v, name):
    if v is None:
        return None
    b = int(v).to_bytes(32, "little") if isinstance(v, int) else bytes(v)
    if len(b) != 32:
        raise ValueError("%s must be 32 bytes" % name)
    return b


def _powers_struct(powers):
    """dict of byte strings -> (wsnark_powers_t, the buffers it points into)"""
    ps, keep = _Powers(powers["domain"]), []
    for name in POWERS_ARRAYS + ("beta_g2",):
        b, n = _ro(powers[name])
        keep.append(b)
        setattr(ps, name, C.cast(b, C.c_void_p))
        if name != "beta_g2":
            setattr(ps, name + "_len", n)
        elif n < 128:
            raise ValueError("beta_g2 must be 128 bytes")
    return ps, keep


def _circuit_struct(circuit):
    cs, keep = _Circuit(circuit["n_vars"], circuit["n_public"], circuit["domain"]), []
    for name in ("polsA", "polsB", "polsC"):
        b, n = _ro(circuit[name])
        keep.append(b)
        setattr(cs, name, C.cast(b, C.c_void_p))
        setattr(cs, name + "_len", n)
    return cs, keep


class _RowsMatrix(C.Structure):    # wsnark_rows_matrix_t
    _fields_ = [("row_ptr", C.c_void_p), ("col", C.c_void_p), ("coef", C.c_void_p)]


class _Rows(C.Structure):          # wsnark_rows_t
    _fields_ = [("n_vars", C.c_uint32), ("n_public", C.c_uint32), ("n_constraints", C.c_uint32), ("domain", C.c_uint32),
                ("A", _RowsMatrix), ("B", _RowsMatrix), ("C", _RowsMatrix)]


class _RowsReport(C.Structure):    # wsnark_rows_report_t
    _fields_ = [("nnz", C.c_uint64 * 3), ("unreduced", C.c_uint64 * 3), ("zero", C.c_uint64 * 3), ("empty_signals", C.c_uint64 * 3),
                ("max_column", C.c_uint64 * 3), ("ms", C.c_double * 4)]


ROWS_PUBLIC_ROWS = 1               # WSNARK_ROWS_PUBLIC_ROWS


def _ro_buffer(b):
    """_ro for anything with the buffer protocol (numpy arrays): C-contiguous, borrowed where it is writable, else copied"""
    if isinstance(b, (bytes, bytearray)):
        return _ro(b)
    mv = memoryview(b)
    if not mv.c_contiguous:
        raise ValueError("expected a C-contiguous buffer")
    if mv.nbytes == 0:
        return C.c_char_p(b"\0"), 0
    if mv.readonly:
        return _ro(mv.tobytes())
    return (C.c_uint8 * mv.nbytes).from_buffer(mv.cast("B")), mv.nbytes


def _rows_struct(rows):
    """wsnark_rows_t over the caller's buffers, their lengths checked against n_constraints and row_ptr's last entry (the C side has
    only the pointers)"""
    nc = int(rows["n_constraints"])
    rs, keep = _Rows(rows["n_vars"], rows["n_public"], nc, int(rows.get("domain") or 0)), []
    for name in ("A", "B", "C"):
        row_ptr, col, coef = rows[name]
        (rp, n_rp), (cl, n_cl), (cf, n_cf) = _ro_buffer(row_ptr), _ro_buffer(col), _ro_buffer(coef)
        if n_rp != 8 * (nc + 1):
            raise ValueError("rows[%r]: row_ptr must hold n_constraints + 1 u64 entries" % name)
        nnz = int.from_bytes(memoryview(row_ptr).cast("B")[8 * nc:8 * nc + 8], "little")
        if n_cl != 4 * nnz or n_cf != 32 * nnz:
            raise ValueError("rows[%r]: col must hold row_ptr[n_constraints] u32 entries and coef as many x 32 bytes" % name)
        keep += [rp, cl, cf]
        setattr(rs, name, _RowsMatrix(C.cast(rp, C.c_void_p), C.cast(cl, C.c_void_p), C.cast(cf, C.c_void_p)))
    return rs, keep


def _rows_report_dict(r):
    return {"nnz": tuple(int(x) for x in r.nnz), "unreduced": tuple(int(x) for x in r.unreduced), "zero": tuple(int(x) for x in r.zero),
            "empty_signals": tuple(int(x) for x in r.empty_signals), "max_column": tuple(int(x) for x in r.max_column),
            "ms": {"upload": r.ms[0], "kernels": r.ms[1], "download": r.ms[2], "total": r.ms[3]}}


DELTA_CHECKS = ("unchanged", "delta1~delta2", "C", "H", "delta_changed")    # bits 0..4 of wsnark_pkey_delta_verdict_t


def _delta_report_dict(r):
    out = {}
    for k, name in enumerate(("C", "H")):
        bad = int(r.bad[k])
        out[name] = {"points": int(r.points[k]), "infinity": int(r.infinity[k]), "bad": bad,
                     "first_bad": int(r.first_bad[k]) if bad else None, "first_reason": KEY_REASONS[r.first_reason[k]] if bad else None}
    out["ok"] = bool(r.ok)
    out["ms"] = {"device": r.ms[0], "host": r.ms[1], "total": r.ms[2]}
    return out


def _delta_verdict_dict(v):
    out = {"checks": {name: (None if not (v.checks_run >> k) & 1 else not (v.checks_bad >> k) & 1) for k, name in enumerate(DELTA_CHECKS)},
           "checks_run": int(v.checks_run), "checks_bad": int(v.checks_bad), "ok": bool(v.ok),
           "ms": {"sums": v.ms[0], "pairings": v.ms[1], "total": v.ms[2]}}
    return out


# bits 0..9 of wsnark_pkey_circuit_verdict_t
CIRCUIT_CHECKS = ("shape_and_streams", "fixed_points", "delta1~delta2", "A", "B1", "B2", "C", "H", "vk_fixed_points", "IC")


def _circuit_verdict_dict(v):
    out = {"checks": {name: (None if not (v.checks_run >> k) & 1 else not (v.checks_bad >> k) & 1) for k, name in enumerate(CIRCUIT_CHECKS)},
           "checks_run": int(v.checks_run), "checks_bad": int(v.checks_bad), "ok": bool(v.ok),
           "ms": {"matrices": v.ms[0], "key_sums": v.ms[1], "powers_sums": v.ms[2], "pairings": v.ms[3], "total": v.ms[4]}}
    return out


class _WitnessReport(C.Structure):  # wsnark_witness_report_t
    _fields_ = [("rows", C.c_uint64), ("bad", C.c_uint64), ("first_bad", C.c_uint64), ("listed", C.c_uint64), ("unreduced", C.c_uint64),
                ("first_unreduced", C.c_uint64), ("one_ok", C.c_uint32), ("ok", C.c_uint32), ("ms", C.c_double * 3)]


def _witness_report_dict(r, rows, values):
    """wsnark_witness_report_t and its two lists as a plain dict; first_bad / first_unreduced stay 2^64 - 1 when there is none"""
    n = int(r.listed)
    val = lambda k: int.from_bytes(bytes(values[32 * k:32 * k + 32]), "little")
    return {"rows": int(r.rows), "bad": int(r.bad), "first_bad": int(r.first_bad), "listed": n, "unreduced": int(r.unreduced),
            "first_unreduced": int(r.first_unreduced), "one_ok": int(r.one_ok), "ok": int(r.ok),
            "ms": {"matrices": r.ms[0], "device": r.ms[1], "total": r.ms[2]},
            "bad_rows": [int(rows[j]) for j in range(n)], "bad_values": [(val(3 * j), val(3 * j + 1), val(3 * j + 2)) for j in range(n)]}


def witness_finding(report):
    """One line naming the first thing check_witness found in a witness that is not ok (None for a good one)."""
    if report["bad"]:
        text = "constraint %d: (A.w)(B.w) != C.w" % report["first_bad"]
        if report["bad_values"] and report["bad_rows"][0] == report["first_bad"]:
            text += ": a=%d, b=%d, c=%d" % report["bad_values"][0]
        return text + (" (%d bad constraints in all)" % report["bad"] if report["bad"] > 1 else "")
    if not report["one_ok"]:
        return "signal 0 is not 1"
    return None if report["ok"] else "public signal >= r (the first unreduced signal is %d)" % report["first_unreduced"]


def _witness_lists(max_rows):
    cap = int(max_rows)
    if cap < 0:
        raise ValueError("max_rows must not be negative")
    return cap, ((C.c_uint64 * cap)() if cap else None), ((C.c_uint8 * (96 * cap))() if cap else None)


class _WitnessVerdict(C.Structure):  # wsnark_witness_verdict_t
    _fields_ = [("bad", C.c_uint64), ("first_bad", C.c_uint64), ("unreduced", C.c_uint64), ("first_unreduced", C.c_uint64),
                ("listed", C.c_uint64), ("one_ok", C.c_uint32), ("ok", C.c_uint32)]


class _WitnessBatchReport(C.Structure):  # wsnark_witness_batch_report_t
    _fields_ = [("count", C.c_uint64), ("rows", C.c_uint64), ("good", C.c_uint64), ("first_not_ok", C.c_uint64), ("chunk", C.c_uint32),
                ("reserved", C.c_uint32), ("ms", C.c_double * 3)]


def _witness_batch_result(verdicts, rows, values, count, cap, rep, report):
    """the verdicts and the two lists of wsnark_circuit_witness_check_batch as a list of check_witness's dicts (without rows and ms,
    which go to `report` with the call's other counts)"""
    if report is not None:
        report.clear()
        report.update({"count": int(rep.count), "rows": int(rep.rows), "good": int(rep.good), "first_not_ok": int(rep.first_not_ok),
                       "chunk": int(rep.chunk), "ms": {"matrices": rep.ms[0], "device": rep.ms[1], "total": rep.ms[2]}})
    vb = bytes(values) if values is not None else b""
    val = lambda k: int.from_bytes(vb[32 * k:32 * k + 32], "little")
    out = []
    for i in range(count):
        v, n, at = verdicts[i], int(verdicts[i].listed), i * cap
        out.append({"bad": int(v.bad), "first_bad": int(v.first_bad), "listed": n, "unreduced": int(v.unreduced),
                    "first_unreduced": int(v.first_unreduced), "one_ok": int(v.one_ok), "ok": int(v.ok),
                    "bad_rows": [int(rows[at + j]) for j in range(n)],
                    "bad_values": [(val(3 * (at + j)), val(3 * (at + j) + 1), val(3 * (at + j) + 2)) for j in range(n)]})
    return out


def _witness_batch_blob(witnesses, stride):
    """a sequence of witness byte strings (each at least `stride` bytes), or ONE bytes-like object holding them back to back, `stride`
    bytes each -> (the witnesses back to back, how many)"""
    if isinstance(witnesses, (bytes, bytearray, memoryview)):
        if stride == 0 or len(witnesses) % stride:
            raise ValueError("witnesses: not a whole number of nVars x 32-byte witnesses")
        return witnesses, len(witnesses) // stride
    ws = [bytes(w) for w in witnesses]
    if any(len(w) < stride for w in ws):
        raise ValueError("a witness is shorter than nVars x 32 bytes")
    return b"".join(w[:stride] for w in ws), len(ws)


def _empty_prove_batch_report():
    return _prove_batch_report_dict(_ProveBatchReport())


def _merge_prove_batch_reports(reports):
    """the reports of several calls as one: counts and times added up, the largest chunk"""
    out = _empty_prove_batch_report()
    for r in reports:
        out["count"] += r["count"]
        out["batched"] += r["batched"]
        out["chunk"] = max(out["chunk"], r["chunk"])
        out["window_bits"] = r["window_bits"]
        for k in out["ms"]:
            out["ms"][k] += r["ms"][k]
    return out


def _pick32(b, which):
    return None if b is None else b"".join(b[32 * i:32 * i + 32] for i in which)


def _good_runs(verdicts):
    """[(first, count)] of every run of consecutive witnesses with ok = 1"""
    runs = []
    for i, v in enumerate(verdicts):
        if v["ok"]:
            if runs and runs[-1][0] + runs[-1][1] == i:
                runs[-1][1] += 1
            else:
                runs.append([i, 1])
    return [tuple(r) for r in runs]


class _ProveBatchReport(C.Structure):  # wsnark_prove_batch_report_t
    _fields_ = [("count", C.c_uint64), ("batched", C.c_uint64), ("chunk", C.c_uint32), ("window_bits", C.c_uint32), ("ms", C.c_double * 5)]


def _prove_batch_report_dict(r):
    return {"count": int(r.count), "batched": int(r.batched), "chunk": int(r.chunk), "window_bits": int(r.window_bits),
            "ms": {"upload": r.ms[0], "calc_h": r.ms[1], "sums": r.ms[2], "assembly": r.ms[3], "total": r.ms[4]}}


def _blinding_array(v, count, name):
    """None, count x 32 bytes, or a sequence of count 32-byte values -> what the C call takes (None: drawn per proof)"""
    if v is None:
        return None
    b = bytes(v) if isinstance(v, (bytes, bytearray, memoryview)) else b"".join(bytes(x) for x in v)
    if len(b) != 32 * count or (not isinstance(v, (bytes, bytearray, memoryview)) and any(len(x) != 32 for x in v)):
        raise ValueError("%s: one 32-byte value per proof" % name)
    return b


def _prove_batch_result(out, rs, count, rep, return_blinding, report):
    if report is not None:
        report.clear()
        report.update(_prove_batch_report_dict(rep))
    b = bytes(out)
    proofs = [proof_from_bytes(b[384 * i:384 * i + 384]) for i in range(count)]
    if not return_blinding:
        return proofs
    rsb = bytes(rs)
    return proofs, [(rsb[64 * i:64 * i + 32], rsb[64 * i + 32:64 * i + 64]) for i in range(count)]


class ResidentCircuit:
    """A circuit's three matrices resident on the device as row-major CSR (wsnark_circuit_load): witnesses are checked against it
    without transposing the record streams again.  Read-only after the load: threads may share one."""

    def __init__(self, lib, circuit=None, rows=None, public_rows=True):
        if (circuit is None) == (rows is None):
            raise ValueError("load_circuit: exactly one of circuit, rows")
        self._lib = lib
        self._h = C.c_void_p()
        if rows is not None:      # wsnark_circuit_load_rows: the CSR built directly, no transposition
            rs, keep = _rows_struct(rows)
            lib.check(lib.c.wsnark_circuit_load_rows(C.byref(rs), ROWS_PUBLIC_ROWS if public_rows else 0, C.byref(self._h)))
        else:
            cs, keep = _circuit_struct(circuit)
            lib.check(lib.c.wsnark_circuit_load(C.byref(cs), C.byref(self._h)))
        inf = self.info()
        self.n_vars, self.n_public, self.domain = inf["n_vars"], inf["n_public"], inf["domain"]

    def info(self):
        """{n_vars, n_public, domain, nnz: (A, B, C), bytes: what the matrices take on the device} (wsnark_circuit_info)"""
        nv, npub, dom, nnz, nb = C.c_uint32(), C.c_uint32(), C.c_uint32(), (C.c_uint64 * 3)(), C.c_uint64()
        self._lib.check(self._lib.c.wsnark_circuit_info(self._h, C.byref(nv), C.byref(npub), C.byref(dom), nnz, C.byref(nb)))
        return {"n_vars": nv.value, "n_public": npub.value, "domain": dom.value, "nnz": tuple(int(x) for x in nnz), "bytes": nb.value}

    def check_witness(self, witness, max_rows=16):
        """Which constraints does `witness` (nVars x 32 bytes plain LE) break?  (wsnark_circuit_witness_check.)  Returns the report
        as a dict -- rows, bad, first_bad, listed, unreduced, first_unreduced (2^64 - 1: none), one_ok, ok, ms -- plus "bad_rows",
        the smallest min(bad, max_rows) bad indices, and "bad_values", (a, b, c) of each as ints.  A bad witness is a result."""
        w, nw = _ro(witness)
        cap, rows, values = _witness_lists(max_rows)
        rep = _WitnessReport()
        self._lib.check(self._lib.c.wsnark_circuit_witness_check(self._h, w, nw, rows, values, cap, C.byref(rep)))
        return _witness_report_dict(rep, rows, values)

    def check_witness_dev(self, d_witness, witness_len, max_rows=16, stream=None):
        """The same for a witness already on the device (a raw device address; stream: the queue it is ready on)."""
        cap, rows, values = _witness_lists(max_rows)
        rep = _WitnessReport()
        self._lib.check(self._lib.c.wsnark_circuit_witness_check_dev(self._h, d_witness, witness_len, rows, values, cap, C.byref(rep), stream))
        return _witness_report_dict(rep, rows, values)

    def check_witnesses(self, witnesses, max_rows=16, report=None):
        """Many witnesses in ONE call (wsnark_circuit_witness_check_batch).  witnesses: a sequence of witness byte strings (each at
        least nVars x 32 bytes), or one bytes-like object holding them back to back, nVars x 32 bytes each.  Returns a list with,
        per witness, the dict check_witness returns for it -- bad, first_bad, listed, unreduced, first_unreduced, one_ok, ok,
        "bad_rows" (at most max_rows), "bad_values" -- without rows and ms.  report: a dict that receives the call's own
        {count, rows, good, first_not_ok (2^64 - 1: none), chunk, ms}.  A bad witness is a result."""
        stride = 32 * self.n_vars
        blob, count = _witness_batch_blob(witnesses, stride)
        return self._check_batch(_ro(blob)[0] if count else None, stride, count, max_rows, report, None, False)

    def check_witnesses_dev(self, d_witnesses, witness_stride, count, max_rows=16, report=None, stream=None):
        """The same for witnesses already on the circuit's device: d_witnesses is a raw device address (16-byte aligned), witness i
        starts witness_stride bytes (a multiple of 16, at least nVars x 32) after witness i - 1; stream: the queue they are ready on."""
        return self._check_batch(d_witnesses, witness_stride, int(count), max_rows, report, stream, True)

    def _check_batch(self, w, stride, count, max_rows, report, stream, dev):
        cap = int(max_rows)
        if cap < 0:
            raise ValueError("max_rows must not be negative")
        rep = _WitnessBatchReport()
        if count == 0:
            rep.rows, rep.first_not_ok = self.domain, (1 << 64) - 1
            return _witness_batch_result(None, None, None, 0, cap, rep, report)
        verdicts = (_WitnessVerdict * count)()
        rows = (C.c_uint64 * (cap * count))() if cap else None
        values = (C.c_uint8 * (96 * cap * count))() if cap else None
        c = self._lib.c
        if dev:
            self._lib.check(c.wsnark_circuit_witness_check_batch_dev(self._h, w, stride, count, verdicts, rows, values, cap, C.byref(rep), stream))
        else:
            self._lib.check(c.wsnark_circuit_witness_check_batch(self._h, w, stride, count, verdicts, rows, values, cap, C.byref(rep)))
        return _witness_batch_result(verdicts, rows, values, count, cap, rep, report)

    def free(self):
        if self._h:
            self._lib.c.wsnark_circuit_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _same_shape(circuit, key):
    if (circuit.n_vars, circuit.n_public, circuit.domain) != (key.n_vars, key.n_public, key.domain):
        raise ValueError("the circuit (nVars %d, nPublic %d, domain %d) is not the key's (%d, %d, %d)"
                         % (circuit.n_vars, circuit.n_public, circuit.domain, key.n_vars, key.n_public, key.domain))


def _require_good(report):
    if not report["ok"]:
        raise ValueError("the witness does not satisfy the circuit: " + witness_finding(report))


def first_finding(report):
    """One line naming the first thing check_key found in a key that is not ok (None for a good key)."""
    for name in KEY_SECTIONS:
        sec = report[name]
        if sec["bad"]:
            return "%d bad point(s) in section %s, the first at index %d: %s" % (sec["bad"], name, sec["first_bad"], sec["first_reason"])
    for name, why in report["fixed"].items():
        if why:
            return "%s: %s" % (name, why)
    for name, holds in report["relations"].items():
        if holds is False:
            return "relation %s does not hold" % name
    return None if report["ok"] else "a requested relation could not be run"


class ProvingKey:
    """Device-resident proving key (wsnark_pkey_load, or wsnark_pkey_load_sections for `sections`)."""

    def __init__(self, lib, data=None, sections=None, shard=None, h_interleave_log=0, wait_tables=True, path=None, zkey=None, zkey_path=None,
                 zkey_report=None):
        """zkey / zkey_path: a snarkjs .zkey as bytes or as a file, straight into the resident key (wsnark_pkey_load_zkey[_file]; whole keys
        only); the handle then carries `vk`, the file's verification key object, and zkey_report (a dict) receives the report.
        path: a key FILE -- proving_key.bin or the WSNARK64 container for keys beyond 4 GiB (wsnark_pkey_load_file: mapped,
        only the share's pages are read); shard / h_interleave_log apply to it as to `sections`.
        shard=(rank, world) with `sections`: only that rank's share of the points becomes resident
        (wsnark_pkey_load_shard; h_interleave_log: the layout of its hExps share, see include/wsnark.h).
        wait_tables: the library builds the fixed-base table rows in the background and serves proofs from the plain sections
        until they are there; this mirror waits for them by default (tests and timing tools want the steady state from the first
        call); wait_tables=False returns as the C call does -- `load_ms` then holds what the caller waited for, and
        `wait_tables()` / `refresh_load_stats()` complete the picture later."""
        self._lib = lib
        self._h = C.c_void_p()
        if shard is not None and sections is None and path is None:
            raise ValueError("a points shard is loaded from sections or from a key file")
        self.vk = None
        if zkey is not None or zkey_path is not None:
            if data is not None or sections is not None or path is not None or shard is not None:
                raise ValueError("a .zkey is loaded as a whole key, and instead of data, sections or path")
            self._load_zkey(lib, zkey, zkey_path, zkey_report)
        elif path is not None:
            rank, world = shard if shard is not None else (0, 1)
            lib.check(lib.c.wsnark_pkey_load_file(os.fsencode(path), rank, world, h_interleave_log, C.byref(self._h)))
        elif sections is not None:
            # dict: n_vars, n_public, domain + byte strings alfa1, beta1, delta1, beta2, delta2, polsA, polsB,
            # pointsA, pointsB1, pointsB2, pointsC, pointsH (64-bit lengths: keys beyond the 4 GiB file format)
            ks = _KeySections(sections["n_vars"], sections["n_public"], sections["domain"])
            keep = []
            for name in ("alfa1", "beta1", "delta1", "beta2", "delta2", "polsA", "polsB", "pointsA", "pointsB1",
                         "pointsB2", "pointsC", "pointsH"):
                b, n = _ro(sections[name])
                keep.append(b)
                setattr(ks, name, C.cast(b, C.c_void_p))
                if name.startswith(("pols", "points")):
                    setattr(ks, name + "_len", n)     # the library checks every section against the header
            if shard is not None:
                lib.check(lib.c.wsnark_pkey_load_shard(C.byref(ks), shard[0], shard[1], h_interleave_log, C.byref(self._h)))
            else:
                lib.check(lib.c.wsnark_pkey_load_sections(C.byref(ks), C.byref(self._h)))
        else:
            b, n = _ro(data)
            lib.check(lib.c.wsnark_pkey_load(b, n, C.byref(self._h)))
        nv, npub, dom = C.c_uint32(), C.c_uint32(), C.c_uint32()
        lib.check(lib.c.wsnark_pkey_info(self._h, C.byref(nv), C.byref(npub), C.byref(dom)))
        self.n_vars, self.n_public, self.domain = nv.value, npub.value, dom.value
        cw, rw, ch, rh, nb = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        lib.check(lib.c.wsnark_pkey_table_info(self._h, C.byref(cw), C.byref(rw), C.byref(ch), C.byref(rh), C.byref(nb)))
        # how the point sections are resident: fixed-base window tables (rows > 1) or the plain sections
        self.table = {"c_w": cw.value, "rows_w": rw.value, "c_h": ch.value, "rows_h": rh.value, "bytes": nb.value}
        if wait_tables:
            lib.check(lib.c.wsnark_pkey_wait_tables(self._h))
        self.refresh_load_stats()
        rk, wd, hl = C.c_uint32(), C.c_uint32(), C.c_uint32()
        lo, nl, nh = C.c_uint64(), C.c_uint64(), C.c_uint64()
        lib.check(lib.c.wsnark_pkey_shard_info(self._h, C.byref(rk), C.byref(wd), C.byref(lo), C.byref(nl), C.byref(nh), C.byref(hl)))
        # which share of the points this handle holds (a whole key: rank 0 of 1, all nVars signals, all hExps)
        self.shard = {"rank": rk.value, "world": wd.value, "first_signal": lo.value, "n_signals": nl.value, "n_hexps": nh.value,
                      "h_interleave_log": hl.value}

    def _load_zkey(self, lib, zkey, zkey_path, report):
        if (zkey is None) == (zkey_path is None):
            raise ValueError("exactly one of zkey, path")
        # the verification key's length from the container and section 2 alone (wsnark_zkey_vk_len*): nothing here maps the file or
        # walks its records -- the library maps a file itself and hands every range back as it is staged
        vk_len, rep = C.c_size_t(), _ZkeyReport()
        if zkey_path is not None:
            fs_path = os.fsencode(zkey_path)
            lib.check(lib.c.wsnark_zkey_vk_len_file(fs_path, C.byref(vk_len)))
            vk = (C.c_uint8 * vk_len.value)()
            lib.check(lib.c.wsnark_pkey_load_zkey_file(fs_path, C.byref(self._h), vk, len(vk), C.byref(rep)))
        else:
            ptr, n = _ro(zkey)
            lib.check(lib.c.wsnark_zkey_vk_len(ptr, n, C.byref(vk_len)))
            vk = (C.c_uint8 * vk_len.value)()
            lib.check(lib.c.wsnark_pkey_load_zkey(ptr, n, C.byref(self._h), vk, len(vk), C.byref(rep)))
        self.vk = vk_from_bytes(bytes(vk), (len(vk) - 448) // 64 - 1)
        if report is not None:
            report.update(_zkey_report_dict(rep))

    def wait_tables(self):
        """Block until the background build of the table rows is over (wsnark_pkey_wait_tables)."""
        self._lib.check(self._lib.c.wsnark_pkey_wait_tables(self._h))
        self.refresh_load_stats()

    def refresh_load_stats(self):
        ms = (C.c_double * 5)()
        self._lib.check(self._lib.c.wsnark_pkey_load_stats(self._h, ms))
        # total = what the load call took; table_build = the background build's own duration (0 while it is still running)
        self.load_ms = {"pols_to_csr": ms[0], "points_h2d": ms[1], "masks_convert": ms[2], "table_build": ms[3], "total": ms[4]}

    def free(self):
        if self._h:
            self._lib.c.wsnark_pkey_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ResidentPoints:
    """A point set kept on the device as fixed-base window tables (wsnark_points_load): sums over the same bases without the
    points' H2D copy, the per-window plans and the host's doubling chain.  g: 1 (G1) or 2 (G2)."""

    def __init__(self, lib, g, points):
        self._lib, self.g = lib, g
        b, nbytes = _ro(points)
        sz = 128 if g == 2 else 64
        if nbytes % sz:
            raise ValueError("points: not a whole number of %d-byte points" % sz)
        self.n = nbytes // sz
        self._h = C.c_void_p()
        lib.check(lib.c.wsnark_points_load(g, b, self.n, C.byref(self._h)))
        gg, n, c, rows, nb = C.c_int(), C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        lib.check(lib.c.wsnark_points_info(self._h, C.byref(gg), C.byref(n), C.byref(c), C.byref(rows), C.byref(nb)))
        self.table = {"c": c.value, "rows": rows.value, "bytes": nb.value}

    def multiexp(self, scalars):
        b, n = _ro(scalars)
        out = (C.c_uint8 * (192 if self.g == 2 else 96))()
        self._lib.check(self._lib.c.wsnark_points_msm(self._h, b, n // 32, out))
        return bytes(out)

    def multiexp_dev(self, d_scalars, n, stream=None):
        out = (C.c_uint8 * (192 if self.g == 2 else 96))()
        self._lib.check(self._lib.c.wsnark_points_msm_dev(self._h, d_scalars, n, out, stream))
        return bytes(out)

    def free(self):
        if self._h:
            self._lib.c.wsnark_points_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _scalar32(v, name):
    """A scalar argument as 32 plain little-endian bytes: an int (any value below 2^256) or 32 bytes."""
    if isinstance(v, int):
        return v.to_bytes(32, "little")
    b = bytes(v)
    if len(b) != 32:
        raise ValueError("%s: expected an int or 32 bytes" % name)
    return b


def _polys(polys):
    """(bytes, len, count) of one polynomial (bytes) or of several of one length (a list of bytes), stored back to back"""
    if isinstance(polys, (bytes, bytearray, memoryview)):
        polys = [polys]
    polys = [bytes(p) for p in polys]
    if not polys or len(polys[0]) % 32 or any(len(p) != len(polys[0]) for p in polys):
        raise ValueError("polynomials: whole 32-byte coefficients, all of one length")
    return b"".join(polys), len(polys[0]) // 32, len(polys)


class KzgSrs:
    """The tau_g1 powers of a transcript resident as a KZG reference string (wsnark_kzg_srs_load): commitments and openings of
    polynomials given as 32-byte plain little-endian coefficients, lowest degree first.  One polynomial (bytes) gives one result, a list
    gives a list."""

    def __init__(self, lib, tau_g1):
        self._lib = lib
        b, nbytes = _ro(tau_g1)
        if nbytes % 64:
            raise ValueError("tau_g1: not a whole number of 64-byte points")
        self.n = nbytes // 64
        self._h = C.c_void_p()
        lib.check(lib.c.wsnark_kzg_srs_load(b, self.n, C.byref(self._h)))

    def info(self):
        n, nb = C.c_uint64(), C.c_uint64()
        self._lib.check(self._lib.c.wsnark_kzg_srs_info(self._h, C.byref(n), C.byref(nb)))
        return {"n": n.value, "bytes": nb.value}

    def commit(self, polys, form=0):
        """form 0: coefficients; form 1: evaluations on the domain of Bn128.fft (a power-of-two length)"""
        blob, ln, count = _polys(polys)
        out = (C.c_uint8 * (64 * count))()
        self._lib.check(self._lib.c.wsnark_kzg_commit(self._h, blob, ln, count, int(form), out))
        out = bytes(out)
        return out if isinstance(polys, (bytes, bytearray, memoryview)) else [out[64 * i:64 * i + 64] for i in range(count)]

    def commit_dev(self, d_polys, length, count=1, form=0, stream=None):
        out = (C.c_uint8 * (64 * count))()
        self._lib.check(self._lib.c.wsnark_kzg_commit_dev(self._h, d_polys, length, count, int(form), out, stream))
        return [bytes(out)[64 * i:64 * i + 64] for i in range(count)]

    def open(self, polys, z, gamma=None):
        """(ys, proof): y_i = f_i(z) for every polynomial and ONE proof for sum_i gamma^i f_i (gamma: the caller's challenge; not
        needed for one polynomial)"""
        blob, ln, count = _polys(polys)
        return self._open(self._lib.c.wsnark_kzg_open, blob, ln, count, z, gamma, ())

    def open_dev(self, d_polys, length, count, z, gamma=None, stream=None):
        return self._open(self._lib.c.wsnark_kzg_open_dev, d_polys, length, count, z, gamma, (stream,))

    def _open(self, fn, polys, ln, count, z, gamma, tail):
        if count > 1 and gamma is None:
            raise ValueError("open: several polynomials need the challenge gamma")
        ys, proof = (C.c_uint8 * (32 * count))(), (C.c_uint8 * 64)()
        self._lib.check(fn(self._h, polys, ln, count, _scalar32(z, "z"), None if gamma is None else _scalar32(gamma, "gamma"), ys, proof, *tail))
        ys = bytes(ys)
        return [ys[32 * i:32 * i + 32] for i in range(count)], bytes(proof)

    def free(self):
        if self._h:
            self._lib.c.wsnark_kzg_srs_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _out_bytes(n):
    """(a new bytes object of n bytes for the library to FILL, its address).  PyBytes_FromStringAndSize(NULL, n) is the C API's own way
    to make a bytes object whose contents the caller writes before anybody else sees it: a key of half a gigabyte then costs neither
    the zero fill of a ctypes array nor the copy out of it.  The object must not be used before the call that fills it has returned."""
    new = C.pythonapi.PyBytes_FromStringAndSize
    new.restype, new.argtypes = C.py_object, [C.c_char_p, C.c_ssize_t]
    b = new(None, max(int(n), 1))
    return b, C.cast(C.c_char_p(b), C.c_void_p)


class _zkey_source:
    """(pointer, length) of a .zkey given as bytes or as a path: the file is mapped read-only for the duration of the block"""

    def __init__(self, zkey, path):
        if (zkey is None) == (path is None):
            raise ValueError("exactly one of zkey, path")
        self.zkey, self.path, self.map, self.file = zkey, path, None, None

    def __enter__(self):
        if self.path is None:
            return _ro(self.zkey)
        import mmap
        self.file = open(self.path, "rb")
        self.map = mmap.mmap(self.file.fileno(), 0, access=mmap.ACCESS_COPY)      # private and writable for ctypes; never written
        self.view = (C.c_uint8 * len(self.map)).from_buffer(self.map)
        return C.c_void_p(C.addressof(self.view)), len(self.map)

    def __exit__(self, *exc):
        if self.map is not None:
            del self.view
            self.map.close()
            self.file.close()
        return False


def _key_sections(sections):
    """dict of byte strings -> (the C struct wsnark_key_sections_t, the buffers it points into)"""
    ks = _KeySections(sections["n_vars"], sections["n_public"], sections["domain"])
    keep = []
    for name in ("alfa1", "beta1", "delta1", "beta2", "delta2", "polsA", "polsB", "pointsA", "pointsB1",
                 "pointsB2", "pointsC", "pointsH"):
        b, n = _ro(sections[name])
        keep.append(b)
        setattr(ks, name, C.cast(b, C.c_void_p))
        if name.startswith(("pols", "points")):
            setattr(ks, name + "_len", n)
    return ks, keep


class GroupKey:
    """One points shard of a proving key per device of a Group (wsnark_group_pkey_load[_sections])."""

    def __init__(self, group, data=None, sections=None, wait_tables=True, path=None):
        self._group, self._lib = group, group._lib
        lib = self._lib
        self._h = C.c_void_p()
        if path is not None:
            lib.check(lib.c.wsnark_group_pkey_load_file(group._h, os.fsencode(path), C.byref(self._h)))
        elif sections is not None:
            ks, keep = _key_sections(sections)
            lib.check(lib.c.wsnark_group_pkey_load_sections(group._h, C.byref(ks), C.byref(self._h)))
        else:
            b, n = _ro(data)
            lib.check(lib.c.wsnark_group_pkey_load(group._h, b, n, C.byref(self._h)))
        nv, npub, dom, world, dist = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int()
        lib.check(lib.c.wsnark_group_pkey_info(self._h, C.byref(nv), C.byref(npub), C.byref(dom), C.byref(world), C.byref(dist)))
        self.n_vars, self.n_public, self.domain, self.world = nv.value, npub.value, dom.value, world.value
        self.distributed_calc_h = bool(dist.value)      # CALC_H on the four-step transform (else complete on every device)
        group._keys.add(self)       # wsnark_group_free deletes every key of the group: terminate() forgets their handles first
        if wait_tables:
            lib.check(lib.c.wsnark_group_pkey_wait_tables(self._h))

    def free(self):
        """Frees the shard on every device.  A no-op once the group is gone: wsnark_group_free has freed the group's keys with it
        (include/wsnark.h: "group_free invalidates every key handle of the group")."""
        if self._h and self._group._h:
            self._lib.c.wsnark_group_pkey_free(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Group:
    """Several GPUs in ONE process (wsnark_group_*, csrc/group.hip): the reference's worker pool (src/bn128.js:173-265, 353-415) with
    GPUs as the workers and the transport inside the library.  devices: HIP ordinals (an ordinal may repeat: two contexts on one GPU)."""

    def __init__(self, lib=None, devices=(0,)):
        self._lib = lib or _lib.load()
        self.devices = [int(d) for d in devices]
        arr = (C.c_int * len(self.devices))(*self.devices)
        self._h = C.c_void_p()
        self._keys = weakref.WeakSet()
        self._lib.check(self._lib.c.wsnark_group_create(arr, len(self.devices), C.byref(self._h)))

    def load_key(self, pkey=None, sections=None, wait_tables=True, path=None):
        return GroupKey(self, data=pkey, sections=sections, wait_tables=wait_tables, path=path)

    def groth16GenProof(self, signals, key, r=None, s=None):
        """src/bn128.js:580-720 over the group: `signals` the witness bytes (host memory), `key` a GroupKey (or the key's bytes)."""
        own = None
        if not isinstance(key, GroupKey):
            own = key = self.load_key(key)
        try:
            b, n = _ro(signals)
            out = (C.c_uint8 * 384)()
            rb = _ro(r)[0] if r is not None else None
            sb = _ro(s)[0] if s is not None else None
            self._lib.check(self._lib.c.wsnark_group_prove(key._h, b, n, rb, sb, out))
            return proof_from_bytes(bytes(out))
        finally:
            if own is not None:
                own.free()

    def last_blinding(self):
        """(r, s) of the group's last proof -- the reference's this._pr / this._ps (src/bn128.js:662-664)."""
        r, s = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
        self._lib.check(self._lib.c.wsnark_group_last_blinding(self._h, r, s))
        return bytes(r), bytes(s)

    def _multiexp(self, g, scalars, points):
        sb, sn = _ro(scalars)
        pb, pn = _ro(points)
        n = sn // 32
        if pn != n * (128 if g else 64):
            raise ValueError("points length does not match scalars")
        out = (C.c_uint8 * (192 if g else 96))()
        fn = self._lib.c.wsnark_group_g2_msm if g else self._lib.c.wsnark_group_g1_msm
        self._lib.check(fn(self._h, sb, pb, n, out))
        return bytes(out)

    def g1_multiexp(self, scalars, points):      # src/bn128.js:353-383
        return self._multiexp(0, scalars, points)

    def g2_multiexp(self, scalars, points):      # src/bn128.js:385-415
        return self._multiexp(1, scalars, points)

    def terminate(self):                         # src/bn128.js:562-566
        if self._h:
            for k in list(self._keys):           # the library frees the group's keys with the group: their handles die here
                k._h = C.c_void_p()
            self._lib.c.wsnark_group_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.terminate()
        except Exception:
            pass


class Bn128:
    """`await buildBn128()` of the reference -> `build()` here (src/bn128.js:173-265)."""

    def __init__(self, lib=None, device=-1):
        self.lib = lib or _lib.load()
        self.device_info = self.lib.init(device)
        self._keys = {}

    # --- src/bn128.js:353-383 ---
    def g1_multiexp(self, scalars, points, shard=None):
        """shard=(rank, world): only the Pippenger windows w % world == rank (a partial sum, see g1_sum)."""
        return self._multiexp(1, scalars, points, shard)

    # --- src/bn128.js:385-415 ---
    def g2_multiexp(self, scalars, points, shard=None):
        return self._multiexp(2, scalars, points, shard)

    def _multiexp(self, g, scalars, points, shard):
        s, ns = _ro(scalars)
        p, np_ = _ro(points)
        n = ns // 32
        sz = 64 if g == 1 else 128
        if np_ < n * sz:
            raise ValueError("points buffer shorter than n*%d bytes" % sz)
        out = (C.c_uint8 * (96 if g == 1 else 192))()
        rank, world = shard or (0, 1)
        fn = self.lib.c.wsnark_g1_msm_windows if g == 1 else self.lib.c.wsnark_g2_msm_windows
        self.lib.check(fn(s, p, n, rank, world, out))
        return bytes(out)

    # --- the gather loop of src/bn128.js:374-382 / 406-414: EC sum of Jacobian partials ---
    def g1_sum(self, partials):
        b, n = _ro(partials)
        out = (C.c_uint8 * 96)()
        self.lib.check(self.lib.c.wsnark_g1_sum(b, n // 96, out))
        return bytes(out)

    def g2_sum(self, partials):
        b, n = _ro(partials)
        out = (C.c_uint8 * 192)()
        self.lib.check(self.lib.c.wsnark_g2_sum(b, n // 192, out))
        return bytes(out)

    # --- device-resident variants (pointers from torch tensors / hipMalloc) ---
    def g1_multiexp_dev(self, d_scalars, d_points, n, stream=None, shard=None):
        out = (C.c_uint8 * 96)()
        rank, world = shard or (0, 1)
        self.lib.check(self.lib.c.wsnark_g1_msm_windows_dev(d_scalars, d_points, n, rank, world, out, stream))
        return bytes(out)

    def g2_multiexp_dev(self, d_scalars, d_points, n, stream=None, shard=None):
        out = (C.c_uint8 * 192)()
        rank, world = shard or (0, 1)
        self.lib.check(self.lib.c.wsnark_g2_msm_windows_dev(d_scalars, d_points, n, rank, world, out, stream))
        return bytes(out)

    def fft_dev(self, d_buf, n, odd=0, inverse=False, stream=None):
        self.lib.check(self.lib.c.wsnark_fr_ntt_dev(d_buf, n, int(odd), 1 if inverse else 0, stream))

    def groth16GenProof_dev(self, d_witness, witness_len, key, r=None, s=None, stream=None, circuit=None):
        """circuit: a ResidentCircuit of the key's shape -- the witness is checked first and a bad one raises ValueError"""
        if circuit is not None:
            _same_shape(circuit, key)
            _require_good(circuit.check_witness_dev(d_witness, witness_len, max_rows=1, stream=stream))
        out = (C.c_uint8 * 384)()
        rb = _ro(r)[0] if r is not None else None
        sb = _ro(s)[0] if s is not None else None
        self.lib.check(self.lib.c.wsnark_groth16_prove_dev(key._h, d_witness, witness_len, rb, sb, out, stream))
        return proof_from_bytes(bytes(out))

    # --- many witnesses of one key (wsnark_groth16_prove_batch; no reference counterpart) ---
    def groth16GenProofBatch(self, witnesses, key, r=None, s=None, return_blinding=False, report=None, circuit=None):
        """witnesses: a sequence of witness.bin byte strings (each at least nVars x 32 bytes), or ONE bytes-like object holding them
        back to back, nVars x 32 bytes each; key: proving_key.bin bytes or a ProvingKey (a whole key).
        r, s: None (drawn from the OS, one independent draw per proof) or one 32-byte value per proof (a sequence, or the
        values back to back).  Returns the list of proofs, proof i being what groth16GenProof(witnesses[i], key, r[i], s[i])
        returns; with return_blinding also the list of (r, s) as used.  report: a dict that receives the call's report
        (count, batched -- 0 when the call looped the single prover --, chunk, window_bits, ms).
        circuit: a ResidentCircuit (load_circuit) whose nVars, nPublic and domain are the key's, else ValueError before anything
        runs.  All witnesses are checked against it in one call (check_witnesses, max_rows=1); those with ok = 1 are proved in
        one call, each with its own r[i], s[i], to the proof the call without circuit= gives for it; a bad witness gives None in
        the list of proofs and in the list of blinding pairs -- no proof is computed and no blinding drawn for it.  The report is
        then that of the good witnesses' call and report["verdicts"] holds every witness's verdict.  None: nothing is checked."""
        pk = key if isinstance(key, ProvingKey) else ProvingKey(self.lib, key)
        try:
            stride = 32 * pk.n_vars
            if circuit is not None:
                _same_shape(circuit, pk)
            blob, count = _witness_batch_blob(witnesses, stride)
            rb, sb = _blinding_array(r, count, "r"), _blinding_array(s, count, "s")
            if circuit is not None:
                verdicts = circuit.check_witnesses(blob, max_rows=1)
                good = [i for i, v in enumerate(verdicts) if v["ok"]]
                inner = {}
                proofs, used = self._prove_batch_host(pk, b"".join(bytes(blob[stride * i:stride * (i + 1)]) for i in good) if len(good) < count else blob,
                                                      stride, len(good), _pick32(rb, good), _pick32(sb, good), inner)
                all_proofs, all_used = [None] * count, [None] * count
                for k, i in enumerate(good):
                    all_proofs[i], all_used[i] = proofs[k], used[k]
                if report is not None:
                    report.clear()
                    report.update(inner or _empty_prove_batch_report())
                    report["verdicts"] = verdicts
                return (all_proofs, all_used) if return_blinding else all_proofs
            proofs, used = self._prove_batch_host(pk, blob, stride, count, rb, sb, report)
            return (proofs, used) if return_blinding else proofs
        finally:
            if pk is not key:
                pk.free()

    def _prove_batch_host(self, pk, blob, stride, count, rb, sb, report):
        if count == 0:
            return [], []
        out, rs, rep = (C.c_uint8 * (384 * count))(), (C.c_uint8 * (64 * count))(), _ProveBatchReport()
        self.lib.check(self.lib.c.wsnark_groth16_prove_batch(pk._h, _ro(blob)[0], stride, count, rb, sb, out, rs, C.byref(rep)))
        return _prove_batch_result(out, rs, count, rep, True, report)

    def groth16GenProofBatch_dev(self, d_witnesses, witness_stride, count, key, r=None, s=None, return_blinding=False, report=None, stream=None,
                                 circuit=None):
        """The same for witnesses already on the key's device: d_witnesses is a raw device address (16-byte aligned), witness i
        starts witness_stride bytes (a multiple of 16, at least nVars x 32) after witness i - 1; stream: the queue they are ready on.
        circuit: as in groth16GenProofBatch; the witnesses stay where they are, so every run of consecutive good witnesses is one
        call, and the report adds those calls up."""
        count = int(count)
        if circuit is not None:
            _same_shape(circuit, key)
        rb, sb = _blinding_array(r, count, "r"), _blinding_array(s, count, "s")
        if count == 0:
            return ([], []) if return_blinding else []
        if circuit is None:
            proofs, used = self._prove_batch_dev(key, d_witnesses, witness_stride, count, rb, sb, report, stream)
            return (proofs, used) if return_blinding else proofs
        verdicts = circuit.check_witnesses_dev(d_witnesses, witness_stride, count, max_rows=1, stream=stream)
        proofs, used, reports = [None] * count, [None] * count, []
        for first, n in _good_runs(verdicts):
            inner, which = {}, range(first, first + n)
            proofs[first:first + n], used[first:first + n] = self._prove_batch_dev(key, int(d_witnesses) + first * int(witness_stride), witness_stride, n,
                                                                                   _pick32(rb, which), _pick32(sb, which), inner, stream)
            reports.append(inner)
        if report is not None:
            report.clear()
            report.update(_merge_prove_batch_reports(reports))
            report["verdicts"] = verdicts
        return (proofs, used) if return_blinding else proofs

    def _prove_batch_dev(self, key, d_witnesses, witness_stride, count, rb, sb, report, stream):
        out, rs, rep = (C.c_uint8 * (384 * count))(), (C.c_uint8 * (64 * count))(), _ProveBatchReport()
        self.lib.check(self.lib.c.wsnark_groth16_prove_batch_dev(key._h, d_witnesses, witness_stride, count, rb, sb, out, rs, C.byref(rep), stream))
        return _prove_batch_result(out, rs, count, rep, True, report)

    # --- src/bn128.js:569-578 (worker CALC_H :126-166) ---
    def calcH(self, signals, polsA, polsB, nSignals, domainSize):
        s, _ = _ro(signals)
        a, la = _ro(polsA)
        b, lb = _ro(polsB)
        out = (C.c_uint8 * (domainSize * 32))()
        self.lib.check(self.lib.c.wsnark_calc_h(s, a, la, b, lb, nSignals, domainSize, out))
        return bytes(out)

    # --- fft_fft / fft_ifft (src/build_fft.js:159-221) on Montgomery Fr elements ---
    def fft(self, data, odd=0, inverse=False):
        b, n = _buf(data)
        self.lib.check(self.lib.c.wsnark_fr_ntt(b, n // 32, int(odd), 1 if inverse else 0))
        return bytes(b)[:n]

    def ifft(self, data, odd=0):
        return self.fft(data, odd, True)

    def toMontgomeryN(self, data):
        b, n = _buf(data)
        self.lib.check(self.lib.c.wsnark_fr_to_montgomery(b, b, n // 32))
        return bytes(b)[:n]

    def fromMontgomeryN(self, data):
        b, n = _buf(data)
        self.lib.check(self.lib.c.wsnark_fr_from_montgomery(b, b, n // 32))
        return bytes(b)[:n]

    # --- synthetic-input helper (no reference counterpart): scalars[i] * generator, affine ---
    def mul_base(self, g, scalars, base=None):
        s, ns = _ro(scalars)
        n = ns // 32
        sz = 64 if g == 1 else 128
        b, _ = _ro(base if base is not None else (G1_GEN if g == 1 else G2_GEN))
        out = (C.c_uint8 * max(n * sz, 1))()
        fn = self.lib.c.wsnark_g1_mul_base_batch if g == 1 else self.lib.c.wsnark_g2_mul_base_batch
        self.lib.check(fn(b, s, n, out))
        return bytes(out)[: n * sz]

    # --- test hook (no reference counterpart): what the MSM's grouping pass and task planner write for a scalar vector ---
    MSM_PLAN_INFO = ("c", "Wall", "W", "w_off", "w_stride", "NB", "nbuckets", "flat", "lmax", "hot_min", "lo_bits", "idx_bits", "nbins",
                     "e32", "once", "partial_slots", "multi_buckets", "tasks", "hot_buckets", "hot_slices", "nvals", "bthr", "n")

    def msm_plan(self, scalars, table_c=0, shard=None, mask=None, capacity=None):
        """wsnark_selftest_msm_plan: {"info": {name: word}, "bstart", "bend", "vals": lists of words, "tasks": [(dst, start, len)],
        "multi": [(bucket, first_partial, ntasks)], "hot": [(bucket, first_partial, ntasks, task_base, rem_index, start, rem,
        slice_base)]}.  shard=(rank, world); mask: n bytes, the plan's masked variant.  capacity: (buckets, vals, tasks) a caller that
        knows the geometry allows for -- one call, and WsnarkError (WSNARK_ERR_SIZE) if the plan is larger; None: the hook's two calls,
        sizes first, then the arrays."""
        s, ns = _ro(scalars)
        n = ns // 32
        m = None
        if mask is not None:
            m, nm = _ro(mask)
            if nm != n:
                raise ValueError("mask: one byte per scalar")
        off, stride = shard or (0, 1)
        fn = self.lib.c.wsnark_selftest_msm_plan
        info = (C.c_uint32 * 24)()
        if capacity is None:
            self.lib.check(fn(s, n, table_c, off, stride, m, info, None, None, 0, None, 0, None, 0, None, 0, None, 0))
            w = dict(zip(self.MSM_PLAN_INFO, info[:]))
            cap = {"b": w["nbuckets"], "v": w["nvals"], "t": w["tasks"], "m": w["multi_buckets"], "h": w["hot_buckets"]}
        else:
            w = None
            cap = {"b": capacity[0], "v": capacity[1], "t": capacity[2], "m": capacity[0], "h": capacity[0]}      # (one record per bucket at most)
        bs, be = (C.c_uint32 * max(cap["b"], 1))(), (C.c_uint32 * max(cap["b"], 1))()
        vals = (C.c_uint32 * max(cap["v"], 1))()
        tasks, multi, hot = (C.c_uint32 * max(3 * cap["t"], 1))(), (C.c_uint32 * max(3 * cap["m"], 1))(), (C.c_uint32 * max(8 * cap["h"], 1))()
        self.lib.check(fn(s, n, table_c, off, stride, m, info, bs, be, cap["b"], vals, cap["v"], tasks, cap["t"], multi, cap["m"], hot, cap["h"]))
        w2 = dict(zip(self.MSM_PLAN_INFO, info[:]))
        if w is not None and w2 != w:
            raise RuntimeError("msm_plan: the two calls disagree on the plan's sizes: %r / %r" % (w, w2))
        rec = lambda a, k, cnt: [tuple(x[i * k:(i + 1) * k]) for x in (a[:k * cnt],) for i in range(cnt)]
        return {"info": w2, "bstart": bs[:w2["nbuckets"]], "bend": be[:w2["nbuckets"]], "vals": vals[:w2["nvals"]],
                "tasks": rec(tasks, 3, w2["tasks"]), "multi": rec(multi, 3, w2["multi_buckets"]), "hot": rec(hot, 8, w2["hot_buckets"])}

    # --- test hook (no reference counterpart): the geometry the MSM's host driver decides for a plan; no device, no init ---
    MSM_GEOMETRY = ("n", "c", "Wall", "W", "w_off", "w_stride", "NB", "nbuckets", "flat", "lmax", "hot_min", "hot_cap",
                    "lo_bits", "idx_bits", "nbins", "bthr", "HB", "tile", "thr", "ps_valid", "e32",
                    "tW", "tNB", "tP", "groups", "m1", "m2", "m", "J1", "J", "logJ", "nsum", "nrows", "reduce")
    MSM_TABLE_C_AUTO = 0xFFFFFFFF

    def msm_geometry(self, n, table_c=0, shard=None):
        """wsnark_selftest_msm_geometry: (rc, {name: word}) for a plan of n pairs -- rc is the library's code (0 = WSNARK_OK), not
        raised: the error rows are part of what a test pins.  table_c: 0, a width, or MSM_TABLE_C_AUTO; shard=(rank, world)."""
        off, stride = shard or (0, 1)
        words = (C.c_uint32 * len(self.MSM_GEOMETRY))()
        rc = self.lib.c.wsnark_selftest_msm_geometry(n, table_c, off, stride, words)
        return rc, dict(zip(self.MSM_GEOMETRY, words[:]))

    # --- test hook (no reference counterpart): the accumulation kernel itself on tasks the caller wrote ---
    def selftest_msm_accumulate(self, g, points, vals, tasks, out=None):
        """wsnark_selftest_msm_accumulate: msm_accumulate over `points` (affine Montgomery bytes, 64 / 128 B each), `vals` (words
        index | sign << 31) and `tasks` [(start, len)]; returns one normalised point (96 / 192 B) per task.  out: a ctypes buffer to
        write into (a test that checks what a failed call leaves).  Bad arguments raise WsnarkError (WSNARK_ERR_ARG) before anything
        is launched."""
        p, np_ = _ro(points)
        sz, osz = (64, 96) if g == 1 else (128, 192)
        nv, nt = len(vals), len(tasks)
        v = (C.c_uint32 * max(nv, 1))(*vals)
        t = (C.c_uint32 * max(2 * nt, 1))(*[w for task in tasks for w in task])
        if out is None:
            out = (C.c_uint8 * max(nt * osz, 1))()
        self.lib.check(self.lib.c.wsnark_selftest_msm_accumulate(g, p, np_ // sz, v, nv, t, nt, out))
        o = bytes(out)
        return [o[i * osz:(i + 1) * osz] for i in range(nt)]

    # --- KZG on a transcript's tau_g1 powers (csrc/kzg.hip; no reference counterpart) ---
    def load_srs(self, tau_g1):
        """tau_g1: tau^k g1, k < n, 64-byte points (a transcript's array or a prefix of it) -> KzgSrs"""
        return KzgSrs(self.lib, tau_g1)

    def kzg_verify(self, g1, g2_pair, commitments, z, ys, proof, gamma=None):
        """e(C - y g1 + z pi, g2) == e(pi, tau g2) for C = sum gamma^i C_i, y = sum gamma^i y_i.  g2_pair: g2 | tau g2 (256 bytes);
        commitments, ys: bytes or lists of 64- / 32-byte items.  Host only."""
        cs = commitments if isinstance(commitments, (bytes, bytearray)) else b"".join(commitments)
        yb = ys if isinstance(ys, (bytes, bytearray)) else b"".join(ys)
        count = len(cs) // 64
        if len(cs) % 64 or len(yb) != 32 * count or len(g1) != 64 or len(g2_pair) != 256 or len(proof) != 64:
            raise ValueError("kzg_verify: 64-byte G1 points, a 256-byte G2 pair, one 32-byte y per commitment")
        if count > 1 and gamma is None:
            raise ValueError("kzg_verify: several commitments need the challenge gamma")
        valid = C.c_int(-1)
        self.lib.check(self.lib.c.wsnark_kzg_verify(bytes(g1), bytes(g2_pair), bytes(cs), count, _scalar32(z, "z"),
                                                    None if gamma is None else _scalar32(gamma, "gamma"), bytes(yb), bytes(proof), C.byref(valid)))
        return valid.value == 1

    def poly_eval(self, polys, z):
        """[f_i(z)] as 32-byte plain values (one value for one polynomial given as bytes)"""
        blob, ln, count = _polys(polys)
        out = (C.c_uint8 * (32 * count))()
        self.lib.check(self.lib.c.wsnark_fr_poly_eval(blob, ln, count, _scalar32(z, "z"), out))
        out = bytes(out)
        return out if isinstance(polys, (bytes, bytearray, memoryview)) else [out[32 * i:32 * i + 32] for i in range(count)]

    def poly_divide(self, poly, z):
        """(q, y): q = (f - f(z)) / (X - z), len - 1 coefficients, and y = f(z)"""
        blob, ln, _ = _polys(poly)
        q, y = (C.c_uint8 * max(32 * (ln - 1), 1))(), (C.c_uint8 * 32)()
        self.lib.check(self.lib.c.wsnark_fr_poly_divide(blob, ln, _scalar32(z, "z"), q, y))
        return bytes(q)[:32 * (ln - 1)], bytes(y)

    def load_points(self, g, points):
        """Make a point set resident as fixed-base tables (no reference counterpart): see ResidentPoints."""
        return ResidentPoints(self.lib, g, points)

    def load_key(self, pkey=None, sections=None, shard=None, h_interleave_log=0, wait_tables=True, path=None, check=False):
        """check=True: audit the key first (check_key: every point, the relations, a fresh seed) and raise WsnarkError naming the
        first finding instead of loading a bad key.  The key's bytes then cross the link twice, audit then load."""
        if check:
            rep = self.check_key(pkey=pkey, sections=sections, path=path)
            if not rep["ok"]:
                raise _lib.WsnarkError(2, "proving key failed its audit: " + first_finding(rep))
        return ProvingKey(self.lib, pkey, sections, shard, h_interleave_log, wait_tables, path)

    def check_key(self, pkey=None, sections=None, path=None, points=True, relations=True, seed=None):
        """The audit of a proving key's bytes on the GPU (wsnark_pkey_check / _check_sections / _check_file; no reference
        counterpart -- snarkjs has `zkey verify`): every point of the five sections and the five fixed points is a reduced,
        on-curve (B2: order-r) point; beta1 ~ beta2, delta1 ~ delta2 and B1 ~ B2 hold the same discrete logs.  Exactly one of
        pkey (proving_key.bin bytes), sections (the dict of load_key) and path (a key file).  seed: 32 bytes for the random
        combination of B1 ~ B2; None draws them from the OS, which is what makes that check sound -- a seed the key's maker
        could know proves nothing.  Returns a dict: "A", "B1", "B2", "C", "H" -> {points, infinity, bad, first_bad,
        first_reason}, fixed, relations (True holds / False violated / None not run), ok, ms.  A bad key is a result, not an
        exception; what load_key rejects (truncated bytes, a bad header) raises WsnarkError as there.  The audit cannot see a
        permutation applied to B1 and B2 alike, nor whether the points belong to the circuit."""
        if (pkey is not None) + (sections is not None) + (path is not None) != 1:
            raise ValueError("check_key: exactly one of pkey, sections, path")
        if seed is not None and len(seed) != 32:
            raise ValueError("seed must be 32 bytes")
        flags = (1 if points else 0) | (2 if relations else 0)
        if not flags:
            raise ValueError("check_key: nothing to check")
        sb = _ro(bytes(seed))[0] if seed is not None else None
        rep = _KeyReport()
        if path is not None:
            rc = self.lib.c.wsnark_pkey_check_file(os.fsencode(path), flags, sb, C.byref(rep))
        elif sections is not None:
            ks, keep = _key_sections(sections)
            rc = self.lib.c.wsnark_pkey_check_sections(C.byref(ks), flags, sb, C.byref(rep))
        else:
            b, n = _ro(pkey)
            rc = self.lib.c.wsnark_pkey_check(b, n, flags, sb, C.byref(rep))
        self.lib.check(rc)
        return _report_dict(rep)

    # --- the phase-2 delta contribution (csrc/pkeydelta.hip; no reference counterpart -- snarkjs: zkey contribute / zkey verify) ---
    def scale_points(self, g, points, k):
        """k * P for every point of `points` (affine Montgomery, 64 bytes each for g = 1, 128 for g = 2; x == 0 is infinity and is
        copied through) and ONE scalar k (an int, or 32 bytes plain LE; reduced mod r): wsnark_g{1,2}_scale_batch."""
        p, nb = _ro(points)
        sz = 64 if g == 1 else 128
        if nb % sz:
            raise ValueError("points: not a whole number of %d-byte points" % sz)
        kb = int(k).to_bytes(32, "little") if isinstance(k, int) else bytes(k)
        if len(kb) != 32:
            raise ValueError("k must be 32 bytes")
        out = (C.c_uint8 * max(nb, 1))()
        fn = self.lib.c.wsnark_g1_scale_batch if g == 1 else self.lib.c.wsnark_g2_scale_batch
        self.lib.check(fn(p, nb // sz, kb, out))
        return bytes(out)[:nb]

    # --- the first key of a ceremony (csrc/pkeysetup.hip; no reference counterpart -- snarkjs: zkey new) ---
    def group_ntt(self, g, points, inverse=False):
        """The transform over group elements: out[i] = sum_k w_n^(ik) P_k (inverse: n^-1 sum_k w_n^(-ik) P_k), natural order, the
        root of fft() -- fft(odd=0) applied to the discrete logarithms.  points: n affine Montgomery points (64 bytes each for
        g = 1, 128 for g = 2; x == 0 is infinity), n a power of two up to 2^24.  A result at infinity is zero bytes:
        wsnark_g{1,2}_ntt."""
        p, nb = _ro(points)
        sz = 64 if g == 1 else 128
        if nb % sz:
            raise ValueError("points: not a whole number of %d-byte points" % sz)
        out = (C.c_uint8 * max(nb, 1))()
        fn = self.lib.c.wsnark_g1_ntt if g == 1 else self.lib.c.wsnark_g2_ntt
        self.lib.check(fn(p, nb // sz, 1 if inverse else 0, out))
        return bytes(out)[:nb]

    def setup_key(self, powers, circuit, pkey=False):
        """The first key of a ceremony: the key of `circuit` under delta = gamma = 1 from a powers-of-tau transcript
        (wsnark_pkey_setup / _setup_pkey), the key contribute_key is then applied to.
        powers: {"domain": n, "tau_g1": 2n points (tau^k G1), "tau_g2": n points, "alpha_tau_g1": n, "beta_tau_g1": n, "beta_g2": 128
        bytes}; circuit: {"n_vars", "n_public", "domain", "polsA", "polsB", "polsC"}, the record streams of a key plus the C
        matrix's (synth.circuit_blobs).  Returns (the key -- a sections dict as load_key takes it, or proving_key.bin bytes with
        pkey=True --, (IC points, gamma2 bytes) for the verification key, report dict: "tau_g1", "tau_g2", "alpha_tau_g1",
        "beta_tau_g1" -> {points, infinity, bad, first_bad, first_reason}, beta_g2, ok, msm_columns, ms).  An unreduced or off-curve
        power is a result: ok is False and the key is None.  Whether the powers ARE powers of one tau is not tested here: that is
        check_powers, the transcript's own audit."""
        ps, keep_p = _powers_struct(powers)
        cs, keep_c = _circuit_struct(circuit)
        nv, npub, dom = circuit["n_vars"], circuit["n_public"], circuit["domain"]
        rep = _SetupReport()
        ic = (C.c_uint8 * max(64 * (npub + 1), 1))()
        if pkey:
            n = C.c_size_t()
            self.lib.check(self.lib.c.wsnark_pkey_setup_size(C.byref(cs), C.byref(n)))
            out = (C.c_uint8 * n.value)()
            self.lib.check(self.lib.c.wsnark_pkey_setup_pkey(C.byref(ps), C.byref(cs), out, n.value, C.byref(n), ic, C.byref(rep)))
            key = bytes(out)[:n.value] if rep.ok else None
        else:
            nC = max(nv - npub - 1, 0)
            sizes = (("pointsA", 64 * nv), ("pointsB1", 64 * nv), ("pointsB2", 128 * nv), ("pointsC", 64 * nC), ("pointsH", 64 * dom),
                     ("alfa1", 64), ("beta1", 64), ("delta1", 64), ("beta2", 128), ("delta2", 128))
            bufs = [(C.c_uint8 * max(sz, 1))() for _, sz in sizes]
            self.lib.check(self.lib.c.wsnark_pkey_setup(C.byref(ps), C.byref(cs), *bufs, ic, C.byref(rep)))
            key = None
            if rep.ok:
                key = {"n_vars": nv, "n_public": npub, "domain": dom, "polsA": bytes(circuit["polsA"]), "polsB": bytes(circuit["polsB"])}
                for (name, sz), b in zip(sizes, bufs):
                    key[name] = bytes(b)[:sz]
        report = _setup_report_dict(rep)
        vk_parts = ([bytes(ic)[64 * i:64 * i + 64] for i in range(npub + 1)], G2_GEN) if rep.ok else None
        return key, vk_parts, report

    # --- powers of tau (csrc/pwtau.hip; no reference counterpart -- snarkjs: powersoftau contribute / powersoftau verify) ---
    def mul_points(self, g, points, scalars):
        """scalars[i] * points[i]: a scalar PER point (affine Montgomery points of 64 bytes for g = 1, 128 for g = 2; x == 0 is
        infinity and is copied through; scalars: 32 bytes plain LE each, any 256-bit value, reduced mod r).  A result at infinity
        is zero bytes: wsnark_g{1,2}_mul_batch -- the third shape beside mul_base (one base) and scale_points (one scalar)."""
        p, nb = _ro(points)
        k, nk = _ro(scalars)
        sz = 64 if g == 1 else 128
        if nb % sz or nk % 32 or nb // sz != nk // 32:
            raise ValueError("mul_points: %d-byte points and 32-byte scalars, as many of one as of the other" % sz)
        out = (C.c_uint8 * max(nb, 1))()
        fn = self.lib.c.wsnark_g1_mul_batch if g == 1 else self.lib.c.wsnark_g2_mul_batch
        self.lib.check(fn(p, k, nb // sz, out))
        return bytes(out)[:nb]

    def contribute_powers(self, powers, tau=None, alpha=None, beta=None):
        """One phase-1 contribution: the transcript of (tau, alpha, beta) becomes the one of (t tau, a alpha, b beta)
        (wsnark_powers_contribute).  powers: the dict of setup_key.  tau, alpha, beta: ints or 32 bytes plain LE, non-zero mod r --
        for tests; None draws the secret from the OS inside the library, which never returns it and wipes it: the production
        case.  Returns (new powers dict, report dict: the four arrays -> {points, infinity, bad, first_bad, first_reason}, beta_g2,
        relations_run, relations_bad (both 0 here), ok, ms).  A bad power or one at infinity is a result: ok is False and the
        returned powers are None."""
        ps, keep = _powers_struct(powers)
        n = powers["domain"]
        secrets = [_secret32(v, name) for v, name in ((tau, "tau"), (alpha, "alpha"), (beta, "beta"))]
        sizes = (("tau_g1", 128 * n), ("tau_g2", 128 * n), ("alpha_tau_g1", 64 * n), ("beta_tau_g1", 64 * n), ("beta_g2", 128))
        bufs = [(C.c_uint8 * max(sz, 1))() for _, sz in sizes]
        rep = _PowersReport()
        self.lib.check(self.lib.c.wsnark_powers_contribute(C.byref(ps), *secrets, *bufs, C.byref(rep)))
        new = None
        if rep.ok:
            new = {"domain": n}
            for (name, sz), b in zip(sizes, bufs):
                new[name] = bytes(b)[:sz]
        return new, _powers_report_dict(rep, ((0, "device"), (1, "host"), (3, "total")))

    def check_powers(self, powers, points=True, relations=True, seed=None):
        """The audit of a powers-of-tau transcript (wsnark_powers_check): every power is a reduced, on-curve point (tau_g2: of order
        r) and none is infinity; tau_g1[0], tau_g2[0] are the generators; both tau arrays are the consecutive powers of ONE tau,
        alpha_tau_g1 and beta_tau_g1 are those powers times one constant each, beta_g2 holds beta_tau_g1[0]'s logarithm.  seed: 32
        bytes for the random combinations; None draws them from the OS, which is what makes them sound -- a seed the
        transcript's author could know proves nothing.  Returns the report dict of contribute_powers with relations (True holds /
        False violated / None not run).  A bad transcript is a result, not an exception.  The audit cannot tell who contributed
        nor whether the transcript descends from an earlier one."""
        if seed is not None and len(seed) != 32:
            raise ValueError("seed must be 32 bytes")
        flags = (1 if points else 0) | (2 if relations else 0)
        if not flags:
            raise ValueError("check_powers: nothing to check")
        ps, keep = _powers_struct(powers)
        sb = _ro(bytes(seed))[0] if seed is not None else None
        rep = _PowersReport()
        self.lib.check(self.lib.c.wsnark_powers_check(C.byref(ps), flags, sb, C.byref(rep)))
        return _powers_report_dict(rep, ((0, "points"), (1, "relation_sums"), (2, "pairings"), (3, "total")))

    def contribute_key(self, pkey=None, sections=None, path=None, out_path=None, d=None):
        """One phase-2 contribution: the same key under delta * d.  Exactly one of pkey (proving_key.bin bytes), sections (the
        dict of load_key) and path (a key file, with out_path: the new file, same format).  d: 32 bytes plain LE (or an int),
        non-zero mod r -- for tests; None draws it from the OS inside the library, which never returns it and wipes it: the
        production case.  Returns (new key in the form it was given -- bytes, a sections dict, or out_path --, report dict with
        "C", "H" -> {points, infinity, bad, first_bad, first_reason}, ok, ms).  A bad input point, or a delta1 / delta2 that fails
        the audit's fixed-point tests, is a result: ok is False and the returned key is None."""
        if (pkey is not None) + (sections is not None) + (path is not None) != 1:
            raise ValueError("contribute_key: exactly one of pkey, sections, path")
        if (path is not None) != (out_path is not None):
            raise ValueError("contribute_key: out_path goes with path")
        db = None
        if d is not None:
            db = int(d).to_bytes(32, "little") if isinstance(d, int) else bytes(d)
            if len(db) != 32:
                raise ValueError("d must be 32 bytes")
        rep = _DeltaReport()
        if path is not None:
            self.lib.check(self.lib.c.wsnark_pkey_contribute_file(os.fsencode(path), os.fsencode(out_path), db, C.byref(rep)))
            new = out_path
        elif sections is not None:
            ks, keep = _key_sections(sections)
            nC = max(sections["n_vars"] - sections["n_public"] - 1, 0)
            oc, oh = (C.c_uint8 * max(nC * 64, 1))(), (C.c_uint8 * (sections["domain"] * 64))()
            d1, d2 = (C.c_uint8 * 64)(), (C.c_uint8 * 128)()
            self.lib.check(self.lib.c.wsnark_pkey_contribute_sections(C.byref(ks), db, oc, oh, d1, d2, C.byref(rep)))
            new = dict(sections, pointsC=bytes(oc)[:nC * 64], pointsH=bytes(oh), delta1=bytes(d1), delta2=bytes(d2))
        else:
            b, n = _ro(pkey)
            out = (C.c_uint8 * max(n, 1))()
            self.lib.check(self.lib.c.wsnark_pkey_contribute(b, n, db, out, n, C.byref(rep)))
            new = bytes(out)[:n]
        report = _delta_report_dict(rep)
        return (new if report["ok"] else None), report

    def verify_contribution(self, old, new, seed=None, check=True):
        """Is `new` exactly `old` under another delta?  (wsnark_pkey_delta_verify*.)  old, new: both proving_key.bin bytes, both
        sections dicts, or both paths of key files.  seed: as check_key's -- None draws it from the OS, which is what makes the two
        random combinations sound.  check=True first audits the new key (check_key) and raises WsnarkError with the audit's message
        if that fails: the relation check itself looks at no single point.  Returns {checks: {unchanged, delta1~delta2, C, H,
        delta_changed -> True holds / False violated / None not run}, checks_run, checks_bad, ok, ms}."""
        if seed is not None and len(seed) != 32:
            raise ValueError("seed must be 32 bytes")
        kind = lambda k: "sections" if isinstance(k, dict) else "path" if isinstance(k, (str, os.PathLike)) else "pkey"
        if kind(old) != kind(new):
            raise ValueError("verify_contribution: old and new must be given in the same form")
        if check:
            rep = self.check_key(**{kind(new): new})
            if not rep["ok"]:
                raise _lib.WsnarkError(2, "proving key failed its audit: " + first_finding(rep))
        sb = _ro(bytes(seed))[0] if seed is not None else None
        v = _DeltaVerdict()
        if kind(old) == "path":
            rc = self.lib.c.wsnark_pkey_delta_verify_file(os.fsencode(old), os.fsencode(new), sb, C.byref(v))
        elif kind(old) == "sections":
            (ko, keep_o), (kn, keep_n) = _key_sections(old), _key_sections(new)
            rc = self.lib.c.wsnark_pkey_delta_verify_sections(C.byref(ko), C.byref(kn), sb, C.byref(v))
        else:
            (bo, no), (bn_, nn) = _ro(old), _ro(new)
            rc = self.lib.c.wsnark_pkey_delta_verify(bo, no, bn_, nn, sb, C.byref(v))
        self.lib.check(rc)
        return _delta_verdict_dict(v)

    # --- a key against its circuit and its powers of tau (csrc/pkeycircuit.hip; no reference counterpart -- snarkjs: zkey verify) ---
    def check_key_circuit(self, powers, circuit, pkey=None, sections=None, path=None, vk=None, seed=None):
        """Is this the key of `circuit` on the transcript `powers`?  (wsnark_pkey_circuit_check*.)  powers, circuit: the dicts of
        setup_key; exactly one of pkey (proving_key.bin bytes), sections (the dict of load_key) and path (a key file).  Works on
        the first key and on a key after any number of contributions: no toxic waste, no group transform -- random combinations of
        the key's points against field transforms of the circuit's row sums.  vk: the verification key, the JSON dict
        groth16Verify takes (or its bytes in wsnark_groth16_verify's layout); with it the IC points and the key's fixed points are
        checked too.  seed: as check_key's -- None draws it from the OS, which is what makes the combinations sound.  Returns
        {checks: {shape_and_streams, fixed_points, delta1~delta2, A, B1, B2, C, H, vk_fixed_points, IC -> True holds / False violated
        / None not run}, checks_run, checks_bad, ok, ms}.  A wrong key is a result, not an exception.  The check looks at no single
        point (check_key and check_powers do), and cannot tell whether the circuit is the intended one nor who contributed."""
        if (pkey is not None) + (sections is not None) + (path is not None) != 1:
            raise ValueError("check_key_circuit: exactly one of pkey, sections, path")
        if seed is not None and len(seed) != 32:
            raise ValueError("seed must be 32 bytes")
        ps, keep_p = _powers_struct(powers)
        cs, keep_c = _circuit_struct(circuit)
        vkb, n_inputs = None, 0
        if vk is not None:
            if isinstance(vk, dict):
                n_inputs = len(vk["IC"]) - 1
                vk = vk_to_bytes(vk, n_inputs)
            else:
                vk = bytes(vk)
                n_inputs = (len(vk) - 448) // 64 - 1
            if n_inputs < 0:
                raise ValueError("vk: no IC point")
            vkb = _ro(vk)[0]
        sb = _ro(bytes(seed))[0] if seed is not None else None
        v = _CircuitVerdict()
        tail = (C.byref(ps), C.byref(cs), vkb, len(vk) if vk is not None else 0, n_inputs, sb, C.byref(v))
        if path is not None:
            rc = self.lib.c.wsnark_pkey_circuit_check_file(os.fsencode(path), *tail)
        elif sections is not None:
            ks, keep = _key_sections(sections)
            rc = self.lib.c.wsnark_pkey_circuit_check_sections(C.byref(ks), *tail)
        else:
            b, n = _ro(pkey)
            rc = self.lib.c.wsnark_pkey_circuit_check(b, n, *tail)
        self.lib.check(rc)
        return _circuit_verdict_dict(v)

    def circuit_row_sums(self, circuit, weights):
        """The building block of check_key_circuit (wsnark_circuit_row_sums): for weights w_j per signal (nVars x 32 bytes plain LE,
        any 256-bit value) the sums sum_j coef_ij w_j of every row i of A, B and C, split into the public columns (j <= nPublic) and
        the private ones.  Returns (public, private): 3 x domain x 32 bytes each, order A, B, C, Montgomery and canonical."""
        cs, keep = _circuit_struct(circuit)
        w, nw = _ro(weights)
        if nw != 32 * circuit["n_vars"]:
            raise ValueError("weights: 32 bytes per signal")
        size = 3 * 32 * circuit["domain"]
        pub, prv = (C.c_uint8 * max(size, 1))(), (C.c_uint8 * max(size, 1))()
        self.lib.check(self.lib.c.wsnark_circuit_row_sums(C.byref(cs), w, pub, prv))
        return bytes(pub)[:size], bytes(prv)[:size]

    # --- a witness against its circuit (csrc/witcheck.hip; no reference counterpart -- snarkjs: wtns check) ---
    def load_circuit(self, circuit=None, rows=None, public_rows=True):
        """circuit: the dict of setup_key ({"n_vars", "n_public", "domain", "polsA", "polsB", "polsC"}); or rows=: the circuit row by
        row, the dict of circuit_from_rows (wsnark_circuit_load_rows: the same handle without a transposition).  Returns a ResidentCircuit:
        .check_witness(witness, max_rows=16), .check_witness_dev(d_witness, witness_len, max_rows=16, stream=None), .check_witnesses(witnesses,
        max_rows=16, report=None), .check_witnesses_dev(d_witnesses, witness_stride, count, ...), .info(), .free()."""
        return ResidentCircuit(self.lib, circuit, rows=rows, public_rows=public_rows)

    # --- a circuit given row by row (csrc/circuitrows.hip; no reference counterpart) ---
    def circuit_from_rows(self, rows, public_rows=True, report=None):
        """The circuit dict of setup_key, check_key_circuit, circuit_row_sums and load_circuit from constraints given ROW BY ROW
        (wsnark_circuit_from_rows).  rows: {"n_vars", "n_public", "n_constraints", "domain" (optional: the smallest power of two that
        holds every row), "A", "B", "C"}, each matrix (row_ptr, col, coef) as buffers (bytes or numpy arrays): row_ptr n_constraints + 1
        u64, col u32 signal indices, coef 32 bytes plain little-endian each, any 256-bit value (formats.rows_from_constraints packs
        them).  public_rows: append the nPublic + 1 input-binding rows old snarkjs and synth.make_circuit use.  Every signal's records
        come out with ascending row, a signal listed twice in a row in the input's order; nothing is merged or dropped.  report: a
        dict that receives {nnz, unreduced, zero, empty_signals, max_column: (A, B, C), ms}."""
        rs, keep = _rows_struct(rows)
        flags = ROWS_PUBLIC_ROWS if public_rows else 0
        dom, lens = C.c_uint32(), (C.c_uint64 * 3)()
        self.lib.check(self.lib.c.wsnark_circuit_from_rows_size(C.byref(rs), flags, C.byref(dom), lens))
        out = [bytearray(max(int(n), 1)) for n in lens]
        ptr = [(C.c_uint8 * len(b)).from_buffer(b) for b in out]
        rep = _RowsReport()
        self.lib.check(self.lib.c.wsnark_circuit_from_rows(C.byref(rs), flags, ptr[0], lens[0], ptr[1], lens[1], ptr[2], lens[2],
                                                          C.byref(dom), C.byref(rep)))
        if report is not None:
            report.update(_rows_report_dict(rep))
        del ptr
        return {"n_vars": rows["n_vars"], "n_public": rows["n_public"], "domain": dom.value,
                "polsA": bytes(out[0][:lens[0]]), "polsB": bytes(out[1][:lens[1]]), "polsC": bytes(out[2][:lens[2]])}

    # --- snarkjs' .zkey / .wtns in and out (csrc/zkey.hip; no reference counterpart) ---
    def h_basis(self, points, to_lagrange=False):
        """A .zkey's H section (the odd Lagrange points of the doubled domain) to the key's hExps (monomial form), or with to_lagrange
        the way back (wsnark_g1_h_basis).  points: n affine Montgomery G1 points of 64 bytes, n a power of two in [2, 2^24]."""
        p, nb = _ro(points)
        if nb % 64:
            raise ValueError("points: not a whole number of 64-byte points")
        out = (C.c_uint8 * max(nb, 1))()
        self.lib.check(self.lib.c.wsnark_g1_h_basis(p, nb // 64, 1 if to_lagrange else 0, out))
        return bytes(out)[:nb]

    def zkey_info(self, zkey=None, path=None):
        """A .zkey's numbers without any device work (wsnark_zkey_info): {n_vars, n_public, domain, n_coeffs, records: (A, B),
        n_contributions, pkey_len, vk_len}."""
        with _zkey_source(zkey, path) as (ptr, n):
            info = _ZkeyInfo()
            self.lib.check(self.lib.c.wsnark_zkey_info(ptr, n, C.byref(info)))
        return {"n_vars": info.n_vars, "n_public": info.n_public, "domain": info.domain, "n_coeffs": info.n_coeffs,
                "records": (int(info.records[0]), int(info.records[1])), "n_contributions": info.n_contributions,
                "pkey_len": int(info.pkey_len), "vk_len": int(info.vk_len)}

    def import_zkey(self, zkey=None, path=None, sections=False, wtns=None, report=None):
        """A snarkjs .zkey (bytes, or path=: the file is mapped and the library reads the mapping) as a key of this library
        (wsnark_zkey_import / _import_sections): returns (proving_key.bin bytes, or with sections=True the sections dict load_key takes
        -- the form for keys past 4 GiB --, the verification key object).  The coefficient records become the two column streams, the H
        section changes basis on the device; sections 3 and 5 - 8 are copied and NOT audited: that is check_key.  wtns: .wtns bytes of a
        witness of the circuit -- a TRIAL PROOF: the witness is proved with the new key and the proof verified against the returned
        verification key; ValueError if it does not verify (a file written under another convention than this reader's fails here,
        not in production).  report: a dict that receives {records, unreduced, zero: (A, B), sorted, H: {...}, ms}."""
        with _zkey_source(zkey, path) as (ptr, n):
            info = _ZkeyInfo()
            self.lib.check(self.lib.c.wsnark_zkey_info(ptr, n, C.byref(info)))
            vk = (C.c_uint8 * int(info.vk_len))()
            rep = _ZkeyReport()
            nv, npub, dom = info.n_vars, info.n_public, info.domain
            if sections:
                sizes = (4 * nv + 36 * int(info.records[0]), 4 * nv + 36 * int(info.records[1]), 64 * nv, 64 * nv, 128 * nv,
                         64 * (nv - npub - 1), 64 * dom, 64, 64, 64, 128, 128)
                bufs = [(C.c_uint8 * max(sz, 1))() for sz in sizes]
                ptrs = (C.c_void_p * 12)(*[C.cast(b, C.c_void_p) for b in bufs])
                caps = (C.c_uint64 * 12)(*sizes)
                self.lib.check(self.lib.c.wsnark_zkey_import_sections(ptr, n, ptrs, caps, vk, len(vk), C.byref(rep)))
                key = {"n_vars": nv, "n_public": npub, "domain": dom}
                for name, sz, b in zip(_ZKEY_OUTPUTS, sizes, bufs):
                    key[name] = bytes(b)[:sz]
            else:
                key, out = _out_bytes(info.pkey_len)
                ln = C.c_size_t()
                self.lib.check(self.lib.c.wsnark_zkey_import(ptr, n, out, len(key), C.byref(ln), vk, len(vk), C.byref(rep)))
                assert ln.value == len(key)
        if report is not None:
            report.update(_zkey_report_dict(rep))
        vk_obj = vk_from_bytes(bytes(vk), npub)
        if wtns is not None:
            from .formats import wtns_to_witness_bin
            wit = wtns_to_witness_bin(wtns)
            handle = self.load_key(sections=key) if sections else self.load_key(key)
            try:
                proof = self.groth16GenProof(wit, handle)
            finally:
                handle.free()
            pub = [int.from_bytes(wit[32 * i:32 * i + 32], "little") for i in range(1, npub + 1)]
            if not self.groth16Verify(vk_obj, pub, proof):
                raise ValueError("import_zkey: the trial proof of the given witness does not verify against the file's verification key -- "
                                 "the file's coefficients or H section follow another convention than this reader's, or the witness is not "
                                 "one of this circuit")
        return key, vk_obj

    def load_zkey(self, zkey=None, path=None, wait_tables=True, wtns=None, report=None):
        """A snarkjs .zkey (bytes, or path=: the library maps the file and never holds it) straight into a resident key
        (wsnark_pkey_load_zkey / _file): returns (ProvingKey, the verification key object).  What load_key(import_zkey(z)[0]) gives,
        without the key's bytes ever existing on the host: the points go up once, H changes basis where it will stay, the coefficient
        records become the prover's row-major matrices directly.  NOT audited, as import_zkey.  wait_tables: see ProvingKey.
        wtns: .wtns bytes of a witness of the circuit -- the TRIAL PROOF of import_zkey on the new handle, verified against the
        returned verification key; ValueError, with the handle freed, if it does not verify.  report: a dict that receives
        {records, unreduced, zero: (A, B), sorted, H: {...}, ms} (ms["download"] is 0: nothing comes back)."""
        key = ProvingKey(self.lib, zkey=zkey, zkey_path=path, wait_tables=wait_tables, zkey_report=report)
        if wtns is not None:
            try:
                from .formats import wtns_to_witness_bin
                wit = wtns_to_witness_bin(wtns)
                proof = self.groth16GenProof(wit, key)
                pub = [int.from_bytes(wit[32 * i:32 * i + 32], "little") for i in range(1, key.n_public + 1)]
                if not self.groth16Verify(key.vk, pub, proof):
                    raise ValueError("load_zkey: the trial proof of the given witness does not verify against the file's verification key "
                                     "-- the file's coefficients or H section follow another convention than this reader's, or the "
                                     "witness is not one of this circuit")
            except Exception:
                key.free()
                raise
        return key, key.vk

    def export_zkey(self, pkey=None, sections=None, vk=None, report=None):
        """A key of this library (proving_key.bin bytes, or sections=) and its verification key object as a snarkjs .zkey
        (wsnark_zkey_export / _export_sections): gamma2 and IC come from vk.  Section 10 holds no contributions and a zero circuit
        hash: provers take the file, `snarkjs zkey verify` does not."""
        if vk is None:
            raise ValueError("export_zkey: vk is required (gamma2 and IC are not part of a proving key)")
        if (pkey is None) == (sections is None):
            raise ValueError("export_zkey: exactly one of pkey, sections")
        if sections is not None:
            ks, keep = _key_sections(sections)
            nv, npub, dom = sections["n_vars"], sections["n_public"], sections["domain"]
            la, lb = len(sections["polsA"]), len(sections["polsB"])
        else:
            p, n = _ro(pkey)
            h = struct.unpack_from("<10I", bytes(pkey[:40]))
            nv, npub, dom, la, lb = h[0], h[1], h[2], h[4] - h[3], h[5] - h[4]
        vkb = vk_to_bytes(vk, npub)
        ln = C.c_size_t()
        self.lib.check(self.lib.c.wsnark_zkey_export_size(nv, npub, dom, max(la - 4 * nv, 0) // 36, max(lb - 4 * nv, 0) // 36, C.byref(ln)))
        z, out = _out_bytes(ln.value)
        rep = _ZkeyReport()
        if sections is not None:
            self.lib.check(self.lib.c.wsnark_zkey_export_sections(C.byref(ks), vkb, len(vkb), npub, out, len(z), C.byref(ln), C.byref(rep)))
        else:
            self.lib.check(self.lib.c.wsnark_zkey_export(p, n, vkb, len(vkb), npub, out, len(z), C.byref(ln), C.byref(rep)))
        assert ln.value == len(z)
        if report is not None:
            report.update(_zkey_report_dict(rep))
        return z

    def check_witness(self, circuit, witness, max_rows=16):
        """Load, check and free in one call (wsnark_witness_check): ResidentCircuit.check_witness's report and lists, with the
        matrices' time in ms["matrices"]."""
        cs, keep = _circuit_struct(circuit)
        w, nw = _ro(witness)
        cap, rows, values = _witness_lists(max_rows)
        rep = _WitnessReport()
        self.lib.check(self.lib.c.wsnark_witness_check(C.byref(cs), w, nw, rows, values, cap, C.byref(rep)))
        return _witness_report_dict(rep, rows, values)

    def key_file_info(self, path):
        """Header of a key file (no GPU work): {n_vars, n_public, domain, file_bytes, format: 'proving_key.bin' | 'WSNARK64'}."""
        nv, npub, dom, nb, fmt = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_int()
        self.lib.check(self.lib.c.wsnark_pkey_file_info(os.fsencode(path), C.byref(nv), C.byref(npub), C.byref(dom), C.byref(nb), C.byref(fmt)))
        return {"n_vars": nv.value, "n_public": npub.value, "domain": dom.value, "file_bytes": nb.value,
                "format": {1: "proving_key.bin", 2: "WSNARK64"}.get(fmt.value, "?")}

    def h_multiexp_dev(self, key, d_h_slice, n, stream=None):
        """The H sum of one rank against the key handle's resident hExps share (wsnark_pkey_h_msm_dev)."""
        out = (C.c_uint8 * 96)()
        self.lib.check(self.lib.c.wsnark_pkey_h_msm_dev(key._h, d_h_slice, n, out, stream))
        return bytes(out)

    # --- multi-GPU proving: per-rank partial sums + host-side finish (include/wsnark.h) ---
    def groth16_prove_partial(self, signals, key, shard=(0, 1), skip_h=False):
        """shard=(rank, world): this rank's 576-byte record of partial sums (windows w % world == rank).
        skip_h: leave CALC_H and the H sum to the caller (WSNARK_PARTIAL_SKIP_H; the H slot is infinity)."""
        w, nw = _ro(signals)
        out = (C.c_uint8 * 576)()
        self.lib.check(self.lib.c.wsnark_groth16_prove_partial(key._h, w, nw, shard[0], shard[1], 1 if skip_h else 0, out))
        return bytes(out)

    def groth16_prove_partial_dev(self, d_witness, witness_len, key, shard=(0, 1), stream=None, skip_h=False):
        out = (C.c_uint8 * 576)()
        self.lib.check(self.lib.c.wsnark_groth16_prove_partial_dev(key._h, d_witness, witness_len, shard[0], shard[1],
                                                                    1 if skip_h else 0, out, stream))
        return bytes(out)

    def last_blinding(self):
        """(r, s) of the last proof assembled by this thread -- the reference's this._pr / this._ps (src/bn128.js:662-664)."""
        r, s = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
        self.lib.check(self.lib.c.wsnark_last_blinding(r, s))
        return bytes(r), bytes(s)

    def groth16_prove_finish(self, key, partials, r=None, s=None):
        p, n = _ro(partials)
        out = (C.c_uint8 * 384)()
        rb = _ro(r)[0] if r is not None else None
        sb = _ro(s)[0] if s is not None else None
        self.lib.check(self.lib.c.wsnark_groth16_prove_finish(key._h, p, n // 576, rb, sb, out))
        return proof_from_bytes(bytes(out))

    # --- src/bn128.js:580-720 ---
    def groth16GenProof(self, signals, pkey, r=None, s=None, circuit=None):
        """signals: witness.bin bytes; pkey: proving_key.bin bytes, the bytes of a snarkjs .zkey (they begin with b"zkey"), or a
        ProvingKey.  r, s: optional 32-byte blinding values (the reference draws them with
        crypto.randomBytes, src/bn128.js:642-661). Returns {pi_a, pi_b, pi_c} of decimal strings.
        circuit: a ResidentCircuit (load_circuit) whose nVars, nPublic and domain are the key's, else ValueError before anything
        runs.  The witness is checked against it first; one that breaks a constraint raises ValueError naming the first bad
        constraint with its a, b, c, and no proof is computed.  None: nothing is checked, as in the reference."""
        if isinstance(pkey, ProvingKey):
            key = pkey
        elif bytes(pkey[:4]) == b"zkey":      # a snarkjs .zkey: straight into a resident key (load_zkey)
            key = ProvingKey(self.lib, zkey=pkey)
        else:
            key = ProvingKey(self.lib, pkey)
        w, nw = _ro(signals)
        out = (C.c_uint8 * 384)()
        rb = _ro(r)[0] if r is not None else None
        sb = _ro(s)[0] if s is not None else None
        if (r is not None and len(r) != 32) or (s is not None and len(s) != 32):
            raise ValueError("r and s must be 32 bytes")
        if circuit is not None:
            try:
                _same_shape(circuit, key)
                _require_good(circuit.check_witness(signals, max_rows=1))
            except Exception:
                if key is not pkey:
                    key.free()
                raise
        self.lib.check(self.lib.c.wsnark_groth16_prove(key._h, w, nw, rb, sb, out))
        if key is not pkey:
            key.free()
        return proof_from_bytes(bytes(out))

    def groth16GenProof_hostptr(self, h_witness, witness_len, key, r=None, s=None):
        """The same call with the witness given as a raw HOST address (e.g. a pinned torch tensor's data_ptr(): a source the
        runtime already knows as pinned is DMA'd in place, chunk by chunk, without the staging copy)."""
        out = (C.c_uint8 * 384)()
        rb = _ro(r)[0] if r is not None else None
        sb = _ro(s)[0] if s is not None else None
        self.lib.check(self.lib.c.wsnark_groth16_prove(key._h, C.c_void_p(h_witness), witness_len, rb, sb, out))
        return proof_from_bytes(bytes(out))

    # --- src/bn128.js:722-791 ---
    def groth16Verify(self, verificationKey, input, proof):
        """verificationKey: the snarkjs "groth" verification_key.json object (vk_alfa_1, vk_beta_2, vk_gamma_2, vk_delta_2,
        IC; vk_alfabeta_12 is not needed); input: public signals (decimal strings / ints, a single value is wrapped like
        the reference does, :724-728); proof: {pi_a, pi_b, pi_c} of decimal strings.  Returns True / False."""
        return groth16_verify(self.lib, verificationKey, input, proof)

    def groth16VerifyBatch(self, verificationKey, inputs, proofs, return_status=False):
        """Many proofs against ONE verification key, on the GPU (wsnark_groth16_verify_batch; no reference counterpart).
        inputs: one list of public signals per proof, all of one length (ValueError otherwise); proofs: a list of
        {pi_a, pi_b, pi_c}.  Returns a list of bool, proof by proof what groth16Verify says (a proof with an unreduced
        coordinate, which the single call raises on, reads as False), or with return_status the raw statuses
        (1 valid, 0 invalid, 2 malformed)."""
        return groth16_verify_batch(self.lib, verificationKey, inputs, proofs, return_status)

    # --- compressed points and 128-byte proofs (csrc/pointcodec.hip; include/wsnark.h has both encodings byte by byte) ---
    def compress_points(self, g, points, encoding):
        """points: affine Montgomery points (64 bytes each for g = 1, 128 for g = 2; x == 0 is infinity) -> (32 / 64 bytes per point,
        status list: 0 ok, 1 a coordinate >= q -- that record is zero).  encoding: "le" (ark-serialize's compressed mode) or "be"
        (gnark-crypto's marshal).  The curve equation is not tested: check_key does that.  wsnark_g{1,2}_compress."""
        return _points_codec(self.lib, g, True, points, encoding, False)

    def decompress_points(self, g, data, encoding, subgroup=False):
        """data: 32 / 64 bytes per point -> (affine Montgomery points, infinity and every bad point as zero bytes; status list: 0 ok,
        1 malformed, 2 no point with that x, 3 outside the order-r subgroup -- g = 2 with subgroup=True only).
        wsnark_g{1,2}_decompress."""
        return _points_codec(self.lib, g, False, data, encoding, subgroup)

    def compress_proofs(self, proofs, encoding):
        """proofs: a list of {pi_a, pi_b, pi_c} as the provers return them -> (128 bytes per proof: A | B | C, status list: 1 written,
        2 a number of that proof is not a reduced field element -- a zero record).  wsnark_proof_compress."""
        proofs = list(proofs)
        for pr in proofs:
            if any(not 0 <= int(v) < 1 << 256 for v in list(pr["pi_a"]) + [x for pair in pr["pi_b"] for x in pair] + list(pr["pi_c"])):
                raise ValueError("a proof's numbers must lie in [0, 2^256)")
        out, st = _proofs_codec(self.lib, True, b"".join(proof_to_bytes(pr) for pr in proofs), encoding)
        return out, st

    def decompress_proofs(self, data, encoding):
        """data: 128 bytes per proof -> (a list of {pi_a, pi_b, pi_c} with z = 1, None where the status is not 1; status list: 1 written,
        2 a malformed point, 0 a point without a y or encoded as infinity).  wsnark_proof_decompress."""
        out, st = _proofs_codec(self.lib, False, data, encoding)
        return [proof_from_bytes(out[384 * i:384 * i + 384]) if v == 1 else None for i, v in enumerate(st)], st

    def groth16VerifyBatchCompressed(self, verificationKey, inputs, proof_bytes, encoding, return_status=False):
        """groth16VerifyBatch on 128-byte proofs (wsnark_groth16_verify_batch_compressed): they are decompressed on the GPU and verified
        there.  proof_bytes: 128 bytes per proof, or a list of 128-byte strings.  Proof by proof what groth16VerifyBatch says about the
        decompressed proof; a malformed point is status 2, a point without a y or at infinity status 0."""
        return groth16_verify_batch_compressed(self.lib, verificationKey, inputs, proof_bytes, encoding, return_status)

    def terminate(self):  # src/bn128.js:562-566
        self.lib.shutdown()


def proof_from_bytes(b):
    """bin2g1 / bin2g2 of the reference (src/bn128.js:319-351, 714-718)."""
    v = [str(int.from_bytes(b[i:i + 32], "little")) for i in range(0, 384, 32)]
    return {"pi_a": v[0:3], "pi_b": [v[3:5], v[5:7], v[7:9]], "pi_c": v[9:12]}


def proof_to_bytes(proof):
    """Inverse of proof_from_bytes: {pi_a, pi_b, pi_c} of decimal strings -> the 384 bytes wsnark_groth16_prove writes."""
    le = lambda v: int(v).to_bytes(32, "little")
    a, b, c = proof["pi_a"], proof["pi_b"], proof["pi_c"]
    return (b"".join(le(x) for x in a) + b"".join(le(x) for pair in b for x in pair) + b"".join(le(x) for x in c))


def vk_to_bytes(vk, n_inputs):
    le = lambda v: int(v).to_bytes(32, "little")
    g1 = lambda p: le(p[0]) + le(p[1])
    g2 = lambda p: le(p[0][0]) + le(p[0][1]) + le(p[1][0]) + le(p[1][1])
    if len(vk["IC"]) < n_inputs + 1:
        raise ValueError("verification key has %d IC points, %d inputs given" % (len(vk["IC"]), n_inputs))
    return (g1(vk["vk_alfa_1"]) + g2(vk["vk_beta_2"]) + g2(vk["vk_gamma_2"]) + g2(vk["vk_delta_2"])
            + b"".join(g1(p) for p in vk["IC"][:n_inputs + 1]))


def groth16_verify(lib, verificationKey, input, proof):
    """Bn128.groth16Verify (src/bn128.js:722-791) over wsnark_groth16_verify: host arithmetic, no GPU needed."""
    if input is None:
        input = []
    elif not isinstance(input, (list, tuple)):
        input = [input]
    vals = [int(x) for x in input]
    if any(v < 0 or v >= 1 << 256 for v in vals):
        return False
    vkb = vk_to_bytes(verificationKey, len(vals))
    inp = b"".join(v.to_bytes(32, "little") for v in vals)
    valid = C.c_int(0)
    lib.check(lib.c.wsnark_groth16_verify(vkb, len(vkb), inp if vals else None, len(vals), proof_to_bytes(proof), C.byref(valid)))
    return bool(valid.value)


def groth16_verify_batch(lib, verificationKey, inputs, proofs, return_status=False):
    """Bn128.groth16VerifyBatch over wsnark_groth16_verify_batch: needs an initialised library (a GPU)."""
    inputs = [list(x) if isinstance(x, (list, tuple)) else ([] if x is None else [x]) for x in inputs]
    proofs = list(proofs)
    if len(inputs) != len(proofs):
        raise ValueError("%d input vectors for %d proofs" % (len(inputs), len(proofs)))
    if not proofs:
        return []
    n_in = len(inputs[0])
    if any(len(x) != n_in for x in inputs):
        raise ValueError("all proofs of a batch share the key, so every input vector must have %d entries" % n_in)
    vkb = vk_to_bytes(verificationKey, n_in)
    vals = [[int(v) for v in x] for x in inputs]
    # an input outside [0, 2^256) makes that proof invalid without reaching the library, as in groth16_verify
    keep = [i for i, x in enumerate(vals) if all(0 <= v < 1 << 256 for v in x)]
    status = [0] * len(proofs)
    if keep:
        inp = b"".join(v.to_bytes(32, "little") for i in keep for v in vals[i])
        prf = b"".join(proof_to_bytes(proofs[i]) for i in keep)
        st = (C.c_uint8 * len(keep))()
        lib.check(lib.c.wsnark_groth16_verify_batch(vkb, len(vkb), inp if n_in else None, n_in, prf, len(keep), st))
        for i, v in zip(keep, st):
            status[i] = int(v)
    return status if return_status else [v == 1 for v in status]


ENCODINGS = {"le": 1, "be": 2}      # WSNARK_ENC_LE, WSNARK_ENC_BE


def _encoding(name):
    if name not in ENCODINGS:
        raise ValueError("encoding must be one of %s" % ", ".join(repr(k) for k in ENCODINGS))
    return ENCODINGS[name]


def _points_codec(lib, g, compress, data, encoding, subgroup):
    if g not in (1, 2):
        raise ValueError("g must be 1 or 2")
    enc = _encoding(encoding)
    b, nb = _ro(data)
    in_sz, out_sz = (64 * g, 32 * g) if compress else (32 * g, 64 * g)
    if nb % in_sz:
        raise ValueError("expected a whole number of %d-byte records" % in_sz)
    n = nb // in_sz
    out, st, bad = (C.c_uint8 * max(n * out_sz, 1))(), (C.c_uint8 * max(n, 1))(), C.c_uint64(0)
    if compress:
        fn = lib.c.wsnark_g1_compress if g == 1 else lib.c.wsnark_g2_compress
        lib.check(fn(b, n, enc, out, st, C.byref(bad)))
    else:
        fn = lib.c.wsnark_g1_decompress if g == 1 else lib.c.wsnark_g2_decompress
        lib.check(fn(b, n, enc, 1 if subgroup else 0, out, st, C.byref(bad)))
    return bytes(out)[:n * out_sz], list(st)[:n]


def _proofs_codec(lib, compress, data, encoding):
    enc = _encoding(encoding)
    if isinstance(data, (list, tuple)):
        data = b"".join(data)
    b, nb = _ro(data)
    in_sz, out_sz = (384, 128) if compress else (128, 384)
    if nb % in_sz:
        raise ValueError("expected a whole number of %d-byte proofs" % in_sz)
    n = nb // in_sz
    out, st = (C.c_uint8 * max(n * out_sz, 1))(), (C.c_uint8 * max(n, 1))()
    lib.check((lib.c.wsnark_proof_compress if compress else lib.c.wsnark_proof_decompress)(b, n, enc, out, st))
    return bytes(out)[:n * out_sz], list(st)[:n]


def groth16_verify_batch_compressed(lib, verificationKey, inputs, proof_bytes, encoding, return_status=False):
    """Bn128.groth16VerifyBatchCompressed over wsnark_groth16_verify_batch_compressed: needs an initialised library (a GPU)."""
    enc = _encoding(encoding)
    if isinstance(proof_bytes, (list, tuple)):
        proof_bytes = b"".join(proof_bytes)
    proof_bytes = bytes(proof_bytes)
    if len(proof_bytes) % 128:
        raise ValueError("expected a whole number of 128-byte proofs")
    n = len(proof_bytes) // 128
    inputs = [list(x) if isinstance(x, (list, tuple)) else ([] if x is None else [x]) for x in inputs]
    if len(inputs) != n:
        raise ValueError("%d input vectors for %d proofs" % (len(inputs), n))
    if not n:
        return []
    n_in = len(inputs[0])
    if any(len(x) != n_in for x in inputs):
        raise ValueError("all proofs of a batch share the key, so every input vector must have %d entries" % n_in)
    vkb = vk_to_bytes(verificationKey, n_in)
    vals = [[int(v) for v in x] for x in inputs]
    # an input outside [0, 2^256) makes that proof invalid without reaching the library, as in groth16_verify_batch
    keep = [i for i, x in enumerate(vals) if all(0 <= v < 1 << 256 for v in x)]
    status = [0] * n
    if keep:
        inp = b"".join(v.to_bytes(32, "little") for i in keep for v in vals[i])
        prf = b"".join(proof_bytes[128 * i:128 * i + 128] for i in keep)
        st = (C.c_uint8 * len(keep))()
        lib.check(lib.c.wsnark_groth16_verify_batch_compressed(vkb, len(vkb), inp if n_in else None, n_in, prf, len(keep), enc, st))
        for i, v in zip(keep, st):
            status[i] = int(v)
    return status if return_status else [v == 1 for v in status]


def build(lib=None, device=-1):
    return Bn128(lib, device)


_singleton = None


def groth16GenProof(witness, provingKey, cb=None):
    """main_bn128.js:26-39 (window.groth16GenProof): optional node-style callback."""
    global _singleton
    try:
        if _singleton is None:
            _singleton = build()
        proof = _singleton.groth16GenProof(witness, provingKey)
    except Exception as e:  # noqa: BLE001 - mirrors cb(err)
        if cb:
            return cb(e, None)
        raise
    return cb(None, proof) if cb else proof


genZKSnarkProof = groth16GenProof  # README.md:28-30 name
