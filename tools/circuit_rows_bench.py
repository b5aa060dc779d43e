#!/usr/bin/env python3
"""Circuits in row form on the GPU (needs the GPU; bench.py is not involved).  Prints ONE JSON line; on ONE circuit of the native
generator's "columns" family (csrc/synth.hip, style 0) at log2(domain) = --log, all three matrices, all in the SAME process:
  from_rows           wsnark_circuit_from_rows: the report's own ms (upload, kernels, download, whole call) and the host clock around
                      Bn128.circuit_from_rows, medians of --reps calls after a warm-up
  load_rows           wsnark_circuit_load_rows (load_circuit(rows=...) and free), host clock
  load_circuit        wsnark_circuit_load on the same circuit's streams: the OPPOSITE transposition over the same records
  kernels             per-kernel times from wsnark_timing_report: rows_prepare, rows_hist, rows_scan, rows_scatter, rows_header,
                      rows_emit of one from_rows call beside csr_count + csr_scan + csr_fill of one load_circuit call (the same three
                      matrices).  ratio_transpose = the first sum / the second; the budget for it is 2 (a stable order costs at least
                      one more pass over the entries than an atomic cursor fill).
  ratio_load_rows_to_load_circuit   expected <= 1: the direct load skips the transposition
  from_rows_hot_column   the same call on the same circuit with signal 0 added to EVERY row of A (a column of domain + its own records)
The rows are derived on the host from the generator's own streams (numpy: every record's row and signal, a stable sort by row), the
coefficients taken out of Montgomery form on the device (fromMontgomeryN).  The generator exports only A and B; its C is "row c holds
1 x its output variable" (tools/witness_check_bench.py: pols_c).  The tool asserts that the streams that come back are the
generator's with every column's records sorted by row, byte for byte, and that both resident circuits accept the generator's witness.
    python tools/circuit_rows_bench.py [--log 20] [--reps 5] [--out profiles/circuit_rows_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROWS_KERNELS = ("rows_prepare", "rows_hist", "rows_scan", "rows_scatter", "rows_header", "rows_emit")
CSR_KERNELS = ("csr_count", "csr_scan", "csr_fill")


def records_of(pols, n_vars):
    """(signal, row, byte offset) of every record of a stream, in stream order, and the offsets of the headers"""
    import numpy as np
    buf = np.frombuffer(pols, dtype=np.uint8)
    counts = np.empty(n_vars, dtype=np.int64)
    starts = np.empty(n_vars, dtype=np.int64)
    pos = 0
    for s in range(n_vars):      # the one sequential walk: a header says where the next one is
        c = int.from_bytes(pols[pos:pos + 4], "little")
        counts[s], starts[s] = c, pos
        pos += 4 + 36 * c
    assert pos == len(pols)
    sig = np.repeat(np.arange(n_vars, dtype=np.int64), counts)
    first = np.cumsum(counts) - counts
    k = np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(first, counts)
    off = np.repeat(starts, counts) + 4 + 36 * k
    row = buf[off[:, None] + np.arange(4)].copy().view("<u4")[:, 0].astype(np.int64)
    return buf, sig, row, off


def rows_matrix(bn, pols, n_vars, n_rows):
    """(row_ptr, col, coef) of a stream, and the stream with every column's records sorted by row (what from_rows must give back)"""
    import numpy as np
    buf, sig, row, off = records_of(pols, n_vars)
    mont = buf[off[:, None] + 4 + np.arange(32)]                    # records x 32 bytes, Montgomery
    order = np.lexsort((sig, row))                                  # by row, then by signal: one row's terms by ascending signal
    plain = np.frombuffer(bn.fromMontgomeryN(mont[order].tobytes()), dtype=np.uint8).copy() if len(order) else np.zeros(0, np.uint8)
    row_ptr = np.zeros(n_rows + 1, dtype="<u8")
    np.cumsum(np.bincount(row, minlength=n_rows), out=row_ptr[1:])
    want = buf.copy()
    by_col = np.lexsort((row, sig))                                 # by signal, then by row (stable): the contract's order
    want[(off[:, None] + np.arange(36)).ravel()] = buf[off[by_col][:, None] + np.arange(36)].ravel()
    return (row_ptr, sig[order].astype("<u4"), plain), want.tobytes()


def timed(fn, reps):
    """(median ms by the host clock, every call's ms, every call's result) of `reps` calls after one warm-up"""
    fn()
    ts, outs = [], []
    for _ in range(max(reps, 1)):
        t = time.perf_counter()
        outs.append(fn())
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), ts, outs


def read_clock():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        lines = [ln.strip() for ln in out.splitlines() if "sclk" in ln.lower()]
        return lines[0] if lines else "not read"
    except Exception:      # noqa: BLE001
        return "not read"


def run(bn, log, reps, say=lambda *x: None):
    from wasmsnark_amd import synth
    from witness_check_bench import pols_c
    lib = bn.lib
    nc = synth.NativeCircuit(lib, log, n_public=2, seed=log, style="columns")
    sec, _ = nc.build_sections()
    circuit = {"n_vars": nc.n_vars, "n_public": nc.n_public, "domain": nc.domain, "polsA": bytes(sec["polsA"]), "polsB": bytes(sec["polsB"]),
               "polsC": pols_c(nc.n_vars, nc.n_public)}
    good = nc.witness_bin()
    t = time.perf_counter()
    rows = {"n_vars": nc.n_vars, "n_public": nc.n_public, "n_constraints": nc.domain, "domain": nc.domain}
    want = {}
    for m in "ABC":
        rows[m], want["pols" + m] = rows_matrix(bn, circuit["pols" + m], nc.n_vars, nc.domain)
    say("rows derived on the host", time.perf_counter() - t, "s")
    row = {"n_vars": nc.n_vars, "n_public": nc.n_public, "domain": nc.domain, "reps": reps, "nnz": [int(rows[m][0][-1]) for m in "ABC"]}

    reports = []

    def from_rows():
        rep = {}
        out = bn.circuit_from_rows(rows, public_rows=False, report=rep)
        reports.append(rep)
        return out

    ms, all_ms, outs = timed(from_rows, reps)
    ok = all(outs[-1][p] == want[p] for p in want) and outs[-1]["domain"] == nc.domain
    med = lambda k: statistics.median(r["ms"][k] for r in reports[1:])
    row["from_rows"] = {"ms_host_clock": ms, "all_ms": all_ms, "report_ms": {k: med(k) for k in ("upload", "kernels", "download", "total")},
                        "max_column": list(reports[-1]["max_column"]), "empty_signals": list(reports[-1]["empty_signals"])}
    say("from_rows", ms, row["from_rows"]["report_ms"], "bytes equal:", ok)

    # THE HOT COLUMN: the same circuit with signal 0 (the constant) added to EVERY row of A, as a real circuit has it
    import numpy as np
    rp, col, coef = rows["A"]
    at = rp[:-1].astype(np.int64)
    one = np.zeros(32, dtype=np.uint8)
    one[0] = 1
    hot = dict(rows, A=((rp + np.arange(len(rp), dtype=rp.dtype)).astype("<u8"), np.insert(col, at, 0).astype("<u4"),
                        np.insert(coef.reshape(-1, 32), at, one, axis=0).reshape(-1).copy()))
    hot_reports = []

    def from_rows_hot():
        rep = {}
        out = bn.circuit_from_rows(hot, public_rows=False, report=rep)
        hot_reports.append(rep)
        return out

    _, _, hot_outs = timed(from_rows_hot, reps)
    ok = ok and hot_outs[-1]["polsB"] == want["polsB"] and len(hot_outs[-1]["polsA"]) == len(want["polsA"]) + 36 * nc.domain
    first = int.from_bytes(want["polsA"][:4], "little")
    ok = ok and int.from_bytes(hot_outs[-1]["polsA"][:4], "little") == first + nc.domain == hot_reports[-1]["max_column"][0]
    row["from_rows_hot_column"] = {"max_column": list(hot_reports[-1]["max_column"]), "nnz": list(hot_reports[-1]["nnz"]),
                                   "report_ms": {k: statistics.median(r["ms"][k] for r in hot_reports[1:]) for k in ("upload", "kernels", "download", "total")}}
    say("from_rows with a hot column", row["from_rows_hot_column"], ok)

    def load_rows():
        bn.load_circuit(rows=rows, public_rows=False).free()

    def load_streams():
        bn.load_circuit(circuit).free()

    ms_rows, all_rows, _ = timed(load_rows, reps)
    ms_cols, all_cols, _ = timed(load_streams, reps)
    row["load_rows"] = {"ms": ms_rows, "all_ms": all_rows}
    row["load_circuit"] = {"ms": ms_cols, "all_ms": all_cols}
    row["ratio_load_rows_to_load_circuit"] = ms_rows / ms_cols if ms_cols > 0 else None
    say("load_rows", ms_rows, "load_circuit", ms_cols)
    a, b = bn.load_circuit(rows=rows, public_rows=False), bn.load_circuit(circuit)
    ra, rb = a.check_witness(good), b.check_witness(good)
    ok = ok and ra["ok"] == 1 and rb["ok"] == 1 and a.info() == b.info()
    a.free(); b.free()

    ks = {k: [] for k in ROWS_KERNELS + CSR_KERNELS + ("rows_resident",)}
    for i in range(reps + 1):
        lib.c.wsnark_timing_reset(); lib.c.wsnark_timing_enable(1)
        bn.circuit_from_rows(rows, public_rows=False)
        t_rows = lib.timing_report()
        lib.c.wsnark_timing_reset()
        load_streams()
        t_csr = lib.timing_report()
        lib.c.wsnark_timing_reset()
        load_rows()
        t_res = lib.timing_report()
        lib.c.wsnark_timing_enable(0)
        if i:
            for k in ROWS_KERNELS:
                ks[k].append(t_rows[k][0])
            for k in CSR_KERNELS:
                ks[k].append(t_csr[k][0])
            ks["rows_resident"].append(t_res["rows_resident"][0])
    m = {k: statistics.median(v) for k, v in ks.items()}
    t_rows_sum, t_csr_sum = sum(m[k] for k in ROWS_KERNELS), sum(m[k] for k in CSR_KERNELS)
    row["kernels"] = {"ms": m, "all_ms": ks, "rows_kernels_ms": t_rows_sum, "csr_kernels_ms": t_csr_sum,
                      "ratio_transpose": t_rows_sum / t_csr_sum if t_csr_sum > 0 else None,      # (the emulator's event timers read 0)
                      "budget": 2.0}
    say("kernels", m, "ratio", row["kernels"]["ratio_transpose"])
    nc.free()
    return row, bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import wasmsnark_amd
    bn = wasmsnark_amd.build(device=0)
    say = lambda *x: print(*x, file=sys.stderr, flush=True)
    row, ok = run(bn, a.log, a.reps, say)
    res = {"device": bn.device_info, "clock": read_clock(), "log_domain": a.log, "result": row, "ok": ok}
    print(json.dumps(res))
    assert ok, "a check of the tool failed (the streams byte for byte, ok == 1 on the generator's witness): no profile is written"
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
