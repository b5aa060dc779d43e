#!/usr/bin/env python3
"""Many witnesses against one resident circuit: the batch call against the loop of the single check (needs the GPU; bench.py is not
involved).  One process, one resident circuit per size (the native generator's "columns" circuits, csrc/synth.hip; their C matrix
written down as in tools/witness_check_bench.py).  Prints ONE JSON line.

For every cell (domain, count, where the witnesses are, column):
  batch_ms    wsnark_circuit_witness_check_batch[_dev], whole call by the host clock
  loop_ms     the loop of wsnark_circuit_witness_check[_dev] over the same witnesses, same cap, one thread: the yardstick
  batch and loop alternated `--reps` times after a warm-up, every repetition kept; loop_spread = max - min of the loop's repetitions.
  A cell is WON when the batch's median is below the loop's median by more than loop_spread.
  same        every verdict of the batch equals the loop's report of that witness (bad, first_bad, listed, ok and the listed rows)
Columns: "good" -- all witnesses are the generator's own, copied count times so that every witness is an array of its own;
"eighth_bad" -- every eighth witness has its last signal changed (one bad row: no later row reads it); cap = 4 in both.

kernel: by the library's event timer, lc_check_batch for 256 witnesses at 2^12 (2^20 rows) beside lc_check on the 2^20 circuit of
tools/witness_check_bench.py (seed = log), in this same run: the rows come from the same generator, so the per-row work is equal, and
ratio = lc_check_batch / lc_check has the project's budget of 1.25 -- the quarter covers 256 witness arrays instead of one behind the
gathers.  Over budget is a finding, not a failure.

guarded_prover: groth16GenProofBatch at 2^10 x 256 on the batch kernels with and without circuit=.
    python tools/witness_check_batch_bench.py [--out profiles/witness_check_batch_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from witness_check_bench import R, pols_c      # noqa: E402

CAP = 4


def native_circuit(lib, log, seed):
    """(NativeCircuit, the circuit dict of load_circuit) without building a key"""
    from wasmsnark_amd import synth
    nc = synth.NativeCircuit(lib, log, n_public=2, seed=seed, style="columns")
    pols = []
    for m, n in ((0, nc.info.pols_a_len), (1, nc.info.pols_b_len)):
        buf = bytearray(n)
        lib.check(lib.c.wsnark_synth_pols(nc._h, m, nc._cbuf(buf), n))
        pols.append(bytes(buf))
    return nc, {"n_vars": nc.n_vars, "n_public": nc.n_public, "domain": nc.domain, "polsA": pols[0], "polsB": pols[1],
                "polsC": pols_c(nc.n_vars, nc.n_public)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--domains", default="10,12,14,16")
    ap.add_argument("--counts", default="1,16,64,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-log", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    domains = [int(x) for x in a.domains.split(",")]
    counts = [int(x) for x in a.counts.split(",")]
    import torch
    import wasmsnark_amd
    from wasmsnark_amd import synth
    from wasmsnark_amd.bn128 import _WitnessBatchReport, _WitnessReport, _WitnessVerdict
    bn = wasmsnark_amd.build(device=0)
    lib, c = bn.lib, bn.lib.c
    say = lambda *x: print(*x, file=sys.stderr, flush=True)
    res = {"device": bn.device_info, "clock": "not read", "reps": a.reps, "cap": CAP, "cells": [], "same": True}
    cmax = max(counts)
    med = statistics.median

    for ld in domains:
        nc, circuit = native_circuit(lib, ld, 5)
        rc = bn.load_circuit(circuit)
        nv, stride = nc.n_vars, 32 * nc.n_vars
        good = nc.witness_bin()
        v = (int.from_bytes(good[32 * (nv - 1):], "little") + 1) % R
        bad = good[:32 * (nv - 1)] + v.to_bytes(32, "little")
        for column in ("good", "eighth_bad"):
            blob = b"".join(bad if (column == "eighth_bad" and i % 8 == 7) else good for i in range(cmax))
            host = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
            d_t = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            del blob
            for where in ("device", "host"):
                base = d_t.data_ptr() if where == "device" else C.addressof(host)

                def batch(n):
                    ver, rows, vals, rep = (_WitnessVerdict * n)(), (C.c_uint64 * (n * CAP))(), (C.c_uint8 * (96 * n * CAP))(), _WitnessBatchReport()
                    t = time.perf_counter()
                    if where == "device":
                        code = c.wsnark_circuit_witness_check_batch_dev(rc._h, base, stride, n, ver, rows, vals, CAP, C.byref(rep), None)
                    else:
                        code = c.wsnark_circuit_witness_check_batch(rc._h, base, stride, n, ver, rows, vals, CAP, C.byref(rep))
                    dt = time.perf_counter() - t
                    lib.check(code)
                    return dt, [(int(x.bad), int(x.first_bad), int(x.listed), int(x.ok), list(rows[i * CAP:i * CAP + int(x.listed)])) for i, x in enumerate(ver)], rep

                def loop(n, collect=False):      # (timed: the calls alone; collect: an untimed pass that keeps every report)
                    rows, vals, rep, out = (C.c_uint64 * CAP)(), (C.c_uint8 * (96 * CAP))(), _WitnessReport(), []
                    one = c.wsnark_circuit_witness_check_dev if where == "device" else c.wsnark_circuit_witness_check
                    args = [rc._h, 0, stride, rows, vals, CAP, C.byref(rep)] + ([None] if where == "device" else [])
                    t = time.perf_counter()
                    for i in range(n):
                        args[1] = base + i * stride
                        if one(*args):
                            raise RuntimeError("the single check failed")
                        if collect:
                            out.append((int(rep.bad), int(rep.first_bad), int(rep.listed), int(rep.ok), list(rows[:int(rep.listed)])))
                    return time.perf_counter() - t, out

                batch(min(cmax, 16)); loop(2)      # warm: code objects, the lane's buffers
                for n in counts:
                    cell = {"log_domain": ld, "n_vars": nv, "count": n, "where": where, "column": column, "batch_ms": [], "loop_ms": []}
                    for _ in range(a.reps):
                        dt, got, rep = batch(n)
                        cell["batch_ms"].append(dt * 1e3)
                        dt, _ = loop(n)
                        cell["loop_ms"].append(dt * 1e3)
                    res["same"] = res["same"] and got == loop(n, collect=True)[1]
                    expect_bad = [i for i in range(n) if column == "eighth_bad" and i % 8 == 7]
                    res["same"] = res["same"] and [i for i, g in enumerate(got) if not g[3]] == expect_bad
                    cell["chunk"] = int(rep.chunk)
                    cell["report_device_ms"] = rep.ms[1]
                    cell["loop_spread"] = max(cell["loop_ms"]) - min(cell["loop_ms"])
                    cell["won"] = bool(med(cell["loop_ms"]) - med(cell["batch_ms"]) > cell["loop_spread"])
                    cell["lost"] = bool(med(cell["batch_ms"]) - med(cell["loop_ms"]) > cell["loop_spread"])
                    res["cells"].append(cell)
                    say("2^%d x %3d %-6s %-10s batch %8.3f  loop %8.3f ms  spread %.3f  %s" % (ld, n, where, column, med(cell["batch_ms"]), med(cell["loop_ms"]),
                                                                                            cell["loop_spread"], "won" if cell["won"] else "lost" if cell["lost"] else "-"))
            del d_t, host
        rc.free(); nc.free()

    # ---- the kernel alone: 256 witnesses at 2^12 against one witness at 2^20, the same generator, the same run ----
    nc12, circ12 = native_circuit(lib, 12, 5)
    ncbig, circbig = native_circuit(lib, a.kernel_log, a.kernel_log)
    n_small = (1 << a.kernel_log) >> 12
    rc12, rcbig = bn.load_circuit(circ12), bn.load_circuit(circbig)
    d12 = torch.frombuffer(bytearray(nc12.witness_bin() * n_small), dtype=torch.uint8).cuda()
    dbig = torch.frombuffer(bytearray(ncbig.witness_bin()), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    ks = {"lc_check_batch": [], "witness_facts_batch": [], "lc_check": [], "witness_facts": []}
    for i in range(a.reps + 3):
        c.wsnark_timing_reset(); c.wsnark_timing_enable(1)
        ok = all(x["ok"] for x in rc12.check_witnesses_dev(d12.data_ptr(), 32 * nc12.n_vars, n_small, max_rows=0))
        ok = ok and rcbig.check_witness_dev(dbig.data_ptr(), dbig.numel(), max_rows=0)["ok"] == 1
        t = lib.timing_report()
        c.wsnark_timing_enable(0)
        res["same"] = res["same"] and bool(ok)
        if i:
            for k in ks:
                ks[k].append(t[k][0])
    m = {k: med(x) for k, x in ks.items()}
    res["kernel"] = {"rows": 1 << a.kernel_log, "witnesses": n_small, "log_domain_batch": 12, "log_domain_single": a.kernel_log,
                     "nnz_batch_per_witness": list(rc12.info()["nnz"]), "nnz_single": list(rcbig.info()["nnz"]),
                     "lc_check_batch_ms": m["lc_check_batch"], "lc_check_ms": m["lc_check"], "witness_facts_batch_ms": m["witness_facts_batch"],
                     "witness_facts_ms": m["witness_facts"], "all_ms": ks, "ratio": m["lc_check_batch"] / m["lc_check"] if m["lc_check"] > 0 else None,
                     "budget": 1.25}
    res["kernel"]["within_budget"] = bool(res["kernel"]["ratio"] is not None and res["kernel"]["ratio"] <= 1.25)
    say("kernel", res["kernel"])
    for h in (rc12, rcbig, nc12, ncbig):
        h.free()
    del d12, dbig

    # ---- the guarded batch prover at 2^10 x 256 ----
    nc, circuit = native_circuit(lib, 10, 5)
    sec, _ = nc.build_sections()
    key, rc = bn.load_key(sections=sec), bn.load_circuit(circuit)
    wits = nc.witness_bin() * 256
    rs = bytes(range(256)) * 32
    lib.tune("BATCH_MIN", 1)
    lib.tune("BATCH_MAX_DOMAIN", 1 << 16)
    rows = {"plain_ms": [], "guarded_ms": []}
    bn.groth16GenProofBatch(wits, key, r=rs, s=rs, circuit=rc)
    for _ in range(a.reps):
        t = time.perf_counter()
        plain = bn.groth16GenProofBatch(wits, key, r=rs, s=rs)
        rows["plain_ms"].append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        guarded = bn.groth16GenProofBatch(wits, key, r=rs, s=rs, circuit=rc)
        rows["guarded_ms"].append((time.perf_counter() - t) * 1e3)
        res["same"] = res["same"] and plain == guarded
    lib.tune("BATCH_MIN", None)
    lib.tune("BATCH_MAX_DOMAIN", None)
    res["guarded_prover"] = dict(rows, log_domain=10, count=256, plain_median_ms=med(rows["plain_ms"]), guarded_median_ms=med(rows["guarded_ms"]))
    say("guarded prover", res["guarded_prover"])
    key.free(); rc.free(); nc.free()

    res["won"] = sum(1 for x in res["cells"] if x["won"])
    res["lost"] = sum(1 for x in res["cells"] if x["lost"])
    res["count_1_lost"] = [[x["log_domain"], x["where"], x["column"]] for x in res["cells"] if x["count"] == 1 and x["lost"]]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if res["same"] else 1)


if __name__ == "__main__":
    main()
