#!/usr/bin/env python3
"""Many witnesses of one key: the batch call against the loop of the single prover (needs the GPU; bench.py is not involved).

One process, one resident key per size (the native generator's "columns" circuits, tables built).  For every cell (domain, batch):
  batch_ms_per_proof    wsnark_groth16_prove_batch from host memory on the batch path (BATCH_MIN = 1, BATCH_MAX_DOMAIN = 2^16)
  loop1_ms_per_proof    the loop of wsnark_groth16_prove from one thread
  loop2_ms_per_proof    the same proofs from two threads, one half each: the two lanes of a context
  batch and the two loops alternated `--reps` times, every repetition kept; report_ms: the batch call's own ms[] (last repetition);
  kernels: per-kernel ms of one more batch call (wsnark_timing_report); same_bytes: the LAST proof of the batch equals the loop's.
  single_kernels / key_table: per domain, the kernels of ONE proof of the single prover and how its key is resident.
  g1_fraction_of_peak   the G1 bucket kernel's product rate against wsnark_peak_probe(0) of the same run: mixed additions x 11
                        products (8 M + 2 S, the fused Y3 as two; curve.h) over the kernel's time.  Random witnesses: 255 of 256
                        digits are non-zero; msm_accumulate's figure for one big sum is 0.85.
A cell is WON when the batch's median beats the two-thread loop's median by more than the spread (max - min) of that loop's own
repetitions.  `crossover`: per domain the smallest batch from which every larger measured batch is won (null: none); `recommended`:
the routing defaults that take the batch path only there.  Prints ONE JSON line.
    python tools/prove_batch_bench.py [--out profiles/prove_batch_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--domains", default="10,12,14,16")
    ap.add_argument("--batches", default="1,4,16,64,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    domains = [int(x) for x in a.domains.split(",")]
    batches = [int(x) for x in a.batches.split(",")]
    import wasmsnark_amd
    from wasmsnark_amd import synth
    from wasmsnark_amd.bn128 import _ProveBatchReport, _prove_batch_report_dict
    bn = wasmsnark_amd.build(device=0)
    lib, c = bn.lib, bn.lib.c
    rnd = random.Random(12)
    g = C.c_double(0)
    lib.check(c.wsnark_peak_probe(0, C.byref(g)))
    res = {"device": bn.device_info, "peak_gmodmul_s": g.value, "reps": a.reps, "cells": [], "same_bytes": True}
    bmax = max(batches)
    for ld in domains:
        nc = synth.NativeCircuit(lib, ld, n_public=2, seed=5)
        sec, _ = nc.build_sections()
        key = bn.load_key(sections=sec)
        nv, stride = nc.n_vars, 32 * nc.n_vars
        raw = lambda b: (C.c_uint8 * len(b)).from_buffer_copy(b)      # (offsets into these: no per-proof copies inside the timed loops)
        wits = raw(nc.witness_bin() + b"".join(rnd.randbytes(stride) for _ in range(bmax - 1)))
        rs, ss = raw(rnd.randbytes(32 * bmax)), raw(rnd.randbytes(32 * bmax))

        def batch(n, timing=False):
            out, rep = (C.c_uint8 * (384 * n))(), _ProveBatchReport()
            lib.tune("BATCH_MIN", 1)
            lib.tune("BATCH_MAX_DOMAIN", 1 << 16)
            t = time.perf_counter()
            rc = c.wsnark_groth16_prove_batch(key._h, wits, stride, n, rs, ss, out, None, C.byref(rep))
            dt = time.perf_counter() - t
            lib.tune("BATCH_MIN", None)
            lib.tune("BATCH_MAX_DOMAIN", None)
            lib.check(rc)
            assert rep.batched == n
            return dt, bytes(out), _prove_batch_report_dict(rep)

        def loop(n, threads):
            out = (C.c_uint8 * (384 * n))()

            def work(lo, hi):
                for i in range(lo, hi):
                    lib.check(c.wsnark_groth16_prove(key._h, C.byref(wits, stride * i), stride, C.byref(rs, 32 * i), C.byref(ss, 32 * i), C.byref(out, 384 * i)))
            parts = [(0, n)] if threads == 1 or n == 1 else [(0, n // 2), (n // 2, n)]
            ts = [threading.Thread(target=work, args=p) for p in parts]
            t = time.perf_counter()
            for th in ts:
                th.start()
            for th in ts:
                th.join()
            return time.perf_counter() - t, bytes(out)

        batch(min(4, bmax)); loop(2, 1); loop(2, 2)      # warm: code objects, plans, the lanes' buffers
        # the single prover's own kernels at this size (one proof under the event timer): what the loop's figure is made of
        c.wsnark_timing_reset(); c.wsnark_timing_enable(1)
        loop(1, 1)
        res.setdefault("single_kernels", {})[str(ld)] = {k: {"ms": v[0], "launches": v[1]} for k, v in lib.timing_report().items()}
        c.wsnark_timing_enable(0)
        res.setdefault("key_table", {})[str(ld)] = key.table
        for n in batches:
            cell = {"log_domain": ld, "n_vars": nv, "batch": n, "batch_ms_per_proof": [], "loop1_ms_per_proof": [], "loop2_ms_per_proof": []}
            for _ in range(a.reps):
                dt, got, rep = batch(n)
                cell["batch_ms_per_proof"].append(dt * 1e3 / n)
                dt, want = loop(n, 1)
                cell["loop1_ms_per_proof"].append(dt * 1e3 / n)
                dt, want2 = loop(n, 2)
                cell["loop2_ms_per_proof"].append(dt * 1e3 / n)
                same = got[-384:] == want[-384:] == want2[-384:]
                res["same_bytes"] = res["same_bytes"] and same
            cell["report_ms"] = rep["ms"]
            cell["chunk"] = rep["chunk"]
            c.wsnark_timing_reset(); c.wsnark_timing_enable(1)
            batch(n)
            krep = lib.timing_report()
            c.wsnark_timing_enable(0)
            cell["kernels"] = {k: v[0] for k, v in krep.items() if k.startswith(("batch_", "ntt_pass"))}
            madds = n * (3 * nv + nc.domain) * 32 * 255 / 256      # A, B1, C over nVars signals, H over the domain; 32 windows
            if cell["kernels"].get("batch_buckets_g1"):
                cell["g1_fraction_of_peak"] = madds * 11 / (cell["kernels"]["batch_buckets_g1"] * 1e-3) / (g.value * 1e9)
            med = statistics.median
            l2 = cell["loop2_ms_per_proof"]
            cell["loop2_spread"] = max(l2) - min(l2)
            cell["won"] = bool(med(l2) - med(cell["batch_ms_per_proof"]) > cell["loop2_spread"])
            res["cells"].append(cell)
            print("2^%d x %d: batch %.3f  loop1 %.3f  loop2 %.3f ms/proof  %s" % (ld, n, med(cell["batch_ms_per_proof"]), med(cell["loop1_ms_per_proof"]),
                                                                                 med(l2), "won" if cell["won"] else "-"), file=sys.stderr, flush=True)
        key.free()
        nc.free()
    cross = {}
    for ld in domains:
        cells = sorted((x for x in res["cells"] if x["log_domain"] == ld), key=lambda x: x["batch"])
        first = None
        for i, x in enumerate(cells):
            if all(y["won"] for y in cells[i:]):
                first = x["batch"]
                break
        cross[str(ld)] = first
    res["crossover"] = cross
    won = [ld for ld in domains if cross[str(ld)] is not None]
    # one pair of thresholds: the domains up to the largest one with a crossover, from the largest crossover among them
    res["recommended"] = ({"BATCH_MAX_DOMAIN": 1 << max(won), "BATCH_MIN": max(cross[str(ld)] or (1 << 17) for ld in domains if ld <= max(won))}
                          if won else {"BATCH_MAX_DOMAIN": 0, "BATCH_MIN": 1 << 17})
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if res["same_bytes"] else 1)


if __name__ == "__main__":
    main()
