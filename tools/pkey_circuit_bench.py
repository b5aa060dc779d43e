#!/usr/bin/env python3
"""The key-against-circuit check on the GPU (needs the GPU; bench.py is not involved).  Prints ONE JSON line; per log2(domain), on
the SAME inputs in the SAME process (a synthetic circuit of the "columns" family and its transcript, tools/pkey_setup_bench.py's):
  check_key_circuit   the whole call from host memory on the key AFTER one contribution (C and hExps under a delta the check does
                      not know), with its verification key and a seed from the OS: the host clock around the call (median of --reps
                      calls after a warm-up) and the verdict's own ms[] (matrices = CSR + row sums + transforms, key_sums,
                      powers_sums, pairings, total), medians over the same calls
  setup_key           the whole call that rebuilds the first key from the transcript -- the only other way to tie a key to its circuit,
                      and only before the first contribution; ratio_check_to_setup = check_key_circuit / setup_key
  check_key           the audit of the same key's points, whole call
  kernels             lc_split_kernel (three matrices, both halves, one walk) beside lc_spmv2_kernel (calcH on the same A and B: two
                      matrices, one sum) from wsnark_timing_report, and both per matrix-row walked; ratio_per_matrix = split / spmv
    python tools/pkey_circuit_bench.py [--logs 20] [--reps 3] [--out profiles/pkey_circuit_bench.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def timed(fn, reps):
    """(median ms by the host clock, every call's result) of `reps` calls after one warm-up; every call ends synchronised"""
    fn()
    ts, outs = [], []
    for _ in range(max(reps, 1)):
        t = time.perf_counter()
        outs.append(fn())
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), ts, outs


def run(bn, log, reps, say=lambda *x: None):
    from pkey_setup_bench import native_inputs
    from wasmsnark_amd import synth
    lib = bn.lib
    powers, circuit, native, delta = native_inputs(bn, log, seed=log)
    say("inputs", log)
    row = {"n_vars": circuit["n_vars"], "n_public": circuit["n_public"], "domain": circuit["domain"], "reps": reps}
    ms_setup, all_setup, outs = timed(lambda: bn.setup_key(powers, circuit), reps)
    new, (ic, gamma2), rep = outs[-1]
    ok = rep["ok"]
    row["setup_key"] = {"ms": ms_setup, "all_ms": all_setup, "split_ms": rep["ms"]}
    say("setup_key", ms_setup)
    that, rep_c = bn.contribute_key(sections=new, d=delta)
    ok = ok and rep_c["ok"] and all(bytes(that[x]) == bytes(native[x]) for x in native if not isinstance(native[x], int))
    vk = synth.vk_with_delta2(synth.vk_from_points(circuit["n_public"], new, ic, gamma2), that)
    ms_audit, all_audit, outs = timed(lambda: bn.check_key(sections=that), reps)
    ok = ok and outs[-1]["ok"]
    row["check_key"] = {"ms": ms_audit, "all_ms": all_audit}
    say("check_key", ms_audit)
    ms_check, all_check, outs = timed(lambda: bn.check_key_circuit(powers, circuit, sections=that, vk=vk), reps)
    ok = ok and all(v["ok"] and v["checks_run"] == 0x3FF for v in outs)
    row["check_key_circuit"] = {"ms": ms_check, "all_ms": all_check,
                                "verdict_ms": {k: statistics.median(v["ms"][k] for v in outs) for k in outs[0]["ms"]}}
    row["ratio_check_to_setup"] = ms_check / ms_setup if ms_setup > 0 else None
    say("check_key_circuit", ms_check, row["check_key_circuit"]["verdict_ms"])
    # a wrong key is found: two points of A swapped
    bad = dict(that, pointsA=bytes(that["pointsA"][64:128]) + bytes(that["pointsA"][:64]) + bytes(that["pointsA"][128:]))
    v = bn.check_key_circuit(powers, circuit, sections=bad, vk=vk)
    ok = ok and not v["ok"] and v["checks_bad"] == 8
    # the two sparse products alone, by the library's event timer
    rnd = random.Random(log)
    signals = b"".join(rnd.randrange(R).to_bytes(32, "little") for _ in range(circuit["n_vars"]))
    split, spmv = [], []
    for i in range(reps + 1):
        lib.c.wsnark_timing_reset(); lib.c.wsnark_timing_enable(1)
        bn.check_key_circuit(powers, circuit, sections=that)
        bn.calcH(signals, circuit["polsA"], circuit["polsB"], circuit["n_vars"], circuit["domain"])
        t = lib.timing_report()
        lib.c.wsnark_timing_enable(0)
        if i:
            split.append(t["lc_split"][0])
            spmv.append(t["lc_spmv"][0])
    ms_split, ms_spmv = statistics.median(split), statistics.median(spmv)
    row["kernels"] = {"lc_split_ms": ms_split, "lc_split_all_ms": split, "lc_split_matrices": 3, "lc_spmv2_ms": ms_spmv, "lc_spmv2_all_ms": spmv,
                      "lc_spmv2_matrices": 2, "lc_split_ms_per_matrix": ms_split / 3, "lc_spmv2_ms_per_matrix": ms_spmv / 2,
                      "ratio_per_matrix": (ms_split / 3) / (ms_spmv / 2) if ms_spmv > 0 else None}      # (the emulator's event timers read 0)
    say("kernels", row["kernels"])
    return row, bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="20")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import wasmsnark_amd
    bn = wasmsnark_amd.build(device=0)
    say = lambda *x: print(*x, file=sys.stderr, flush=True)
    res = {"device": bn.device_info, "clock": "not read", "reps": a.reps, "keys": {}}
    ok = True
    for log in (int(x) for x in a.logs.split(",")):
        row, good = run(bn, log, a.reps, say)
        res["keys"][str(log)] = row
        ok = ok and good
    res["ok"] = bool(ok)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
