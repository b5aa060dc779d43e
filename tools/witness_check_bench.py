#!/usr/bin/env python3
"""The witness check on the GPU (needs the GPU; bench.py is not involved).  Prints ONE JSON line; on ONE circuit of the native
generator's "columns" family (csrc/synth.hip, style 0) at log2(domain) = --log, all in the SAME process:
  load_circuit        wsnark_circuit_load: the three record streams to resident CSR, whole call by the host clock
  check_host          a resident check from a host witness (upload + kernels + one small download): the host clock and the report's own
                      ms[] (device, total), medians of --reps calls after a warm-up
  check_dev           the same from a witness already on the device
  check_one_shot      load + check + free in one call
  kernels             lc_check_kernel, witness_facts_kernel (and lc_row_values_kernel for the planted-bad witness) from
                      wsnark_timing_report, beside lc_split_kernel on the same three matrices with the witness as weights
                      (circuit_row_sums): it walks the same records once and writes six vectors where lc_check writes a bitmask.
                      ratio_check_to_split = (lc_check + witness_facts) / lc_split; the issue's budget for it is 1.25
  proof               groth16GenProof on the same witness and a key of the same circuit; check_share_of_proof = check_host / proof
The generator exports only A and B; its C is "row c holds 1 x its output variable 1 + nFree + c" (synth.hip), written here as a
record stream.  The tool asserts ok == 1 on the generator's witness and bad == 1 after one private signal that a single row uses
(the last variable: no later row reads it) has changed.
    python tools/witness_check_bench.py [--log 20] [--reps 5] [--out profiles/witness_check_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def pols_c(n_vars, n_public):
    """the C matrix of the native generator's styles 0 and 1 as a record stream: signal s >= 1 + nFree has ONE record (row s - 1 - nFree,
    coefficient 1 in Montgomery form), every other signal none"""
    import numpy as np
    n_free = n_public + 2
    first = 1 + n_free
    rec = np.zeros(n_vars - first, dtype=[("count", "<u4"), ("row", "<u4"), ("coef", "V32")])
    rec["count"] = 1
    rec["row"] = np.arange(n_vars - first, dtype=np.uint32)
    rec["coef"] = np.frombuffer(((1 << 256) % R).to_bytes(32, "little"), dtype="V32")[0]
    return bytes(4 * first) + rec.tobytes()


def timed(fn, reps):
    """(median ms by the host clock, every call's ms, every call's result) of `reps` calls after one warm-up"""
    fn()
    ts, outs = [], []
    for _ in range(max(reps, 1)):
        t = time.perf_counter()
        outs.append(fn())
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), ts, outs


def run(bn, log, reps, dev=True, say=lambda *x: None):
    from wasmsnark_amd import synth
    lib = bn.lib
    nc = synth.NativeCircuit(lib, log, n_public=2, seed=log, style="columns")
    sec, _ = nc.build_sections()
    circuit = {"n_vars": nc.n_vars, "n_public": nc.n_public, "domain": nc.domain, "polsA": bytes(sec["polsA"]), "polsB": bytes(sec["polsB"]),
               "polsC": pols_c(nc.n_vars, nc.n_public)}
    good = nc.witness_bin()
    last = nc.n_vars - 1
    v = (int.from_bytes(good[32 * last:], "little") + 1) % R
    bad = good[:32 * last] + v.to_bytes(32, "little")
    say("inputs", log)
    row = {"n_vars": nc.n_vars, "n_public": nc.n_public, "domain": nc.domain, "reps": reps}

    def load_and_free():
        h = bn.load_circuit(circuit)
        h.free()

    ms_load, all_load, _ = timed(load_and_free, reps)
    row["load_circuit"] = {"ms": ms_load, "all_ms": all_load}
    rc = bn.load_circuit(circuit)
    inf = rc.info()
    row["nnz"], row["csr_bytes"] = list(inf["nnz"]), inf["bytes"]
    say("load_circuit", ms_load, inf)

    med = lambda outs, k: statistics.median(o["ms"][k] for o in outs)
    ms_host, all_host, outs = timed(lambda: rc.check_witness(good), reps)
    ok = all(o["ok"] == 1 and o["bad"] == 0 for o in outs)
    row["check_host"] = {"ms": ms_host, "all_ms": all_host, "report_ms": {"device": med(outs, "device"), "total": med(outs, "total")}}
    say("check_host", ms_host)
    ms_bad, all_bad, outs = timed(lambda: rc.check_witness(bad), reps)
    ok = ok and all(o["ok"] == 0 and o["bad"] == 1 and o["bad_rows"] == [nc.domain - nc.n_public - 2] for o in outs)
    a, b, c = outs[-1]["bad_values"][0] if outs[-1]["bad_values"] else (0, 0, 0)
    ok = ok and a * b % R == (c - 1) % R      # the row held before its output variable went up by one
    row["check_host_one_bad_row"] = {"ms": ms_bad, "all_ms": all_bad}
    say("check_host (one bad row)", ms_bad, outs[-1]["bad"], outs[-1]["bad_rows"])
    if dev:
        import torch
        d_w = torch.frombuffer(bytearray(good), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        ms_dev, all_dev, outs = timed(lambda: rc.check_witness_dev(d_w.data_ptr(), d_w.numel()), reps)
        ok = ok and all(o["ok"] == 1 and o["bad"] == 0 for o in outs)
        row["check_dev"] = {"ms": ms_dev, "all_ms": all_dev, "report_ms": {"device": med(outs, "device"), "total": med(outs, "total")}}
        say("check_dev", ms_dev)
    ms_shot, all_shot, outs = timed(lambda: bn.check_witness(circuit, good), reps)
    ok = ok and all(o["ok"] == 1 for o in outs)
    row["check_one_shot"] = {"ms": ms_shot, "all_ms": all_shot, "report_ms": {"matrices": med(outs, "matrices"), "device": med(outs, "device")}}
    say("check_one_shot", ms_shot)

    # the kernels alone, by the library's event timer: the check (good and bad witness) and lc_split on the same matrices
    ks = {"lc_check": [], "witness_facts": [], "lc_row_values": [], "lc_split": []}
    for i in range(reps + 1):
        lib.c.wsnark_timing_reset(); lib.c.wsnark_timing_enable(1)
        rc.check_witness(good)
        t_good = lib.timing_report()
        lib.c.wsnark_timing_reset()
        rc.check_witness(bad)
        bn.circuit_row_sums(circuit, good)
        t = lib.timing_report()
        lib.c.wsnark_timing_enable(0)
        if i:
            ks["lc_check"].append(t_good["lc_check"][0])
            ks["witness_facts"].append(t_good["witness_facts"][0])
            ks["lc_row_values"].append(t["lc_row_values"][0])
            ks["lc_split"].append(t["lc_split"][0])
    m = {k: statistics.median(x) for k, x in ks.items()}
    part = m["lc_check"] + m["witness_facts"]
    row["kernels"] = {"lc_check_ms": m["lc_check"], "witness_facts_ms": m["witness_facts"], "lc_row_values_ms": m["lc_row_values"],
                      "lc_split_ms": m["lc_split"], "all_ms": ks, "check_device_part_ms": part,
                      "ratio_check_to_split": part / m["lc_split"] if m["lc_split"] > 0 else None,      # (the emulator's event timers read 0)
                      "budget": 1.25}
    say("kernels", row["kernels"])

    key = bn.load_key(sections=sec)
    r, s = bytes(range(1, 33)), bytes(range(40, 72))
    ms_proof, all_proof, outs = timed(lambda: bn.groth16GenProof(good, key, r=r, s=s), reps)
    ok = ok and outs[-1] == nc.expected_proof(r, s)
    row["proof"] = {"ms": ms_proof, "all_ms": all_proof}
    row["check_share_of_proof"] = ms_host / ms_proof if ms_proof > 0 else None
    ms_both, all_both, outs2 = timed(lambda: bn.groth16GenProof(good, key, r=r, s=s, circuit=rc), reps)
    ok = ok and outs2[-1] == outs[-1]
    row["proof_with_circuit"] = {"ms": ms_both, "all_ms": all_both}
    say("proof", ms_proof, "with circuit", ms_both)
    key.free(); rc.free(); nc.free()
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
    row, ok = run(bn, a.log, a.reps, True, say)
    res = {"device": bn.device_info, "clock": "not read", "log_domain": a.log, "result": row, "ok": ok}
    print(json.dumps(res))
    assert ok, "a check of the tool failed (ok == 1 on the generator's witness, bad == 1 on the planted one, the proofs): no profile is written"
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
