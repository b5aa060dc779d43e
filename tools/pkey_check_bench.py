#!/usr/bin/env python3
"""The audit of a proving key on the GPU beside the load it would precede (needs the GPU; bench.py is not involved).

For valid synthetic keys of 2^16 and 2^20 constraints (wasmsnark_amd.synth.NativeCircuit) prints ONE JSON line:
  keys[log]   points_only / with_relations   wsnark_pkey_check_sections end to end from host memory, best of three: ms, and the
                                             report's own split ms[] (upload + point kernels, relation sums, host pairings, whole call)
              kernels                        per-kernel ms of one full call (wsnark_timing_report): pkcheck_g1 (four sections),
                                             pkcheck_g2, and everything the two relation sums launch
              psi                            the same audit with the subgroup test psi(Q) == [6x^2] Q (WSNARK_PKCHECK_SUBGROUP=1):
                                             points-only ms, its kernel's ms, and whether its report equals the shipped one's
              load_ms                        wsnark_pkey_load_stats of the SAME key loaded in the same process right after: element [4]
                                             is what the load call took -- with check: true a key's bytes cross the link twice, and
                                             audit + load is what the caller waits for
              b2_points_per_s, b2_fraction_of_peak   the B2 kernel against the multiplier peak (wsnark_peak_probe(0)) of the same run
  products_per_b2_point   base-field multiplier calls of one [r] Q chain (and of the psi chain), from the formulas of curve.h
  reports_ok  every report said ok with 7 relations run, and the psi reports equal the shipped ones
    python tools/pkey_check_bench.py [--logs 16,20] [--out profiles/pkey_check_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def product_counts():
    """Product equivalents per finite B2 point (one product = 1, a fused double product 1.5, a four-product reduction 2.5; an Fq2
    product is 2 double products, an Fq2 squaring 2 products, mulsub2 in Fq2 2 four-product reductions).  curve.h: the XYZZ doubling
    is 3 S + 4 M + mulsub2, the mixed addition 2 S + 6 M + mulsub2; the curve equation 2 S + 1 M; to_internal one product per word."""
    pc = lambda v: bin(v).count("1")
    f2mul, f2sqr, mulsub2 = 3.0, 2.0, 5.0
    dbl, madd = 3 * f2sqr + 4 * f2mul + mulsub2, 2 * f2sqr + 6 * f2mul + mulsub2
    head = 4 + 2 * f2sqr + f2mul
    t = P - R
    return {"r_chain": head + 254 * dbl + pc(R) * madd, "psi_chain": head + 127 * dbl + pc(t) * madd + 4 * f2mul,
            "doubling": dbl, "mixed_addition": madd, "set_bits_of_r": pc(R), "set_bits_of_6x2": pc(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import wasmsnark_amd
    from wasmsnark_amd import synth
    bn = wasmsnark_amd.build(device=0)
    lib = bn.lib
    res = {"device": bn.device_info, "clock": "not read", "chunk_points": 1 << 18, "keys": {}}
    pcnt = product_counts()
    res["products_per_b2_point"] = pcnt
    g = C.c_double(0)
    lib.check(lib.c.wsnark_peak_probe(0, C.byref(g)))
    res["peak_gmodmul_s"] = g.value
    ok = True
    strip = lambda r: {k: v for k, v in r.items() if k != "ms"}

    def timed(sec, n=3, **kw):
        best, rep = None, None
        for _ in range(n):
            t = time.perf_counter()
            r = bn.check_key(sections=sec, **kw)
            dt = (time.perf_counter() - t) * 1e3
            if best is None or dt < best:
                best, rep = dt, r
        return best, rep

    def kernels(sec, **kw):
        lib.c.wsnark_timing_reset(); lib.c.wsnark_timing_enable(1)
        bn.check_key(sections=sec, **kw)
        rep = lib.timing_report()
        lib.c.wsnark_timing_enable(0)
        return {k: v[0] for k, v in rep.items()}

    for log in [int(x) for x in a.logs.split(",")]:
        sec = synth.NativeCircuit(lib, log, n_public=2, seed=log).build_sections()[0]
        nbytes = sum(len(sec[k]) for k in ("pointsA", "pointsB1", "pointsB2", "pointsC", "pointsH"))
        bn.check_key(sections=sec)          # warm: code objects, the staging ring, the sums' workspaces
        ms_p, rep_p = timed(sec, relations=False)
        ms_f, rep_f = timed(sec)
        ok = ok and rep_p["ok"] and rep_f["ok"] and rep_f["relations_run"] == 7 and rep_p["relations_run"] == 0
        kern = kernels(sec)
        finite_b2 = rep_f["B2"]["points"] - rep_f["B2"]["infinity"]
        lib.tune("PKCHECK_SUBGROUP", 1)
        ms_psi, rep_psi = timed(sec, relations=False)
        kern_psi = kernels(sec, relations=False)
        lib.tune("PKCHECK_SUBGROUP", None)
        ok = ok and strip(rep_psi) == strip(rep_p)
        key = bn.load_key(sections=sec)
        load_ms = dict(key.load_ms)
        key.free()
        g2_ms = kern.get("pkcheck_g2", 0.0)
        entry = {"n_vars": sec["n_vars"], "domain": sec["domain"], "point_bytes": nbytes, "b2_finite_points": finite_b2,
                 "points_only": {"ms": ms_p, "split_ms": rep_p["ms"]}, "with_relations": {"ms": ms_f, "split_ms": rep_f["ms"]},
                 "kernels": {"pkcheck_g1": kern.get("pkcheck_g1", 0.0), "pkcheck_g2": g2_ms,
                             "relation_sum_kernels": sum(v for k, v in kern.items() if not k.startswith("pkcheck"))},
                 "psi": {"points_only_ms": ms_psi, "pkcheck_g2_psi": kern_psi.get("pkcheck_g2_psi", 0.0), "same_report": strip(rep_psi) == strip(rep_p)},
                 "load_ms": load_ms, "audit_plus_load_ms": ms_f + load_ms["total"]}
        if g2_ms > 0:
            entry["b2_points_per_s"] = finite_b2 / (g2_ms * 1e-3)
            entry["b2_fraction_of_peak"] = pcnt["r_chain"] * entry["b2_points_per_s"] / (g.value * 1e9)
            if entry["psi"]["pkcheck_g2_psi"] > 0:
                entry["psi"]["b2_points_per_s"] = finite_b2 / (entry["psi"]["pkcheck_g2_psi"] * 1e-3)
        res["keys"][str(log)] = entry
    res["reports_ok"] = bool(ok)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
