#!/usr/bin/env python3
"""The phase-2 delta contribution on the GPU (needs the GPU; bench.py is not involved).  Prints ONE JSON line:
  scale_kernel   scale_points_kernel<G1> at n = 2^20 random valid points, one random 254-bit scalar: kernel ms per call (the sum of
                 the call's chunk launches, wsnark_timing_report; median of --reps calls after a warm-up), points/s, and the fraction
                 of the multiplier peak (wsnark_peak_probe(0), same process) at products_per_point field products per point
  yardstick      mul_base_kernel<G1> at n = 2^20 with random 254-bit scalars, same process, same timer, and the ratio
                 scale / mul_base of the per-point kernel times (required: <= 1)
  keys[log]      contribute / delta_verify end to end from host memory with their own ms[] splits, beside check_key and load_key
                 of the same key, and the link time of the bytes a contribution moves (2 x the C and hExps bytes at the H2D rate
                 measured by the load of the same key)
  sha256         of the output bytes of every timed call that returns bytes, by the call's name (the inputs are seeded)
    python tools/pkey_delta_bench.py [--logs 16,20] [--reps 5] [--out profiles/pkey_delta_bench.json]
"""
import argparse
import ctypes as C
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


def naf_shape(k):
    """(digits, non-zero digits) of k's non-adjacent form"""
    n = w = 0
    while k:
        if k & 1:
            k -= 2 - (k & 3)
            w += 1
        k >>= 1
        n += 1
    return n, w


def products_per_point(k):
    """Field products per finite G1 point, squarings counted as products and the fused two-product Y3 as 2, from curve.h's formulas:
    to_internal 2, curve equation 3, doubling 4 M + 3 S + 2, mixed addition 7 M + 2 S + 2, Fermat inversion 253 S + popcount(q - 2)
    M, its three surrounding products + 2 for x, y, from_internal 2.  The shared inversion puts 3 products per tree level and lane
    (8 + 16) and 1/4 of a Fermat chain (one wavefront of four inverts) in the place of a chain per lane."""
    q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
    dbl, madd = 9, 11
    digits, weight = naf_shape(k)
    chain = (digits - 1) * dbl + (weight - 1) * madd
    fermat = 253 + bin(q - 2).count("1")
    return {"doubling": dbl, "mixed_addition": madd, "naf_digits": digits, "naf_weight": weight, "chain": chain, "fermat_inversion": fermat,
            "shared_inversion_total": 5 + chain + 24 + fermat / 4 + 5 + 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import wasmsnark_amd
    from wasmsnark_amd import synth
    from pkey_setup_bench import sha256_of
    bn = wasmsnark_amd.build(device=0)
    lib = bn.lib
    rnd = random.Random(11)
    res = {"device": bn.device_info, "clock": "not read", "chunk_points": 1 << 18, "reps": a.reps, "n": a.n}
    g = C.c_double(0)
    lib.check(lib.c.wsnark_peak_probe(0, C.byref(g)))
    res["peak_gmodmul_s"] = g.value
    n = a.n
    scalars = b"".join(rnd.randrange(1 << 253, R).to_bytes(32, "little") for _ in range(n))
    k = rnd.randrange(1 << 253, R)
    res["products_per_point"] = products_per_point(k)
    res["sha256"] = {}

    def kernel_ms(name, fn, prefix):
        out = []
        for i in range(a.reps + 1):
            lib.c.wsnark_timing_reset(); lib.c.wsnark_timing_enable(1)
            got = fn()
            rep = lib.timing_report()
            lib.c.wsnark_timing_enable(0)
            if i:
                out.append(sum(v[0] for kk, v in rep.items() if kk.startswith(prefix)))
        res["sha256"][name] = sha256_of(got)
        return statistics.median(out), out

    pts = bn.mul_base(1, scalars)
    mb, mb_all = kernel_ms("mul_base G1", lambda: bn.mul_base(1, scalars), "mul_base_g1")
    res["yardstick"] = {"kernel": "mul_base_kernel<G1>", "ms": mb, "all_ms": mb_all, "points_per_s": n / (mb * 1e-3)}
    ms, all_ms = kernel_ms("scale_points G1", lambda: bn.scale_points(1, pts, k), "scale_points_g1_shared_inv")
    ppp = res["products_per_point"]["shared_inversion_total"]
    res["scale_kernel"] = {"kernel": "scale_points_kernel<G1>", "ms": ms, "all_ms": all_ms, "points_per_s": n / (ms * 1e-3),
                           "products_per_point_used": ppp, "fraction_of_peak": ppp * n / (ms * 1e-3) / (g.value * 1e9)}
    res["yardstick"]["ratio_scale_over_mul_base"] = ms / mb
    ok = ms <= mb
    del pts, scalars

    def timed(fn):
        fn()
        ts, last = [], None
        for _ in range(a.reps):
            t = time.perf_counter()
            last = fn()
            ts.append((time.perf_counter() - t) * 1e3)
        return statistics.median(ts), last

    res["keys"] = {}
    d = (k * 7 + 1) % R
    for log in [int(x) for x in a.logs.split(",")]:
        sec = synth.NativeCircuit(lib, log, n_public=2, seed=log).build_sections()[0]
        moved = 2 * (len(sec["pointsC"]) + len(sec["pointsH"]))
        ms_c, (new, rep) = timed(lambda: bn.contribute_key(sections=sec, d=d))
        res["sha256"]["contribute_key 2^%d" % log] = sha256_of(new)
        ms_v, ver = timed(lambda: bn.verify_contribution(sec, new, check=False))
        ms_a, aud = timed(lambda: bn.check_key(sections=new))
        key = bn.load_key(sections=sec)
        load_ms = dict(key.load_ms)
        key.free()
        nbytes = sum(len(sec[x]) for x in ("pointsA", "pointsB1", "pointsB2", "pointsC", "pointsH"))
        h2d = nbytes / (load_ms["points_h2d"] * 1e-3) / 1e9 if load_ms["points_h2d"] > 0 else None
        ok = ok and rep["ok"] and ver["ok"] and aud["ok"]
        res["keys"][str(log)] = {"n_vars": sec["n_vars"], "domain": sec["domain"], "contribute": {"ms": ms_c, "split_ms": rep["ms"]},
                                 "delta_verify": {"ms": ms_v, "split_ms": ver["ms"]}, "check_key_ms": ms_a, "load_ms": load_ms,
                                 "bytes_moved": moved, "h2d_gb_s": h2d, "link_ms_of_bytes_moved": moved / (h2d * 1e9) * 1e3 if h2d else None}
    res["ok"] = bool(ok)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
