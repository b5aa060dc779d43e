#!/usr/bin/env python3
"""Powers of tau on the GPU (needs the GPU; bench.py is not involved).  Prints ONE JSON line:
  mul_kernel[G1|G2]   mul_points_kernel (fixed signed 4-bit windows) at n = 2^20 random valid points with random 254-bit scalars:
                      kernel ms per call (the sum of the call's chunk launches, wsnark_timing_report; median of --reps calls after a
                      warm-up), points/s, and on G1 the fraction of the multiplier peak (wsnark_peak_probe(0), same process) at
                      products_per_point field products per point
  between[G1|G2]      the two existing kernels this one sits between, same process, same timer, same scalars or points:
                      mul_base_kernel (one base, a scalar per lane) and scale_points_kernel (a base per lane, ONE scalar: the floor);
                      required: the G1 kernel is faster than mul_base_kernel<G1>
  transcripts[log]    contribute_powers and check_powers (points and relations separately) end to end from host memory with their own
                      ms[] splits, beside setup_key on the same transcript
  sha256              of the output bytes of every timed call that returns bytes, by the call's name (the inputs are seeded)
    python tools/pwtau_bench.py [--logs 16,20] [--reps 5] [--out profiles/pwtau_bench.json]
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
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
WIN = 4


def window_weight(k):
    """non-zero digits of k's signed 4-bit window form (digits in [-8, 8], a value above 8 carries)"""
    w = c = 0
    for j in range(256 // WIN):
        v = ((k >> (WIN * j)) & 15) + c
        c = 1 if v > 8 else 0
        w += 1 if v not in (0, 16) else 0
    return w


def products_per_point(ks):
    """Field products per finite G1 point, averaged over the scalars ks, squarings counted as products and the fused two-product Y3 as
    2, from curve.h's formulas as tools/pkey_delta_bench.py counts: to_internal 2, curve equation 3, doubling 9, affine doubling 7,
    mixed addition 11, full addition 14; the shared inversion 3 products per tree level and lane (8 + 16) and 1/4 of a Fermat chain;
    1 + 4 products around it, from_internal 2.
    windows: the table 7 + 6 x 11, then 63 x 4 doublings and one full addition per non-zero digit but the first (which meets infinity)."""
    dbl, mdbl, madd, add = 9, 7, 11, 14
    fermat = 253 + bin(Q - 2).count("1")
    around = 5 + 24 + fermat / 4 + 5 + 2
    ww = statistics.mean(window_weight(k) for k in ks)
    return {"doubling": dbl, "mixed_addition": madd, "full_addition": add, "window_digits_nonzero": ww,
            "windows": around + mdbl + 6 * madd + 63 * 4 * dbl + (ww - 1) * add}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-only", action="store_true", help="the shipped G1 kernel alone, a few calls: the run to put under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    import wasmsnark_amd
    from pkey_setup_bench import native_inputs, sha256_of
    bn = wasmsnark_amd.build(device=0)
    lib = bn.lib
    rnd = random.Random(13)
    res = {"device": bn.device_info, "clock": "not read", "chunk_points": 1 << 18, "reps": a.reps, "n": a.n}
    g = C.c_double(0)
    lib.check(lib.c.wsnark_peak_probe(0, C.byref(g)))
    res["peak_gmodmul_s"] = g.value
    n = a.n
    ks = [rnd.randrange(1 << 253, R) for _ in range(n)]
    scalars = b"".join(k.to_bytes(32, "little") for k in ks)
    k_one = rnd.randrange(1 << 253, R)
    res["products_per_point"] = products_per_point(ks[:4096])
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

    if a.kernel_only:
        pts = bn.mul_base(1, scalars)
        for _ in range(3):
            bn.mul_points(1, pts, scalars)
        print(json.dumps({"kernel_only": True, "n": n}))
        return

    rate = lambda ms: n / (ms * 1e-3) if ms > 0 else None      # (the emulator's timer reads 0: a dry run of this script)
    ratio = lambda x, y: x / y if y > 0 else None
    ok = True
    res["mul_kernel"], res["between"] = {}, {}
    for grp in (1, 2):
        name = "G%d" % grp
        pts = bn.mul_base(grp, scalars)
        mb, mb_all = kernel_ms("mul_base " + name, lambda: bn.mul_base(grp, scalars), "mul_base_g%d" % grp)
        sp, sp_all = kernel_ms("scale_points " + name, lambda: bn.scale_points(grp, pts, k_one), "scale_points_g%d" % grp)
        ms, all_ms = kernel_ms("mul_points " + name, lambda: bn.mul_points(grp, pts, scalars), "mul_points_g%d_win" % grp)
        row = {"shipped": {"mode": "win", "ms": ms, "all_ms": all_ms, "points_per_s": rate(ms)}}
        if grp == 1:
            ppp = res["products_per_point"]["windows"]
            row["shipped"]["products_per_point_used"] = ppp
            row["shipped"]["fraction_of_peak"] = ppp * rate(ms) / (g.value * 1e9) if ms > 0 else None
        res["mul_kernel"][name] = row
        res["between"][name] = {"mul_base_kernel": {"ms": mb, "all_ms": mb_all}, "scale_points_kernel": {"ms": sp, "all_ms": sp_all},
                                "ratio_shipped_over_mul_base": ratio(ms, mb), "ratio_shipped_over_scale_points": ratio(ms, sp)}
        ok = ok and (grp != 1 or ms < mb)
        del pts
    del scalars, ks

    def timed(fn, reps):
        fn()
        ts, last = [], None
        for _ in range(reps):
            t = time.perf_counter()
            last = fn()
            ts.append((time.perf_counter() - t) * 1e3)
        return statistics.median(ts), last

    res["transcripts"] = {}
    t, al, be = (rnd.randrange(1, R) for _ in range(3))
    for log in [int(x) for x in a.logs.split(",")]:
        powers, circuit, native, delta = native_inputs(bn, log, seed=log)
        reps = a.reps
        ms_c, (new, rep) = timed(lambda: bn.contribute_powers(powers, t, al, be), reps)
        res["sha256"]["contribute_powers 2^%d" % log] = sha256_of(new)
        ms_p, chk_p = timed(lambda: bn.check_powers(new, relations=False), reps)
        ms_r, chk_r = timed(lambda: bn.check_powers(new, points=False), reps)
        ms_s, (key, vk, srep) = timed(lambda: bn.setup_key(new, circuit), reps)
        res["sha256"]["setup_key 2^%d" % log] = sha256_of((key, vk))
        ok = ok and rep["ok"] and chk_p["ok"] and chk_r["ok"] and chk_r["relations_run"] == 63 and srep["ok"]
        res["transcripts"][str(log)] = {"domain": powers["domain"], "reps": reps, "contribute_powers": {"ms": ms_c, "split_ms": rep["ms"]},
                                        "check_powers_points": {"ms": ms_p, "split_ms": chk_p["ms"]},
                                        "check_powers_relations": {"ms": ms_r, "split_ms": chk_r["ms"]},
                                        "setup_key": {"ms": ms_s, "split_ms": srep["ms"]}}
        del powers, new, key
    res["ok"] = bool(ok)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
