#!/usr/bin/env python3
"""Compressed points and proofs on the GPU (needs the GPU; bench.py is not involved).  Prints ONE JSON line and writes it to --out.
All in the SAME process, kernel times from wsnark_timing_report, medians of --reps calls after a warm-up:
  g1_decompress / g2_decompress   at 2^20 and 2^18 points: points/s, the fraction of the multiplier peak (wsnark_peak_probe(0)) at
                        products_per_point field products per point (a COUNT from the formulas: the windowed chain is 14 + 248 + 56 = 318,
                        the curve equation, the conversions, the sign and the check 8 more; G2 runs two chains and about 18 more), and ratio_to_inversion: the time per point over the time of ONE field inversion
                        per lane (wsnark_peak_probe(5)).  Budgets: 1.25 (G1), 3.5 (G2); reported, not gated.
  g1_compress / g2_compress       the bytes they read per second over a streaming read's (wsnark_peak_probe(4)); no budget.
  verify                groth16VerifyBatchCompressed against groth16VerifyBatch on the same 4096 and 16384 forged proofs, whole call on
                        the host clock, and their ratio.
The tool asserts that every decompressed point is the point that was compressed, byte for byte, and that both verifiers give the
same statuses.
    python tools/point_codec_bench.py [--reps 5] [--out profiles/point_codec_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

PRODUCTS = {1: 326, 2: 654}
BUDGET = {1: 1.25, 2: 3.5}


def probe(lib, which):
    v = C.c_double(0)
    lib.check(lib.c.wsnark_peak_probe(which, C.byref(v)))
    return v.value


def kernel_ms(lib, fn, name, reps):
    """median over reps (after one warm-up) of the summed kernel time `name` of one call of fn"""
    out, ms = None, []
    for k in range(reps + 1):
        lib.c.wsnark_timing_reset()
        lib.c.wsnark_timing_enable(1)
        out = fn()
        lib.c.wsnark_timing_enable(0)
        if k:
            ms.append(lib.timing_report()[name][0])
    return out, statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import wasmsnark_amd
    import verify_batch_common as vb
    bn = wasmsnark_amd.build(device=0)
    lib = bn.lib
    rnd = random.Random(12)
    peak, inv, stream = probe(lib, 0), probe(lib, 5), probe(lib, 4)
    res = {"device": bn.device_info, "reps": a.reps, "peak_gproducts_per_s": peak, "ginversions_per_s": inv, "stream_read_gb_per_s": stream,
           "budget_ratio_to_inversion": {"g1": BUDGET[1], "g2": BUDGET[2]}, "points": {}}
    for g in (1, 2):
        for log in (18, 20):
            n = 1 << log
            pts = bn.mul_base(g, b"".join(rnd.randrange(1, vb.R).to_bytes(32, "little") for _ in range(n)))
            (data, st), ms_c = kernel_ms(lib, lambda: bn.compress_points(g, pts, "le"), "g%d_compress" % g, a.reps)
            assert st == [0] * n
            (back, st), ms_d = kernel_ms(lib, lambda: bn.decompress_points(g, data, "le"), "g%d_decompress" % g, a.reps)
            assert st == [0] * n and back == pts, "decompress(compress(P)) != P"
            per_s = n / (ms_d * 1e-3)
            res["points"]["g%d_2^%d" % (g, log)] = {
                "decompress_ms": ms_d, "points_per_s": per_s, "products_per_point": PRODUCTS[g],
                "fraction_of_peak": per_s * PRODUCTS[g] / (peak * 1e9), "ratio_to_inversion": (ms_d * 1e-3 / n) * inv * 1e9,
                "compress_ms": ms_c, "compress_read_gb_per_s": n * 64 * g / (ms_c * 1e-3) / 1e9,
                "compress_fraction_of_stream": n * 64 * g / (ms_c * 1e-3) / 1e9 / stream}
            print(g, log, res["points"]["g%d_2^%d" % (g, log)], file=sys.stderr)
    # the two verifiers on the same forged proofs
    F = vb.Forger(bn, 3, seed=31)
    vkb = F.vk_bytes()
    ib, pb = F.forge(16384)
    # 5 % invalid: A negated (a point of the curve still, so the compressed proof is the same proof)
    tp, want = bytearray(pb), {}
    for i in sorted(rnd.sample(range(16384), 16384 // 20)):
        y = int.from_bytes(tp[384 * i + 32:384 * i + 64], "little")
        tp[384 * i + 32:384 * i + 64] = (vb.Q - y).to_bytes(32, "little")
        want[i] = 0
    tp = bytes(tp)
    out128 = (C.c_uint8 * (128 * 16384))()
    cst = (C.c_uint8 * 16384)()
    lib.check(lib.c.wsnark_proof_compress(tp, 16384, 1, out128, cst))
    assert list(cst) == [1] * 16384
    comp = bytes(out128)
    res["verify"] = {}
    for n in (4096, 16384):
        t_plain, t_comp = [], []
        for k in range(a.reps + 1):
            s1, s2 = (C.c_uint8 * n)(), (C.c_uint8 * n)()
            t = time.perf_counter()
            lib.check(lib.c.wsnark_groth16_verify_batch(vkb, len(vkb), ib, 3, tp, n, s1))
            t1 = time.perf_counter()
            lib.check(lib.c.wsnark_groth16_verify_batch_compressed(vkb, len(vkb), ib, 3, comp, n, 1, s2))
            t2 = time.perf_counter()
            if k:
                t_plain.append((t1 - t) * 1e3)
                t_comp.append((t2 - t1) * 1e3)
            assert list(s1) == list(s2) == [want.get(i, 1) for i in range(n)], "the two verifiers differ"
        mp, mc = statistics.median(t_plain), statistics.median(t_comp)
        res["verify"][str(n)] = {"verify_batch_ms": mp, "verify_batch_compressed_ms": mc, "ratio": mc / mp, "compressed_proofs_per_s": n / (mc * 1e-3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
