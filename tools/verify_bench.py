#!/usr/bin/env python3
"""Batch verification on the GPU against the host verifier beside it (needs the GPU; bench.py is not involved).

Builds one synthetic key with known toxic waste, forges N valid proofs with distinct public inputs (the forger of
tests/verify_batch_common.py: three fixed-base multiplications per proof, no proving), tampers 5 % of them, and prints ONE JSON line:
  host_ms_per_proof_1thread / host_proofs_per_s_16threads   wsnark_groth16_verify (each thread its own proofs; ctypes drops the GIL)
  batch[N]              wsnark_groth16_verify_batch end to end from host memory: ms and proofs per second, N = 1 .. 16384
  batch_dev_4096        the same from device memory
  kernels_4096 / kernels_16384 / kernels_4096_plain_exp / kernels_4096_hard_bit_by_bit      per-kernel ms of one call (wsnark_timing_report)
  plain_exp_4096        the call with the final exponentiation by the plain exponent (WSNARK_VERIFY_PLAIN_EXP=1; =2: split, but
                        the hard part bit by bit with ordinary squarings)
  peak_gmodmul_s, products_per_proof, fraction_of_peak_16384    against the multiplier peak measured in the same run
  statuses_ok           every status of every size equals the construction, and a 64-proof sample equals the host call
    python tools/verify_bench.py [--out profiles/verify_batch_bench.json]
    python tools/verify_bench.py --one 4096        # two calls of that size and nothing else: the run to put under rocprofv3
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
N_PUBLIC = 3


def product_counts(n_inputs):
    """Base-field multiplier calls per proof of the shipped path, from the formulas of pairing.hip / fp12.h / curve.h, by phase:
    (single products and squarings, fused double products mul2add, fused four-product reductions mul4add).  An Fq2 product is
    2 mul2add, an Fq2 squaring 2 products, a scaling by an Fq element 2 products, mulsub2 in Fq2 2 mul4add (in Fq 1 mul2add).
    Inputs are taken as uniform: half of their 254 bits set."""
    pc = lambda v: bin(v).count("1")
    add = lambda *xs: tuple(sum(c) for c in zip(*xs))
    mul = lambda k, x: tuple(k * c for c in x)
    F2MUL, F2SQR, SCALE = (0, 2, 0), (2, 0, 0), (2, 0, 0)
    f12_mul, f12_sqr, line = mul(36, F2MUL), add(mul(15, F2MUL), mul(6, F2SQR)), mul(18, F2MUL)
    fermat = (254 + pc(P - 2), 0, 0)                                          # Fq29::inv: a squaring per bit, a product per set bit
    # prepare: curve equations; [r] B (XYZZ doubling: 2 S + 5 M + mulsub2; full addition: 2 S + 11 M + mulsub2, in Fq2);
    # IC(x) (G1 XYZZ doubling 2 S + 5 M + mulsub2, mixed addition 2 S + 7 M + mulsub2) and its affine form
    g2_dbl = add(mul(2, F2SQR), mul(5, F2MUL), (0, 0, 2))
    g2_add = add(mul(2, F2SQR), mul(11, F2MUL), (0, 0, 2))
    g1_dbl, g1_madd = (7, 1, 0), (9, 1, 0)
    prepare = add(mul(12, (1, 0, 0)), (4, 0, 0), add(mul(2, F2SQR), F2MUL),
                  mul(254, g2_dbl), mul(pc(R), g2_add),
                  mul(254, g1_dbl), mul(127 * n_inputs + 1, g1_madd), fermat, (5, 0, 0))
    # Miller: per bit of T one squaring of f, B's doubling (5 S + 6 M + 2 scalings) and three lines (two of them stored: a
    # scaling each); per set bit B's addition (3 S + 10 M + 2 scalings) and three lines; then f * m(-alfa1, beta2)
    T = P - R
    per_bit = add(f12_sqr, mul(5, F2SQR), mul(6, F2MUL), mul(4, SCALE), mul(3, line))
    per_add = add(mul(3, F2SQR), mul(10, F2MUL), mul(4, SCALE), mul(3, line))
    miller = add(mul(126, per_bit), mul(pc(T) - 1, per_add), f12_mul)
    # final exponentiation: inversion (2 Fp12 products, the Fp6 inverse: 9 M + 3 S + an Fq2 inverse = 2 S + Fermat + 2 M in Fq),
    # conj(f) / f, Frobenius (10 products), one more product; then the hard part through the curve's parameter x (63 bits): three
    # powers of x on cyclotomic squarings (6 Fq2 products each), then 13 products, 4 cyclotomic squarings, 5 p-Frobenius maps
    # (5 Fq2 products) and 2 p^2-Frobenius maps (10 products)
    hard = (P ** 4 - P ** 2 + 1) // R
    easy = add(mul(4, f12_mul), mul(9, F2MUL), mul(3, F2SQR), (4, 0, 0), fermat, (10, 0, 0))
    lo, hi = 1, 1 << 64                      # x: the root of p = 36 x^4 + 36 x^3 + 24 x^2 + 6 x + 1 (tools/gen_pairing_consts.py)
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (mid + 1, hi) if 36 * mid ** 4 + 36 * mid ** 3 + 24 * mid ** 2 + 6 * mid + 1 < P else (lo, mid)
    x = lo
    cyc_sqr = mul(6, F2MUL)
    finalexp = add(easy, mul(3 * (x.bit_length() - 1) + 4, cyc_sqr), mul(3 * (pc(x) - 1) + 13, f12_mul), mul(25, F2MUL), (20, 0, 0))
    finalexp_bits = add(easy, mul(hard.bit_length() - 1, f12_sqr), mul(pc(hard) - 1, f12_mul))
    plain = (P ** 12 - 1) // R
    finalexp_plain = add(mul(plain.bit_length() - 1, f12_sqr), mul(pc(plain) - 1, f12_mul))
    # in units of ONE product (162 multiply-adds): a fused double product is 243 of them, a four-product reduction 405
    eq = lambda x: x[0] + 1.5 * x[1] + 2.5 * x[2]
    out = {}
    for k, v in (("prepare", prepare), ("miller", miller), ("finalexp", finalexp), ("finalexp_hard_bit_by_bit", finalexp_bits), ("finalexp_plain", finalexp_plain)):
        out[k] = {"mul_sqr": v[0], "mul2add": v[1], "mul4add": v[2], "product_equivalents": eq(v)}
    out["total_product_equivalents"] = eq(prepare) + eq(miller) + eq(finalexp)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,1024,4096,16384")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--one", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    import torch
    import wasmsnark_amd
    import verify_batch_common as vb
    bn = wasmsnark_amd.build(device=0)
    lib = bn.lib
    nmax = max(sizes + [a.one, 4096])
    F = vb.Forger(bn, N_PUBLIC, seed=31)
    vkb = F.vk_bytes()
    ib, pb = F.forge(nmax)
    rnd = random.Random(8)
    tp, want = vb.tamper(pb, sorted(rnd.sample(range(nmax), nmax // 20)), rnd)
    isz = 32 * N_PUBLIC

    def call(n, dev=None):
        st = (C.c_uint8 * n)()
        t = time.perf_counter()
        if dev is None:
            rc = lib.c.wsnark_groth16_verify_batch(vkb, len(vkb), ib, N_PUBLIC, tp, n, st)
        else:
            rc = lib.c.wsnark_groth16_verify_batch_dev(vkb, len(vkb), dev[0].data_ptr(), N_PUBLIC, dev[1].data_ptr(), n, st, None)
        dt = time.perf_counter() - t
        lib.check(rc)
        return dt, list(st)

    if a.one:
        call(a.one)
        dt, st = call(a.one)
        print(json.dumps({"n": a.one, "ms": dt * 1e3, "ok": st == [want.get(i, 1) for i in range(a.one)]}))
        return

    def host(i):
        return vb.host_status(lib, vkb, N_PUBLIC, ib[isz * i:isz * (i + 1)], tp[384 * i:384 * i + 384])

    res = {"n_public": N_PUBLIC, "device": bn.device_info, "tampered_fraction": 0.05}
    ok = True
    # the host verifier: one thread, then `threads` threads with their own proofs
    valid = [i for i in range(nmax) if i not in want]
    t = time.perf_counter()
    for i in valid[:16]:
        ok = ok and host(i) == 1
    res["host_ms_per_proof_1thread"] = (time.perf_counter() - t) / 16 * 1e3
    per = 8
    with ThreadPoolExecutor(a.threads) as ex:
        t = time.perf_counter()
        outs = list(ex.map(lambda k: [host(i) for i in valid[16 + per * k:16 + per * (k + 1)]], range(a.threads)))
        dt = time.perf_counter() - t
    ok = ok and all(v == 1 for o in outs for v in o)
    res["host_threads"] = a.threads
    res["host_proofs_per_s_%dthreads" % a.threads] = a.threads * per / dt
    # the batch call
    res["batch"] = {}
    call(4096)
    for n in sizes:
        runs = [call(n) for _ in range(3)]
        best = min(r[0] for r in runs)
        ok = ok and all(r[1] == [want.get(i, 1) for i in range(n)] for r in runs)
        res["batch"][str(n)] = {"ms": best * 1e3, "proofs_per_s": n / best}
    dev = (torch.frombuffer(bytearray(ib), dtype=torch.uint8).cuda(), torch.frombuffer(bytearray(tp), dtype=torch.uint8).cuda())
    torch.cuda.synchronize()
    runs = [call(4096, dev) for _ in range(3)]
    ok = ok and all(r[1] == [want.get(i, 1) for i in range(4096)] for r in runs)
    best = min(r[0] for r in runs)
    res["batch_dev_4096"] = {"ms": best * 1e3, "proofs_per_s": 4096 / best}
    # a 64-proof sample (half tampered) against the host call
    sample = rnd.sample(sorted(i for i in want if i < 4096), 32) + rnd.sample([i for i in range(4096) if i not in want], 32)
    st = call(4096)[1]
    ok = ok and all(host(i) == st[i] for i in sample)

    def kernels(n):
        lib.c.wsnark_timing_reset(); lib.c.wsnark_timing_enable(1)
        call(n)
        rep = lib.timing_report()
        lib.c.wsnark_timing_enable(0)
        return {k: v[0] for k, v in rep.items() if k.startswith("verify_")}

    res["kernels_4096"] = kernels(4096)
    res["kernels_16384"] = kernels(16384) if nmax >= 16384 else None
    lib.tune("VERIFY_PLAIN_EXP", 1)
    runs = [call(4096) for _ in range(2)]
    ok = ok and all(r[1] == [want.get(i, 1) for i in range(4096)] for r in runs)
    best = min(r[0] for r in runs)
    res["plain_exp_4096"] = {"ms": best * 1e3, "proofs_per_s": 4096 / best}
    res["kernels_4096_plain_exp"] = kernels(4096)
    lib.tune("VERIFY_PLAIN_EXP", 2)
    ok = ok and call(4096)[1] == [want.get(i, 1) for i in range(4096)]
    res["kernels_4096_hard_bit_by_bit"] = kernels(4096)
    lib.tune("VERIFY_PLAIN_EXP", None)
    g = C.c_double(0)
    lib.check(lib.c.wsnark_peak_probe(0, C.byref(g)))
    res["peak_gmodmul_s"] = g.value
    pcnt = product_counts(N_PUBLIC)
    res["products_per_proof"] = pcnt
    if "16384" in res["batch"]:
        n_run = 16384 - 16384 // 20         # the tampered proofs leave after the first kernel
        res["fraction_of_peak_16384"] = pcnt["total_product_equivalents"] * n_run / (res["batch"]["16384"]["ms"] * 1e-3) / (g.value * 1e9)
    res["statuses_ok"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
