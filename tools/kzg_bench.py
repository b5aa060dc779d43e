#!/usr/bin/env python3
"""The KZG calls (csrc/kzg.hip) measured on the device (needs the GPU; bench.py is not involved).  Prints ONE JSON line per part and
writes the whole record to --out.  ONE process; every timed shape runs once unrecorded first; variants that are compared alternate
--reps times; recorded: medians with min and max, the device and its clock.  Times are host clocks around calls that end in a drained
queue (the division's value and every sum come back to the host; wsnark_fr_mul_dev is followed by a device synchronise).
  division   the three launches (wsnark_fr_poly_divide_dev, resident input and output) against wsnark_fr_mul_dev at the same n,
             2^20, 2^22 and 2^24: both move 96 bytes per element.  The ratio, its budget of 1.5 at 2^24, and -- from a pass of its own
             with the library's kernel timer on -- the time of each launch.  Parity in the same run: y and every q[k] against Python
             integers at 2^20; above that y = f[0] + z q[0] and q[k - 1] = f[k] + z q[k] at 4096 sampled k.
  open       wsnark_kzg_open[_dev] at count 1 and 8, len = n = 2^--log, against wsnark_points_msm_dev over the same powers: open's time,
             the share of it that is not the sum (device inputs), the upload (host inputs minus device inputs).  Parity: values and
             proof in closed form from the known tau; at count 8 polynomials 1 .. 7 have 1024 non-zero coefficients (the kernels' work
             does not depend on the values; the Python yardstick's does).
  commit     len = n / 2, n / 4, n / 8, n / 16 on both paths (KZG_PAD_PCT 0: padded into the table sum, 101: the prefix sum); the
             crossover the library's default then encodes.  Same bytes on both paths, checked.
  verify     wsnark_kzg_verify (count 1 and 8) beside wsnark_groth16_verify on the committed t6 key, ms per call on the host CPU.
    python tools/kzg_bench.py [--log 20] [--reps 7] [--out profiles/kzg_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
TAU = 0x1D2C3B4A5968778695A4B3C2D1E0F00112233445566778899AABBCCDDEEFF01 % R
le = lambda v: int(v).to_bytes(32, "little")


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "all_ms": ms}


def clock(fn, sync):
    t = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t) * 1e3


def horner(f, z):
    acc = 0
    for c in reversed(f):
        acc = (acc * z + c) % R
    return acc


def quotient(f, z):
    q, acc = [0] * (len(f) - 1), 0
    for k in range(len(f) - 1, 0, -1):
        acc = (f[k] + z * acc) % R
        q[k - 1] = acc
    return q, (f[0] + z * acc) % R


def random_scalars(rnd, n):
    """n values below r as bytes: 248 random bits each"""
    import numpy as np
    a = np.random.default_rng(rnd.randrange(1 << 32)).integers(0, 256, (n, 32), dtype=np.uint8)
    a[:, 31] = 0
    return a.tobytes()


def ints(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def part_division(bn, torch, reps, say, logs=(20, 22, 24)):
    c = bn.lib.c
    sync = torch.cuda.synchronize
    rnd = random.Random(1)
    rows, ok = {}, True
    z = rnd.randrange(R)
    for log in logs:
        n = 1 << log
        fb = random_scalars(rnd, n)
        d_f = torch.frombuffer(bytearray(fb), dtype=torch.uint8).cuda()
        d_b = torch.frombuffer(bytearray(random_scalars(rnd, n)), dtype=torch.uint8).cuda()
        d_q = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
        y = (C.c_uint8 * 32)()
        div = lambda: bn.lib.check(c.wsnark_fr_poly_divide_dev(d_f.data_ptr(), n, le(z), d_q.data_ptr(), y, None))
        mul = lambda: bn.lib.check(c.wsnark_fr_mul_dev(d_f.data_ptr(), d_b.data_ptr(), d_q.data_ptr(), n, None))
        t_div, t_mul = [], []
        for rnd_i in range(reps + 1):
            a, b = clock(mul, sync), clock(div, sync)      # (the division last: d_q holds the quotient for the parity check)
            if rnd_i:
                t_mul.append(a)
                t_div.append(b)
        q = bytes(d_q.cpu().numpy().tobytes())[:32 * (n - 1)]
        yv = int.from_bytes(bytes(y), "little")
        if log <= 20:
            wq, wy = quotient(ints(fb), z)
            good = yv == wy and q == b"".join(le(v) for v in wq)
        else:
            at = lambda b, k: int.from_bytes(b[32 * k:32 * k + 32], "little")
            ks = [1, 2, n - 1, n - 2] + [rnd.randrange(1, n - 1) for _ in range(4092)]
            good = yv == (at(fb, 0) + z * at(q, 0)) % R and at(q, n - 2) == at(fb, n - 1) and all(
                at(q, k - 1) == (at(fb, k) + z * at(q, k)) % R for k in ks if k < n - 1)
        ok = ok and good
        # the launches one by one: a pass of its own with the library's kernel timer on
        c.wsnark_timing_enable(1)
        c.wsnark_timing_reset()
        for _ in range(3):
            div()
        rep = bn.lib.timing_report()
        c.wsnark_timing_enable(0)
        launches = {k: rep[k][0] / rep[k][1] for k in ("kzg_tile", "kzg_carry", "kzg_quotient") if k in rep}
        row = {"n": n, "divide": stats(t_div), "fr_mul": stats(t_mul), "ratio": statistics.median(t_div) / statistics.median(t_mul),
               "bytes_per_element": 96, "divide_gb_per_s": 96 * n / statistics.median(t_div) / 1e6, "launch_ms": launches, "parity": bool(good)}
        if log == 24:
            row["budget"] = 1.5
            row["within_budget"] = row["ratio"] <= 1.5
            if not row["within_budget"] and launches:
                row["largest_launch"] = max(launches, key=launches.get)
        rows[str(log)] = row
        say("division", log, row["ratio"], launches)
        del d_f, d_b, d_q
    return rows, ok


def part_open_commit(bn, torch, log, reps, say):
    c = bn.lib.c
    sync = torch.cuda.synchronize
    n = 1 << log
    rnd = random.Random(2)
    t = time.perf_counter()
    tp, acc = [], 1
    for _ in range(n):
        tp.append(acc)
        acc = acc * TAU % R
    tau_g1 = bn.mul_base(1, b"".join(le(v) for v in tp))
    srs, pts = bn.load_srs(tau_g1), bn.load_points(1, tau_g1)
    say("reference string of 2^%d" % log, time.perf_counter() - t, "s", srs.info())
    point = lambda lg: bn.mul_base(1, le(lg % R))
    tau_eval = lambda f: sum(cf * p for cf, p in zip(f, tp)) % R
    # polynomial 0 dense, 1 .. 7 with 1024 non-zero coefficients
    f0 = random_scalars(rnd, n)
    sparse = [random_scalars(rnd, 1024) + bytes(32 * (n - 1024)) for _ in range(7)]
    polys = [f0] + sparse
    z, gamma = rnd.randrange(R), rnd.randrange(R)
    res, ok = {"n": n, "srs": srs.info()}, True
    d_all = torch.frombuffer(bytearray(b"".join(polys)), dtype=torch.uint8).cuda()
    d_sc = torch.frombuffer(bytearray(random_scalars(rnd, n)), dtype=torch.uint8).cuda()
    msm = lambda: pts.multiexp_dev(d_sc.data_ptr(), n)
    for count in (1, 8):
        blob = b"".join(polys[:count])
        gm = gamma if count > 1 else None
        host = lambda: srs._open(c.wsnark_kzg_open, blob, n, count, z, gm, ())      # (the joined bytes: no copy on the Python side)
        dev = lambda: srs.open_dev(d_all.data_ptr(), n, count, z, gm)
        t_host, t_dev, t_msm = [], [], []
        for rnd_i in range(reps + 1):
            a, b, m = clock(host, sync), clock(dev, sync), clock(msm, sync)
            if rnd_i:
                t_host.append(a)
                t_dev.append(b)
                t_msm.append(m)
        # parity: the closed form from tau
        fi = [ints(p[:32 * (n if i == 0 else 1024)]) for i, p in enumerate(polys[:count])]
        F = list(fi[0])
        for i in range(1, count):
            g = pow(gamma, i, R)
            for k, v in enumerate(fi[i]):
                F[k] = (F[k] + g * v) % R
        want_ys = [le(horner(f, z)) for f in fi]
        want_pi = point(tau_eval(quotient(F, z)[0]))
        got_h, got_d = host(), dev()
        good = got_h == got_d == (want_ys, want_pi)
        cs = srs.commit_dev(d_all.data_ptr(), n, count)
        good = good and cs == [point(tau_eval(f)) for f in fi]
        ok = ok and good
        md, mm, mh = statistics.median(t_dev), statistics.median(t_msm), statistics.median(t_host)
        res["open_count_%d" % count] = {"host_inputs": stats(t_host), "device_inputs": stats(t_dev), "points_msm_dev": stats(t_msm),
                                        "not_the_sum_ms": md - mm, "not_the_sum_share": (md - mm) / md, "upload_ms": mh - md,
                                        "upload_bytes": len(blob), "parity": bool(good)}
        say("open", count, md, mm, mh)
        res["_verify_case_%d" % count] = (tau_g1[:64], cs, z, got_d[0], got_d[1], gamma if count > 1 else None)
    # commit at len < n on both paths
    commit = {}
    for shift in (1, 2, 3, 4):
        ln = n >> shift
        times = {0: [], 101: []}
        got = {}
        for rnd_i in range(reps + 1):
            for pct in (0, 101):
                bn.lib.tune("KZG_PAD_PCT", pct)
                t0 = time.perf_counter()
                got[pct] = srs.commit_dev(d_all.data_ptr(), ln, 1)
                sync()
                if rnd_i:
                    times[pct].append((time.perf_counter() - t0) * 1e3)
        bn.lib.tune("KZG_PAD_PCT", None)
        same = got[0] == got[101] == [point(tau_eval(ints(f0[:32 * ln])))]
        ok = ok and same
        commit["n/%d" % (1 << shift)] = {"len": ln, "padded_table_sum": stats(times[0]), "prefix_sum": stats(times[101]),
                                         "padded_faster": statistics.median(times[0]) < statistics.median(times[101]), "same_bytes": bool(same)}
        say("commit", ln, statistics.median(times[0]), statistics.median(times[101]))
    full = [clock(lambda: srs.commit_dev(d_all.data_ptr(), n, 1), sync) for _ in range(reps + 1)][1:]
    commit["n"] = {"len": n, "table_sum": stats(full)}
    res["commit"] = commit
    return res, ok


def part_verify(bn, cases, reps):
    g2_pair = bn.mul_base(2, le(1) + le(TAU))
    gold = os.path.join(ROOT, "tests", "golden")
    vk = json.load(open(os.path.join(gold, "keys", "t6.vk.json")))
    pub = json.load(open(os.path.join(gold, "keys", "t6.public.json")))
    proof = json.load(open(os.path.join(gold, "proofs.json")))["t6"][1]["proof"]
    out, ok = {}, True
    for count, (g1, cs, z, ys, pi, gamma) in cases.items():
        good = bn.kzg_verify(g1, g2_pair, cs, z, ys, pi, gamma) is True and bn.kzg_verify(g1, g2_pair, cs, (z + 1) % R, ys, pi, gamma) is False
        ok = ok and good
        ms = [clock(lambda: bn.kzg_verify(g1, g2_pair, cs, z, ys, pi, gamma), lambda: None) for _ in range(reps + 1)][1:]
        out["kzg_verify_count_%d" % count] = dict(stats(ms), verdicts_as_expected=bool(good))
    good = bool(bn.groth16Verify(vk, pub, proof))
    ms = [clock(lambda: bn.groth16Verify(vk, pub, proof), lambda: None) for _ in range(reps + 1)][1:]
    out["groth16_verify_t6"] = dict(stats(ms), accepted=good)
    return out, ok and good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="", help="recorded as it is (a copy of the tree that is no git checkout cannot tell)")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "kzg_bench needs a GPU: nothing here is measured without one"
    import wasmsnark_amd
    from circuit_rows_bench import read_clock
    bn = wasmsnark_amd.build(device=0)
    say = lambda *x: print(*x, file=sys.stderr, flush=True)
    try:
        commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, timeout=30).stdout.strip() or "not a git checkout"
    except Exception:      # noqa: BLE001
        commit = "not read"
    res = {"device": bn.device_info, "clock": read_clock(), "commit": commit, "reps": a.reps, "ok": True}
    res["division"], ok = part_division(bn, torch, a.reps, say)
    res["ok"] = res["ok"] and ok
    print(json.dumps({"division": res["division"]}), flush=True)
    oc, ok = part_open_commit(bn, torch, a.log, a.reps, say)
    cases = {cnt: oc.pop("_verify_case_%d" % cnt) for cnt in (1, 8)}
    res["open_commit"] = oc
    res["ok"] = res["ok"] and ok
    print(json.dumps({"open_commit": oc}), flush=True)
    res["verify"], ok = part_verify(bn, cases, a.reps)
    res["ok"] = res["ok"] and ok
    print(json.dumps({"verify": res["verify"]}), flush=True)
    res["clock_after"] = read_clock()
    assert res["ok"], "a result differed from its closed form: no profile is written"
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
