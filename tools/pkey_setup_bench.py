#!/usr/bin/env python3
"""The key setup from powers of tau on the GPU (needs the GPU; bench.py is not involved).  Prints ONE JSON line:
  transform[log][G1|G2]   wsnark_g{1,2}_ntt (forward: no 1/n pass) at n = 2^log points: the sum of the call's stage kernels
                          (wsnark_timing_report, names group_ntt_g*_uniform / _lane; median of --reps calls after a warm-up): ONE
                          twiddle per wavefront while a stage has 64 blocks (uniform_stages_ms), then per-lane digits in block order
                          (late_stages_ms = the last six stages alone); butterflies per second = (n/2) log2 n / kernel time
  yardstick[G1|G2]        scale_points_kernel in the same process and with the same timer: one scalar for all lanes, the best this
                          multiplication can do, in points per second; ratio = butterflies/s over points/s (the kernel is linear in its
                          point count, so the rate stands for "the same count")
  keys[log]               setup_key end to end from host memory with its own ms[] split, the column sums with PKSETUP_MSM_MIN at its
                          default, off (0) and 2, beside contribute_key, check_key and load_key of the same key.  The key is checked:
                          after a contribution by the generator's delta it must equal the generator's own key byte for byte.
  sha256                  of the output bytes of every timed call that returns bytes, by the call's name: the inputs are seeded, so two
                          builds of the library that compute the same print the same digests
    python tools/pkey_setup_bench.py [--logs 16,20] [--key-logs 20] [--reps 5] [--out profiles/pkey_setup_bench.json]
"""
import argparse
import hashlib
import json
import os
import random
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = 1 << 256


def native_inputs(bn, log, seed):
    """(powers, circuit blobs, the generator's own key sections, its delta) of a NativeCircuit: tau, alpha, beta, delta read back from
    the generator's key scalars (hExps_1 / hExps_0 = tau); the C matrix of the "columns" family: row c holds 1 x its output variable."""
    import ctypes as C
    from wasmsnark_amd import synth
    lib = bn.lib
    nc = synth.NativeCircuit(lib, log, n_public=2, seed=seed)
    sec = nc.build_sections()[0]
    nv, npub, dom = nc.n_vars, nc.n_public, nc.domain
    s1 = bytearray(nc.info.n_g1_scalars * 32)
    lib.check(lib.c.wsnark_synth_key_scalars(nc._h, 1, nc._cbuf(s1)))
    val = lambda i: int.from_bytes(s1[32 * i:32 * i + 32], "little")
    alpha, beta, delta = val(0), val(1), val(2)
    oh = 3 + 2 * nv + (nv - npub - 1)
    tau = val(oh + 1) * pow(val(oh), -1, R) % R
    polsA, polsB = bytes(sec["polsA"]), bytes(sec["polsB"])
    nc.free()
    tp = [1] * (2 * dom)
    for k in range(1, 2 * dom):
        tp[k] = tp[k - 1] * tau % R
    cat = lambda xs: b"".join(int(x).to_bytes(32, "little") for x in xs)
    powers = {"domain": dom,
              "tau_g1": bn.mul_base(1, cat(tp)),
              "alpha_tau_g1": bn.mul_base(1, cat(alpha * t % R for t in tp[:dom])),
              "beta_tau_g1": bn.mul_base(1, cat(beta * t % R for t in tp[:dom])),
              "tau_g2": bn.mul_base(2, cat(tp[:dom])),
              "beta_g2": bn.mul_base(2, cat([beta]))}
    n_free = npub + 2
    one = (MONT % R).to_bytes(32, "little")
    polsC = struct.pack("<I", 0) * (1 + n_free) + b"".join(struct.pack("<II", 1, c) + one for c in range(nv - 1 - n_free))
    circuit = {"n_vars": nv, "n_public": npub, "domain": dom, "polsA": polsA, "polsB": polsB, "polsC": polsC}
    return powers, circuit, sec, delta


def sha256_of(out):
    """SHA-256 over the bytes a call returned: bytes themselves, the values of a dict in the order of its names (a key's sections), the
    items of a tuple or list in order; anything else (a report with its times, a count) is left out"""
    h = hashlib.sha256()

    def walk(x):
        if isinstance(x, (bytes, bytearray, memoryview)):
            h.update(x)
        elif isinstance(x, dict):
            for k in sorted(x):
                walk(x[k])
        elif isinstance(x, (tuple, list)):
            for v in x:
                walk(v)
    walk(out)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--key-logs", default="", help="the sizes of keys[log] where they are not those of transform[log]")
    a = ap.parse_args()
    import wasmsnark_amd
    bn = wasmsnark_amd.build(device=0)
    lib = bn.lib
    rnd = random.Random(17)
    logs = [int(x) for x in a.logs.split(",")]
    res = {"device": bn.device_info, "clock": "not read", "reps": a.reps, "transform": {}, "yardstick": {}, "keys": {}, "sha256": {}}
    ok = True

    def kernel_ms(name, fn, *prefixes):
        """one figure per prefix: the median over the calls of the summed times of the kernels whose names start with it"""
        out = [[] for _ in prefixes]
        for i in range(a.reps + 1):
            lib.c.wsnark_timing_reset(); lib.c.wsnark_timing_enable(1)
            got = fn()
            rep = lib.timing_report()
            lib.c.wsnark_timing_enable(0)
            for o, p in zip(out, prefixes):
                if i:
                    o.append(sum(v[0] for kk, v in rep.items() if kk.startswith(p)))
        res["sha256"][name] = sha256_of(got)
        return [(statistics.median(o), o) for o in out]

    say = lambda *x: print(*x, file=sys.stderr, flush=True)
    rate = lambda count, ms: count / (ms * 1e-3) if ms > 0 else None      # (the emulator's event timers read 0)
    pts = {}
    top = max(logs)
    for g in (1, 2):
        pts[g] = bn.mul_base(g, b"".join(rnd.randrange(1, R).to_bytes(32, "little") for _ in range(1 << top)))
        n_y = 1 << min(top, 20 if g == 1 else 18)
        sz = 64 * g
        k = rnd.randrange(1 << 253, R)
        (ms, all_ms), = kernel_ms("scale_points G%d" % g, lambda: bn.scale_points(g, pts[g][:n_y * sz], k), "scale_points_g%d" % g)
        res["yardstick"]["G%d" % g] = {"kernel": "scale_points_kernel<G%d>" % g, "n": n_y, "ms": ms, "all_ms": all_ms, "points_per_s": rate(n_y, ms)}
    for log in logs:
        n = 1 << log
        res["transform"][str(log)] = {}
        for g in (1, 2):
            data = pts[g][:n * 64 * g]
            row = {"butterflies": (n // 2) * log}
            (uni, uni_all), (late, late_all) = kernel_ms("group_ntt 2^%d G%d" % (log, g), lambda: bn.group_ntt(g, data),
                                                         "group_ntt_g%d_uniform" % g, "group_ntt_g%d_lane" % g)
            all_ms = [x + y for x, y in zip(uni_all, late_all)]
            ms = statistics.median(all_ms)
            row["shipped"] = {"ms": ms, "all_ms": all_ms, "butterflies_per_s": rate(row["butterflies"], ms), "uniform_stages_ms": uni,
                              "uniform_stages_all_ms": uni_all, "late_stages_ms": late, "late_stages_all_ms": late_all}
            if row["shipped"]["butterflies_per_s"] and res["yardstick"]["G%d" % g]["points_per_s"]:
                row["ratio_to_scale_points"] = row["shipped"]["butterflies_per_s"] / res["yardstick"]["G%d" % g]["points_per_s"]
            out = bn.group_ntt(g, data)
            t = time.perf_counter()
            back = bn.group_ntt(g, out, True)
            row["inverse_call_ms"] = (time.perf_counter() - t) * 1e3
            ok = ok and back == data
            res["transform"][str(log)]["G%d" % g] = row
            say("transform", log, "G%d" % g, ms)
    del pts

    def timed(fn, reps):
        if reps:
            fn()
        ts, last = [], None
        for _ in range(max(reps, 1)):
            t = time.perf_counter()
            last = fn()
            ts.append((time.perf_counter() - t) * 1e3)
        return statistics.median(ts), last

    for log in [int(x) for x in a.key_logs.split(",")] if a.key_logs else logs:
        powers, circuit, native, delta = native_inputs(bn, log, seed=log)
        say("inputs", log)
        reps = a.reps if log <= 16 else min(a.reps, 3)
        row = {"n_vars": circuit["n_vars"], "domain": circuit["domain"], "reps": reps, "column_sums": {}}
        keys = {}
        for mm, name in ((None, "default"), (0, "off"), (2, "2")):
            if name == "2" and log > 16:
                continue      # (every multi-record column as an MSM of its own: a 2^16 figure only)
            lib.tune("PKSETUP_MSM_MIN", mm)
            ms, (key, vk, rep) = timed(lambda: bn.setup_key(powers, circuit), reps if name != "2" else 0)      # ("2": one call, tens of seconds)
            keys[name] = key
            res["sha256"]["setup_key 2^%d msm_min=%s" % (log, name)] = sha256_of((key, vk))
            say("setup_key", log, name, ms)
            row["column_sums"][name] = {"ms": rep["ms"]["column_sums"], "msm_columns": rep["msm_columns"], "setup_key_ms": ms}
            if name == "default":
                row["setup_key"] = {"ms": ms, "split_ms": rep["ms"]}
        lib.tune("PKSETUP_MSM_MIN", None)
        new = keys["default"]
        ok = ok and all(k is not None and all(bytes(k[x]) == bytes(new[x]) for x in new if not isinstance(new[x], int)) for k in keys.values())
        ms_c, (that, rep_c) = timed(lambda: bn.contribute_key(sections=new, d=delta), reps)
        res["sha256"]["contribute_key 2^%d" % log] = sha256_of(that)
        ok = ok and rep_c["ok"] and all(bytes(that[x]) == bytes(native[x]) for x in native if not isinstance(native[x], int))
        ms_a, aud = timed(lambda: bn.check_key(sections=new), reps)
        ok = ok and aud["ok"]
        h = bn.load_key(sections=new)
        row["load_ms"] = dict(h.load_ms)
        h.free()
        row["contribute_key_ms"], row["check_key_ms"] = ms_c, ms_a
        res["keys"][str(log)] = row
    res["ok"] = bool(ok)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
