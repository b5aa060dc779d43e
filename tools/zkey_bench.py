#!/usr/bin/env python3
"""snarkjs' .zkey in and out on the GPU (needs the GPU; bench.py is not involved).  Prints ONE JSON line per size; on ONE key of the
native generator's "columns" family (csrc/synth.hip, style 0: the bench's C4 circuit) at log2(domain) = --log, all in the SAME process:
  export / import       wsnark_zkey_export and wsnark_zkey_import: the report's own ms (parse + upload, coefficients, H basis, download,
                        whole call) and the host clock around Bn128.export_zkey / import_zkey, medians of --reps calls after a warm-up.
                        The file that is imported is the one the export wrote: there is no snarkjs-written file to measure.
  load_key / check_key  the same key through the loader and the audit, host clock, as the other README rows have them
  h_basis_kernels       per-kernel times from wsnark_timing_report of one wsnark_g1_h_basis call (load, twiddles, stages, fr_powers,
                        mul_points) beside the STAGE kernels of one wsnark_g1_ntt call of the same size.  ratio_to_ntt_stages: the first
                        sum / the second; expected ~1.12 from profiles/pkey_setup_bench.json and profiles/pwtau_bench.json, budget 1.2.
  composition           what a caller could do before this entry point existed, through host memory: group_ntt + mul_points on the H
                        section (the twist scalars computed on the host are NOT counted) + circuit_from_rows on the same coefficients
                        (rows derived on the host are NOT counted either).  ratio_import_to_composition: expected <= 1.
The tool asserts that the imported key's streams are the generator's with every column sorted by constraint, that every point section
comes back byte for byte, and that the imported key proves the generator's witness to the closed form of its toxic waste.
    python tools/zkey_bench.py [--log 16 20] [--reps 5] [--out profiles/zkey_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

H_KERNELS = ("group_ntt_g1_load", "group_ntt_twiddles", "group_ntt_g1_uniform", "group_ntt_g1_lane", "fr_powers", "mul_points_g1_win")
STAGE_KERNELS = ("group_ntt_g1_uniform", "group_ntt_g1_lane")
PHASES = ("upload", "coefficients", "h_basis", "download", "total")


def run(bn, log, reps, say=lambda *x: None):
    import numpy as np
    from circuit_rows_bench import read_clock, rows_matrix, timed      # noqa: F401
    from wasmsnark_amd import formats, synth
    lib = bn.lib
    nc = synth.NativeCircuit(lib, log, n_public=2, seed=log, style="columns")
    pkey, vk = nc.build_key()
    sec = formats.pkey_bin_to_sections(pkey)
    nv, n = nc.n_vars, nc.domain
    row = {"n_vars": nv, "n_public": nc.n_public, "domain": n, "reps": reps, "pkey_bytes": len(pkey)}

    ex_reports, im_reports = [], []

    def export():
        rep = {}
        out = bn.export_zkey(pkey=pkey, vk=vk, report=rep)
        ex_reports.append(rep)
        return out

    ms_ex, all_ex, outs = timed(export, reps)
    z = outs[-1]
    row["zkey_bytes"] = len(z)

    def imp():
        rep = {}
        out = bn.import_zkey(z, report=rep)
        im_reports.append(rep)
        return out

    ms_im, all_im, outs = timed(imp, reps)
    back, vk_back = outs[-1]
    med = lambda reps_, k: statistics.median(r["ms"][k] for r in reps_[1:])
    row["export"] = {"ms_host_clock": ms_ex, "all_ms": all_ex, "report_ms": {k: med(ex_reports, k) for k in PHASES}}
    row["import"] = {"ms_host_clock": ms_im, "all_ms": all_im, "report_ms": {k: med(im_reports, k) for k in PHASES},
                     "records": list(im_reports[-1]["records"]), "sorted": im_reports[-1]["sorted"]}
    say("export", row["export"]["report_ms"], "import", row["import"]["report_ms"])

    # the streams: the generator's with every column sorted by constraint; the point sections byte for byte
    t = time.perf_counter()
    rows = {"n_vars": nv, "n_public": nc.n_public, "n_constraints": n, "domain": n}
    want = {}
    for m in "AB":
        rows[m], want["pols" + m] = rows_matrix(bn, bytes(sec["pols" + m]), nv, n)
    rows["C"] = (np.zeros(n + 1, dtype="<u8"), np.zeros(0, dtype="<u4"), np.zeros(0, dtype=np.uint8))
    say("rows derived on the host", time.perf_counter() - t, "s")
    bsec = formats.pkey_bin_to_sections(back)
    ok = all(bytes(bsec[k]) == want[k] for k in want)
    ok = ok and all(bytes(bsec[k]) == bytes(sec[k]) for k in sec if k.startswith("points") or k in ("alfa1", "beta1", "delta1", "beta2", "delta2"))
    ok = ok and vk_back == vk and im_reports[-1]["sorted"] is True
    r32, s32 = bytes([3]) * 32, bytes([5]) * 32
    proof = bn.groth16GenProof(nc.witness_bin(), back, r=r32, s=s32)
    ok = ok and proof == nc.expected_proof(r32, s32) and bn.groth16Verify(vk_back, nc.public_signals(), proof)
    row["imported_key_proves_to_the_closed_form"] = bool(ok)
    say("imported key: streams, sections, proof:", ok)

    # the same key through the loader and the audit
    ms_load, all_load, _ = timed(lambda: bn.load_key(pkey).free(), reps)
    ms_check, all_check, checks = timed(lambda: bn.check_key(pkey=pkey), reps)
    ok = ok and checks[-1]["ok"]
    row["load_key"] = {"ms": ms_load, "all_ms": all_load}
    row["check_key"] = {"ms": ms_check, "all_ms": all_check}

    # the H kernels beside the transform's stage kernels
    H = bytes(sec["pointsH"])
    ks_h, ks_n = {k: [] for k in H_KERNELS}, {k: [] for k in STAGE_KERNELS}
    for i in range(reps + 1):
        lib.c.wsnark_timing_reset(); lib.c.wsnark_timing_enable(1)
        N = bn.h_basis(H, to_lagrange=True)
        t_h = lib.timing_report()
        lib.c.wsnark_timing_reset()
        bn.group_ntt(1, H, inverse=False)
        t_n = lib.timing_report()
        lib.c.wsnark_timing_enable(0)
        if i:
            for k in H_KERNELS:
                ks_h[k].append(t_h.get(k, (0.0, 0))[0])
            for k in STAGE_KERNELS:
                ks_n[k].append(t_n.get(k, (0.0, 0))[0])
    mh = {k: statistics.median(v) for k, v in ks_h.items()}
    mn = {k: statistics.median(v) for k, v in ks_n.items()}
    sh, sn = sum(mh.values()), sum(mn.values())
    row["h_basis_kernels"] = {"ms": mh, "all_ms": ks_h, "sum_ms": sh, "ntt_stage_kernels_ms": mn, "ntt_stage_sum_ms": sn,
                              "ratio_to_ntt_stages": sh / sn if sn > 0 else None, "expected": 1.12, "budget": 1.2}
    say("h_basis kernels", sh, "ntt stages", sn, "ratio", row["h_basis_kernels"]["ratio_to_ntt_stages"])

    # the composition of the calls that existed before: transform + twist through host memory, streams from rows
    R = synth.R
    w2 = synth.root_of_unity(log + 1)
    sc, x = bytearray(32 * n), (-2) % R
    for k in range(n):
        sc[32 * k:32 * k + 32] = x.to_bytes(32, "little")
        x = x * w2 % R
    sc = bytes(sc)

    def composition():
        h = bn.mul_points(1, bn.group_ntt(1, N, inverse=False), sc)
        return h, bn.circuit_from_rows(rows, public_rows=False)

    ms_co, all_co, outs = timed(composition, reps)
    ok = ok and outs[-1][0] == H and outs[-1][1]["polsA"] == want["polsA"] and outs[-1][1]["polsB"] == want["polsB"]
    row["composition"] = {"ms_host_clock": ms_co, "all_ms": all_co}
    row["ratio_import_to_composition"] = ms_im / ms_co if ms_co > 0 else None
    say("composition", ms_co, "import", ms_im, "ratio", row["ratio_import_to_composition"])
    nc.free()
    return row, bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import wasmsnark_amd
    from circuit_rows_bench import read_clock
    bn = wasmsnark_amd.build(device=0)
    say = lambda *x: print(*x, file=sys.stderr, flush=True)
    res = {"device": bn.device_info, "clock": read_clock(), "results": {}, "ok": True}
    for log in a.log:
        row, ok = run(bn, log, a.reps, say)
        res["results"][str(log)] = row
        res["ok"] = res["ok"] and ok
        print(json.dumps({"log_domain": log, "result": row, "ok": ok}), flush=True)
    assert res["ok"], "a check of the tool failed (streams, sections, the proof's closed form): no profile is written"
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
