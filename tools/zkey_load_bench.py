#!/usr/bin/env python3
"""A .zkey straight into a resident key against the two-step path (needs the GPU; bench.py is not involved).  Prints ONE JSON line per
size.  On ONE key of the native generator's "columns" family (csrc/synth.hip, style 0: the bench's C4 circuit) at log2(domain) = --log,
written to a .zkey FILE by export_zkey -- there is no snarkjs-written file to measure --, in ONE process, the variants alternate --reps
times after one unrecorded round of all of them:
  a        load_zkey(path=, wait_tables=False)                                  host clock; the call ends in a drained queue
  b        import_zkey(path=) then load_key(pkey, wait_tables=False)            host clock around both
  a_wait / b_wait   the same with wait_tables=True: up to the steady state
Every loaded key proves the generator's witness, and the proof is compared with the closed form of the toxic waste in the same run.
Recorded: medians, the min - max range, the reports' own ms of (a) and of (b)'s import, (b)'s load_ms; what to expect of (a) --
b - import.ms[download] - load_ms[points_h2d] - load_ms[pols_to_csr] of the same run -- and by how much (a) misses it, beside the
run-to-run spread; the resident set of a fresh child process (peak, and now by kind) before load_zkey(path=) alone, after it and after
a second one (the file variant never holds the key: what the first load adds and the second does not is one-time set-up);
the commit and the device.  The criterion: a below b at every size, else no profile is written.
    python tools/zkey_load_bench.py [--log 16 20] [--reps 5] [--out profiles/zkey_load_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PHASES = ("upload", "coefficients", "h_basis", "download", "total")
LOAD_PHASES = ("pols_to_csr", "points_h2d", "masks_convert", "total")
R32, S32 = bytes([3]) * 32, bytes([5]) * 32


def memory_kb():
    """the process's resident set by kind (kB): the peak, now, and now split into anonymous, file-backed (a mapped key's pages are
    these) and shared (pinned host memory shows here or as anonymous)"""
    want = ("VmHWM", "VmRSS", "RssAnon", "RssFile", "RssShmem")
    out = {}
    with open("/proc/self/status") as f:
        for line in f:
            name = line.split(":")[0]
            if name in want:
                out[name] = int(line.split()[1])
    return out


def child(path):
    """a fresh process: init, one small call to settle the runtime's own memory, then the file-variant load alone"""
    import wasmsnark_amd
    bn = wasmsnark_amd.build(device=0)
    bn.fft(bytes(32 * 256), 1)
    before = memory_kb()
    key, _ = bn.load_zkey(path=path, wait_tables=True)
    after = memory_kb()
    key.free()
    key, _ = bn.load_zkey(path=path, wait_tables=True)      # a second load: whatever the first one set up once (the staging ring) is there
    again = memory_kb()
    key.free()
    print(json.dumps({"kb_before": before, "kb_after_first_load": after, "kb_after_second_load": again, "file_bytes": os.path.getsize(path),
                      "vm_hwm_growth_kb": [after["VmHWM"] - before["VmHWM"], again["VmHWM"] - after["VmHWM"]]}))


def run(bn, log, reps, tmp, say=lambda *x: None):
    from wasmsnark_amd import synth
    nc = synth.NativeCircuit(bn.lib, log, n_public=2, seed=log, style="columns")
    pkey, vk = nc.build_key()
    path = os.path.join(tmp, "bench_%d.zkey" % log)
    with open(path, "wb") as f:
        f.write(bn.export_zkey(pkey=pkey, vk=vk))
    pkey_bytes = len(pkey)
    del pkey
    wit, want = nc.witness_bin(), nc.expected_proof(R32, S32)
    ok = True

    def proves(key):
        return bn.groth16GenProof(wit, key, r=R32, s=S32) == want

    def variant_a(wait):
        rep = {}
        t = time.perf_counter()
        key, _ = bn.load_zkey(path=path, wait_tables=wait, report=rep)
        ms = (time.perf_counter() - t) * 1e3
        good = proves(key)
        load_ms = dict(key.load_ms)
        key.free()
        return ms, good, {"report_ms": rep["ms"], "load_ms": load_ms}

    def variant_b(wait):
        rep = {}
        t = time.perf_counter()
        imported, _ = bn.import_zkey(path=path, report=rep)
        t_mid = time.perf_counter()
        key = bn.load_key(imported, wait_tables=wait)
        ms = (time.perf_counter() - t) * 1e3
        good = proves(key)
        load_ms = dict(key.load_ms)
        key.free()
        return ms, good, {"report_ms": rep["ms"], "load_ms": load_ms, "import_ms": (t_mid - t) * 1e3}

    variants = (("a", variant_a, False), ("b", variant_b, False), ("a_wait", variant_a, True), ("b_wait", variant_b, True))
    times = {name: [] for name, _, _ in variants}
    parts = {name: [] for name, _, _ in variants}
    for rnd in range(reps + 1):                      # round 0: the warm-up of every shape the timed rounds use
        for name, fn, wait in variants:
            ms, good, extra = fn(wait)
            ok = ok and good
            if rnd:
                times[name].append(ms)
                parts[name].append(extra)
        say("log", log, "round", rnd, {k: (v[-1] if v else None) for k, v in times.items()})
    med = statistics.median
    row = {"n_vars": nc.n_vars, "n_public": nc.n_public, "domain": nc.domain, "reps": reps, "pkey_bytes": pkey_bytes,
           "zkey_bytes": os.path.getsize(path), "every_key_proved_to_the_closed_form": bool(ok)}
    for name in times:
        row[name] = {"median_ms": med(times[name]), "min_ms": min(times[name]), "max_ms": max(times[name]), "all_ms": times[name]}
    row["a"]["report_ms"] = {k: med(p["report_ms"][k] for p in parts["a"]) for k in PHASES}
    row["a"]["load_ms"] = {k: med(p["load_ms"][k] for p in parts["a"]) for k in LOAD_PHASES}
    row["b"]["import_report_ms"] = {k: med(p["report_ms"][k] for p in parts["b"]) for k in PHASES}
    row["b"]["import_ms_host_clock"] = med(p["import_ms"] for p in parts["b"])
    row["b"]["load_ms"] = {k: med(p["load_ms"][k] for p in parts["b"]) for k in LOAD_PHASES}
    # what (a) should cost: (b) without import's download, the loader's second upload of the points, its header walk and transposition
    saved = row["b"]["import_report_ms"]["download"] + row["b"]["load_ms"]["points_h2d"] + row["b"]["load_ms"]["pols_to_csr"]
    spread = max(row["a"]["max_ms"] - row["a"]["min_ms"], row["b"]["max_ms"] - row["b"]["min_ms"])
    row["expected_a_ms"] = row["b"]["median_ms"] - saved
    row["a_minus_expected_ms"] = row["a"]["median_ms"] - row["expected_a_ms"]
    row["run_to_run_spread_ms"] = spread
    row["a"]["host_clock_minus_report_total_ms"] = row["a"]["median_ms"] - row["a"]["report_ms"]["total"]      # the Python mirror around the C call
    row["a_below_b"] = row["a"]["median_ms"] < row["b"]["median_ms"] and row["a_wait"]["median_ms"] < row["b_wait"]["median_ms"]
    if abs(row["a_minus_expected_ms"]) > spread:
        ra = row["a"]["report_ms"]
        rest = row["a"]["median_ms"] - ra["total"]
        row["where_the_time_went"] = ("a = parse + upload %.1f + coefficients %.1f + H basis %.1f + masks, conversion and the table build's launches %.1f "
                                      "(report total %.1f) + %.1f ms of the Python mirror around the call; b's import spends upload %.1f + "
                                      "coefficients %.1f + H basis %.1f + download %.1f, its load %.1f" %
                                      (ra["upload"], ra["coefficients"], ra["h_basis"], ra["total"] - ra["upload"] - ra["coefficients"] - ra["h_basis"],
                                       ra["total"], rest, *(row["b"]["import_report_ms"][k] for k in PHASES[:4]), row["b"]["load_ms"]["total"]))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-hwm", path], capture_output=True, text=True, timeout=900)
    row["file_variant_child"] = json.loads(out.stdout.strip().splitlines()[-1]) if out.returncode == 0 and out.stdout.strip() else {"error": out.stderr[-400:]}
    os.remove(path)
    nc.free()
    return row, bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="", help="recorded as it is (a copy of the tree that is no git checkout cannot tell)")
    ap.add_argument("--child-hwm", default="")
    a = ap.parse_args()
    if a.child_hwm:
        return child(a.child_hwm)
    import wasmsnark_amd
    from circuit_rows_bench import read_clock
    bn = wasmsnark_amd.build(device=0)
    say = lambda *x: print(*x, file=sys.stderr, flush=True)
    try:
        commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, timeout=30).stdout.strip() or "not a git checkout"
    except Exception:      # noqa: BLE001
        commit = "not read"
    res = {"device": bn.device_info, "clock": read_clock(), "commit": commit, "results": {}, "ok": True}
    with tempfile.TemporaryDirectory() as tmp:
        for log in a.log:
            row, ok = run(bn, log, a.reps, tmp, say)
            res["results"][str(log)] = row
            res["ok"] = res["ok"] and ok and row["a_below_b"]
            print(json.dumps({"log_domain": log, "result": row, "ok": ok}), flush=True)
    assert res["ok"], "a loaded key did not prove to the closed form, or load_zkey was not below the two-step path: no profile is written"
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
