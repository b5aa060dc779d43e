// Drives contributeKey and verifyContribution of wasmsnark_amd/js over the keys tests/test_node_pkey_delta.py wrote to argv[2]:
// old.bin / old.wsnark64, want.bin / want.wsnark64 (the closed form of old under delta * d), one tampered file per row of the
// rejection table (expect.json: the bits that must be bad and the bits that must have run), off_curve.bin.
"use strict";
const fs = require("fs");
const path = require("path");
const root = path.join(__dirname, "..");
const dir = process.argv[2];
// argv[3] (any value): bind the emulator build of the addon -- a test-side module swap, the product has no such option
if (process.argv[3]) require(path.join(__dirname, "emul", "use_emulator_addon.js"));
const ws = require(path.join(root, "wasmsnark_amd", "js", "index.js"));
const rd = (n) => fs.readFileSync(path.join(dir, n));
const eq = (a, b) => Buffer.compare(Buffer.from(a), Buffer.from(b)) === 0;

(async () => {
    const want = JSON.parse(rd("expect.json").toString("utf8"));
    const d = Buffer.from(want.d, "hex");
    const old = rd("old.bin"), twin = rd("want.bin");
    const bn = await ws.buildBn128();
    // key bytes: the closed form, byte for byte
    const r1 = await bn.contributeKey(old, { entropy: d });
    if (!r1.report.ok || r1.report.C.points !== want.nC || r1.report.H.points !== want.nH || r1.report.C.bad !== 0 || r1.report.H.firstBad !== null || !(r1.report.ms.total > 0))
        throw new Error("report: " + JSON.stringify(r1.report));
    if (!(r1.key instanceof ArrayBuffer) || !eq(r1.key, twin)) throw new Error("contributeKey(bytes) is not the closed form");
    // key files, both formats
    for (const ext of ["bin", "wsnark64"]) {
        const out = path.join(dir, "node_out." + ext);
        const r = await bn.contributeKey(path.join(dir, "old." + ext), { outPath: out, entropy: d });
        if (r.key !== out || !r.report.ok || !eq(fs.readFileSync(out), rd("want." + ext))) throw new Error("contributeKey(path) " + ext);
    }
    // accepted: bytes and paths, three seeds
    for (const seed of [Buffer.alloc(32, 9), Buffer.from(Array.from({ length: 32 }, (_, i) => i)), null]) {
        const v = await bn.verifyContribution(old, twin, { seed });
        if (!v.ok || v.checksRun !== 31 || v.checksBad !== 0 || v.checks.C !== true || v.checks.delta_changed !== true) throw new Error("accept: " + JSON.stringify(v));
    }
    const vp = await bn.verifyContribution(path.join(dir, "old.bin"), path.join(dir, "want.wsnark64"));
    if (!vp.ok) throw new Error("accept by path: " + JSON.stringify(vp));
    // a chain of two contributions checked as old -> newest
    const r2 = await bn.contributeKey(r1.key, { entropy: Buffer.alloc(32, 3) });
    if (!(await bn.verifyContribution(old, r2.key)).ok || !(await bn.verifyContribution(twin, r2.key)).ok) throw new Error("chain");
    // the rejection table
    for (const [name, c] of Object.entries(want.cases)) {
        for (const how of ["bytes", "path"]) {
            const v = how === "bytes" ? await bn.verifyContribution(old, rd(name + ".bin"), { check: false })
                                      : await bn.verifyContribution(path.join(dir, "old.bin"), path.join(dir, name + ".bin"), { check: false, seed: Buffer.alloc(32, 5) });
            if (v.ok || v.checksBad !== c.bad || v.checksRun !== c.run) throw new Error(name + " (" + how + "): " + JSON.stringify(v));
        }
    }
    // d = 1: bit 4 only
    const one = Buffer.alloc(32); one[0] = 1;
    const same = await bn.contributeKey(old, { entropy: one });
    if (!eq(same.key, old)) throw new Error("d = 1 changed the key");
    const v1 = await bn.verifyContribution(old, same.key);
    if (v1.ok || v1.checksBad !== 16 || v1.checksRun !== 31) throw new Error("d = 1: " + JSON.stringify(v1));
    // the audit in front: an off-curve C' point is refused with the audit's message; a bad INPUT point is a result
    let err = null;
    try { await bn.verifyContribution(old, rd("off_curve.bin")); } catch (e) { err = e; }
    if (!(err instanceof Error) || !err.report || !/failed its audit/.test(err.message) || !/section C/.test(err.message) || err.report.C.firstBad !== want.off_curve_index) throw new Error("audit: " + err);
    const rb = await bn.contributeKey(rd("off_curve.bin"), { entropy: d });
    if (rb.key !== null || rb.report.ok || rb.report.C.bad !== 1 || rb.report.C.firstBad !== want.off_curve_index || rb.report.C.firstReason !== "off_curve") throw new Error("bad input: " + JSON.stringify(rb.report));
    const outBad = path.join(dir, "node_bad_out.bin");
    const rbf = await bn.contributeKey(path.join(dir, "off_curve.bin"), { outPath: outBad, entropy: d });
    if (rbf.key !== null || fs.existsSync(outBad)) throw new Error("bad input by path left a file");
    // library-drawn d: two different keys, both accepted
    const a = await bn.contributeKey(old), b = await bn.contributeKey(old);
    if (eq(a.key, b.key) || !(await bn.verifyContribution(old, a.key)).ok || !(await bn.verifyContribution(old, b.key)).ok) throw new Error("library-drawn d");
    // errors: d = 0, truncated bytes, in == out
    for (const [what, fn, re] of [["d = 0", () => bn.contributeKey(old, { entropy: Buffer.alloc(32) }), /wsnark error 4/],
                                  ["truncated", () => bn.contributeKey(old.subarray(0, 300), { entropy: d }), /wsnark error 2/],
                                  ["same file", () => bn.contributeKey(path.join(dir, "old.bin"), { outPath: path.join(dir, "old.bin"), entropy: d }), /wsnark error 4/]]) {
        err = null;
        try { await fn(); } catch (e) { err = e; }
        if (!err || !re.test(err.message)) throw new Error(what + ": " + err);
    }
    if (!eq(rd("old.bin"), old)) throw new Error("the input file changed");
    bn.terminate();
    console.log("NODE_PKEY_DELTA_OK");
})().catch((e) => { console.error(e); process.exit(1); });
