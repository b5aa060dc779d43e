// Drives checkWitnesses of a loaded circuit and groth16GenProofBatch's {circuit} option of wasmsnark_amd/js over the files
// tests/test_node_witness_check_batch.py wrote to argv[2]: the circuit's three record streams (and those of a larger circuit, other_*),
// witnesses.bin (five witnesses back to back), key.bin (a proving key of the circuit) and expect.json (the counts, and per witness what
// Python integers say: bad, first_bad, ok, bad_rows, and a, b, c of every bad row as decimal strings).
"use strict";
const fs = require("fs");
const path = require("path");
const root = path.join(__dirname, "..");
const dir = process.argv[2];
// argv[3] (any value): bind the emulator build of the addon -- a test-side module swap, the product has no such option
if (process.argv[3]) require(path.join(__dirname, "emul", "use_emulator_addon.js"));
const ws = require(path.join(root, "wasmsnark_amd", "js", "index.js"));
const rd = (n) => fs.readFileSync(path.join(dir, n));
const same = (a, b) => JSON.stringify(a) === JSON.stringify(b);
const show = (x) => JSON.stringify(x, (k, v) => (typeof v === "bigint" ? String(v) : v));

function checkVerdict(v, want, cap, where) {
    const listed = Math.min(want.bad, cap);
    const values = v.badValues.map((abc) => abc.map(String));
    if (v.ok !== want.ok || v.bad !== want.bad || v.firstBad !== want.first_bad || v.listed !== listed || !v.oneOk || v.unreduced !== 0 ||
        v.firstUnreduced !== null || !same(v.badRows, want.bad_rows.slice(0, listed)) || !same(values, want.bad_values.slice(0, listed)) ||
        "rows" in v || "ms" in v)
        throw new Error(where + ", maxRows " + cap + ": " + show(v));
}

(async () => {
    const want = JSON.parse(rd("expect.json").toString("utf8"));
    const bn = await ws.buildBn128();
    const circuit = { nVars: want.nVars, nPublic: want.nPublic, domain: want.domain, polsA: rd("polsA.bin"), polsB: rd("polsB.bin"), polsC: rd("polsC.bin") };
    const blob = rd("witnesses.bin"), key = rd("key.bin");
    const stride = 32 * want.nVars, count = want.witnesses.length;
    const wits = want.witnesses.map((w, i) => blob.subarray(stride * i, stride * (i + 1)));
    const good = want.witnesses.map((w, i) => (w.ok ? i : -1)).filter((i) => i >= 0);
    if (count !== 5 || !same(good, [0, 2, 3])) throw new Error("the files are not the ones this script was written for");
    const rc = await bn.loadCircuit(circuit);
    // one buffer and an array of buffers; every cap; each verdict is the single call's
    for (const cap of [0, 1, want.domain]) {
        const report = {};
        const fromBlob = await rc.checkWitnesses(blob, { maxRows: cap, report });
        const fromArray = await rc.checkWitnesses(wits, { maxRows: cap });
        if (fromBlob.length !== count || show(fromBlob) !== show(fromArray)) throw new Error("blob and array differ, maxRows " + cap);
        for (let i = 0; i < count; i++) {
            checkVerdict(fromBlob[i], want.witnesses[i], cap, "checkWitnesses[" + i + "]");
            const single = await rc.checkWitness(wits[i], { maxRows: cap });
            for (const k of Object.keys(fromBlob[i])) if (show(fromBlob[i][k]) !== show(single[k])) throw new Error(`witness ${i}, ${k}: ${show(fromBlob[i][k])} != ${show(single[k])}`);
        }
        if (report.count !== count || report.rows !== want.domain || report.good !== 3 || report.firstNotOk !== 1 || !(report.chunk >= 1) || !(report.ms.total > 0))
            throw new Error("report: " + JSON.stringify(report));
    }
    checkVerdict((await rc.checkWitnesses(blob))[1], want.witnesses[1], 16, "default maxRows");
    const allGood = {};
    await rc.checkWitnesses(good.map((i) => wits[i]), { report: allGood });
    if (allGood.good !== 3 || allGood.firstNotOk !== null) throw new Error("all good: " + JSON.stringify(allGood));
    if (!same(await rc.checkWitnesses([]), [])) throw new Error("empty batch");
    let err = null;
    try { await rc.checkWitnesses(blob.subarray(0, blob.length - 1)); } catch (e) { err = e; }
    if (!err || !/whole number/.test(err.message)) throw new Error("a ragged buffer: " + err);
    err = null;
    try { await rc.checkWitnesses([wits[0].subarray(0, stride - 32)]); } catch (e) { err = e; }
    if (!err || !/shorter/.test(err.message)) throw new Error("a short witness: " + err);
    // groth16GenProofBatch with {circuit}: the good witnesses prove to what they prove to without, the bad ones give null
    const r = wits.map((w, i) => Buffer.alloc(32, 3 + i)), s = wits.map((w, i) => Buffer.alloc(32, 40 + i));
    const pick = (xs) => good.map((i) => xs[i]);
    const plain = await bn.groth16GenProofBatch(pick(wits), key, { r: pick(r), s: pick(s) });
    const report = {}, blinding = [];
    const got = await bn.groth16GenProofBatch(blob, key, { r, s, circuit: rc, report, blinding });
    if (got.length !== count || got[1] !== null || got[4] !== null || !same(pick(got), plain)) throw new Error("{circuit}: the proofs differ");
    if (!blinding.every((b, i) => (good.includes(i) ? Buffer.from(b.r).equals(r[i]) && Buffer.from(b.s).equals(s[i]) : b === null))) throw new Error("{circuit}: blinding");
    if (report.count !== 3 || report.batched !== 3 || got.verdicts.length !== count || report.verdicts !== got.verdicts) throw new Error("{circuit}: report " + show(report));
    got.verdicts.forEach((v, i) => checkVerdict(v, want.witnesses[i], 1, "verdicts[" + i + "]"));
    const drawn = [];
    const fresh = await bn.groth16GenProofBatch(wits, key, { circuit: rc, blinding: drawn });
    if (!same(fresh.map((p) => p === null), [false, true, false, false, true]) || !same(drawn.map((b) => b === null), [false, true, false, false, true]))
        throw new Error("{circuit}, drawn blinding");
    const none = await bn.groth16GenProofBatch([wits[1], wits[4]], key, { circuit: rc });
    if (!same(none, [null, null]) || none.verdicts.some((v) => v.ok)) throw new Error("{circuit}: all bad");
    const every = await bn.groth16GenProofBatch(wits, key, { r, s });
    if (every.some((p) => p === null) || every.verdicts !== undefined || !same(pick(every), plain)) throw new Error("without {circuit} the bad witnesses still prove");
    const other = await bn.loadCircuit({ nVars: want.otherNVars, nPublic: want.nPublic, domain: want.otherDomain, polsA: rd("other_polsA.bin"),
                                         polsB: rd("other_polsB.bin"), polsC: rd("other_polsC.bin") });
    err = null;
    try { await bn.groth16GenProofBatch(wits, key, { r, s, circuit: other }); } catch (e) { err = e; }
    if (!err || !/is not the key's/.test(err.message)) throw new Error("a circuit of another shape: " + err);
    other.free();
    rc.free();
    err = null;
    try { await rc.checkWitnesses(blob); } catch (e) { err = e; }
    if (!err || !/freed/.test(err.message)) throw new Error("a freed circuit: " + err);
    bn.terminate();
    console.log("NODE_WITNESS_CHECK_BATCH_OK");
})().catch((e) => { console.error(e); process.exit(1); });
