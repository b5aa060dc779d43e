// Drives groth16VerifyBatch of wasmsnark_amd/js (method, module-level Promise form and callback form) over the reference's own
// verifier data, tests/golden/verify.json: 18 cases in ONE call, verdicts recorded from the reference.  Run by
// tests/test_node_verify_batch.py.
"use strict";
const fs = require("fs");
const path = require("path");
const root = path.join(__dirname, "..");
// argv[2] (any value): bind the emulator build of the addon -- a test-side module swap, the product has no such option
if (process.argv[2]) require(path.join(__dirname, "emul", "use_emulator_addon.js"));
const ws = require(path.join(root, "wasmsnark_amd", "js", "index.js"));
const g = JSON.parse(fs.readFileSync(path.join(root, "tests", "golden", "verify.json"), "utf8"));
const same = (a, b) => JSON.stringify(a) === JSON.stringify(b);

(async () => {
    const vk = g.verification_key, cases = g.cases;
    if (cases.length !== 18) throw new Error("expected the 18 golden cases");
    const want = cases.map((c) => !!c.reference_verdict);
    if (want.filter((x) => x).length !== 3) throw new Error("expected 3 valid cases");
    const inputs = cases.map((c) => c.inputs), proofs = cases.map((c) => c.proof);
    const bn = await ws.buildBn128();
    const got = await bn.groth16VerifyBatch(vk, inputs, proofs);
    if (!same(got, want)) throw new Error("batch verdicts differ: " + JSON.stringify(got));
    // every verdict is the single call's
    for (let i = 0; i < cases.length; i += 5) {
        if ((await bn.groth16Verify(vk, inputs[i], proofs[i])) !== got[i]) throw new Error("single call differs at " + i);
    }
    // a malformed proof and an out-of-range input read false and leave their neighbours alone
    const q = 21888242871839275222246405745257275088696311157297823662689037894645226208583n;
    const bad = Object.assign({}, proofs[0], { pi_a: [(q + 5n).toString(), proofs[0].pi_a[1], "1"] });
    const big = [(1n << 256n).toString()].concat(inputs[0].slice(1));
    const mixed = await bn.groth16VerifyBatch(vk, [inputs[0], inputs[0], big, inputs[0]], [proofs[0], bad, proofs[0], proofs[0]]);
    if (!same(mixed, [want[0], false, false, want[0]]) || !want[0]) throw new Error("mixed batch: " + JSON.stringify(mixed));
    if (!same(await bn.groth16VerifyBatch(vk, [], []), [])) throw new Error("empty batch");
    let threw = false;
    try { await bn.groth16VerifyBatch(vk, [inputs[0], inputs[1].slice(1)], [proofs[0], proofs[1]]); } catch (e) { threw = e instanceof TypeError; }
    if (!threw) throw new Error("input arrays of two lengths must be refused");
    // module-level forms: Promise and node-style callback
    if (!same(await ws.groth16VerifyBatch(vk, inputs, proofs), want)) throw new Error("module-level Promise form differs");
    const viaCb = await new Promise((res, rej) => {
        const r = ws.groth16VerifyBatch(vk, inputs, proofs, (err, ok) => (err ? rej(err) : res(ok)));
        if (r !== undefined) rej(new Error("the callback form must return undefined"));
    });
    if (!same(viaCb, want)) throw new Error("callback form differs");
    ws.terminate();
    bn.terminate();
    console.log("NODE_VERIFY_BATCH_OK " + cases.length);
})().catch((e) => { console.error(e); process.exit(1); });
