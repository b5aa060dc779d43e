// Drives groth16GenProofBatch of wasmsnark_amd/js (method, module-level Promise form and callback form): a batch of 3 on the t6 golden
// key equals three groth16GenProof calls with the same r, s, and the reference's own recorded proofs.  argv[3] says which route the
// environment's WSNARK_BATCH_* switches select ("batch": the batch kernels, "loop": the loop over the single prover); the report must
// agree.  Run by tests/test_node_prove_batch.py.
"use strict";
const fs = require("fs");
const path = require("path");
const crypto = require("crypto");
const root = path.join(__dirname, "..");
// argv[2] ("emul"): bind the emulator build of the addon -- a test-side module swap, the product has no such option
if (process.argv[2] === "emul") require(path.join(__dirname, "emul", "use_emulator_addon.js"));
const route = process.argv[3];
const ws = require(path.join(root, "wasmsnark_amd", "js", "index.js"));
const gold = path.join(root, "tests", "golden");
const same = (a, b) => JSON.stringify(a) === JSON.stringify(b);
const hex = (s) => new Uint8Array(Buffer.from(s, "hex"));

(async () => {
    const pkey = fs.readFileSync(path.join(gold, "keys", "t6.pkey.bin")), wit = fs.readFileSync(path.join(gold, "keys", "t6.witness.bin"));
    const recorded = JSON.parse(fs.readFileSync(path.join(gold, "proofs.json"), "utf8")).t6.slice(0, 3);
    const bn = await ws.buildBn128();
    const key = await bn.loadKey(pkey);
    // a second witness that is NOT the circuit's: random 256-bit values (the yardstick is the single prover, not the circuit)
    const other = new Uint8Array(crypto.randomBytes(wit.length));
    const wits = [wit, other, wit];
    const r = recorded.map((c) => hex(c.r)), s = recorded.map((c) => hex(c.s));
    const want = [];
    for (let i = 0; i < 3; i++) want.push(await bn.groth16GenProof(wits[i], key, { r: r[i], s: s[i] }));
    if (!same(want[0], recorded[0].proof) || !same(want[2], recorded[2].proof)) throw new Error("the single prover differs from the reference");
    const report = {}, blinding = [];
    const got = await bn.groth16GenProofBatch(wits, key, { r, s, report, blinding });
    if (!same(got, want)) throw new Error("the batch differs from three groth16GenProof calls");
    if (report.count !== 3 || report.batched !== (route === "batch" ? 3 : 0) || !(report.ms.total > 0)) throw new Error("report: " + JSON.stringify(report));
    if (blinding.length !== 3 || !blinding.every((b, i) => Buffer.from(b.r).equals(Buffer.from(r[i])) && Buffer.from(b.s).equals(Buffer.from(s[i])))) throw new Error("blinding as used");
    // the witnesses and the blinding values back to back in one buffer each; key BYTES instead of a handle
    const cat = (xs) => Buffer.concat(xs.map((x) => Buffer.from(x)));
    if (!same(await bn.groth16GenProofBatch(cat(wits), pkey, { r: cat(r), s: cat(s) }), want)) throw new Error("back-to-back form differs");
    // drawn blinding: distinct per proof, and the single prover reproduces each proof with it
    const drawn = [];
    const fresh = await bn.groth16GenProofBatch(wits, key, { blinding: drawn });
    if (new Set(drawn.map((b) => Buffer.from(b.r).toString("hex") + Buffer.from(b.s).toString("hex"))).size !== 3) throw new Error("drawn blinding repeats");
    for (let i = 0; i < 3; i++)
        if (!same(await bn.groth16GenProof(wits[i], key, { r: drawn[i].r, s: drawn[i].s }), fresh[i])) throw new Error("drawn blinding does not reproduce proof " + i);
    if (!same(await bn.groth16GenProofBatch([], key), [])) throw new Error("empty batch");
    let threw = false;
    try { await bn.groth16GenProofBatch([wit.subarray(0, wit.length - 32)], key); } catch (e) { threw = true; }
    if (!threw) throw new Error("a short witness must be refused");
    threw = false;
    try { await bn.groth16GenProofBatch(wits, key, { r: r.slice(0, 2), s }); } catch (e) { threw = true; }
    if (!threw) throw new Error("two r values for three proofs must be refused");
    // module-level forms: Promise and node-style callback
    if (!same(await ws.groth16GenProofBatch(wits, pkey, { r, s }), want)) throw new Error("module-level Promise form differs");
    const viaCb = await new Promise((res, rej) => {
        const ret = ws.groth16GenProofBatch(wits, pkey, { r, s }, (err, proofs) => (err ? rej(err) : res(proofs)));
        if (ret !== undefined) rej(new Error("the callback form must return undefined"));
    });
    if (!same(viaCb, want)) throw new Error("callback form differs");
    bn.terminate();
    ws.terminate();
    console.log("NODE_PROVE_BATCH_OK " + route + " 3");
})().catch((e) => { console.error(e); process.exit(1); });
