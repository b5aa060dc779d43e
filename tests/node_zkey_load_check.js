// Drives loadKey and groth16GenProof of wasmsnark_amd/js on a snarkjs .zkey over the files tests/test_node_zkey_load.py wrote to
// argv[2]: the model file (model.zkey, sections in snarkjs' order), the closed form's key and verification key (pkey.bin, vk.json), the
// circuit's witness as witness.bin and witness.wtns, and expect.json (the numbers and the proof's closed form for fixed r and s).
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

(async () => {
    const want = JSON.parse(rd("expect.json").toString("utf8"));
    const vkWant = JSON.parse(rd("vk.json").toString("utf8"));
    const bn = await ws.buildBn128();
    const z = rd("model.zkey"), wtns = rd("witness.wtns"), wit = rd("witness.bin");
    const r = Buffer.from(want.r, "hex"), s = Buffer.from(want.s, "hex");
    // the file is told by its first four bytes, not by its name: a copy under another name loads the same
    const other = path.join(dir, "circuit_final.key");
    fs.writeFileSync(other, z);
    for (const src of [z, path.join(dir, "model.zkey"), other]) {
        const h = await bn.loadKey(src);
        if (!h || !same(h.vk, vkWant)) throw new Error("loadKey(.zkey): the handle's vk differs: " + JSON.stringify(h && h.vk));
        if (!same(h.report.records, want.records) || h.report.sorted !== true || h.report.H.points !== want.domain || h.report.H.bad !== 0 ||
            h.report.ms.download !== 0)
            throw new Error("loadKey(.zkey): report " + JSON.stringify(h.report));
        const ki = await bn.keyInfo(h);
        if (ki.nVars !== want.nVars || ki.nPublic !== want.nPublic || ki.domainSize !== want.domain) throw new Error("keyInfo: " + JSON.stringify(ki));
        if (!(await bn.waitTables(h))) throw new Error("waitTables");
        const p = await bn.groth16GenProof(wtns, h, { r, s });
        if (!same(p, want.proof)) throw new Error("groth16GenProof(wtns, zkey handle): " + JSON.stringify(p));
        if (!(await bn.groth16Verify(h.vk, want.public, p))) throw new Error("the proof does not verify against the handle's vk");
    }
    // the drop-in call on the file's bytes, .wtns and witness.bin; the second call finds the handle through the digest cache
    const before = bn.fullDigests;
    const p1 = await bn.groth16GenProof(wtns, z, { r, s });
    const mid = bn.fullDigests;
    const p2 = await bn.groth16GenProof(wit, z, { r, s });
    if (!same(p1, want.proof) || !same(p2, want.proof)) throw new Error("groth16GenProof(witness, zkey bytes): " + JSON.stringify(p1));
    if (!(mid >= before && bn.fullDigests === mid + 1)) throw new Error("the digest cache: " + [before, mid, bn.fullDigests].join(" "));
    if ((await bn.loadKey(z)) !== (await bn.loadKey(z))) throw new Error("loadKey(zkey bytes): two handles for the same bytes");
    // one call of two witnesses on the handle
    const batch = await bn.groth16GenProofBatch([wit, wit], await bn.loadKey(z), { r: [r, r], s: [s, s] });
    if (!same(batch, [want.proof, want.proof])) throw new Error("groth16GenProofBatch on a zkey handle");
    // the same key through proving_key.bin proves to the same bytes
    if (!same(await bn.groth16GenProof(wit, rd("pkey.bin"), { r, s }), want.proof)) throw new Error("groth16GenProof(witness, pkey.bin)");
    // a malformed file rejects with the library's text, bytes and path
    const bad = Buffer.from(z); bad[20] ^= 0xff;      // section 1's length
    const badPath = path.join(dir, "bad.zkey");
    fs.writeFileSync(badPath, bad);
    for (const src of [bad, badPath]) {
        let msg = "";
        try { await bn.loadKey(src); } catch (e) { msg = e.message; }
        if (!/zkey: /.test(msg)) throw new Error("loadKey: a malformed .zkey gave: " + msg);
    }
    await bn.terminate();
    // a {devices} group refuses a .zkey with a message
    const grp = await ws.buildBn128({ devices: [0, 0] });
    for (const src of [z, path.join(dir, "model.zkey")]) {
        let msg = "";
        try { await grp.loadKey(src); } catch (e) { msg = e.message; }
        if (!/single GPU/.test(msg)) throw new Error("a group took a .zkey: " + msg);
    }
    let msg = "";
    try { await grp.groth16GenProof(wit, z, { r, s }); } catch (e) { msg = e.message; }
    if (!/single GPU/.test(msg)) throw new Error("a group proved on a .zkey: " + msg);
    await grp.terminate();
    console.log("NODE_ZKEY_LOAD_OK");
})().catch((e) => { console.error(e); process.exit(1); });
