// Drives zkeyInfo, importZkey, exportZkey and the .wtns input of groth16GenProof of wasmsnark_amd/js over the files
// tests/test_node_zkey.py wrote to argv[2]: a model .zkey (model.zkey), what the Python side's import_zkey made of it (pkey.bin, vk.json),
// the circuit's witness as witness.bin and witness.wtns, two files written under another convention (wrong_root.zkey, wrong_coef.zkey),
// and expect.json (the numbers, the report, a proof for fixed r and s).
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
    const z = rd("model.zkey");
    const info = bn.zkeyInfo(z);
    if (!same(info, want.info)) throw new Error("zkeyInfo: " + JSON.stringify(info));
    if (!same(bn.zkeyInfo(path.join(dir, "model.zkey")), want.info)) throw new Error("zkeyInfo(path)");
    const wtns = rd("witness.wtns"), wit = rd("witness.bin");
    if (!Buffer.from(ws.wtnsToWitness(wtns)).equals(wit) || !Buffer.from(ws.witnessToWtns(wit)).equals(wtns)) throw new Error("wtnsToWitness / witnessToWtns");
    for (const src of [z, path.join(dir, "model.zkey")]) {
        const got = await bn.importZkey(src, { wtns });
        if (!got.pkey.equals(rd("pkey.bin"))) throw new Error("importZkey: the key differs from the Python side's");
        if (!same(got.vk, vkWant)) throw new Error("importZkey: the verification key differs");
        if (!same(got.report.records, want.info.records) || !same(got.report.unreduced, [0, 0]) || got.report.sorted !== true ||
            got.report.H.points !== want.info.domain || got.report.H.bad !== 0 || !(got.report.ms.total >= got.report.ms.hBasis && got.report.ms.hBasis > 0))
            throw new Error("importZkey: report " + JSON.stringify(got.report));
    }
    const { pkey, vk } = await bn.importZkey(z);
    const back = await bn.exportZkey(pkey, vk);
    if (!back.equals(z)) throw new Error("exportZkey: not the file that was imported");
    if (!same(back.report.records, want.info.records)) throw new Error("exportZkey: report");
    // the trial proof tells a file written under another convention
    for (const name of ["wrong_root.zkey", "wrong_coef.zkey"]) {
        await bn.importZkey(rd(name));      // (it parses)
        let refused = false;
        try { await bn.importZkey(rd(name), { wtns }); } catch (e) { refused = /trial proof/.test(e.message); }
        if (!refused) throw new Error("importZkey: the trial proof passed on " + name);
    }
    // a malformed file rejects with the library's text
    const bad = Buffer.from(z); bad[0] = 0x78;
    let msg = "";
    try { await bn.importZkey(bad); } catch (e) { msg = e.message; }
    if (!/magic/.test(msg)) throw new Error("importZkey: a bad magic gave: " + msg);
    // groth16GenProof takes the .wtns as it is
    const r = Buffer.from(want.r, "hex"), s = Buffer.from(want.s, "hex");
    const p1 = await bn.groth16GenProof(wtns, pkey, { r, s }), p2 = await bn.groth16GenProof(wit, pkey, { r, s });
    if (!same(p1, want.proof) || !same(p2, want.proof)) throw new Error("groth16GenProof(.wtns): " + JSON.stringify(p1));
    if (!(await bn.groth16Verify(vk, want.public, p1))) throw new Error("the proof does not verify");
    await bn.terminate();
    console.log("NODE_ZKEY_OK");
})().catch((e) => { console.error(e); process.exit(1); });
