// Drives compressProofs / decompressProofs / compressPoints / decompressPoints / groth16VerifyBatchCompressed of wasmsnark_amd/js over a
// job file written by tests/test_node_point_codec.py: the golden proofs of the t6 key and two planted ones, with the bytes and the
// statuses the Python binding gave for them.  Every answer here must be Python's.
"use strict";
const fs = require("fs");
const path = require("path");
const root = path.join(__dirname, "..");
const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
// argv[3] (any value): bind the emulator build of the addon -- a test-side module swap, the product has no such option
if (process.argv[3]) require(path.join(__dirname, "emul", "use_emulator_addon.js"));
const ws = require(path.join(root, "wasmsnark_amd", "js", "index.js"));
const same = (a, b) => JSON.stringify(a) === JSON.stringify(b);
const hex = (ab) => Buffer.from(ab).toString("hex");

(async () => {
    const bn = await ws.buildBn128();
    let checked = 0;
    for (const enc of ["le", "be"]) {
        const want = job[enc];
        const c = await bn.compressProofs(job.proofs, enc);
        if (hex(c.data) !== want.data || !same(c.status, want.compress_status)) throw new Error(enc + ": compressProofs differs");
        const all = Buffer.concat([Buffer.from(c.data), Buffer.from(want.planted, "hex")]);
        const inputs = new Array(all.length / 128).fill(job.inputs);
        const st = await bn.groth16VerifyBatchCompressed(job.vk, inputs, all, enc, true);
        if (!same(st, want.verify_status)) throw new Error(enc + ": verify statuses " + JSON.stringify(st));
        if (!same(await bn.groth16VerifyBatchCompressed(job.vk, inputs, all, enc), want.verify_status.map((v) => v === 1))) throw new Error(enc + ": verdicts");
        const d = await bn.decompressProofs(all, enc);
        if (!same(d.status, want.decompress_status) || !same(d.proofs, want.decompressed)) throw new Error(enc + ": decompressProofs differs");
        for (const g of [1, 2]) {
            const pts = Buffer.from(job.points[g], "hex");
            const cp = await bn.compressPoints(g, pts, enc);
            if (hex(cp.data) !== want.points[g].data || !same(cp.status, want.points[g].status)) throw new Error(enc + ": compressPoints " + g);
            const dp = await bn.decompressPoints(g, Buffer.from(want.points[g].bad, "hex"), enc, g === 2);
            if (hex(dp.data) !== want.points[g].bad_out || !same(dp.status, want.points[g].bad_status)) throw new Error(enc + ": decompressPoints " + g);
        }
        checked += st.length;
    }
    if (!same(await bn.groth16VerifyBatchCompressed(job.vk, [], Buffer.alloc(0), "le"), [])) throw new Error("empty batch");
    let threw = false;
    try { await bn.compressProofs(job.proofs, "xx"); } catch (e) { threw = e instanceof TypeError; }
    if (!threw) throw new Error("an unknown encoding must be refused");
    bn.terminate();
    console.log("NODE_POINT_CODEC_OK " + checked);
})().catch((e) => { console.error(e); process.exit(1); });
