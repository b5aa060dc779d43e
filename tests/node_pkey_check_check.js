// Drives checkKey and loadKey(..., {check: true}) of wasmsnark_amd/js over a valid and a tampered synthetic key that
// tests/test_node_pkey_check.py wrote to argv[2] (good.bin, good.wsnark64, bad.bin, expect.json).
"use strict";
const fs = require("fs");
const path = require("path");
const root = path.join(__dirname, "..");
const dir = process.argv[2];
// argv[3] (any value): bind the emulator build of the addon -- a test-side module swap, the product has no such option
if (process.argv[3]) require(path.join(__dirname, "emul", "use_emulator_addon.js"));
const ws = require(path.join(root, "wasmsnark_amd", "js", "index.js"));
const same = (a, b) => JSON.stringify(a) === JSON.stringify(b);
const noMs = (r) => Object.assign({}, r, { ms: null });

(async () => {
    const want = JSON.parse(fs.readFileSync(path.join(dir, "expect.json"), "utf8"));
    const good = fs.readFileSync(path.join(dir, "good.bin")), bad = fs.readFileSync(path.join(dir, "bad.bin"));
    const bn = await ws.buildBn128();
    // bytes and both file formats: the same report
    const rep = await bn.checkKey(good);
    if (!rep.ok || rep.relationsRun !== 7 || rep.relationsBad !== 0) throw new Error("valid key: " + JSON.stringify(rep));
    for (const s of ["A", "B1", "B2", "C", "H"]) {
        if (rep[s].points !== want.points[s] || rep[s].infinity !== want.infinity[s] || rep[s].bad !== 0 || rep[s].firstBad !== null) throw new Error("section " + s + ": " + JSON.stringify(rep[s]));
    }
    if (!(rep.ms.total > 0)) throw new Error("ms: " + JSON.stringify(rep.ms));
    for (const p of ["good.bin", "good.wsnark64"]) {
        if (!same(noMs(await bn.checkKey(path.join(dir, p))), noMs(rep))) throw new Error("file report differs: " + p);
    }
    if (!same(noMs(await bn.checkKey(good.buffer.slice(good.byteOffset, good.byteOffset + good.length), { seed: Buffer.alloc(32, 9) })), noMs(rep))) throw new Error("ArrayBuffer + seed");
    const pointsOnly = await bn.checkKey(good, { relations: false });
    if (!pointsOnly.ok || pointsOnly.relationsRun !== 0 || pointsOnly.relations["B1~B2"] !== null) throw new Error("points only");
    // the tampered key: a result, not a rejection
    const r2 = await bn.checkKey(bad);
    const b2 = r2.B2;
    if (r2.ok || b2.bad !== 1 || b2.firstBad !== want.bad_index || b2.firstReason !== "outside_subgroup" || r2.relations["B1~B2"] !== null || r2.relations["beta1~beta2"] !== true)
        throw new Error("tampered key: " + JSON.stringify(r2));
    if (!same(noMs(await bn.checkKey(path.join(dir, "bad.bin"))), noMs(r2))) throw new Error("tampered key by path");
    // loadKey with the option rejects with .report; without it nothing changes (the tampered key loads, the handle is cached)
    let err = null;
    try { await bn.loadKey(bad, { check: true }); } catch (e) { err = e; }
    if (!(err instanceof Error) || !err.report || err.report.ok !== false || err.report.B2.firstBad !== want.bad_index || !/section B2/.test(err.message)) throw new Error("loadKey check: " + err);
    err = null;
    try { await bn.loadKey(path.join(dir, "bad.bin"), { check: true }); } catch (e) { err = e; }
    if (!err || !err.report) throw new Error("loadKey(path, check)");
    const h = await bn.loadKey(bad);
    if (h !== (await bn.loadKey(bad))) throw new Error("the handle cache changed");
    const hg = await bn.loadKey(good, { check: true });
    if (hg !== (await bn.loadKey(good))) throw new Error("a checked load must cache its handle like any other");
    const proof = await bn.groth16GenProof(fs.readFileSync(path.join(dir, "witness.bin")), hg);
    if (!proof.pi_a || proof.pi_a.length !== 3) throw new Error("proof after a checked load");
    // truncated bytes: the loader's error
    err = null;
    try { await bn.checkKey(good.subarray(0, 300)); } catch (e) { err = e; }
    if (!err || !/wsnark error 2/.test(err.message)) throw new Error("truncated: " + err);
    bn.terminate();
    console.log("NODE_PKEY_CHECK_OK");
})().catch((e) => { console.error(e); process.exit(1); });
