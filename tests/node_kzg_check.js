// Drives kzgLoadSrs, kzgCommit, kzgOpen, kzgVerify, polyEval and polyDivide of wasmsnark_amd/js over the files tests/test_node_kzg.py
// wrote to argv[2]: a reference string (tau_g1.bin, g2_pair.bin), three polynomials of expect.json's len (polys.bin), their
// commitments, values at z and the one proof under gamma in closed form (commitments.bin, ys.bin, proof.bin), the quotient of the first
// polynomial (q0.bin), and a spoilt proof with its expected verdict.
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
    const z = Buffer.from(want.z, "hex"), gamma = Buffer.from(want.gamma, "hex"), len = want.len;
    const bn = await ws.buildBn128();
    const polys = rd("polys.bin"), first = polys.subarray(0, 32 * len), g2Pair = rd("g2_pair.bin"), tauG1 = rd("tau_g1.bin"), g1 = tauG1.subarray(0, 64);
    // the field side
    const ys = await bn.polyEval(polys, len, z);
    if (!(ys instanceof ArrayBuffer) || !eq(ys, rd("ys.bin"))) throw new Error("polyEval");
    const d = await bn.polyDivide(first, z);
    if (!eq(d.q, rd("q0.bin")) || !eq(d.y, rd("ys.bin").subarray(0, 32))) throw new Error("polyDivide");
    // the reference string, commitments, the opening
    const srs = await bn.kzgLoadSrs(tauG1);
    const cs = await bn.kzgCommit(srs, polys, len);
    if (!(cs instanceof ArrayBuffer) || !eq(cs, rd("commitments.bin"))) throw new Error("kzgCommit");
    if (!eq(await bn.kzgCommit(srs, first, len), rd("commitments.bin").subarray(0, 64))) throw new Error("kzgCommit of one");
    const o = await bn.kzgOpen(srs, polys, len, z, gamma);
    if (!eq(o.ys, rd("ys.bin")) || !eq(o.proof, rd("proof.bin"))) throw new Error("kzgOpen");
    const one = await bn.kzgOpen(srs, first, len, z);
    if (!eq(one.ys, rd("ys.bin").subarray(0, 32))) throw new Error("kzgOpen of one");
    // the check: the opening, the single opening, the spoilt proof
    if ((await bn.kzgVerify(g1, g2Pair, cs, z, o.ys, o.proof, gamma)) !== true) throw new Error("kzgVerify rejected the opening");
    if ((await bn.kzgVerify(g1, g2Pair, rd("commitments.bin").subarray(0, 64), z, one.ys, one.proof)) !== true) throw new Error("kzgVerify rejected the single opening");
    if ((await bn.kzgVerify(g1, g2Pair, cs, z, o.ys, rd("spoilt_proof.bin"), gamma)) !== want.spoiltVerdict) throw new Error("kzgVerify accepted the spoilt proof");
    // arguments and errors
    let err = null;
    try { await bn.kzgOpen(srs, polys, len, z); } catch (e) { err = e; }
    if (!err || !(err instanceof TypeError)) throw new Error("three polynomials without gamma: " + err);
    err = null;
    try { await bn.kzgCommit(srs, polys, 3 * len); } catch (e) { err = e; }
    if (!err || !/wsnark error 1/.test(err.message)) throw new Error("len > n: " + err);
    err = null;
    try { await bn.kzgCommit({}, polys, len); } catch (e) { err = e; }
    if (!err || !(err instanceof TypeError)) throw new Error("no handle: " + err);
    const spoilt = Buffer.from(tauG1);
    spoilt[64 * 2 + 32] ^= 1;
    err = null;
    try { await bn.kzgLoadSrs(spoilt); } catch (e) { err = e; }
    if (!err || !/wsnark error 2/.test(err.message) || !/index 2 /.test(err.message)) throw new Error("off-curve power: " + err);
    bn.terminate();
    console.log("NODE_KZG_OK");
})().catch((e) => { console.error(e); process.exit(1); });
