// Drives mulPoints, contributePowers and checkPowers of wasmsnark_amd/js over the files tests/test_node_pwtau.py wrote to argv[2]: a
// transcript (tau_g1.bin, tau_g2.bin, alpha_tau_g1.bin, beta_tau_g1.bin, beta_g2.bin), the closed form of the contributed transcript
// (want_*.bin) under the secrets of expect.json, a transcript with one replaced alpha power, and per group points, scalars and the
// expected products.
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
const PARTS = [["tauG1", "tau_g1"], ["tauG2", "tau_g2"], ["alphaTauG1", "alpha_tau_g1"], ["betaTauG1", "beta_tau_g1"], ["betaG2", "beta_g2"]];

(async () => {
    const want = JSON.parse(rd("expect.json").toString("utf8"));
    const bn = await ws.buildBn128();
    // a scalar per point, both groups; the inputs are left as they were
    for (const g of [1, 2]) {
        const pts = rd(`mul_g${g}_in.bin`), copy = Buffer.from(pts), sc = rd("mul_scalars.bin");
        const out = await bn.mulPoints(g, pts, sc);
        if (!(out instanceof ArrayBuffer) || !eq(out, rd(`mul_g${g}_want.bin`)) || !eq(pts, copy)) throw new Error("mulPoints G" + g);
    }
    let err = null;
    try { await bn.mulPoints(1, rd("mul_g1_in.bin"), rd("mul_scalars.bin").subarray(32)); } catch (e) { err = e; }
    if (!err || !(err instanceof TypeError)) throw new Error("one scalar short: " + err);
    const spoiltPts = Buffer.from(rd("mul_g1_in.bin"));
    spoiltPts[64 * 2 + 32] ^= 1;
    err = null;
    try { await bn.mulPoints(1, spoiltPts, rd("mul_scalars.bin")); } catch (e) { err = e; }
    if (!err || !/wsnark error 2/.test(err.message) || !/index 2/.test(err.message)) throw new Error("off-curve point: " + err);
    // the contribution: the closed form, all five parts
    const powers = { domain: want.domain };
    for (const [k, f] of PARTS) powers[k] = rd(f + ".bin");
    const secrets = { tau: Buffer.from(want.tau, "hex"), alpha: Buffer.from(want.alpha, "hex"), beta: Buffer.from(want.beta, "hex") };
    const c = await bn.contributePowers(powers, secrets);
    if (!c.report.ok || c.report.tauG1.points !== 2 * want.domain || c.report.tauG2.points !== want.domain || c.report.tauG1.bad !== 0 ||
        c.report.betaG2 !== null || c.report.relationsRun !== 0 || !(c.report.ms.total > 0))
        throw new Error("contribution report: " + JSON.stringify(c.report));
    for (const [k, f] of PARTS) if (!(c.powers[k] instanceof ArrayBuffer) || !eq(c.powers[k], rd("want_" + f + ".bin"))) throw new Error("contributePowers: " + k);
    // the audit: the contributed transcript passes; drawn secrets give another transcript that passes too
    let rep = await bn.checkPowers(c.powers);
    if (!rep.ok || rep.relationsRun !== 63 || rep.relationsBad !== 0 || rep.relations.tauG2 !== true) throw new Error("audit: " + JSON.stringify(rep));
    const drawn = await bn.contributePowers(powers);
    if (!drawn.report.ok || eq(drawn.powers.betaG2, powers.betaG2) || eq(drawn.powers.betaG2, c.powers.betaG2)) throw new Error("drawn secrets");
    if (!(await bn.checkPowers(drawn.powers, { points: false })).ok) throw new Error("audit of the drawn contribution");
    // one replaced alpha power (another multiple of G): relation bit 3 alone; the halves
    const replaced = Object.assign({}, powers, { alphaTauG1: rd("replaced_alpha_tau_g1.bin") });
    rep = await bn.checkPowers(replaced, { seed: Buffer.alloc(32, 7) });
    if (rep.ok || rep.relationsRun !== 63 || rep.relationsBad !== 8 || rep.relations.alphaTauG1 !== false || rep.alphaTauG1.bad !== 0) throw new Error("replaced power: " + JSON.stringify(rep));
    rep = await bn.checkPowers(replaced, { relations: false });
    if (!rep.ok || rep.relationsRun !== 0 || rep.relations.alphaTauG1 !== null) throw new Error("points only: " + JSON.stringify(rep));
    // a bad power is a result, for both calls
    const spoilt = Buffer.from(powers.betaTauG1);
    spoilt[64 * want.badIndex + 32] ^= 1;
    const bad = Object.assign({}, powers, { betaTauG1: spoilt });
    const cb = await bn.contributePowers(bad, secrets);
    if (cb.powers !== null || cb.report.ok || cb.report.betaTauG1.bad !== 1 || cb.report.betaTauG1.firstBad !== want.badIndex ||
        cb.report.betaTauG1.firstReason !== "off_curve" || cb.report.tauG1.bad !== 0)
        throw new Error("bad power: " + JSON.stringify(cb.report));
    rep = await bn.checkPowers(bad);
    if (rep.ok || rep.betaTauG1.firstBad !== want.badIndex || rep.relations.betaTauG1 !== null || rep.relationsRun !== (63 & ~16)) throw new Error("audit of a bad power: " + JSON.stringify(rep));
    // errors: a short array, a zero secret, a domain that is no power of two
    for (const [what, fn, re] of [["short", () => bn.checkPowers(Object.assign({}, powers, { tauG2: powers.tauG2.subarray(0, powers.tauG2.length - 128) })), /wsnark error 2/],
                                  ["short", () => bn.contributePowers(Object.assign({}, powers, { tauG1: powers.tauG1.subarray(64) }), secrets), /wsnark error 2/],
                                  ["zero secret", () => bn.contributePowers(powers, Object.assign({}, secrets, { alpha: Buffer.alloc(32) })), /wsnark error 4/],
                                  ["domain", () => bn.contributePowers(Object.assign({}, powers, { domain: 48 }), secrets), /wsnark error 1/]]) {
        err = null;
        try { await fn(); } catch (e) { err = e; }
        if (!err || !re.test(err.message)) throw new Error(what + ": " + err);
    }
    bn.terminate();
    console.log("NODE_PWTAU_OK");
})().catch((e) => { console.error(e); process.exit(1); });
