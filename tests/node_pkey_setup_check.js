// Drives newKey and groupNtt of wasmsnark_amd/js over the files tests/test_node_pkey_setup.py wrote to argv[2]: the powers
// (tau_g1.bin, tau_g2.bin, alpha_tau_g1.bin, beta_tau_g1.bin, beta_g2.bin), the circuit's three record streams, want.bin (the closed
// form of the key under delta = gamma = 1), want_ic.bin, and per group a transform's input and its two expected outputs.
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
    const bn = await ws.buildBn128();
    // the transform, both groups, both directions; the input is left as it was
    for (const g of [1, 2]) {
        const pts = rd(`ntt_g${g}_in.bin`), copy = Buffer.from(pts);
        const fwd = await bn.groupNtt(g, pts), inv = await bn.groupNtt(g, pts, true);
        if (!(fwd instanceof ArrayBuffer) || !eq(fwd, rd(`ntt_g${g}_fwd.bin`)) || !eq(inv, rd(`ntt_g${g}_inv.bin`)) || !eq(pts, copy)) throw new Error("groupNtt G" + g);
        if (!eq(await bn.groupNtt(g, fwd, true), pts)) throw new Error("groupNtt round trip G" + g);
    }
    let err = null;
    try { await bn.groupNtt(1, rd("ntt_g1_in.bin").subarray(0, 3 * 64)); } catch (e) { err = e; }
    if (!err || !/wsnark error 1/.test(err.message)) throw new Error("three points: " + err);
    // the key
    const powers = { domain: want.domain, tauG1: rd("tau_g1.bin"), tauG2: rd("tau_g2.bin"), alphaTauG1: rd("alpha_tau_g1.bin"),
                     betaTauG1: rd("beta_tau_g1.bin"), betaG2: rd("beta_g2.bin") };
    const circuit = { nVars: want.nVars, nPublic: want.nPublic, domain: want.domain, polsA: rd("polsA.bin"), polsB: rd("polsB.bin"), polsC: rd("polsC.bin") };
    const r = await bn.newKey(powers, circuit);
    if (!r.report.ok || r.report.tauG1.points !== 2 * want.domain || r.report.tauG2.points !== want.domain || r.report.tauG1.bad !== 0 ||
        r.report.betaTauG1.firstBad !== null || r.report.betaG2 !== null || !(r.report.ms.total > 0))
        throw new Error("report: " + JSON.stringify(r.report));
    if (!(r.key instanceof ArrayBuffer) || !eq(r.key, rd("want.bin"))) throw new Error("newKey is not the closed form");
    if (!eq(r.ic, rd("want_ic.bin"))) throw new Error("IC");
    // the chain: audit, contribution, its check, a proof under the contributed key
    if (!(await bn.checkKey(r.key)).ok) throw new Error("audit of the new key");
    const c = await bn.contributeKey(r.key, { entropy: Buffer.from(want.delta, "hex") });
    if (!c.report.ok || !eq(c.key, rd("want_contributed.bin"))) throw new Error("contribution");
    if (!(await bn.verifyContribution(r.key, c.key)).ok) throw new Error("verifyContribution");
    // a bad power is a result
    const spoilt = Buffer.from(powers.alphaTauG1);
    spoilt[64 * want.badIndex + 32] ^= 1;
    const rb = await bn.newKey(Object.assign({}, powers, { alphaTauG1: spoilt }), circuit);
    if (rb.key !== null || rb.ic !== null || rb.report.ok || rb.report.alphaTauG1.bad !== 1 || rb.report.alphaTauG1.firstBad !== want.badIndex ||
        rb.report.alphaTauG1.firstReason !== "off_curve" || rb.report.tauG1.bad !== 0)
        throw new Error("bad power: " + JSON.stringify(rb.report));
    // errors: a short array, tau_g1[0] not the generator
    for (const [what, p, re] of [["short", Object.assign({}, powers, { tauG2: powers.tauG2.subarray(0, powers.tauG2.length - 128) }), /wsnark error 2/],
                                 ["generator", Object.assign({}, powers, { tauG1: Buffer.concat([powers.tauG1.subarray(64, 128), powers.tauG1.subarray(64)]) }), /wsnark error 2/]]) {
        err = null;
        try { await bn.newKey(p, circuit); } catch (e) { err = e; }
        if (!err || !re.test(err.message)) throw new Error(what + ": " + err);
    }
    bn.terminate();
    console.log("NODE_PKEY_SETUP_OK");
})().catch((e) => { console.error(e); process.exit(1); });
