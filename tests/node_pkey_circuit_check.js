// Drives checkKeyCircuit of wasmsnark_amd/js over the files tests/test_node_pkey_circuit.py wrote to argv[2]: the powers (tau_g1.bin,
// tau_g2.bin, alpha_tau_g1.bin, beta_tau_g1.bin, beta_g2.bin), the circuit's three record streams, key.bin (a good key of that circuit
// on that transcript, after a contribution), vk.json (its verification key), tampered_key.bin (two points of A swapped) and
// tampered_vk.json (IC_0 and IC_1 swapped).
"use strict";
const fs = require("fs");
const path = require("path");
const root = path.join(__dirname, "..");
const dir = process.argv[2];
// argv[3] (any value): bind the emulator build of the addon -- a test-side module swap, the product has no such option
if (process.argv[3]) require(path.join(__dirname, "emul", "use_emulator_addon.js"));
const ws = require(path.join(root, "wasmsnark_amd", "js", "index.js"));
const rd = (n) => fs.readFileSync(path.join(dir, n));

(async () => {
    const want = JSON.parse(rd("expect.json").toString("utf8"));
    const bn = await ws.buildBn128();
    const powers = { domain: want.domain, tauG1: rd("tau_g1.bin"), tauG2: rd("tau_g2.bin"), alphaTauG1: rd("alpha_tau_g1.bin"),
                     betaTauG1: rd("beta_tau_g1.bin"), betaG2: rd("beta_g2.bin") };
    const circuit = { nVars: want.nVars, nPublic: want.nPublic, domain: want.domain, polsA: rd("polsA.bin"), polsB: rd("polsB.bin"), polsC: rd("polsC.bin") };
    const vk = JSON.parse(rd("vk.json").toString("utf8")), badVk = JSON.parse(rd("tampered_vk.json").toString("utf8"));
    const seed = Buffer.alloc(32, 7);
    // a good key, as bytes and as a file; with and without the verification key
    for (const key of [rd("key.bin"), path.join(dir, "key.bin")]) {
        const v = await bn.checkKeyCircuit(powers, circuit, key, { vk, seed });
        if (!v.ok || v.checksRun !== 0x3ff || v.checksBad !== 0 || v.checks.A !== true || v.checks.IC !== true || !(v.ms.total > 0))
            throw new Error("good key: " + JSON.stringify(v));
    }
    const plain = await bn.checkKeyCircuit(powers, circuit, rd("key.bin"));      // a seed from the OS
    if (!plain.ok || plain.checksRun !== 0xff || plain.checks.IC !== null || plain.checks.vk_fixed_points !== null) throw new Error("no vk: " + JSON.stringify(plain));
    // a wrong key and a wrong verification key are results
    const t = await bn.checkKeyCircuit(powers, circuit, rd("tampered_key.bin"), { vk, seed });
    if (t.ok || t.checksRun !== 0x3ff || t.checksBad !== 8 || t.checks.A !== false || t.checks.B1 !== true) throw new Error("tampered key: " + JSON.stringify(t));
    const u = await bn.checkKeyCircuit(powers, circuit, rd("key.bin"), { vk: badVk, seed });
    if (u.ok || u.checksRun !== 0x3ff || u.checksBad !== 512 || u.checks.IC !== false) throw new Error("tampered vk: " + JSON.stringify(u));
    // what the loaders reject is a rejection
    let err = null;
    try { await bn.checkKeyCircuit(Object.assign({}, powers, { tauG2: powers.tauG2.subarray(0, powers.tauG2.length - 128) }), circuit, rd("key.bin")); } catch (e) { err = e; }
    if (!err || !/wsnark error 2/.test(err.message)) throw new Error("short array: " + err);
    bn.terminate();
    console.log("NODE_PKEY_CIRCUIT_OK");
})().catch((e) => { console.error(e); process.exit(1); });
