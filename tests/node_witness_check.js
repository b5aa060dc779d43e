// Drives checkWitness, loadCircuit and groth16GenProof's {circuit} option of wasmsnark_amd/js over the files
// tests/test_node_witness_check.py wrote to argv[2]: the circuit's three record streams (and those of a larger circuit, other_*),
// good_witness.bin, bad_witness.bin (two signals changed), key.bin (a proving key of the circuit) and expect.json (the counts, and
// what Python integers say about the bad witness: bad, first_bad, bad_rows, and a, b, c of every bad row as decimal strings).
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

function checkGood(r, want, where) {
    if (!r.ok || r.bad !== 0 || r.firstBad !== null || r.listed !== 0 || !r.oneOk || r.unreduced !== 0 || r.firstUnreduced !== null ||
        r.rows !== want.domain || r.badRows.length || r.badValues.length || !(r.ms.total > 0))
        throw new Error(where + ", good witness: " + JSON.stringify(r, (k, v) => (typeof v === "bigint" ? String(v) : v)));
}
function checkBad(r, want, cap, where) {
    const listed = Math.min(want.bad, cap);
    const values = r.badValues.map((abc) => abc.map(String));
    if (r.ok || r.bad !== want.bad || r.firstBad !== want.first_bad || r.listed !== listed || !r.oneOk || r.rows !== want.domain ||
        !same(r.badRows, want.bad_rows.slice(0, listed)) || !same(values, want.bad_values.slice(0, listed)))
        throw new Error(where + ", bad witness, maxRows " + cap + ": " + JSON.stringify(r, (k, v) => (typeof v === "bigint" ? String(v) : v)));
}

(async () => {
    const want = JSON.parse(rd("expect.json").toString("utf8"));
    const bn = await ws.buildBn128();
    const circuit = { nVars: want.nVars, nPublic: want.nPublic, domain: want.domain, polsA: rd("polsA.bin"), polsB: rd("polsB.bin"), polsC: rd("polsC.bin") };
    const good = rd("good_witness.bin"), bad = rd("bad_witness.bin"), key = rd("key.bin");
    // the one-shot call
    checkGood(await bn.checkWitness(circuit, good), want, "checkWitness");
    for (const cap of [0, 1, want.domain]) checkBad(await bn.checkWitness(circuit, bad, { maxRows: cap }), want, cap, "checkWitness");
    checkBad(await bn.checkWitness(circuit, bad), want, 16, "checkWitness");
    // the resident circuit; two checks side by side on the one handle
    const rc = await bn.loadCircuit(circuit);
    const inf = rc.info();
    if (inf.nVars !== want.nVars || inf.nPublic !== want.nPublic || inf.domain !== want.domain || !same(inf.nnz, want.nnz) || !(inf.bytes > 0))
        throw new Error("info: " + JSON.stringify(inf));
    const [g, b] = await Promise.all([rc.checkWitness(good), rc.checkWitness(bad, { maxRows: want.domain })]);
    checkGood(g, want, "loadCircuit");
    checkBad(b, want, want.domain, "loadCircuit");
    checkBad(await rc.checkWitness(bad, { maxRows: 1 }), want, 1, "loadCircuit");
    // what the library rejects is a rejection: a short witness, a truncated stream
    let err = null;
    try { await rc.checkWitness(good.subarray(0, good.length - 1)); } catch (e) { err = e; }
    if (!err || !/wsnark error 1/.test(err.message)) throw new Error("short witness: " + err);
    err = null;
    try { await bn.checkWitness(Object.assign({}, circuit, { polsC: circuit.polsC.subarray(0, circuit.polsC.length - 1) }), good); } catch (e) { err = e; }
    if (!err || !/wsnark error 2/.test(err.message)) throw new Error("truncated polsC: " + err);
    err = null;
    try { await bn.loadCircuit(Object.assign({}, circuit, { domain: 48 })); } catch (e) { err = e; }
    if (!err || !/wsnark error 1/.test(err.message)) throw new Error("domain 48: " + err);
    // groth16GenProof with {circuit}: the good witness gives the proof it gives without; the bad one names its first bad constraint
    const r = Buffer.alloc(32, 3), s = Buffer.alloc(32, 5);
    const plain = await bn.groth16GenProof(good, key, { r, s });
    if (!same(await bn.groth16GenProof(good, key, { r, s, circuit: rc }), plain)) throw new Error("{circuit} changed the proof of a good witness");
    err = null;
    try { await bn.groth16GenProof(bad, key, { r, s, circuit: rc }); } catch (e) { err = e; }
    const v0 = want.bad_values[0];
    const text = `constraint ${want.first_bad}: (A.w)(B.w) != C.w: a=${v0[0]}, b=${v0[1]}, c=${v0[2]}`;
    if (!err || !err.message.includes(text) || !err.report || err.report.bad !== want.bad) throw new Error("bad witness with {circuit}: " + err);
    if (same(await bn.groth16GenProof(bad, key, { r, s }), plain)) throw new Error("without {circuit} a bad witness still proves, to another proof");
    const other = await bn.loadCircuit({ nVars: want.otherNVars, nPublic: want.nPublic, domain: want.otherDomain, polsA: rd("other_polsA.bin"),
                                         polsB: rd("other_polsB.bin"), polsC: rd("other_polsC.bin") });
    err = null;
    try { await bn.groth16GenProof(bad, key, { r, s, circuit: other }); } catch (e) { err = e; }
    if (!err || !/is not the key's/.test(err.message)) throw new Error("a circuit of another shape: " + err);
    other.free();
    rc.free();
    err = null;
    try { await rc.checkWitness(good); } catch (e) { err = e; }
    if (!err || !/freed/.test(err.message)) throw new Error("a freed circuit: " + err);
    bn.terminate();
    console.log("NODE_WITNESS_CHECK_OK");
})().catch((e) => { console.error(e); process.exit(1); });
