// Drives circuitFromRows and loadCircuit({rows}) of wasmsnark_amd/js over the files tests/test_node_circuit_rows.py wrote to argv[2]:
// a circuit row by row ({A,B,C}_{row_ptr,col,coef}.bin), what the Python side's circuit_from_rows made of it (polsA.bin, polsB.bin,
// polsC.bin), a good and a bad witness, and expect.json (the counts, the report, and what check_witness says about the bad witness).
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
// a file's bytes in an ArrayBuffer of their own: typed arrays of 8- and 4-byte elements need the alignment
const own = (n) => { const b = rd(n); const ab = new ArrayBuffer(b.length); Buffer.from(ab).set(b); return ab; };

(async () => {
    const want = JSON.parse(rd("expect.json").toString("utf8"));
    const bn = await ws.buildBn128();
    const rows = { nVars: want.nVars, nPublic: want.nPublic, nConstraints: want.nConstraints };
    for (const m of ["A", "B", "C"])
        rows[m] = { rowPtr: new BigUint64Array(own(m + "_row_ptr.bin")), col: new Uint32Array(own(m + "_col.bin")), coef: rd(m + "_coef.bin") };
    const [c1, c2] = await Promise.all([bn.circuitFromRows(rows), bn.circuitFromRows(rows, { publicRows: true })]);
    for (const c of [c1, c2]) {
        if (c.nVars !== want.nVars || c.nPublic !== want.nPublic || c.domain !== want.domain) throw new Error("circuitFromRows: the counts");
        for (const name of ["polsA", "polsB", "polsC"])
            if (!Buffer.from(c[name]).equals(rd(name + ".bin"))) throw new Error("circuitFromRows: " + name + " differs from the Python side's");
        for (const name of ["nnz", "unreduced", "zero", "emptySignals", "maxColumn"])
            if (!same(c.report[name], want.report[name])) throw new Error("circuitFromRows: report." + name + " " + JSON.stringify(c.report[name]));
        if (!(c.report.ms.total >= c.report.ms.kernels && c.report.ms.kernels > 0)) throw new Error("circuitFromRows: report.ms");
    }
    // without the public rows: another domain, A shorter by nPublic + 1 records
    const c3 = await bn.circuitFromRows(rows, { publicRows: false });
    if (c3.domain !== want.domainWithout || c3.polsA.length !== c1.polsA.length - 36 * (want.nPublic + 1) || !Buffer.from(c3.polsB).equals(Buffer.from(c1.polsB)))
        throw new Error("circuitFromRows without public rows");
    // the resident circuit from rows against the one from the streams
    const good = rd("good_witness.bin"), bad = rd("bad_witness.bin");
    const [ra, rb] = await Promise.all([bn.loadCircuit(c1), bn.loadCircuit({ rows })]);
    if (!same(ra.info(), rb.info()) || rb.info().domain !== want.domain || !same(rb.info().nnz, want.report.nnz)) throw new Error("loadCircuit({rows}): info " + JSON.stringify(rb.info()));
    const strip = (r) => JSON.stringify(r, (k, v) => (k === "ms" ? undefined : typeof v === "bigint" ? String(v) : v));
    for (const w of [good, bad]) {
        const [x, y] = await Promise.all([ra.checkWitness(w, { maxRows: want.domain }), rb.checkWitness(w, { maxRows: want.domain })]);
        if (strip(x) !== strip(y)) throw new Error("loadCircuit({rows}): checkWitness differs");
    }
    const g = await rb.checkWitness(good), b = await rb.checkWitness(bad, { maxRows: want.domain });
    if (!g.ok || g.bad !== 0) throw new Error("the good witness: " + strip(g));
    if (b.ok || b.bad !== want.bad || b.firstBad !== want.first_bad || !same(b.badRows, want.bad_rows) ||
        !same(b.badValues.map((abc) => abc.map(String)), want.bad_values)) throw new Error("the bad witness: " + strip(b));
    const v = await rb.checkWitnesses([good, bad, good], { maxRows: 1 });
    if (!same(v.map((r) => r.ok), [true, false, true]) && !same(v.map((r) => r.ok), [1, 0, 1])) throw new Error("checkWitnesses: " + strip(v));
    // what the library rejects is a rejection; what the addon cannot pass on safely is a TypeError
    let err = null;
    const col = new Uint32Array(rows.B.col);
    col[0] = want.nVars;
    try { await bn.circuitFromRows(Object.assign({}, rows, { B: Object.assign({}, rows.B, { col }) })); } catch (e) { err = e; }
    if (!err || !/wsnark error 2/.test(err.message) || !/ B,/.test(err.message) || !/entry 0/.test(err.message)) throw new Error("a signal >= nVars: " + err);
    err = null;
    try { await bn.loadCircuit({ rows: Object.assign({}, rows, { domain: 48 }) }); } catch (e) { err = e; }
    if (!err || !/wsnark error 1/.test(err.message)) throw new Error("domain 48: " + err);
    err = null;
    try { await bn.circuitFromRows(Object.assign({}, rows, { C: Object.assign({}, rows.C, { coef: rows.C.coef.subarray(1) }) })); } catch (e) { err = e; }
    if (!(err instanceof TypeError)) throw new Error("a short coef array: " + err);
    ra.free();
    rb.free();
    bn.terminate();
    console.log("NODE_CIRCUIT_ROWS_OK");
})().catch((e) => { console.error(e); process.exit(1); });
