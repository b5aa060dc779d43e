/*
 * Drop-in for wasmsnark's BN128 prover API on an MI355X (see ../../INTEGRATION.md).
 *
 * Same names and shapes as the reference:
 *   buildBn128() -> Promise<Bn128>                          (reference index.js:21, src/bn128.js:173-265)
 *   buildBn128({devices: [0, 1, ...]}) -> the same object over SEVERAL GPUs of this one process: the reference's worker pool
 *       (src/bn128.js:173-265: `build()` starts its workers; :353-415, :607-622: every sum is cut into one contiguous range of the
 *       pairs per worker and the partial results are added) with GPUs as the workers -- a points shard of the key per device,
 *       CALC_H on the distributed transform, the transport inside libwsnark.so (csrc/group.hip)
 *   Bn128.groth16GenProof(signals, pkey) -> Promise<{pi_a, pi_b, pi_c}> of decimal strings (src/bn128.js:580-720)
 *   Bn128.g1_multiexp / g2_multiexp / calcH / terminate      (src/bn128.js:353-415, 569-578, 562-566)
 *   groth16GenProof(witness, provingKey[, cb]) and the README name genZKSnarkProof (main_bn128.js:26-39, README.md:28-30)
 * Inputs may be ArrayBuffer (what the reference requires), Buffer or TypedArray.
 * All arithmetic runs in libwsnark.so (hand-written HIP); this file only marshals and formats.
 */
"use strict";
const addon = require("./build/wsnark_napi.node");
addon.g1g2 = (which, scalars, points) => (which ? addon.g2Multiexp(scalars, points) : addon.g1Multiexp(scalars, points));

// bin2int / bin2g1 / bin2g2 (src/bn128.js:319-351, 714-718): the twelve 256-bit integers of a proof as decimal strings, formatted in
// the addon (native code, no BigInt: ~5 us)
function proofFromBytes(ab) { return addon.proofToObject(ab); }

/* Two checks that a cached key handle still describes the bytes the caller is holding.
 *   fingerprint(u8): synchronous, a few KiB -- the 488-byte header + fixed points, 64 samples of 32 bytes spread over the buffer and
 *                    its tail.  It catches a buffer that was refilled with another key.
 *   digest(u8):      ALL of the bytes (addon.hashBytes, off the event loop, several threads; ~10 ms for a 0.6 GB key).
 * The reference re-parses pkey inside every call (src/bn128.js:581-604): a caller may patch a few bytes of a key between two proofs
 * and is served with the new key.  The DEFAULT here gives the same guarantee (round 5): every call that is handed key BYTES takes
 * the digest of all of them -- groth16GenProof takes it BESIDE the proof on the cached handle and, should it differ from the
 * digest taken when that handle was loaded, loads the new bytes and proves again (the stale proof is never returned).  Callers who
 * know their key bytes do not change opt into the sampled check alone with {trustCache: true}; callers who want no check at all hold
 * the handle of loadKey() and pass that. */
/* the verifier's plain layout (alfa1 | beta2 | gamma2 | delta2 | IC[0 .. nPublic]) -> the verification key object */
function vkFromBytes(vkb) {
    const nPublic = (vkb.length - 448) / 64 - 1;
    const dec = (o) => { let x = 0n; for (let i = 31; i >= 0; i--) x = (x << 8n) | BigInt(vkb[o + i]); return x.toString(); };
    const g1 = (o) => [dec(o), dec(o + 32), "1"], g2 = (o) => [[dec(o), dec(o + 32)], [dec(o + 64), dec(o + 96)], ["1", "0"]];
    const vk = { protocol: "groth", nPublic, vk_alfa_1: g1(0), vk_beta_2: g2(64), vk_gamma_2: g2(192), vk_delta_2: g2(320), IC: [] };
    for (let i = 0; i <= nPublic; i++) vk.IC.push(g1(448 + 64 * i));
    return vk;
}
/* do these bytes, or does this file, begin with a .zkey's magic?  (decided by the first four bytes, never by a file's name) */
function isZkey(x) {
    if (typeof x === "string") {
        const fs = require("fs"), b = Buffer.alloc(4), fd = fs.openSync(x, "r");
        try { return fs.readSync(fd, b, 0, 4, 0) === 4 && b.toString("latin1") === "zkey"; } finally { fs.closeSync(fd); }
    }
    const u8 = asBytes(x);
    return u8.byteLength >= 4 && u8[0] === 0x7a && u8[1] === 0x6b && u8[2] === 0x65 && u8[3] === 0x79;
}
/* the addon's handle of a .zkey load: zkeyOut (the report, the vk's bytes) becomes .report and .vk */
async function zkeyHandle(load) {
    const h = await load;
    if (h.zkeyOut) {
        h.report = zkeyReport(new DataView(h.zkeyOut), 0);
        h.vk = vkFromBytes(Buffer.from(h.zkeyOut, 136));
        delete h.zkeyOut;
    }
    return h;
}
async function digest(u8) {
    return Buffer.from(await addon.hashBytes(u8)).toString("hex");
}
function fingerprint(u8) {
    const n = u8.byteLength;
    const b = Buffer.from(u8.buffer, u8.byteOffset, n);          // (a view: no copy)
    let h1 = 0x811c9dc5 | 0, h2 = 0x9e3779b9 | 0;                 // two 32-bit multiply-xor lanes over the sampled words (no BigInt: microseconds)
    const take = (off, len) => {
        const end = Math.min(off + len, n);
        let i = off;
        for (; i + 4 <= end; i += 4) {
            const w = b.readUInt32LE(i);
            h1 = Math.imul(h1 ^ w, 0x01000193);
            h2 = Math.imul((h2 ^ w) + ((h2 << 13) | (h2 >>> 19)), 0x85ebca6b);
        }
        for (; i < end; i++) { h1 = Math.imul(h1 ^ b[i], 0x01000193); h2 = Math.imul(h2 ^ b[i], 0x85ebca6b); }
    };
    take(0, 488);
    const step = Math.max(32, Math.floor(n / 64 / 32) * 32);
    for (let k = 1; k <= 64; k++) if (k * step <= n) take(k * step - 32, 32);
    take(Math.max(0, n - 64), 64);
    return (h1 >>> 0).toString(16) + (h2 >>> 0).toString(16) + ":" + n;
}
function asBytes(x) {
    if (x instanceof ArrayBuffer) return new Uint8Array(x);
    if (ArrayBuffer.isView(x)) return new Uint8Array(x.buffer, x.byteOffset, x.byteLength);
    throw new TypeError("expected an ArrayBuffer, Buffer or TypedArray");
}

/* wsnark_pkey_report_t (include/wsnark.h, 248 bytes) -> the object checkKey() resolves to: per-section objects keyed A, B1, B2, C,
 * H ({points, infinity, bad, firstBad, firstReason}), then fixed, relations (true holds / false violated / null not run), ok, ms.
 * Counts are Numbers (a section has at most 2^27 points). */
const KEY_SECTIONS = ["A", "B1", "B2", "C", "H"], KEY_FIXED = ["alfa1", "beta1", "delta1", "beta2", "delta2"];
const KEY_RELATIONS = ["beta1~beta2", "delta1~delta2", "B1~B2"], KEY_REASONS = [null, "unreduced", "off_curve", "outside_subgroup", "infinity"];
function keyReport(ab) {
    const v = new DataView(ab);
    const u64 = (o) => Number(v.getBigUint64(o, true));
    const out = {};
    KEY_SECTIONS.forEach((name, k) => {
        const bad = u64(80 + 8 * k);
        out[name] = { points: u64(8 * k), infinity: u64(40 + 8 * k), bad, firstBad: bad ? u64(120 + 8 * k) : null,
                      firstReason: bad ? KEY_REASONS[v.getUint32(160 + 4 * k, true)] : null };
    });
    out.fixed = {};
    KEY_FIXED.forEach((name, k) => { out.fixed[name] = KEY_REASONS[v.getUint32(180 + 4 * k, true)]; });
    const run = v.getUint32(200, true), bad = v.getUint32(204, true);
    out.relations = {};
    KEY_RELATIONS.forEach((name, k) => { out.relations[name] = (run >> k) & 1 ? !((bad >> k) & 1) : null; });
    out.relationsRun = run;
    out.relationsBad = bad;
    out.ok = v.getUint32(208, true) === 1;
    out.ms = { points: v.getFloat64(216, true), relationSums: v.getFloat64(224, true), pairings: v.getFloat64(232, true), total: v.getFloat64(240, true) };
    return out;
}
/* wsnark_pkey_delta_report_t (104 bytes) and wsnark_pkey_delta_verdict_t (40 bytes) -> the objects of contributeKey() / verifyContribution() */
const DELTA_CHECKS = ["unchanged", "delta1~delta2", "C", "H", "delta_changed"];
function deltaReport(ab) {
    const v = new DataView(ab, 0, 104);
    const u64 = (o) => Number(v.getBigUint64(o, true));
    const out = {};
    ["C", "H"].forEach((name, k) => {
        const bad = u64(32 + 8 * k);
        out[name] = { points: u64(8 * k), infinity: u64(16 + 8 * k), bad, firstBad: bad ? u64(48 + 8 * k) : null,
                      firstReason: bad ? KEY_REASONS[v.getUint32(64 + 4 * k, true)] : null };
    });
    out.ok = v.getUint32(72, true) === 1;
    out.ms = { device: v.getFloat64(80, true), host: v.getFloat64(88, true), total: v.getFloat64(96, true) };
    return out;
}
function deltaVerdict(ab) {
    const v = new DataView(ab);
    const run = v.getUint32(0, true), bad = v.getUint32(4, true);
    const out = { checks: {}, checksRun: run, checksBad: bad, ok: v.getUint32(8, true) === 1,
                  ms: { sums: v.getFloat64(16, true), pairings: v.getFloat64(24, true), total: v.getFloat64(32, true) } };
    DELTA_CHECKS.forEach((name, k) => { out.checks[name] = (run >> k) & 1 ? !((bad >> k) & 1) : null; });
    return out;
}
/* wsnark_pkey_circuit_verdict_t (56 bytes) -> the object of checkKeyCircuit() */
const CIRCUIT_CHECKS = ["shape_and_streams", "fixed_points", "delta1~delta2", "A", "B1", "B2", "C", "H", "vk_fixed_points", "IC"];
/* the addon's arguments for a circuit in row form: the counts, the flags (bit 0: append the public rows) and the nine arrays */
function rowsArgs(rows, publicRows) {
    const bufs = [];
    for (const name of ["A", "B", "C"]) {
        const m = rows[name];
        if (!m || !(m.rowPtr instanceof BigUint64Array) || !(m.col instanceof Uint32Array))
            throw new TypeError("wsnark: rows." + name + " must be {rowPtr: BigUint64Array, col: Uint32Array, coef: bytes}");
        asBytes(m.coef);
        bufs.push(Buffer.from(m.rowPtr.buffer, m.rowPtr.byteOffset, m.rowPtr.byteLength), Buffer.from(m.col.buffer, m.col.byteOffset, m.col.byteLength), m.coef);
    }
    return [rows.nVars, rows.nPublic, rows.nConstraints, rows.domain || 0, publicRows === false ? 0 : 1, bufs];
}
function circuitVerdict(ab) {
    const v = new DataView(ab);
    const run = v.getUint32(0, true), bad = v.getUint32(4, true);
    const out = { checks: {}, checksRun: run, checksBad: bad, ok: v.getUint32(8, true) === 1,
                  ms: { matrices: v.getFloat64(16, true), keySums: v.getFloat64(24, true), powersSums: v.getFloat64(32, true),
                        pairings: v.getFloat64(40, true), total: v.getFloat64(48, true) } };
    CIRCUIT_CHECKS.forEach((name, k) => { out.checks[name] = (run >> k) & 1 ? !((bad >> k) & 1) : null; });
    return out;
}
/* wsnark_pkey_setup_report_t (192 bytes) -> the report object of newKey() */
const POWERS_ARRAYS = ["tauG1", "tauG2", "alphaTauG1", "betaTauG1"];
function setupReport(ab) {
    const v = new DataView(ab, 0, 192);
    const u64 = (o) => Number(v.getBigUint64(o, true));
    const out = {};
    POWERS_ARRAYS.forEach((name, k) => {
        const bad = u64(64 + 8 * k);
        out[name] = { points: u64(8 * k), infinity: u64(32 + 8 * k), bad, firstBad: bad ? u64(96 + 8 * k) : null,
                      firstReason: bad ? KEY_REASONS[v.getUint32(128 + 4 * k, true)] : null };
    });
    out.betaG2 = KEY_REASONS[v.getUint32(144, true)];
    out.ok = v.getUint32(148, true) === 1;
    out.msmColumns = v.getUint32(152, true);
    out.ms = { transforms: v.getFloat64(160, true), columnSums: v.getFloat64(168, true), hexps: v.getFloat64(176, true), total: v.getFloat64(184, true) };
    return out;
}
/* wsnark_powers_report_t (192 bytes) -> the report object of contributePowers() and checkPowers(); relations: true holds, false
 * violated, null not run */
const POWERS_RELATIONS = ["generators", "tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2"];
function powersReport(ab, msNames) {
    const v = new DataView(ab, 0, 192);
    const u64 = (o) => Number(v.getBigUint64(o, true));
    const out = {};
    POWERS_ARRAYS.forEach((name, k) => {
        const bad = u64(64 + 8 * k);
        out[name] = { points: u64(8 * k), infinity: u64(32 + 8 * k), bad, firstBad: bad ? u64(96 + 8 * k) : null,
                      firstReason: bad ? KEY_REASONS[v.getUint32(128 + 4 * k, true)] : null };
    });
    out.betaG2 = KEY_REASONS[v.getUint32(144, true)];
    const run = v.getUint32(148, true), bad = v.getUint32(152, true);
    out.relations = {};
    POWERS_RELATIONS.forEach((name, k) => { out.relations[name] = (run >> k) & 1 ? !((bad >> k) & 1) : null; });
    out.relationsRun = run;
    out.relationsBad = bad;
    out.ok = v.getUint32(156, true) === 1;
    out.ms = {};
    msNames.forEach((name, k) => { if (name) out.ms[name] = v.getFloat64(160 + 8 * k, true); });
    return out;
}
/* wsnark_witness_report_t (80 bytes) and its two lists of `cap` entries -> the object of checkWitness(): counts are Numbers, firstBad /
 * firstUnreduced null when there is none, badRows Numbers, badValues [a, b, c] BigInts of each listed row */
function witnessReport(ab, cap) {
    const v = new DataView(ab);
    const u64 = (o) => Number(v.getBigUint64(o, true));
    const big = (o) => { let x = 0n; for (let i = 3; i >= 0; i--) x = (x << 64n) | v.getBigUint64(o + 8 * i, true); return x; };
    const bad = u64(8), unreduced = u64(32), listed = u64(24);
    const out = { rows: u64(0), bad, firstBad: bad ? u64(16) : null, listed, unreduced, firstUnreduced: unreduced ? u64(40) : null,
                  oneOk: v.getUint32(48, true) === 1, ok: v.getUint32(52, true) === 1,
                  ms: { matrices: v.getFloat64(56, true), device: v.getFloat64(64, true), total: v.getFloat64(72, true) }, badRows: [], badValues: [] };
    for (let j = 0; j < listed; j++) {
        out.badRows.push(u64(80 + 8 * j));
        const o = 80 + 8 * cap + 96 * j;
        out.badValues.push([big(o), big(o + 32), big(o + 64)]);
    }
    return out;
}
/* the buffer of addon.circuitCheckWitnesses -- wsnark_witness_batch_report_t (64 bytes), count wsnark_witness_verdict_t (48 bytes each),
 * count x cap row indices, count x cap x 96 bytes of values -- -> {verdicts: per witness the object of checkWitness() without rows and
 * ms, report: {count, rows, good, firstNotOk (null: none), chunk, ms}} */
function witnessVerdicts(ab, count, cap) {
    const v = new DataView(ab);
    const u64 = (o) => Number(v.getBigUint64(o, true));
    const big = (o) => { let x = 0n; for (let i = 3; i >= 0; i--) x = (x << 64n) | v.getBigUint64(o + 8 * i, true); return x; };
    const good = u64(16);
    const report = { count: u64(0), rows: u64(8), good, firstNotOk: good === count ? null : u64(24), chunk: v.getUint32(32, true),
                     ms: { matrices: v.getFloat64(40, true), device: v.getFloat64(48, true), total: v.getFloat64(56, true) } };
    const rowsAt = 64 + 48 * count, valuesAt = rowsAt + 8 * count * cap;
    const verdicts = [];
    for (let i = 0; i < count; i++) {
        const o = 64 + 48 * i, bad = u64(o), unreduced = u64(o + 16), listed = u64(o + 32);
        const one = { bad, firstBad: bad ? u64(o + 8) : null, listed, unreduced, firstUnreduced: unreduced ? u64(o + 24) : null,
                      oneOk: v.getUint32(o + 40, true) === 1, ok: v.getUint32(o + 44, true) === 1, badRows: [], badValues: [] };
        for (let j = 0; j < listed; j++) {
            one.badRows.push(u64(rowsAt + 8 * (i * cap + j)));
            const q = valuesAt + 96 * (i * cap + j);
            one.badValues.push([big(q), big(q + 32), big(q + 64)]);
        }
        verdicts.push(one);
    }
    return { verdicts, report };
}
/* an array of witness buffers (each at least `stride` bytes), or ONE buffer holding them back to back -> {blob, count} */
function witnessBlob(witnesses, stride) {
    if (Array.isArray(witnesses)) {
        const ws = witnesses.map(asBytes);
        if (ws.some((w) => w.byteLength < stride)) throw new Error("wsnark: a witness is shorter than nVars x 32 bytes");
        const blob = new Uint8Array(stride * ws.length);
        ws.forEach((w, i) => blob.set(w.subarray(0, stride), stride * i));
        return { blob, count: ws.length };
    }
    const blob = asBytes(witnesses);
    if (stride === 0 || blob.byteLength % stride) throw new Error("wsnark: not a whole number of nVars x 32-byte witnesses");
    return { blob, count: blob.byteLength / stride };
}
function witnessFinding(rep) {
    if (rep.bad) {
        let text = `constraint ${rep.firstBad}: (A.w)(B.w) != C.w`;
        if (rep.badRows.length && rep.badRows[0] === rep.firstBad) text += `: a=${rep.badValues[0][0]}, b=${rep.badValues[0][1]}, c=${rep.badValues[0][2]}`;
        return text + (rep.bad > 1 ? ` (${rep.bad} bad constraints in all)` : "");
    }
    if (!rep.oneOk) return "signal 0 is not 1";
    return rep.ok ? null : `public signal >= r (the first unreduced signal is ${rep.firstUnreduced})`;
}
const maxRowsOf = (opts) => (opts && opts.maxRows !== undefined ? opts.maxRows : 16);
function firstFinding(rep) {
    for (const name of KEY_SECTIONS) if (rep[name].bad) return `${rep[name].bad} bad point(s) in section ${name}, the first at index ${rep[name].firstBad}: ${rep[name].firstReason}`;
    for (const name of KEY_FIXED) if (rep.fixed[name]) return `${name}: ${rep.fixed[name]}`;
    for (const name of KEY_RELATIONS) if (rep.relations[name] === false) return `relation ${name} does not hold`;
    return "a requested relation could not be run";
}

class Bn128 {
    constructor(deviceInfo, group, devices) {
        this.deviceInfo = deviceInfo;
        this._group = group || null;      // several GPUs: wsnark_group_* (keys are points shards over the devices, proofs run on all of them)
        this.devices = devices || null;
        // proving-key OBJECT (the exact ArrayBuffer / view the caller passed) -> {handle (a Promise), byteOffset, byteLength,
        // fp (sampled fingerprint), digest (Promise of the whole-buffer digest taken at load time)}.
        // Two views of one ArrayBuffer (sub-arrays of a bundle, Node's pooled small Buffers) are different keys here.
        // A cached handle is reused while offset, length and the sampled fingerprint still match -- and, for callers that
        // ask ({trustCache: false}), the digest of the WHOLE buffer; see fingerprint() / digest() above.
        this._keys = new WeakMap();
        this._files = new Map();    // key FILE path -> {size, mtimeMs, handle (a Promise)}
        this.fullDigests = 0;   // how many whole-buffer digests this object has computed (tests, tools/node_bench.js)
        this._pr = null;     // blinding values of the last proof, "for tests" like the reference (src/bn128.js:662-664)
        this._ps = null;
        this._live = true;
    }
    /* points: the bytes (as in the reference, src/bn128.js:353-415), or a handle from loadPoints() */
    g1_multiexp(scalars, points) { return this._msm(0, scalars, points); }
    g2_multiexp(scalars, points) { return this._msm(1, scalars, points); }
    _msm(which, scalars, points) {
        if (!this._live) return Promise.reject(new Error("wsnark: this Bn128 object has been terminated"));
        if (points !== null && typeof points === "object" && !(points instanceof ArrayBuffer) && !ArrayBuffer.isView(points)) return addon.pointsMultiexp(points, scalars);
        return this._group ? addon.groupMultiexp(this._group, which, scalars, points) : addon.g1g2(which, scalars, points);
    }
    /* No counterpart in the reference: bases that are summed over again and again (a prover's key sections) made RESIDENT once, as
     * fixed-base window tables -- later g1_multiexp / g2_multiexp calls that pass the handle instead of the bytes pay neither the
     * points' upload nor the per-window plans (about half the time of a 2^20 sum).  group: 1 or 2. */
    loadPoints(group, points) { return addon.loadPoints(group, points); }
    /* No counterpart in the reference: KZG commitments on a transcript's tauG1 powers (include/wsnark.h: wsnark_kzg_*).  Scalars --
     * coefficients, z, gamma, values -- are 32 bytes plain little-endian, reduced mod r; a polynomial is len coefficients, lowest degree
     * first, count of them back to back; points are 64-byte affine Montgomery points, infinity is zero bytes.
     * kzgLoadSrs(tauG1) resolves to a handle (freed by the GC); a bad power or one at infinity rejects with the first index.
     * kzgCommit(srs, polys, len, opts): opts.form === 1 takes evaluations on the domain of fft(); resolves to count x 64 bytes.
     * kzgOpen(srs, polys, len, z, gamma): {ys: count x 32 bytes, proof: 64 bytes}, ONE proof for sum_i gamma^i f_i; gamma (the caller's
     * Fiat-Shamir challenge) may be left out for one polynomial.
     * kzgVerify(g1, g2Pair (g2 | tau g2), commitments, z, ys, proof, gamma): boolean, on the host.
     * polyEval(polys, len, z): count x 32 bytes.  polyDivide(poly, z): {q: (f - f(z)) / (X - z), y: f(z)}. */
    _kzgReady() {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (this._group) throw new Error("wsnark: the KZG calls run on a single GPU (build a Bn128 without {devices})");
    }
    async kzgLoadSrs(tauG1) { this._kzgReady(); asBytes(tauG1); return addon.kzgLoadSrs(tauG1); }
    async kzgCommit(srs, polys, len, opts) { this._kzgReady(); asBytes(polys); return addon.kzgCommit(srs, polys, len, opts && opts.form === 1 ? 1 : 0); }
    async kzgOpen(srs, polys, len, z, gamma) {
        this._kzgReady();
        asBytes(polys);
        const ab = await addon.kzgOpen(srs, polys, len, z, gamma || null);
        return { ys: ab.slice(0, ab.byteLength - 64), proof: ab.slice(ab.byteLength - 64) };
    }
    async kzgVerify(g1, g2Pair, commitments, z, ys, proof, gamma) { return addon.kzgVerify(g1, g2Pair, commitments, z, gamma || null, ys, proof); }
    async polyEval(polys, len, z) { this._kzgReady(); asBytes(polys); return addon.polyEval(polys, len, z); }
    async polyDivide(poly, z) {
        this._kzgReady();
        asBytes(poly);
        const ab = await addon.polyDivide(poly, z);
        return { q: ab.slice(0, ab.byteLength - 32), y: ab.slice(ab.byteLength - 32) };
    }
    calcH(signals, polsA, polsB, nSignals, domainSize) { return addon.calcH(signals, polsA, polsB, nSignals, domainSize); }
    fft(buf, odd) { return addon.fft(buf, odd | 0, false); }
    ifft(buf, odd) { return addon.fft(buf, odd | 0, true); }
    /* the cache entry of a key object if offset, length and the sampled fingerprint still match its bytes */
    _cached(pkey, u8) {
        const hit = this._keys.get(pkey);
        return hit && hit.byteOffset === u8.byteOffset && hit.byteLength === u8.byteLength && hit.fp === fingerprint(u8) ? hit : null;
    }
    /* pkey bytes -> device-resident key handle (stays in HBM across proofs; freed by the GC).
     * Bytes (or a file: _loadKeyFile) that begin with "zkey" are a snarkjs .zkey: it is loaded straight into the resident key
     * (include/wsnark.h: wsnark_pkey_load_zkey*), the handle carries .vk -- the file's verification key object -- and .report, and
     * groth16GenProof(witness | wtns, zkey bytes | that handle) follows, digest cache included.  NOT audited, like importZkey; one GPU.
     * A cached handle is returned when the digest of ALL bytes equals the one taken when it was loaded; opts.trustCache === true: when
     * the sampled fingerprint does.  Concurrent callers with the same key object share ONE load: the entry is in the map before it is awaited. */
    async loadKey(pkey, opts) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (opts && opts.check === true) {           // opt-in: audit the bytes first (they then cross the link twice); the Error carries .report
            const report = await this.checkKey(pkey);
            if (!report.ok) throw Object.assign(new Error("wsnark: proving key failed its audit: " + firstFinding(report)), { report });
        }
        if (typeof pkey === "string") return this._loadKeyFile(pkey);
        if (pkey !== null && typeof pkey === "object" && !(pkey instanceof ArrayBuffer) && !ArrayBuffer.isView(pkey)) return pkey;   // already a handle
        const u8 = asBytes(pkey);
        const hit = this._cached(pkey, u8);
        if (hit) {
            if (opts && opts.trustCache === true) return hit.handle;                     // (a Promise: resolved, or the load in flight)
            this.fullDigests++;
            if ((await hit.digest) === (await digest(u8))) return hit.handle;
        }
        // The digest is taken beside the load (addon.hashBytes deals the buffer's blocks to several threads: ~10 ms for a 0.6 GB
        // key, a quarter of the load) and loadKey() resolves only when BOTH are done: a caller who rewrites bytes in place as
        // soon as the first call returns must find them compared against the bytes that were loaded, not against a digest that
        // was still being taken while they changed.
        // a snarkjs .zkey goes straight into the resident key (wsnark_pkey_load_zkey): the handle carries .vk and .report
        const zkey = isZkey(u8);
        if (zkey && this._group) throw new Error("wsnark: a .zkey is loaded on a single GPU (build a Bn128 without {devices}, or importZkey it first)");
        const load = zkey ? zkeyHandle(addon.loadKeyZkey(pkey)) : this._group ? addon.groupLoadKey(this._group, pkey) : addon.loadKey(pkey);
        const entry = { byteOffset: u8.byteOffset, byteLength: u8.byteLength, fp: fingerprint(u8), handle: load, digest: digest(u8) };
        this.fullDigests++;
        this._keys.set(pkey, entry);
        entry.digest.catch(() => {});
        try {
            const h = await entry.handle;
            await entry.digest;
            return h;
        } catch (e) {
            if (this._keys.get(pkey) === entry) this._keys.delete(pkey);                // a key that failed to parse is not cached
            throw e;
        }
    }
    /* No counterpart in the reference (snarkjs: `zkey verify`): the audit of a proving key on the GPU -- every point of the five sections
     * and the five fixed points is a reduced, on-curve (B2: order-r) point, and beta1 ~ beta2, delta1 ~ delta2, B1 ~ B2 hold the same
     * discrete logs (include/wsnark.h: wsnark_pkey_check).  pkey: proving_key.bin bytes, or the path of a key file (either format).
     * opts.points / opts.relations: false leaves that half out; opts.seed: 32 bytes for the random combination of B1 ~ B2 -- by default
     * drawn from the OS, which is what makes that check sound (a seed the key's maker could know proves nothing).  Resolves to the
     * report object (keyReport above); a bad key is a result ({ok: false}), not a rejection.  Single GPU only: an object built with
     * {devices} audits with a one-GPU object first.  The audit cannot see a permutation applied to B1 and B2 alike, nor whether the
     * points belong to the circuit. */
    async checkKey(pkey, opts) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (this._group) throw new Error("wsnark: checkKey runs on a single GPU (build a Bn128 without {devices} for the audit)");
        const flags = (!opts || opts.points !== false ? 1 : 0) | (!opts || opts.relations !== false ? 2 : 0);
        if (!flags) throw new TypeError("checkKey: nothing to check");
        if (typeof pkey !== "string") asBytes(pkey);
        return keyReport(await addon.checkKey(pkey, flags, opts && opts.seed ? opts.seed : null));
    }
    /* No counterpart in the reference (snarkjs: `zkey contribute`): one phase-2 contribution -- the same key under delta * d, with
     * C and hExps scaled by 1/d on the GPU (include/wsnark.h: wsnark_pkey_contribute).  key: proving_key.bin bytes, or the path of a key
     * file (either format) together with opts.outPath, the new file.  opts.entropy: 32 bytes plain LE used as d (tests); by default the
     * library draws d from the OS, never returns it and wipes it.  Resolves to {key: the new key's ArrayBuffer, or outPath; report}; a bad
     * input point is a result ({key: null, report: {ok: false, ...}}), not a rejection. */
    async contributeKey(key, opts) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (this._group) throw new Error("wsnark: contributeKey runs on a single GPU (build a Bn128 without {devices})");
        const isPath = typeof key === "string";
        if (!isPath) asBytes(key);
        if (isPath !== !!(opts && opts.outPath)) throw new TypeError("contributeKey: outPath goes with a key file path");
        const ab = await addon.contributeKey(key, isPath ? opts.outPath : null, opts && opts.entropy ? opts.entropy : null);
        const report = deltaReport(ab);
        return { key: !report.ok ? null : isPath ? opts.outPath : ab.slice(104), report };
    }
    /* No counterpart in the reference: the transform over GROUP elements (include/wsnark.h: wsnark_g{1,2}_ntt) -- fft(odd = 0) / ifft
     * applied to the points' discrete logarithms, natural order in and out.  group: 1 (64-byte affine Montgomery points) or 2 (128);
     * a power-of-two number of points up to 2^24; a result at infinity is zero bytes.  Resolves to a fresh ArrayBuffer. */
    groupNtt(group, points, inverse) {
        if (!this._live) return Promise.reject(new Error("wsnark: this Bn128 object has been terminated"));
        if (this._group) return Promise.reject(new Error("wsnark: groupNtt runs on a single GPU (build a Bn128 without {devices})"));
        asBytes(points);
        return addon.groupNtt(group, points, !!inverse);
    }
    /* No counterpart in the reference (snarkjs: `zkey new`): the first key of a ceremony, the key of a circuit under delta = gamma = 1
     * from a powers-of-tau transcript (include/wsnark.h: wsnark_pkey_setup_pkey) -- the key contributeKey() is then applied to.
     * powers: {domain, tauG1 (2 x domain points), tauG2, alphaTauG1, betaTauG1 (domain points each), betaG2 (128 bytes)}; circuit:
     * {nVars, nPublic, domain, polsA, polsB, polsC}: a key's two record streams and the C matrix's.  Resolves to {key: proving_key.bin
     * as an ArrayBuffer, ic: the nPublic + 1 IC points of the verification key (gamma2 and delta2 are the G2 generator), report}; an
     * unreduced or off-curve power is a result ({key: null, ic: null, report: {ok: false, ...}}), not a rejection. */
    async newKey(powers, circuit) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (this._group) throw new Error("wsnark: newKey runs on a single GPU (build a Bn128 without {devices})");
        if (powers.domain !== circuit.domain) throw new TypeError("newKey: the powers and the circuit name different domains");
        const bufs = [powers.tauG1, powers.tauG2, powers.alphaTauG1, powers.betaTauG1, powers.betaG2, circuit.polsA, circuit.polsB, circuit.polsC];
        bufs.forEach(asBytes);
        const ab = await addon.newKey(circuit.nVars, circuit.nPublic, circuit.domain, bufs);
        const report = setupReport(ab);
        const head = 192 + 64 * (circuit.nPublic + 1);
        return { key: report.ok ? ab.slice(head) : null, ic: report.ok ? ab.slice(192, head) : null, report };
    }
    /* No counterpart in the reference: scalars[i] * points[i], a scalar PER point (include/wsnark.h: wsnark_g{1,2}_mul_batch) -- the
     * third shape beside one base with many scalars and many bases with one scalar.  group: 1 (64-byte affine Montgomery points) or 2
     * (128); scalars: 32 bytes plain little-endian each, reduced mod r; x == 0 is infinity and is copied through; a result at infinity
     * is zero bytes.  Resolves to a fresh ArrayBuffer. */
    mulPoints(group, points, scalars) {
        if (!this._live) return Promise.reject(new Error("wsnark: this Bn128 object has been terminated"));
        if (this._group) return Promise.reject(new Error("wsnark: mulPoints runs on a single GPU (build a Bn128 without {devices})"));
        asBytes(points); asBytes(scalars);
        return addon.mulPoints(group, points, scalars);
    }
    /* No counterpart in the reference (snarkjs: `powersoftau contribute`): one phase-1 contribution -- the transcript of (tau, alpha,
     * beta) becomes the one of (t tau, a alpha, b beta) (include/wsnark.h: wsnark_powers_contribute).  powers: the object of newKey().
     * opts.tau, opts.alpha, opts.beta: 32 bytes plain little-endian, non-zero mod r -- for tests; a secret left out is drawn from the
     * OS inside the library, which never returns it and wipes it: the production case.  Resolves to {powers: the new transcript
     * (ArrayBuffers), report}; a bad power or one at infinity is a result ({powers: null, report: {ok: false, ...}}). */
    async contributePowers(powers, opts) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (this._group) throw new Error("wsnark: contributePowers runs on a single GPU (build a Bn128 without {devices})");
        const bufs = [powers.tauG1, powers.tauG2, powers.alphaTauG1, powers.betaTauG1, powers.betaG2];
        bufs.forEach(asBytes);
        const secrets = ["tau", "alpha", "beta"].map((k) => (opts && opts[k] ? opts[k] : null));
        const ab = await addon.contributePowers(powers.domain, bufs, secrets);
        const report = powersReport(ab, ["device", "host", null, "total"]);
        if (!report.ok) return { powers: null, report };
        const n = powers.domain, o = 192;
        return { powers: { domain: n, tauG1: ab.slice(o, o + 128 * n), tauG2: ab.slice(o + 128 * n, o + 256 * n), alphaTauG1: ab.slice(o + 256 * n, o + 320 * n),
                           betaTauG1: ab.slice(o + 320 * n, o + 384 * n), betaG2: ab.slice(o + 384 * n, o + 384 * n + 128) }, report };
    }
    /* No counterpart in the reference (snarkjs: `powersoftau verify`): the audit of a transcript (include/wsnark.h:
     * wsnark_powers_check) -- every power a reduced, on-curve point (tauG2: of order r), none at infinity, and the six pairing relations
     * that make the arrays the consecutive powers of ONE tau.  opts.points / opts.relations === false leave that half out; opts.seed: 32
     * bytes for the random combinations, by default from the OS (a seed the transcript's author could know proves nothing).  Resolves
     * to the report; a bad transcript is a result, not a rejection.  The audit cannot tell who contributed. */
    async checkPowers(powers, opts) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (this._group) throw new Error("wsnark: checkPowers runs on a single GPU (build a Bn128 without {devices})");
        const flags = ((opts && opts.points === false) ? 0 : 1) | ((opts && opts.relations === false) ? 0 : 2);
        if (!flags) throw new TypeError("checkPowers: nothing to check");
        const bufs = [powers.tauG1, powers.tauG2, powers.alphaTauG1, powers.betaTauG1, powers.betaG2];
        bufs.forEach(asBytes);
        return powersReport(await addon.checkPowers(powers.domain, bufs, flags, opts && opts.seed ? opts.seed : null), ["points", "relationSums", "pairings", "total"]);
    }
    /* What the next participant runs: is newKey exactly oldKey under another delta (include/wsnark.h: wsnark_pkey_delta_verify)?  Both
     * keys as bytes, or both as file paths.  opts.seed: 32 bytes for the two random combinations, by default from the OS (a seed the
     * contributor could know proves nothing); opts.check !== false audits the new key first (checkKey) and rejects with the audit's
     * message and .report if that fails -- the relation check itself looks at no single point.  Resolves to {checks: {unchanged,
     * "delta1~delta2", C, H, delta_changed: true holds / false violated / null not run}, checksRun, checksBad, ok, ms}. */
    async verifyContribution(oldKey, newKey, opts) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (this._group) throw new Error("wsnark: verifyContribution runs on a single GPU (build a Bn128 without {devices})");
        if ((typeof oldKey === "string") !== (typeof newKey === "string")) throw new TypeError("verifyContribution: both keys as bytes, or both as paths");
        if (typeof oldKey !== "string") { asBytes(oldKey); asBytes(newKey); }
        if (!opts || opts.check !== false) {
            const report = await this.checkKey(newKey);
            if (!report.ok) throw Object.assign(new Error("wsnark: proving key failed its audit: " + firstFinding(report)), { report });
        }
        return deltaVerdict(await addon.deltaVerify(oldKey, newKey, opts && opts.seed ? opts.seed : null));
    }
    /* No counterpart in the reference (snarkjs: `zkey verify <r1cs> <ptau> <zkey>`): is this the key of THIS circuit on THIS transcript
     * (include/wsnark.h: wsnark_pkey_circuit_check)?  Works on the first key and after any number of contributions, without toxic waste
     * and without a group transform.  powers, circuit: the objects of newKey(); key: proving_key.bin bytes, or the path of a key file;
     * opts.vk: the verification_key.json object -- with it the IC points and the key's fixed points are checked too; opts.seed: 32 bytes
     * for the random combinations, by default from the OS (a seed the key's author could know proves nothing).  Resolves to {checks:
     * {shape_and_streams, fixed_points, "delta1~delta2", A, B1, B2, C, H, vk_fixed_points, IC: true holds / false violated / null not
     * run}, checksRun, checksBad, ok, ms}; a wrong key is a result, not a rejection.  The check looks at no single point (checkKey and
     * checkPowers do), and cannot tell whether the circuit is the intended one nor who contributed. */
    async checkKeyCircuit(powers, circuit, key, opts) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (this._group) throw new Error("wsnark: checkKeyCircuit runs on a single GPU (build a Bn128 without {devices})");
        if (typeof key !== "string") asBytes(key);
        const bufs = [powers.tauG1, powers.tauG2, powers.alphaTauG1, powers.betaTauG1, powers.betaG2, circuit.polsA, circuit.polsB, circuit.polsC];
        bufs.forEach(asBytes);
        let vk = null;
        if (opts && opts.vk) {
            const k = opts.vk;
            if (!k.IC || k.IC.length < 1) throw new Error("verification key has no IC point");
            const g1 = (p) => [p[0], p[1]], g2 = (p) => [p[0][0], p[0][1], p[1][0], p[1][1]];
            vk = le32cat([].concat(g1(k.vk_alfa_1), g2(k.vk_beta_2), g2(k.vk_gamma_2), g2(k.vk_delta_2), ...k.IC.map(g1)));
        }
        return circuitVerdict(await addon.checkKeyCircuit(key, circuit.nVars, circuit.nPublic, circuit.domain, bufs, vk, opts && opts.seed ? opts.seed : null));
    }
    /* No counterpart in the reference (snarkjs: `wtns check <r1cs> <wtns>`): which constraints does a witness break (include/wsnark.h:
     * wsnark_witness_check)?  The prover cannot tell -- a key holds no C matrix -- and a proof of a bad witness is simply rejected by
     * every verifier.  circuit: the object of newKey() ({nVars, nPublic, domain, polsA, polsB, polsC}); witness: nVars x 32 bytes.
     * Resolves to {rows, bad, firstBad, listed, unreduced, firstUnreduced, oneOk, ok, ms, badRows, badValues}: the smallest
     * min(bad, opts.maxRows = 16) bad rows and [a, b, c] of each as BigInts.  A bad witness is a result, not a rejection. */
    async checkWitness(circuit, witness, opts) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (this._group) throw new Error("wsnark: checkWitness runs on a single GPU (build a Bn128 without {devices})");
        const bufs = [circuit.polsA, circuit.polsB, circuit.polsC];
        bufs.forEach(asBytes);
        asBytes(witness);
        const cap = maxRowsOf(opts);
        return witnessReport(await addon.checkWitness(circuit.nVars, circuit.nPublic, circuit.domain, bufs, witness, cap), cap);
    }
    /* The circuit's three matrices made RESIDENT once (wsnark_circuit_load): resolves to {checkWitness(witness, {maxRows}),
     * checkWitnesses(witnesses, {maxRows, report}), info(), free()}.  checkWitnesses checks many witnesses in ONE call
     * (wsnark_circuit_witness_check_batch): an array of witness buffers, or one buffer holding them back to back; it resolves to the
     * array of what checkWitness resolves to for each, without rows and ms, which go to opts.report with count, good, firstNotOk, chunk.  Checks on one loaded circuit may run side by side; free() hands the device memory back once those in flight are done
     * (the garbage collector does it otherwise).  Pass the object to groth16GenProof as opts.circuit to have every witness checked
     * before it is proved. */
    /* loadCircuit({rows, publicRows}): the same object from a circuit given ROW BY ROW (wsnark_circuit_load_rows: the CSR is built
     * directly, no transposition); rows as circuitFromRows takes them. */
    async loadCircuit(circuit) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (this._group) throw new Error("wsnark: loadCircuit runs on a single GPU (build a Bn128 without {devices})");
        let handle;
        if (circuit.rows) {
            handle = await addon.loadCircuitRows(...rowsArgs(circuit.rows, circuit.publicRows));
            const inf = addon.circuitInfo(handle);
            circuit = { nVars: inf.nVars, nPublic: inf.nPublic, domain: inf.domain };
        } else {
            const bufs = [circuit.polsA, circuit.polsB, circuit.polsC];
            bufs.forEach(asBytes);
            handle = await addon.loadCircuit(circuit.nVars, circuit.nPublic, circuit.domain, bufs);
        }
        let inflight = 0, freed = false;
        const release = () => { if (freed && inflight === 0) addon.circuitFree(handle); };
        return {
            async checkWitness(witness, opts) {
                if (freed) throw new Error("wsnark: this circuit has been freed");
                asBytes(witness);
                const cap = maxRowsOf(opts);
                inflight++;
                try { return witnessReport(await addon.circuitCheckWitness(handle, witness, cap), cap); } finally { inflight--; release(); }
            },
            async checkWitnesses(witnesses, opts) {
                if (freed) throw new Error("wsnark: this circuit has been freed");
                const { blob, count } = witnessBlob(witnesses, 32 * circuit.nVars);
                const cap = maxRowsOf(opts);
                let res = { verdicts: [], report: { count: 0, rows: circuit.domain, good: 0, firstNotOk: null, chunk: 0, ms: { matrices: 0, device: 0, total: 0 } } };
                if (count) {
                    inflight++;
                    try { res = witnessVerdicts(await addon.circuitCheckWitnesses(handle, blob, count, cap), count, cap); } finally { inflight--; release(); }
                }
                if (opts && opts.report && typeof opts.report === "object") Object.assign(opts.report, res.report);
                return res.verdicts;
            },
            info() {
                if (freed) throw new Error("wsnark: this circuit has been freed");
                return addon.circuitInfo(handle);
            },
            free() { freed = true; release(); },
        };
    }
    /* No counterpart in the reference: the circuit object of newKey(), checkKeyCircuit(), checkWitness() and loadCircuit() --
     * {nVars, nPublic, domain, polsA, polsB, polsC} -- from constraints given ROW BY ROW (include/wsnark.h: wsnark_circuit_from_rows).
     * rows: {nVars, nPublic, nConstraints, domain (optional), A, B, C}, each matrix {rowPtr, col, coef}: a BigUint64Array of
     * nConstraints + 1 entries, a Uint32Array of signal indices and 32 bytes per entry, plain little-endian, any 256-bit value.
     * opts.publicRows (default true): append the nPublic + 1 input-binding rows.  Every signal's records come out with ascending
     * row; nothing is merged or dropped.  The object also carries .report: {nnz, unreduced, zero, emptySignals, maxColumn, ms}. */
    async circuitFromRows(rows, opts) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (this._group) throw new Error("wsnark: circuitFromRows runs on a single GPU (build a Bn128 without {devices})");
        const ab = await addon.circuitFromRows(...rowsArgs(rows, opts ? opts.publicRows : undefined));
        const v = new DataView(ab);
        const lens = [0, 1, 2].map((k) => Number(v.getBigUint64(8 + 8 * k, true)));
        const triple = (off) => [0, 1, 2].map((k) => Number(v.getBigUint64(32 + off + 8 * k, true)));
        const report = { nnz: triple(0), unreduced: triple(24), zero: triple(48), emptySignals: triple(72), maxColumn: triple(96),
                         ms: { upload: v.getFloat64(152, true), kernels: v.getFloat64(160, true), download: v.getFloat64(168, true), total: v.getFloat64(176, true) } };
        let off = 184;
        const pols = lens.map((n) => { const b = Buffer.from(ab, off, n); off += n; return b; });
        return { nVars: rows.nVars, nPublic: rows.nPublic, domain: v.getUint32(0, true), polsA: pols[0], polsB: pols[1], polsC: pols[2], report };
    }
    /* No counterpart in the reference: snarkjs' .zkey in and out (include/wsnark.h: wsnark_zkey_*; a key of one GPU's 4 GiB at most).
     * zkeyInfo(zkey) -> {nVars, nPublic, domain, nCoeffs, records: [A, B], nContributions, pkeyLen, vkLen}, host work only.
     * importZkey(zkey bytes | path, {wtns}) -> {pkey: Buffer (proving_key.bin), vk: the verification key object, report}.  The
     * coefficient records become the key's column streams and the H section changes basis on the device; the other point sections
     * are copied and NOT audited (checkKey does that).  opts.wtns: .wtns (or witness.bin) bytes of a witness of the circuit -- a TRIAL
     * PROOF: it is proved with the new key and verified against the returned vk, and the call rejects if that fails, so that a file
     * written under another convention than this reader's fails here and not in production.
     * exportZkey(pkey bytes, vk) -> Buffer (.zkey): gamma2 and IC come from vk; section 10 holds no contributions and a zero circuit
     * hash, so provers take the file and `snarkjs zkey verify` does not. */
    zkeyInfo(zkey) {
        const v = new DataView(addon.zkeyInfo(typeof zkey === "string" ? require("fs").readFileSync(zkey) : zkey));
        return { nVars: v.getUint32(0, true), nPublic: v.getUint32(4, true), domain: v.getUint32(8, true), nCoeffs: v.getUint32(12, true),
                 records: [Number(v.getBigUint64(16, true)), Number(v.getBigUint64(24, true))], nContributions: v.getUint32(32, true),
                 pkeyLen: Number(v.getBigUint64(40, true)), vkLen: Number(v.getBigUint64(48, true)) };
    }
    async importZkey(zkey, opts) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (this._group) throw new Error("wsnark: importZkey runs on a single GPU (build a Bn128 without {devices})");
        if (typeof zkey === "string") zkey = require("fs").readFileSync(zkey);
        const ab = await addon.importZkey(zkey);
        const v = new DataView(ab);
        const keyLen = Number(v.getBigUint64(0, true)), vkLen = Number(v.getBigUint64(8, true));
        const report = zkeyReport(v, 16);
        const vkb = Buffer.from(ab, 152, vkLen), pkey = Buffer.from(ab, 152 + vkLen, keyLen);
        const vk = vkFromBytes(vkb), nPublic = vk.nPublic;
        if (opts && opts.wtns) {
            const wit = formats.isWtns(opts.wtns) ? formats.wtnsToWitness(opts.wtns) : Buffer.from(asBytes(opts.wtns));
            const proof = await this.groth16GenProof(wit, pkey, { trustCache: false });
            const pub = [];
            for (let i = 1; i <= nPublic; i++) { let x = 0n; for (let k = 31; k >= 0; k--) x = (x << 8n) | BigInt(wit[32 * i + k]); pub.push(x.toString()); }
            if (!(await this.groth16Verify(vk, pub, proof)))
                throw new Error("wsnark: importZkey: the trial proof of the given witness does not verify against the file's verification key -- " +
                                "the file's coefficients or H section follow another convention than this reader's, or the witness is not one of this circuit");
        }
        return { pkey, vk, report };
    }
    async exportZkey(pkey, vk) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (this._group) throw new Error("wsnark: exportZkey runs on a single GPU (build a Bn128 without {devices})");
        if (!vk || !vk.IC) throw new Error("wsnark: exportZkey needs the verification key (gamma2 and IC are not part of a proving key)");
        const g1 = (p) => [p[0], p[1]], g2 = (p) => [p[0][0], p[0][1], p[1][0], p[1][1]];
        const vkb = le32cat([].concat(g1(vk.vk_alfa_1), g2(vk.vk_beta_2), g2(vk.vk_gamma_2), g2(vk.vk_delta_2), ...vk.IC.map(g1)).map((x) => BigInt(x)));
        const ab = await addon.exportZkey(pkey, vkb, vk.IC.length - 1);
        const out = Buffer.from(ab, 152, Number(new DataView(ab).getBigUint64(0, true)));
        out.report = zkeyReport(new DataView(ab), 16);
        return out;
    }
    /* A key FILE -- the reference's proving_key.bin or the WSNARK64 container for keys beyond its 4 GiB (js/formats.js:
     * writeKeyContainer; 2^24 constraints = 7.8 GB, more than one Buffer holds).  The library maps the file and reads only what it makes
     * resident; with a group every device reads its own shard.  Handles are cached per path while the file's size and mtime stand. */
    async _loadKeyFile(path) {
        const fs = require("fs");
        const st = fs.statSync(path);
        const hit = this._files.get(path);
        if (hit && hit.size === st.size && hit.mtimeMs === st.mtimeMs) return hit.handle;
        const zkey = isZkey(path);
        if (zkey && this._group) throw new Error("wsnark: a .zkey is loaded on a single GPU (build a Bn128 without {devices}, or importZkey it first)");
        const entry = { size: st.size, mtimeMs: st.mtimeMs,
                        handle: zkey ? zkeyHandle(addon.loadKeyZkeyFile(path)) : this._group ? addon.groupLoadKeyFile(this._group, path) : addon.loadKeyFile(path) };
        this._files.set(path, entry);
        try { return await entry.handle; } catch (e) { if (this._files.get(path) === entry) this._files.delete(path); throw e; }
    }
    /* {nVars, nPublic, domainSize, fileBytes, format} of a key file, from its header (nothing is loaded) */
    keyFileInfo(path) { return addon.keyFileInfo(path); }
    /* forget the cached handle of a key object (its bytes were rewritten in place, or its HBM should go back) */
    invalidateKey(pkey) { return typeof pkey === "string" ? this._files.delete(pkey) : this._keys.delete(pkey); }
    /* {nVars, nPublic, domainSize, loadMs: {polsToCsr, pointsH2d, masksConvert, tableBuild, total}} of a key (bytes or handle) */
    async keyInfo(pkey) { const h = await this.loadKey(pkey); return this._group ? addon.groupKeyInfo(h) : addon.keyInfo(h); }
    /* loadKey() returns once the key's sections are resident: proofs may start at once and run on the plain sections while the rows
     * of the fixed-base tables are built behind them (about 0.2 s for a 2^20 key).  A caller that wants its first timed proof at the
     * steady-state rate awaits this first. */
    async waitTables(pkey) { const h = await this.loadKey(pkey); return (this._group ? addon.groupWaitTables(h) : addon.waitTables(h)).then(() => true); }
    /* an ArrayBuffer of `bytes` bytes in PINNED host memory: a witness written into it is DMA'd to the GPU in place, chunk by
     * chunk, instead of being copied through the library's staging ring first (no counterpart in the reference) */
    allocInput(bytes) { return addon.allocPinned(bytes); }
    /* pkey: proving_key.bin bytes, or a handle from loadKey().
     * opts.r / opts.s: optional 32-byte blinding values (the reference draws them from crypto.randomBytes)
     * opts.trustCache: see loadKey.  opts.timing: an object that receives {loadKey_ms, prove_ms, format_ms} of this call
     * opts.circuit: an object from loadCircuit() whose nVars, nPublic and domain are the key's (else the call rejects before anything
     * runs on the witness): the witness is checked first, and one that breaks a constraint rejects with an Error naming the first
     * bad constraint and its a, b, c (.report holds the whole report); no proof is computed.  Without it nothing changes. */
    async groth16GenProof(signals, pkey, opts) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        // a snarkjs .wtns is taken for its section 2, which is witness.bin (found by its magic: a witness.bin starts with the signal 1)
        if ((signals instanceof ArrayBuffer || ArrayBuffer.isView(signals)) && formats.isWtns(signals)) signals = formats.wtnsToWitness(signals);
        const t0 = process.hrtime.bigint();
        if (opts && opts.circuit) {
            const ci = opts.circuit.info(), ki = await this.keyInfo(pkey);
            if (ci.nVars !== ki.nVars || ci.nPublic !== ki.nPublic || ci.domain !== ki.domainSize)
                throw new Error(`wsnark: the circuit (nVars ${ci.nVars}, nPublic ${ci.nPublic}, domain ${ci.domain}) is not the key's (${ki.nVars}, ${ki.nPublic}, ${ki.domainSize})`);
            const report = await opts.circuit.checkWitness(signals, { maxRows: 1 });
            if (!report.ok) throw Object.assign(new Error("wsnark: the witness does not satisfy the circuit: " + witnessFinding(report)), { report });
        }
        // which entry point a handle goes to is fixed when the call STARTS: terminate() clears this._group while calls may still be
        // awaiting their key, and a group key must never reach the single-context prove()
        const proveFn = this._group ? addon.groupProve : addon.prove;
        const prove = (h) => proveFn(h, signals, opts && opts.r ? opts.r : null, opts && opts.s ? opts.s : null);
        const isBytes = pkey instanceof ArrayBuffer || ArrayBuffer.isView(pkey);      // (else: a handle, or the path of a key file)
        let t1, out;
        const hit = isBytes && !(opts && opts.trustCache === true) ? this._cached(pkey, asBytes(pkey)) : null;
        if (hit) {
            // key BYTES with a cached handle: prove on it at once, take the digest of all bytes beside the proof, and only return the
            // proof if those are the bytes the handle was loaded from (else: load what the caller holds now and prove again)
            this.fullDigests++;
            const h = await hit.handle;
            t1 = process.hrtime.bigint();
            const first = prove(h);
            first.catch(() => {});
            // The digest's eight threads read the key at the host's memory bandwidth; started together with the proof they compete with
            // the witness's staging copy (the first ~1 ms of the call) -- 0.15 ms per call on most boxes, 1.7 ms on one.  For keys large
            // enough for that to matter the digest starts a timer tick later: it still ends well before the proof does.
            const bytes = asBytes(pkey);
            const now = bytes.byteLength >= (64 << 20) ? new Promise((res) => setTimeout(res, 1)).then(() => digest(bytes)) : digest(bytes);
            now.catch(() => {});
            if ((await now) === (await hit.digest)) out = await first;
            else {
                await first.catch(() => {});
                if (this._keys.get(pkey) === hit) this._keys.delete(pkey);
                out = await prove(await this.loadKey(pkey, opts));
            }
        } else {
            const h = await this.loadKey(pkey, opts);
            t1 = process.hrtime.bigint();
            out = await prove(h);
        }
        const t2 = process.hrtime.bigint();
        this._pr = new Uint8Array(out.slice(384, 416));
        this._ps = new Uint8Array(out.slice(416, 448));
        const proof = proofFromBytes(out.slice(0, 384));
        if (opts && opts.timing) {
            const ms = (a, b) => Number(b - a) / 1e6;
            Object.assign(opts.timing, { loadKey_ms: ms(t0, t1), prove_ms: ms(t1, t2), format_ms: ms(t2, process.hrtime.bigint()) });
        }
        return proof;
    }
    /* Many witnesses of ONE key in one call (wsnark_groth16_prove_batch; no reference counterpart).  witnesses: an array of witness
     * buffers (each at least nVars x 32 bytes), or ONE buffer holding them back to back, nVars x 32 bytes each; pkey: key bytes, a
     * handle or a key file, as groth16GenProof takes them (a whole key on one device: not with {devices}).  opts.r / opts.s: one
     * 32-byte value per proof (an array, or the values back to back); absent: drawn per proof.  Resolves to the array of proofs,
     * proof i being what groth16GenProof(witnesses[i], pkey, {r: r[i], s: s[i]}) resolves to.  opts.blinding (an array) receives
     * {r, s} of every proof as used, opts.report (an object) the call's report: count, batched (0: the call looped the single
     * prover), chunk, windowBits, ms.
     * opts.circuit: an object from loadCircuit() whose nVars, nPublic and domain are the key's (else the call rejects before anything
     * runs).  All witnesses are checked against it in one call (checkWitnesses, maxRows 1); those that are ok are proved in one call,
     * each with its own r[i], s[i], to the proof the call without opts.circuit gives for it; a bad witness gives null in the array of
     * proofs and in opts.blinding -- no proof is computed and no blinding drawn for it.  The resolved array then carries the
     * verdicts of all witnesses as its property `verdicts` (and opts.report.verdicts), the report being the good witnesses' call's. */
    async groth16GenProofBatch(witnesses, pkey, opts) {
        if (!this._live) throw new Error("wsnark: this Bn128 object has been terminated");
        if (this._group) throw new Error("wsnark: groth16GenProofBatch needs a whole key on one device (not buildBn128({devices}))");
        const h = await this.loadKey(pkey, opts);
        const ki = addon.keyInfo(h);
        const stride = 32 * ki.nVars;
        if (opts && opts.circuit) {
            const ci = opts.circuit.info();
            if (ci.nVars !== ki.nVars || ci.nPublic !== ki.nPublic || ci.domain !== ki.domainSize)
                throw new Error(`wsnark: the circuit (nVars ${ci.nVars}, nPublic ${ci.nPublic}, domain ${ci.domain}) is not the key's (${ki.nVars}, ${ki.nPublic}, ${ki.domainSize})`);
        }
        const { blob, count } = witnessBlob(witnesses, stride);
        const values = (v, name) => {
            if (v === undefined || v === null) return null;
            const parts = Array.isArray(v) ? v.map(asBytes) : [asBytes(v)];
            const out = new Uint8Array(32 * count);
            let off = 0;
            for (const p of parts) {
                if ((Array.isArray(v) && p.byteLength !== 32) || off + p.byteLength > out.byteLength) throw new Error("wsnark: " + name + ": one 32-byte value per proof");
                out.set(p, off);
                off += p.byteLength;
            }
            if (off !== out.byteLength) throw new Error("wsnark: " + name + ": one 32-byte value per proof");
            return out;
        };
        const r = values(opts && opts.r, "r"), s = values(opts && opts.s, "s");
        if (count === 0) return [];
        // which witnesses are proved: all of them, or those the circuit passes
        let which = null, verdicts = null;
        if (opts && opts.circuit) {
            verdicts = await opts.circuit.checkWitnesses(blob, { maxRows: 1 });
            which = [];
            verdicts.forEach((v, i) => { if (v.ok) which.push(i); });
        }
        const pick = (buf, width) => {
            if (!buf || !which || which.length === count) return buf;
            const out = new Uint8Array(width * which.length);
            which.forEach((i, k) => out.set(buf.subarray(width * i, width * i + width), width * k));
            return out;
        };
        const n = which ? which.length : count;
        const out = n ? await addon.proveBatch(h, pick(blob, stride), n, pick(r, 32), pick(s, 32)) : new ArrayBuffer(64);
        const at = (k) => (which ? which[k] : k);
        if (opts && Array.isArray(opts.blinding)) {
            opts.blinding.length = 0;
            for (let i = 0; i < count; i++) opts.blinding.push(null);
            for (let k = 0; k < n; k++) {
                const o = 384 * n + 64 * k;
                opts.blinding[at(k)] = { r: new Uint8Array(out.slice(o, o + 32)), s: new Uint8Array(out.slice(o + 32, o + 64)) };
            }
        }
        if (opts && opts.report && typeof opts.report === "object") {
            const dv = new DataView(out, 448 * n, 64);
            const ms = [0, 1, 2, 3, 4].map((k) => dv.getFloat64(24 + 8 * k, true));
            Object.assign(opts.report, { count: Number(dv.getBigUint64(0, true)), batched: Number(dv.getBigUint64(8, true)), chunk: dv.getUint32(16, true),
                windowBits: dv.getUint32(20, true), ms: { upload: ms[0], calcH: ms[1], sums: ms[2], assembly: ms[3], total: ms[4] } });
            if (verdicts) opts.report.verdicts = verdicts;
        }
        const proofs = new Array(count).fill(null);
        for (let k = 0; k < n; k++) proofs[at(k)] = proofFromBytes(out.slice(384 * k, 384 * k + 384));
        if (verdicts) proofs.verdicts = verdicts;
        return proofs;
    }
    /* src/bn128.js:722-791: verificationKey = snarkjs "groth" verification_key.json object, input = public signals
     * (one value is wrapped like the reference does), proof = {pi_a, pi_b, pi_c}.  Native host arithmetic, no GPU. */
    async groth16Verify(verificationKey, input, proof) {
        if (input === undefined || input === null) input = [];
        else if (!Array.isArray(input)) input = [input];
        const vals = input.map((x) => BigInt(x));
        if (vals.some((v) => v < 0n || v >= (1n << 256n))) return false;
        const IC = verificationKey.IC;
        if (!IC || IC.length < vals.length + 1) throw new Error("verification key has fewer IC points than inputs + 1");
        const g1 = (p) => [p[0], p[1]], g2 = (p) => [p[0][0], p[0][1], p[1][0], p[1][1]];
        const vk = le32cat([].concat(g1(verificationKey.vk_alfa_1), g2(verificationKey.vk_beta_2), g2(verificationKey.vk_gamma_2),
            g2(verificationKey.vk_delta_2), ...IC.slice(0, vals.length + 1).map(g1)));
        const pf = le32cat([].concat(proof.pi_a, proof.pi_b[0], proof.pi_b[1], proof.pi_b[2], proof.pi_c));
        return addon.verify(vk, le32cat(vals), pf);
    }
    /* Many proofs against ONE verification key, on the GPU (wsnark_groth16_verify_batch; no reference counterpart): inputs = one array
     * of public signals per proof, all of one length; proofs = [{pi_a, pi_b, pi_c}, ...].  Resolves to boolean[], proof by proof
     * what groth16Verify says (a proof with an unreduced coordinate, which the single call rejects with an error, reads false). */
    async groth16VerifyBatch(verificationKey, inputs, proofs) {
        if (!Array.isArray(inputs) || !Array.isArray(proofs) || inputs.length !== proofs.length) throw new TypeError("expected one input array per proof");
        if (proofs.length === 0) return [];
        const rows = inputs.map((x) => (x === undefined || x === null ? [] : Array.isArray(x) ? x : [x]).map((v) => BigInt(v)));
        const nIn = rows[0].length;
        if (rows.some((r) => r.length !== nIn)) throw new TypeError("all proofs of a batch share the key: every input array must have " + nIn + " entries");
        const IC = verificationKey.IC;
        if (!IC || IC.length < nIn + 1) throw new Error("verification key has fewer IC points than inputs + 1");
        const g1 = (p) => [p[0], p[1]], g2 = (p) => [p[0][0], p[0][1], p[1][0], p[1][1]];
        const vk = le32cat([].concat(g1(verificationKey.vk_alfa_1), g2(verificationKey.vk_beta_2), g2(verificationKey.vk_gamma_2),
            g2(verificationKey.vk_delta_2), ...IC.slice(0, nIn + 1).map(g1)));
        // an input outside [0, 2^256) makes that proof false without reaching the library, as in groth16Verify
        const keep = rows.map((r, i) => i).filter((i) => !rows[i].some((v) => v < 0n || v >= (1n << 256n)));
        const out = new Array(proofs.length).fill(false);
        if (keep.length === 0) return out;
        const pf = le32cat([].concat(...keep.map((i) => { const p = proofs[i]; return [].concat(p.pi_a, p.pi_b[0], p.pi_b[1], p.pi_b[2], p.pi_c); })));
        const st = new Uint8Array(await addon.verifyBatch(vk, le32cat([].concat(...keep.map((i) => rows[i]))), pf, nIn));
        keep.forEach((i, k) => { out[i] = st[k] === 1; });
        return out;
    }
    /* Compressed points and 128-byte proofs (csrc/pointcodec.hip; include/wsnark.h has both encodings byte by byte).  encoding: "le"
     * (ark-serialize's compressed mode) or "be" (gnark-crypto's marshal).  Each resolves to {data: ArrayBuffer, status: number[]}:
     * compressPoints(g, points)        affine Montgomery points (64 g bytes) -> 32 g bytes each; status 0 ok, 1 a coordinate >= q
     * decompressPoints(g, data)        -> points; status 0 ok, 1 malformed, 2 no point, 3 outside the subgroup (g = 2 with subgroup)
     * compressProofs(proofs)           [{pi_a, pi_b, pi_c}] -> 128 bytes each (A | B | C); status 1 written, 2 malformed
     * decompressProofs(data)           -> {proofs: [{pi_a, pi_b, pi_c} | null], status}: 1 written, 2 malformed, 0 no point / infinity */
    async compressPoints(g, points, encoding) { return codecSplit(await addon.codecPoints(g, true, points, encodingId(encoding), 0), 32 * g); }
    async decompressPoints(g, data, encoding, subgroup) {
        return codecSplit(await addon.codecPoints(g, false, data, encodingId(encoding), subgroup ? 1 : 0), 64 * g);
    }
    async compressProofs(proofs, encoding) {
        if (!Array.isArray(proofs)) throw new TypeError("expected an array of proofs");
        if (proofs.length === 0) return { data: new ArrayBuffer(0), status: [] };
        const pf = le32cat([].concat(...proofs.map((p) => [].concat(p.pi_a, p.pi_b[0], p.pi_b[1], p.pi_b[2], p.pi_c))));
        return codecSplit(await addon.codecProofs(true, pf, encodingId(encoding)), 128);
    }
    async decompressProofs(data, encoding) {
        if (data.byteLength === 0) return { proofs: [], status: [] };
        const r = codecSplit(await addon.codecProofs(false, data, encodingId(encoding)), 384);
        const w = new Uint8Array(r.data);
        const num = (i, k) => { let v = 0n; for (let b = 31; b >= 0; b--) v = (v << 8n) | BigInt(w[384 * i + 32 * k + b]); return v.toString(); };
        const proofs = r.status.map((st, i) => st !== 1 ? null : {
            pi_a: [num(i, 0), num(i, 1), num(i, 2)], pi_b: [[num(i, 3), num(i, 4)], [num(i, 5), num(i, 6)], [num(i, 7), num(i, 8)]],
            pi_c: [num(i, 9), num(i, 10), num(i, 11)] });
        return { proofs, status: r.status };
    }
    /* groth16VerifyBatch on 128-byte proofs (one buffer of count x 128 bytes): decompressed on the GPU and verified there.  Resolves to
     * boolean[], or with returnStatus to the raw statuses (1 valid, 0 invalid, 2 malformed). */
    async groth16VerifyBatchCompressed(verificationKey, inputs, proofBytes, encoding, returnStatus) {
        const enc = encodingId(encoding), count = proofBytes.byteLength / 128;
        if (!Array.isArray(inputs) || !Number.isInteger(count) || inputs.length !== count) throw new TypeError("expected one input array per 128-byte proof");
        if (count === 0) return [];
        const rows = inputs.map((x) => (x === undefined || x === null ? [] : Array.isArray(x) ? x : [x]).map((v) => BigInt(v)));
        const nIn = rows[0].length;
        if (rows.some((r) => r.length !== nIn)) throw new TypeError("all proofs of a batch share the key: every input array must have " + nIn + " entries");
        const IC = verificationKey.IC;
        if (!IC || IC.length < nIn + 1) throw new Error("verification key has fewer IC points than inputs + 1");
        const g1 = (p) => [p[0], p[1]], g2 = (p) => [p[0][0], p[0][1], p[1][0], p[1][1]];
        const vk = le32cat([].concat(g1(verificationKey.vk_alfa_1), g2(verificationKey.vk_beta_2), g2(verificationKey.vk_gamma_2),
            g2(verificationKey.vk_delta_2), ...IC.slice(0, nIn + 1).map(g1)));
        const keep = rows.map((r, i) => i).filter((i) => !rows[i].some((v) => v < 0n || v >= (1n << 256n)));
        const status = new Array(count).fill(0);
        if (keep.length) {
            const all = new Uint8Array(proofBytes.buffer || proofBytes, proofBytes.byteOffset || 0, proofBytes.byteLength), pf = new Uint8Array(128 * keep.length);
            keep.forEach((i, k) => pf.set(all.subarray(128 * i, 128 * i + 128), 128 * k));
            const st = new Uint8Array(await addon.verifyBatchCompressed(vk, le32cat([].concat(...keep.map((i) => rows[i]))), pf, nIn, enc));
            keep.forEach((i, k) => { status[i] = st[k]; });
        }
        return returnStatus ? status : status.map((v) => v === 1);
    }
    /* src/bn128.js:562-566.  The GPU context is process-wide (one per addon): it is shut down when the LAST live Bn128
     * object terminates, so one object's terminate() does not pull the device out from under another's proofs. */
    terminate() {
        if (!this._live) return;
        this._live = false;
        this._files.clear();
        if (this._group) { addon.groupFree(this._group); this._group = null; }     // (a group's contexts belong to this object alone)
        if (--liveInstances === 0) addon.shutdown();
    }
}
let liveInstances = 0;
function encodingId(name) {         // WSNARK_ENC_LE, WSNARK_ENC_BE
    if (name === "le") return 1;
    if (name === "be") return 2;
    throw new TypeError('encoding must be "le" or "be"');
}
function codecSplit(buf, recordBytes) {      // the addon's `records | one status byte each`
    const n = buf.byteLength / (recordBytes + 1);
    return { data: buf.slice(0, n * recordBytes), status: Array.from(new Uint8Array(buf, n * recordBytes, n)) };
}
function le32cat(list) {            // decimal strings / BigInts -> concatenated 32-byte little-endian integers
    const out = new Uint8Array(32 * list.length);
    list.forEach((x, k) => { let v = BigInt(x); for (let i = 0; i < 32; i++) { out[32 * k + i] = Number(v & 0xffn); v >>= 8n; } });
    return out;
}

let singleton = null;
/* buildBn128([device]) | buildBn128({devices: [...]}).  The addon binds the in-tree libwsnark.so and nothing else: there is no
 * library-path option and no CPU path in the product (the test-suite's emulator host is its own build of the addon under tests/). */
async function buildBn128(device, opts) {
    if (device !== null && typeof device === "object") { opts = device; device = undefined; }      // buildBn128({devices: [...]})
    const devices = opts && opts.devices ? Array.from(opts.devices, (d) => d | 0) : null;
    if (devices && devices.length === 0) throw new TypeError("devices: expected at least one device ordinal");
    // (the default context serves calcH / fft and the pinned input buffers; with a group it sits on the group's first device)
    const info = addon.init(devices ? devices[0] : (device === undefined || device === null ? -1 : device));
    liveInstances++;
    if (!devices) return new Bn128(info);
    try {
        return new Bn128(info + " x" + devices.length + " (devices " + devices.join(", ") + ")", addon.groupCreate(devices), devices);
    } catch (e) {
        if (--liveInstances === 0) addon.shutdown();
        throw e;
    }
}
/* The module-level calls share one Bn128 object that is never terminated on its own, exactly like the reference's
 * (main_bn128.js:26-39 builds its singleton and leaves the workers running; src/bn128.js:562-566 needs an explicit call): a
 * process that only uses these forms ends with terminate() below (the reference has no such export), or process.exit(). */
function terminate() {
    if (singleton) { singleton.terminate(); singleton = null; }
}
function zkeyReport(v, o) {      // wsnark_zkey_report_t
    const pair = (at) => [Number(v.getBigUint64(o + at, true)), Number(v.getBigUint64(o + at + 8, true))];
    const bad = Number(v.getBigUint64(o + 72, true));
    return { records: pair(0), unreduced: pair(16), zero: pair(32), sorted: v.getUint32(o + 48, true) !== 0,
             H: { points: Number(v.getBigUint64(o + 56, true)), infinity: Number(v.getBigUint64(o + 64, true)), bad,
                  firstBad: bad ? Number(v.getBigUint64(o + 80, true)) : null },
             ms: { upload: v.getFloat64(o + 96, true), coefficients: v.getFloat64(o + 104, true), hBasis: v.getFloat64(o + 112, true),
                   download: v.getFloat64(o + 120, true), total: v.getFloat64(o + 128, true) } };
}

function groth16GenProof(witness, provingKey, cb) {   // main_bn128.js:26-39
    const p = (async () => {
        if (!singleton) singleton = await buildBn128();
        return singleton.groth16GenProof(witness, provingKey);
    })();
    if (cb) { p.then((proof) => cb(null, proof), (err) => cb(err)); return undefined; }
    return p;
}

function groth16GenProofBatch(witnesses, provingKey, opts, cb) {
    if (typeof opts === "function") { cb = opts; opts = undefined; }
    const p = (async () => {
        if (!singleton) singleton = await buildBn128();
        return singleton.groth16GenProofBatch(witnesses, provingKey, opts);
    })();
    if (cb) { p.then((proofs) => cb(null, proofs), (err) => cb(err)); return undefined; }
    return p;
}

function groth16Verify(verificationKey, input, proof, cb) {   // main_bn128.js:41-55
    const p = (async () => {
        if (!singleton) singleton = await buildBn128();
        return singleton.groth16Verify(verificationKey, input, proof);
    })();
    if (cb) { p.then((ok) => cb(null, ok), (err) => cb(err)); return undefined; }
    return p;
}

function groth16VerifyBatch(verificationKey, inputs, proofs, cb) {
    const p = (async () => {
        if (!singleton) singleton = await buildBn128();
        return singleton.groth16VerifyBatch(verificationKey, inputs, proofs);
    })();
    if (cb) { p.then((ok) => cb(null, ok), (err) => cb(err)); return undefined; }
    return p;
}

const formats = require("./formats.js");     // snarkjs JSON -> proving_key.bin / witness.bin (reference tools/build*.js)
module.exports = { buildBn128, groth16GenProof, groth16GenProofBatch, genZKSnarkProof: groth16GenProof, groth16Verify, groth16VerifyBatch, terminate, Bn128, proofFromBytes,
    pkeyJsonToBin: formats.pkeyJsonToBin, witnessJsonToBin: formats.witnessJsonToBin,
    pkeyBinSections: formats.pkeyBinSections, writeKeyContainer: formats.writeKeyContainer, pkeyBinToContainer: formats.pkeyBinToContainer,
    wtnsToWitness: formats.wtnsToWitness, witnessToWtns: formats.witnessToWtns };
