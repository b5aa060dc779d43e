// pkeycircuit.hip -- is this proving key the key of THIS circuit on THIS powers-of-tau transcript?  (snarkjs: `zkey verify <r1cs> <ptau>
// <zkey>`; no counterpart in the reference.)  The last link of the ceremony chain: wsnark_powers_check audits a transcript,
// wsnark_pkey_setup builds the first key on it, wsnark_pkey_contribute / _delta_verify move its delta, wsnark_pkey_check audits the
// key's points -- and none of them ties the points to the circuit's polynomials.  Rebuilding the key and comparing bytes does, but
// costs the four group transforms and stops working after the first contribution (C and hExps are then scaled by an unknown 1/d).
//
// No toxic waste is needed.  With random weights rho_j per signal, u = (A-matrix rows) . rho and L_i the Lagrange basis of the domain:
//     sum_j rho_j A_j = sum_i u_i L_i(tau) G = sum_k c_k tau^k G,      c = iNTT(u)
// and c is a transform over the FIELD.  The same with B against tau_g1 and tau_g2; split by public and private signal (p = the sum
// over columns j <= nPublic, v = over j > nPublic, u = p + v) the private halves give C under delta, the public ones IC under gamma:
//     K_x = sum_k [c(x_A)_k beta_tau_g1[k] + c(x_B)_k alpha_tau_g1[k] + c(x_C)_k tau_g1[k]],   x in {p, v}
//     e(sum_{j > np} rho_j C_j, delta2) = e(K_v, G2)        e(sum_{j <= np} rho_j IC_j, gamma2) = e(K_p, G2)
// and hExps_i = tau_g1[n + i] - tau_g1[i] under delta.  Three sparse products (one kernel), six field transforms, the ordinary MSMs
// chunk by chunk and a handful of host pairings.
//
//   lc_split_kernel: one lane per (row, matrix); the row's CSR range is walked ONCE and leaves both halves.  The arithmetic is
//     lc_row_dot's (internal.h): the radix-2^29 field, two consecutive terms of one half through the fused double product, a single
//     product otherwise, one closing product by CIN per half.  Both sums leave canonical: bit for bit what two masked lc_row_dot
//     calls give, whatever order the transposition left the row's terms in.
//   streaming: key sections and transcript arrays go through the staging ring in chunks of PKCIRCUIT_CHUNK points (default 2^18);
//     the three CSR matrices and the six domain-length vectors stay resident for the call, the nVars weights only for the kernel.
//     c(u) = c(p) + c(v) is formed per chunk (fr_add_kernel), so A, B1 and B2 cost one MSM each per chunk; K_v and K_p are one MSM of
//     3 x chunk terms each over the three G1 arrays staged side by side.
//   The check tests no single point (wsnark_pkey_check and wsnark_powers_check do): unreduced or off-curve bytes only make the sums
//   meaningless.  It cannot tell whether the circuit is the intended one, nor who contributed.
#include <string.h>

#include "keybytes.h"

namespace wsnark {

using namespace hostpair;

// ---- device ----
struct SplitTriple { const uint32_t* row_ptr[3]; const uint32_t* col[3]; const Fe* coef[3]; Fe* pub[3]; Fe* prv[3]; };

// pub[m][r] = sum over the row's terms with column <= n_public of coef * w[col], prv[m][r] = the same over the columns > n_public
// (pol_constructLC restricted to the public resp. private signals), matrix m = blockIdx.y.  coef is c R^2 (pols_to_csr), w plain -- any
// 256-bit value --, the sums are Montgomery and canonical.  A wavefront runs as long as its longest row, as in lc_spmv2_kernel.
__global__ __launch_bounds__(256) void lc_split_kernel(SplitTriple M, const Fe* __restrict__ w, uint32_t n_public, uint32_t n_rows) {
    typedef Fr29 F;
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const uint32_t* __restrict__ col = M.col[blockIdx.y];
    const Fe* __restrict__ coef = M.coef[blockIdx.y];
    uint32_t k = M.row_ptr[blockIdx.y][r];
    const uint32_t e = M.row_ptr[blockIdx.y][r + 1];
    F29 acc_pub = F::zero(), acc_prv = F::zero();
    while (k < e) {
        const uint32_t c0 = col[k];
        const bool prv = c0 > n_public;
        F29 t;
        uint32_t c1 = 0;
        if (k + 1 < e) c1 = col[k + 1];
        if (k + 1 < e && (c1 > n_public) == prv) {      // the next term belongs to the same half: one reduction for the two
            t = F::mul2add_inl(F::unpack(coef[k]), F::unpack(w[c0]), F::unpack(coef[k + 1]), F::unpack(w[c1]));
            k += 2;
        } else {
            t = F::mul_inl(F::unpack(coef[k]), F::unpack(w[c0]));
            k += 1;
        }
        if (prv) acc_prv = F::add(acc_prv, t);
        else acc_pub = F::add(acc_pub, t);
    }
    const F29 cin = F::from_words(Fr29Params::CIN0, Fr29Params::CIN1, Fr29Params::CIN2, Fr29Params::CIN3);
    M.pub[blockIdx.y][r] = F::pack(F::canonical(F::mul_inl(acc_pub, cin)));
    M.prv[blockIdx.y][r] = F::pack(F::canonical(F::mul_inl(acc_prv, cin)));
}

// out[i] = a[i] + b[i] mod r: a chunk of c(u) = c(p) + c(v) (the transform is linear), so that the sums over A, B1 and B2 are one MSM
// each and no seventh domain-length vector exists
__global__ __launch_bounds__(256) void fr_add_kernel(const Fe* __restrict__ a, const Fe* __restrict__ b, Fe* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = Fr::add(a[i], b[i]);
}

// ---- shared with witcheck.hip (keybytes.h) ----
// what setup_prepare (pkeysetup.hip) rejects of a circuit, with its codes
int circuit_shape_check(const wsnark_circuit_t* K) {
    if (!K || !K->polsA || !K->polsB || !K->polsC) return WS_ERR_ARG;
    if (int rc = key_vars_check(K->n_vars, K->n_public)) return rc;
    const uint64_t n = K->domain;
    if (n < 2 || (n & (n - 1)) || n > ((uint64_t)1 << 24)) { set_last_error("circuit check: domain must be a power of two in [2, 2^24]"); return WS_ERR_SIZE; }
    return WS_OK;
}

// the three record streams as row-major CSR (rows: constraints, columns: signals), with the loaders' conditions and codes
int circuit_to_csr(const wsnark_circuit_t* K, CsrMatrix M[3], hipStream_t s) {
    const uint8_t* pols[3] = {(const uint8_t*)K->polsA, (const uint8_t*)K->polsB, (const uint8_t*)K->polsC};
    const uint64_t lens[3] = {K->polsA_len, K->polsB_len, K->polsC_len};
    for (int m = 0; m < 3; m++) {
        size_t used = 0;
        if (int rc = pols_to_csr(pols[m], (size_t)lens[m], K->n_vars, K->domain, &M[m], &used, s)) return rc;
    }
    return WS_OK;
}

namespace {
// what setup_prepare (pkeysetup.hip) rejects of a transcript, with its codes
int powers_shape_check(const wsnark_powers_t* P, uint64_t n) {
    if (!P || !P->tau_g1 || !P->tau_g2 || !P->alpha_tau_g1 || !P->beta_tau_g1 || !P->beta_g2) return WS_ERR_ARG;
    if (P->domain != n) { set_last_error("circuit check: the powers and the circuit name different domains"); return WS_ERR_SIZE; }
    if (P->tau_g1_len < 2 * n * 64 || P->tau_g2_len < n * 128 || P->alpha_tau_g1_len < n * 64 || P->beta_tau_g1_len < n * 64) {
        set_last_error("circuit check: an array of powers is shorter than the domain implies (tau_g1: 2n, the others: n)");
        return WS_ERR_FORMAT;
    }
    const G1A g1 = gen1();
    const G2A g2 = gen2();
    if (memcmp(P->tau_g1, &g1.x, 64) != 0 || memcmp(P->tau_g2, &g2.x, 128) != 0) {
        set_last_error("circuit check: tau_g1[0] / tau_g2[0] is not the generator");
        return WS_ERR_FORMAT;
    }
    return WS_OK;
}

// d_pub, d_prv: 3 x domain elements each, order A, B, C
int lc_split_dev(Context* X, const CsrMatrix M[3], const Fe* d_w, uint32_t n_public, uint32_t domain, Fe* d_pub, Fe* d_prv, hipStream_t s) {
    SplitTriple T;
    for (int m = 0; m < 3; m++) {
        T.row_ptr[m] = M[m].row_ptr.as<uint32_t>();
        T.col[m] = M[m].col.as<uint32_t>();
        T.coef[m] = M[m].coef.as<Fe>();
        T.pub[m] = d_pub + (size_t)m * domain;
        T.prv[m] = d_prv + (size_t)m * domain;
    }
    X->timer.begin("lc_split", s);
    hipLaunchKernelGGL(lc_split_kernel, dim3(ceil_div_u64(domain, 256), 3), dim3(256), 0, s, T, d_w, n_public, domain);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    return WS_OK;
}

bool same_point(const G1A& a, const G1A& b) { return a.inf == b.inf && (a.inf || (memcmp(&a.x, &b.x, 32) == 0 && memcmp(&a.y, &b.y, 32) == 0)); }
bool same_point(const G2A& a, const G2A& b) { return a.inf == b.inf && (a.inf || (memcmp(&a.x, &b.x, 64) == 0 && memcmp(&a.y, &b.y, 64) == 0)); }

// a verification key's point (plain integers) in the key's own form (Montgomery; infinity: zero bytes); false if a coordinate is >= q
bool vk_g1(const uint8_t* p, uint8_t out[64]) {
    G1A a;
    if (!load_g1(p, false, &a)) return false;
    memset(out, 0, 64);
    if (!a.inf) { memcpy(out, &a.x, 32); memcpy(out + 32, &a.y, 32); }
    return true;
}
bool vk_g2(const uint8_t* p, uint8_t out[128]) {
    G2A a;
    if (!load_g2(p, false, &a)) return false;
    memset(out, 0, 128);
    if (!a.inf) { memcpy(out, &a.x, 64); memcpy(out + 64, &a.y, 64); }
    return true;
}

// host bytes [lo, lo + n) of a point array onto the device, then sum_i d_sc[i] P_i into `sum`
template <class F>
int staged_sum(Lane& L, void* d_pts, const uint8_t* src, uint64_t n, const Fe* d_sc, RhoSum<F>* sum, hipStream_t s,
               void (*release)(const void*, size_t)) {
    if (int rc = stage_chunk(d_pts, src, (size_t)n * sizeof(Affine<F>), s, release)) return rc;
    return sum->add(L, d_sc, reinterpret_cast<const Affine<F>*>(d_pts), n, s);
}
}  // namespace

int circuit_row_sums(const wsnark_circuit_t* K, const void* weights, void* out_public, void* out_private) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (!weights || !out_public || !out_private) return WS_ERR_ARG;
    int rc;
    if ((rc = circuit_shape_check(K))) return rc;
    const uint64_t n = K->domain;
    LaneLock L = acquire_lane(X);
    hipStream_t s = L->stream;
    CsrMatrix M[3];
    if ((rc = circuit_to_csr(K, M, s))) return rc;
    DevBuf d_w, d_out;
    WS_HIP_CHECK(d_w.alloc((size_t)K->n_vars * 32));
    WS_HIP_CHECK(d_out.alloc((size_t)6 * n * 32));
    if ((rc = upload_staged(d_w.p, weights, (size_t)K->n_vars * 32, s))) return rc;
    if ((rc = lc_split_dev(X, M, d_w.as<Fe>(), K->n_public, K->domain, d_out.as<Fe>(), d_out.as<Fe>() + 3 * n, s))) return rc;
    WS_HIP_CHECK(hipMemcpyAsync(out_public, d_out.p, (size_t)3 * n * 32, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipMemcpyAsync(out_private, d_out.as<Fe>() + 3 * n, (size_t)3 * n * 32, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    return WS_OK;
}

int pkey_circuit_check_sections(const KeySections& S, const wsnark_powers_t* P, const wsnark_circuit_t* K, const uint8_t* vk, size_t vk_len,
                                uint64_t n_inputs, const uint8_t* seed32, wsnark_pkey_circuit_verdict_t* out) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (!out) return WS_ERR_ARG;
    int rc;
    // everything that can fail, before anything is written
    if ((rc = circuit_shape_check(K))) return rc;
    const uint64_t n = K->domain, nv = K->n_vars, np = K->n_public;
    if ((rc = powers_shape_check(P, n))) return rc;
    if ((rc = key_shape_check(S))) return rc;
    if (vk && (n_inputs > ((uint64_t)1 << 32) || vk_len < 448 + (n_inputs + 1) * 64)) {
        set_last_error("circuit check: the verification key holds fewer than n_inputs + 1 IC points");
        return WS_ERR_SIZE;
    }
    uint8_t seed[32];
    if ((rc = draw_seed(seed32, seed))) return rc;
    const auto t_begin = Clock::now();
    wsnark_pkey_circuit_verdict_t V;
    memset(&V, 0, sizeof V);
    const uint32_t requested = vk ? 0x3ffu : 0xffu;

    double ms_mat = 0, ms_key = 0, ms_pow = 0, ms_pair = 0;
    auto t0 = Clock::now();

    // bit 0: the key is a key of this shape, and its two record streams are the circuit's
    const bool same_counts = S.n_vars == K->n_vars && S.n_public == K->n_public && S.domain == K->domain;
    V.checks_run |= 1;
    {
        bool same = same_counts && S.lenA == K->polsA_len && S.lenB == K->polsB_len;
        auto cmp = [&](const uint8_t* a, const uint8_t* b, uint64_t len) {
            for (uint64_t at = 0; same && at < len; at += (uint64_t)16 << 20) {      // in pieces: a mapped file gets its pages back
                const size_t piece = (size_t)std::min<uint64_t>(len - at, (uint64_t)16 << 20);
                same = memcmp(a + at, b + at, piece) == 0;
                if (S.release) S.release(a + at, piece);
            }
        };
        if (same) {
            cmp(S.polsA, (const uint8_t*)K->polsA, S.lenA);
            cmp(S.polsB, (const uint8_t*)K->polsB, S.lenB);
        }
        if (!same) V.checks_bad |= 1;
    }
    // bit 1: the fixed points that come straight from the transcript
    if (same_counts) V.checks_run |= 2;
    if (same_counts && (memcmp(S.alfa1, P->alpha_tau_g1, 64) != 0 || memcmp(S.beta1, P->beta_tau_g1, 64) != 0 || memcmp(S.beta2, P->beta_g2, 128) != 0)) V.checks_bad |= 2;
    // bit 2: delta1 and delta2 hold the same logarithm
    G1A d1;
    G2A d2;
    t0 = Clock::now();
    if (same_counts && fixed_g1(S.delta1, true, &d1) == 0 && fixed_g2(S.delta2, true, &d2) == 0) {
        V.checks_run |= 4;
        if (!same_log(d1, d2)) V.checks_bad |= 4;
    }
    const bool with_delta = (V.checks_run & 4) && !(V.checks_bad & 4);      // bits 6, 7 mean something
    // bit 8, and what bit 9 needs: the verification key in the key's own form
    G2A gamma2;
    bool with_gamma = false;
    std::vector<uint8_t> ic;
    if (vk && same_counts) {
        V.checks_run |= 256;
        uint8_t a1[64], b2[128], g2b[128], dl2[128];
        const bool red = vk_g1(vk, a1) && vk_g2(vk + 64, b2) && vk_g2(vk + 320, dl2);
        if (!red || n_inputs != np || memcmp(a1, S.alfa1, 64) != 0 || memcmp(b2, S.beta2, 128) != 0 || memcmp(dl2, S.delta2, 128) != 0) V.checks_bad |= 256;
        with_gamma = n_inputs == np && vk_g2(vk + 192, g2b) && fixed_g2(g2b, true, &gamma2) == 0;
        if (with_gamma) {
            ic.resize((size_t)(np + 1) * 64);
            for (uint64_t j = 0; with_gamma && j <= np; j++) {
                G1A pt;
                with_gamma = vk_g1(vk + 448 + 64 * j, ic.data() + 64 * j) && fixed_g1(ic.data() + 64 * j, true, &pt) == 0;
            }
        }
    }
    ms_pair += ms_since(t0);

    G1A keyA, keyB1, keyC, keyH, keyIC, powA, powB1, Kv, Kp, Hd;
    G2A keyB2, powB2;
    {
        LaneLock L = acquire_lane(X);
        hipStream_t s = L->stream;
        t0 = Clock::now();
        CsrMatrix M[3];
        if ((rc = circuit_to_csr(K, M, s))) return rc;      // (a stream the loaders reject is an error whatever bit 0 says)
        ms_mat = ms_since(t0);
        if (!same_counts) {      // sections of other lengths: nothing else can be asked
            wipe(seed, sizeof seed);
            V.ms[0] = ms_mat;
            V.ms[4] = ms_since(t_begin);
            *out = V;
            return WS_OK;
        }
        const uint64_t chunk = key_chunk("PKCIRCUIT_CHUNK");
        const uint64_t cap = key_chunk_cap(chunk, std::max<uint64_t>(nv, n));
        DevBuf d_vec, d_pts, d_rho;
        WS_HIP_CHECK(d_vec.alloc((size_t)6 * n * 32));      // p_A p_B p_C v_A v_B v_C, then their coefficient vectors in place
        Fe* vec = d_vec.as<Fe>();
        Fe* const pub[3] = {vec, vec + n, vec + 2 * n};
        Fe* const prv[3] = {vec + 3 * n, vec + 4 * n, vec + 5 * n};

        // the row sums over rho_j, j < nVars, and c(x) = fromMontgomery(iNTT(x)) of the six
        t0 = Clock::now();
        {
            DevBuf d_w;      // (the weights of all signals live for the one kernel only)
            WS_HIP_CHECK(d_w.alloc((size_t)nv * 32));
            if ((rc = pkcheck_rho_dev(d_w.as<Fe>(), nv, 0, seed, s))) return rc;
            if ((rc = lc_split_dev(X, M, d_w.as<Fe>(), K->n_public, K->domain, vec, vec + 3 * n, s))) return rc;
            WS_HIP_CHECK(hipStreamSynchronize(s));
        }
        for (int k = 0; k < 6; k++)
            if ((rc = ntt_dev(*L, vec + (size_t)k * n, n, 0, 1, s))) return rc;
        if ((rc = fr_map_dev(vec, vec, 6 * n, 0, s))) return rc;
        WS_HIP_CHECK(hipStreamSynchronize(s));
        ms_mat += ms_since(t0);

        DevBuf d_sc, d_k;
        WS_HIP_CHECK(d_pts.alloc((size_t)cap * 192));      // a chunk of G2 points, or of three G1 arrays side by side
        WS_HIP_CHECK(d_rho.alloc((size_t)cap * 32));
        WS_HIP_CHECK(d_sc.alloc((size_t)cap * 64));        // a chunk of c(u_A) | c(u_B)
        WS_HIP_CHECK(d_k.alloc((size_t)cap * 96));         // a chunk of c(x_C) | c(x_A) | c(x_B), x = v then p
        Fe* rho = d_rho.as<Fe>();

        // the key's side: sum rho_j P_j per section, rho by the GLOBAL signal index (C starts at nPublic + 1, hExps at nVars)
        t0 = Clock::now();
        RhoSum<Fq> sA, sB1, sC, sH, sIC;
        RhoSum<Fq2> sB2;
        for (uint64_t lo = 0; lo < nv; lo += chunk) {
            const uint64_t m = std::min<uint64_t>(chunk, nv - lo);
            if ((rc = pkcheck_rho_dev(rho, m, lo, seed, s))) return rc;
            if ((rc = staged_sum(*L, d_pts.p, S.A + lo * 64, m, rho, &sA, s, S.release))) return rc;
            if ((rc = staged_sum(*L, d_pts.p, S.B1 + lo * 64, m, rho, &sB1, s, S.release))) return rc;
            if ((rc = staged_sum(*L, d_pts.p, S.B2 + lo * 128, m, rho, &sB2, s, S.release))) return rc;
        }
        const uint64_t nC = nv - np - 1;
        for (uint64_t lo = 0; with_delta && lo < nC; lo += chunk) {
            const uint64_t m = std::min<uint64_t>(chunk, nC - lo);
            if ((rc = pkcheck_rho_dev(rho, m, np + 1 + lo, seed, s))) return rc;
            if ((rc = staged_sum(*L, d_pts.p, S.Cpts + lo * 64, m, rho, &sC, s, S.release))) return rc;
        }
        for (uint64_t lo = 0; with_delta && lo < n; lo += chunk) {
            const uint64_t m = std::min<uint64_t>(chunk, n - lo);
            if ((rc = pkcheck_rho_dev(rho, m, nv + lo, seed, s))) return rc;
            if ((rc = staged_sum(*L, d_pts.p, S.H + lo * 64, m, rho, &sH, s, S.release))) return rc;
        }
        for (uint64_t lo = 0; with_gamma && lo <= np; lo += chunk) {
            const uint64_t m = std::min<uint64_t>(chunk, np + 1 - lo);
            if ((rc = pkcheck_rho_dev(rho, m, lo, seed, s))) return rc;
            if ((rc = staged_sum(*L, d_pts.p, ic.data() + lo * 64, m, rho, &sIC, s, nullptr))) return rc;
        }
        WS_HIP_CHECK(hipStreamSynchronize(s));
        keyA = sA.finish(); keyB1 = sB1.finish(); keyB2 = sB2.finish(); keyC = sC.finish(); keyH = sH.finish(); keyIC = sIC.finish();
        ms_key = ms_since(t0);

        // the transcript's side: a chunk of powers against the resident coefficients at the chunk's offset
        t0 = Clock::now();
        RhoSum<Fq> tA, tB1, tKv, tKp, tHhi, tHlo;
        RhoSum<Fq2> tB2;
        const uint8_t* tau1 = (const uint8_t*)P->tau_g1;
        for (uint64_t lo = 0; lo < n; lo += chunk) {
            const uint64_t m = std::min<uint64_t>(chunk, n - lo);
            const Affine<Fq>* p1 = d_pts.as<Affine<Fq>>();
            Fe* uA = d_sc.as<Fe>();
            Fe* uB = uA + m;
            Fe* kx = d_k.as<Fe>();
            // tau_g1[k] against c(u_A) and c(u_B); hExps' lower term
            if ((rc = stage_chunk(d_pts.p, tau1 + lo * 64, (size_t)m * 64, s, nullptr))) return rc;
            hipLaunchKernelGGL(fr_add_kernel, dim3(ceil_div_u64(m, 256)), dim3(256), 0, s, pub[0] + lo, prv[0] + lo, uA, m);
            hipLaunchKernelGGL(fr_add_kernel, dim3(ceil_div_u64(m, 256)), dim3(256), 0, s, pub[1] + lo, prv[1] + lo, uB, m);
            WS_HIP_CHECK(hipGetLastError());
            if ((rc = tA.add(*L, uA, p1, m, s)) || (rc = tB1.add(*L, uB, p1, m, s))) return rc;
            if (with_delta) {
                if ((rc = pkcheck_rho_dev(rho, m, nv + lo, seed, s))) return rc;
                if ((rc = tHlo.add(*L, rho, p1, m, s))) return rc;
            }
            if (with_delta || with_gamma) {
                // K_x over tau_g1[k] | beta_tau_g1[k] | alpha_tau_g1[k] side by side against c(x_C) | c(x_A) | c(x_B): one sum of 3m terms
                if ((rc = stage_chunk(d_pts.as<uint8_t>() + m * 64, (const uint8_t*)P->beta_tau_g1 + lo * 64, (size_t)m * 64, s, nullptr))) return rc;
                if ((rc = stage_chunk(d_pts.as<uint8_t>() + 2 * m * 64, (const uint8_t*)P->alpha_tau_g1 + lo * 64, (size_t)m * 64, s, nullptr))) return rc;
                for (int x = 0; x < 2; x++) {
                    if (!(x == 0 ? with_delta : with_gamma)) continue;
                    Fe* const* vecs = x == 0 ? prv : pub;
                    const int order[3] = {2, 0, 1};
                    for (int q = 0; q < 3; q++)
                        WS_HIP_CHECK(hipMemcpyAsync(kx + q * m, vecs[order[q]] + lo, (size_t)m * 32, hipMemcpyDeviceToDevice, s));
                    if ((rc = (x == 0 ? tKv : tKp).add(*L, kx, p1, 3 * m, s))) return rc;
                }
            }
            // tau_g1[n + k]: hExps' upper term, the same rho'
            if (with_delta && (rc = staged_sum(*L, d_pts.p, tau1 + (n + lo) * 64, m, rho, &tHhi, s, nullptr))) return rc;
            // tau_g2[k] against c(u_B)
            if ((rc = staged_sum(*L, d_pts.p, (const uint8_t*)P->tau_g2 + lo * 128, m, uB, &tB2, s, nullptr))) return rc;
        }
        WS_HIP_CHECK(hipStreamSynchronize(s));
        powA = tA.finish(); powB1 = tB1.finish(); powB2 = tB2.finish(); Kv = tKv.finish(); Kp = tKp.finish();
        // sum rho'_i tau_g1[n + i] - sum rho'_i tau_g1[i]
        const G1A lo_sum = tHlo.finish();
        if (!lo_sum.inf) tHhi.part.push_back(Jac<Fq>{lo_sum.x, Fq::neg(lo_sum.y), Fq::one()});
        Hd = tHhi.finish();
        ms_pow = ms_since(t0);
    }      // (the lane goes back before the pairings: they need none)

    // bits 3, 4, 5: equal points
    V.checks_run |= 8 | 16 | 32;
    if (!same_point(keyA, powA)) V.checks_bad |= 8;
    if (!same_point(keyB1, powB1)) V.checks_bad |= 16;
    if (!same_point(keyB2, powB2)) V.checks_bad |= 32;
    t0 = Clock::now();
    const G2A g2 = gen2();
    if (with_delta) {
        V.checks_run |= 64 | 128;
        if (!same_pairing(keyC, d2, Kv, g2)) V.checks_bad |= 64;
        if (!same_pairing(keyH, d2, Hd, g2)) V.checks_bad |= 128;
    }
    if (with_gamma) {
        V.checks_run |= 512;
        if (!same_pairing(keyIC, gamma2, Kp, g2)) V.checks_bad |= 512;
    }
    ms_pair += ms_since(t0);
    wipe(seed, sizeof seed);
    V.ok = (V.checks_run == requested && V.checks_bad == 0) ? 1 : 0;
    V.ms[0] = ms_mat;
    V.ms[1] = ms_key;
    V.ms[2] = ms_pow;
    V.ms[3] = ms_pair;
    V.ms[4] = ms_since(t_begin);
    *out = V;
    return WS_OK;
}

}  // namespace wsnark
