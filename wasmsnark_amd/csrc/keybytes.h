// keybytes.h -- the parts shared by everything that walks the BYTES of a proving key: the loaders (prove.hip, keyfile.hip), the audit
// (pkeycheck.hip) and the phase-2 contribution with its check (pkeydelta.hip).  One copy each of: the header conditions a key must
// meet and its five section counts; the per-point classifier on the device and its reduction; the decoding of that reduction on
// the host; the fixed-point tests and the pairing relation; the seed draw; the chunked staging; the random-combination sums.
#pragma once
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "../../include/wsnark.h"
#include "internal.h"
#include "fp12_host.h"

namespace wsnark {

// ---- a key's shape ----
// the first header condition alone (nPublic + 1 <= nVars): the parsers need nVars - nPublic - 1 before they can bound a section
int key_vars_check(uint32_t n_vars, uint32_t n_public);
// what every consumer of a key's bytes rejects, with the loaders' codes and messages, in this order: too few variables for the inputs
// (WS_ERR_FORMAT), domainSize not a power of two in [2, 2^27] (WS_ERR_SIZE), a point section shorter than the header implies
// (WS_ERR_FORMAT)
int key_shape_check(const KeySections& S);
// points per section, indexed by WSNARK_PK_A .. WSNARK_PK_H (a key that passed key_shape_check)
struct KeyCounts {
    uint64_t n[5];
    uint64_t operator[](int k) const { return n[k]; }
};
inline KeyCounts key_counts(const KeySections& S) {
    const uint64_t nv = S.n_vars;
    return KeyCounts{{nv, nv, nv, nv - S.n_public - 1, S.domain}};
}

// ---- the per-point tests (device) ----
// one section's running result; `first` holds ~(index << 3 | reason) of the smallest bad index (0 = none) so that atomicMax finds
// the minimum
struct PkAcc { unsigned long long inf, bad, first; };

__device__ inline bool pk_ge(const Fe& x, const uint64_t* m) {        // x >= m
    for (int i = 3; i >= 0; i--) {
        if (x.l[i] > m[i]) return true;
        if (x.l[i] < m[i]) return false;
    }
    return true;
}
__device__ inline bool pk_zero(const Fe& x) { return (x.l[0] | x.l[1] | x.l[2] | x.l[3]) == 0; }

// One point of a key in reference format (canonical Montgomery words) -> pk_reduce's state: 4 infinity by the loaders' rule (every
// word of x zero; y is never read), 1 a coordinate word string >= q, 2 off the curve sqr(Y) == X^3 + b, 0 good -- and then *P is
// the point in the field's internal form.  curve_b: 3 on G1, 3 / (9 + u) on the twist, internal form (pk_curve_b).
template <class C>
__device__ inline int pk_classify(const typename C::AffP& p, const typename C::El& curve_b, typename C::Aff* P) {
    typedef typename C::Field F;
    constexpr int NW = (int)(sizeof(typename C::AffP) / 32);      // 32-byte words of a point: 2 (G1), 4 (G2); the first half is x
    const uint64_t q[4] = {FqParams::P0, FqParams::P1, FqParams::P2, FqParams::P3};
    const Fe* w = reinterpret_cast<const Fe*>(&p);
    typename C::AffP v;                                            // every word is loaded once, the y half only behind a finite x
    Fe* vw = reinterpret_cast<Fe*>(&v);
    bool inf = true, big = false;
    for (int k = 0; k < NW / 2; k++) { vw[k] = w[k]; inf = inf && pk_zero(vw[k]); }
    if (inf) return 4;
    for (int k = NW / 2; k < NW; k++) vw[k] = w[k];
    for (int k = 0; k < NW; k++) big = big || pk_ge(vw[k], q);
    if (big) return 1;
    *P = C::aff_to_internal(v);
    if (!F::eq(F::sqr(P->y), F::add(F::mul(F::sqr(P->x), P->x), curve_b))) return 2;
    return 0;
}

// st: 0 good, 1..3 the reason, 4 infinity.  Every lane of the wavefront arrives here (lanes past the end with st = 0).
__device__ inline void pk_reduce(int st, uint64_t index, PkAcc* __restrict__ acc) {
    const unsigned long long m_inf = __ballot(st == 4), m_bad = __ballot(st >= 1 && st <= 3);
    if ((threadIdx.x & 63) == 0) {
        if (m_inf) atomicAdd(&acc->inf, (unsigned long long)__popcll(m_inf));
        if (m_bad) atomicAdd(&acc->bad, (unsigned long long)__popcll(m_bad));
    }
    if (st >= 1 && st <= 3) atomicMax(&acc->first, ~(((unsigned long long)index << 3) | (unsigned long long)st));
}

// ---- one scalar for many points (pkeydelta.hip: scale_points_kernel; pkeysetup.hip: the twiddles of the group transform and the
// coefficients of the column sums) ----
// a wipe the compiler cannot drop: the stores are volatile
inline void wipe(void* p, size_t n) {
    volatile uint8_t* v = reinterpret_cast<volatile uint8_t*>(p);
    for (size_t i = 0; i < n; i++) v[i] = 0;
}

// the scalar in non-adjacent form: digit i is non-zero iff bit i of nz, negative iff bit i of neg; top = index of the leading digit
// (always +1), -1 for k = 0.  k < r < 2^254, so the form has at most 255 digits.
struct ScaleDigits { uint64_t nz[4], neg[4]; int32_t top; };

// word w of a four-word digit mask held in registers: selects, so that the masks stay in registers (an index would put them in scratch)
__device__ __forceinline__ uint64_t word4(uint64_t a0, uint64_t a1, uint64_t a2, uint64_t a3, int w) {
    uint64_t r = a0;
    r = w == 1 ? a1 : r;
    r = w == 2 ? a2 : r;
    r = w == 3 ? a3 : r;
    return r;
}
// k (plain, < 2^255) -> non-adjacent form: while k: odd -> digit 2 - (k mod 4) in {1, -1}, k -= digit; k >>= 1.  On the host k may be
// a contribution's secret (pkeydelta.hip: d^-1, the scalar of scale_batch): the working words are wiped before the function returns.
WS_HD void naf_digits(const Fe& k, ScaleDigits* D) {
    for (int i = 0; i < 4; i++) D->nz[i] = D->neg[i] = 0;
    D->top = -1;
    uint64_t w[5] = {k.l[0], k.l[1], k.l[2], k.l[3], 0};
    for (int i = 0; i < 256 && (w[0] | w[1] | w[2] | w[3] | w[4]); i++) {
        if (w[0] & 1) {
            D->nz[i >> 6] |= (uint64_t)1 << (i & 63);
            D->top = i;
            if ((w[0] & 3) == 3) {                      // digit -1: k += 1 (the carry chain of a run of ones)
                D->neg[i >> 6] |= (uint64_t)1 << (i & 63);
                for (int j = 0; j < 5 && ++w[j] == 0; j++) {}
            } else {
                w[0] -= 1;
            }
        }
        for (int j = 0; j < 4; j++) w[j] = (w[j] >> 1) | (w[j + 1] << 63);
        w[4] >>= 1;
    }
#ifndef __HIP_DEVICE_COMPILE__
    wipe(w, sizeof w);
#endif
}

// The double-and-add chain over the digits z (non-zero) and g (negative), most significant first: a enters as P itself in XYZZ -- the
// leading digit `top` is +1 -- and leaves as k P.  The masks are eight values, not two arrays: they stay in registers (word4), and
// where the caller's digits are the wavefront's (the argument block of scale_points_kernel, readfirstlane in the group transform)
// the digit test is a scalar branch.
// Every addition is C::madd, the mixed addition WITH all four corner cases, and it has to be: a = m P with m the value of the digits
// read so far, doubled; a == +/-P happens iff 2m = +/-1 mod ord(P), which a scalar near the group order reaches in its last steps
// (k = r - 2 passes through -P and adds -P: a doubling), and which a G2 point outside the order-r subgroup -- legal input here, the
// subgroup test is the audit's -- can reach anywhere; a == infinity follows one step later.  The unguarded madd_fast would need a
// proof that the input has order r and that no digit prefix is +/-1/2 mod r: not available.  The doubling handles infinity and
// y == 0 by itself (curve.h).
template <class C>
__device__ __forceinline__ void naf_chain(typename C::Pt& a, const typename C::Aff& P, uint64_t z0, uint64_t z1, uint64_t z2, uint64_t z3,
                                          uint64_t g0, uint64_t g1, uint64_t g2, uint64_t g3, int top) {
#pragma unroll 1
    for (int d = top - 1; d >= 0; d--) {
        a = C::dbl(a);
        if ((word4(z0, z1, z2, z3, d >> 6) >> (d & 63)) & 1) C::madd(a, P, ((word4(g0, g1, g2, g3, d >> 6) >> (d & 63)) & 1) != 0);
    }
}

// One result R (XYZZ) behind its inverse inv = 1 / (ZZ ZZZ): affine, in reference format (last: canonical words, what leaves the
// device) or in the field's packed internal form (between the stages of the group transform).  Not finite -- R = O, which x == 0
// encodes, or a lane whose input was bad (unspecified) -- is zero bytes.
template <class C>
__device__ inline typename C::AffP affine_result(const typename C::Pt& R, bool fin, const typename C::El& inv, int last) {
    typedef typename C::Field F;
    typename C::AffP r;
    if (!fin) {
        memset(&r, 0, sizeof r);
    } else {
        const typename C::El x = F::mul(R.x, F::mul(inv, R.zzz)), y = F::mul(R.y, F::mul(inv, R.zz));
        r = last ? typename C::AffP{F::from_internal(x), F::from_internal(y)} : typename C::AffP{F::pack(x), F::pack(y)};
    }
    return r;
}

// 1 / z for every lane of a 256-lane workgroup behind ONE inversion: heap-ordered products in LDS, node j = node 2j x node 2j+1,
// leaves 256 + lane; wavefront 0 inverts the root while the other three wait; down again node j holds the INVERSE of its product: the
// children of j are inv(j) x the sibling's product, both written by the one lane that read both (24 products and a quarter of an
// inversion per lane instead of a Fermat inversion's 363).  Every lane of the workgroup arrives (a lane with nothing to invert passes
// 1); once per kernel.
template <class F>
__device__ inline typename F::El block_inverse(const typename F::El& z) {
    typedef typename F::El El;
    __shared__ El tree[512];
    const unsigned l = threadIdx.x;
    tree[256 + l] = z;
    __syncthreads();
    for (unsigned w = 128; w >= 1; w >>= 1) {
        if (l < w) tree[w + l] = F::mul(tree[2 * (w + l)], tree[2 * (w + l) + 1]);
        __syncthreads();
    }
    if (l < 64) {                             // every lane the same value: a uniform chain, one store
        const El r = F::inv(tree[1]);
        if (l == 0) tree[1] = r;
    }
    __syncthreads();
    for (unsigned w = 1; w <= 128; w <<= 1) {
        if (l < w) {
            const El up = tree[w + l], lo = tree[2 * (w + l)], hi = tree[2 * (w + l) + 1];
            tree[2 * (w + l)] = F::mul(up, hi);
            tree[2 * (w + l) + 1] = F::mul(up, lo);
        }
        __syncthreads();
    }
    return tree[256 + l];
}

// ---- host ----
// a section's result as the reports hold it: *first_bad = UINT64_MAX and *first_reason = 0 without a bad point
inline void pk_decode(const PkAcc& a, uint64_t* inf, uint64_t* bad, uint64_t* first_bad, uint32_t* first_reason) {
    const unsigned long long key = ~a.first;
    *inf = a.inf;
    *bad = a.bad;
    *first_bad = a.first ? key >> 3 : UINT64_MAX;
    *first_reason = a.first ? (uint32_t)(key & 7) : 0;
}
// pk_classify's curve_b for the two device curves (either may be nullptr); the twist's comes from pairing_consts
int pk_curve_b(G1R29::El* b1, G2R29::El* b2);
inline int curve_b(G1R29::El* out) { return pk_curve_b(out, nullptr); }
inline int curve_b(G2R29::El* out) { return pk_curve_b(nullptr, out); }
// k32 (plain LE, any 256-bit value, possibly a secret: the copy is wiped) reduced mod r
inline Fe load_scalar(const uint8_t* k32) {
    Fe k;
    memcpy(&k, k32, 32);
    const Fe r = Fr::reduce_full(k);
    wipe(&k, sizeof k);
    return r;
}

// reference-format bytes -> the host pairing's point; the reason it is bad (0 = good).  check = false: only the infinity rule
uint32_t fixed_g1(const uint8_t* p, bool check, hostpair::G1A* out);
uint32_t fixed_g2(const uint8_t* p, bool check, hostpair::G2A* out);
hostpair::G1A gen1();
hostpair::G2A gen2();
// e(P1, Q1) == e(P2, Q2): two Miller values, one with a negated argument, one final exponentiation
bool same_pairing(const hostpair::G1A& P1, const hostpair::G2A& Q1, const hostpair::G1A& P2, const hostpair::G2A& Q2);
// e(P, G2) == e(G1, Q): P and Q hold the same logarithm
inline bool same_log(const hostpair::G1A& P, const hostpair::G2A& Q) { return same_pairing(P, gen2(), gen1(), Q); }

// out = the caller's 32 bytes, else the system's (os_random); WS_ERR_ARG with the entropy message if that fails
int draw_seed(const uint8_t* caller32, uint8_t out[32]);

typedef std::chrono::steady_clock Clock;
inline double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }

// points per chunk of a streamed section: the switch `name` (PKCHECK_CHUNK, PKDELTA_CHUNK, PKCIRCUIT_CHUNK; default 2^18) within [64, 2^22]
inline uint64_t key_chunk(const char* name) {
    return std::min<uint64_t>(std::max<uint64_t>((uint64_t)tuning_get(name, 1 << 18), 64), (uint64_t)1 << 22);
}
// ... and the points the device buffers must hold for sections of at most `most` points
inline uint64_t key_chunk_cap(uint64_t chunk, uint64_t most) { return std::min(chunk, std::max<uint64_t>(most, 1)); }
// one range of a section to the device through the staging ring; a mapped key file gets the range back (KeySections::release)
inline int stage_chunk(void* d_dst, const uint8_t* src, size_t bytes, hipStream_t s, void (*release)(const void*, size_t)) {
    const int rc = upload_staged(d_dst, src, bytes, s);
    if (!rc && release) release(src, bytes);
    return rc;
}

// pieces of ONE device allocation (calch.hip on why: every hipMalloc / hipFree is a call into the driver, and a free waits for the device)
struct Slab {
    DevBuf buf;
    std::vector<std::pair<void**, size_t>> want;
    static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
    template <class T> void add(T** p, size_t bytes) { want.emplace_back((void**)p, up256(bytes ? bytes : 1)); }
    hipError_t alloc() {
        size_t total = 0;
        for (auto& w : want) total += w.second;
        const hipError_t e = buf.alloc(total);
        if (e != hipSuccess) return e;
        size_t off = 0;
        for (auto& w : want) { *w.first = (uint8_t*)buf.p + off; off += w.second; }
        return hipSuccess;
    }
};

// d_out[i] = rho_(base + i), i < n: 128 non-zero bits of the ChaCha20 block under key = seed32, counter = the global index
int pkcheck_rho_dev(Fe* d_out, uint64_t n, uint64_t base, const uint8_t* seed32, hipStream_t s);

// sum_j rho_j P_j over a section that goes through the device chunk by chunk: each resident chunk is summed by the ordinary MSM on
// the caller's lane and queue, the partial sums are added on the host.  F = Fq: G1, Fq2: G2.
inline int rho_msm(Lane& L, const Fe* d_rho, const Affine<Fq>* d_pts, uint64_t n, Jac<Fq>* out, hipStream_t s) {
    return msm_g1_dev(L, d_rho, d_pts, n, WindowShard{}, out, s);
}
inline int rho_msm(Lane& L, const Fe* d_rho, const Affine<Fq2>* d_pts, uint64_t n, Jac<Fq2>* out, hipStream_t s) {
    return msm_g2_dev(L, d_rho, d_pts, n, WindowShard{}, out, s);
}
inline hostpair::G1A rho_total(const std::vector<Jac<Fq>>& part) {
    Jac<Fq> t;
    g1_sum_host(reinterpret_cast<const uint8_t*>(part.data()), part.size(), reinterpret_cast<uint8_t*>(&t));
    return hostpair::G1A{t.x, t.y, Fq::is_zero(t.z)};
}
inline hostpair::G2A rho_total(const std::vector<Jac<Fq2>>& part) {
    Jac<Fq2> t;
    g2_sum_host(reinterpret_cast<const uint8_t*>(part.data()), part.size(), reinterpret_cast<uint8_t*>(&t));
    return hostpair::G2A{t.x, t.y, Fq2::is_zero(t.z)};
}
template <class F>
struct RhoSum {
    std::vector<Jac<F>> part;
    int add(Lane& L, const Fe* d_rho, const Affine<F>* d_pts, uint64_t n, hipStream_t s) {
        Jac<F> p;
        const int rc = rho_msm(L, d_rho, d_pts, n, &p, s);
        if (!rc) part.push_back(p);
        return rc;
    }
    auto finish() const { return rho_total(part); }      // the host pairing's affine point
};

// ---- the workers behind the C ABI (cabi.hip opens the bytes, the sections or the file) ----
int pkey_check_sections(const KeySections& S, uint32_t flags, const uint8_t* seed32, wsnark_pkey_report_t* out);
int g1_scale_batch(const void* points, uint64_t n, const void* k32, void* out);
int g2_scale_batch(const void* points, uint64_t n, const void* k32, void* out);
// d_out[i] = k d_in[i] on device-resident points in reference format (k given by its digits), on queue s; d_acc takes pk_reduce's counts
int g1_scale_dev(Context* X, const void* d_in, uint64_t n, const ScaleDigits& D, void* d_out, PkAcc* d_acc, hipStream_t s);
int g2_scale_dev(Context* X, const void* d_in, uint64_t n, const ScaleDigits& D, void* d_out, PkAcc* d_acc, hipStream_t s);
// the group transforms (pkeysetup.hip)
int g1_group_ntt(const void* points, uint64_t n, int inverse, void* out);
int g2_group_ntt(const void* points, uint64_t n, int inverse, void* out);
// out: pointsA, pointsB1, pointsB2, pointsC, pointsH, alfa1, beta1, delta1, beta2, delta2, IC
int pkey_setup_sections(const wsnark_powers_t* P, const wsnark_circuit_t* K, void* const out[11], wsnark_pkey_setup_report_t* rep);
int pkey_setup_size(const wsnark_circuit_t* K, size_t* out_len);
int pkey_setup_bytes(const wsnark_powers_t* P, const wsnark_circuit_t* K, uint8_t* out, size_t out_cap, size_t* out_len, uint8_t* out_ic,
                     wsnark_pkey_setup_report_t* rep);
int pkey_contribute_sections(const KeySections& S, const uint8_t* d32, uint8_t* out_pointsC, uint8_t* out_pointsH, uint8_t* out_delta1,
                             uint8_t* out_delta2, wsnark_pkey_delta_report_t* rep);
// S: the sections of the image pkey[0 .. len) (pkey_parse)
int pkey_contribute_bytes(const KeySections& S, const uint8_t* pkey, size_t len, const uint8_t* d32, uint8_t* out, size_t out_cap,
                          wsnark_pkey_delta_report_t* rep);
// S: the sections of the mapped file F (keyfile_open of in_path)
int pkey_contribute_file(const KeySections& S, const KeyFile& F, const char* in_path, const char* out_path, const uint8_t* d32,
                         wsnark_pkey_delta_report_t* rep);
int pkey_delta_verify_sections(const KeySections& O, const KeySections& N, const uint8_t* seed32, wsnark_pkey_delta_verdict_t* out);
// a key against its circuit and its powers of tau (pkeycircuit.hip); vk: wsnark_groth16_verify's layout or nullptr
int pkey_circuit_check_sections(const KeySections& S, const wsnark_powers_t* P, const wsnark_circuit_t* K, const uint8_t* vk, size_t vk_len,
                                uint64_t n_inputs, const uint8_t* seed32, wsnark_pkey_circuit_verdict_t* out);
int circuit_row_sums(const wsnark_circuit_t* K, const void* weights, void* out_public, void* out_private);
// what setup_prepare (pkeysetup.hip) rejects of a circuit, with its codes; the three record streams as row-major CSR with the loaders'
// conditions and codes (a truncated stream, a record index >= domain: WS_ERR_FORMAT)
int circuit_shape_check(const wsnark_circuit_t* K);
int circuit_to_csr(const wsnark_circuit_t* K, CsrMatrix M[3], hipStream_t s);
// a witness against its circuit (witcheck.hip): a circuit's three matrices resident as row-major CSR; which rows fail for a witness on
// the host or (on_device) already resident, on queue s (nullptr: the lane's own)
struct CircuitRes {
    Context* owner = nullptr;
    uint32_t n_vars = 0, n_public = 0, domain = 0;
    CsrMatrix M[3];
    double load_ms = 0;
};
Context* circuit_context(const CircuitRes* H);
int circuit_load(const wsnark_circuit_t* K, CircuitRes** out);
void circuit_free(CircuitRes* H);
void circuit_info(const CircuitRes* H, uint32_t* n_vars, uint32_t* n_public, uint32_t* domain, uint64_t nnz[3], uint64_t* bytes);
int circuit_witness_check(CircuitRes* H, const void* witness, size_t witness_len, bool on_device, uint64_t* bad_rows, void* bad_values,
                          uint64_t cap, wsnark_witness_report_t* rep, hipStream_t s);
int witness_check(const wsnark_circuit_t* K, const void* witness, size_t witness_len, uint64_t* bad_rows, void* bad_values, uint64_t cap,
                  wsnark_witness_report_t* rep);
// many witnesses against one resident circuit in one call; witnesses / outputs as include/wsnark.h: wsnark_circuit_witness_check_batch
int circuit_witness_check_batch(CircuitRes* H, const void* witnesses, size_t witness_stride, uint64_t count, bool on_device,
                                wsnark_witness_verdict_t* verdicts, uint64_t* bad_rows, void* bad_values, uint64_t cap,
                                wsnark_witness_batch_report_t* rep, hipStream_t stream);
// a circuit in row form (circuitrows.hip): the sizes, the three record streams, the resident handle built directly
int circuit_from_rows_size(const wsnark_rows_t* R, uint32_t flags, uint32_t* domain, uint64_t lens[3]);
int circuit_from_rows(const wsnark_rows_t* R, uint32_t flags, void* const out[3], const uint64_t cap[3], uint32_t* domain, wsnark_rows_report_t* rep);
int circuit_load_rows(const wsnark_rows_t* R, uint32_t flags, CircuitRes** out);
// ... and its sort and its emit on device-resident (key, entry) pairs (zkey.hip: a .zkey's coefficient records in, a key's streams out
// by constraint).  One matrix's running result; first_bad holds ~index of the smallest bad entry (0 = none) so that atomicMax finds the
// minimum (PkAcc)
struct RowsAcc { unsigned long long first_bad, unreduced, zero, empty, max_column; };
// the sort's arrays, the caller's: two pairs of n words each, three arrays of rows_sort_counters words, ceil(that / 1024) words; tile = rows_tile's
struct RowsSort { uint32_t* key[2]; uint32_t* val[2]; uint32_t *hist, *base, *cursor, *tiles; uint32_t tile; };
inline uint32_t rows_sort_counters(uint64_t most, uint32_t tile) { return 64 * (uint32_t)((std::max<uint64_t>(most, 1) + tile - 1) / tile); }
int rows_tile(uint32_t* tile);      // ROWS_TILE, a multiple of 256 in [256, 4096], else WS_ERR_ARG
int rows_sort_dev(Context* X, const RowsSort& B, uint32_t n, uint32_t first_bit, uint32_t bits, int* cur, hipStream_t s);
int rows_emit_dev(Context* X, const uint32_t* d_key, const uint32_t* d_val, uint32_t n, uint32_t nnz, uint32_t n_vars, const uint32_t* d_row,
                  const Fe* d_coef, uint32_t* d_words, RowsAcc* d_acc, hipStream_t s);
// the audit's per-point kernels on device-resident points in reference format (pkeycheck.hip): counts into d_acc with the global index
// base + i; the G2 one with the order-r subgroup test (PKCHECK_SUBGROUP picks its form), d_K: the pairing constants on the device
int pkcheck_g1_dev(Context* X, const void* d_pts, uint64_t n, uint64_t base, PkAcc* d_acc, hipStream_t s);
int pkcheck_g2_dev(Context* X, const void* d_pts, uint64_t n, uint64_t base, const PairConsts* d_K, PkAcc* d_acc, hipStream_t s);
// many witnesses of one resident key in one call (provebatch.hip); witnesses / outputs as include/wsnark.h: wsnark_groth16_prove_batch
int groth16_prove_batch(ProvingKey* K, const void* witnesses, size_t witness_stride, uint64_t count, bool on_device, const uint8_t* r32s,
                        const uint8_t* s32s, uint8_t* out384s, uint8_t* out_rs64s, wsnark_prove_batch_report_t* rep, hipStream_t stream);
// powers of tau (pwtau.hip): a scalar per point, the phase-1 contribution, the transcript's audit
int g1_mul_batch(const void* points, const void* scalars, uint64_t n, void* out);
int g2_mul_batch(const void* points, const void* scalars, uint64_t n, void* out);
int powers_contribute(const wsnark_powers_t* P, const uint8_t* tau32, const uint8_t* alpha32, const uint8_t* beta32, uint8_t* const out[5],
                      wsnark_powers_report_t* rep);
int powers_check(const wsnark_powers_t* P, uint32_t flags, const uint8_t* seed32, wsnark_powers_report_t* rep);
// the pieces of the two above on device-resident G1 points in reference format, on queue s (zkey.hip: the H basis change is the
// group transform with a scalar per point in front of it or behind it).  group_root_of_unity: w_(2^bits), Montgomery;
// g1_ntt_load_dev: the input tests (counts into d_acc), the internal form and the bit reversal, d_in -> d_work; g1_ntt_stages_dev: the
// twiddle table into d_tw (n/2 entries) and the log2 n stages over d_work, reference format out, WITHOUT the inverse's 1/n;
// fr_powers_dev: d_out[i] = c t^(first + i), plain; g1_mul_dev: d_out[i] = d_scalars[i] d_pts[i] (d_out != d_pts), synchronises s
Fe group_root_of_unity(int bits);
int g1_ntt_load_dev(Context* X, const void* d_in, void* d_work, uint64_t n, int bits, PkAcc* d_acc, hipStream_t s);
int g1_ntt_stages_dev(Context* X, void* d_work, int bits, int inverse, ScaleDigits* d_tw, hipStream_t s);
int fr_powers_dev(Context* X, const Fe& c_mont, const Fe& t_mont, uint64_t first, uint64_t count, Fe* d_out, hipStream_t s);
int g1_mul_dev(Context* X, const void* d_pts, const Fe* d_scalars, uint64_t n, void* d_out, PkAcc* d_acc, hipStream_t s);
// snarkjs' .zkey (zkey.hip); include/wsnark.h has the contracts
int g1_h_basis(const void* points, uint64_t n, int to_lagrange, void* out);
int zkey_info(const uint8_t* zkey, size_t len, wsnark_zkey_info_t* out);
int zkey_import(const uint8_t* zkey, size_t len, void* const out[12], const uint64_t caps[12], uint8_t* out_pkey, size_t pkey_cap, size_t* out_len,
                uint8_t* out_vk, size_t vk_cap, wsnark_zkey_report_t* rep);
int zkey_export(const KeySections& S, const uint8_t* vk, size_t vk_len, uint64_t n_inputs, uint8_t* out, size_t cap, size_t* out_len,
                wsnark_zkey_report_t* rep);
// ... straight into a resident key (release: a mapped file's, see KeySections::release; out_vk and rep may be nullptr)
int zkey_load(const uint8_t* zkey, size_t len, void (*release)(const void*, size_t), ProvingKey** out, uint8_t* out_vk, size_t vk_cap,
              wsnark_zkey_report_t* rep);
int zkey_load_file(const char* path, ProvingKey** out, uint8_t* out_vk, size_t vk_cap, wsnark_zkey_report_t* rep);
int zkey_vk_len(const uint8_t* zkey, size_t len, size_t* out_len);      // host only, from the container and section 2 alone
int zkey_vk_len_file(const char* path, size_t* out_len);
int zkey_export_size(uint32_t n_vars, uint32_t n_public, uint32_t domain, uint64_t nnzA, uint64_t nnzB, size_t* out_len);

}  // namespace wsnark
