// pkeycheck.hip -- the audit of a proving key (wsnark_pkey_check / _check_sections / _check_file, include/wsnark.h).
//
// The loaders copy a key's five point sections to the device and never look at a point.  This file looks at every one of them,
// on the key's BYTES (reference format: canonical Montgomery words) -- after a load the points are in the device field's domain
// and an unreduced coordinate can no longer be told from a reduced one.
//
//   per point (one lane each, kernels pkcheck_g1 / pkcheck_g2; the first three tests are keybytes.h: pk_classify, which the
//   contribution's kernel applies too):
//     x == 0 (all words of x)            infinity by the loader's own rule (msm_points_mask_kernel, Curve::aff_is_inf): counted,
//                                        the rest of its bytes is not read -- the prover never reads them either
//     a coordinate word string >= q      WSNARK_PK_UNREDUCED
//     y^2 != x^3 + b                     WSNARK_PK_OFF_CURVE        (b = 3, on the twist 3 / (9 + u))
//     G2 only: [r] Q != O                WSNARK_PK_OUTSIDE_SUBGROUP (254 doublings + a mixed addition per set bit of r)
//                                        PKCHECK_SUBGROUP=1: psi(Q) == [6 x^2] Q instead (127 doublings; DESIGN.md section 4 has
//                                        both measured; the shipped verdict is the one of [r] Q)
//   A section is streamed through the staging ring in chunks of PKCHECK_CHUNK points (default 2^18), so the audit's device memory
//   is 224 bytes x chunk whatever the key's size; a mapped key file gets every range back as soon as it has been staged.
//   Counts and the first bad index are reduced on the device: one 64-bit add per wavefront (ballot) for the two counts, and for the
//   minimum one atomicMax on ~(index << 3 | reason) per bad point -- neither depends on the launch geometry or the chunk size.
//
//   relations (host pairings, fp12_host.h):  e(beta1, G2) = e(G1, beta2),  e(delta1, G2) = e(G1, delta2),  and
//     e(sum rho_j B1_j, G2) = e(G1, sum rho_j B2_j)  with rho_j = the first 128 bits of the ChaCha20 block (key = the seed,
//     counter = the GLOBAL index j), made non-zero.  B1 and B2 go up chunk by chunk side by side, each pair of chunks is summed by
//     the ordinary MSMs (msm_g1_dev / msm_g2_dev) over the chunk's rho, the partial sums are added on the host (keybytes.h: RhoSum).
//     If B1_j = b_j G1 and B2_j = b'_j G2 the check passes with b != b' only if sum rho_j (b_j - b'_j) = 0 mod r: probability
//     2^-128 over a seed the key's maker did not know.  A seed known in advance gives no soundness at all.
#include <string.h>

#include "fp12.h"
#include "keybytes.h"

namespace wsnark {

using namespace hostpair;

// ---- device ----
typedef Curve<Fq29> G1c;                    // products as calls: the kernel is bound by its loads, not by issue
typedef G2R29 G2c;                          // Curve<Fp2T<Fq29>>: products as calls, as in pairing.hip (the chain is ~12 000 of them)

__global__ __launch_bounds__(256) void pkcheck_g1_kernel(const G1c::AffP* __restrict__ pts, uint64_t n, uint64_t base, G1c::El curve_b,
                                                           PkAcc* __restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    G1c::Aff P;
    const int st = i < n ? pk_classify<G1c>(pts[i], curve_b, &P) : 0;
    pk_reduce(st, base + i, acc);
}

// mode 0: [r] Q == O.  mode 1: psi(Q) == [6 x^2] Q, psi = twist o Frobenius o untwist: (x, y) -> (conj(x) g^2, conj(y) g^3),
// g = xi^((p - 1) / 6) (PairConsts::gamma1), and 6 x^2 = p - r = the Miller loop's T (PairConsts::ate, bit 126 leading)
// (one wavefront per workgroup: the chain takes all 256 registers of a lane, so a SIMD holds one wavefront whatever the group size;
// measured the same as 256-lane groups -- a 2^16 key's 65 537 finite points are 1025 wavefronts, two rounds on 1024 SIMDs either way)
__global__ __launch_bounds__(64) void pkcheck_g2_kernel(const G2c::AffP* __restrict__ pts, uint64_t n, uint64_t base, G2c::El curve_b,
                                                           const PairConsts* __restrict__ K, int mode, PkAcc* __restrict__ acc) {
    typedef Fq2d F;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    G2c::Aff Q;
    int st = i < n ? pk_classify<G2c>(pts[i], curve_b, &Q) : 0;
    if (i < n && st == 0) {
        const F2d X = Q.x, Y = Q.y;
        G2c::Pt a = G2c::infinity();
        if (mode == 0) {
#pragma unroll 1
            for (int bit = 253; bit >= 0; bit--) {
                a = G2c::dbl(a);
                if ((K->r[bit >> 6] >> (bit & 63)) & 1) G2c::madd(a, Q, false);
            }
            if (!G2c::is_inf(a)) st = 3;
        } else {
#pragma unroll 1
            for (int bit = 126; bit >= 0; bit--) {
                a = G2c::dbl(a);
                if ((K->ate[bit >> 6] >> (bit & 63)) & 1) G2c::madd(a, Q, false);
            }
            const F2d px = F::mul(F2d{X.c0, Fq29::neg(X.c1)}, F2d{K->gamma1[1][0], K->gamma1[1][1]});
            const F2d py = F::mul(F2d{Y.c0, Fq29::neg(Y.c1)}, F2d{K->gamma1[2][0], K->gamma1[2][1]});
            if (G2c::is_inf(a) || !F::eq(F::mul(px, a.zz), a.x) || !F::eq(F::mul(py, a.zzz), a.y)) st = 3;
        }
    }
    pk_reduce(st, base + i, acc);
}

struct PkSeed { uint32_t w[8]; };
// rho_j for j = base .. base + n: words 0..3 of the ChaCha20 block (RFC 8439 state layout) under key = seed, 64-bit counter = j
__device__ inline uint32_t pk_rotl(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }
#define PK_QR(a, b, c, d)                          \
    a += b; d ^= a; d = pk_rotl(d, 16);            \
    c += d; b ^= c; b = pk_rotl(b, 12);            \
    a += b; d ^= a; d = pk_rotl(d, 8);             \
    c += d; b ^= c; b = pk_rotl(b, 7)
__global__ __launch_bounds__(256) void pkcheck_rho_kernel(Fe* __restrict__ out, uint64_t n, uint64_t base, PkSeed seed) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t j = base + i;
    uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, seed.w[0], seed.w[1], seed.w[2], seed.w[3],
                      seed.w[4], seed.w[5], seed.w[6], seed.w[7], (uint32_t)j, (uint32_t)(j >> 32), 0x68636b70u, 0x316b6365u};
    uint32_t x[16];
    for (int k = 0; k < 16; k++) x[k] = s[k];
#pragma unroll 1
    for (int round = 0; round < 10; round++) {
        PK_QR(x[0], x[4], x[8], x[12]);
        PK_QR(x[1], x[5], x[9], x[13]);
        PK_QR(x[2], x[6], x[10], x[14]);
        PK_QR(x[3], x[7], x[11], x[15]);
        PK_QR(x[0], x[5], x[10], x[15]);
        PK_QR(x[1], x[6], x[11], x[12]);
        PK_QR(x[2], x[7], x[8], x[13]);
        PK_QR(x[3], x[4], x[9], x[14]);
    }
    uint64_t lo = (uint64_t)(x[0] + s[0]) | ((uint64_t)(x[1] + s[1]) << 32), hi = (uint64_t)(x[2] + s[2]) | ((uint64_t)(x[3] + s[3]) << 32);
    if ((lo | hi) == 0) lo = 1;
    out[i] = Fe{{lo, hi, 0, 0}};
}
#undef PK_QR
int pkcheck_rho_dev(Fe* d_out, uint64_t n, uint64_t base, const uint8_t* seed32, hipStream_t s) {
    PkSeed sd;
    memcpy(sd.w, seed32, 32);
    hipLaunchKernelGGL(pkcheck_rho_kernel, dim3(ceil_div_u64(n, 256)), dim3(256), 0, s, d_out, n, base, sd);
    WS_HIP_CHECK(hipGetLastError());
    return WS_OK;
}

// ---- host: a key's shape, the seed ----
int key_vars_check(uint32_t nv, uint32_t np) {
    if (nv == 0 || (uint64_t)np + 1 > nv) { set_last_error("proving key: nPublic + 1 > nVars"); return WS_ERR_FORMAT; }
    return WS_OK;
}
int key_shape_check(const KeySections& S) {
    const uint32_t dom = S.domain;
    if (int rc = key_vars_check(S.n_vars, S.n_public)) return rc;
    if (dom < 2 || (dom & (dom - 1)) || dom > (1u << 27)) { set_last_error("proving key: domainSize must be a power of two in [2, 2^27]"); return WS_ERR_SIZE; }
    const KeyCounts c = key_counts(S);
    if (S.lenPA < c[0] * 64 || S.lenPB1 < c[1] * 64 || S.lenPB2 < c[2] * 128 || S.lenPC < c[3] * 64 || S.lenPH < c[4] * 64) {
        set_last_error("proving key: a point section is shorter than its header-implied size");
        return WS_ERR_FORMAT;
    }
    return WS_OK;
}
int draw_seed(const uint8_t* caller32, uint8_t out[32]) {
    if (caller32) memcpy(out, caller32, 32);
    else if (os_random(out, 32)) { set_last_error("no entropy: getrandom(2) and /dev/urandom both failed"); return WS_ERR_ARG; }
    return WS_OK;
}
int pk_curve_b(G1R29::El* b1, G2R29::El* b2) {
    if (b1) *b1 = Fq29::to_internal(Fq::to_mont(Fe{{3, 0, 0, 0}}));
    if (b2) {
        const PairConsts* K = nullptr;
        if (int rc = pairing_consts(&K)) return rc;
        *b2 = G2R29::El{K->b2[0], K->b2[1]};
    }
    return WS_OK;
}

// ---- host: the five fixed points and the pairings ----
namespace {
bool h_zero(const Fe& x) { return (x.l[0] | x.l[1] | x.l[2] | x.l[3]) == 0; }
bool h_reduced(const Fe& x) {
    const Fe q = Fq::modulus();
    for (int i = 3; i >= 0; i--) {
        if (x.l[i] < q.l[i]) return true;
        if (x.l[i] > q.l[i]) return false;
    }
    return false;
}
}  // namespace
// reference-format bytes -> the host pairing's point; the reason it is bad (0 = good).  check = false: only the infinity rule
uint32_t fixed_g1(const uint8_t* p, bool check, G1A* out) {
    memcpy(&out->x, p, 32);
    memcpy(&out->y, p + 32, 32);
    out->inf = h_zero(out->x);
    if (!check) return 0;
    if (out->inf) return WSNARK_PK_INFINITY;
    if (!h_reduced(out->x) || !h_reduced(out->y)) return WSNARK_PK_UNREDUCED;
    return g1_ok(*out) ? 0 : WSNARK_PK_OFF_CURVE;
}
uint32_t fixed_g2(const uint8_t* p, bool check, G2A* out) {
    memcpy(&out->x, p, 64);
    memcpy(&out->y, p + 64, 64);
    out->inf = h_zero(out->x.c0) && h_zero(out->x.c1);
    if (!check) return 0;
    if (out->inf) return WSNARK_PK_INFINITY;
    if (!h_reduced(out->x.c0) || !h_reduced(out->x.c1) || !h_reduced(out->y.c0) || !h_reduced(out->y.c1)) return WSNARK_PK_UNREDUCED;
    const F2 b2 = Fq2::mul(F2{Fq::to_mont(Fe{{3, 0, 0, 0}}), Fq::zero()}, Fq2::inv(F2{Fq::to_mont(Fe{{9, 0, 0, 0}}), Fq::one()}));
    if (!Fq2::eq(Fq2::sqr(out->y), Fq2::add(Fq2::mul(Fq2::sqr(out->x), out->x), b2))) return WSNARK_PK_OFF_CURVE;
    return g2_ok(*out) ? 0 : WSNARK_PK_OUTSIDE_SUBGROUP;
}

// the standard generators (src/bn128/build_bn128.js:59-90; wasmsnark_amd/bn128.py: G1_GEN, G2_GEN), plain integers
G1A gen1() { return G1A{Fq::one(), Fq::to_mont(Fe{{2, 0, 0, 0}}), false}; }
G2A gen2() {
    return G2A{F2{Fq::to_mont(Fe{{0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull}}),
                  Fq::to_mont(Fe{{0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull}})},
               F2{Fq::to_mont(Fe{{0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull}}),
                  Fq::to_mont(Fe{{0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull}})},
               false};
}
// e(P1, Q1) == e(P2, Q2): two Miller values, one with a negated argument, one final exponentiation
bool same_pairing(const G1A& P1, const G2A& Q1, const G1A& P2, const G2A& Q2) {
    G1A n2 = P2;
    n2.y = Fq::neg(n2.y);
    F12 m1, m2;
    if (!miller_ate(Q1, P1, &m1) || !miller_ate(Q2, n2, &m2)) return false;      // (a degenerate step: a Q not of order r)
    return f12_is_one(final_exponentiation(f12_mul(m1, m2)));
}

// the two per-point kernels alone, on points that are already on the device (pwtau.hip: the audit of a transcript's four arrays)
int pkcheck_g1_dev(Context* X, const void* d_pts, uint64_t n, uint64_t base, PkAcc* d_acc, hipStream_t s) {
    G1c::El b1;
    if (int rc = pk_curve_b(&b1, nullptr)) return rc;
    X->timer.begin("pkcheck_g1", s);
    hipLaunchKernelGGL(pkcheck_g1_kernel, dim3(ceil_div_u64(n, 256)), dim3(256), 0, s, reinterpret_cast<const G1c::AffP*>(d_pts), n, base, b1, d_acc);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    return WS_OK;
}
int pkcheck_g2_dev(Context* X, const void* d_pts, uint64_t n, uint64_t base, const PairConsts* d_K, PkAcc* d_acc, hipStream_t s) {
    G2c::El b2;
    if (int rc = pk_curve_b(nullptr, &b2)) return rc;
    const int sub_mode = tuning_get("PKCHECK_SUBGROUP", 0) == 1 ? 1 : 0;
    X->timer.begin(sub_mode ? "pkcheck_g2_psi" : "pkcheck_g2", s);
    hipLaunchKernelGGL(pkcheck_g2_kernel, dim3(ceil_div_u64(n, 64)), dim3(64), 0, s, reinterpret_cast<const G2c::AffP*>(d_pts), n, base, b2, d_K, sub_mode,
                       d_acc);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    return WS_OK;
}

int pkey_check_sections(const KeySections& S, uint32_t flags, const uint8_t* seed32, wsnark_pkey_report_t* out) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (!out || (flags & ~(uint32_t)(WSNARK_PKCHECK_POINTS | WSNARK_PKCHECK_RELATIONS))) return WS_ERR_ARG;
    if (!flags) flags = WSNARK_PKCHECK_POINTS | WSNARK_PKCHECK_RELATIONS;
    const bool do_points = (flags & WSNARK_PKCHECK_POINTS) != 0, do_rel = (flags & WSNARK_PKCHECK_RELATIONS) != 0;
    int rc = key_shape_check(S);      // what the loaders reject, with their codes
    if (rc) return rc;
    const PairConsts* K = nullptr;
    G1c::El b1;
    G2c::El b2;
    if ((rc = pairing_consts(&K)) || (rc = pk_curve_b(&b1, &b2))) return rc;
    uint8_t seed[32];
    if (do_rel && (rc = draw_seed(seed32, seed))) return rc;
    const auto t_begin = Clock::now();
    wsnark_pkey_report_t R;
    memset(&R, 0, sizeof R);
    const KeyCounts counts = key_counts(S);
    for (int k = 0; k < 5; k++) { R.points[k] = counts[k]; R.first_bad[k] = UINT64_MAX; }

    G1A alfa1, beta1, delta1;
    G2A beta2, delta2;
    R.fixed_reason[0] = fixed_g1(S.alfa1, do_points, &alfa1);
    R.fixed_reason[1] = fixed_g1(S.beta1, do_points, &beta1);
    R.fixed_reason[2] = fixed_g1(S.delta1, do_points, &delta1);
    R.fixed_reason[3] = fixed_g2(S.beta2, do_points, &beta2);
    R.fixed_reason[4] = fixed_g2(S.delta2, do_points, &delta2);

    const uint64_t chunk = key_chunk("PKCHECK_CHUNK");
    const int sub_mode = tuning_get("PKCHECK_SUBGROUP", 0) == 1 ? 1 : 0;
    const uint64_t cap = key_chunk_cap(chunk, std::max(counts[WSNARK_PK_A], counts[WSNARK_PK_H]));

    PkAcc h_acc[5];
    memset(h_acc, 0, sizeof h_acc);
    double ms_points = 0, ms_sums = 0;
    RhoSum<Fq> sum1;
    RhoSum<Fq2> sum2;
    bool sums_on = do_rel;          // off from the first chunk on in which B1 or B2 has a bad point
    {
        LaneLock L = acquire_lane(X);   // (released before the pairings: they need no lane)
        hipStream_t s = L->stream;
        DevBuf d_g1, d_g2, d_rho, d_small;
        WS_HIP_CHECK(d_g1.alloc((size_t)cap * 64));
        WS_HIP_CHECK(d_g2.alloc((size_t)cap * 128));
        if (do_rel) WS_HIP_CHECK(d_rho.alloc((size_t)cap * 32));
        const size_t o_acc = (sizeof(PairConsts) + 255) & ~(size_t)255;
        WS_HIP_CHECK(d_small.alloc(o_acc + 5 * sizeof(PkAcc)));
        WS_HIP_CHECK(hipMemcpyAsync(d_small.p, K, sizeof *K, hipMemcpyHostToDevice, s));      // (K: a static of pairing.hip, never freed)
        WS_HIP_CHECK(hipMemsetAsync(d_small.as<uint8_t>() + o_acc, 0, 5 * sizeof(PkAcc), s));
        const PairConsts* d_K = d_small.as<PairConsts>();
        PkAcc* d_acc = reinterpret_cast<PkAcc*>(d_small.as<uint8_t>() + o_acc);

        auto stage = [&](void* dst, const uint8_t* src, size_t bytes) { return stage_chunk(dst, src, bytes, s, S.release); };
        auto run_g1 = [&](int sec, uint64_t lo, uint64_t n) -> int {
            X->timer.begin("pkcheck_g1", s);
            hipLaunchKernelGGL(pkcheck_g1_kernel, dim3(ceil_div_u64(n, 256)), dim3(256), 0, s, d_g1.as<G1c::AffP>(), n, lo, b1, d_acc + sec);
            WS_HIP_CHECK(hipGetLastError());
            X->timer.end(s);
            return WS_OK;
        };
        const uint8_t* g1_src[5] = {S.A, S.B1, nullptr, S.Cpts, S.H};
        const int order[4] = {WSNARK_PK_A, WSNARK_PK_B1, WSNARK_PK_C, WSNARK_PK_H};
        for (int sec : order) {
            const bool pair = sec == WSNARK_PK_B1;      // B1 and B2 go side by side
            if (!do_points && !pair) continue;
            for (uint64_t lo = 0; lo < counts[sec]; lo += chunk) {
                const uint64_t n = std::min<uint64_t>(chunk, counts[sec] - lo);
                auto t0 = Clock::now();
                if ((rc = stage(d_g1.p, g1_src[sec] + lo * 64, (size_t)n * 64))) return rc;
                if (do_points && (rc = run_g1(sec, lo, n))) return rc;
                if (pair) {
                    if ((rc = stage(d_g2.p, S.B2 + lo * 128, (size_t)n * 128))) return rc;
                    if (do_points) {
                        X->timer.begin(sub_mode ? "pkcheck_g2_psi" : "pkcheck_g2", s);
                        hipLaunchKernelGGL(pkcheck_g2_kernel, dim3(ceil_div_u64(n, 64)), dim3(64), 0, s, d_g2.as<G2c::AffP>(), n, lo, b2, d_K, sub_mode,
                                           d_acc + WSNARK_PK_B2);
                        WS_HIP_CHECK(hipGetLastError());
                        X->timer.end(s);
                    }
                    if (do_points && sums_on) {      // the sums only ever see points that passed
                        WS_HIP_CHECK(hipMemcpyAsync(h_acc, d_acc, sizeof h_acc, hipMemcpyDeviceToHost, s));
                        WS_HIP_CHECK(hipStreamSynchronize(s));
                        if (h_acc[WSNARK_PK_B1].bad || h_acc[WSNARK_PK_B2].bad) sums_on = false;
                    }
                }
                if (pair && sums_on) {
                    WS_HIP_CHECK(hipStreamSynchronize(s));
                    ms_points += ms_since(t0);
                    t0 = Clock::now();
                    if ((rc = pkcheck_rho_dev(d_rho.as<Fe>(), n, lo, seed, s))) return rc;
                    if ((rc = sum1.add(*L, d_rho.as<Fe>(), d_g1.as<Affine<Fq>>(), n, s))) return rc;
                    if ((rc = sum2.add(*L, d_rho.as<Fe>(), d_g2.as<Affine<Fq2>>(), n, s))) return rc;
                    ms_sums += ms_since(t0);
                } else {
                    ms_points += ms_since(t0);      // (the kernels of this chunk are still running: the next lap, or the drain below, has them)
                }
            }
        }
        {
            const auto t0 = Clock::now();
            WS_HIP_CHECK(hipMemcpyAsync(h_acc, d_acc, sizeof h_acc, hipMemcpyDeviceToHost, s));
            WS_HIP_CHECK(hipStreamSynchronize(s));
            ms_points += ms_since(t0);
        }
    }
    for (int k = 0; k < 5; k++) pk_decode(h_acc[k], &R.infinity[k], &R.bad[k], &R.first_bad[k], &R.first_reason[k]);

    const auto t_pair = Clock::now();
    if (do_rel) {
        if (!R.fixed_reason[1] && !R.fixed_reason[3]) {
            R.relations_run |= 1;
            if (!same_log(beta1, beta2)) R.relations_bad |= 1;
        }
        if (!R.fixed_reason[2] && !R.fixed_reason[4]) {
            R.relations_run |= 2;
            if (!same_log(delta1, delta2)) R.relations_bad |= 2;
        }
        if (sums_on && !R.bad[WSNARK_PK_B1] && !R.bad[WSNARK_PK_B2]) {
            R.relations_run |= 4;
            if (!same_log(sum1.finish(), sum2.finish())) R.relations_bad |= 4;
        }
    }
    R.ms[0] = ms_points;
    R.ms[1] = ms_sums;
    R.ms[2] = ms_since(t_pair);
    bool ok = R.relations_bad == 0 && (!do_rel || R.relations_run == 7);
    for (int k = 0; k < 5; k++) ok = ok && R.bad[k] == 0 && R.fixed_reason[k] == 0;
    R.ok = ok ? 1 : 0;
    R.ms[3] = ms_since(t_begin);
    *out = R;
    return WS_OK;
}

}  // namespace wsnark
