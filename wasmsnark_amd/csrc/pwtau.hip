// pwtau.hip -- powers of tau: a contribution to a phase-1 transcript and the transcript's audit (wsnark_powers_contribute,
// wsnark_powers_check, wsnark_g{1,2}_mul_batch; include/wsnark.h), the steps before wsnark_pkey_setup (pkeysetup.hip).
//
// A transcript holds tau^k G1 (k < 2n), tau^k G2, alpha tau^k G1, beta tau^k G1 (k < n) and beta G2.  A contribution by (t, a, b)
// multiplies power k by t^k (and by a, b): point i times scalar i, the third shape beside mul_base_kernel (one base, a scalar per
// lane) and scale_points_kernel (a base per lane, ONE scalar, its digits in the argument block).
//
//   mul_points_kernel<C>: one lane per point (reference format in and out), the scalar from memory, reduced mod r by the lane.
//     Input tests, counts and the copy-through of infinity are scale_points_kernel's (keybytes.h: pk_classify, pk_reduce); the
//     result leaves affine behind the shared per-workgroup inversion (keybytes.h: block_inverse, affine_result).
//     Fixed signed windows: the scalar is cut into 64 windows of 4 bits, digits in [-8, 8] (a window value above
//       8 becomes value - 16 and carries into the next window; k < r < 2^254 leaves at most 3 in the top window, bits 252..255, so
//       the carry INTO it is absorbed there and nothing leaves it).  The lane first writes the table 1P .. 8P of ITS point (one
//       affine doubling, six mixed additions; XYZZ, not normalised) to a global scratch array laid out [entry][lane], then walks
//       the windows from the top: four doublings, one full addition C::add of entry |digit| (y negated for a negative digit).
//       Every lane adds at the same 64 steps -- uniform control flow, only the table row differs -- and a zero digit (1 in 16)
//       adds nothing.  Products per finite G1 point, counted from curve.h's formulas as pkeydelta.hip counts (squarings as
//       products, the fused Y3 as two): input tests 2 + 3, table 7 + 6 x 11, chain 252 x 9 (dbl) + ~60 x 14 (add), the shared
//       inversion 24 + 363 / 4 (one wavefront of four inverts), normalisation 5, output 2: ~3290 (tools/pwtau_bench.py counts it over
//       the scalars of its run) -- the count of ONE lane of a per-lane NAF chain (~3330), without the divergence that makes a
//       wavefront of 64 unrelated digit strings pay ~5200 there (docs/HISTORY.md has that chain measured).
//       The table is 8 x 128 B per G1 lane, 8 x 256 B per G2 lane: in LDS that is 256 KiB for a 256-lane workgroup against the CU's
//       160 KiB, and a runtime-indexed per-thread array would be scratch with nothing coalesced; [entry][lane] in global memory
//       makes a wavefront's load of one row a run of neighbouring 128-byte records per distinct digit.  A lane reads ~60 x 128 B
//       against ~3200 products of ~500 instructions: the loads hide behind the doublings that precede each addition.
//     Every addition is the guarded one (C::madd building the table, C::add in the chain): the chain passes through +/- P for
//     scalars next to r, and a G2 point outside the order-r subgroup -- legal input here -- makes table entries collide or vanish
//     (an entry at infinity is stored with ZZ = 0 and C::add takes it as such).
//   fr_powers_kernel: out[i] = c t^(first + i), plain, from the t^(2^j) in the argument block (as group_twiddle_kernel builds its
//     twiddles); `first` is the GLOBAL index of the chunk's first power, so the scalars do not depend on the chunking.
//   streaming: an array goes through the staging ring in chunks of PWTAU_CHUNK points (default 2^18): up, scalars, kernel, down.
//     Device memory: (2 x 128 + 32) B x chunk, plus the window table (2 KiB x chunk), whatever the transcript's size.
//
//   wsnark_powers_check: the point tests are the key audit's own kernels (pkeycheck.hip: pkcheck_g1_dev, pkcheck_g2_dev -- the
//     latter with the order-r subgroup test, for tau_g2); the relations are random-combination sums with the audit's rho (ChaCha20,
//     the global index) over ONE array at offsets k and k + 1: a chunk of m terms stages m + 1 points and sums the same rho against
//     d_pts and d_pts + 1 by the ordinary MSMs (keybytes.h: RhoSum); the power at a chunk boundary is the k + 1 of one chunk's last
//     term and the k of the next chunk's first.  Two host Miller loops per relation (same_pairing).
#include <string.h>

#include "fp12.h"
#include "keybytes.h"

namespace wsnark {

using namespace hostpair;

// ---- device ----
constexpr int PW_WIN = 4;                       // window width
constexpr int PW_TAB = 1 << (PW_WIN - 1);       // table entries: 1P .. 8P
constexpr int PW_NWIN = 256 / PW_WIN;           // windows over the 256 bits of a scalar word string
static_assert((FrParams::P3 >> 60) + 1 <= (uint64_t)PW_TAB, "the top window of a scalar below r must absorb the carry into it");

// window j of k with the carry into it: the signed digit's magnitude (0 .. 8) and sign
__device__ __forceinline__ void pw_digit(const Fe& k, uint64_t carries, int j, unsigned* mag, bool* neg) {
    const uint64_t word = word4(k.l[0], k.l[1], k.l[2], k.l[3], j >> 4);
    const unsigned v = (unsigned)((word >> ((j & 15) * PW_WIN)) & 15) + (unsigned)((carries >> j) & 1);
    *neg = v > (unsigned)PW_TAB;
    *mag = v > (unsigned)PW_TAB ? 16 - v : v;
}

template <class C>
__global__ __launch_bounds__(256) void mul_points_kernel(const typename C::AffP* __restrict__ pts, const Fe* __restrict__ scalars, uint64_t n,
                                                           uint64_t base, typename C::El curve_b, typename C::AffP* __restrict__ out,
                                                           typename C::PtP* __restrict__ table, uint64_t lanes, PkAcc* __restrict__ acc) {
    typedef typename C::Field F;
    typedef typename C::El El;
    typedef typename C::Pt Pt;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int st = 0;               // pk_reduce's states: 0 good, 1 unreduced, 2 off the curve, 4 infinity
    bool live = false;        // a good finite point and a scalar that is not 0 mod r: this lane runs the chain
    typename C::Aff P = typename C::Aff{F::zero(), F::zero()};
    Fe k = Fe{{0, 0, 0, 0}};
    if (i < n) {
        st = pk_classify<C>(pts[i], curve_b, &P);
        k = Fr::reduce_full(scalars[i]);
        live = st == 0 && (k.l[0] | k.l[1] | k.l[2] | k.l[3]) != 0;
    }
    pk_reduce(st, base + i, acc);

    Pt a = C::infinity();
    if (live) {
        // bit j of `carries`: the carry INTO window j (none leaves window 63: the static_assert above)
        uint64_t carries = 0;
        unsigned c = 0;
#pragma unroll 1
        for (int j = 0; j < PW_NWIN - 1; j++) {
            const uint64_t word = word4(k.l[0], k.l[1], k.l[2], k.l[3], j >> 4);
            c = ((unsigned)((word >> ((j & 15) * PW_WIN)) & 15) + c) > (unsigned)PW_TAB ? 1u : 0u;
            carries |= (uint64_t)c << (j + 1);
        }
        // the table e P, e = 1 .. 8, row e - 1 of [entry][lane]; guarded additions: 2P = -P (order 3) and its like are legal on G2
        Pt T = Pt{P.x, P.y, F::one(), F::one()};
        table[i] = C::pack_pt(T);
        T = C::dbl_affine(P.x, P.y);
        table[lanes + i] = C::pack_pt(T);
#pragma unroll 1
        for (int e = 2; e < PW_TAB; e++) {
            C::madd(T, P, false);
            table[(uint64_t)e * lanes + i] = C::pack_pt(T);
        }
        // the windows from the top: the first one meets a == infinity and needs no doubling
#pragma unroll 1
        for (int j = PW_NWIN - 1; j >= 0; j--) {
            unsigned mag;
            bool neg;
            pw_digit(k, carries, j, &mag, &neg);
            if (j != PW_NWIN - 1) {
                a = C::dbl(a);
                a = C::dbl(a);
                a = C::dbl(a);
                a = C::dbl(a);
            }
            if (mag != 0) {      // (a zero window adds nothing)
                Pt E = C::unpack_pt(table[(uint64_t)(mag - 1) * lanes + i]);
                E.y = F::cneg(E.y, neg);
                a = C::add(a, E);
            }
        }
    }
    const bool fin = live && !C::is_inf(a);

    // one inversion per workgroup (blockDim.x == 256): every lane arrives, a lane with nothing to normalise passes 1
    const El inv = block_inverse<F>(fin ? F::mul(a.zz, a.zzz) : F::one());
    if (i < n) out[i] = st == 4 ? pts[i] : affine_result<C>(a, fin, inv, 1);      // infinity: copied through byte for byte
}

// out[i] = c t^(first + i), plain: the lane multiplies the t^(2^j) of the set bits of its GLOBAL index (< 2^25: tau_g1 has 2n <= 2^25 powers)
struct PowerBase { Fe p[25]; Fe c; };      // Montgomery
__global__ __launch_bounds__(256) void fr_powers_kernel(PowerBase W, uint64_t first, uint64_t count, Fe* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint64_t e = first + i;
    Fe acc = W.c;
    for (int j = 0; j < 25; j++)
        if ((e >> j) & 1) acc = Fr::mul(acc, W.p[j]);
    out[i] = Fr::from_mont(acc);
}

// ---- host ----
namespace {
// what a chunk in flight needs on the device; the scalars are overwritten when this goes (every exit path of a contribution)
struct MulBufs {
    hipStream_t s = nullptr;
    DevBuf d_pts, d_out, d_sc, d_tab;
    uint64_t cap = 0;
    bool secret = false;
    // cap points of at most point_bytes each, and the window table: 8 XYZZ points per lane
    int init(hipStream_t s_, uint64_t cap_, size_t point_bytes, bool secret_) {
        s = s_; cap = cap_; secret = secret_;
        WS_HIP_CHECK(d_pts.alloc((size_t)cap * point_bytes));
        WS_HIP_CHECK(d_out.alloc((size_t)cap * point_bytes));
        WS_HIP_CHECK(d_sc.alloc((size_t)cap * 32));
        WS_HIP_CHECK(d_tab.alloc((size_t)cap * PW_TAB * 2 * point_bytes));
        return WS_OK;
    }
    ~MulBufs() {
        if (!s) return;
        if (secret && d_sc.p) (void)hipMemsetAsync(d_sc.p, 0, (size_t)cap * 32, s);
        (void)hipStreamSynchronize(s);      // (also the error paths: nothing may still read or write the buffers)
    }
};

// d_out[i] = d_sc[i] x d_pts[i], i < m; counts into d_acc under the global index base + i
template <class C>
int mul_launch(Context* X, MulBufs& B, uint64_t m, uint64_t base, PkAcc* d_acc) {
    typedef typename C::AffP AffP;
    typedef typename C::PtP PtP;
    typename C::El cb;
    const int rc = curve_b(&cb);
    if (rc) return rc;
    X->timer.begin(sizeof(AffP) == 64 ? "mul_points_g1_win" : "mul_points_g2_win", B.s);
    hipLaunchKernelGGL(mul_points_kernel<C>, dim3(ceil_div_u64(m, 256)), dim3(256), 0, B.s, B.d_pts.as<AffP>(), B.d_sc.as<Fe>(), m, base, cb,
                       B.d_out.as<AffP>(), B.d_tab.as<PtP>(), B.cap, d_acc);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(B.s);
    return WS_OK;
}

template <class C>
int mul_batch(const void* points, const void* scalars, uint64_t n, void* out) {
    typedef typename C::AffP AffP;
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (n == 0) return WS_OK;
    if (!points || !scalars || !out) return WS_ERR_ARG;
    if (n > ((uint64_t)1 << 24)) { set_last_error("mul_batch: n > 2^24"); return WS_ERR_SIZE; }
    const size_t psz = sizeof(AffP);
    const uint64_t chunk = key_chunk("PWTAU_CHUNK");
    // out stays untouched behind a bad point: one chunk is tested before it comes down; several come down into a host copy first
    std::vector<uint8_t> held;
    if (n > chunk) held.resize((size_t)n * psz);
    uint8_t* dst = n > chunk ? held.data() : (uint8_t*)out;
    PkAcc h_acc;
    memset(&h_acc, 0, sizeof h_acc);
    {
        int rc;
        LaneLock L = acquire_lane(X);
        hipStream_t s = L->stream;
        DevBuf d_acc;
        WS_HIP_CHECK(d_acc.alloc(sizeof(PkAcc)));
        WS_HIP_CHECK(hipMemsetAsync(d_acc.p, 0, sizeof(PkAcc), s));
        MulBufs B;
        if ((rc = B.init(s, key_chunk_cap(chunk, n), psz, false))) return rc;
        for (uint64_t lo = 0; lo < n; lo += chunk) {
            const uint64_t m = std::min<uint64_t>(chunk, n - lo);
            if ((rc = stage_chunk(B.d_pts.p, (const uint8_t*)points + lo * psz, (size_t)m * psz, s, nullptr))) return rc;
            if ((rc = stage_chunk(B.d_sc.p, (const uint8_t*)scalars + lo * 32, (size_t)m * 32, s, nullptr))) return rc;
            if ((rc = mul_launch<C>(X, B, m, lo, d_acc.as<PkAcc>()))) return rc;
            WS_HIP_CHECK(hipMemcpyAsync(&h_acc, d_acc.p, sizeof h_acc, hipMemcpyDeviceToHost, s));
            WS_HIP_CHECK(hipStreamSynchronize(s));
            if (h_acc.bad) continue;      // (the later chunks are still counted: the message names the first index and the count)
            WS_HIP_CHECK(hipMemcpyAsync(dst + lo * psz, B.d_out.p, (size_t)m * psz, hipMemcpyDeviceToHost, s));
            WS_HIP_CHECK(hipStreamSynchronize(s));
        }
    }
    uint64_t inf, bad, first;
    uint32_t reason;
    pk_decode(h_acc, &inf, &bad, &first, &reason);
    if (bad) {
        set_last_error("mul_batch: " + std::to_string(bad) + " point(s) unreduced or off the curve, the first at index " + std::to_string(first));
        return WS_ERR_FORMAT;
    }
    if (n > chunk) memcpy(out, held.data(), held.size());
    return WS_OK;
}

// ---- a transcript's shape ----
struct PwArray { const uint8_t* src; uint64_t count; size_t psz; };
// what every consumer of a transcript rejects, with wsnark_pkey_setup's codes, in its order
int powers_shape_check(const wsnark_powers_t* P, const char* who) {
    if (!P || !P->tau_g1 || !P->tau_g2 || !P->alpha_tau_g1 || !P->beta_tau_g1 || !P->beta_g2) return WS_ERR_ARG;
    const uint64_t n = P->domain;
    if (n < 2 || (n & (n - 1)) || n > ((uint64_t)1 << 24)) { set_last_error(std::string(who) + ": domain must be a power of two in [2, 2^24]"); return WS_ERR_SIZE; }
    if (P->tau_g1_len < 2 * n * 64 || P->tau_g2_len < n * 128 || P->alpha_tau_g1_len < n * 64 || P->beta_tau_g1_len < n * 64) {
        set_last_error(std::string(who) + ": an array of powers is shorter than the domain implies (tau_g1: 2n, the others: n)");
        return WS_ERR_FORMAT;
    }
    return WS_OK;
}
// the four arrays in report order (WSNARK_PW_TAU_G1 ..)
void powers_arrays(const wsnark_powers_t* P, PwArray A[4]) {
    const uint64_t n = P->domain;
    A[WSNARK_PW_TAU_G1] = PwArray{(const uint8_t*)P->tau_g1, 2 * n, 64};
    A[WSNARK_PW_TAU_G2] = PwArray{(const uint8_t*)P->tau_g2, n, 128};
    A[WSNARK_PW_ALPHA_TAU_G1] = PwArray{(const uint8_t*)P->alpha_tau_g1, n, 64};
    A[WSNARK_PW_BETA_TAU_G1] = PwArray{(const uint8_t*)P->beta_tau_g1, n, 64};
}

// the secrets of one contribution and the table t^(2^j); wiped when it goes
struct PwSecret {
    Fe t, a, b;          // plain, reduced
    Fe coef[4];          // the constant of each array in report order: 1, 1, a, b (Montgomery)
    PowerBase W;         // Montgomery; c is set per array
    ~PwSecret() { wipe(this, sizeof *this); }
};
int draw_secret(const uint8_t* caller32, const char* name, Fe* out) {
    uint8_t raw[32];
    int rc = draw_seed(caller32, raw);
    if (rc) return rc;
    *out = load_scalar(raw);
    wipe(raw, sizeof raw);
    if (Fr::is_zero(*out)) { set_last_error(std::string("powers contribution: ") + name + " = 0 mod r"); return WS_ERR_ARG; }
    return WS_OK;
}
}  // namespace

// ---- the same two kernels on device-resident arrays (zkey.hip: the twist of the H basis change) ----
int fr_powers_dev(Context* X, const Fe& c_mont, const Fe& t_mont, uint64_t first, uint64_t count, Fe* d_out, hipStream_t s) {
    if (!count) return WS_OK;
    PowerBase W;
    W.c = c_mont;
    W.p[0] = t_mont;
    for (int j = 1; j < 25; j++) W.p[j] = Fr::sqr(W.p[j - 1]);
    X->timer.begin("fr_powers", s);
    hipLaunchKernelGGL(fr_powers_kernel, dim3(ceil_div_u64(count, 256)), dim3(256), 0, s, W, first, count, d_out);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    return WS_OK;
}
int g1_mul_dev(Context* X, const void* d_pts, const Fe* d_scalars, uint64_t n, void* d_out, PkAcc* d_acc, hipStream_t s) {
    typedef G1R29 C;
    if (!n) return WS_OK;
    C::El cb;
    int rc = curve_b(&cb);
    if (rc) return rc;
    // PWTAU_CHUNK points per launch: the table of the windowed chain is sized by the chunk, not by the array
    const uint64_t chunk = key_chunk("PWTAU_CHUNK"), cap = key_chunk_cap(chunk, n);
    DevBuf d_tab;
    WS_HIP_CHECK(d_tab.alloc((size_t)cap * PW_TAB * sizeof(C::PtP)));
    const C::AffP* in = (const C::AffP*)d_pts;
    C::AffP* out = (C::AffP*)d_out;
    for (uint64_t lo = 0; lo < n; lo += chunk) {
        const uint64_t m = std::min<uint64_t>(chunk, n - lo);
        X->timer.begin("mul_points_g1_win", s);
        hipLaunchKernelGGL(mul_points_kernel<C>, dim3(ceil_div_u64(m, 256)), dim3(256), 0, s, in + lo, d_scalars + lo, m, lo, cb, out + lo,
                           d_tab.as<C::PtP>(), cap, d_acc);
        WS_HIP_CHECK(hipGetLastError());
        X->timer.end(s);
    }
    WS_HIP_CHECK(hipStreamSynchronize(s));      // (the table goes with this call)
    return WS_OK;
}

int g1_mul_batch(const void* points, const void* scalars, uint64_t n, void* out) { return mul_batch<G1R29>(points, scalars, n, out); }
int g2_mul_batch(const void* points, const void* scalars, uint64_t n, void* out) { return mul_batch<G2R29>(points, scalars, n, out); }

int powers_contribute(const wsnark_powers_t* P, const uint8_t* tau32, const uint8_t* alpha32, const uint8_t* beta32, uint8_t* const out[5],
                      wsnark_powers_report_t* rep) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (!rep || !out[0] || !out[1] || !out[2] || !out[3] || !out[4]) return WS_ERR_ARG;
    int rc;
    if ((rc = powers_shape_check(P, "powers contribution"))) return rc;
    PwSecret K;
    if ((rc = draw_secret(tau32, "tau", &K.t)) || (rc = draw_secret(alpha32, "alpha", &K.a)) || (rc = draw_secret(beta32, "beta", &K.b))) return rc;
    K.W.p[0] = Fr::to_mont(K.t);
    for (int j = 1; j < 25; j++) K.W.p[j] = Fr::sqr(K.W.p[j - 1]);
    K.coef[WSNARK_PW_TAU_G1] = K.coef[WSNARK_PW_TAU_G2] = Fr::one();
    K.coef[WSNARK_PW_ALPHA_TAU_G1] = Fr::to_mont(K.a);
    K.coef[WSNARK_PW_BETA_TAU_G1] = Fr::to_mont(K.b);

    const auto t_begin = Clock::now();
    wsnark_powers_report_t R;
    memset(&R, 0, sizeof R);
    PwArray A[4];
    powers_arrays(P, A);
    for (int a = 0; a < 4; a++) { R.points[a] = A[a].count; R.first_bad[a] = UINT64_MAX; }

    // beta_g2' = b beta_g2: the host curve of proof assembly
    auto t0 = Clock::now();
    G2A b2;
    R.beta2_reason = fixed_g2((const uint8_t*)P->beta_g2, true, &b2);
    if (!R.beta2_reason) {
        G2::Pt p2 = G2::mul_bytes(G2::Pt{b2.x, b2.y, Fq2::one(), Fq2::one()}, reinterpret_cast<const uint8_t*>(&K.b), 32);
        const Jac<Fq2> j2 = G2::to_affine_jac(p2);      // (b != 0 mod r and the point has order r: never infinity)
        memcpy(out[4], &j2, 128);
        wipe(&p2, sizeof p2);
    }
    const double ms_host = ms_since(t0);
    double ms_dev = 0;

    PkAcc h_acc[4];
    memset(h_acc, 0, sizeof h_acc);
    if (!R.beta2_reason) {
        t0 = Clock::now();
        const uint64_t chunk = key_chunk("PWTAU_CHUNK");
        LaneLock L = acquire_lane(X);
        hipStream_t s = L->stream;
        DevBuf d_acc;
        WS_HIP_CHECK(d_acc.alloc(sizeof h_acc));
        WS_HIP_CHECK(hipMemsetAsync(d_acc.p, 0, sizeof h_acc, s));
        MulBufs B;
        if ((rc = B.init(s, key_chunk_cap(chunk, A[WSNARK_PW_TAU_G1].count), 128, true))) return rc;
        for (int a = 0; a < 4; a++) {
            K.W.c = K.coef[a];
            for (uint64_t lo = 0; lo < A[a].count; lo += chunk) {
                const uint64_t m = std::min<uint64_t>(chunk, A[a].count - lo);
                // (in place: the chunk has left the caller's buffer before its result comes back to it)
                if ((rc = stage_chunk(B.d_pts.p, A[a].src + lo * A[a].psz, (size_t)m * A[a].psz, s, nullptr))) return rc;
                X->timer.begin("fr_powers", s);
                hipLaunchKernelGGL(fr_powers_kernel, dim3(ceil_div_u64(m, 256)), dim3(256), 0, s, K.W, lo, m, B.d_sc.as<Fe>());
                WS_HIP_CHECK(hipGetLastError());
                X->timer.end(s);
                if (A[a].psz == 64) rc = mul_launch<G1R29>(X, B, m, lo, d_acc.as<PkAcc>() + a);
                else rc = mul_launch<G2R29>(X, B, m, lo, d_acc.as<PkAcc>() + a);
                if (rc) return rc;
                WS_HIP_CHECK(hipMemcpyAsync(out[a] + lo * A[a].psz, B.d_out.p, (size_t)m * A[a].psz, hipMemcpyDeviceToHost, s));
                WS_HIP_CHECK(hipStreamSynchronize(s));
            }
        }
        WS_HIP_CHECK(hipMemcpyAsync(h_acc, d_acc.p, sizeof h_acc, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));
        ms_dev = ms_since(t0);
    }
    bool ok = R.beta2_reason == 0;
    for (int a = 0; a < 4; a++) {
        pk_decode(h_acc[a], &R.infinity[a], &R.bad[a], &R.first_bad[a], &R.first_reason[a]);
        ok = ok && R.bad[a] == 0 && R.infinity[a] == 0;
    }
    R.ok = ok ? 1 : 0;
    R.ms[0] = ms_dev;
    R.ms[1] = ms_host;
    R.ms[3] = ms_since(t_begin);
    *rep = R;
    return WS_OK;
}

int powers_check(const wsnark_powers_t* P, uint32_t flags, const uint8_t* seed32, wsnark_powers_report_t* rep) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (!rep || (flags & ~(uint32_t)(WSNARK_PWCHECK_POINTS | WSNARK_PWCHECK_RELATIONS))) return WS_ERR_ARG;
    if (!flags) flags = WSNARK_PWCHECK_POINTS | WSNARK_PWCHECK_RELATIONS;
    const bool do_points = (flags & WSNARK_PWCHECK_POINTS) != 0, do_rel = (flags & WSNARK_PWCHECK_RELATIONS) != 0;
    int rc;
    if ((rc = powers_shape_check(P, "powers audit"))) return rc;
    const PairConsts* K = nullptr;
    if ((rc = pairing_consts(&K))) return rc;
    uint8_t seed[32];
    if (do_rel && (rc = draw_seed(seed32, seed))) return rc;
    const auto t_begin = Clock::now();
    wsnark_powers_report_t R;
    memset(&R, 0, sizeof R);
    PwArray A[4];
    powers_arrays(P, A);
    for (int a = 0; a < 4; a++) { R.points[a] = A[a].count; R.first_bad[a] = UINT64_MAX; }

    // the points the relations name one by one: T2 = tau_g2[1], tau_g1[1], beta_tau_g1[0], beta_g2 (the host's fixed-point tests)
    G1A tau1, beta1;
    G2A T2, beta2;
    R.beta2_reason = fixed_g2((const uint8_t*)P->beta_g2, do_points, &beta2);
    const bool T2_ok = fixed_g2(A[WSNARK_PW_TAU_G2].src + 128, do_points, &T2) == 0;
    const bool tau1_ok = fixed_g1(A[WSNARK_PW_TAU_G1].src + 64, do_points, &tau1) == 0;
    const bool beta1_ok = fixed_g1(A[WSNARK_PW_BETA_TAU_G1].src, do_points, &beta1) == 0;

    // sums_on[a]: the two sums of array a are worth taking -- off from the first chunk on in which the array has a bad point
    bool sums_on[4] = {do_rel && T2_ok, do_rel && tau1_ok, do_rel && T2_ok, do_rel && T2_ok};
    RhoSum<Fq> lo1[4], hi1[4];      // sum rho_k P[k], sum rho_k P[k + 1]
    RhoSum<Fq2> lo2, hi2;
    PkAcc h_acc[4];
    memset(h_acc, 0, sizeof h_acc);
    double ms_points = 0, ms_sums = 0;
    {
        const uint64_t chunk = key_chunk("PWTAU_CHUNK");
        const uint64_t cap = key_chunk_cap(chunk, A[WSNARK_PW_TAU_G1].count);
        LaneLock L = acquire_lane(X);      // (released before the pairings: they need no lane)
        hipStream_t s = L->stream;
        DevBuf d_pts, d_rho, d_small;
        WS_HIP_CHECK(d_pts.alloc((size_t)(cap + 1) * 128));      // a chunk reads one point beyond its end
        if (do_rel) WS_HIP_CHECK(d_rho.alloc((size_t)cap * 32));
        const size_t o_acc = (sizeof(PairConsts) + 255) & ~(size_t)255;
        WS_HIP_CHECK(d_small.alloc(o_acc + sizeof h_acc));
        WS_HIP_CHECK(hipMemcpyAsync(d_small.p, K, sizeof *K, hipMemcpyHostToDevice, s));      // (K: a static of pairing.hip, never freed)
        WS_HIP_CHECK(hipMemsetAsync(d_small.as<uint8_t>() + o_acc, 0, sizeof h_acc, s));
        PkAcc* d_acc = reinterpret_cast<PkAcc*>(d_small.as<uint8_t>() + o_acc);
        for (int a = 0; a < 4; a++) {
            const bool g2 = A[a].psz == 128;
            const uint64_t N = A[a].count;
            for (uint64_t lo = 0; lo < N; lo += chunk) {
                if (!do_points && !sums_on[a]) break;
                const uint64_t m = std::min<uint64_t>(chunk, N - lo);      // points [lo, lo + m) are this chunk's to test
                const uint64_t ext = std::min<uint64_t>(m + 1, N - lo);    // ... and [lo, lo + ext) are staged: terms k = lo .. lo + ext - 2
                auto t0 = Clock::now();
                if ((rc = stage_chunk(d_pts.p, A[a].src + lo * A[a].psz, (size_t)ext * A[a].psz, s, nullptr))) return rc;
                if (do_points) {
                    if (g2) rc = pkcheck_g2_dev(X, d_pts.p, m, lo, d_small.as<PairConsts>(), d_acc + a, s);
                    else rc = pkcheck_g1_dev(X, d_pts.p, m, lo, d_acc + a, s);
                    if (rc) return rc;
                    if (sums_on[a]) {      // the sums only ever see points that passed
                        WS_HIP_CHECK(hipMemcpyAsync(h_acc, d_acc, sizeof h_acc, hipMemcpyDeviceToHost, s));
                        WS_HIP_CHECK(hipStreamSynchronize(s));
                        if (h_acc[a].bad || h_acc[a].inf) sums_on[a] = false;
                    }
                }
                WS_HIP_CHECK(hipStreamSynchronize(s));
                ms_points += ms_since(t0);
                const uint64_t terms = ext - 1;
                if (sums_on[a] && terms) {
                    t0 = Clock::now();
                    if ((rc = pkcheck_rho_dev(d_rho.as<Fe>(), terms, lo, seed, s))) return rc;      // the SAME rho_k against P[k] and P[k + 1]
                    if (g2) {
                        if ((rc = lo2.add(*L, d_rho.as<Fe>(), d_pts.as<Affine<Fq2>>(), terms, s))) return rc;
                        if ((rc = hi2.add(*L, d_rho.as<Fe>(), d_pts.as<Affine<Fq2>>() + 1, terms, s))) return rc;
                    } else {
                        if ((rc = lo1[a].add(*L, d_rho.as<Fe>(), d_pts.as<Affine<Fq>>(), terms, s))) return rc;
                        if ((rc = hi1[a].add(*L, d_rho.as<Fe>(), d_pts.as<Affine<Fq>>() + 1, terms, s))) return rc;
                    }
                    WS_HIP_CHECK(hipStreamSynchronize(s));
                    ms_sums += ms_since(t0);
                }
            }
        }
        const auto t0 = Clock::now();
        WS_HIP_CHECK(hipMemcpyAsync(h_acc, d_acc, sizeof h_acc, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));
        ms_points += ms_since(t0);
    }
    bool array_ok[4];
    for (int a = 0; a < 4; a++) {
        pk_decode(h_acc[a], &R.infinity[a], &R.bad[a], &R.first_bad[a], &R.first_reason[a]);
        array_ok[a] = R.bad[a] == 0 && R.infinity[a] == 0;
    }

    const auto t_pair = Clock::now();
    if (do_rel) {
        const G1A g1 = gen1();
        const G2A g2 = gen2();
        R.relations_run |= 1;
        if (memcmp(A[WSNARK_PW_TAU_G1].src, &g1.x, 64) != 0 || memcmp(A[WSNARK_PW_TAU_G2].src, &g2.x, 128) != 0) R.relations_bad |= 1;
        const int g1_bits[3][2] = {{WSNARK_PW_TAU_G1, 1}, {WSNARK_PW_ALPHA_TAU_G1, 3}, {WSNARK_PW_BETA_TAU_G1, 4}};
        for (const auto& ab : g1_bits) {      // e(sum rho_k P[k + 1], G2) = e(sum rho_k P[k], T2)
            const int a = ab[0];
            if (!sums_on[a] || !array_ok[a]) continue;
            R.relations_run |= 1u << ab[1];
            if (!same_pairing(hi1[a].finish(), g2, lo1[a].finish(), T2)) R.relations_bad |= 1u << ab[1];
        }
        if (sums_on[WSNARK_PW_TAU_G2] && array_ok[WSNARK_PW_TAU_G2]) {      // e(tau_g1[1], sum rho_k Q[k]) = e(G1, sum rho_k Q[k + 1])
            R.relations_run |= 4;
            if (!same_pairing(tau1, lo2.finish(), g1, hi2.finish())) R.relations_bad |= 4;
        }
        if (beta1_ok && !R.beta2_reason) {
            R.relations_run |= 32;
            if (!same_log(beta1, beta2)) R.relations_bad |= 32;
        }
        wipe(seed, sizeof seed);
    }
    R.ms[0] = ms_points;
    R.ms[1] = ms_sums;
    R.ms[2] = ms_since(t_pair);
    bool ok = R.relations_bad == 0 && (!do_rel || R.relations_run == 63) && R.beta2_reason == 0;
    for (int a = 0; a < 4; a++) ok = ok && array_ok[a];
    R.ok = ok ? 1 : 0;
    R.ms[3] = ms_since(t_begin);
    *rep = R;
    return WS_OK;
}

}  // namespace wsnark
