// pkeysetup.hip -- the first key of a ceremony from a powers-of-tau transcript: the transform over GROUP elements
// (wsnark_g{1,2}_ntt) and the key of a circuit under delta = gamma = 1 (wsnark_pkey_setup*; include/wsnark.h), the key
// wsnark_pkey_contribute (pkeydelta.hip) is then applied to.
//
// A key's points are the circuit's columns evaluated "in the exponent" on the Lagrange basis, and
//     L_i(tau) G = (1/n) sum_k w_n^(-ik) (tau^k G)
// is the inverse transform of the powers with points where ntt.hip has field elements.  The reference has no counterpart (its FFT is
// built over frm only, src/bn128/build_bn128.js:37).  A butterfly costs one 254-bit scalar multiplication: the workload of
// scale_points_kernel (pkeydelta.hip), n/2 log2 n of them per transform.
//
//   group_load_kernel<C>: one lane per input point.  The audit's two cheap tests (keybytes.h: pk_classify; counts and the first bad
//     index through pk_reduce), the change to the field's internal form, and the bit reversal: point i goes to brev(i) of the work
//     array, so that the stages below are decimation in time, natural order out.
//   group_stage_kernel<C, UNIFORM>: one butterfly per lane, T = w Q, then P + T and P - T, in place.  The work array stays AFFINE
//     between stages (internal form, x == 0 is infinity): the chain then runs on mixed additions, and every stage ends in the
//     per-workgroup shared inversion of scale_points_kernel -- here for two results per lane: the lane multiplies its two ZZ ZZZ
//     first, the tree in LDS holds the 256 products, and the lane splits its inverse again.  A result at infinity contributes 1.
//     Every addition is C::madd, WITH the corner cases: P = +/- w Q and infinity operands are ordinary inputs here (a constant
//     input makes every first-stage butterfly a doubling and a cancellation), and the chain itself passes through +/- Q for
//     twiddles near r, as naf_chain's comment explains (keybytes.h).
//     Lanes: in the stage of half-span m there are m distinct twiddles w_n^(j n/2m), each used by the n/2m blocks.  Butterfly t is
//     block (t mod n/2m), offset j = t / (n/2m): neighbouring lanes share j.  With n/2m >= 64 a whole wavefront shares ONE twiddle
//     (UNIFORM): its digit masks are read through readfirstlane, the chain's "add on a non-zero digit" branch is a scalar branch as
//     in scale_points_kernel, ~253 dbl + ~85 madd.  Later stages (UNIFORM = false) read per-lane digits: the branch diverges, and a
//     wavefront with d distinct digit strings executes the addition in 1 - (2/3)^d of the steps; the same lane order keeps d at
//     64 / (n/2m) instead of 64.  Twiddle 1 (j = 0, and the whole first stage) runs no multiplication.
//   group_twiddle_kernel: the table of n/2 twiddles w^k (w = w_n or its inverse), lane k multiplying the w^(2^i) of its set bits,
//     recoded on the spot into the NAF digit masks of ScaleDigits.
//   the 1/n of the inverse transform is one scalar for the whole array: scale_points_kernel once, after the last stage.
//
// The setup: L1, L2, aL, bL = the inverse transforms of tau^k G1, tau^k G2, alpha tau^k G1, beta tau^k G1 (k < n; one twiddle table
// for the four), kept on the device in reference format; then
//   column_sum_kernel<C>: one lane per column sum ("job"): A_j = sum a_ji L1_i, B1_j = sum b_ji L1_i, K_j = sum a_ji bL_i + sum b_ji aL_i
//     + sum c_ji L1_i (one job over the concatenated base array L1 | aL | bL; C for j > nPublic, IC for j <= nPublic) on G1, B2_j = sum
//     b_ji L2_i on G2.  The lane walks its records: the coefficient leaves Montgomery form, c or r - c (the shorter: -1 is a negation)
//     is recoded into NAF, the chain runs on guarded mixed additions, the sums are full additions with the corner cases; the results
//     leave affine behind the shared inversion.  A job of more than PKSETUP_MSM_MIN records (default 32; a real circuit's constant
//     signal sits in 10^5 rows) is skipped by the lanes: column_gather_kernel collects its points and plain scalars and the library's
//     ordinary MSM sums them.  Both ways end in the canonical affine bytes of one group element: the key does not depend on the switch.
//   hexps_kernel: hExps_i = tau^(n+i) G1 - tau^i G1, one lane per point, one guarded mixed addition, the shared inversion; it also
//     gives the upper half of tau_g1 its input tests.
//   Every power gets pk_classify's two tests before anything is computed from it; a bad one is a RESULT (ok = 0, per-array counts
//     through pk_reduce), as in the audit and the contribution.
//
// Not here: whether the powers ARE powers of one tau and the G2 subgroup test of tau_g2 -- both are the transcript's own audit,
// wsnark_powers_check (pwtau.hip), to be run before a key is built on the powers; .ptau / .r1cs parsers, file-to-file variants, more
// than one GPU.
#include <string.h>

#include "keybytes.h"

namespace wsnark {

using namespace hostpair;

// one value for the wavefront (the first active lane's): what the compiler then keeps in scalar registers and branches on without
// a lane mask.  On the thread emulator a lane is its own wavefront.
#ifdef WSNARK_EMUL
#define WS_WAVE_U32(x) ((uint32_t)(x))
#else
#define WS_WAVE_U32(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#endif
__device__ inline uint64_t wave_u64(uint64_t v) {
    return (uint64_t)WS_WAVE_U32((uint32_t)v) | ((uint64_t)WS_WAVE_U32((uint32_t)(v >> 32)) << 32);
}

// ---- device ----
// (naf_digits, naf_chain, block_inverse and affine_result -- the recoding, the chain over the digit masks in registers with the
// argument for its guarded additions, the shared inversion, the affine output -- are keybytes.h's: scale_points_kernel and the
// phase-1 contribution's kernel, pwtau.hip, use them too)
struct TwiddleBase { Fe p[24]; };      // w^(2^i), Montgomery
__global__ __launch_bounds__(256) void group_twiddle_kernel(TwiddleBase W, uint32_t count, ScaleDigits* __restrict__ out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    Fe acc = Fr::one();
    for (int i = 0; i < 24; i++)
        if ((k >> i) & 1) acc = Fr::mul(acc, W.p[i]);
    ScaleDigits D;
    naf_digits(Fr::from_mont(acc), &D);
    out[k] = D;
}

template <class C>
__global__ __launch_bounds__(256) void group_load_kernel(const typename C::AffP* __restrict__ pts, uint64_t n, uint32_t log_n,
                                                           typename C::El curve_b, typename C::AffP* __restrict__ work, PkAcc* __restrict__ acc) {
    typedef typename C::Field F;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int st = 0;
    typename C::Aff P = typename C::Aff{F::zero(), F::zero()};
    if (i < n) st = pk_classify<C>(pts[i], curve_b, &P);
    pk_reduce(st, i, acc);
    if (i < n) {
        if (st != 0) P = typename C::Aff{F::zero(), F::zero()};      // infinity; a bad point fails the call before any stage runs
        const uint64_t to = log_n ? (uint64_t)(__brev((unsigned)i) >> (32 - log_n)) : 0;
        work[to] = C::pack_aff(P);
    }
}

// the stage of half-span m = 2^log_m over the n = 2^log_n points of `a` (n >= 2, log_m < log_n); tw[k] = the digits of w^k, k < n/2.
// last: the results leave in reference format (canonical; infinity as zero bytes) instead of the internal form.
template <class C, bool UNIFORM>
__global__ __launch_bounds__(256) void group_stage_kernel(typename C::AffP* __restrict__ a, uint32_t log_n, uint32_t log_m,
                                                            const ScaleDigits* __restrict__ tw, int last) {
    typedef typename C::Field F;
    typedef typename C::El El;
    typedef typename C::Aff Aff;
    typedef typename C::Pt Pt;
    const uint64_t half = (uint64_t)1 << (log_n - 1);
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = t < half;                                   // (n < 512: lanes past the end only keep the barriers company)
    const uint32_t log_cnt = log_n - 1 - log_m;                 // n/2m blocks
    const uint64_t tt = on ? t : 0;
    // block order: neighbouring lanes share the offset j, hence the twiddle
    const uint64_t j = tt >> log_cnt, blk = tt & (((uint64_t)1 << log_cnt) - 1);
    const uint64_t i0 = (blk << (log_m + 1)) + j, i1 = i0 + ((uint64_t)1 << log_m);
    uint32_t k = (uint32_t)(j << log_cnt);                      // the twiddle w_n^(j n/2m): < n/2
    if (UNIFORM) k = WS_WAVE_U32(k);                            // n/2m >= 64: the wavefront's 64 butterflies share j

    Aff Q = Aff{F::zero(), F::zero()};
    if (on) Q = C::unpack_aff(a[i1]);
    // T = w^k Q: the chain starts as Q itself
    Pt T = C::infinity();
    if (on && !C::aff_is_inf(Q)) {
        T = Pt{Q.x, Q.y, F::one(), F::one()};
        if (k != 0) {
            uint64_t nz[4], ng[4];
            int top = tw[k].top;
            for (int w = 0; w < 4; w++) { nz[w] = tw[k].nz[w]; ng[w] = tw[k].neg[w]; }
            if (UNIFORM) {
                top = (int)WS_WAVE_U32(top);
                for (int w = 0; w < 4; w++) { nz[w] = wave_u64(nz[w]); ng[w] = wave_u64(ng[w]); }
            }
            naf_chain<C>(T, Q, nz[0], nz[1], nz[2], nz[3], ng[0], ng[1], ng[2], ng[3], top);
        }
    }
    // R0 = P + T; R1 = P - T = -(T - P).  P is loaded here, behind the chain, and not beside Q: held across the chain it costs the
    // G2 kernels ~100 registers parked in AGPRs (only this lane writes a[i0], and only below)
    Pt R0 = T, R1 = T;
    if (on) {
        const Aff P = C::unpack_aff(a[i0]);
        C::madd(R0, P, false);
        C::madd(R1, P, true);
        R1 = C::neg(R1);
    }
    const bool fin0 = on && !C::is_inf(R0), fin1 = on && !C::is_inf(R1);

    // one inversion per workgroup: the leaves of the tree are the lanes' PRODUCTS of two
    const El z0 = fin0 ? F::mul(R0.zz, R0.zzz) : F::one(), z1 = fin1 ? F::mul(R1.zz, R1.zzz) : F::one();
    const El inv = block_inverse<F>(F::mul(z0, z1));
    if (!on) return;
    a[i0] = affine_result<C>(R0, fin0, F::mul(inv, z1), last);
    a[i1] = affine_result<C>(R1, fin1, F::mul(inv, z0), last);
}

// ---- the column sums and hExps (wsnark_pkey_setup) ----
// k (plain, < r) or r - k, whichever is smaller; *neg says which: a coefficient of -1 is one point negation, not a 254-bit chain
__device__ inline Fe fr_short(const Fe& k, bool* neg) {
    const uint64_t r[4] = {FrParams::P0, FrParams::P1, FrParams::P2, FrParams::P3};
    Fe d;
    unsigned long long borrow = 0;
    for (int i = 0; i < 4; i++) {
        const uint64_t t = r[i] - k.l[i], u = t - borrow;
        borrow = (r[i] < k.l[i]) || (t < borrow);
        d.l[i] = u;
    }
    bool less = false;      // d < k
    for (int i = 3; i >= 0; i--) {
        if (d.l[i] != k.l[i]) { less = d.l[i] < k.l[i]; break; }
    }
    *neg = less;
    return less ? d : k;
}

// One lane per job = one column sum: out[j] = sum over the job's entries of coef x base[src].  coef: Fr Montgomery as in the record
// streams, taken out of Montgomery form here; base: reference format (the transforms' results), x == 0 is infinity.  A zero
// coefficient or an infinity base adds nothing, repeated indices simply add, a job without entries is infinity (zero bytes).  A job
// with more than msm_min entries is left alone: its column goes through the MSM and the host writes its point.  The sums are full
// additions WITH the corner cases (two records may name one row); the results leave affine, canonical, behind the shared inversion.
template <class C>
__global__ __launch_bounds__(256) void column_sum_kernel(const uint64_t* __restrict__ job_ptr, uint64_t n_jobs, const uint32_t* __restrict__ ent_src,
                                                          const Fe* __restrict__ ent_coef, const typename C::AffP* __restrict__ base,
                                                          uint64_t msm_min, typename C::AffP* __restrict__ out) {
    typedef typename C::Field F;
    typedef typename C::El El;
    typedef typename C::Pt Pt;
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool mine = j < n_jobs;
    Pt acc = C::infinity();
    if (mine) {
        const uint64_t lo = job_ptr[j], hi = job_ptr[j + 1];
        if (hi - lo > msm_min) mine = false;
        for (uint64_t e = lo; mine && e < hi; e++) {
            bool neg;
            const Fe k = fr_short(Fr::reduce_full(Fr::from_mont(ent_coef[e])), &neg);
            const typename C::AffP bp = base[ent_src[e]];
            ScaleDigits D;
            naf_digits(k, &D);
            bool inf = true;      // the loaders' rule: every word of x zero
            for (unsigned w = 0; w < sizeof(bp) / 64; w++) inf = inf && pk_zero(reinterpret_cast<const Fe*>(&bp)[w]);
            if (D.top < 0 || inf) continue;
            const typename C::Aff B = C::aff_to_internal(bp);
            Pt T = Pt{B.x, F::cneg(B.y, neg), F::one(), F::one()};
            const typename C::Aff Bs = typename C::Aff{T.x, T.y};
            naf_chain<C>(T, Bs, D.nz[0], D.nz[1], D.nz[2], D.nz[3], D.neg[0], D.neg[1], D.neg[2], D.neg[3], D.top);
            acc = C::add(acc, T);
        }
    }
    const bool fin = mine && !C::is_inf(acc);
    const El inv = block_inverse<F>(fin ? F::mul(acc.zz, acc.zzz) : F::one());
    if (mine) out[j] = affine_result<C>(acc, fin, inv, 1);
}

// a long column's points and plain scalars, gathered for the ordinary MSM
template <class AffP>
__global__ __launch_bounds__(256) void column_gather_kernel(const uint32_t* __restrict__ ent_src, const Fe* __restrict__ ent_coef, uint64_t lo,
                                                             uint64_t count, const AffP* __restrict__ base, AffP* __restrict__ pts, Fe* __restrict__ sc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    pts[i] = base[ent_src[lo + i]];
    sc[i] = Fr::reduce_full(Fr::from_mont(ent_coef[lo + i]));
}

// hExps_i = tau^(n+i) G - tau^i G: one lane per point, one mixed addition, the shared inversion.  The upper half of tau_g1 gets its
// tests here (indices n + i into acc); the lower half was counted by its transform's load kernel.
__global__ __launch_bounds__(256) void hexps_kernel(const G1R29::AffP* __restrict__ lo, const G1R29::AffP* __restrict__ hi, uint64_t n,
                                                    G1R29::El curve_b, G1R29::AffP* __restrict__ out, PkAcc* __restrict__ acc) {
    typedef G1R29 C;
    typedef C::Field F;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int st_hi = 0, st_lo = 0;
    C::Aff P = C::Aff{F::zero(), F::zero()}, Q = P;
    if (i < n) {
        st_hi = pk_classify<C>(hi[i], curve_b, &P);
        st_lo = pk_classify<C>(lo[i], curve_b, &Q);
    }
    pk_reduce(st_hi, n + i, acc);
    C::Pt R = C::infinity();
    if (i < n && (st_hi == 0 || st_hi == 4) && (st_lo == 0 || st_lo == 4)) {      // (a bad power: the outputs are unspecified)
        if (st_hi == 0) R = C::Pt{P.x, P.y, F::one(), F::one()};
        if (st_lo == 0) C::madd(R, Q, true);
    }
    const bool fin = !C::is_inf(R);
    const C::El inv = block_inverse<F>(fin ? F::mul(R.zz, R.zzz) : F::one());
    if (i < n) out[i] = affine_result<C>(R, fin, inv, 1);
}

// ---- host ----
namespace {
inline int scale_dev(G1R29*, Context* X, const void* in, uint64_t n, const ScaleDigits& D, void* out, PkAcc* acc, hipStream_t s) {
    return g1_scale_dev(X, in, n, D, out, acc, s);
}
inline int scale_dev(G2R29*, Context* X, const void* in, uint64_t n, const ScaleDigits& D, void* out, PkAcc* acc, hipStream_t s) {
    return g2_scale_dev(X, in, n, D, out, acc, s);
}
template <class C> const char* stage_name(bool uniform) {
    constexpr bool g1 = sizeof(typename C::AffP) == 64;
    return g1 ? (uniform ? "group_ntt_g1_uniform" : "group_ntt_g1_lane") : (uniform ? "group_ntt_g2_uniform" : "group_ntt_g2_lane");
}

// w_{2^28} = 5^((r-1)/2^28), the root wsnark_fr_ntt uses (ntt.hip: root_of_unity), squared down to w_n
Fe root_of_unity(int bits) {
    const Fe plain = {{0x9bd61b6e725b19f0ull, 0x402d111e41112ed4ull, 0x00e0a7eb8ef62abcull, 0x2a3c09f0a58a7e85ull}};
    Fe w = Fr::to_mont(plain);
    for (int i = 28; i > bits; i--) w = Fr::sqr(w);
    return w;
}

// d_tw[k] = the digits of w^k, k < n/2, w = w_n (forward) or w_n^-1 (inverse)
int build_twiddles(Context* X, int bits, int inverse, ScaleDigits* d_tw, hipStream_t s) {
    TwiddleBase W;
    Fe w = root_of_unity(bits);
    if (inverse) w = Fr::inv(w);
    for (int i = 0; i < 24; i++) { W.p[i] = w; w = Fr::sqr(w); }
    const uint32_t count = (uint32_t)1 << (bits - 1);
    X->timer.begin("group_ntt_twiddles", s);
    hipLaunchKernelGGL(group_twiddle_kernel, dim3(ceil_div_u64(count, 256)), dim3(256), 0, s, W, count, d_tw);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    return WS_OK;
}

// the log2 n stages over d_work (bit-reversed internal form in, natural order out; the last stage leaves reference format)
template <class C>
int run_stages(Context* X, typename C::AffP* d_work, int bits, const ScaleDigits* d_tw, hipStream_t s) {
    // one twiddle per wavefront while the stage has 64 blocks, per-lane digits in block order after that
    const uint32_t grid = ceil_div_u64((uint64_t)1 << (bits - 1), 256);
    for (int lm = 0; lm < bits; lm++) {
        const bool uniform = bits - 1 - lm >= 6;
        const int last = lm == bits - 1;
        X->timer.begin(stage_name<C>(uniform), s);
        if (uniform)
            hipLaunchKernelGGL((group_stage_kernel<C, true>), dim3(grid), dim3(256), 0, s, d_work, (uint32_t)bits, (uint32_t)lm, d_tw, last);
        else
            hipLaunchKernelGGL((group_stage_kernel<C, false>), dim3(grid), dim3(256), 0, s, d_work, (uint32_t)bits, (uint32_t)lm, d_tw, last);
        WS_HIP_CHECK(hipGetLastError());
        X->timer.end(s);
    }
    return WS_OK;
}

// the input's tests, the internal form and the bit reversal: d_in (reference format) -> d_work; counts into d_acc
template <class C>
int ntt_load(Context* X, const typename C::AffP* d_in, typename C::AffP* d_work, uint64_t n, int bits, PkAcc* d_acc, hipStream_t s) {
    typename C::El cb;
    const int rc = curve_b(&cb);
    if (rc) return rc;
    X->timer.begin(sizeof(typename C::AffP) == 64 ? "group_ntt_g1_load" : "group_ntt_g2_load", s);
    hipLaunchKernelGGL(group_load_kernel<C>, dim3(ceil_div_u64(n, 256)), dim3(256), 0, s, d_in, n, (uint32_t)bits, cb, d_work, d_acc);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    return WS_OK;
}
// ... and the transform of what ntt_load left in d_work (bits >= 1): the result, in reference format, is in d_work (forward) or
// d_in (inverse: the 1/n pass goes back there); *d_res says which.  d_tw: n/2 entries, filled here unless have_tw (the setup's four
// transforms share one table); d_spare: a PkAcc nobody reads.
template <class C>
int ntt_finish(Context* X, typename C::AffP* d_in, typename C::AffP* d_work, ScaleDigits* d_tw, uint64_t n, int bits, int inverse,
               PkAcc* d_spare, typename C::AffP** d_res, hipStream_t s, bool have_tw = false) {
    int rc;
    if (!have_tw && (rc = build_twiddles(X, bits, inverse, d_tw, s))) return rc;
    if ((rc = run_stages<C>(X, d_work, bits, d_tw, s))) return rc;
    *d_res = d_work;
    if (inverse) {      // n^-1 = (2^-1)^bits
        Fe half = Fr::inv(Fr::add(Fr::one(), Fr::one())), ninv = Fr::one();
        for (int i = 0; i < bits; i++) ninv = Fr::mul(ninv, half);
        ScaleDigits D;
        naf_digits(Fr::from_mont(ninv), &D);
        if ((rc = scale_dev((C*)nullptr, X, d_work, n, D, d_in, d_spare, s))) return rc;
        *d_res = d_in;
    }
    return WS_OK;
}

int size_bits(uint64_t n, int* bits) {
    if (n == 0 || (n & (n - 1)) || n > ((uint64_t)1 << 24)) {
        set_last_error("group transform: n must be a power of two in [1, 2^24]");
        return WS_ERR_SIZE;
    }
    int b = 0;
    while (((uint64_t)1 << b) < n) b++;
    *bits = b;
    return WS_OK;
}

template <class C>
int group_ntt(const void* points, uint64_t n, int inverse, void* out) {
    typedef typename C::AffP AffP;
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    int bits, rc;
    if ((rc = size_bits(n, &bits))) return rc;
    if (!points || !out) return WS_ERR_ARG;
    const size_t bytes = (size_t)n * sizeof(AffP);
    LaneLock L = acquire_lane(X);
    hipStream_t s = L->stream;
    DevBuf d_in, d_work, d_tw, d_acc;
    WS_HIP_CHECK(d_in.alloc(bytes));
    WS_HIP_CHECK(d_work.alloc(bytes));
    WS_HIP_CHECK(d_tw.alloc((size_t)std::max<uint64_t>(n / 2, 1) * sizeof(ScaleDigits)));
    WS_HIP_CHECK(d_acc.alloc(2 * sizeof(PkAcc)));
    WS_HIP_CHECK(hipMemsetAsync(d_acc.p, 0, 2 * sizeof(PkAcc), s));
    if ((rc = upload_staged(d_in.p, points, bytes, s))) return rc;
    // the input's tests first: a bad point fails the call before a stage has run on it
    if ((rc = ntt_load<C>(X, d_in.as<AffP>(), d_work.as<AffP>(), n, bits, d_acc.as<PkAcc>(), s))) return rc;
    PkAcc h_acc;
    WS_HIP_CHECK(hipMemcpyAsync(&h_acc, d_acc.p, sizeof h_acc, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    uint64_t inf, bad, first;
    uint32_t reason;
    pk_decode(h_acc, &inf, &bad, &first, &reason);
    if (bad) {
        set_last_error("group transform: " + std::to_string(bad) + " point(s) unreduced or off the curve, the first at index " + std::to_string(first));
        return WS_ERR_FORMAT;
    }
    if (bits == 0) {      // the identity; infinity leaves as zero bytes like every other result
        if (inf) memset(out, 0, bytes);
        else if (out != points) memcpy(out, points, bytes);
        return WS_OK;
    }
    AffP* d_res = nullptr;
    if ((rc = ntt_finish<C>(X, d_in.as<AffP>(), d_work.as<AffP>(), d_tw.as<ScaleDigits>(), n, bits, inverse, d_acc.as<PkAcc>() + 1, &d_res, s))) return rc;
    WS_HIP_CHECK(hipMemcpyAsync(out, d_res, bytes, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    return WS_OK;
}

// ---- the setup ----
// a record stream in its own (column) order: signal j's records are [ptr[j], ptr[j + 1])
struct Columns {
    std::vector<uint64_t> ptr;
    std::vector<uint32_t> idx;
    std::vector<Fe> coef;      // Fr Montgomery, as stored
};
// `ncoefs, (idx, coef)*` per signal (src/build_pol.js:62-144), with the loaders' conditions and codes (calch.hip: pols_to_csr)
int parse_columns(const uint8_t* pols, uint64_t len, uint32_t n_vars, uint32_t domain, Columns* out) {
    out->ptr.assign((size_t)n_vars + 1, 0);
    uint64_t pp = 0, nnz = 0;
    for (uint32_t j = 0; j < n_vars; j++) {      // lengths first: the arrays are sized once
        if (pp + 4 > len) { set_last_error("pols: truncated record header"); return WS_ERR_FORMAT; }
        uint32_t nc;
        memcpy(&nc, pols + pp, 4);
        pp += 4;
        if ((uint64_t)nc * 36 > len - pp) { set_last_error("pols: truncated coefficient records"); return WS_ERR_FORMAT; }
        pp += (uint64_t)nc * 36;
        nnz += nc;
        if (nnz >= ((uint64_t)1 << 32)) return WS_ERR_SIZE;
        out->ptr[j + 1] = nnz;
    }
    out->idx.resize((size_t)nnz);
    out->coef.resize((size_t)nnz);
    pp = 0;
    for (uint32_t j = 0; j < n_vars; j++) {
        pp += 4;
        for (uint64_t e = out->ptr[j]; e < out->ptr[j + 1]; e++, pp += 36) {
            memcpy(&out->idx[e], pols + pp, 4);
            memcpy(&out->coef[e], pols + pp + 4, 32);
            if (out->idx[e] >= domain) { set_last_error("pols: constraint index out of range"); return WS_ERR_FORMAT; }
        }
    }
    return WS_OK;
}

// the column sums of one group as jobs over ONE base array: entry = (coefficient, index into the base array)
struct Jobs {
    std::vector<uint64_t> ptr{0};
    std::vector<uint32_t> src;
    std::vector<Fe> coef;
    void part(const Columns& M, uint32_t j, uint32_t offset) {
        for (uint64_t e = M.ptr[j]; e < M.ptr[j + 1]; e++) { src.push_back(offset + M.idx[e]); coef.push_back(M.coef[e]); }
    }
    void close() { ptr.push_back(src.size()); }
    uint64_t count() const { return ptr.size() - 1; }
};
struct DevJobs {
    DevBuf ptr, src, coef;
    int upload(const Jobs& J, hipStream_t s) {
        WS_HIP_CHECK(ptr.alloc(J.ptr.size() * 8));
        WS_HIP_CHECK(src.alloc(J.src.size() * 4));
        WS_HIP_CHECK(coef.alloc(J.coef.size() * sizeof(Fe)));
        WS_HIP_CHECK(hipMemcpyAsync(ptr.p, J.ptr.data(), J.ptr.size() * 8, hipMemcpyHostToDevice, s));
        if (!J.src.empty()) {
            WS_HIP_CHECK(hipMemcpyAsync(src.p, J.src.data(), J.src.size() * 4, hipMemcpyHostToDevice, s));
            WS_HIP_CHECK(hipMemcpyAsync(coef.p, J.coef.data(), J.coef.size() * sizeof(Fe), hipMemcpyHostToDevice, s));
        }
        WS_HIP_CHECK(hipStreamSynchronize(s));      // (the vectors are the caller's temporaries)
        return WS_OK;
    }
};

inline int lane_msm(Lane& L, const Fe* sc, const G1R29::AffP* pts, uint64_t n, uint8_t* out, hipStream_t s) {
    Jac<Fq> r;
    const int rc = msm_g1_dev(L, sc, reinterpret_cast<const Affine<Fq>*>(pts), n, WindowShard{}, &r, s);
    if (rc) return rc;
    if (Fq::is_zero(r.z)) memset(out, 0, 64);
    else memcpy(out, &r, 64);
    return WS_OK;
}
inline int lane_msm(Lane& L, const Fe* sc, const G2R29::AffP* pts, uint64_t n, uint8_t* out, hipStream_t s) {
    Jac<Fq2> r;
    const int rc = msm_g2_dev(L, sc, reinterpret_cast<const Affine<Fq2>*>(pts), n, WindowShard{}, &r, s);
    if (rc) return rc;
    if (Fq2::is_zero(r.z)) memset(out, 0, 128);
    else memcpy(out, &r, 128);
    return WS_OK;
}

// d_out[j] = job j's sum for every job of at most msm_min entries (the lanes); the longer ones through the MSM into long_out
// (job index, point bytes), which the caller writes over its copy of d_out
template <class C>
int column_sums(Context* X, Lane& L, const Jobs& J, const typename C::AffP* d_base, uint64_t msm_min, typename C::AffP* d_out,
                std::vector<std::pair<uint64_t, std::vector<uint8_t>>>* long_out, hipStream_t s) {
    typedef typename C::AffP AffP;
    DevJobs D;
    int rc;
    if ((rc = D.upload(J, s))) return rc;
    const uint64_t n_jobs = J.count();
    X->timer.begin(sizeof(AffP) == 64 ? "column_sum_g1" : "column_sum_g2", s);
    hipLaunchKernelGGL(column_sum_kernel<C>, dim3(ceil_div_u64(n_jobs, 256)), dim3(256), 0, s, D.ptr.as<uint64_t>(), n_jobs, D.src.as<uint32_t>(),
                       D.coef.as<Fe>(), d_base, msm_min, d_out);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    uint64_t longest = 0;
    for (uint64_t j = 0; j < n_jobs; j++)
        if (J.ptr[j + 1] - J.ptr[j] > msm_min) longest = std::max(longest, J.ptr[j + 1] - J.ptr[j]);
    if (!longest) return WS_OK;
    DevBuf d_pts, d_sc;
    WS_HIP_CHECK(d_pts.alloc((size_t)longest * sizeof(AffP)));
    WS_HIP_CHECK(d_sc.alloc((size_t)longest * sizeof(Fe)));
    for (uint64_t j = 0; j < n_jobs; j++) {
        const uint64_t lo = J.ptr[j], cnt = J.ptr[j + 1] - lo;
        if (cnt <= msm_min) continue;
        hipLaunchKernelGGL(column_gather_kernel<AffP>, dim3(ceil_div_u64(cnt, 256)), dim3(256), 0, s, D.src.as<uint32_t>(), D.coef.as<Fe>(), lo, cnt,
                           d_base, d_pts.as<AffP>(), d_sc.as<Fe>());
        WS_HIP_CHECK(hipGetLastError());
        long_out->emplace_back(j, std::vector<uint8_t>(sizeof(AffP)));
        if ((rc = lane_msm(L, d_sc.as<Fe>(), d_pts.as<AffP>(), cnt, long_out->back().second.data(), s))) return rc;
    }
    return WS_OK;
}

struct SetupOut { uint8_t *A, *B1, *B2, *Cp, *H, *alfa1, *beta1, *delta1, *beta2, *delta2, *ic; };
struct SetupIn {
    const wsnark_powers_t* P;
    const wsnark_circuit_t* K;
    Columns A, B, Cm;
    int bits;
};

// everything that can fail before a byte is written
int setup_prepare(const wsnark_powers_t* P, const wsnark_circuit_t* K, SetupIn* in) {
    if (!ctx()) return WS_ERR_NOINIT;
    if (!P || !K || !P->tau_g1 || !P->tau_g2 || !P->alpha_tau_g1 || !P->beta_tau_g1 || !P->beta_g2 || !K->polsA || !K->polsB || !K->polsC)
        return WS_ERR_ARG;
    int rc;
    if ((rc = key_vars_check(K->n_vars, K->n_public))) return rc;
    const uint64_t n = K->domain;
    if (n < 2 || (n & (n - 1)) || n > ((uint64_t)1 << 24)) { set_last_error("key setup: domain must be a power of two in [2, 2^24]"); return WS_ERR_SIZE; }
    if (P->domain != K->domain) { set_last_error("key setup: the powers and the circuit name different domains"); return WS_ERR_SIZE; }
    if (P->tau_g1_len < 2 * n * 64 || P->tau_g2_len < n * 128 || P->alpha_tau_g1_len < n * 64 || P->beta_tau_g1_len < n * 64) {
        set_last_error("key setup: an array of powers is shorter than the domain implies (tau_g1: 2n, the others: n)");
        return WS_ERR_FORMAT;
    }
    if ((rc = parse_columns((const uint8_t*)K->polsA, K->polsA_len, K->n_vars, K->domain, &in->A))) return rc;
    if ((rc = parse_columns((const uint8_t*)K->polsB, K->polsB_len, K->n_vars, K->domain, &in->B))) return rc;
    if ((rc = parse_columns((const uint8_t*)K->polsC, K->polsC_len, K->n_vars, K->domain, &in->Cm))) return rc;
    const G1A g1 = gen1();
    const G2A g2 = gen2();
    if (memcmp(P->tau_g1, &g1.x, 64) != 0 || memcmp(P->tau_g2, &g2.x, 128) != 0) {
        set_last_error("key setup: tau_g1[0] / tau_g2[0] is not the generator");
        return WS_ERR_FORMAT;
    }
    in->P = P;
    in->K = K;
    in->bits = 0;
    while (((uint64_t)1 << in->bits) < n) in->bits++;
    return WS_OK;
}

int setup_run(const SetupIn& in, const SetupOut& out, wsnark_pkey_setup_report_t* rep) {
    typedef G1R29::AffP A1;
    typedef G2R29::AffP A2;
    Context* X = ctx();
    const auto t_begin = Clock::now();
    const wsnark_powers_t& P = *in.P;
    const uint64_t n = in.K->domain, nv = in.K->n_vars, npub = in.K->n_public, nC = nv - npub - 1;
    const int bits = in.bits;
    wsnark_pkey_setup_report_t R;
    memset(&R, 0, sizeof R);
    int rc;
    G1R29::El cb1;
    if ((rc = curve_b(&cb1))) return rc;

    LaneLock L = acquire_lane(X);
    hipStream_t s = L->stream;
    DevBuf d_in1, d_work1, d_hi, d_in2, d_work2, d_tw, d_acc, d_h;
    WS_HIP_CHECK(d_in1.alloc(3 * n * 64));       // tau^k G1 | alpha tau^k G1 | beta tau^k G1, then L1 | aL | bL: the G1 sums' base array
    WS_HIP_CHECK(d_work1.alloc(3 * n * 64));
    WS_HIP_CHECK(d_hi.alloc(n * 64));            // tau^(n + k) G1
    WS_HIP_CHECK(d_in2.alloc(n * 128));
    WS_HIP_CHECK(d_work2.alloc(n * 128));
    WS_HIP_CHECK(d_tw.alloc((n / 2) * sizeof(ScaleDigits)));
    WS_HIP_CHECK(d_acc.alloc(5 * sizeof(PkAcc)));
    WS_HIP_CHECK(d_h.alloc(n * 64));
    WS_HIP_CHECK(hipMemsetAsync(d_acc.p, 0, 5 * sizeof(PkAcc), s));
    A1* in1 = d_in1.as<A1>();
    A1* work1 = d_work1.as<A1>();
    PkAcc* acc = d_acc.as<PkAcc>();
    const uint8_t* src1[3] = {(const uint8_t*)P.tau_g1, (const uint8_t*)P.alpha_tau_g1, (const uint8_t*)P.beta_tau_g1};
    const int acc_of[3] = {WSNARK_PW_TAU_G1, WSNARK_PW_ALPHA_TAU_G1, WSNARK_PW_BETA_TAU_G1};

    // 1. the powers go up; every one gets the audit's two tests (the transforms' load kernels, and hExps for the upper half of tau_g1)
    auto t0 = Clock::now();
    for (int a = 0; a < 3; a++) {
        if ((rc = upload_staged(in1 + a * n, src1[a], n * 64, s))) return rc;
        if ((rc = ntt_load<G1R29>(X, in1 + a * n, work1 + a * n, n, bits, acc + acc_of[a], s))) return rc;
    }
    if ((rc = upload_staged(d_hi.p, (const uint8_t*)P.tau_g1 + n * 64, n * 64, s))) return rc;
    if ((rc = upload_staged(d_in2.p, P.tau_g2, n * 128, s))) return rc;
    if ((rc = ntt_load<G2R29>(X, d_in2.as<A2>(), d_work2.as<A2>(), n, bits, acc + WSNARK_PW_TAU_G2, s))) return rc;
    WS_HIP_CHECK(hipStreamSynchronize(s));
    double ms_tr = ms_since(t0);
    t0 = Clock::now();
    X->timer.begin("hexps", s);
    hipLaunchKernelGGL(hexps_kernel, dim3(ceil_div_u64(n, 256)), dim3(256), 0, s, in1, d_hi.as<A1>(), n, cb1, d_h.as<A1>(), acc + WSNARK_PW_TAU_G1);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    PkAcc h_acc[4];
    WS_HIP_CHECK(hipMemcpyAsync(h_acc, d_acc.p, sizeof h_acc, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    const double ms_h = ms_since(t0);
    bool ok = true;
    for (int a = 0; a < 4; a++) {
        R.points[a] = a == WSNARK_PW_TAU_G1 ? 2 * n : n;
        pk_decode(h_acc[a], &R.infinity[a], &R.bad[a], &R.first_bad[a], &R.first_reason[a]);
        ok = ok && R.bad[a] == 0;
    }
    G2A b2;
    R.beta2_reason = fixed_g2((const uint8_t*)P.beta_g2, true, &b2);
    ok = ok && R.beta2_reason == 0;
    double ms_sums = 0;
    if (ok) {
        // 2. the four inverse transforms, one twiddle table
        t0 = Clock::now();
        ScaleDigits* tw = d_tw.as<ScaleDigits>();
        if ((rc = build_twiddles(X, bits, 1, tw, s))) return rc;
        A1* res1 = nullptr;
        A2* res2 = nullptr;
        for (int a = 0; a < 3; a++)
            if ((rc = ntt_finish<G1R29>(X, in1 + a * n, work1 + a * n, tw, n, bits, 1, acc + 4, &res1, s, true))) return rc;
        if ((rc = ntt_finish<G2R29>(X, d_in2.as<A2>(), d_work2.as<A2>(), tw, n, bits, 1, acc + 4, &res2, s, true))) return rc;
        WS_HIP_CHECK(hipStreamSynchronize(s));
        ms_tr += ms_since(t0);

        // 3. the column sums: A | B1 | K over (L1 | aL | bL), B2 over L2
        t0 = Clock::now();
        const long mm = tuning_get("PKSETUP_MSM_MIN", 32);
        const uint64_t msm_min = mm <= 0 ? UINT64_MAX : (uint64_t)mm;      // 0: no column goes through the MSM
        Jobs J1, J2;
        for (uint32_t j = 0; j < nv; j++) { J1.part(in.A, j, 0); J1.close(); }
        for (uint32_t j = 0; j < nv; j++) { J1.part(in.B, j, 0); J1.close(); }
        for (uint32_t j = 0; j < nv; j++) {
            J1.part(in.A, j, (uint32_t)(2 * n));
            J1.part(in.B, j, (uint32_t)n);
            J1.part(in.Cm, j, 0);
            J1.close();
        }
        for (uint32_t j = 0; j < nv; j++) { J2.part(in.B, j, 0); J2.close(); }
        DevBuf d_out1, d_out2;
        WS_HIP_CHECK(d_out1.alloc(3 * nv * 64));
        WS_HIP_CHECK(d_out2.alloc(nv * 128));
        std::vector<std::pair<uint64_t, std::vector<uint8_t>>> long1, long2;
        if ((rc = column_sums<G1R29>(X, *L, J1, in1, msm_min, d_out1.as<A1>(), &long1, s))) return rc;
        if ((rc = column_sums<G2R29>(X, *L, J2, d_in2.as<A2>(), msm_min, d_out2.as<A2>(), &long2, s))) return rc;
        R.msm_columns = (uint32_t)(long1.size() + long2.size());
        // 4. down into the caller's buffers; K splits into IC (j <= nPublic) and C
        const A1* o1 = d_out1.as<A1>();
        auto slot1 = [&](uint64_t job) -> uint8_t* {
            if (job < nv) return out.A + 64 * job;
            if (job < 2 * nv) return out.B1 + 64 * (job - nv);
            const uint64_t j = job - 2 * nv;
            return j <= npub ? out.ic + 64 * j : out.Cp + 64 * (j - npub - 1);
        };
        WS_HIP_CHECK(hipMemcpyAsync(out.A, o1, nv * 64, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipMemcpyAsync(out.B1, o1 + nv, nv * 64, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipMemcpyAsync(out.ic, o1 + 2 * nv, (npub + 1) * 64, hipMemcpyDeviceToHost, s));
        if (nC) WS_HIP_CHECK(hipMemcpyAsync(out.Cp, o1 + 2 * nv + npub + 1, nC * 64, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipMemcpyAsync(out.B2, d_out2.p, nv * 128, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipMemcpyAsync(out.H, d_h.p, n * 64, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));
        for (const auto& e : long1) memcpy(slot1(e.first), e.second.data(), 64);
        for (const auto& e : long2) memcpy(out.B2 + 128 * e.first, e.second.data(), 128);
        ms_sums = ms_since(t0);
        // the fixed points: delta = gamma = 1
        const G1A g1 = gen1();
        const G2A g2 = gen2();
        memcpy(out.alfa1, P.alpha_tau_g1, 64);
        memcpy(out.beta1, P.beta_tau_g1, 64);
        memcpy(out.delta1, &g1.x, 64);
        memcpy(out.beta2, P.beta_g2, 128);
        memcpy(out.delta2, &g2.x, 128);
    }
    R.ok = ok ? 1 : 0;
    R.ms[0] = ms_tr;
    R.ms[1] = ms_sums;
    R.ms[2] = ms_h;
    R.ms[3] = ms_since(t_begin);
    *rep = R;
    return WS_OK;
}

// proving_key.bin's layout (tools/buildpkey.js:124-186): ten u32, the five fixed points, the two streams, the five point sections
struct PkeyLayout { uint64_t off[7], len; };
PkeyLayout pkey_layout(const wsnark_circuit_t& K) {
    const uint64_t nv = K.n_vars, nC = nv - K.n_public - 1;
    const uint64_t part[7] = {K.polsA_len, K.polsB_len, nv * 64, nv * 64, nv * 128, nC * 64, (uint64_t)K.domain * 64};
    PkeyLayout Y;
    uint64_t o = 40 + 448;
    for (int k = 0; k < 7; k++) { Y.off[k] = o; o += part[k]; }
    Y.len = o;
    return Y;
}
}  // namespace

int pkey_setup_sections(const wsnark_powers_t* P, const wsnark_circuit_t* K, void* const out[11], wsnark_pkey_setup_report_t* rep) {
    if (!rep) return WS_ERR_ARG;
    SetupIn in;
    int rc = setup_prepare(P, K, &in);
    if (rc) return rc;
    for (int k = 0; k < 11; k++)
        if (!out[k] && !(k == 3 && (uint64_t)K->n_vars == (uint64_t)K->n_public + 1)) return WS_ERR_ARG;
    uint8_t* const* o = reinterpret_cast<uint8_t* const*>(out);
    return setup_run(in, SetupOut{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], o[10]}, rep);
}

int pkey_setup_size(const wsnark_circuit_t* K, size_t* out_len) {
    if (!K || !out_len) return WS_ERR_ARG;
    if (int rc = key_vars_check(K->n_vars, K->n_public)) return rc;
    const PkeyLayout Y = pkey_layout(*K);
    if (Y.len >= ((uint64_t)1 << 32)) { set_last_error("key setup: the key is beyond the 4 GiB of proving_key.bin's u32 offsets"); return WS_ERR_SIZE; }
    *out_len = (size_t)Y.len;
    return WS_OK;
}

int pkey_setup_bytes(const wsnark_powers_t* P, const wsnark_circuit_t* K, uint8_t* out, size_t out_cap, size_t* out_len, uint8_t* out_ic,
                     wsnark_pkey_setup_report_t* rep) {
    if (!rep || !out || !out_ic) return WS_ERR_ARG;
    SetupIn in;
    int rc = setup_prepare(P, K, &in);
    if (rc) return rc;
    size_t len;
    if ((rc = pkey_setup_size(K, &len))) return rc;
    if (out_cap < len) { set_last_error("key setup: the output buffer is smaller than the key"); return WS_ERR_SIZE; }
    const PkeyLayout Y = pkey_layout(*K);
    uint8_t* f = out + 40;
    rc = setup_run(in, SetupOut{out + Y.off[2], out + Y.off[3], out + Y.off[4], out + Y.off[5], out + Y.off[6], f, f + 64, f + 128, f + 192, f + 320, out_ic}, rep);
    if (rc == WS_OK && rep->ok) {
        uint32_t h[10] = {K->n_vars, K->n_public, K->domain};
        for (int k = 0; k < 7; k++) h[3 + k] = (uint32_t)Y.off[k];
        memcpy(out, h, 40);
        memcpy(out + Y.off[0], K->polsA, K->polsA_len);
        memcpy(out + Y.off[1], K->polsB, K->polsB_len);
        if (out_len) *out_len = len;
    }
    return rc;
}

// ---- the transform's steps on device-resident G1 points (zkey.hip: the H basis change puts its twist before or behind the stages) ----
Fe group_root_of_unity(int bits) { return root_of_unity(bits); }
int g1_ntt_load_dev(Context* X, const void* d_in, void* d_work, uint64_t n, int bits, PkAcc* d_acc, hipStream_t s) {
    return ntt_load<G1R29>(X, (const G1R29::AffP*)d_in, (G1R29::AffP*)d_work, n, bits, d_acc, s);
}
int g1_ntt_stages_dev(Context* X, void* d_work, int bits, int inverse, ScaleDigits* d_tw, hipStream_t s) {
    if (int rc = build_twiddles(X, bits, inverse, d_tw, s)) return rc;
    return run_stages<G1R29>(X, (G1R29::AffP*)d_work, bits, d_tw, s);
}

int g1_group_ntt(const void* points, uint64_t n, int inverse, void* out) { return group_ntt<G1R29>(points, n, inverse, out); }
int g2_group_ntt(const void* points, uint64_t n, int inverse, void* out) { return group_ntt<G2R29>(points, n, inverse, out); }

}  // namespace wsnark
