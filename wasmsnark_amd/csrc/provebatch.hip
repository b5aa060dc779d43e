// provebatch.hip -- many witnesses of ONE resident key in one call (wsnark_groth16_prove_batch[_dev]; include/wsnark.h).  No
// counterpart in the reference, whose groth16GenProof (src/bn128.js:580-720) takes one witness; proof i of a batch is byte for byte
// what wsnark_groth16_prove writes for witness i with r_i, s_i.
//
// Why a path of its own: the single prover's sums are built for one big sum (prove.hip, msm.hip: one grouping pass, fixed-base tables
// of rows x n entries, reduction tails of ~30 dependent additions) and its assembly runs on the host.  At 2^10 .. 2^16 constraints a
// proof is a string of launches of a few hundred workgroups; B proofs over the SAME bases are B x 5 x (windows) independent small sums.
//
//   lc_spmv2_batch_kernel: lc_spmv2_kernel with a proof dimension (blockIdx.z): a = A.w, b = B.w of every proof of the chunk in one
//     launch; the a of all proofs are stored back to back, then the b.
//   CALC_H of the chunk: the transforms of calc_h_dev (calch.hip) with count = proofs (ntt_dev runs transforms stored back to back);
//     the two pointwise products are fr_mul_dev over the stack and batch_combine_kernel is dist_combine_kernel's formula over it (the
//     transforms' fused product-on-load and combining last pass take one transform only).
//   batch_buckets_kernel<C>: ONE workgroup (256 lanes) per (proof, sum, window), unsigned windows of c bits (c = 8: 32 windows, the top
//     one holds bits 248..255 -- nothing is carried), against ROW 0 of the key's resident sections, the prepared points.
//       1. the window's digits are counted into 2^c LDS counters and the non-zero ones are counting-sorted into an index list
//          (global scratch, n x u32 per workgroup: 2^16 entries do not fit LDS beside anything else, and one workgroup per CU is what
//          a 128 KB LDS list would leave -- see profiles/prove_batch_kernel_resources.md);
//       2. every bucket's run is cut into pieces of at most ceil(m / 256) entries (m = the window's non-zero digits), at most 511 pieces
//          whatever the digits are: a boolean-heavy witness puts half of window 0 into bucket 1, and that run is then spread over ~128
//          lanes instead of one.  A lane adds the entries of its (at most two) pieces: madd_fast with madd_wide for the corner cases, a
//          base at infinity (x == 0) skipped by the load;
//       3. lane d sums the pieces of bucket d (no atomics on points: the pieces are stored and re-read);
//       4. sum_d d S_d by running sums on two levels: 16 lanes fold 16 buckets each, lane 0 folds the 16 results (84 dependent additions
//          instead of 510).
//     Nothing depends on the order the LDS atomics hand out: a bucket's entries are summed in any order, and results are compared after
//     the affine normalisation, where a group element has one representation.
//   batch_horner_kernel: one lane per (proof, sum): sum_w 2^(c w) W_w, on the device.
//   batch_fixed_kernel, batch_mid_kernel, batch_final_kernel: the assembly (src/bn128.js:671-718), prove.hip's host code lane by lane:
//     r delta1, s delta1, rs delta1, s delta2; pi_a and s pi_a, pib1 and r pib1; pi_b, pi_c, the affine normalisation, fromMontgomery.
//     One download of chunk x 384 bytes.  These run on the saturated field with curve.h's guarded additions -- the very functions of
//     prove_assemble -- as latency chains on a few lanes per proof.
//   r, s and rs reach the device in a buffer that is overwritten on the call's queue before the call returns, on every exit path, with
//   the multiples of delta derived from them; the host copies are wiped likewise (as pwtau.hip treats its secrets).
//   Routing: above BATCH_MAX_DOMAIN or below BATCH_MIN proofs the call loops the single prover (report: batched = 0).
#include <string.h>

#include "keybytes.h"

namespace wsnark {

// ---- device ----
struct SpmvBatch { const uint32_t* row_ptr[2]; const uint32_t* col[2]; const Fe* coef[2]; Fe* res[2]; const uint8_t* sig; uint64_t sig_stride; };
__global__ __launch_bounds__(256) void lc_spmv2_batch_kernel(SpmvBatch M, uint32_t n_rows) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const uint32_t m = blockIdx.y, p = blockIdx.z;
    const uint32_t* __restrict__ row_ptr = M.row_ptr[m];
    const Fe* __restrict__ sig = reinterpret_cast<const Fe*>(M.sig + (uint64_t)p * M.sig_stride);
    M.res[m][(uint64_t)p * n_rows + r] = lc_row_dot(M.coef[m], M.col[m], sig, row_ptr[r], row_ptr[r + 1]);
}

// h[p][t] = fromMontgomery((e[p][t] - w_2n^-t o[p][t]) / 2): dist_combine_kernel (calch.hip) with log_n1 = 0, over `total` = proofs x n
__global__ __launch_bounds__(256) void batch_combine_kernel(const Fe* __restrict__ e, const Fe* __restrict__ o, Fe* __restrict__ h, uint64_t total,
                                                              uint32_t log_n, const Fe* __restrict__ cs_lo, const Fe* __restrict__ cs_hi, uint32_t hc, Fe half) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const uint64_t t = idx & (((uint64_t)1 << log_n) - 1);
    Fe v;
    if (t == 0) {
        v = Fr::sub(e[idx], o[idx]);
    } else {
        const uint64_t x = ((uint64_t)1 << log_n) - t;
        v = Fr::add(e[idx], Fr::mul(Fr::mul(cs_hi[x >> hc], cs_lo[x & (((uint64_t)1 << hc) - 1)]), o[idx]));
    }
    h[idx] = Fr::from_mont(Fr::mul(v, half));
}

constexpr uint32_t kBatchLanes = 256;        // lanes of a workgroup = bucket slots of a window (c <= 8)
constexpr uint32_t kBatchPieces = 512;       // piece slots per workgroup (at most 255 + 256 are used)
constexpr uint32_t kBatchFold = 288;         // 256 bucket sums, 16 weighted block sums, 16 block sums

struct BatchSum { const void* points; const uint8_t* scalars; uint64_t stride; uint32_t n; };      // proof p's scalars: scalars + p x stride bytes
struct BatchArgs {
    BatchSum s[4];
    uint32_t c, nwin;
    uint32_t* idx; uint64_t idx_stride;      // per workgroup: idx_stride entries
    void* part;                              // per workgroup: kBatchPieces points (internal form)
    void* fold;                              // per workgroup: kBatchFold points
    void* win;                               // [proof][sum][window], reference format
};

__device__ __forceinline__ uint32_t batch_digit(const uint8_t* scalars, uint32_t i, uint32_t lo, uint32_t c) {
    const uint64_t* q = reinterpret_cast<const uint64_t*>(scalars + (uint64_t)i * 32);
    const uint32_t word = lo >> 6, sh = lo & 63;
    uint64_t v = q[word] >> sh;
    if (sh + c > 64 && word < 3) v |= q[word + 1] << (64 - sh);
    return (uint32_t)v & ((1u << c) - 1);
}

template <class C>
__global__ __launch_bounds__(256) void batch_buckets_kernel(BatchArgs A) {
    typedef typename C::Field F;
    typedef typename C::Pt Pt;
    typedef typename C::PtP PtP;
    typedef typename C::AffP AffP;
    __shared__ uint32_t cnt[kBatchLanes], off[kBatchLanes], cur[kBatchLanes], tstart[kBatchLanes + 1];
    __shared__ uint32_t s_cap;
    const uint32_t l = threadIdx.x, w = blockIdx.x, k = blockIdx.y, p = blockIdx.z;
    const uint64_t wg = ((uint64_t)p * gridDim.y + k) * gridDim.x + w;
    const AffP* __restrict__ points = reinterpret_cast<const AffP*>(A.s[k].points);
    const uint8_t* __restrict__ scalars = A.s[k].scalars + (uint64_t)p * A.s[k].stride;
    const uint32_t n = A.s[k].n, c = A.c, lo = w * c;
    uint32_t* __restrict__ idx = A.idx + wg * A.idx_stride;
    PtP* __restrict__ part = reinterpret_cast<PtP*>(A.part) + wg * kBatchPieces;
    PtP* __restrict__ fold = reinterpret_cast<PtP*>(A.fold) + wg * kBatchFold;

    // 1. counting sort of the non-zero digits
    cnt[l] = 0;
    __syncthreads();
    for (uint32_t i = l; i < n; i += kBatchLanes) {
        const uint32_t d = batch_digit(scalars, i, lo, c);
        if (d) atomicAdd(&cnt[d], 1u);
    }
    __syncthreads();
    if (l == 0) {
        uint32_t run = 0;
        for (uint32_t d = 0; d < kBatchLanes; d++) { off[d] = cur[d] = run; run += cnt[d]; }
        const uint32_t cap = run ? (run + kBatchLanes - 1) / kBatchLanes : 1;
        uint32_t t = 0;
        for (uint32_t d = 0; d < kBatchLanes; d++) { tstart[d] = t; t += (cnt[d] + cap - 1) / cap; }
        tstart[kBatchLanes] = t;      // <= 255 + 256
        s_cap = cap;
    }
    __syncthreads();
    for (uint32_t i = l; i < n; i += kBatchLanes) {
        const uint32_t d = batch_digit(scalars, i, lo, c);
        if (d) idx[atomicAdd(&cur[d], 1u)] = i;
    }
    __syncthreads();

    // 2. the pieces: piece t belongs to the bucket d with tstart[d] <= t < tstart[d + 1]
    const uint32_t cap = s_cap, T = tstart[kBatchLanes];
    for (uint32_t t = l; t < T; t += kBatchLanes) {
        uint32_t a = 0, b = kBatchLanes;
        while (b - a > 1) { const uint32_t mid = (a + b) >> 1; if (tstart[mid] <= t) a = mid; else b = mid; }
        const uint32_t first = off[a] + (t - tstart[a]) * cap, end = off[a] + cnt[a];
        const uint32_t last = first + cap < end ? first + cap : end;
        Pt acc = C::infinity();
        for (uint32_t j = first; j < last; j++) {
            const AffP cp = points[idx[j]];
            if (F::packed_is_zero(cp.x)) continue;      // the key's points at infinity
            const typename C::Aff cur_pt = C::unpack_aff(cp);
            if (C::is_inf(acc) || !C::madd_fast(acc, cur_pt, false)) C::madd_wide(acc, cur_pt, false);
        }
        C::narrow_x(acc);
        part[t] = C::pack_pt(acc);
    }
    __syncthreads();

    // 3. bucket d = the sum of its pieces (bucket 0 and the empty ones: infinity)
    {
        Pt S = C::infinity();
        for (uint32_t t = tstart[l]; t < tstart[l + 1]; t++) S = C::add(S, C::unpack_pt(part[t]));
        fold[l] = C::pack_pt(S);
    }
    __syncthreads();

    // 4. sum_d d S_d.  Level 1: lane j takes the buckets [16 j, 16 j + 16): wj = sum (d - 16 j) S_d, run = sum S_d
    if (l < 16) {
        Pt run = C::infinity(), wj = C::infinity();
        for (uint32_t d = 16 * l + 16; d-- > 16 * l;) {
            wj = C::add(wj, run);
            run = C::add(run, C::unpack_pt(fold[d]));
        }
        fold[256 + l] = C::pack_pt(wj);
        fold[272 + l] = C::pack_pt(run);
    }
    __syncthreads();
    // level 2: sum_j wj + 16 sum_j j run_j
    if (l == 0) {
        Pt run = C::infinity(), t2 = C::infinity();
        for (uint32_t j = 16; j-- > 0;) {
            t2 = C::add(t2, run);
            run = C::add(run, C::unpack_pt(fold[272 + j]));
        }
        for (int i = 0; i < 4; i++) t2 = C::dbl(t2);
        for (uint32_t j = 0; j < 16; j++) t2 = C::add(t2, C::unpack_pt(fold[256 + j]));
        reinterpret_cast<PtP*>(A.win)[wg] = C::pt_from_internal(t2);
    }
}

// sums[i] = sum_w 2^(c w) win[i][w], one lane per (proof, sum); saturated field, reference format
template <class G>
__global__ __launch_bounds__(256) void batch_horner_kernel(const typename G::Pt* __restrict__ win, uint32_t lanes, uint32_t c, uint32_t nwin,
                                                             typename G::Pt* __restrict__ sums) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= lanes) return;
    const typename G::Pt* W = win + (uint64_t)i * nwin;
    typename G::Pt acc = W[nwin - 1];
#pragma unroll 1
    for (uint32_t w = nwin - 1; w-- > 0;) {
#pragma unroll 1
        for (uint32_t b = 0; b < c; b++) acc = G::dbl(acc);
        acc = G::add(acc, W[w]);
    }
    sums[i] = acc;
}

// out[i] = sc[3 (i / per) + first + i % per] x base: G1 (per 3, first 0): r delta1, s delta1, rs delta1; G2 (per 1, first 1): s delta2
template <class G>
__global__ __launch_bounds__(256) void batch_fixed_kernel(typename G::Aff base, const Fe* __restrict__ sc, uint32_t lanes, uint32_t per, uint32_t first,
                                                            typename G::Pt* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= lanes) return;
    const Fe k = sc[3 * (uint64_t)(i / per) + first + i % per];
    out[i] = G::mul_bytes(G::from_affine(base), reinterpret_cast<const uint8_t*>(&k), 32);
}

// lane 2 p: pi_a = sum A + alfa1 + r delta1, s pi_a; lane 2 p + 1: pib1 = sum B1 + beta1 + s delta1, r pib1   (src/bn128.js:671-696)
// sums1: [proof][A, B1, C, H]; fixed1: [proof][r delta1, s delta1, rs delta1]; mid: [proof][pi_a, s pi_a, r pib1]
__global__ __launch_bounds__(256) void batch_mid_kernel(Affine<Fq> alfa1, Affine<Fq> beta1, const G1::Pt* __restrict__ sums1, const G1::Pt* __restrict__ fixed1,
                                                          const Fe* __restrict__ sc, uint32_t count, G1::Pt* __restrict__ mid) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * count) return;
    const uint32_t p = i >> 1, j = i & 1;
    const G1::Pt q = G1::add(G1::add(G1::from_affine(j ? beta1 : alfa1), sums1[4 * (uint64_t)p + j]), fixed1[3 * (uint64_t)p + j]);
    const Fe k = sc[3 * (uint64_t)p + (j ? 0 : 1)];
    if (j == 0) mid[3 * (uint64_t)p] = q;
    mid[3 * (uint64_t)p + 1 + j] = G1::mul_bytes(q, reinterpret_cast<const uint8_t*>(&k), 32);
}

// one lane per proof: pi_b, pi_c, affine + fromMontgomery (src/bn128.js:676-712; prove.hip: prove_assemble)
__global__ __launch_bounds__(256) void batch_final_kernel(Affine<Fq2> beta2, const G1::Pt* __restrict__ sums1, const G2::Pt* __restrict__ sums2,
                                                            const G1::Pt* __restrict__ fixed1, const G2::Pt* __restrict__ fixed2,
                                                            const G1::Pt* __restrict__ mid, uint32_t count, Fe* __restrict__ out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= count) return;
    const G2::Pt pi_b = G2::add(G2::add(G2::from_affine(beta2), sums2[p]), fixed2[p]);
    G1::Pt pi_c = G1::add(sums1[4 * (uint64_t)p + 2], sums1[4 * (uint64_t)p + 3]);
    pi_c = G1::add(pi_c, mid[3 * (uint64_t)p + 1]);
    pi_c = G1::add(pi_c, mid[3 * (uint64_t)p + 2]);
    pi_c = G1::add(pi_c, G1::neg(fixed1[3 * (uint64_t)p + 2]));
    const Jac<Fq> a = G1::to_affine_jac(mid[3 * (uint64_t)p]), cc = G1::to_affine_jac(pi_c);
    const Jac<Fq2> b = G2::to_affine_jac(pi_b);
    Fe* o = out + 12 * (uint64_t)p;
    o[0] = Fq::from_mont(a.x); o[1] = Fq::from_mont(a.y); o[2] = Fq::from_mont(a.z);
    o[3] = Fq::from_mont(b.x.c0); o[4] = Fq::from_mont(b.x.c1);
    o[5] = Fq::from_mont(b.y.c0); o[6] = Fq::from_mont(b.y.c1);
    o[7] = Fq::from_mont(b.z.c0); o[8] = Fq::from_mont(b.z.c1);
    o[9] = Fq::from_mont(cc.x); o[10] = Fq::from_mont(cc.y); o[11] = Fq::from_mont(cc.z);
}

// ---- host ----
namespace {
struct HostSecret {
    std::vector<uint8_t> rs;      // count x (r | s), raw
    std::vector<Fe> sc;           // count x (r mod r, s mod r, rs mod r), plain
    ~HostSecret() {
        if (!rs.empty()) wipe(rs.data(), rs.size());
        if (!sc.empty()) wipe(sc.data(), sc.size() * sizeof(Fe));
    }
};
// the device copy of the chunk's scalars and what is derived from them alone: overwritten on the call's queue when this goes
struct DeviceSecret {
    hipStream_t s = nullptr;
    void* p = nullptr;
    size_t bytes = 0;
    ~DeviceSecret() {
        if (!p) return;
        (void)hipMemsetAsync(p, 0, bytes, s);
        (void)hipStreamSynchronize(s);      // (also the error paths: nothing of this call is in flight when the lane goes back)
    }
};

constexpr size_t kBatchBudget = (size_t)2 << 30;      // scratch of one pass
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the pass's scratch, carved out of the lane's grow-only buffer
struct BatchBufs {
    uint8_t *w, *ab, *e, *h, *idx, *part1, *fold1, *part2, *fold2, *win1, *win2, *sums1, *sums2, *out, *secret;
    uint8_t *sc, *fixed1, *fixed2, *mid;      // inside `secret`
    size_t secret_bytes, total;
};
// (base as an integer: the sizes are asked for with base 0, and offsets from a null POINTER would be undefined)
BatchBufs batch_layout(uintptr_t base, uint64_t B, uint64_t nv, uint64_t dom, uint32_t nwin, bool own_w) {
    BatchBufs L;
    size_t off = 0;
    auto take = [&](size_t bytes) { uint8_t* p = reinterpret_cast<uint8_t*>(base + off); off += up256(bytes); return p; };
    const uint64_t nmax = nv > dom ? nv : dom, wg1 = B * 4 * nwin, wg2 = B * nwin;
    L.w = take(own_w ? B * nv * 32 : 0);
    L.ab = take(2 * B * dom * 32);
    L.e = take(B * dom * 32);
    L.h = take(B * dom * 32);
    L.idx = take((wg1 + wg2) * nmax * 4);
    L.part1 = take(wg1 * kBatchPieces * 128);
    L.fold1 = take(wg1 * kBatchFold * 128);
    L.part2 = take(wg2 * kBatchPieces * 256);
    L.fold2 = take(wg2 * kBatchFold * 256);
    L.win1 = take(wg1 * 128);
    L.win2 = take(wg2 * 256);
    L.sums1 = take(B * 4 * 128);
    L.sums2 = take(B * 256);
    L.out = take(B * 384);
    const size_t secret_off = off;
    L.secret = reinterpret_cast<uint8_t*>(base + off);
    L.sc = take(B * 96);
    L.fixed1 = take(B * 3 * 128);
    L.fixed2 = take(B * 256);
    L.mid = take(B * 3 * 128);
    L.secret_bytes = off - secret_off;
    L.total = off;
    return L;
}

int check_hip_launch() { WS_HIP_CHECK(hipGetLastError()); return WS_OK; }

// one pass: proofs [0, B) of the chunk, their witnesses resident at d_w (stride bytes apart); proofs into tmp_out
int batch_pass(ProvingKey* K, Lane& L, hipStream_t s, const BatchBufs& U, const uint8_t* d_w, uint64_t w_stride, uint32_t B, uint32_t c,
               const Fe* sc_host, uint8_t* out_host, hipEvent_t* ev) {
    Context* X = K->owner;
    KernelTimer& T = X->timer;
    const uint32_t nv = K->n_vars, dom = K->domain, nwin = (256 + c - 1) / c;
    const int bits = (int)ceil_log2(dom);
    int rc;
    // the scalars first: the multiples of delta need nothing else
    WS_HIP_CHECK(hipMemcpyAsync(U.sc, sc_host, (size_t)B * 96, hipMemcpyHostToDevice, s));

    // ---- CALC_H of the chunk (calch.hip: calc_h_dev, every step over the stack) ----
    Fe* a = reinterpret_cast<Fe*>(U.ab);
    Fe* b = a + (uint64_t)B * dom;
    Fe* e = reinterpret_cast<Fe*>(U.e);
    Fe* h = reinterpret_cast<Fe*>(U.h);
    // BATCH_STACK (A/B): bit 0 = the sparse products of all proofs in one launch, bit 1 = the transforms of all
    // proofs in one launch per pass; cleared, the proofs go through the single prover's own launches one after the other
    const long stack_sw = tuning_get("BATCH_STACK", 3);
    T.begin("batch_spmv", s);
    if (stack_sw & 1) {
        const CsrMatrix &MA = K->polsA, &MB = K->polsB;
        const SpmvBatch M{{MA.row_ptr.as<uint32_t>(), MB.row_ptr.as<uint32_t>()}, {MA.col.as<uint32_t>(), MB.col.as<uint32_t>()},
                          {MA.coef.as<Fe>(), MB.coef.as<Fe>()}, {a, b}, d_w, w_stride};
        hipLaunchKernelGGL(lc_spmv2_batch_kernel, dim3(ceil_div_u64(dom, 256), 2, B), dim3(256), 0, s, M, dom);
    } else {
        for (uint32_t p = 0; p < B; p++)
            if ((rc = eval_ab_dev(L, reinterpret_cast<const Fe*>(d_w + (uint64_t)p * w_stride), nv, K->polsA, K->polsB, dom, a + (uint64_t)p * dom,
                                  b + (uint64_t)p * dom, s))) return rc;
    }
    T.end(s);
    if ((rc = check_hip_launch())) return rc;
    auto transforms = [&](Fe* d, int odd, int inverse, uint64_t cnt) -> int {
        if (stack_sw & 2) return ntt_dev(L, d, dom, odd, inverse, s, cnt);
        for (uint64_t i = 0; i < cnt; i++)
            if (int r = ntt_dev(L, d + i * dom, dom, odd, inverse, s, 1)) return r;
        return WS_OK;
    };
    // (the transforms' product-on-load reads its second operand without the batch offset: the products are fr_mul_dev's)
    const uint64_t stack = (uint64_t)B * dom;
    if ((rc = fr_mul_dev(a, b, e, stack, s))) return rc;
    if ((rc = transforms(e, 0, 1, B))) return rc;                            // e = iNTT(A.B)
    if ((rc = transforms(a, 0, 1, 2 * (uint64_t)B))) return rc;              // evaluations -> coefficients (a, b)
    if ((rc = transforms(a, 1, 0, 2 * (uint64_t)B))) return rc;              // -> odd-coset evaluations
    if ((rc = fr_mul_dev(a, b, a, stack, s))) return rc;
    if ((rc = transforms(a, 0, 1, B))) return rc;                            // o = iNTT(A.B on the coset)
    {
        const Fe *lo, *hi;
        int hc;
        Fe n_inv;
        if ((rc = ntt_coset_tables(bits, &lo, &hi, &hc, &n_inv, s))) return rc;
        const Fe half = Fr::inv(Fr::add(Fr::one(), Fr::one()));
        const uint64_t total = (uint64_t)B * dom;
        T.begin("batch_combine", s);
        hipLaunchKernelGGL(batch_combine_kernel, dim3(ceil_div_u64(total, 256)), dim3(256), 0, s, e, a, h, total, (uint32_t)bits, lo, hi, (uint32_t)hc, half);
        T.end(s);
        if ((rc = check_hip_launch())) return rc;
    }
    if (ev) WS_HIP_CHECK(hipEventRecord(ev[2], s));

    // ---- the five sums ----
    const uint64_t nmax = nv > dom ? nv : dom;
    BatchArgs A1, A2;
    memset(&A1, 0, sizeof A1);
    memset(&A2, 0, sizeof A2);
    A1.s[0] = BatchSum{K->pointsA.p, d_w, w_stride, nv};
    A1.s[1] = BatchSum{K->pointsB1.p, d_w, w_stride, nv};
    A1.s[2] = BatchSum{K->pointsC.p, d_w, w_stride, nv};
    A1.s[3] = BatchSum{K->pointsH.p, U.h, (uint64_t)dom * 32, dom};
    A1.c = c; A1.nwin = nwin; A1.idx = reinterpret_cast<uint32_t*>(U.idx); A1.idx_stride = nmax;
    A1.part = U.part1; A1.fold = U.fold1; A1.win = U.win1;
    A2.s[0] = BatchSum{K->pointsB2.p, d_w, w_stride, nv};
    A2.c = c; A2.nwin = nwin; A2.idx = reinterpret_cast<uint32_t*>(U.idx) + (uint64_t)B * 4 * nwin * nmax; A2.idx_stride = nmax;
    A2.part = U.part2; A2.fold = U.fold2; A2.win = U.win2;
    T.begin("batch_buckets_g2", s);
    hipLaunchKernelGGL((batch_buckets_kernel<G2R29>), dim3(nwin, 1, B), dim3(kBatchLanes), 0, s, A2);
    T.end(s);
    if ((rc = check_hip_launch())) return rc;
    T.begin("batch_buckets_g1", s);
    hipLaunchKernelGGL((batch_buckets_kernel<G1R29>), dim3(nwin, 4, B), dim3(kBatchLanes), 0, s, A1);
    T.end(s);
    if ((rc = check_hip_launch())) return rc;
    G1::Pt *sums1 = reinterpret_cast<G1::Pt*>(U.sums1), *fixed1 = reinterpret_cast<G1::Pt*>(U.fixed1), *mid = reinterpret_cast<G1::Pt*>(U.mid);
    G2::Pt *sums2 = reinterpret_cast<G2::Pt*>(U.sums2), *fixed2 = reinterpret_cast<G2::Pt*>(U.fixed2);
    T.begin("batch_horner", s);
    hipLaunchKernelGGL((batch_horner_kernel<G2>), dim3(ceil_div_u64(B, 256)), dim3(256), 0, s, reinterpret_cast<const G2::Pt*>(U.win2), B, c, nwin, sums2);
    hipLaunchKernelGGL((batch_horner_kernel<G1>), dim3(ceil_div_u64(4 * (uint64_t)B, 256)), dim3(256), 0, s, reinterpret_cast<const G1::Pt*>(U.win1), 4 * B, c, nwin, sums1);
    T.end(s);
    if ((rc = check_hip_launch())) return rc;
    if (ev) WS_HIP_CHECK(hipEventRecord(ev[3], s));

    // ---- assembly ----
    const Fe* d_sc = reinterpret_cast<const Fe*>(U.sc);
    T.begin("batch_assemble", s);
    hipLaunchKernelGGL((batch_fixed_kernel<G2>), dim3(ceil_div_u64(B, 256)), dim3(256), 0, s, K->delta2, d_sc, B, 1u, 1u, fixed2);
    hipLaunchKernelGGL((batch_fixed_kernel<G1>), dim3(ceil_div_u64(3 * (uint64_t)B, 256)), dim3(256), 0, s, K->delta1, d_sc, 3 * B, 3u, 0u, fixed1);
    hipLaunchKernelGGL(batch_mid_kernel, dim3(ceil_div_u64(2 * (uint64_t)B, 256)), dim3(256), 0, s, K->alfa1, K->beta1, sums1, fixed1, d_sc, B, mid);
    hipLaunchKernelGGL(batch_final_kernel, dim3(ceil_div_u64(B, 256)), dim3(256), 0, s, K->beta2, sums1, sums2, fixed1, fixed2, mid, B, reinterpret_cast<Fe*>(U.out));
    T.end(s);
    if ((rc = check_hip_launch())) return rc;
    WS_HIP_CHECK(hipMemcpyAsync(out_host, U.out, (size_t)B * 384, hipMemcpyDeviceToHost, s));
    if (ev) WS_HIP_CHECK(hipEventRecord(ev[4], s));
    // the scalars and their multiples of delta go before the next pass (or the return) reuses the buffer
    WS_HIP_CHECK(hipMemsetAsync(U.secret, 0, U.secret_bytes, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    return WS_OK;
}
}  // namespace

int groth16_prove_batch(ProvingKey* K, const void* witnesses, size_t witness_stride, uint64_t count, bool on_device, const uint8_t* r32s,
                        const uint8_t* s32s, uint8_t* out384s, uint8_t* out_rs64s, wsnark_prove_batch_report_t* rep, hipStream_t stream) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (!K) return WS_ERR_ARG;
    if (count == 0) return WS_OK;
    if (!witnesses || !out384s) return WS_ERR_ARG;
    if (count > ((uint64_t)1 << 16)) { set_last_error("prove_batch: more than 2^16 proofs in one call"); return WS_ERR_SIZE; }
    if (K->shard_world > 1 || K->h_log_m) { set_last_error("prove_batch: this handle holds a shard of the key (whole keys only)"); return WS_ERR_ARG; }
    const uint32_t nv = K->n_vars, dom = K->domain;
    if (witness_stride < (size_t)nv * 32) { set_last_error("prove_batch: witness_stride is less than nVars*32 bytes"); return WS_ERR_SIZE; }
    if (on_device && (((uintptr_t)witnesses | (uintptr_t)witness_stride) % 16)) {
        set_last_error("prove_batch: the device witnesses must be 16-byte aligned (pointer and stride)");
        return WS_ERR_ARG;
    }
    const long c_sw = tuning_get("BATCH_WINDOW", 8);
    if (c_sw < 4 || c_sw > 8) { set_last_error("prove_batch: BATCH_WINDOW must be in [4, 8]"); return WS_ERR_ARG; }
    const uint32_t c = (uint32_t)c_sw, nwin = (256 + c - 1) / c;
    const auto t_call = Clock::now();

    // the blinding values: the caller's, else one independent draw per proof
    HostSecret H;
    H.rs.resize((size_t)count * 64);
    if ((!r32s || !s32s) && os_random(H.rs.data(), H.rs.size())) { set_last_error("no entropy: getrandom(2) and /dev/urandom both failed"); return WS_ERR_ARG; }
    for (uint64_t i = 0; i < count; i++) {
        if (r32s) memcpy(&H.rs[(size_t)i * 64], r32s + i * 32, 32);
        if (s32s) memcpy(&H.rs[(size_t)i * 64 + 32], s32s + i * 32, 32);
    }
    std::vector<uint8_t> held((size_t)count * 384);      // the outputs stay untouched behind an error
    wsnark_prove_batch_report_t R;
    memset(&R, 0, sizeof R);
    R.count = count;
    R.window_bits = c;
    const uint8_t* wb = reinterpret_cast<const uint8_t*>(witnesses);

    // ---- routing ----
    // The defaults are the measured crossover (profiles/prove_batch_bench.json): a pass costs ~50 ms of dependent additions
    // whatever the batch, so the batch path beat the two-thread loop of the single prover only at 2^10 and from 64 proofs on.
    const bool batch = (uint64_t)dom <= (uint64_t)tuning_get("BATCH_MAX_DOMAIN", 1 << 10) && count >= (uint64_t)tuning_get("BATCH_MIN", 64) && dom <= (1u << 16);
    if (!batch) {
        for (uint64_t i = 0; i < count; i++) {
            const uint8_t *wi = wb + i * witness_stride, *ri = &H.rs[(size_t)i * 64], *si = ri + 32;
            const int rc = on_device ? groth16_prove_dev_witness(K, reinterpret_cast<const Fe*>(wi), (size_t)nv * 32, ri, si, &held[(size_t)i * 384], stream)
                                     : groth16_prove_host_witness(K, wi, (size_t)nv * 32, ri, si, &held[(size_t)i * 384]);
            if (rc) return rc;
        }
        R.chunk = 1;
        R.ms[4] = ms_since(t_call);
    } else {
        H.sc.resize((size_t)count * 3);
        for (uint64_t i = 0; i < count; i++) {
            Fe rr, ss;
            memcpy(&rr, &H.rs[(size_t)i * 64], 32);
            memcpy(&ss, &H.rs[(size_t)i * 64 + 32], 32);
            rr = Fr::reduce_full(rr);
            ss = Fr::reduce_full(ss);
            H.sc[(size_t)i * 3] = rr;
            H.sc[(size_t)i * 3 + 1] = ss;
            H.sc[(size_t)i * 3 + 2] = Fr::from_mont(Fr::mul(Fr::to_mont(rr), Fr::to_mont(ss)));
            wipe(&rr, sizeof rr);
            wipe(&ss, sizeof ss);
        }
        // proofs per pass: what keeps the scratch under the budget (BATCH_CHUNK overrides), and the transforms' stack under 2^30 elements
        const size_t per_proof = batch_layout(0, 1, nv, dom, nwin, !on_device).total;
        uint64_t chunk = (uint64_t)tuning_get("BATCH_CHUNK", 0);
        if (!chunk) chunk = std::max<uint64_t>(kBatchBudget / per_proof, 1);
        chunk = std::min<uint64_t>(std::min<uint64_t>(chunk, count), std::min<uint64_t>(((uint64_t)1 << 29) / dom, 32767));
        LaneLock L = acquire_lane(X);
        hipStream_t s = stream ? stream : L->stream;
        const BatchBufs probe = batch_layout(0, chunk, nv, dom, nwin, !on_device);
        WS_HIP_CHECK(L->batch_ws.reserve(probe.total + 256));
        const BatchBufs U = batch_layout(reinterpret_cast<uintptr_t>(L->batch_ws.p), chunk, nv, dom, nwin, !on_device);
        DeviceSecret guard;
        guard.s = s; guard.p = U.secret; guard.bytes = U.secret_bytes;
        hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int i = 0; i < 5; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } ev_guard{ev};
        if (rep) for (auto& e : ev) WS_HIP_CHECK(hipEventCreate(&e));
        for (uint64_t i0 = 0; i0 < count; i0 += chunk) {
            const uint32_t B = (uint32_t)std::min<uint64_t>(chunk, count - i0);
            if (rep) WS_HIP_CHECK(hipEventRecord(ev[0], s));
            const uint8_t* d_w = wb + i0 * witness_stride;
            uint64_t w_stride = witness_stride;
            if (!on_device) {
                // through the staging ring: in one piece when the witnesses are packed, else one after the other
                int rc = WS_OK;
                if (witness_stride == (size_t)nv * 32) rc = upload_staged(U.w, d_w, (size_t)B * nv * 32, s);
                else for (uint32_t j = 0; j < B && !rc; j++) rc = upload_staged(U.w + (size_t)j * nv * 32, d_w + (size_t)j * witness_stride, (size_t)nv * 32, s);
                if (rc) return rc;
                d_w = U.w;
                w_stride = (uint64_t)nv * 32;
            }
            if (rep) WS_HIP_CHECK(hipEventRecord(ev[1], s));
            const int rc = batch_pass(K, *L, s, U, d_w, w_stride, B, c, &H.sc[(size_t)i0 * 3], &held[(size_t)i0 * 384], rep ? ev : nullptr);
            if (rc) return rc;
            if (rep) {
                for (int k = 0; k < 4; k++) {
                    float ms = 0.f;
                    WS_HIP_CHECK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
                    R.ms[k] += ms;
                }
            }
        }
        R.batched = count;
        R.chunk = (uint32_t)chunk;
        R.ms[4] = ms_since(t_call);
    }
    // nothing can fail from here on
    memcpy(out384s, held.data(), held.size());
    if (out_rs64s) memcpy(out_rs64s, H.rs.data(), H.rs.size());
    if (rep) *rep = R;
    return WS_OK;
}

}  // namespace wsnark
