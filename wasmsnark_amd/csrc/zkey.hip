// zkey.hip -- snarkjs' .zkey in and out (wsnark_zkey_info, wsnark_zkey_import*, wsnark_zkey_export*), straight into a resident proving
// key (wsnark_pkey_load_zkey*: zkey_load at the end of this file) and the basis change of the H section (wsnark_g1_h_basis);
// include/wsnark.h has the contracts, README.md section "zkey" the file format as this file reads it.
//
// A .zkey is no re-packing of proving_key.bin: two of its sections are in another form.
//   H.  Section 9 holds N_i = (L^{2n}_{2i+1}(tau) / delta) G1, the odd Lagrange points of the doubled domain; CALC_H's sum
//     (src/bn128.js:126-166) wants hExps_k = (tau^k (tau^n - 1) / delta) G1.  A polynomial P of degree < 2n that vanishes on the
//     n-domain is P(tau) = sum_i P(x_i) L^{2n}_{2i+1}(tau), x_i = w_2n^(2i+1); P = x^k (x^n - 1) has P(x_i) = -2 x_i^k, so
//         hExps_k = (-2 w_2n^k) sum_i w_n^(ik) N_i            N_i = sum_k w_n^(-ik) (-(2n)^-1 w_2n^(-k)) hExps_k.
//     Both are the group transform of pkeysetup.hip (load, stages) and one scalar per point (pwtau.hip: fr_powers_kernel for c t^k,
//     mul_points_kernel), the scalars BEHIND the stages on the way in and IN FRONT of them on the way out, where they carry the
//     inverse's 1/n: the scale_points pass of wsnark_g1_ntt(inverse) is not run.  The points stay on the device in between.  No kernel
//     of those files is copied: keybytes.h has their launchers.  The scalars are public: nothing is wiped.
//   Coefficients.  Section 4 is one list of (matrix, constraint, signal, c R^2) records in constraint order, A and B interleaved; a
//     key holds one column stream per matrix with c R.
//       zk_count_kernel      a tile's records of matrix 0 (a count is a sum: LDS atomics), and the three tests no host loop makes:
//                            matrix > 1, signal >= nVars, constraint >= domainSize, each the SMALLEST bad record by a min-reduction
//       scan_exclusive_dev   the tiles' bases
//       zk_partition_kernel  the STABLE partition by matrix: lane l of a tile owns records [l K, l K + K) of it, counts its records of
//                            matrix 0, one exclusive scan over the 256 counts ranks the lane inside the tile, and the lane walks its
//                            records again in order: matrix 0 goes to base0[tile] + rank, matrix 1 to (records before the tile -
//                            base0[tile]) + (records before it in the tile - rank).  No order comes from an atomic.  The value
//                            leaves with both Montgomery factors taken off (c, canonical): rows_emit_kernel puts one back.
//       zk_order_kernel      was every matrix's constraint column non-decreasing?  (a flag, not an order)
//       then circuitrows.hip's stable radix sort of (signal, entry) pairs and its emit, entered with these device-resident arrays;
//       where the flag says no, passes over the constraint bits run first and zk_keys_kernel re-keys the pairs by signal: two stable
//       sorts, least significant key first.
//     Out: the two streams' records are ONE array of entries in stream order (A's, then B's: ascending signal, stream order inside a
//     signal), stably sorted by constraint with the same sort -- which is section 4's order -- and zk_emit_kernel stages 256 records of
//     11 words in LDS (value times R) and stores them with 32-bit stores in output order.  (The row-major transposition of calch.hip
//     fills its rows through atomic cursors: the order inside a row would be the atomics', so it is not used here.)
#include <string.h>

#include "keybytes.h"

namespace wsnark {

// ---- device ----
// ~index of the smallest bad record per test (0 = none), the records >= r per matrix, and whether a matrix's constraints decrease
// (zero[]: the values that are 0 mod r, counted by the partition of the resident path alone -- the import's come from its emit)
struct ZkAcc { unsigned long long bad_matrix, bad_signal, bad_constraint, unreduced[2], unsorted[2], zero[2]; };
static constexpr uint32_t kRecWords = 11;      // u32 matrix, u32 constraint, u32 signal, 8 words of value

__global__ __launch_bounds__(256) void zk_count_kernel(const uint32_t* __restrict__ rec, uint32_t n, uint32_t tile, uint32_t n_vars, uint32_t domain,
                                                       uint32_t* __restrict__ tile_cnt0, ZkAcc* __restrict__ acc) {
    __shared__ uint32_t cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const uint64_t e0 = (uint64_t)blockIdx.x * tile, e1 = e0 + tile < n ? e0 + tile : n;
    uint32_t mine = 0;
    for (uint64_t e = e0 + threadIdx.x; e < e1; e += 256) {
        const uint32_t m = rec[kRecWords * e], c = rec[kRecWords * e + 1], sg = rec[kRecWords * e + 2];
        mine += m == 0;
        if (m > 1) atomicMax(&acc->bad_matrix, ~(unsigned long long)e);
        if (sg >= n_vars) atomicMax(&acc->bad_signal, ~(unsigned long long)e);
        if (c >= domain) atomicMax(&acc->bad_constraint, ~(unsigned long long)e);
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt0[blockIdx.x] = cnt;
}

// base0[t]: matrix 0's records before tile t.  per_lane = tile / 256.  sig / row / coef: the two matrices' arrays, n0 and n - n0 long.
// kKeep (the resident path, zkey_load): the value stays as the file has it, c R^2 -- what the prover's CSR holds (calch.hip) -- reduced
// below r where it is not, and the zero values are counted here.
struct ZkParts { uint32_t* sig[2]; uint32_t* row[2]; Fe* coef[2]; };
template <bool kKeep>
__global__ __launch_bounds__(256) void zk_partition_kernel(const uint32_t* __restrict__ rec, uint32_t n, uint32_t per_lane,
                                                           const uint32_t* __restrict__ base0, ZkParts out, ZkAcc* __restrict__ acc) {
    __shared__ uint32_t part[256];
    const uint64_t rmod[4] = {FrParams::P0, FrParams::P1, FrParams::P2, FrParams::P3};
    const uint32_t l = threadIdx.x;
    const uint64_t tile0 = (uint64_t)blockIdx.x * 256 * per_lane, t0 = tile0 + (uint64_t)l * per_lane;
    const uint64_t e0 = t0 < n ? t0 : n, e1 = t0 + per_lane < n ? t0 + per_lane : n;
    uint32_t zeros = 0;
    for (uint64_t e = e0; e < e1; e++) zeros += rec[kRecWords * e] == 0;
    part[l] = zeros;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t x = l >= d ? part[l - d] : 0;
        __syncthreads();
        part[l] += x;
        __syncthreads();
    }
    const uint32_t b0 = base0[blockIdx.x];
    uint64_t p0 = (uint64_t)b0 + part[l] - zeros;                      // matrix 0: records before this lane's run
    uint64_t p1 = (tile0 - b0) + ((e0 - tile0) - (part[l] - zeros));   // matrix 1 (e0 >= tile0: a lane past the end has an empty run)
    uint32_t big0 = 0, big1 = 0, zero0 = 0, zero1 = 0;
    for (uint64_t e = e0; e < e1; e++) {
        const uint32_t* w = rec + kRecWords * e;
        const bool m = (w[0] & 1) != 0;                                // (matrix > 1 fails the call before anything is read back)
        Fe v;
        for (int k = 0; k < 4; k++) v.l[k] = (uint64_t)w[3 + 2 * k] | ((uint64_t)w[4 + 2 * k] << 32);
        const bool ge = pk_ge(v, rmod);
        big0 += (!m && ge) ? 1u : 0u;
        big1 += (m && ge) ? 1u : 0u;
        const uint64_t p = m ? p1++ : p0++;
        (m ? out.sig[1] : out.sig[0])[p] = w[2];
        (m ? out.row[1] : out.row[0])[p] = w[1];
        if (kKeep) {
            const Fe c = ge ? Fr::reduce_full(v) : v;                              // canonical for any 256-bit value (2^256 < 6 r)
            const bool z = pk_zero(c);
            zero0 += (!m && z) ? 1u : 0u;
            zero1 += (m && z) ? 1u : 0u;
            (m ? out.coef[1] : out.coef[0])[p] = c;
        } else {
            (m ? out.coef[1] : out.coef[0])[p] = Fr::from_mont(Fr::from_mont(v));      // c R^2 -> c: canonical for any 256-bit value
        }
    }
    if (big0) atomicAdd(&acc->unreduced[0], (unsigned long long)big0);
    if (big1) atomicAdd(&acc->unreduced[1], (unsigned long long)big1);
    if (kKeep && zero0) atomicAdd(&acc->zero[0], (unsigned long long)zero0);
    if (kKeep && zero1) atomicAdd(&acc->zero[1], (unsigned long long)zero1);
}

__global__ __launch_bounds__(256) void zk_order_kernel(const uint32_t* __restrict__ row, uint32_t n, unsigned long long* __restrict__ unsorted) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 || i >= n) return;
    if (row[i] < row[i - 1]) atomicMax(unsorted, 1ull);
}

// the pairs of a sort: (src[p], p), or with `through` the new key of pairs already sorted by another one: (src[through[p]], through[p])
__global__ __launch_bounds__(256) void zk_keys_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ through, uint32_t n,
                                                      uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (through) { key[p] = src[through[p]]; return; }
    key[p] = src[p];
    val[p] = p;
}

// Entry g of the two streams laid end to end (column j < n_vars: A's signal j; j >= n_vars: B's signal j - n_vars): its column by
// binary search in the record prefix (csr_count_kernel's search), its constraint as the sort key.
__global__ __launch_bounds__(256) void zk_unpack_kernel(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ start,
                                                        const uint32_t* __restrict__ rec_base, uint32_t n_cols, uint32_t n, uint32_t domain,
                                                        uint32_t* __restrict__ key, uint32_t* __restrict__ val, uint32_t* __restrict__ col_of,
                                                        ZkAcc* __restrict__ acc) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    uint32_t lo = 0, hi = n_cols;                       // largest j with rec_base[j] <= g (rec_base[n_cols] = n > g)
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (rec_base[mid] <= g) lo = mid; else hi = mid; }
    const uint32_t idx = *reinterpret_cast<const uint32_t*>(blob + start[lo] + 4 + (uint64_t)36 * (g - rec_base[lo]));
    col_of[g] = lo;
    val[g] = g;
    key[g] = idx < domain ? idx : 0;
    if (idx >= domain) atomicMax(&acc->bad_constraint, ~(unsigned long long)g);
}

// 256 sorted records per workgroup: lane q builds record q (matrix, constraint, signal, (c R) R) in LDS, then the workgroup stores the
// 2816 words with 32-bit stores in output order
__global__ __launch_bounds__(256) void zk_emit_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, uint32_t n, uint32_t n_vars,
                                                      const uint32_t* __restrict__ col_of, const uint8_t* __restrict__ blob,
                                                      const uint64_t* __restrict__ start, const uint32_t* __restrict__ rec_base,
                                                      uint32_t* __restrict__ words) {
    __shared__ uint32_t rec[256 * kRecWords];
    const uint32_t l = threadIdx.x;
    const uint64_t p0 = (uint64_t)blockIdx.x * 256, p = p0 + l;
    if (p < n) {
        const uint32_t g = val[p], j = col_of[g], m = j >= n_vars ? 1u : 0u;
        const uint32_t* w = reinterpret_cast<const uint32_t*>(blob + start[j] + 8 + (uint64_t)36 * (g - rec_base[j]));      // (4-byte aligned)
        Fe c;
        for (int k = 0; k < 4; k++) c.l[k] = (uint64_t)w[2 * k] | ((uint64_t)w[2 * k + 1] << 32);
        const Fe v = Fr::to_mont(c);
        rec[kRecWords * l] = m;
        rec[kRecWords * l + 1] = key[p];
        rec[kRecWords * l + 2] = j - m * n_vars;
        for (int k = 0; k < 4; k++) { rec[kRecWords * l + 3 + 2 * k] = (uint32_t)v.l[k]; rec[kRecWords * l + 4 + 2 * k] = (uint32_t)(v.l[k] >> 32); }
    }
    __syncthreads();
    const uint32_t n_rec = n - p0 < 256 ? (uint32_t)(n - p0) : 256;
    for (uint32_t w = l; w < kRecWords * n_rec; w += 256) words[kRecWords * p0 + w] = rec[w];
}

// ---- the resident path (zkey_load): one matrix's records, non-decreasing in the constraint, as the prover's row-major CSR ----
// row_ptr[k], k = 0 .. domain: the records with constraint < k.  One lane per k, a binary search in the constraints: every entry is
// written by exactly one lane with a plain store, rows without records and a matrix without records (n = 0) included.
__global__ __launch_bounds__(256) void zk_rowptr_kernel(const uint32_t* __restrict__ row, uint32_t n, uint32_t domain, uint32_t* __restrict__ row_ptr) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > domain) return;
    uint32_t lo = 0, hi = n;                            // the first p with row[p] >= k
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (row[mid] < k) lo = mid + 1; else hi = mid; }
    row_ptr[k] = lo;
}
// a matrix that had to be sorted: entry p of the result is entry val[p] of the partition's
__global__ __launch_bounds__(256) void zk_gather_kernel(const uint32_t* __restrict__ val, uint32_t n, const uint32_t* __restrict__ sig_in,
                                                        const Fe* __restrict__ coef_in, uint32_t* __restrict__ sig_out, Fe* __restrict__ coef_out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t e = val[p];
    sig_out[p] = sig_in[e];
    coef_out[p] = coef_in[e];
}

// ---- host ----
namespace {
const uint64_t kQ[4] = {FqParams::P0, FqParams::P1, FqParams::P2, FqParams::P3};
const uint64_t kR[4] = {FrParams::P0, FrParams::P1, FrParams::P2, FrParams::P3};
constexpr uint64_t kSec2Len = 4 + 32 + 4 + 32 + 12 + 3 * 64 + 3 * 128;      // 660
constexpr uint64_t kFixedAt = 4 + 32 + 4 + 32 + 12;                          // alpha1 | beta1 | beta2 | gamma2 | delta1 | delta2

int fmt(const std::string& what) { set_last_error("zkey: " + what); return WS_ERR_FORMAT; }
uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
uint64_t rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
void wr32(uint8_t* p, uint32_t v) { memcpy(p, &v, 4); }
void wr64(uint8_t* p, uint64_t v) { memcpy(p, &v, 8); }
int log2_of(uint64_t n) { int b = 0; while (((uint64_t)1 << b) < n) b++; return b; }

struct ZkSec { const uint8_t* p = nullptr; uint64_t len = 0; bool have = false; };
struct ZkFile {
    ZkSec sec[11];
    uint32_t n_vars = 0, n_public = 0, domain = 0, n_coeffs = 0, n_contrib = 0;
    uint64_t nC = 0;
    const uint8_t* fixed() const { return sec[2].p + kFixedAt; }
};

// the container and every size the header implies, with the texts include/wsnark.h promises
int zk_parse(const uint8_t* z, size_t len, ZkFile* F) {
    if (!z) return WS_ERR_ARG;
    if (len < 12) return fmt("truncated file (no container header)");
    if (memcmp(z, "zkey", 4) != 0) return fmt("bad magic (not \"zkey\")");
    if (rd32(z + 4) != 1) return fmt("unknown version " + std::to_string(rd32(z + 4)));
    const uint32_t n_sec = rd32(z + 8);
    uint64_t at = 12;
    for (uint32_t k = 0; k < n_sec; k++) {
        if (len - at < 12) return fmt("truncated file (section header " + std::to_string(k) + ")");
        const uint32_t type = rd32(z + at);
        const uint64_t size = rd64(z + at + 4);
        at += 12;
        if (size > len - at) return fmt("truncated file (section of type " + std::to_string(type) + " runs past the end)");
        if (type >= 1 && type <= 10) {
            if (F->sec[type].have) return fmt("section " + std::to_string(type) + " is present twice");
            F->sec[type] = ZkSec{z + at, size, true};
        }
        at += size;
    }
    for (int t = 1; t <= 9; t++)
        if (!F->sec[t].have) return fmt("section " + std::to_string(t) + " is missing");
    if (F->sec[1].len != 4) return fmt("section 1 size does not match (4 bytes)");
    const uint32_t proto = rd32(F->sec[1].p);
    if (proto != 1) return fmt("protocol " + std::to_string(proto) + " is not Groth16 (PLONK and FFLONK keys are not supported)");
    const ZkSec& h = F->sec[2];
    if (h.len < 4) return fmt("section 2 size does not match");
    if (rd32(h.p) != 32) return fmt("n8q is not 32");
    if (h.len != kSec2Len) return fmt("section 2 size does not match its counts");
    if (memcmp(h.p + 4, kQ, 32) != 0) return fmt("q is not BN128's base field modulus");
    if (rd32(h.p + 36) != 32) return fmt("n8r is not 32");
    if (memcmp(h.p + 40, kR, 32) != 0) return fmt("r is not BN128's group order");
    F->n_vars = rd32(h.p + 72); F->n_public = rd32(h.p + 76); F->domain = rd32(h.p + 80);
    if ((uint64_t)F->n_public + 1 > F->n_vars) return fmt("nPublic + 1 > nVars");
    const uint64_t n = F->domain, nv = F->n_vars;
    if (n < 2 || (n & (n - 1)) || n > ((uint64_t)1 << 24)) { set_last_error("zkey: domainSize must be a power of two in [2, 2^24]"); return WS_ERR_SIZE; }
    F->nC = nv - F->n_public - 1;
    if (F->sec[4].len < 4) return fmt("section 4 size does not match its counts");
    F->n_coeffs = rd32(F->sec[4].p);
    const uint64_t want[10] = {0, 4, kSec2Len, 64 * ((uint64_t)F->n_public + 1), 4 + 44 * (uint64_t)F->n_coeffs, 64 * nv, 64 * nv, 128 * nv, 64 * F->nC, 64 * n};
    for (int t = 3; t <= 9; t++)
        if (F->sec[t].len != want[t]) return fmt("section " + std::to_string(t) + " size does not match its counts");
    if (F->sec[10].have) {
        if (F->sec[10].len < 68) return fmt("section 10 size does not match its counts");
        F->n_contrib = rd32(F->sec[10].p + 64);
    }
    return WS_OK;
}

uint64_t pkey_len_of(uint64_t nv, uint64_t nC, uint64_t n, uint64_t lenA, uint64_t lenB) { return 40 + 448 + lenA + lenB + 64 * nv + 64 * nv + 128 * nv + 64 * nC + 64 * n; }
uint64_t vk_len_of(uint64_t n_public) { return 64 + 3 * 128 + 64 * (n_public + 1); }

// coordinates between Montgomery (a key, a .zkey) and plain (the verifier's vk), 32 bytes each
void q_from_mont(const uint8_t* in, uint8_t* out, size_t coords) {
    for (size_t k = 0; k < coords; k++) { Fe x; memcpy(&x, in + 32 * k, 32); x = Fq::from_mont(x); memcpy(out + 32 * k, &x, 32); }
}
void q_to_mont(const uint8_t* in, uint8_t* out, size_t coords) {
    for (size_t k = 0; k < coords; k++) { Fe x; memcpy(&x, in + 32 * k, 32); x = Fq::to_mont(x); memcpy(out + 32 * k, &x, 32); }
}

// The H basis change on device-resident points: d_a holds the n input points (reference format), d_b is as large; the result, in
// reference format, is where *d_res says.  d_sc: n scalars, d_tw: n/2 twiddles, d_acc: two PkAcc, zeroed -- [0] counts the INPUT.
// The input's counts are read back before a stage runs: *bad != 0 ends the call there.
int h_basis_dev(Context* X, void* d_a, void* d_b, Fe* d_sc, ScaleDigits* d_tw, uint64_t n, int bits, int to_lagrange, PkAcc* d_acc, PkAcc* h_in,
                void** d_res, hipStream_t s) {
    int rc;
    Fe w2n = group_root_of_unity(bits + 1);
    const Fe two = Fr::add(Fr::one(), Fr::one());
    auto input_counts = [&]() -> int {
        WS_HIP_CHECK(hipMemcpyAsync(h_in, d_acc, sizeof(PkAcc), hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));
        return WS_OK;
    };
    if (!to_lagrange) {
        if ((rc = g1_ntt_load_dev(X, d_a, d_b, n, bits, d_acc, s))) return rc;
        if ((rc = input_counts())) return rc;
        if (h_in->bad) return WS_OK;
        if ((rc = g1_ntt_stages_dev(X, d_b, bits, 0, d_tw, s))) return rc;
        if ((rc = fr_powers_dev(X, Fr::neg(two), w2n, 0, n, d_sc, s))) return rc;                 // -2 w_2n^k
        if ((rc = g1_mul_dev(X, d_b, d_sc, n, d_a, d_acc + 1, s))) return rc;
        *d_res = d_a;
    } else {
        Fe c = Fr::one();                                                                          // -(2n)^-1 = -(2^-1)^(bits + 1)
        const Fe half = Fr::inv(two);
        for (int i = 0; i <= bits; i++) c = Fr::mul(c, half);
        if ((rc = fr_powers_dev(X, Fr::neg(c), Fr::inv(w2n), 0, n, d_sc, s))) return rc;         // -(2n)^-1 w_2n^(-k)
        if ((rc = g1_mul_dev(X, d_a, d_sc, n, d_b, d_acc, s))) return rc;
        if ((rc = input_counts())) return rc;
        if (h_in->bad) return WS_OK;
        if ((rc = g1_ntt_load_dev(X, d_b, d_a, n, bits, d_acc + 1, s))) return rc;
        if ((rc = g1_ntt_stages_dev(X, d_a, bits, 1, d_tw, s))) return rc;
        *d_res = d_a;
    }
    return WS_OK;
}
struct HBufs {
    void *a = nullptr, *b = nullptr;
    Fe* sc = nullptr;
    ScaleDigits* tw = nullptr;
    PkAcc* acc = nullptr;      // two, to be zeroed
    void add(Slab& S, uint64_t n, bool with_a = true) {      // (without a: the caller's own buffer holds the input and takes the result)
        if (with_a) S.add(&a, (size_t)n * 64);
        S.add(&b, (size_t)n * 64);
        S.add(&sc, (size_t)n * 32);
        S.add(&tw, (size_t)std::max<uint64_t>(n / 2, 1) * sizeof(ScaleDigits));
        S.add(&acc, 2 * sizeof(PkAcc));
    }
};
int h_bad_error(const char* who, const PkAcc& a) {
    uint64_t inf, bad, first;
    uint32_t reason;
    pk_decode(a, &inf, &bad, &first, &reason);
    set_last_error(std::string(who) + ": " + std::to_string(bad) + " point(s) of H unreduced or off the curve, the first at index " + std::to_string(first));
    return WS_ERR_FORMAT;
}
void h_report(const PkAcc& a, uint64_t n, wsnark_zkey_report_t* R) {
    R->h_points = n;
    pk_decode(a, &R->h_infinity, &R->h_bad, &R->h_first_bad, &R->h_first_reason);
}

// the sort's arrays for at most `most` pairs (the object stays where it is between add and the slab's alloc)
struct SortBufs {
    RowsSort B;
    void add(Slab& S, uint64_t most, uint32_t tile) {
        const size_t nz = (size_t)std::max<uint64_t>(most, 1) * 4;
        const uint32_t n_hist = rows_sort_counters(most, tile);
        for (int k = 0; k < 2; k++) { S.add(&B.key[k], nz); S.add(&B.val[k], nz); }
        S.add(&B.hist, (size_t)n_hist * 4);
        S.add(&B.base, (size_t)n_hist * 4);
        S.add(&B.cursor, (size_t)n_hist * 4);
        S.add(&B.tiles, (size_t)ceil_div_u64(n_hist, 1024) * 4);
        B.tile = tile;
    }
};
}  // namespace

int g1_h_basis(const void* points, uint64_t n, int to_lagrange, void* out) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (n < 2 || (n & (n - 1)) || n > ((uint64_t)1 << 24)) { set_last_error("H basis: n must be a power of two in [2, 2^24]"); return WS_ERR_SIZE; }
    if (!points || !out) return WS_ERR_ARG;
    const int bits = log2_of(n);
    LaneLock L = acquire_lane(X);
    hipStream_t s = L->stream;
    HBufs H;
    Slab slab;
    H.add(slab, n);
    WS_HIP_CHECK(slab.alloc());
    WS_HIP_CHECK(hipMemsetAsync(H.acc, 0, 2 * sizeof(PkAcc), s));
    int rc;
    if ((rc = upload_staged(H.a, points, (size_t)n * 64, s))) return rc;
    PkAcc h_in;
    void* d_res = nullptr;
    if ((rc = h_basis_dev(X, H.a, H.b, H.sc, H.tw, n, bits, to_lagrange, H.acc, &h_in, &d_res, s))) return rc;
    if (h_in.bad) return h_bad_error("H basis", h_in);
    WS_HIP_CHECK(hipMemcpyAsync(out, d_res, (size_t)n * 64, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    return WS_OK;
}

int zkey_info(const uint8_t* zkey, size_t len, wsnark_zkey_info_t* out) {
    if (!out) return WS_ERR_ARG;
    ZkFile F;
    if (int rc = zk_parse(zkey, len, &F)) return rc;
    uint64_t cnt[2] = {0, 0};
    const uint8_t* r = F.sec[4].p + 4;
    for (uint64_t e = 0; e < F.n_coeffs; e++) {
        const uint32_t m = rd32(r + 44 * e);
        if (m > 1) return fmt("matrix > 1 in coefficient record " + std::to_string(e));
        cnt[m]++;
    }
    wsnark_zkey_info_t I;
    memset(&I, 0, sizeof I);
    I.n_vars = F.n_vars; I.n_public = F.n_public; I.domain = F.domain; I.n_coeffs = F.n_coeffs;
    I.records[0] = cnt[0]; I.records[1] = cnt[1];
    I.n_contributions = F.n_contrib;
    I.pkey_len = pkey_len_of(F.n_vars, F.nC, F.domain, 4 * (uint64_t)F.n_vars + 36 * cnt[0], 4 * (uint64_t)F.n_vars + 36 * cnt[1]);
    I.vk_len = vk_len_of(F.n_public);
    *out = I;
    return WS_OK;
}

// out / caps: polsA, polsB, pointsA, pointsB1, pointsB2, pointsC, pointsH, alfa1, beta1, delta1, beta2, delta2 -- or, with out_pkey, the
// whole proving_key.bin there (out and caps are then not read)
int zkey_import(const uint8_t* zkey, size_t len, void* const out[12], const uint64_t caps[12], uint8_t* out_pkey, size_t pkey_cap, size_t* out_len,
                uint8_t* out_vk, size_t vk_cap, wsnark_zkey_report_t* rep) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    const auto t_call = Clock::now();
    if (!zkey || !out_vk || !rep || (!out_pkey && (!out || !caps))) return WS_ERR_ARG;
    ZkFile F;
    int rc;
    if ((rc = zk_parse(zkey, len, &F))) return rc;
    const uint64_t nv = F.n_vars, n = F.domain, nC = F.nC;
    const uint32_t nrec = F.n_coeffs;
    const int bits = log2_of(n);
    if (vk_cap < vk_len_of(F.n_public)) { set_last_error("zkey import: the capacity of the verification key is too small"); return WS_ERR_SIZE; }
    if (!out_pkey)
        for (int k = 0; k < 12; k++)
            if (!out[k] && !(k == 5 && nC == 0)) return WS_ERR_ARG;
    uint32_t tile;
    if ((rc = rows_tile(&tile))) return rc;
    const uint32_t n_tiles = ceil_div_u64(std::max<uint32_t>(nrec, 1), tile);
    uint32_t sig_bits = 0;
    while (sig_bits < 32 && ((uint64_t)1 << sig_bits) < nv) sig_bits++;

    LaneLock L = acquire_lane(X);
    hipStream_t s = L->stream;
    KernelTimer& T = X->timer;
    // 1. the two sections that change form go up
    // ONE allocation: nothing below is sized by what the device finds (a matrix's arrays are the two ends of one array of nrec entries)
    uint32_t *d_rec, *d_cnt, *d_base, *d_cursor, *d_tiles, *d_sig, *d_row, *d_words;
    Fe* d_coef;
    ZkAcc* acc;
    RowsAcc* d_racc;
    HBufs H;
    SortBufs SB;
    Slab slab;
    slab.add(&d_rec, (size_t)nrec * 44);
    slab.add(&d_cnt, ((size_t)n_tiles + 1) * 4);
    slab.add(&d_base, ((size_t)n_tiles + 1) * 4);
    slab.add(&d_cursor, ((size_t)n_tiles + 1) * 4);
    slab.add(&d_tiles, (size_t)ceil_div_u64((uint64_t)n_tiles + 1, 1024) * 4);
    slab.add(&acc, sizeof(ZkAcc));
    slab.add(&d_racc, 2 * sizeof(RowsAcc));
    slab.add(&d_sig, (size_t)nrec * 4);
    slab.add(&d_row, (size_t)nrec * 4);
    slab.add(&d_coef, (size_t)nrec * 32);
    slab.add(&d_words, (size_t)(8 * nv + 36 * (uint64_t)nrec));
    H.add(slab, n);
    SB.add(slab, nrec, tile);
    WS_HIP_CHECK(slab.alloc());
    WS_HIP_CHECK(hipMemsetAsync(d_cnt, 0, ((size_t)n_tiles + 1) * 4, s));
    WS_HIP_CHECK(hipMemsetAsync(acc, 0, sizeof(ZkAcc), s));
    WS_HIP_CHECK(hipMemsetAsync(d_racc, 0, 2 * sizeof(RowsAcc), s));
    WS_HIP_CHECK(hipMemsetAsync(H.acc, 0, 2 * sizeof(PkAcc), s));
    if (nrec && (rc = upload_staged(d_rec, F.sec[4].p + 4, (size_t)nrec * 44, s))) return rc;
    if ((rc = upload_staged(H.a, F.sec[9].p, (size_t)n * 64, s))) return rc;
    WS_HIP_CHECK(hipStreamSynchronize(s));
    const double ms_up = ms_since(t_call);

    // 2. the coefficients: counts and tests, then everything the sizes decide, then the partition, the sort and the emit
    const auto t_coef = Clock::now();
    const uint32_t* rec = d_rec;
    if (nrec) {
        T.begin("zkey_count", s);
        hipLaunchKernelGGL(zk_count_kernel, dim3(n_tiles), dim3(256), 0, s, rec, nrec, tile, F.n_vars, F.domain, d_cnt, acc);
        WS_HIP_CHECK(hipGetLastError());
        T.end(s);
    }
    // (n_tiles + 1 counters, the last one zero: the scan's last entry is matrix 0's total)
    if ((rc = scan_exclusive_dev(d_cnt, n_tiles + 1, d_tiles, d_base, d_cursor, s))) return rc;
    ZkAcc h_acc;
    uint32_t n0 = 0;
    WS_HIP_CHECK(hipMemcpyAsync(&h_acc, acc, sizeof h_acc, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipMemcpyAsync(&n0, d_base + n_tiles, 4, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    if (h_acc.bad_matrix) return fmt("matrix > 1 in a coefficient record, first at record " + std::to_string(~h_acc.bad_matrix));
    if (h_acc.bad_signal) return fmt("signal >= nVars in a coefficient record, first at record " + std::to_string(~h_acc.bad_signal));
    if (h_acc.bad_constraint) return fmt("constraint >= domainSize in a coefficient record, first at record " + std::to_string(~h_acc.bad_constraint));
    const uint32_t cnt[2] = {n0, nrec - n0};
    const uint64_t lens[2] = {4 * nv + 36 * (uint64_t)cnt[0], 4 * nv + 36 * (uint64_t)cnt[1]};
    const uint64_t sizes[12] = {lens[0], lens[1], 64 * nv, 64 * nv, 128 * nv, 64 * nC, 64 * n, 64, 64, 64, 128, 128};
    uint8_t* dst[12];
    const uint64_t total = pkey_len_of(nv, nC, n, lens[0], lens[1]);
    uint32_t head[10] = {F.n_vars, F.n_public, F.domain};
    if (out_pkey) {
        if (total >= ((uint64_t)1 << 32)) { set_last_error("zkey import: the key is beyond the 4 GiB of proving_key.bin's u32 offsets: use the sections variant"); return WS_ERR_SIZE; }
        if (pkey_cap < total) { set_last_error("zkey import: the output buffer is smaller than the key"); return WS_ERR_SIZE; }
        uint64_t o = 40;
        for (int k = 7; k < 12; k++) { dst[k] = out_pkey + o; o += sizes[k]; }      // alfa1, beta1, delta1, beta2, delta2
        for (int k = 0; k < 7; k++) { dst[k] = out_pkey + o; head[3 + k] = (uint32_t)o; o += sizes[k]; }
    } else {
        for (int k = 0; k < 12; k++) {
            if (caps[k] < sizes[k]) { set_last_error("zkey import: the capacity of output " + std::to_string(k) + " is too small"); return WS_ERR_SIZE; }
            dst[k] = (uint8_t*)out[k];
        }
    }
    uint32_t* const m_sig[2] = {d_sig, d_sig + n0};
    uint32_t* const m_row[2] = {d_row, d_row + n0};
    Fe* const m_coef[2] = {d_coef, d_coef + n0};
    uint32_t* const m_words[2] = {d_words, d_words + lens[0] / 4};
    if (nrec) {
        const ZkParts parts{{m_sig[0], m_sig[1]}, {m_row[0], m_row[1]}, {m_coef[0], m_coef[1]}};
        T.begin("zkey_partition", s);
        hipLaunchKernelGGL(zk_partition_kernel<false>, dim3(n_tiles), dim3(256), 0, s, rec, nrec, tile / 256, d_base, parts, acc);
        WS_HIP_CHECK(hipGetLastError());
        T.end(s);
        T.begin("zkey_order", s);
        for (int m = 0; m < 2; m++)
            if (cnt[m] > 1) hipLaunchKernelGGL(zk_order_kernel, dim3(ceil_div_u64(cnt[m], 256)), dim3(256), 0, s, m_row[m], cnt[m], &acc->unsorted[m]);
        WS_HIP_CHECK(hipGetLastError());
        T.end(s);
        WS_HIP_CHECK(hipMemcpyAsync(&h_acc, acc, sizeof h_acc, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));
    }
    for (int m = 0; m < 2; m++) {
        const uint32_t c = cnt[m];
        const dim3 grid(ceil_div_u64(std::max<uint32_t>(c, 1), 256)), block(256);
        int cur = 0;
        if (c && h_acc.unsorted[m]) {      // by constraint first; the signal passes below then keep that order inside a signal
            hipLaunchKernelGGL(zk_keys_kernel, grid, block, 0, s, (const uint32_t*)m_row[m], (const uint32_t*)nullptr, c, SB.B.key[0], SB.B.val[0]);
            WS_HIP_CHECK(hipGetLastError());
            if ((rc = rows_sort_dev(X, SB.B, c, 0, (uint32_t)bits, &cur, s))) return rc;
            hipLaunchKernelGGL(zk_keys_kernel, grid, block, 0, s, (const uint32_t*)m_sig[m], (const uint32_t*)SB.B.val[cur], c, SB.B.key[cur], SB.B.val[cur]);
            WS_HIP_CHECK(hipGetLastError());
        } else if (c) {
            hipLaunchKernelGGL(zk_keys_kernel, grid, block, 0, s, (const uint32_t*)m_sig[m], (const uint32_t*)nullptr, c, SB.B.key[0], SB.B.val[0]);
            WS_HIP_CHECK(hipGetLastError());
        }
        if ((rc = rows_sort_dev(X, SB.B, c, 0, sig_bits, &cur, s))) return rc;
        if ((rc = rows_emit_dev(X, SB.B.key[cur], SB.B.val[cur], c, c, F.n_vars, m_row[m], m_coef[m], m_words[m], d_racc + m, s)))
            return rc;
    }
    RowsAcc h_racc[2];
    WS_HIP_CHECK(hipMemcpyAsync(h_racc, d_racc, sizeof h_racc, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    const double ms_coef = ms_since(t_coef);

    // 3. H: the forward transform, then -2 w_2n^k per point
    const auto t_h = Clock::now();
    PkAcc h_in;
    void* d_res = nullptr;
    if ((rc = h_basis_dev(X, H.a, H.b, H.sc, H.tw, n, bits, 0, H.acc, &h_in, &d_res, s))) return rc;
    if (h_in.bad) return h_bad_error("zkey import", h_in);
    WS_HIP_CHECK(hipStreamSynchronize(s));
    const double ms_h = ms_since(t_h);

    // 4. down: nothing was written before this line
    const auto t_down = Clock::now();
    for (int m = 0; m < 2; m++) WS_HIP_CHECK(hipMemcpyAsync(dst[m], m_words[m], (size_t)lens[m], hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipMemcpyAsync(dst[6], d_res, (size_t)n * 64, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    for (int k = 0; k < 4; k++)
        if (sizes[2 + k]) memcpy(dst[2 + k], F.sec[5 + k].p, (size_t)sizes[2 + k]);
    const uint8_t* fx = F.fixed();      // alpha1 | beta1 | beta2 | gamma2 | delta1 | delta2
    memcpy(dst[7], fx, 64);
    memcpy(dst[8], fx + 64, 64);
    memcpy(dst[9], fx + 384, 64);
    memcpy(dst[10], fx + 128, 128);
    memcpy(dst[11], fx + 448, 128);
    if (out_pkey) {
        memcpy(out_pkey, head, 40);
        if (out_len) *out_len = (size_t)total;
    }
    q_from_mont(fx, out_vk, 2);                       // alfa1
    q_from_mont(fx + 128, out_vk + 64, 4);            // beta2
    q_from_mont(fx + 256, out_vk + 192, 4);           // gamma2
    q_from_mont(fx + 448, out_vk + 320, 4);           // delta2
    q_from_mont(F.sec[3].p, out_vk + 448, 2 * ((size_t)F.n_public + 1));
    wsnark_zkey_report_t R;
    memset(&R, 0, sizeof R);
    for (int m = 0; m < 2; m++) { R.records[m] = cnt[m]; R.unreduced[m] = nrec ? h_acc.unreduced[m] : 0; R.zero[m] = h_racc[m].zero; }
    R.sorted = nrec == 0 || (!h_acc.unsorted[0] && !h_acc.unsorted[1]);
    h_report(h_in, n, &R);
    R.ms[0] = ms_up; R.ms[1] = ms_coef; R.ms[2] = ms_h; R.ms[3] = ms_since(t_down); R.ms[4] = ms_since(t_call);
    *rep = R;
    return WS_OK;
}

int zkey_export_size(uint32_t n_vars, uint32_t n_public, uint32_t domain, uint64_t nnzA, uint64_t nnzB, size_t* out_len) {
    if (!out_len) return WS_ERR_ARG;
    if (int rc = key_vars_check(n_vars, n_public)) return rc;
    const uint64_t nv = n_vars, nC = nv - n_public - 1;
    *out_len = (size_t)(12 + 10 * 12 + 4 + kSec2Len + 64 * ((uint64_t)n_public + 1) + 4 + 44 * (nnzA + nnzB) + 64 * nv + 64 * nv + 128 * nv + 64 * nC +
                        64 * (uint64_t)domain + 68);
    return WS_OK;
}

namespace {
// where every signal's records start in a stream and how many records precede it, appended to start / rec_base (pols_to_csr's walk)
int walk_stream(const uint8_t* pols, uint64_t len, uint32_t n_vars, uint64_t blob_at, std::vector<uint64_t>* start, std::vector<uint32_t>* rec_base,
                uint64_t* nnz) {
    uint64_t pp = 0;
    for (uint32_t j = 0; j < n_vars; j++) {
        start->push_back(blob_at + pp);
        rec_base->push_back((uint32_t)*nnz);
        if (pp + 4 > len) { set_last_error("pols: truncated record header"); return WS_ERR_FORMAT; }
        const uint32_t nc = rd32(pols + pp);
        pp += 4;
        if ((uint64_t)nc * 36 > len - pp) { set_last_error("pols: truncated coefficient records"); return WS_ERR_FORMAT; }
        pp += (uint64_t)nc * 36;
        *nnz += nc;
        if (*nnz >= ((uint64_t)1 << 32)) { set_last_error("zkey export: 2^32 coefficient records or more"); return WS_ERR_SIZE; }
    }
    return WS_OK;
}
}  // namespace

int zkey_export(const KeySections& S, const uint8_t* vk, size_t vk_len, uint64_t n_inputs, uint8_t* out, size_t cap, size_t* out_len,
                wsnark_zkey_report_t* rep) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    const auto t_call = Clock::now();
    if (!vk || !out || !rep) return WS_ERR_ARG;
    int rc;
    if ((rc = key_shape_check(S))) return rc;
    const uint64_t nv = S.n_vars, n = S.domain, npub = S.n_public, nC = nv - npub - 1;
    if (n > ((uint64_t)1 << 24)) { set_last_error("zkey export: domainSize must be a power of two in [2, 2^24]"); return WS_ERR_SIZE; }
    if (n_inputs != npub || vk_len < vk_len_of(npub)) { set_last_error("zkey export: the verification key does not hold nPublic + 1 IC points"); return WS_ERR_ARG; }
    const int bits = log2_of(n);
    std::vector<uint64_t> start;
    std::vector<uint32_t> rec_base;
    start.reserve(2 * nv + 1);
    rec_base.reserve(2 * nv + 1);
    uint64_t nnz = 0;
    if ((rc = walk_stream(S.polsA, S.lenA, S.n_vars, 0, &start, &rec_base, &nnz))) return rc;
    const uint64_t usedA = 4 * nv + 36 * nnz, nnzA = nnz;
    if ((rc = walk_stream(S.polsB, S.lenB, S.n_vars, usedA, &start, &rec_base, &nnz))) return rc;
    const uint64_t usedB = 4 * nv + 36 * (nnz - nnzA);
    start.push_back(usedA + usedB);
    rec_base.push_back((uint32_t)nnz);
    const uint32_t nrec = (uint32_t)nnz;
    size_t total;
    if ((rc = zkey_export_size(S.n_vars, S.n_public, S.domain, nnzA, nnz - nnzA, &total))) return rc;
    if (cap < total) { set_last_error("zkey export: the output buffer is smaller than the file"); return WS_ERR_SIZE; }
    uint32_t tile;
    if ((rc = rows_tile(&tile))) return rc;

    LaneLock L = acquire_lane(X);
    hipStream_t s = L->stream;
    KernelTimer& T = X->timer;
    uint8_t* d_blob;
    uint64_t* d_start;
    uint32_t *d_rbase, *d_col, *d_out;
    ZkAcc* d_acc;
    HBufs H;
    SortBufs SB;
    Slab slab;
    slab.add(&d_blob, (size_t)(usedA + usedB) + 64);
    slab.add(&d_start, start.size() * 8);
    slab.add(&d_rbase, rec_base.size() * 4);
    slab.add(&d_col, (size_t)nrec * 4);
    slab.add(&d_out, (size_t)nrec * 44);
    slab.add(&d_acc, sizeof(ZkAcc));
    H.add(slab, n);
    SB.add(slab, nrec, tile);
    WS_HIP_CHECK(slab.alloc());
    WS_HIP_CHECK(hipMemsetAsync(d_acc, 0, sizeof(ZkAcc), s));
    WS_HIP_CHECK(hipMemsetAsync(H.acc, 0, 2 * sizeof(PkAcc), s));
    if ((rc = upload_staged(d_blob, S.polsA, (size_t)usedA, s))) return rc;
    if ((rc = upload_staged(d_blob + usedA, S.polsB, (size_t)usedB, s))) return rc;
    if ((rc = upload_staged(d_start, start.data(), start.size() * 8, s))) return rc;
    if ((rc = upload_staged(d_rbase, rec_base.data(), rec_base.size() * 4, s))) return rc;
    if ((rc = upload_staged(H.a, S.H, (size_t)n * 64, s))) return rc;
    WS_HIP_CHECK(hipStreamSynchronize(s));
    const double ms_up = ms_since(t_call);

    // the coefficients: entries in stream order, stably sorted by constraint, emitted as records
    const auto t_coef = Clock::now();
    int cur = 0;
    if (nrec) {
        T.begin("zkey_unpack", s);
        hipLaunchKernelGGL(zk_unpack_kernel, dim3(ceil_div_u64(nrec, 256)), dim3(256), 0, s, (const uint8_t*)d_blob, (const uint64_t*)d_start, (const uint32_t*)d_rbase,
                           (uint32_t)(2 * nv), nrec, S.domain, SB.B.key[0], SB.B.val[0], d_col, d_acc);
        WS_HIP_CHECK(hipGetLastError());
        T.end(s);
        ZkAcc h_acc;
        WS_HIP_CHECK(hipMemcpyAsync(&h_acc, d_acc, sizeof h_acc, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));
        if (h_acc.bad_constraint) { set_last_error("pols: coefficient index >= domainSize"); return WS_ERR_FORMAT; }
        if ((rc = rows_sort_dev(X, SB.B, nrec, 0, (uint32_t)bits, &cur, s))) return rc;
        T.begin("zkey_emit", s);
        hipLaunchKernelGGL(zk_emit_kernel, dim3(ceil_div_u64(nrec, 256)), dim3(256), 0, s, (const uint32_t*)SB.B.key[cur], (const uint32_t*)SB.B.val[cur], nrec, S.n_vars, (const uint32_t*)d_col,
                           (const uint8_t*)d_blob, (const uint64_t*)d_start, (const uint32_t*)d_rbase, d_out);
        WS_HIP_CHECK(hipGetLastError());
        T.end(s);
        WS_HIP_CHECK(hipStreamSynchronize(s));
    }
    const double ms_coef = ms_since(t_coef);

    // H: -(2n)^-1 w_2n^(-k) per point, then the inverse transform's stages
    const auto t_h = Clock::now();
    PkAcc h_in;
    void* d_res = nullptr;
    if ((rc = h_basis_dev(X, H.a, H.b, H.sc, H.tw, n, bits, 1, H.acc, &h_in, &d_res, s))) return rc;
    if (h_in.bad) return h_bad_error("zkey export", h_in);
    WS_HIP_CHECK(hipStreamSynchronize(s));
    const double ms_h = ms_since(t_h);

    // the file: sections 1 - 10 in numeric order
    const auto t_down = Clock::now();
    uint8_t* p = out;
    memcpy(p, "zkey", 4); wr32(p + 4, 1); wr32(p + 8, 10); p += 12;
    auto section = [&](uint32_t type, uint64_t size) { wr32(p, type); wr64(p + 4, size); p += 12; };
    section(1, 4); wr32(p, 1); p += 4;
    section(2, kSec2Len);
    wr32(p, 32); memcpy(p + 4, kQ, 32); wr32(p + 36, 32); memcpy(p + 40, kR, 32);
    wr32(p + 72, S.n_vars); wr32(p + 76, S.n_public); wr32(p + 80, S.domain);
    uint8_t* fx = p + kFixedAt;
    memcpy(fx, S.alfa1, 64); memcpy(fx + 64, S.beta1, 64); memcpy(fx + 128, S.beta2, 128);
    q_to_mont(vk + 192, fx + 256, 4);      // gamma2
    memcpy(fx + 384, S.delta1, 64); memcpy(fx + 448, S.delta2, 128);
    p += kSec2Len;
    section(3, 64 * (npub + 1)); q_to_mont(vk + 448, p, 2 * (size_t)(npub + 1)); p += 64 * (npub + 1);
    section(4, 4 + 44 * (uint64_t)nrec); wr32(p, nrec); p += 4;
    if (nrec) WS_HIP_CHECK(hipMemcpyAsync(p, d_out, (size_t)nrec * 44, hipMemcpyDeviceToHost, s));
    p += (size_t)nrec * 44;
    section(5, 64 * nv); memcpy(p, S.A, 64 * nv); p += 64 * nv;
    section(6, 64 * nv); memcpy(p, S.B1, 64 * nv); p += 64 * nv;
    section(7, 128 * nv); memcpy(p, S.B2, 128 * nv); p += 128 * nv;
    section(8, 64 * nC); if (nC) memcpy(p, S.Cpts, 64 * nC); p += 64 * nC;
    section(9, 64 * n);
    WS_HIP_CHECK(hipMemcpyAsync(p, d_res, (size_t)n * 64, hipMemcpyDeviceToHost, s));
    p += 64 * n;
    section(10, 68); memset(p, 0, 68); p += 68;
    WS_HIP_CHECK(hipStreamSynchronize(s));
    if (out_len) *out_len = total;
    wsnark_zkey_report_t R;
    memset(&R, 0, sizeof R);
    R.records[0] = nnzA; R.records[1] = nnz - nnzA;
    R.sorted = 1;
    h_report(h_in, n, &R);
    R.ms[0] = ms_up; R.ms[1] = ms_coef; R.ms[2] = ms_h; R.ms[3] = ms_since(t_down); R.ms[4] = ms_since(t_call);
    *rep = R;
    return WS_OK;
}

// ---- a .zkey straight into a resident proving key (wsnark_pkey_load_zkey*) ----
// What wsnark_zkey_import followed by wsnark_pkey_load computes, without the way through a key's bytes: nothing but the verification
// key comes back to the host.
//   points        sections 5 - 8 go through the staging ring into row 0 of the handle's buffers (C behind its nPublic + 1 infinities),
//                 section 9 into H's, where the basis change runs in place: h_basis_dev leaves its result in its input buffer.
//   coefficients  the records are counted, tested and partitioned as for the import, but the value stays c R^2 -- the prover's CSR
//                 holds exactly that (calch.hip: csr_fill_kernel) -- and a matrix's partition IS col[] and coef[] once its constraints
//                 are non-decreasing, which snarkjs' files are.  Where they are not, the import's stable sort by constraint runs and
//                 zk_gather_kernel applies it.  row_ptr is zk_rowptr_kernel's.  No order comes from an atomic: the arrays are in file
//                 order inside a row and the same for the same file.
// Then prove.hip's second half of a load: masks, conversion, tables.  release (a mapped file): every range is staged in pieces and
// handed back piece by piece, so the process never holds the file.
namespace {
int stage_pieces(void* d_dst, const uint8_t* src, size_t bytes, hipStream_t s, void (*release)(const void*, size_t)) {
    const size_t piece = release ? std::max<size_t>((size_t)tuning_get("POLS_PIECE_KB", 32768) << 10, 4096) : std::max<size_t>(bytes, 1);
    for (size_t at = 0; at < bytes; at += piece)
        if (int rc = stage_chunk((uint8_t*)d_dst + at, src + at, std::min(piece, bytes - at), s, release)) return rc;
    return WS_OK;
}
}  // namespace

int zkey_load(const uint8_t* zkey, size_t len, void (*release)(const void*, size_t), ProvingKey** out, uint8_t* out_vk, size_t vk_cap,
              wsnark_zkey_report_t* rep) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    const auto t_call = Clock::now();
    if (!zkey || !out || (!out_vk && vk_cap)) return WS_ERR_ARG;
    ZkFile F;
    int rc;
    if ((rc = zk_parse(zkey, len, &F))) return rc;
    const uint64_t nv = F.n_vars, n = F.domain, nC = F.nC;
    const uint32_t nrec = F.n_coeffs;
    const int bits = log2_of(n);
    if (out_vk && vk_cap < vk_len_of(F.n_public)) { set_last_error("zkey import: the capacity of the verification key is too small")      /* (the import's texts throughout) */; return WS_ERR_SIZE; }
    uint32_t tile;
    if ((rc = rows_tile(&tile))) return rc;
    const uint32_t n_tiles = ceil_div_u64(std::max<uint32_t>(nrec, 1), tile);

    LaneLock L = acquire_lane(X);
    hipStream_t s = L->stream;
    KernelTimer& T = X->timer;
    std::unique_ptr<ProvingKey> K(new ProvingKey());
    KeyLoadClock clock;
    if ((rc = pkey_load_begin(X, K.get(), F.n_vars, F.n_public, F.domain, KeyShard{}, s, &clock))) return rc;
    const uint8_t* fx = F.fixed();      // alpha1 | beta1 | beta2 | gamma2 | delta1 | delta2
    memcpy(&K->alfa1, fx, 64);
    memcpy(&K->beta1, fx + 64, 64);
    memcpy(&K->delta1, fx + 384, 64);
    memcpy(&K->beta2, fx + 128, 128);
    memcpy(&K->delta2, fx + 448, 128);

    // 1. everything goes up once.  The temporaries in ONE allocation (the sort's only where a matrix needs them, below).
    // Deliberately BEFORE the tests that only the device can make (signal, constraint, the H points): the allocation above is what
    // decides between tables and plain sections, H changes basis inside its table, and the uploads are the small part of the call
    // (20 ms of 264 at 2^20: profiles/zkey_load_bench.json).  A malformed file pays them before its error; the error path frees all of it.
    uint32_t *d_rec, *d_cnt, *d_base, *d_cursor, *d_tiles, *d_row;
    ZkAcc* acc;
    HBufs H;
    Slab slab;
    slab.add(&d_rec, (size_t)nrec * 44);
    slab.add(&d_cnt, ((size_t)n_tiles + 1) * 4);
    slab.add(&d_base, ((size_t)n_tiles + 1) * 4);
    slab.add(&d_cursor, ((size_t)n_tiles + 1) * 4);
    slab.add(&d_tiles, (size_t)ceil_div_u64((uint64_t)n_tiles + 1, 1024) * 4);
    slab.add(&acc, sizeof(ZkAcc));
    slab.add(&d_row, (size_t)nrec * 4);
    H.add(slab, n, false);
    H.a = K->pointsH.p;
    WS_HIP_CHECK(slab.alloc());
    WS_HIP_CHECK(hipMemsetAsync(d_cnt, 0, ((size_t)n_tiles + 1) * 4, s));
    WS_HIP_CHECK(hipMemsetAsync(acc, 0, sizeof(ZkAcc), s));
    WS_HIP_CHECK(hipMemsetAsync(H.acc, 0, 2 * sizeof(PkAcc), s));
    if (nrec && (rc = stage_pieces(d_rec, F.sec[4].p + 4, (size_t)nrec * 44, s, release))) return rc;
    if ((rc = stage_pieces(H.a, F.sec[9].p, (size_t)n * 64, s, release))) return rc;
    if ((rc = stage_pieces(K->pointsA.p, F.sec[5].p, (size_t)nv * 64, s, release))) return rc;
    if ((rc = stage_pieces(K->pointsB1.p, F.sec[6].p, (size_t)nv * 64, s, release))) return rc;
    if ((rc = stage_pieces(K->pointsB2.p, F.sec[7].p, (size_t)nv * 128, s, release))) return rc;
    // C holds points for the signals nPublic + 1 .. only: the resident copy is padded in front with infinities (prove.hip)
    const size_t c_front = ((size_t)F.n_public + 1) * 64;
    WS_HIP_CHECK(hipMemsetAsync(K->pointsC.p, 0, c_front, s));
    if (nC && (rc = stage_pieces((uint8_t*)K->pointsC.p + c_front, F.sec[8].p, (size_t)nC * 64, s, release))) return rc;
    WS_HIP_CHECK(hipStreamSynchronize(s));
    const double ms_up = ms_since(t_call);

    // 2. the coefficients: counts and tests, the partition into the matrices' own arrays, the order, the row pointers
    const auto t_coef = Clock::now();
    if (nrec) {
        T.begin("zkey_count", s);
        hipLaunchKernelGGL(zk_count_kernel, dim3(n_tiles), dim3(256), 0, s, (const uint32_t*)d_rec, nrec, tile, F.n_vars, F.domain, d_cnt, acc);
        WS_HIP_CHECK(hipGetLastError());
        T.end(s);
    }
    if ((rc = scan_exclusive_dev(d_cnt, n_tiles + 1, d_tiles, d_base, d_cursor, s))) return rc;
    ZkAcc h_acc;
    uint32_t n0 = 0;
    WS_HIP_CHECK(hipMemcpyAsync(&h_acc, acc, sizeof h_acc, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipMemcpyAsync(&n0, d_base + n_tiles, 4, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    if (h_acc.bad_matrix) return fmt("matrix > 1 in a coefficient record, first at record " + std::to_string(~h_acc.bad_matrix));
    if (h_acc.bad_signal) return fmt("signal >= nVars in a coefficient record, first at record " + std::to_string(~h_acc.bad_signal));
    if (h_acc.bad_constraint) return fmt("constraint >= domainSize in a coefficient record, first at record " + std::to_string(~h_acc.bad_constraint));
    const uint32_t cnt[2] = {n0, nrec - n0};
    CsrMatrix* const M[2] = {&K->polsA, &K->polsB};
    uint32_t* const m_row[2] = {d_row, d_row + n0};
    for (int m = 0; m < 2; m++) {
        const size_t nz = std::max<uint32_t>(cnt[m], 1);
        M[m]->n_rows = F.domain; M[m]->n_cols = F.n_vars; M[m]->nnz = cnt[m];
        WS_HIP_CHECK(M[m]->row_ptr.alloc(((size_t)n + 1) * 4));
        WS_HIP_CHECK(M[m]->col.alloc(nz * 4));
        WS_HIP_CHECK(M[m]->coef.alloc(nz * sizeof(Fe)));
    }
    if (nrec) {
        const ZkParts parts{{M[0]->col.as<uint32_t>(), M[1]->col.as<uint32_t>()}, {m_row[0], m_row[1]}, {M[0]->coef.as<Fe>(), M[1]->coef.as<Fe>()}};
        T.begin("zkey_partition", s);
        hipLaunchKernelGGL(zk_partition_kernel<true>, dim3(n_tiles), dim3(256), 0, s, (const uint32_t*)d_rec, nrec, tile / 256, (const uint32_t*)d_base, parts, acc);
        WS_HIP_CHECK(hipGetLastError());
        T.end(s);
        T.begin("zkey_order", s);
        for (int m = 0; m < 2; m++)
            if (cnt[m] > 1) hipLaunchKernelGGL(zk_order_kernel, dim3(ceil_div_u64(cnt[m], 256)), dim3(256), 0, s, (const uint32_t*)m_row[m], cnt[m], &acc->unsorted[m]);
        WS_HIP_CHECK(hipGetLastError());
        T.end(s);
        WS_HIP_CHECK(hipMemcpyAsync(&h_acc, acc, sizeof h_acc, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));
    }
    {
        SortBufs SB;
        Slab sort_slab;
        DevBuf col2[2], coef2[2];      // (what a sorted matrix's arrays were: freed behind the queue's last reader, at the end of this block)
        if (nrec && (h_acc.unsorted[0] || h_acc.unsorted[1])) {
            SB.add(sort_slab, std::max(h_acc.unsorted[0] ? cnt[0] : 0u, h_acc.unsorted[1] ? cnt[1] : 0u), tile);
            WS_HIP_CHECK(sort_slab.alloc());
        }
        for (int m = 0; m < 2; m++) {
            const uint32_t c = cnt[m];
            const uint32_t* rows = m_row[m];
            if (c && h_acc.unsorted[m]) {
                const dim3 grid(ceil_div_u64(c, 256)), block(256);
                int cur = 0;
                hipLaunchKernelGGL(zk_keys_kernel, grid, block, 0, s, (const uint32_t*)m_row[m], (const uint32_t*)nullptr, c, SB.B.key[0], SB.B.val[0]);
                WS_HIP_CHECK(hipGetLastError());
                if ((rc = rows_sort_dev(X, SB.B, c, 0, (uint32_t)bits, &cur, s))) return rc;
                WS_HIP_CHECK(col2[m].alloc((size_t)c * 4));
                WS_HIP_CHECK(coef2[m].alloc((size_t)c * sizeof(Fe)));
                T.begin("zkey_gather", s);
                hipLaunchKernelGGL(zk_gather_kernel, grid, block, 0, s, (const uint32_t*)SB.B.val[cur], c, (const uint32_t*)M[m]->col.as<uint32_t>(),
                                   (const Fe*)M[m]->coef.as<Fe>(), col2[m].as<uint32_t>(), coef2[m].as<Fe>());
                WS_HIP_CHECK(hipGetLastError());
                T.end(s);
                std::swap(M[m]->col.p, col2[m].p); std::swap(M[m]->col.bytes, col2[m].bytes);
                std::swap(M[m]->coef.p, coef2[m].p); std::swap(M[m]->coef.bytes, coef2[m].bytes);
                rows = SB.B.key[cur];
            }
            T.begin("zkey_rowptr", s);
            hipLaunchKernelGGL(zk_rowptr_kernel, dim3(ceil_div_u64(n + 1, 256)), dim3(256), 0, s, rows, c, F.domain, M[m]->row_ptr.as<uint32_t>());
            WS_HIP_CHECK(hipGetLastError());
            T.end(s);
            // (the next matrix's sort reuses the pairs: this one's row pointers are read out of them first, on the same queue)
        }
        WS_HIP_CHECK(hipStreamSynchronize(s));
    }
    const double ms_coef = ms_since(t_coef);

    // 3. H: the forward transform, then -2 w_2n^k per point, where the section lies
    const auto t_h = Clock::now();
    PkAcc h_in;
    void* d_res = nullptr;
    if ((rc = h_basis_dev(X, H.a, H.b, H.sc, H.tw, n, bits, 0, H.acc, &h_in, &d_res, s))) return rc;
    if (h_in.bad) return h_bad_error("zkey import", h_in);
    if (d_res != K->pointsH.p) WS_HIP_CHECK(hipMemcpyAsync(K->pointsH.p, d_res, (size_t)n * 64, hipMemcpyDeviceToDevice, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    const double ms_h = ms_since(t_h);
    slab.buf.release();      // (before the table build is queued: a free waits for the whole device)

    // 4. sections resident: the masks, the conversion, the tables (prove.hip)
    clock.t_phase = Clock::now();
    if ((rc = pkey_load_convert(K.get(), &clock))) return rc;
    if ((rc = pkey_load_finish(X, K.get(), &clock))) return rc;
    K->load_ms[0] = ms_coef;
    K->load_ms[1] = ms_up;
    if (out_vk) {
        q_from_mont(fx, out_vk, 2);                       // alfa1
        q_from_mont(fx + 128, out_vk + 64, 4);            // beta2
        q_from_mont(fx + 256, out_vk + 192, 4);           // gamma2
        q_from_mont(fx + 448, out_vk + 320, 4);           // delta2
        q_from_mont(F.sec[3].p, out_vk + 448, 2 * ((size_t)F.n_public + 1));
    }
    if (rep) {
        wsnark_zkey_report_t R;
        memset(&R, 0, sizeof R);
        for (int m = 0; m < 2; m++) { R.records[m] = cnt[m]; R.unreduced[m] = nrec ? h_acc.unreduced[m] : 0; R.zero[m] = nrec ? h_acc.zero[m] : 0; }
        R.sorted = nrec == 0 || (!h_acc.unsorted[0] && !h_acc.unsorted[1]);
        h_report(h_in, n, &R);
        R.ms[0] = ms_up; R.ms[1] = ms_coef; R.ms[2] = ms_h; R.ms[3] = 0; R.ms[4] = ms_since(t_call);
        *rep = R;
    }
    *out = K.release();
    return WS_OK;
}

int zkey_load_file(const char* path, ProvingKey** out, uint8_t* out_vk, size_t vk_cap, wsnark_zkey_report_t* rep) {
    if (!ctx()) return WS_ERR_NOINIT;
    if (!path || !out || (!out_vk && vk_cap)) return WS_ERR_ARG;
    KeyFile file;
    if (int rc = keyfile_map(path, &file, 0)) return rc;      // (whatever is shorter than a container, an empty file included, is zk_parse's to name)
    static const uint8_t kNoBytes[1] = {0};
    return zkey_load(file.len ? file.base : kNoBytes, file.len, keyfile_release, out, out_vk, vk_cap, rep);
}

// The length of the verification key from the container and section 2 ALONE: what a caller needs to size out_vk of the calls above.
// zk_parse reads the section table and the small sections' payloads; no byte of sections 3 - 9 is touched (zkey_info counts section 4's
// records on the host, which a mapped file of a large key must not pay).
int zkey_vk_len(const uint8_t* zkey, size_t len, size_t* out_len) {
    if (!out_len) return WS_ERR_ARG;
    ZkFile F;
    if (int rc = zk_parse(zkey, len, &F)) return rc;
    *out_len = (size_t)vk_len_of(F.n_public);
    return WS_OK;
}
int zkey_vk_len_file(const char* path, size_t* out_len) {
    if (!path || !out_len) return WS_ERR_ARG;
    KeyFile file;
    if (int rc = keyfile_map(path, &file, 0)) return rc;
    static const uint8_t kNoBytes[1] = {0};
    return zkey_vk_len(file.len ? file.base : kNoBytes, file.len, out_len);
}

}  // namespace wsnark
