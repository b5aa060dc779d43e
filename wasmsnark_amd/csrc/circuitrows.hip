// circuitrows.hip -- a circuit given ROW BY ROW (the form every front end emits: .r1cs, snarkjs' JSON export, gnark, arkworks) into the
// two forms the rest of the library takes: the proving key's column record streams (wsnark_circuit_t: setup_key, check_key_circuit,
// circuit_row_sums, a key's polsA / polsB) and the resident row-major CSR of the witness check (wsnark_circuit_res_t).  No counterpart
// in the reference, whose keys arrive transposed (tools/buildpkey.js:79-89 writes the streams from snarkjs' column dicts).  The
// opposite direction is pols_to_csr (calch.hip).
//
//   the streams (circuit_from_rows): a STABLE partition of the entries by signal -- the order inside a column is the contract: ascending
//     row, and for equal rows the input's order, which in row-major CSR is ascending ENTRY INDEX.  So: sort (signal, entry index) pairs
//     by signal with a stable least-significant-digit radix sort, kBits = 6 bits per pass, ceil(bits(n_vars - 1) / 6) passes (4 at 2^20
//     signals).  One pass:
//       rows_hist_kernel     a tile's digit histogram (LDS atomics: a count is a sum) to hist[digit][tile]
//       scan_exclusive_dev   calch.hip's three scan kernels over the 64 x tiles counters: base[digit][tile]
//       rows_scatter_kernel  lane l of a tile owns entries [l K, l K + K) of it (K = ROWS_TILE / 256): it counts its digits into its own
//                            LDS column cnt[digit][l], one exclusive scan over cnt in digit-major order ranks every (digit, lane) inside
//                            the tile, and the lane walks its entries again in order: position = base[digit][tile] + rank.  Entries of
//                            one digit leave a tile in entry order, tiles follow each other in order: the pass is stable, and NO order
//                            comes from an atomic.
//     THE HOT COLUMN (a real circuit's constant signal sits in 10^5 rows, nearly every other column has 1-3 records) is no case of
//     its own: no lane and no workgroup is tied to a column, a column of 10^6 records costs what 10^6 columns of one record cost.
//     The alternative -- an atomic cursor fill as csr_fill_kernel's, then a sort of every column by entry index -- is one pass over
//     the entries cheaper on a flat circuit, and needs a second algorithm (a segmented workgroup or device-wide sort) for that one column.
//       rows_prepare_kernel  one lane per entry: the pair, the entry's row (binary search in row_ptr; the public rows are entries nnz ..
//                            of A), the smallest entry whose signal is >= n_vars
//       rows_emit_kernel     256 sorted records per workgroup: lane q converts record q's coefficient ((c mod r) R, canonical: one
//                            Montgomery product by R^2 of ANY 256-bit value) and puts its 9 words in LDS; then the workgroup stores the
//                            2304 words with 32-bit stores in output order -- word 9 p + signal + 1 + k for word k of sorted record p,
//                            contiguous but for the 4-byte headers.  Counts the coefficients >= r and those that reduce to 0.
//       rows_header_kernel   one lane per signal: where its records start among the sorted pairs and where the next signal's do (two
//                            binary searches: no per-signal counter, so no atomic that the hot column would pile onto one address, and
//                            no scan of n_vars counters); its `u32 ncoefs` at 4 s + 36 first; empty signals, the longest column
//   the resident CSR (circuit_load_rows): the input IS row-major CSR.  col and coef go up into the handle's own buffers,
//     rows_resident_kernel narrows row_ptr to 32 bits (rows past the last one are empty), appends the public rows and converts the
//     coefficients in place to c R^2 (csr_fill_kernel's comment says why).  No transposition.
//   Nothing in a result depends on the launch geometry: positions are sums of counts, counts are sums, the bad entry is a minimum.
#include <string.h>

#include "keybytes.h"

namespace wsnark {

// ---- device ----
static constexpr uint32_t kBits = 6, kDigits = 1u << kBits;      // digits per radix pass
static constexpr uint32_t kMaxPerLane = 16;                      // a tile is at most 4096 entries: its ranks fit 16 bits

// (RowsAcc, one matrix's running result, is keybytes.h's: zkey.hip enters the sort and the emit below with pairs of its own)

// entry e of a matrix: its signal and its row.  e < nnz: the input's; e >= nnz: public row e - nnz, {signal e - nnz: 1}
__device__ __forceinline__ uint32_t rows_signal(const uint32_t* __restrict__ col, uint32_t nnz, uint32_t e) { return e < nnz ? col[e] : e - nnz; }
__device__ __forceinline__ uint32_t rows_row(const uint64_t* __restrict__ row_ptr, uint32_t n_cons, uint32_t nnz, uint32_t e) {
    if (e >= nnz) return n_cons + (e - nnz);
    uint32_t lo = 0, hi = n_cons;      // largest r with row_ptr[r] <= e (row_ptr[0] = 0 <= e < nnz = row_ptr[n_cons]); it is not empty
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (row_ptr[mid] <= e) lo = mid; else hi = mid; }
    return lo;
}

__global__ __launch_bounds__(256) void rows_prepare_kernel(const uint64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, uint32_t n_cons,
                                                           uint32_t nnz, uint32_t n_entries, uint32_t n_vars, uint32_t* __restrict__ key,
                                                           uint32_t* __restrict__ val, uint32_t* __restrict__ row_of, RowsAcc* __restrict__ acc) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_entries) return;
    const uint32_t sig = rows_signal(col, nnz, e);
    val[e] = e;
    row_of[e] = rows_row(row_ptr, n_cons, nnz, e);
    if (sig >= n_vars) {      // (nothing is indexed by it: the host stops before the sort)
        key[e] = 0;
        atomicMax(&acc->first_bad, ~(unsigned long long)e);
        return;
    }
    key[e] = sig;
}

// hist[d x n_tiles + t] = how many keys of tile t have digit d
__global__ __launch_bounds__(256) void rows_hist_kernel(const uint32_t* __restrict__ key, uint32_t n, uint32_t tile, uint32_t shift,
                                                        uint32_t* __restrict__ hist, uint32_t n_tiles) {
    __shared__ uint32_t h[kDigits];
    if (threadIdx.x < kDigits) h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t e0 = (uint64_t)blockIdx.x * tile, e1 = e0 + tile < n ? e0 + tile : n;
    for (uint64_t e = e0 + threadIdx.x; e < e1; e += 256) atomicAdd(&h[(key[e] >> shift) & (kDigits - 1)], 1u);
    __syncthreads();
    if (threadIdx.x < kDigits) hist[threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

// counter (digit d, lane l) of a tile at linear index d x 256 + l, one word of padding per 64 so that the scan's lanes (64
// consecutive counters each) start on different banks
__device__ __forceinline__ uint32_t rows_slot(uint32_t i) { return i + (i >> 6); }

// base: the exclusive scan of rows_hist_kernel's counters.  per_lane = tile / 256 <= kMaxPerLane.
__global__ __launch_bounds__(256) void rows_scatter_kernel(const uint32_t* __restrict__ key_in, const uint32_t* __restrict__ val_in, uint32_t n,
                                                           uint32_t per_lane, uint32_t shift, const uint32_t* __restrict__ base, uint32_t n_tiles,
                                                           uint32_t* __restrict__ key_out, uint32_t* __restrict__ val_out) {
    __shared__ uint16_t cnt[kDigits * 256 + kDigits * 4];
    __shared__ uint32_t part[256];
    __shared__ uint32_t first[kDigits];      // base[d][tile] - (the tile's entries of smaller digits)
    const uint32_t l = threadIdx.x;
    for (uint32_t d = 0; d < kDigits; d++) cnt[rows_slot(d * 256 + l)] = 0;
    const uint64_t t0 = (uint64_t)blockIdx.x * 256 * per_lane + (uint64_t)l * per_lane;
    const uint64_t e0 = t0 < n ? t0 : n, e1 = t0 + per_lane < n ? t0 + per_lane : n;
    for (uint64_t e = e0; e < e1; e++) cnt[rows_slot(((key_in[e] >> shift) & (kDigits - 1)) * 256 + l)]++;
    __syncthreads();
    // exclusive scan in digit-major order: lane l owns counters [64 l, 64 l + 64) = digit l / 4, lanes 64 (l % 4) ..
    uint32_t sum = 0;
    for (uint32_t j = 0; j < 64; j++) sum += cnt[rows_slot(64 * l + j)];
    part[l] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t x = l >= d ? part[l - d] : 0;
        __syncthreads();
        part[l] += x;
        __syncthreads();
    }
    uint32_t run = part[l] - sum;
    for (uint32_t j = 0; j < 64; j++) {
        const uint32_t s = rows_slot(64 * l + j), x = cnt[s];
        cnt[s] = (uint16_t)run;
        run += x;
    }
    __syncthreads();
    if (l < kDigits) first[l] = base[l * n_tiles + blockIdx.x] - cnt[rows_slot(l * 256)];
    __syncthreads();
    for (uint64_t e = e0; e < e1; e++) {
        const uint32_t k = key_in[e], d = (k >> shift) & (kDigits - 1), s = rows_slot(d * 256 + l);
        const uint32_t pos = first[d] + cnt[s];
        cnt[s]++;
        key_out[pos] = k;
        val_out[pos] = val_in[e];
    }
}

// how many of the n sorted keys are < s
__device__ __forceinline__ uint32_t rows_lower_bound(const uint32_t* __restrict__ key, uint32_t n, uint32_t s) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (key[mid] < s) lo = mid + 1; else hi = mid; }
    return lo;
}
// One lane per signal: where its records start among the SORTED keys and where the next signal's do -- two binary searches, no
// counter and no atomic (a count per signal by atomicAdd would put the hot column's 10^5 .. 10^6 additions on one address).  words:
// the stream as 32-bit words.  The two statistics leave a workgroup as at most two atomics: the empty signals are summed over its four
// wavefronts in LDS first, and the longest column (a maximum per wavefront, then per workgroup) is offered only where it beats the
// value read back -- a stale read costs one atomic too many, never a wrong maximum.  (One atomicMax per wavefront on the one address
// was most of this kernel's time at 2^20 signals.)
__global__ __launch_bounds__(256) void rows_header_kernel(const uint32_t* __restrict__ key, uint32_t n_entries, uint32_t n_vars,
                                                          uint32_t* __restrict__ words, RowsAcc* __restrict__ acc) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c = 0;
    const bool live = s < n_vars;
    if (live) {
        const uint32_t first = rows_lower_bound(key, n_entries, s);
        c = rows_lower_bound(key, n_entries, s + 1) - first;
        words[(uint64_t)s + 9 * (uint64_t)first] = c;
    }
    __shared__ uint32_t wave_empty[4], wave_most[4];
    const unsigned long long empty = __ballot(live && c == 0);
    uint32_t most = c;
    for (int m = 1; m < 64; m <<= 1) { const uint32_t x = __shfl_xor(most, m); most = x > most ? x : most; }
    if ((threadIdx.x & 63) == 0) { wave_empty[threadIdx.x >> 6] = (uint32_t)__popcll(empty); wave_most[threadIdx.x >> 6] = most; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t e = 0, w = 0;
        for (int k = 0; k < 4; k++) { e += wave_empty[k]; w = wave_most[k] > w ? wave_most[k] : w; }
        if (e) atomicAdd(&acc->empty, (unsigned long long)e);
        if (w > *reinterpret_cast<volatile unsigned long long*>(&acc->max_column)) atomicMax(&acc->max_column, (unsigned long long)w);
    }
}
__global__ __launch_bounds__(256) void rows_emit_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, uint32_t n_entries,
                                                        uint32_t nnz, const uint32_t* __restrict__ row_of, const Fe* __restrict__ coef,
                                                        uint32_t* __restrict__ words, RowsAcc* __restrict__ acc) {
    __shared__ uint32_t rec[256 * 9];
    __shared__ uint32_t sig[256];
    const uint64_t rmod[4] = {FrParams::P0, FrParams::P1, FrParams::P2, FrParams::P3};
    const uint32_t l = threadIdx.x;
    const uint64_t p0 = (uint64_t)blockIdx.x * 256, p = p0 + l;
    bool big = false, zero = false;
    if (p < n_entries) {
        const uint32_t e = val[p];
        Fe m = Fr::one();                   // a public row's coefficient 1
        if (e < nnz) {
            const Fe c = coef[e];
            big = pk_ge(c, rmod);
            m = Fr::to_mont(c);             // (c mod r) R, canonical, for any c < 2^256
            zero = pk_zero(m);
        }
        rec[9 * l] = row_of[e];
        for (int k = 0; k < 4; k++) { rec[9 * l + 1 + 2 * k] = (uint32_t)m.l[k]; rec[9 * l + 2 + 2 * k] = (uint32_t)(m.l[k] >> 32); }
        sig[l] = key[p];
    }
    const unsigned long long m_big = __ballot(big), m_zero = __ballot(zero);
    if ((l & 63) == 0) {
        if (m_big) atomicAdd(&acc->unreduced, (unsigned long long)__popcll(m_big));
        if (m_zero) atomicAdd(&acc->zero, (unsigned long long)__popcll(m_zero));
    }
    __syncthreads();
    const uint32_t n_rec = n_entries - p0 < 256 ? (uint32_t)(n_entries - p0) : 256;
    for (uint32_t w = l; w < 9 * n_rec; w += 256) {
        const uint32_t q = w / 9, k = w - 9 * q;
        words[9 * (p0 + q) + sig[q] + 1 + k] = rec[w];
    }
}

// The resident form from the rows themselves.  One lane per index i: row_ptr32[i] for i <= domain (rows past the last one empty; the
// public rows of A one entry each), and entry i < n_entries: the signal checked (and appended for a public row), the coefficient
// in place to c R^2 -- a PLAIN c here, so two products by R^2; a public row's 1 R^2 = to_mont(one).
__global__ __launch_bounds__(256) void rows_resident_kernel(const uint64_t* __restrict__ row_ptr, uint32_t n_cons, uint32_t nnz, uint32_t n_entries,
                                                            uint32_t n_vars, uint32_t domain, uint32_t* __restrict__ row_ptr32,
                                                            uint32_t* __restrict__ col, Fe* __restrict__ coef, RowsAcc* __restrict__ acc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= domain) {
        uint32_t v = n_entries;
        if (i <= n_cons) v = (uint32_t)row_ptr[i];
        else if (i - n_cons < n_entries - nnz) v = nnz + (i - n_cons);
        row_ptr32[i] = v;
    }
    if (i >= n_entries) return;
    if (i < nnz) {
        if (col[i] >= n_vars) atomicMax(&acc->first_bad, ~(unsigned long long)i);
        coef[i] = Fr::to_mont(Fr::to_mont(coef[i]));
    } else {
        col[i] = i - nnz;
        coef[i] = Fr::to_mont(Fr::one());
    }
}

// ---- host ----
namespace {
const char* const kMatrixName[3] = {"A", "B", "C"};

struct RowsPlan {
    uint32_t n_vars = 0, n_cons = 0, n_pub_rows = 0, domain = 0;
    const wsnark_rows_matrix_t* M[3] = {nullptr, nullptr, nullptr};
    uint64_t nnz[3] = {0, 0, 0}, entries[3] = {0, 0, 0}, lens[3] = {0, 0, 0};
};

// everything the host can say about the rows before any device work, with the codes of include/wsnark.h
int rows_plan(const wsnark_rows_t* R, uint32_t flags, RowsPlan* P) {
    if (!R || (flags & ~WSNARK_ROWS_PUBLIC_ROWS)) return WS_ERR_ARG;
    P->M[0] = &R->A; P->M[1] = &R->B; P->M[2] = &R->C;
    for (int m = 0; m < 3; m++)
        if (!P->M[m]->row_ptr || !P->M[m]->col || !P->M[m]->coef) return WS_ERR_ARG;
    if (int rc = key_vars_check(R->n_vars, R->n_public)) return rc;
    if (R->n_vars > (1u << 30)) { set_last_error("circuit rows: more than 2^30 signals"); return WS_ERR_SIZE; }
    P->n_vars = R->n_vars; P->n_cons = R->n_constraints;
    P->n_pub_rows = (flags & WSNARK_ROWS_PUBLIC_ROWS) ? R->n_public + 1 : 0;
    for (int m = 0; m < 3; m++) {
        const uint64_t* rp = P->M[m]->row_ptr;
        bool ok = rp[0] == 0;
        for (uint64_t i = 0; ok && i < R->n_constraints; i++) ok = rp[i] <= rp[i + 1];
        if (!ok) { set_last_error(std::string("circuit rows: row_ptr of ") + kMatrixName[m] + " does not start at 0 or decreases"); return WS_ERR_FORMAT; }
        P->nnz[m] = rp[R->n_constraints];
        P->entries[m] = P->nnz[m] + (m == 0 ? P->n_pub_rows : 0);
        if (P->entries[m] >= ((uint64_t)1 << 32)) { set_last_error(std::string("circuit rows: 2^32 records or more in ") + kMatrixName[m]); return WS_ERR_SIZE; }
        P->lens[m] = 4 * (uint64_t)R->n_vars + 36 * P->entries[m];
    }
    const uint64_t total = (uint64_t)R->n_constraints + P->n_pub_rows;
    uint64_t dom = R->domain;
    if (dom == 0) for (dom = 2; dom < total; dom <<= 1) {}
    if (dom < 2 || (dom & (dom - 1)) || dom > ((uint64_t)1 << 24) || dom < total) {
        set_last_error("circuit rows: the domain must be a power of two in [2, 2^24] that holds every row");
        return WS_ERR_SIZE;
    }
    P->domain = (uint32_t)dom;
    return WS_OK;
}

// a timer bracket that is closed on every way out of its scope
struct TimerScope {
    KernelTimer& T;
    hipStream_t s;
    TimerScope(KernelTimer& T_, const char* name, hipStream_t s_) : T(T_), s(s_) { T.begin(name, s); }
    ~TimerScope() { T.end(s); }
    TimerScope(const TimerScope&) = delete;
    TimerScope& operator=(const TimerScope&) = delete;
};

// (Slab, the pieces of ONE device allocation, is keybytes.h's)
int bad_entry_error(int m, unsigned long long first_bad) {
    set_last_error(std::string("circuit rows: a signal index >= nVars in ") + kMatrixName[m] + ", first at entry " + std::to_string(~first_bad));
    return WS_ERR_FORMAT;
}
}  // namespace

int rows_tile(uint32_t* tile) {
    const long tile_asked = tuning_get("ROWS_TILE", 2048);
    if (tile_asked < 256 || tile_asked > 256 * (long)kMaxPerLane || tile_asked % 256) {
        set_last_error("circuit rows: ROWS_TILE must be a multiple of 256 in [256, 4096]");
        return WS_ERR_ARG;
    }
    *tile = (uint32_t)tile_asked;
    return WS_OK;
}

// the stable sort of the n pairs (key, val) of B.key / B.val[*cur] by bits [first_bit, first_bit + bits) of the key: ceil(bits / 6)
// passes, each one hist / scan / scatter into the other pair of arrays; *cur names the pair that holds the result
int rows_sort_dev(Context* X, const RowsSort& B, uint32_t n, uint32_t first_bit, uint32_t bits, int* cur, hipStream_t s) {
    KernelTimer& T = X->timer;
    const uint32_t passes = (bits + kBits - 1) / kBits, per_lane = B.tile / 256, n_tiles = ceil_div_u64(n, B.tile);
    int c = *cur, rc;
    for (uint32_t pass = 0; pass < passes && n; pass++, c ^= 1) {
        const uint32_t shift = first_bit + pass * kBits;
        {
            TimerScope t(T, "rows_hist", s);
            hipLaunchKernelGGL(rows_hist_kernel, dim3(n_tiles), dim3(256), 0, s, B.key[c], n, B.tile, shift, B.hist, n_tiles);
            WS_HIP_CHECK(hipGetLastError());
        }
        {
            TimerScope t(T, "rows_scan", s);
            if ((rc = scan_exclusive_dev(B.hist, kDigits * n_tiles, B.tiles, B.base, B.cursor, s))) return rc;
        }
        {
            TimerScope t(T, "rows_scatter", s);
            hipLaunchKernelGGL(rows_scatter_kernel, dim3(n_tiles), dim3(256), 0, s, B.key[c], B.val[c], n, per_lane, shift, B.base, n_tiles,
                               B.key[c ^ 1], B.val[c ^ 1]);
            WS_HIP_CHECK(hipGetLastError());
        }
    }
    *cur = c;
    return WS_OK;
}

// one record stream from the n pairs sorted by signal: the headers, then the records (entry e: row d_row[e], coefficient d_coef[e],
// any 256-bit value; e >= nnz: a public row's 1); the counts into d_acc
int rows_emit_dev(Context* X, const uint32_t* d_key, const uint32_t* d_val, uint32_t n, uint32_t nnz, uint32_t n_vars, const uint32_t* d_row,
                  const Fe* d_coef, uint32_t* d_words, RowsAcc* d_acc, hipStream_t s) {
    KernelTimer& T = X->timer;
    {
        TimerScope t(T, "rows_header", s);
        hipLaunchKernelGGL(rows_header_kernel, dim3(ceil_div_u64(n_vars, 256)), dim3(256), 0, s, d_key, n, n_vars, d_words, d_acc);
        WS_HIP_CHECK(hipGetLastError());
    }
    {
        TimerScope t(T, "rows_emit", s);
        if (n) hipLaunchKernelGGL(rows_emit_kernel, dim3(ceil_div_u64(n, 256)), dim3(256), 0, s, d_key, d_val, n, nnz, d_row, d_coef, d_words, d_acc);
        WS_HIP_CHECK(hipGetLastError());
    }
    return WS_OK;
}

int circuit_from_rows_size(const wsnark_rows_t* R, uint32_t flags, uint32_t* domain, uint64_t lens[3]) {
    if (!domain || !lens) return WS_ERR_ARG;
    RowsPlan P;
    if (int rc = rows_plan(R, flags, &P)) return rc;
    *domain = P.domain;
    for (int m = 0; m < 3; m++) lens[m] = P.lens[m];
    return WS_OK;
}

int circuit_from_rows(const wsnark_rows_t* R, uint32_t flags, void* const out[3], const uint64_t cap[3], uint32_t* domain, wsnark_rows_report_t* rep) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    const auto t_call = Clock::now();
    if (!out[0] || !out[1] || !out[2] || !domain || !rep) return WS_ERR_ARG;
    RowsPlan P;
    if (int rc = rows_plan(R, flags, &P)) return rc;
    for (int m = 0; m < 3; m++)
        if (cap[m] < P.lens[m]) { set_last_error(std::string("circuit rows: the capacity of pols") + kMatrixName[m] + " is below its length"); return WS_ERR_SIZE; }

    const uint32_t nv = P.n_vars;
    uint32_t tile;
    if (int rc = rows_tile(&tile)) return rc;
    uint32_t bits = 0;
    while (bits < 32 && ((uint64_t)1 << bits) < nv) bits++;      // bits of n_vars - 1
    const uint64_t most = std::max(P.entries[0], std::max(P.entries[1], P.entries[2]));
    const uint32_t most_tiles = ceil_div_u64(std::max<uint64_t>(most, 1), tile);
    const uint32_t n_hist = kDigits * most_tiles;
    static_assert(kDigits == 64, "rows_sort_counters (keybytes.h) counts 64 digits per tile");

    LaneLock L = acquire_lane(X);
    hipStream_t s = L->stream;
    KernelTimer& T = X->timer;
    // inputs and outputs of the three matrices, one set of scratch for the matrix at work
    uint64_t* d_rp[3]; uint32_t* d_col[3]; Fe* d_coef[3]; uint32_t* d_out[3];
    uint32_t *d_key[2], *d_val[2], *d_row, *d_cursor, *d_hist, *d_base, *d_tiles;
    RowsAcc* d_acc;
    Slab slab;
    for (int m = 0; m < 3; m++) {
        slab.add((void**)&d_rp[m], ((size_t)P.n_cons + 1) * 8);
        slab.add((void**)&d_col[m], (size_t)P.nnz[m] * 4);
        slab.add((void**)&d_coef[m], (size_t)P.nnz[m] * 32);
        slab.add((void**)&d_out[m], (size_t)P.lens[m]);
    }
    for (int k = 0; k < 2; k++) { slab.add((void**)&d_key[k], (size_t)most * 4); slab.add((void**)&d_val[k], (size_t)most * 4); }
    slab.add((void**)&d_row, (size_t)most * 4);
    slab.add((void**)&d_cursor, (size_t)n_hist * 4);             // (the scan's second output: not used here)
    slab.add((void**)&d_hist, (size_t)n_hist * 4);
    slab.add((void**)&d_base, (size_t)n_hist * 4);
    slab.add((void**)&d_tiles, (size_t)ceil_div_u64(n_hist, 1024) * 4);
    slab.add((void**)&d_acc, 3 * sizeof(RowsAcc));
    WS_HIP_CHECK(slab.alloc());
    const RowsSort B{{d_key[0], d_key[1]}, {d_val[0], d_val[1]}, d_hist, d_base, d_cursor, d_tiles, tile};

    // 1. up, through the staging ring
    int rc;
    for (int m = 0; m < 3; m++) {
        if ((rc = upload_staged(d_rp[m], P.M[m]->row_ptr, ((size_t)P.n_cons + 1) * 8, s))) return rc;
        if (P.nnz[m] && (rc = upload_staged(d_col[m], P.M[m]->col, (size_t)P.nnz[m] * 4, s))) return rc;
        if (P.nnz[m] && (rc = upload_staged(d_coef[m], P.M[m]->coef, (size_t)P.nnz[m] * 32, s))) return rc;
    }
    WS_HIP_CHECK(hipMemsetAsync(d_acc, 0, 3 * sizeof(RowsAcc), s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    const double ms_up = ms_since(t_call);

    // 2. the transposition, one matrix after the other
    const auto t_kernels = Clock::now();
    RowsAcc acc[3];
    for (int m = 0; m < 3; m++) {
        const uint32_t n = (uint32_t)P.entries[m], nnz = (uint32_t)P.nnz[m];
        {
            TimerScope t(T, "rows_prepare", s);
            if (n) hipLaunchKernelGGL(rows_prepare_kernel, dim3(ceil_div_u64(n, 256)), dim3(256), 0, s, d_rp[m], d_col[m], P.n_cons, nnz, n, nv,
                                      d_key[0], d_val[0], d_row, d_acc + m);
            WS_HIP_CHECK(hipGetLastError());
        }
        WS_HIP_CHECK(hipMemcpyAsync(&acc[m], d_acc + m, sizeof(RowsAcc), hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));
        if (acc[m].first_bad) return bad_entry_error(m, acc[m].first_bad);
        int cur = 0;
        if ((rc = rows_sort_dev(X, B, n, 0, bits, &cur, s))) return rc;
        if ((rc = rows_emit_dev(X, d_key[cur], d_val[cur], n, nnz, nv, d_row, d_coef[m], d_out[m], d_acc + m, s))) return rc;
    }
    WS_HIP_CHECK(hipMemcpyAsync(acc, d_acc, sizeof acc, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    const double ms_kernels = ms_since(t_kernels);

    // 3. down
    const auto t_down = Clock::now();
    for (int m = 0; m < 3; m++) WS_HIP_CHECK(hipMemcpyAsync(out[m], d_out[m], (size_t)P.lens[m], hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    wsnark_rows_report_t Rp;
    memset(&Rp, 0, sizeof Rp);
    for (int m = 0; m < 3; m++) {
        Rp.nnz[m] = P.entries[m];
        Rp.unreduced[m] = acc[m].unreduced;
        Rp.zero[m] = acc[m].zero;
        Rp.empty_signals[m] = acc[m].empty;
        Rp.max_column[m] = acc[m].max_column;
    }
    Rp.ms[0] = ms_up; Rp.ms[1] = ms_kernels; Rp.ms[2] = ms_since(t_down); Rp.ms[3] = ms_since(t_call);
    *domain = P.domain;
    *rep = Rp;
    return WS_OK;
}

int circuit_load_rows(const wsnark_rows_t* R, uint32_t flags, CircuitRes** out) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (!out) return WS_ERR_ARG;
    const auto t0 = Clock::now();
    RowsPlan P;
    if (int rc = rows_plan(R, flags, &P)) return rc;
    std::unique_ptr<CircuitRes> H(new CircuitRes());
    H->owner = X; H->n_vars = P.n_vars; H->n_public = R->n_public; H->domain = P.domain;
    {
        LaneLock L = acquire_lane(X);
        hipStream_t s = L->stream;
        DevBuf d_rp, d_acc;
        WS_HIP_CHECK(d_rp.alloc(((size_t)P.n_cons + 1) * 8));
        WS_HIP_CHECK(d_acc.alloc(3 * sizeof(RowsAcc)));
        WS_HIP_CHECK(hipMemsetAsync(d_acc.p, 0, 3 * sizeof(RowsAcc), s));
        for (int m = 0; m < 3; m++) {
            CsrMatrix& M = H->M[m];
            const uint32_t n = (uint32_t)P.entries[m], nnz = (uint32_t)P.nnz[m];
            const size_t nz = n ? n : 1;
            M.n_rows = P.domain; M.n_cols = P.n_vars; M.nnz = n;
            WS_HIP_CHECK(M.row_ptr.alloc(((size_t)P.domain + 1) * 4));      // (the sizes of pols_to_csr: wsnark_circuit_info's bytes)
            WS_HIP_CHECK(M.col.alloc(nz * 4));
            WS_HIP_CHECK(M.coef.alloc(nz * sizeof(Fe)));
            int rc;
            if ((rc = upload_staged(d_rp.p, P.M[m]->row_ptr, ((size_t)P.n_cons + 1) * 8, s))) return rc;
            if (nnz && (rc = upload_staged(M.col.p, P.M[m]->col, (size_t)nnz * 4, s))) return rc;
            if (nnz && (rc = upload_staged(M.coef.p, P.M[m]->coef, (size_t)nnz * 32, s))) return rc;
            {
            TimerScope t(X->timer, "rows_resident", s);
            hipLaunchKernelGGL(rows_resident_kernel, dim3(ceil_div_u64(std::max<uint64_t>((uint64_t)P.domain + 1, n), 256)), dim3(256), 0, s,
                               d_rp.as<uint64_t>(), P.n_cons, nnz, n, P.n_vars, P.domain, M.row_ptr.as<uint32_t>(), M.col.as<uint32_t>(),
                               M.coef.as<Fe>(), d_acc.as<RowsAcc>() + m);
            WS_HIP_CHECK(hipGetLastError());
            }
            WS_HIP_CHECK(hipStreamSynchronize(s));      // (d_rp goes up again for the next matrix)
        }
        RowsAcc acc[3];
        WS_HIP_CHECK(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));
        for (int m = 0; m < 3; m++)
            if (acc[m].first_bad) return bad_entry_error(m, acc[m].first_bad);
    }
    H->load_ms = ms_since(t0);
    *out = H.release();
    return WS_OK;
}

}  // namespace wsnark
