// witcheck.hip -- does this witness satisfy its circuit, and if not, which constraints fail and with what values?  (snarkjs: `wtns check
// <r1cs> <wtns>`; no counterpart in the reference.)  The prover evaluates a = A.w and b = B.w and takes a o b on the domain as C.w
// (src/bn128.js:126-166): a proving key holds no C matrix, so a witness that breaks a constraint proves like any other and the proof
// is rejected by every verifier without a word about why.  This is the step between the witness generator and the prover.
//
//   resident circuit: the three matrices as row-major CSR (circuit_to_csr: the loaders' transposition), made once per circuit.  The
//     handle is read-only after the load; everything a check writes belongs to the call (buffers of the lane the call holds), so any
//     number of threads may check witnesses on one handle at once.
//   lc_check_kernel: one lane per constraint row, 256-lane workgroups.  a, b, c = the row's three dot products (lc_row_dot: the
//     radix-2^29 field, canonical Montgomery sums), bad iff a b != c.  A wavefront's 64 verdicts leave as ONE 64-bit word of the
//     bad-row bitmask (__ballot, stored by lane 0); the count (popcount) and the smallest bad index (first set bit) cost two atomics
//     per wavefront THAT HAS a bad row, none otherwise.  A wavefront runs as long as its longest row, as in lc_spmv2_kernel.
//   witness_facts_kernel: one lane per signal: witness[0] == 1; how many signals are >= r, the first of them, how many of them public.
//   lc_row_values_kernel: for the listed rows only (at most `cap`), a | b | c out of Montgomery form.
//   Nothing in a result depends on the launch geometry: the mask is indexed by row, the count is a sum, the first index a minimum.
//   The bitmask (domain / 8 bytes) comes to the host only when bad > 0 and the caller asked for a list; a good witness costs one
//   48-byte download.
//
//   many witnesses of one resident circuit in one call (wsnark_circuit_witness_check_batch[_dev]): verdict i and witness i's lists are
//   field for field what the single call reports for witness i.  The three kernels above with a witness dimension, one launch each per
//   pass of `chunk` witnesses (WITCHECK_BATCH_CHUNK, else what a fixed byte budget holds):
//   lc_check_batch_kernel: ONE flat index over (witness, row): witness = index >> log_pad, row = index & (pad - 1), pad = max(64,
//     domain).  The grid is one-dimensional -- no grid dimension is the witness count (gridDim.y / .z stop at 65535, a call may hold
//     65536 witnesses) -- and the host keeps chunk x pad <= 2^30.  A domain is a power of two, so from 64 rows on a wavefront lies
//     inside one witness and its ballot word is word (row >> 6) of THAT witness's mask (max(1, domain / 64) words each, back to back).
//     DOMAINS BELOW 64: a wavefront is wider than a witness's rows.  Every witness is padded to one whole wavefront: lanes domain .. 63
//     idle (they vote "good"), the ballot word is the witness's single mask word, and no word or counter is shared by two witnesses.
//     The other layout -- 64 / domain witnesses per wavefront, the ballot word cut up -- saves idle lanes of launches that are a few
//     wavefronts anyway and needs a shift and a mask per witness exactly where an off-by-one stays silent.
//     Each witness has its own WitAcc: two atomics per wavefront that has a bad row, on that witness's counters; a good batch issues none.
//   witness_facts_batch_kernel: the same over (witness, signal), every witness padded to whole wavefronts (nVars is any number).
//   mask_gather_batch_kernel: the masks of the witnesses with bad > 0, picked out on the device into one run: one launch and one
//     download whichever and however many they are (none when cap == 0 or the pass is all good).
//   lc_row_values_batch_kernel: a | b | c for a list of (witness, row) pairs: one launch per pass, not one per bad witness.
//   A pass costs one memset, two launches and one download of chunk x 48 bytes; with bad witnesses and cap > 0 two more launches and
//   two more downloads, whatever their number.  Results are indexed by (witness, row), sums and minima: neither the launch geometry nor
//   the pass size shows in them.
#include <string.h>

#include "keybytes.h"

namespace wsnark {

// ---- device ----
// one call's running result; first_* hold ~index of the smallest index found (0 = none) so that atomicMax finds the minimum (PkAcc)
struct WitAcc { unsigned long long bad, first_bad, unreduced, first_unreduced, unreduced_public, one_ok; };

struct CheckTriple { const uint32_t* row_ptr[3]; const uint32_t* col[3]; const Fe* coef[3]; };

// v[m] = (row r of matrix m) . w, m = A, B, C: Montgomery and canonical.  One copy of the dot product's code, run three times: the
// matrix index is uniform over the launch
__device__ __forceinline__ void lc_row_abc(const CheckTriple& M, const Fe* __restrict__ w, uint32_t r, Fe* a, Fe* b, Fe* c) {
#pragma unroll 1
    for (int m = 0; m < 3; m++) {
        const uint32_t* __restrict__ rp = M.row_ptr[m];
        const Fe v = lc_row_dot(M.coef[m], M.col[m], w, rp[r], rp[r + 1]);
        if (m == 0) *a = v;
        else if (m == 1) *b = v;
        else *c = v;
    }
}

// mask: n_words = max(1, n_rows / 64) words, bit (r & 63) of word (r >> 6) set iff row r is bad.  Lanes past the last row vote "good"
// (every lane of a wavefront reaches the ballot); a wavefront wholly past it stores nothing.
__global__ __launch_bounds__(256) void lc_check_kernel(CheckTriple M, const Fe* __restrict__ w, uint32_t n_rows,
                                                       unsigned long long* __restrict__ mask, uint32_t n_words, WitAcc* __restrict__ acc) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (r < n_rows) {
        Fe a, b, c;
        lc_row_abc(M, w, r, &a, &b, &c);
        bad = !Fr::eq(Fr::mul(a, b), c);      // a R . b R . R^-1 = a b R against c R, both canonical
    }
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0) {
        const uint32_t word = r >> 6;
        if (word < n_words) mask[word] = m;
        if (m) {
            atomicAdd(&acc->bad, (unsigned long long)__popcll(m));
            atomicMax(&acc->first_bad, ~((unsigned long long)r + (unsigned long long)(__ffsll(m) - 1)));
        }
    }
}

// out[3 j .. 3 j + 2] = a, b, c of row rows[j], plain and canonical
__global__ __launch_bounds__(256) void lc_row_values_kernel(CheckTriple M, const Fe* __restrict__ w, const unsigned long long* __restrict__ rows,
                                                            uint32_t n_listed, Fe* __restrict__ out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_listed) return;
    Fe a, b, c;
    lc_row_abc(M, w, (uint32_t)rows[j], &a, &b, &c);
    out[3 * (size_t)j] = Fr::from_mont(a);
    out[3 * (size_t)j + 1] = Fr::from_mont(b);
    out[3 * (size_t)j + 2] = Fr::from_mont(c);
}

__global__ __launch_bounds__(256) void witness_facts_kernel(const Fe* __restrict__ w, uint32_t n_vars, uint32_t n_public, WitAcc* __restrict__ acc) {
    const uint64_t rmod[4] = {FrParams::P0, FrParams::P1, FrParams::P2, FrParams::P3};
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool big = false;
    if (i < n_vars) {
        const Fe x = w[i];
        big = pk_ge(x, rmod);
        if (i == 0 && x.l[0] == 1 && (x.l[1] | x.l[2] | x.l[3]) == 0) acc->one_ok = 1;
    }
    const unsigned long long m = __ballot(big), m_pub = __ballot(big && i <= n_public);
    if ((threadIdx.x & 63) == 0 && m) {
        atomicAdd(&acc->unreduced, (unsigned long long)__popcll(m));
        if (m_pub) atomicAdd(&acc->unreduced_public, (unsigned long long)__popcll(m_pub));
        atomicMax(&acc->first_unreduced, ~((unsigned long long)i + (unsigned long long)(__ffsll(m) - 1)));
    }
}


// ---- the same with a witness dimension (the layout: the head of this file) ----
// A wavefront lies inside ONE witness (pad >= 64): its witness index is one value for the wavefront, and said so it stays in scalar
// registers with the witness's base address: 96 VGPRs and five wavefronts per SIMD, as lc_check_kernel (94), where the per-lane
// index took 99 and four.  (The kernel's time at 256 x 2^12 did not move with it: DESIGN.md.)  On the thread emulator a lane is its
// own wavefront.
#ifdef WSNARK_EMUL
#define WITCHECK_WAVE_U32(x) ((uint32_t)(x))
#else
#define WITCHECK_WAVE_U32(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#endif
// witness p of the pass starts p x stride bytes after w; only its first nVars signals are read
struct BatchWit { const uint8_t* w; uint64_t stride; uint32_t count; };
__device__ __forceinline__ const Fe* batch_wit(const BatchWit& W, uint32_t p) { return reinterpret_cast<const Fe*>(W.w + (uint64_t)p * W.stride); }

// mask: count x n_words words, witness p's at p x n_words; acc: one per witness.  pad = 1 << log_pad = max(64, n_rows): lanes past a
// witness's last row and past the last witness vote "good"; a wavefront wholly past the last witness stores nothing.
__global__ __launch_bounds__(256) void lc_check_batch_kernel(CheckTriple M, BatchWit W, uint32_t n_rows, uint32_t log_pad,
                                                             unsigned long long* __restrict__ mask, uint32_t n_words, WitAcc* __restrict__ acc) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t r = (uint32_t)(idx & (((uint64_t)1 << log_pad) - 1));
    const uint32_t p64 = WITCHECK_WAVE_U32(idx >> log_pad);      // (chunk x pad <= 2^30: the index fits)
    const bool live = p64 < W.count;
    const uint32_t p = live ? p64 : 0;
    bool bad = false;
    if (live && r < n_rows) {
        Fe a, b, c;
        lc_row_abc(M, batch_wit(W, p), r, &a, &b, &c);
        bad = !Fr::eq(Fr::mul(a, b), c);
    }
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && live) {
        const uint32_t word = r >> 6;
        if (word < n_words) mask[(uint64_t)p * n_words + word] = m;
        if (m) {
            atomicAdd(&acc[p].bad, (unsigned long long)__popcll(m));
            atomicMax(&acc[p].first_bad, ~((unsigned long long)r + (unsigned long long)(__ffsll(m) - 1)));
        }
    }
}

// waves = ceil(n_vars / 64) wavefronts per witness: wavefront v of the launch holds signals 64 (v % waves) .. of witness v / waves
__global__ __launch_bounds__(256) void witness_facts_batch_kernel(BatchWit W, uint32_t n_vars, uint32_t n_public, uint32_t waves, WitAcc* __restrict__ acc) {
    const uint64_t rmod[4] = {FrParams::P0, FrParams::P1, FrParams::P2, FrParams::P3};
    const uint32_t wave = (uint32_t)(((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const uint32_t p64 = WITCHECK_WAVE_U32(wave / waves);
    const uint64_t i = (uint64_t)(wave - p64 * waves) * 64 + (threadIdx.x & 63);
    const bool live = p64 < W.count;
    const uint32_t p = live ? p64 : 0;
    bool big = false;
    if (live && i < n_vars) {
        const Fe x = batch_wit(W, p)[i];
        big = pk_ge(x, rmod);
        if (i == 0 && x.l[0] == 1 && (x.l[1] | x.l[2] | x.l[3]) == 0) acc[p].one_ok = 1;
    }
    const unsigned long long m = __ballot(big), m_pub = __ballot(big && i <= n_public);
    if ((threadIdx.x & 63) == 0 && m) {      // (m != 0 only where live)
        atomicAdd(&acc[p].unreduced, (unsigned long long)__popcll(m));
        if (m_pub) atomicAdd(&acc[p].unreduced_public, (unsigned long long)__popcll(m_pub));
        atomicMax(&acc[p].first_unreduced, ~((unsigned long long)i + (unsigned long long)(__ffsll(m) - 1)));
    }
}

// out[j n_words .. ] = the mask of witness which[j]
__global__ __launch_bounds__(256) void mask_gather_batch_kernel(const unsigned long long* __restrict__ mask, const uint32_t* __restrict__ which,
                                                                uint32_t n_which, uint32_t n_words, unsigned long long* __restrict__ out) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (uint64_t)n_which * n_words) return;
    const uint32_t j = (uint32_t)(idx / n_words), k = (uint32_t)(idx - (uint64_t)j * n_words);
    out[idx] = mask[(uint64_t)which[j] * n_words + k];
}

// out[3 j .. 3 j + 2] = a, b, c of row (pairs[j] & 2^32 - 1) for witness (pairs[j] >> 32), plain and canonical
__global__ __launch_bounds__(256) void lc_row_values_batch_kernel(CheckTriple M, BatchWit W, const unsigned long long* __restrict__ pairs,
                                                                  uint64_t n_listed, Fe* __restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_listed) return;
    const unsigned long long pr = pairs[j];
    Fe a, b, c;
    lc_row_abc(M, batch_wit(W, (uint32_t)(pr >> 32)), (uint32_t)pr, &a, &b, &c);
    out[3 * j] = Fr::from_mont(a);
    out[3 * j + 1] = Fr::from_mont(b);
    out[3 * j + 2] = Fr::from_mont(c);
}

// ---- host ----
Context* circuit_context(const CircuitRes* H) { return H ? H->owner : nullptr; }

int circuit_load(const wsnark_circuit_t* K, CircuitRes** out) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (!out) return WS_ERR_ARG;
    int rc;
    if ((rc = circuit_shape_check(K))) return rc;
    const auto t0 = Clock::now();
    std::unique_ptr<CircuitRes> H(new CircuitRes());
    H->owner = X; H->n_vars = K->n_vars; H->n_public = K->n_public; H->domain = K->domain;
    {
        LaneLock L = acquire_lane(X);
        if ((rc = circuit_to_csr(K, H->M, L->stream))) return rc;
    }
    H->load_ms = ms_since(t0);
    *out = H.release();
    return WS_OK;
}
void circuit_free(CircuitRes* H) { delete H; }
void circuit_info(const CircuitRes* H, uint32_t* n_vars, uint32_t* n_public, uint32_t* domain, uint64_t nnz[3], uint64_t* bytes) {
    if (n_vars) *n_vars = H->n_vars;
    if (n_public) *n_public = H->n_public;
    if (domain) *domain = H->domain;
    uint64_t total = 0;
    for (int m = 0; m < 3; m++) {
        if (nnz) nnz[m] = H->M[m].nnz;
        total += H->M[m].row_ptr.bytes + H->M[m].col.bytes + H->M[m].coef.bytes;
    }
    if (bytes) *bytes = total;
}

namespace {
CheckTriple triple_of(const CircuitRes* H) {
    CheckTriple T;
    for (int m = 0; m < 3; m++) {
        T.row_ptr[m] = H->M[m].row_ptr.as<uint32_t>();
        T.col[m] = H->M[m].col.as<uint32_t>();
        T.coef[m] = H->M[m].coef.as<Fe>();
    }
    return T;
}

// what every variant rejects before it takes a lane: the pointers (circuit: the struct or the handle), then the witness's length
// once nVars may be read
int check_args(const void* circuit, const void* witness, const uint64_t* bad_rows, const void* bad_values, uint64_t cap,
               const wsnark_witness_report_t* rep) {
    return (!circuit || !witness || !rep || (cap && (!bad_rows || !bad_values))) ? WS_ERR_ARG : WS_OK;
}
int check_len(uint32_t n_vars, size_t witness_len) {
    if (witness_len >= (size_t)n_vars * 32) return WS_OK;
    set_last_error("witness check: the witness is shorter than nVars x 32 bytes");
    return WS_ERR_SIZE;
}

// The check itself on lane L (held by the caller) and queue s, the witness resident at d_w.  The lane's second boundary buffer holds
// the counters and the bitmask, later the listed rows and their values; the report and the lists are written last.
// s may be the CALLER's queue (the _dev variant): the lane's buffer is then written by work queued there, which is safe because every
// path below waits for s before it returns -- nothing of this call is in flight when the lane goes back.
int check_on(const CircuitRes* H, Lane& L, const Fe* d_w, hipStream_t s, uint64_t* bad_rows, void* bad_values, uint64_t cap,
             wsnark_witness_report_t* rep, double ms_matrices, Clock::time_point t_call, Clock::time_point t_dev) {
    Context* X = H->owner;
    const uint32_t n = H->domain, nv = H->n_vars;
    const uint32_t n_words = n >= 64 ? n / 64 : 1;
    const CheckTriple T = triple_of(H);
    DevBuf& buf = L.host_in[1];
    const size_t mask_off = 64;      // the counters, padded
    WS_HIP_CHECK(buf.reserve(mask_off + (size_t)n_words * 8));
    WitAcc* d_acc = buf.as<WitAcc>();
    unsigned long long* d_mask = reinterpret_cast<unsigned long long*>(buf.as<uint8_t>() + mask_off);
    WS_HIP_CHECK(hipMemsetAsync(d_acc, 0, sizeof(WitAcc), s));
    X->timer.begin("witness_facts", s);
    hipLaunchKernelGGL(witness_facts_kernel, dim3(ceil_div_u64(nv, 256)), dim3(256), 0, s, d_w, nv, H->n_public, d_acc);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    X->timer.begin("lc_check", s);
    hipLaunchKernelGGL(lc_check_kernel, dim3(ceil_div_u64(n, 256)), dim3(256), 0, s, T, d_w, n, d_mask, n_words, d_acc);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    WitAcc acc;
    WS_HIP_CHECK(hipMemcpyAsync(&acc, d_acc, sizeof acc, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));

    const uint64_t listed = std::min<uint64_t>(acc.bad, cap);
    std::vector<unsigned long long> rows;
    std::vector<uint8_t> values;
    if (listed) {
        std::vector<unsigned long long> mask(n_words);
        WS_HIP_CHECK(hipMemcpyAsync(mask.data(), d_mask, (size_t)n_words * 8, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));
        rows.reserve((size_t)listed);
        for (uint32_t k = 0; k < n_words && rows.size() < listed; k++)
            for (unsigned long long m = mask[k]; m && rows.size() < listed; m &= m - 1)
                rows.push_back((unsigned long long)k * 64 + (unsigned long long)__builtin_ctzll(m));
        if (rows.size() != listed) { set_last_error("witness check: the bitmask and the count disagree"); return WS_ERR_HIP; }
        const size_t val_off = ((size_t)listed * 8 + 63) & ~(size_t)63;
        WS_HIP_CHECK(buf.reserve(val_off + (size_t)listed * 96));      // (the mask has been read: the buffer may move)
        values.resize((size_t)listed * 96);
        WS_HIP_CHECK(hipMemcpyAsync(buf.p, rows.data(), (size_t)listed * 8, hipMemcpyHostToDevice, s));
        Fe* d_val = reinterpret_cast<Fe*>(buf.as<uint8_t>() + val_off);
        X->timer.begin("lc_row_values", s);
        hipLaunchKernelGGL(lc_row_values_kernel, dim3(ceil_div_u64(listed, 256)), dim3(256), 0, s, T, d_w, buf.as<unsigned long long>(),
                           (uint32_t)listed, d_val);
        WS_HIP_CHECK(hipGetLastError());
        X->timer.end(s);
        WS_HIP_CHECK(hipMemcpyAsync(values.data(), d_val, values.size(), hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));
    }
    // nothing can fail from here on
    for (uint64_t j = 0; j < listed; j++) bad_rows[j] = rows[(size_t)j];
    if (listed) memcpy(bad_values, values.data(), values.size());
    wsnark_witness_report_t R;
    memset(&R, 0, sizeof R);
    R.rows = n;
    R.bad = acc.bad;
    R.first_bad = acc.first_bad ? ~acc.first_bad : UINT64_MAX;
    R.listed = listed;
    R.unreduced = acc.unreduced;
    R.first_unreduced = acc.first_unreduced ? ~acc.first_unreduced : UINT64_MAX;
    R.one_ok = acc.one_ok ? 1 : 0;
    R.ok = (acc.bad == 0 && acc.one_ok && acc.unreduced_public == 0) ? 1 : 0;
    R.ms[0] = ms_matrices;
    R.ms[1] = ms_since(t_dev);
    R.ms[2] = ms_since(t_call);
    *rep = R;
    return WS_OK;
}

int check_host(const CircuitRes* H, const void* witness, uint64_t* bad_rows, void* bad_values, uint64_t cap, wsnark_witness_report_t* rep,
               double ms_matrices, Clock::time_point t_call) {
    LaneLock L = acquire_lane(H->owner);
    hipStream_t s = L->stream;
    const auto t_dev = Clock::now();
    WS_HIP_CHECK(L->host_in[0].reserve((size_t)H->n_vars * 32));
    if (int rc = upload_staged(L->host_in[0].p, witness, (size_t)H->n_vars * 32, s)) return rc;
    return check_on(H, *L, L->host_in[0].as<Fe>(), s, bad_rows, bad_values, cap, rep, ms_matrices, t_call, t_dev);
}
}  // namespace

int circuit_witness_check(CircuitRes* H, const void* witness, size_t witness_len, bool on_device, uint64_t* bad_rows, void* bad_values,
                          uint64_t cap, wsnark_witness_report_t* rep, hipStream_t s) {
    if (!ctx()) return WS_ERR_NOINIT;
    const auto t_call = Clock::now();
    int rc;
    if ((rc = check_args(H, witness, bad_rows, bad_values, cap, rep)) || (rc = check_len(H->n_vars, witness_len))) return rc;
    if (!on_device) return check_host(H, witness, bad_rows, bad_values, cap, rep, 0, t_call);
    if ((uintptr_t)witness % alignof(Fe)) {      // the kernels read whole elements
        set_last_error("witness check: the device witness must be 16-byte aligned");
        return WS_ERR_ARG;
    }
    LaneLock L = acquire_lane(H->owner);
    if (!s) s = L->stream;
    return check_on(H, *L, (const Fe*)witness, s, bad_rows, bad_values, cap, rep, 0, t_call, Clock::now());
}

// load, check, free: the resident call's report and lists (the matrices' time in ms[0])
int witness_check(const wsnark_circuit_t* K, const void* witness, size_t witness_len, uint64_t* bad_rows, void* bad_values, uint64_t cap,
                  wsnark_witness_report_t* rep) {
    if (!ctx()) return WS_ERR_NOINIT;
    const auto t_call = Clock::now();
    int rc;
    if ((rc = check_args(K, witness, bad_rows, bad_values, cap, rep)) || (rc = circuit_shape_check(K)) || (rc = check_len(K->n_vars, witness_len))) return rc;
    CircuitRes* raw = nullptr;
    if ((rc = circuit_load(K, &raw))) return rc;
    std::unique_ptr<CircuitRes> H(raw);
    return check_host(raw, witness, bad_rows, bad_values, cap, rep, raw->load_ms, t_call);
}

// ---- many witnesses in one call ----
namespace {
constexpr size_t kCheckBatchBudget = (size_t)256 << 20;      // device bytes of one pass: the witness copies, masks, counters and lists
size_t up64(size_t b) { return (b + 63) & ~(size_t)63; }

// waits for the call's queue on every exit path: s may be the caller's queue and the buffers written there are the lane's
struct QueueDrain {
    hipStream_t s;
    ~QueueDrain() { (void)hipStreamSynchronize(s); }
};

// what a batch holds back until nothing can fail any more
struct HeldBatch {
    std::vector<WitAcc> acc;                       // one per witness of the call
    std::vector<unsigned long long> pairs;         // (witness of the call << 32) | row, witness by witness, rows ascending
    std::vector<uint8_t> values;                   // 96 bytes per pair
};

// one pass: witnesses [i0, i0 + B) of the call, resident at W
int check_batch_pass(const CircuitRes* H, Lane& L, hipStream_t s, const BatchWit& W, uint64_t i0, uint64_t cap, HeldBatch* out) {
    Context* X = H->owner;
    KernelTimer& T = X->timer;
    const uint32_t n = H->domain, nv = H->n_vars, B = W.count;
    const uint32_t n_words = n >= 64 ? n / 64 : 1;
    uint32_t log_pad = 6;
    while (((uint64_t)1 << log_pad) < n) log_pad++;
    const uint32_t waves = (uint32_t)ceil_div_u64(nv, 64);
    const CheckTriple M = triple_of(H);
    DevBuf& buf = L.host_in[1];
    // counters | masks | the bad witnesses' indices | their masks, gathered
    const size_t mask_off = up64((size_t)B * sizeof(WitAcc)), which_off = mask_off + (size_t)B * n_words * 8;
    const size_t gather_off = which_off + up64((size_t)B * 4);
    WS_HIP_CHECK(buf.reserve(gather_off + (size_t)B * n_words * 8));
    WitAcc* d_acc = buf.as<WitAcc>();
    unsigned long long* d_mask = reinterpret_cast<unsigned long long*>(buf.as<uint8_t>() + mask_off);
    WS_HIP_CHECK(hipMemsetAsync(d_acc, 0, (size_t)B * sizeof(WitAcc), s));
    T.begin("witness_facts_batch", s);
    hipLaunchKernelGGL(witness_facts_batch_kernel, dim3(ceil_div_u64((uint64_t)B * waves * 64, 256)), dim3(256), 0, s, W, nv, H->n_public, waves, d_acc);
    WS_HIP_CHECK(hipGetLastError());
    T.end(s);
    T.begin("lc_check_batch", s);
    hipLaunchKernelGGL(lc_check_batch_kernel, dim3(ceil_div_u64((uint64_t)B << log_pad, 256)), dim3(256), 0, s, M, W, n, log_pad, d_mask, n_words, d_acc);
    WS_HIP_CHECK(hipGetLastError());
    T.end(s);
    WitAcc* acc = &out->acc[(size_t)i0];
    WS_HIP_CHECK(hipMemcpyAsync(acc, d_acc, (size_t)B * sizeof(WitAcc), hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    if (!cap) return WS_OK;

    std::vector<uint32_t> which;
    for (uint32_t p = 0; p < B; p++)
        if (acc[p].bad) which.push_back(p);
    if (which.empty()) return WS_OK;
    const uint32_t nb = (uint32_t)which.size();
    std::vector<unsigned long long> masks((size_t)nb * n_words);
    uint32_t* d_which = reinterpret_cast<uint32_t*>(buf.as<uint8_t>() + which_off);
    unsigned long long* d_gather = reinterpret_cast<unsigned long long*>(buf.as<uint8_t>() + gather_off);
    WS_HIP_CHECK(hipMemcpyAsync(d_which, which.data(), (size_t)nb * 4, hipMemcpyHostToDevice, s));
    T.begin("mask_gather_batch", s);
    hipLaunchKernelGGL(mask_gather_batch_kernel, dim3(ceil_div_u64((uint64_t)nb * n_words, 256)), dim3(256), 0, s, d_mask, d_which, nb, n_words, d_gather);
    WS_HIP_CHECK(hipGetLastError());
    T.end(s);
    WS_HIP_CHECK(hipMemcpyAsync(masks.data(), d_gather, masks.size() * 8, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    const size_t first_pair = out->pairs.size();
    for (uint32_t j = 0; j < nb; j++) {
        const uint64_t listed = std::min<uint64_t>(acc[which[j]].bad, cap);
        uint64_t got = 0;
        for (uint32_t k = 0; k < n_words && got < listed; k++)
            for (unsigned long long m = masks[(size_t)j * n_words + k]; m && got < listed; m &= m - 1, got++)
                out->pairs.push_back(((unsigned long long)(i0 + which[j]) << 32) | ((unsigned long long)k * 64 + (unsigned long long)__builtin_ctzll(m)));
        if (got != listed) { set_last_error("witness check: the bitmask and the count disagree"); return WS_ERR_HIP; }
    }
    // the values: the pairs with the pass's own witness index, then one launch
    const size_t n_pairs = out->pairs.size() - first_pair;
    std::vector<unsigned long long> local(n_pairs);
    for (size_t j = 0; j < n_pairs; j++) local[j] = out->pairs[first_pair + j] - ((unsigned long long)i0 << 32);
    const size_t val_off = up64(n_pairs * 8);
    WS_HIP_CHECK(buf.reserve(val_off + n_pairs * 96));      // (the counters and the masks have been read: the buffer may move)
    out->values.resize((first_pair + n_pairs) * 96);
    WS_HIP_CHECK(hipMemcpyAsync(buf.p, local.data(), n_pairs * 8, hipMemcpyHostToDevice, s));
    Fe* d_val = reinterpret_cast<Fe*>(buf.as<uint8_t>() + val_off);
    T.begin("lc_row_values_batch", s);
    hipLaunchKernelGGL(lc_row_values_batch_kernel, dim3(ceil_div_u64(n_pairs, 256)), dim3(256), 0, s, M, W, buf.as<unsigned long long>(), (uint64_t)n_pairs, d_val);
    WS_HIP_CHECK(hipGetLastError());
    T.end(s);
    WS_HIP_CHECK(hipMemcpyAsync(&out->values[first_pair * 96], d_val, n_pairs * 96, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    return WS_OK;
}
}  // namespace

int circuit_witness_check_batch(CircuitRes* H, const void* witnesses, size_t witness_stride, uint64_t count, bool on_device,
                                wsnark_witness_verdict_t* verdicts, uint64_t* bad_rows, void* bad_values, uint64_t cap,
                                wsnark_witness_batch_report_t* rep, hipStream_t stream) {
    if (!ctx()) return WS_ERR_NOINIT;
    if (!H) return WS_ERR_ARG;
    if (count == 0) return WS_OK;
    if (!witnesses || !verdicts || (cap && (!bad_rows || !bad_values))) return WS_ERR_ARG;
    if (count > ((uint64_t)1 << 16)) { set_last_error("witness check: more than 2^16 witnesses in one call"); return WS_ERR_SIZE; }
    const uint32_t n = H->domain, nv = H->n_vars;
    if (witness_stride < (size_t)nv * 32) { set_last_error("witness check: witness_stride is less than nVars x 32 bytes"); return WS_ERR_SIZE; }
    if (on_device && (((uintptr_t)witnesses | (uintptr_t)witness_stride) % alignof(Fe))) {
        set_last_error("witness check: the device witnesses must be 16-byte aligned (pointer and stride)");
        return WS_ERR_ARG;
    }
    const auto t_call = Clock::now();
    if (count == 1) {
        // A batch of one IS the single call: on an MI355X it was the one shape the batch path lost by more than the loop's spread
        // (2^16, host witness; profiles/witness_check_batch_bench.json), so it goes where the contract points.  check_on writes
        // the lists and its report last, after the last call that can fail.
        wsnark_witness_report_t r;
        if (int rc = circuit_witness_check(H, witnesses, (size_t)nv * 32, on_device, bad_rows, bad_values, cap, &r, stream)) return rc;
        wsnark_witness_verdict_t V;
        memset(&V, 0, sizeof V);
        V.bad = r.bad; V.first_bad = r.first_bad; V.unreduced = r.unreduced; V.first_unreduced = r.first_unreduced;
        V.listed = r.listed; V.one_ok = r.one_ok; V.ok = r.ok;
        verdicts[0] = V;
        if (rep) {
            wsnark_witness_batch_report_t R;
            memset(&R, 0, sizeof R);
            R.count = 1; R.rows = n; R.good = r.ok; R.first_not_ok = r.ok ? UINT64_MAX : 0; R.chunk = 1;
            R.ms[1] = r.ms[1]; R.ms[2] = ms_since(t_call);
            *rep = R;
        }
        return WS_OK;
    }
    // witnesses per pass: what keeps a pass's device bytes under the budget (WITCHECK_BATCH_CHUNK overrides) and its flat lane
    // index under 2^30.  A device batch is read in place: there the chunk only bounds the masks, the counters and the lists.
    const uint64_t n_words = n >= 64 ? n / 64 : 1, pad = n >= 64 ? n : 64, nv_pad = ceil_div_u64(nv, 64) * 64;
    const uint64_t per_witness = (on_device ? 0 : (uint64_t)nv * 32) + 2 * n_words * 8 + 128 + std::min<uint64_t>(cap, n) * 104;
    uint64_t chunk = (uint64_t)std::max<long>(tuning_get("WITCHECK_BATCH_CHUNK", 0), 0);
    if (!chunk) chunk = kCheckBatchBudget / per_witness;
    chunk = std::min<uint64_t>(chunk, ((uint64_t)1 << 30) / std::max<uint64_t>(pad, nv_pad));
    chunk = std::max<uint64_t>(std::min<uint64_t>(chunk, count), 1);

    HeldBatch held;
    held.acc.resize((size_t)count);
    const uint8_t* wb = reinterpret_cast<const uint8_t*>(witnesses);
    double ms_dev = 0;
    {
        LaneLock L = acquire_lane(H->owner);
        hipStream_t s = stream ? stream : L->stream;
        QueueDrain drain{s};
        const auto t_dev = Clock::now();
        if (!on_device) WS_HIP_CHECK(L->host_in[0].reserve((size_t)chunk * nv * 32));
        for (uint64_t i0 = 0; i0 < count; i0 += chunk) {
            const uint32_t B = (uint32_t)std::min<uint64_t>(chunk, count - i0);
            BatchWit W{wb + i0 * witness_stride, (uint64_t)witness_stride, B};
            if (!on_device) {
                // through the staging ring: in one piece when the witnesses are packed, else one after the other
                uint8_t* d = L->host_in[0].as<uint8_t>();
                int rc = WS_OK;
                if (witness_stride == (size_t)nv * 32) rc = upload_staged(d, W.w, (size_t)B * nv * 32, s);
                else for (uint32_t j = 0; j < B && !rc; j++) rc = upload_staged(d + (size_t)j * nv * 32, W.w + (size_t)j * witness_stride, (size_t)nv * 32, s);
                if (rc) return rc;
                W.w = d;
                W.stride = (uint64_t)nv * 32;
            }
            if (int rc = check_batch_pass(H, *L, s, W, i0, cap, &held)) return rc;
        }
        ms_dev = ms_since(t_dev);
    }
    // nothing can fail from here on
    wsnark_witness_batch_report_t R;
    memset(&R, 0, sizeof R);
    R.count = count;
    R.rows = n;
    R.first_not_ok = UINT64_MAX;
    R.chunk = (uint32_t)chunk;
    size_t j = 0;
    for (uint64_t i = 0; i < count; i++) {
        const WitAcc& a = held.acc[(size_t)i];
        wsnark_witness_verdict_t V;
        memset(&V, 0, sizeof V);
        V.bad = a.bad;
        V.first_bad = a.first_bad ? ~a.first_bad : UINT64_MAX;
        V.unreduced = a.unreduced;
        V.first_unreduced = a.first_unreduced ? ~a.first_unreduced : UINT64_MAX;
        V.listed = std::min<uint64_t>(a.bad, cap);
        V.one_ok = a.one_ok ? 1 : 0;
        V.ok = (a.bad == 0 && a.one_ok && a.unreduced_public == 0) ? 1 : 0;
        for (uint64_t k = 0; k < V.listed; k++, j++) {      // (the pairs are in the order of the witnesses)
            bad_rows[i * cap + k] = held.pairs[j] & 0xFFFFFFFFull;
            memcpy((uint8_t*)bad_values + (size_t)(i * cap + k) * 96, &held.values[j * 96], 96);
        }
        verdicts[i] = V;
        if (V.ok) R.good++;
        else if (R.first_not_ok == UINT64_MAX) R.first_not_ok = i;
    }
    R.ms[1] = ms_dev;
    R.ms[2] = ms_since(t_call);
    if (rep) *rep = R;
    return WS_OK;
}


}  // namespace wsnark
