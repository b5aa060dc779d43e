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

// ---- host ----
struct CircuitRes {
    Context* owner = nullptr;
    uint32_t n_vars = 0, n_public = 0, domain = 0;
    CsrMatrix M[3];
    double load_ms = 0;
};
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

}  // namespace wsnark
