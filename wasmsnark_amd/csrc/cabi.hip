// cabi.hip -- the extern "C" surface declared in include/wsnark.h.
#include <limits.h>
#include <string.h>

#include "../../include/wsnark.h"
#include "internal.h"
#include "keybytes.h"

using namespace wsnark;

static_assert(sizeof(Fe) == 32, "field element must be 32 bytes");
static_assert(sizeof(Affine<Fq>) == 64 && sizeof(Affine<Fq2>) == 128, "affine layouts");
static_assert(sizeof(Jac<Fq>) == 96 && sizeof(Jac<Fq2>) == 192, "jacobian layouts");
static_assert(sizeof(XYZZ<Fq>) == 128 && sizeof(XYZZ<Fq2>) == 256, "xyzz layouts");
static_assert(sizeof(wsnark_pkey_delta_report_t) == 104 && sizeof(wsnark_pkey_delta_verdict_t) == 40, "the bindings read these by offset");
static_assert(sizeof(wsnark_pkey_setup_report_t) == 192, "the bindings read this by offset");
static_assert(sizeof(wsnark_powers_report_t) == 192, "the bindings read this by offset");
static_assert(sizeof(wsnark_pkey_circuit_verdict_t) == 56, "the bindings read this by offset");
static_assert(sizeof(wsnark_witness_report_t) == 80, "the bindings read this by offset");
static_assert(sizeof(wsnark_witness_verdict_t) == 48 && sizeof(wsnark_witness_batch_report_t) == 64, "the bindings read these by offset");
static_assert(sizeof(wsnark_prove_batch_report_t) == 64, "the bindings read this by offset");
static_assert(sizeof(wsnark_rows_report_t) == 152 && sizeof(wsnark_rows_matrix_t) == 24 && sizeof(wsnark_rows_t) == 88, "the bindings read these by offset");

// HIP's current device is per host thread (default 0) and every entry point may be called from any thread (the Node
// addon runs on the libuv pool): select the context's device first.
#define REQUIRE_CTX()                                                        \
    Context* C = ctx();                                                      \
    if (!C) { set_last_error("wsnark_init() has not been called"); return WSNARK_ERR_NOINIT; } \
    WS_HIP_CHECK(hipSetDevice(C->device))
// entry points that take a key handle run on the context (device) the key is resident on, whichever thread calls
#define REQUIRE_KEY_CTX(h)                                                   \
    if (!(h)) return WSNARK_ERR_ARG;                                         \
    Context* C = pkey_context(reinterpret_cast<const ProvingKey*>(h));       \
    if (!C) { set_last_error("wsnark_init() has not been called"); return WSNARK_ERR_NOINIT; } \
    CtxScope _key_scope(C)
static bool shard_ok(uint32_t rank, uint32_t world) { return world != 0 && rank < world; }

template <class JacT, class Fn>
static int msm_entry(Context* C, bool host, const void* scalars, const void* points, uint64_t n, uint32_t rank, uint32_t world,
                     void* out, Fn run) {
    if (!out || (n && (!scalars || !points))) return WSNARK_ERR_ARG;
    if (!shard_ok(rank, world)) return WSNARK_ERR_ARG;
    if (n > ((uint64_t)1 << 28)) return WSNARK_ERR_SIZE;
    (void)host;
    JacT r;
    LaneLock L = acquire_lane(C);
    int rc = run(*L, WindowShard{rank, world}, &r);
    if (rc) return rc;
    memcpy(out, &r, sizeof r);
    return WSNARK_OK;
}

// ---- a key's bytes as the entry points below receive them: an image in memory, separate sections, or a file ----
struct KeyInput {
    KeySections S;
    KeyFile file;      // the third case: the mapping S points into (S.release hands every range the callee has read back to the kernel)
    int open(const void* pkey, size_t len) { return pkey_parse((const uint8_t*)pkey, len, &S); }
    int open(const wsnark_key_sections_t* ks) {
        if (!ks || !ks->alfa1 || !ks->beta1 || !ks->delta1 || !ks->beta2 || !ks->delta2 || !ks->polsA ||
            !ks->polsB || !ks->pointsA || !ks->pointsB1 || !ks->pointsB2 || !ks->pointsH ||
            (!ks->pointsC && (uint64_t)ks->n_vars > (uint64_t)ks->n_public + 1))
            return WSNARK_ERR_ARG;
        S = KeySections{ks->n_vars, ks->n_public, ks->domain, (const uint8_t*)ks->alfa1, (const uint8_t*)ks->beta1,
                        (const uint8_t*)ks->delta1, (const uint8_t*)ks->beta2, (const uint8_t*)ks->delta2,
                        (const uint8_t*)ks->polsA, ks->polsA_len, (const uint8_t*)ks->polsB, ks->polsB_len,
                        (const uint8_t*)ks->pointsA, (const uint8_t*)ks->pointsB1, (const uint8_t*)ks->pointsB2,
                        (const uint8_t*)ks->pointsC, (const uint8_t*)ks->pointsH,
                        ks->pointsA_len, ks->pointsB1_len, ks->pointsB2_len, ks->pointsC_len, ks->pointsH_len};
        return WSNARK_OK;
    }
    int open(const char* path) { return keyfile_open(path, &file, &S); }
};
static int load_entry(const KeySections& S, KeyShard shard, wsnark_pkey_t** out_handle) {
    ProvingKey* K = nullptr;
    int rc = pkey_load_sections(S, &K, shard);      // (returns with every byte it needs copied: a mapped file may go)
    if (rc) return rc;
    *out_handle = reinterpret_cast<wsnark_pkey_t*>(K);
    return WSNARK_OK;
}

extern "C" {

int wsnark_init(int device) { return context_init(device); }
void wsnark_shutdown(void) { context_shutdown(); }
const char* wsnark_last_error(void) { return get_last_error().c_str(); }
const char* wsnark_device_info(void) { return device_info().c_str(); }

// ---- MSM ----
int wsnark_g1_msm_windows(const void* scalars, const void* points, uint64_t n, uint32_t rank, uint32_t world, void* out96) {
    REQUIRE_CTX();
    return msm_entry<Jac<Fq>>(C, true, scalars, points, n, rank, world, out96,
                              [&](Lane& L, WindowShard sh, Jac<Fq>* r) { return msm_g1_host(L, scalars, points, n, sh, r); });
}
int wsnark_g2_msm_windows(const void* scalars, const void* points, uint64_t n, uint32_t rank, uint32_t world, void* out192) {
    REQUIRE_CTX();
    return msm_entry<Jac<Fq2>>(C, true, scalars, points, n, rank, world, out192,
                               [&](Lane& L, WindowShard sh, Jac<Fq2>* r) { return msm_g2_host(L, scalars, points, n, sh, r); });
}
int wsnark_g1_msm_windows_dev(const void* d_scalars, const void* d_points, uint64_t n, uint32_t rank, uint32_t world,
                              void* out96_host, void* stream) {
    REQUIRE_CTX();
    return msm_entry<Jac<Fq>>(C, false, d_scalars, d_points, n, rank, world, out96_host, [&](Lane& L, WindowShard sh, Jac<Fq>* r) {
        return msm_g1_dev(L, (const Fe*)d_scalars, (const Affine<Fq>*)d_points, n, sh, r, (hipStream_t)stream);
    });
}
int wsnark_g2_msm_windows_dev(const void* d_scalars, const void* d_points, uint64_t n, uint32_t rank, uint32_t world,
                              void* out192_host, void* stream) {
    REQUIRE_CTX();
    return msm_entry<Jac<Fq2>>(C, false, d_scalars, d_points, n, rank, world, out192_host, [&](Lane& L, WindowShard sh, Jac<Fq2>* r) {
        return msm_g2_dev(L, (const Fe*)d_scalars, (const Affine<Fq2>*)d_points, n, sh, r, (hipStream_t)stream);
    });
}
int wsnark_g1_msm(const void* scalars, const void* points, uint64_t n, void* out96) {
    return wsnark_g1_msm_windows(scalars, points, n, 0, 1, out96);
}
int wsnark_g2_msm(const void* scalars, const void* points, uint64_t n, void* out192) {
    return wsnark_g2_msm_windows(scalars, points, n, 0, 1, out192);
}
int wsnark_g1_msm_dev(const void* d_scalars, const void* d_points, uint64_t n, void* out96_host, void* stream) {
    return wsnark_g1_msm_windows_dev(d_scalars, d_points, n, 0, 1, out96_host, stream);
}
int wsnark_g2_msm_dev(const void* d_scalars, const void* d_points, uint64_t n, void* out192_host, void* stream) {
    return wsnark_g2_msm_windows_dev(d_scalars, d_points, n, 0, 1, out192_host, stream);
}

int wsnark_g1_sum(const void* jac_points, uint64_t count, void* out96) {
    if (!out96 || (count && !jac_points)) return WSNARK_ERR_ARG;
    g1_sum_host((const uint8_t*)jac_points, count, (uint8_t*)out96);
    return WSNARK_OK;
}
int wsnark_g2_sum(const void* jac_points, uint64_t count, void* out192) {
    if (!out192 || (count && !jac_points)) return WSNARK_ERR_ARG;
    g2_sum_host((const uint8_t*)jac_points, count, (uint8_t*)out192);
    return WSNARK_OK;
}

// ---- resident bases: a point set kept on the device as fixed-base window tables (fixedbase.hip) ----
int wsnark_points_load(int group, const void* points, uint64_t n, wsnark_points_t** out_handle) {
    REQUIRE_CTX();
    if (group != 1 && group != 2) return WSNARK_ERR_ARG;
    ResidentPoints* H = nullptr;
    int rc = points_load(group - 1, points, n, &H);
    if (rc) return rc;
    *out_handle = reinterpret_cast<wsnark_points_t*>(H);
    return WSNARK_OK;
}
void wsnark_points_free(wsnark_points_t* h) {
    if (!h) return;
    CtxScope scope(points_context(reinterpret_cast<const ResidentPoints*>(h)));
    points_free(reinterpret_cast<ResidentPoints*>(h));
}
int wsnark_points_info(const wsnark_points_t* h, int* group, uint64_t* n, uint32_t* window_bits, uint32_t* rows, uint64_t* table_bytes) {
    if (!h) return WSNARK_ERR_ARG;
    int which = 0;
    points_info(reinterpret_cast<const ResidentPoints*>(h), &which, n, window_bits, rows, table_bytes);
    if (group) *group = which + 1;
    return WSNARK_OK;
}
int wsnark_points_msm(wsnark_points_t* h, const void* scalars, uint64_t n, void* out) {
    if (!h) return WSNARK_ERR_ARG;
    Context* C = points_context(reinterpret_cast<const ResidentPoints*>(h));
    if (!C) return WSNARK_ERR_NOINIT;
    CtxScope scope(C);
    return points_msm(reinterpret_cast<ResidentPoints*>(h), scalars, false, n, out, nullptr);
}
int wsnark_points_msm_dev(wsnark_points_t* h, const void* d_scalars, uint64_t n, void* out_host, void* stream) {
    if (!h) return WSNARK_ERR_ARG;
    Context* C = points_context(reinterpret_cast<const ResidentPoints*>(h));
    if (!C) return WSNARK_ERR_NOINIT;
    CtxScope scope(C);
    return points_msm(reinterpret_cast<ResidentPoints*>(h), d_scalars, true, n, out_host, (hipStream_t)stream);
}

// ---- NTT ----
int wsnark_fr_ntt_dev(void* d_buf, uint64_t n, int odd, int inverse, void* stream) {
    REQUIRE_CTX();
    LaneLock L = acquire_lane(C);
    return ntt_dev(*L, (Fe*)d_buf, n, odd, inverse, (hipStream_t)stream);
}
int wsnark_fr_ntt_batch_dev(void* d_buf, uint64_t n, uint64_t count, int inverse, void* stream) {
    REQUIRE_CTX();
    LaneLock L = acquire_lane(C);
    return ntt_dev(*L, (Fe*)d_buf, n, 0, inverse, (hipStream_t)stream, count);
}
int wsnark_fr_dist_scale_dev(void* d_buf, uint64_t stack, uint64_t rows, uint64_t cols, uint64_t row0, uint32_t log_n1, uint32_t log_n, int mode,
                             int inverse, void* stream) {
    REQUIRE_CTX();
    return dist_scale_dev((Fe*)d_buf, stack, rows, cols, row0, log_n1, log_n, mode, inverse, (hipStream_t)stream);
}
int wsnark_fr_ntt(void* buf, uint64_t n, int odd, int inverse) {
    REQUIRE_CTX();
    if (!buf) return WSNARK_ERR_ARG;
    if (n == 0 || (n & (n - 1)) || n > ((uint64_t)1 << 28)) return WSNARK_ERR_SIZE;
    DevBuf d;
    WS_HIP_CHECK(d.alloc(n * 32));
    LaneLock L = acquire_lane(C);
    WS_HIP_CHECK(hipMemcpyAsync(d.p, buf, n * 32, hipMemcpyHostToDevice, L->stream));
    int rc = ntt_dev(*L, d.as<Fe>(), n, odd, inverse, L->stream);
    if (rc) return rc;
    WS_HIP_CHECK(hipMemcpyAsync(buf, d.p, n * 32, hipMemcpyDeviceToHost, L->stream));
    WS_HIP_CHECK(hipStreamSynchronize(L->stream));
    return WSNARK_OK;
}
static int fr_map_host(const void* in, void* out, uint64_t n, int to_mont) {
    REQUIRE_CTX();
    if (n == 0) return WSNARK_OK;
    if (!in || !out) return WSNARK_ERR_ARG;
    DevBuf d;
    WS_HIP_CHECK(d.alloc(n * 32));
    int rc = upload_staged(d.p, in, n * 32, C->stream);
    if (!rc) rc = fr_map_dev(d.as<Fe>(), d.as<Fe>(), n, to_mont, C->stream);
    if (rc) return rc;
    WS_HIP_CHECK(hipMemcpyAsync(out, d.p, n * 32, hipMemcpyDeviceToHost, C->stream));
    WS_HIP_CHECK(hipStreamSynchronize(C->stream));
    return WSNARK_OK;
}
int wsnark_fr_to_montgomery(const void* in, void* out, uint64_t n) { return fr_map_host(in, out, n, 1); }
int wsnark_fr_from_montgomery(const void* in, void* out, uint64_t n) { return fr_map_host(in, out, n, 0); }

// ---- CALC_H ----
int wsnark_calc_h(const void* signals, const void* polsA, size_t lenA, const void* polsB, size_t lenB,
                  uint32_t n_signals, uint32_t domain, void* out_h) {
    REQUIRE_CTX();
    if (!signals || !polsA || !polsB || !out_h) return WSNARK_ERR_ARG;
    if (domain < 2 || (domain & (domain - 1)) || domain > (1u << 27)) return WSNARK_ERR_SIZE;
    CsrMatrix A, B;
    size_t used = 0;
    int rc = pols_to_csr((const uint8_t*)polsA, lenA, n_signals, domain, &A, &used, C->stream);
    if (rc) return rc;
    rc = pols_to_csr((const uint8_t*)polsB, lenB, n_signals, domain, &B, &used, C->stream);
    if (rc) return rc;
    DevBuf dsig, dh;
    WS_HIP_CHECK(dsig.alloc((size_t)n_signals * 32));
    WS_HIP_CHECK(dh.alloc((size_t)domain * 32));
    LaneLock L = acquire_lane(C);
    hipStream_t s = L->stream;
    WS_HIP_CHECK(hipMemcpyAsync(dsig.p, signals, (size_t)n_signals * 32, hipMemcpyHostToDevice, s));
    rc = calc_h_dev(*L, dsig.as<Fe>(), n_signals, A, B, domain, dh.as<Fe>(), s);
    if (rc) return rc;
    WS_HIP_CHECK(hipMemcpyAsync(out_h, dh.p, (size_t)domain * 32, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    return WSNARK_OK;
}

// ---- proving key / prove ----
int wsnark_pkey_load(const void* pkey, size_t len, wsnark_pkey_t** out_handle) {
    REQUIRE_CTX();
    if (!out_handle) return WSNARK_ERR_ARG;
    KeyInput in;
    int rc = in.open(pkey, len);
    return rc ? rc : load_entry(in.S, KeyShard{}, out_handle);
}
void wsnark_pkey_free(wsnark_pkey_t* h) {
    if (!h) return;
    CtxScope scope(pkey_context(reinterpret_cast<const ProvingKey*>(h)));
    pkey_free(reinterpret_cast<ProvingKey*>(h));
}
int wsnark_pkey_info(const wsnark_pkey_t* h, uint32_t* nv, uint32_t* np, uint32_t* dom) {
    if (!h) return WSNARK_ERR_ARG;
    pkey_info(reinterpret_cast<const ProvingKey*>(h), nv, np, dom);
    return WSNARK_OK;
}
int wsnark_pkey_table_info(const wsnark_pkey_t* h, uint32_t* cw, uint32_t* rw, uint32_t* ch, uint32_t* rh, uint64_t* bytes) {
    if (!h) return WSNARK_ERR_ARG;
    pkey_table_info(reinterpret_cast<const ProvingKey*>(h), cw, rw, ch, rh, bytes);
    return WSNARK_OK;
}
int wsnark_groth16_prove(wsnark_pkey_t* h, const void* witness, size_t witness_len, const void* r32, const void* s32,
                         void* out384) {
    REQUIRE_KEY_CTX(h);
    if (!h || !witness || !out384) return WSNARK_ERR_ARG;
    return groth16_prove_host_witness(reinterpret_cast<ProvingKey*>(h), (const uint8_t*)witness, witness_len,
                                      (const uint8_t*)r32, (const uint8_t*)s32, (uint8_t*)out384);
}
int wsnark_groth16_prove_dev(wsnark_pkey_t* h, const void* d_witness, size_t witness_len, const void* r32,
                             const void* s32, void* out384_host, void* stream) {
    REQUIRE_KEY_CTX(h);
    if (!h || !d_witness || !out384_host) return WSNARK_ERR_ARG;
    return groth16_prove_dev_witness(reinterpret_cast<ProvingKey*>(h), (const Fe*)d_witness, witness_len,
                                     (const uint8_t*)r32, (const uint8_t*)s32, (uint8_t*)out384_host, (hipStream_t)stream);
}

// many witnesses of one key (provebatch.hip).  Before wsnark_init no handle can exist: that is said first
int wsnark_groth16_prove_batch(wsnark_pkey_t* h, const void* witnesses, size_t witness_stride, uint64_t count, const void* r32s,
                               const void* s32s, void* out384s, void* out_rs64s, wsnark_prove_batch_report_t* rep) {
    if (!ctx()) { set_last_error("wsnark_init() has not been called"); return WSNARK_ERR_NOINIT; }
    REQUIRE_KEY_CTX(h);
    return groth16_prove_batch(reinterpret_cast<ProvingKey*>(h), witnesses, witness_stride, count, false, (const uint8_t*)r32s,
                               (const uint8_t*)s32s, (uint8_t*)out384s, (uint8_t*)out_rs64s, rep, nullptr);
}
int wsnark_groth16_prove_batch_dev(wsnark_pkey_t* h, const void* d_witnesses, size_t witness_stride, uint64_t count, const void* r32s,
                                   const void* s32s, void* out384s_host, void* out_rs64s_host, wsnark_prove_batch_report_t* rep, void* stream) {
    if (!ctx()) { set_last_error("wsnark_init() has not been called"); return WSNARK_ERR_NOINIT; }
    REQUIRE_KEY_CTX(h);
    return groth16_prove_batch(reinterpret_cast<ProvingKey*>(h), d_witnesses, witness_stride, count, true, (const uint8_t*)r32s,
                               (const uint8_t*)s32s, (uint8_t*)out384s_host, (uint8_t*)out_rs64s_host, rep, (hipStream_t)stream);
}

int wsnark_pkey_load_sections(const wsnark_key_sections_t* ks, wsnark_pkey_t** out_handle) {
    REQUIRE_CTX();
    KeyInput in;
    if (!out_handle || in.open(ks)) return WSNARK_ERR_ARG;
    return load_entry(in.S, KeyShard{}, out_handle);
}
int wsnark_pkey_load_shard(const wsnark_key_sections_t* ks, uint32_t rank, uint32_t world, uint32_t h_interleave_log,
                           wsnark_pkey_t** out_handle) {
    REQUIRE_CTX();
    KeyInput in;
    if (!shard_ok(rank, world) || !out_handle || in.open(ks)) return WSNARK_ERR_ARG;
    return load_entry(in.S, KeyShard{rank, world, h_interleave_log}, out_handle);
}
// a key FILE: proving_key.bin or the WSNARK64 container (keyfile.hip); rank / world / h_interleave_log as wsnark_pkey_load_shard
int wsnark_pkey_load_file(const char* path, uint32_t rank, uint32_t world, uint32_t h_interleave_log, wsnark_pkey_t** out_handle) {
    REQUIRE_CTX();
    if (!path || !out_handle || !shard_ok(rank, world)) return WSNARK_ERR_ARG;
    KeyInput in;
    int rc = in.open(path);
    return rc ? rc : load_entry(in.S, KeyShard{rank, world, h_interleave_log}, out_handle);
}
int wsnark_pkey_file_info(const char* path, uint32_t* n_vars, uint32_t* n_public, uint32_t* domain, uint64_t* file_bytes, int* format) {
    if (!path) return WSNARK_ERR_ARG;
    KeyInput in;
    int rc = in.open(path);
    if (rc) return rc;
    if (n_vars) *n_vars = in.S.n_vars;
    if (n_public) *n_public = in.S.n_public;
    if (domain) *domain = in.S.domain;
    if (file_bytes) *file_bytes = in.file.len;
    if (format) *format = in.file.format;
    return WSNARK_OK;
}
// ---- the audit of a key's bytes (pkeycheck.hip): what the three loaders take, no handle ----
int wsnark_pkey_check(const void* pkey, size_t len, uint32_t flags, const void* seed32, wsnark_pkey_report_t* out) {
    REQUIRE_CTX();
    if (!out) return WSNARK_ERR_ARG;
    KeyInput in;
    int rc = in.open(pkey, len);
    return rc ? rc : pkey_check_sections(in.S, flags, (const uint8_t*)seed32, out);
}
int wsnark_pkey_check_sections(const wsnark_key_sections_t* ks, uint32_t flags, const void* seed32, wsnark_pkey_report_t* out) {
    REQUIRE_CTX();
    KeyInput in;
    if (!out || in.open(ks)) return WSNARK_ERR_ARG;
    return pkey_check_sections(in.S, flags, (const uint8_t*)seed32, out);
}
int wsnark_pkey_check_file(const char* path, uint32_t flags, const void* seed32, wsnark_pkey_report_t* out) {
    REQUIRE_CTX();
    if (!path || !out) return WSNARK_ERR_ARG;
    KeyInput in;
    int rc = in.open(path);
    return rc ? rc : pkey_check_sections(in.S, flags, (const uint8_t*)seed32, out);
}
// ---- the phase-2 delta contribution and its check (pkeydelta.hip) ----
int wsnark_g1_scale_batch(const void* points, uint64_t n, const void* k32, void* out_affine) {
    REQUIRE_CTX();
    return g1_scale_batch(points, n, k32, out_affine);
}
int wsnark_g2_scale_batch(const void* points, uint64_t n, const void* k32, void* out_affine) {
    REQUIRE_CTX();
    return g2_scale_batch(points, n, k32, out_affine);
}
int wsnark_pkey_contribute(const void* pkey, size_t len, const void* d32, void* out_pkey, size_t out_cap, wsnark_pkey_delta_report_t* rep) {
    REQUIRE_CTX();
    if (!rep || !out_pkey) return WSNARK_ERR_ARG;
    KeyInput in;
    int rc = in.open(pkey, len);
    return rc ? rc : pkey_contribute_bytes(in.S, (const uint8_t*)pkey, len, (const uint8_t*)d32, (uint8_t*)out_pkey, out_cap, rep);
}
int wsnark_pkey_contribute_sections(const wsnark_key_sections_t* ks, const void* d32, void* out_pointsC, void* out_pointsH,
                                    void* out_delta1_64, void* out_delta2_128, wsnark_pkey_delta_report_t* rep) {
    REQUIRE_CTX();
    KeyInput in;
    if (!rep || in.open(ks)) return WSNARK_ERR_ARG;
    return pkey_contribute_sections(in.S, (const uint8_t*)d32, (uint8_t*)out_pointsC, (uint8_t*)out_pointsH, (uint8_t*)out_delta1_64,
                                    (uint8_t*)out_delta2_128, rep);
}
int wsnark_pkey_contribute_file(const char* in_path, const char* out_path, const void* d32, wsnark_pkey_delta_report_t* rep) {
    REQUIRE_CTX();
    if (!in_path || !out_path || !rep) return WSNARK_ERR_ARG;
    KeyInput in;
    int rc = in.open(in_path);
    return rc ? rc : pkey_contribute_file(in.S, in.file, in_path, out_path, (const uint8_t*)d32, rep);
}
// ---- the first key of a ceremony (pkeysetup.hip) ----
int wsnark_g1_ntt(const void* points, uint64_t n, int inverse, void* out) {
    REQUIRE_CTX();
    return g1_group_ntt(points, n, inverse, out);
}
int wsnark_g2_ntt(const void* points, uint64_t n, int inverse, void* out) {
    REQUIRE_CTX();
    return g2_group_ntt(points, n, inverse, out);
}
int wsnark_pkey_setup(const wsnark_powers_t* powers, const wsnark_circuit_t* circuit, void* out_pointsA, void* out_pointsB1, void* out_pointsB2,
                      void* out_pointsC, void* out_pointsH, void* out_alfa1_64, void* out_beta1_64, void* out_delta1_64, void* out_beta2_128,
                      void* out_delta2_128, void* out_ic, wsnark_pkey_setup_report_t* rep) {
    REQUIRE_CTX();
    void* const out[11] = {out_pointsA, out_pointsB1, out_pointsB2, out_pointsC, out_pointsH, out_alfa1_64, out_beta1_64, out_delta1_64,
                           out_beta2_128, out_delta2_128, out_ic};
    return pkey_setup_sections(powers, circuit, out, rep);
}
int wsnark_pkey_setup_pkey(const wsnark_powers_t* powers, const wsnark_circuit_t* circuit, void* out_pkey, size_t out_cap, size_t* out_len,
                           void* out_ic, wsnark_pkey_setup_report_t* rep) {
    REQUIRE_CTX();
    return pkey_setup_bytes(powers, circuit, (uint8_t*)out_pkey, out_cap, out_len, (uint8_t*)out_ic, rep);
}
int wsnark_pkey_setup_size(const wsnark_circuit_t* circuit, size_t* out_len) { return pkey_setup_size(circuit, out_len); }
// ---- snarkjs' .zkey in and out, the H basis change (zkey.hip) ----
static_assert(sizeof(wsnark_zkey_info_t) == 56 && sizeof(wsnark_zkey_report_t) == 136, "the bindings read these by offset");
int wsnark_g1_h_basis(const void* points, uint64_t n, int to_lagrange, void* out) {
    REQUIRE_CTX();
    return g1_h_basis(points, n, to_lagrange, out);
}
int wsnark_zkey_info(const void* zkey, size_t len, wsnark_zkey_info_t* out) { return zkey_info((const uint8_t*)zkey, len, out); }
int wsnark_zkey_import(const void* zkey, size_t len, void* out_pkey, size_t cap, size_t* out_len, void* out_vk, size_t vk_cap,
                       wsnark_zkey_report_t* rep) {
    REQUIRE_CTX();
    if (!out_pkey) return WSNARK_ERR_ARG;
    return zkey_import((const uint8_t*)zkey, len, nullptr, nullptr, (uint8_t*)out_pkey, cap, out_len, (uint8_t*)out_vk, vk_cap, rep);
}
int wsnark_zkey_import_sections(const void* zkey, size_t len, void* const out[12], const uint64_t caps[12], void* out_vk, size_t vk_cap,
                                wsnark_zkey_report_t* rep) {
    REQUIRE_CTX();
    if (!out || !caps) return WSNARK_ERR_ARG;
    return zkey_import((const uint8_t*)zkey, len, out, caps, nullptr, 0, nullptr, (uint8_t*)out_vk, vk_cap, rep);
}
// ... and straight into a resident key: the handle is wsnark_pkey_load's.  Nothing is written before the load has succeeded.
int wsnark_pkey_load_zkey(const void* zkey, size_t len, wsnark_pkey_t** out_handle, void* out_vk, size_t vk_cap, wsnark_zkey_report_t* rep) {
    REQUIRE_CTX();
    ProvingKey* K = nullptr;
    int rc = zkey_load((const uint8_t*)zkey, len, nullptr, out_handle ? &K : nullptr, (uint8_t*)out_vk, vk_cap, rep);
    if (rc) return rc;
    *out_handle = reinterpret_cast<wsnark_pkey_t*>(K);
    return WSNARK_OK;
}
int wsnark_pkey_load_zkey_file(const char* path, wsnark_pkey_t** out_handle, void* out_vk, size_t vk_cap, wsnark_zkey_report_t* rep) {
    REQUIRE_CTX();
    ProvingKey* K = nullptr;
    int rc = zkey_load_file(path, out_handle ? &K : nullptr, (uint8_t*)out_vk, vk_cap, rep);
    if (rc) return rc;
    *out_handle = reinterpret_cast<wsnark_pkey_t*>(K);
    return WSNARK_OK;
}
int wsnark_zkey_vk_len(const void* zkey, size_t len, size_t* out_len) { return zkey_vk_len((const uint8_t*)zkey, len, out_len); }
int wsnark_zkey_vk_len_file(const char* path, size_t* out_len) { return zkey_vk_len_file(path, out_len); }
int wsnark_zkey_export(const void* pkey, size_t len, const void* vk, size_t vk_len, uint64_t n_inputs, void* out_zkey, size_t cap,
                       size_t* out_len, wsnark_zkey_report_t* rep) {
    REQUIRE_CTX();
    if (!pkey || !vk) return WSNARK_ERR_ARG;
    KeyInput in;
    int rc = in.open(pkey, len);
    return rc ? rc : zkey_export(in.S, (const uint8_t*)vk, vk_len, n_inputs, (uint8_t*)out_zkey, cap, out_len, rep);
}
int wsnark_zkey_export_sections(const wsnark_key_sections_t* key, const void* vk, size_t vk_len, uint64_t n_inputs, void* out_zkey,
                                size_t cap, size_t* out_len, wsnark_zkey_report_t* rep) {
    REQUIRE_CTX();
    KeyInput in;
    if (!vk || in.open(key)) return WSNARK_ERR_ARG;
    return zkey_export(in.S, (const uint8_t*)vk, vk_len, n_inputs, (uint8_t*)out_zkey, cap, out_len, rep);
}
int wsnark_zkey_export_size(uint32_t n_vars, uint32_t n_public, uint32_t domain, uint64_t nnzA, uint64_t nnzB, size_t* out_len) {
    return zkey_export_size(n_vars, n_public, domain, nnzA, nnzB, out_len);
}
// ---- powers of tau: a scalar per point, the contribution, the audit (pwtau.hip) ----
int wsnark_g1_mul_batch(const void* points, const void* scalars, uint64_t n, void* out_affine) {
    REQUIRE_CTX();
    return g1_mul_batch(points, scalars, n, out_affine);
}
int wsnark_g2_mul_batch(const void* points, const void* scalars, uint64_t n, void* out_affine) {
    REQUIRE_CTX();
    return g2_mul_batch(points, scalars, n, out_affine);
}
int wsnark_powers_contribute(const wsnark_powers_t* in, const void* tau32, const void* alpha32, const void* beta32, void* out_tau_g1,
                             void* out_tau_g2, void* out_alpha_tau_g1, void* out_beta_tau_g1, void* out_beta_g2_128, wsnark_powers_report_t* rep) {
    REQUIRE_CTX();
    uint8_t* const out[5] = {(uint8_t*)out_tau_g1, (uint8_t*)out_tau_g2, (uint8_t*)out_alpha_tau_g1, (uint8_t*)out_beta_tau_g1, (uint8_t*)out_beta_g2_128};
    return powers_contribute(in, (const uint8_t*)tau32, (const uint8_t*)alpha32, (const uint8_t*)beta32, out, rep);
}
int wsnark_powers_check(const wsnark_powers_t* powers, uint32_t flags, const void* seed32, wsnark_powers_report_t* rep) {
    REQUIRE_CTX();
    return powers_check(powers, flags, (const uint8_t*)seed32, rep);
}
// ---- KZG commitments on powers of tau (kzg.hip).  Before wsnark_init no handle can exist: that is said first ----
#define REQUIRE_SRS_CTX(h)                                                   \
    if (!ctx()) { set_last_error("wsnark_init() has not been called"); return WSNARK_ERR_NOINIT; } \
    if (!(h)) return WSNARK_ERR_ARG;                                         \
    CtxScope _srs_scope(kzg_context(reinterpret_cast<const KzgSrs*>(h)))
int wsnark_kzg_srs_load(const void* tau_g1, uint64_t n, wsnark_kzg_srs_t** out_handle) {
    REQUIRE_CTX();
    KzgSrs* S = nullptr;
    int rc = kzg_srs_load(tau_g1, n, out_handle ? &S : nullptr);
    if (rc) return rc;
    *out_handle = reinterpret_cast<wsnark_kzg_srs_t*>(S);
    return WSNARK_OK;
}
void wsnark_kzg_srs_free(wsnark_kzg_srs_t* h) {
    if (!h) return;
    CtxScope scope(kzg_context(reinterpret_cast<const KzgSrs*>(h)));
    kzg_srs_free(reinterpret_cast<KzgSrs*>(h));
}
int wsnark_kzg_srs_info(const wsnark_kzg_srs_t* h, uint64_t* n, uint64_t* bytes) {
    if (!h) return WSNARK_ERR_ARG;
    kzg_srs_info(reinterpret_cast<const KzgSrs*>(h), n, bytes);
    return WSNARK_OK;
}
int wsnark_fr_poly_eval(const void* polys, uint64_t len, uint64_t count, const void* z32, void* out_y) {
    REQUIRE_CTX();
    return fr_poly_eval(polys, len, count, (const uint8_t*)z32, out_y);
}
int wsnark_fr_poly_divide(const void* poly, uint64_t len, const void* z32, void* out_q, void* out_y32) {
    REQUIRE_CTX();
    return fr_poly_divide(poly, len, (const uint8_t*)z32, out_q, out_y32, false, nullptr);
}
int wsnark_fr_poly_divide_dev(const void* d_poly, uint64_t len, const void* z32, void* d_q, void* out_y32_host, void* stream) {
    REQUIRE_CTX();
    return fr_poly_divide(d_poly, len, (const uint8_t*)z32, d_q, out_y32_host, true, (hipStream_t)stream);
}
int wsnark_kzg_commit(wsnark_kzg_srs_t* h, const void* polys, uint64_t len, uint64_t count, int form, void* out_commitments) {
    REQUIRE_SRS_CTX(h);
    return kzg_commit(reinterpret_cast<KzgSrs*>(h), polys, len, count, form, false, out_commitments, nullptr);
}
int wsnark_kzg_commit_dev(wsnark_kzg_srs_t* h, const void* d_polys, uint64_t len, uint64_t count, int form, void* out_commitments_host, void* stream) {
    REQUIRE_SRS_CTX(h);
    return kzg_commit(reinterpret_cast<KzgSrs*>(h), d_polys, len, count, form, true, out_commitments_host, (hipStream_t)stream);
}
int wsnark_kzg_open(wsnark_kzg_srs_t* h, const void* polys, uint64_t len, uint64_t count, const void* z32, const void* gamma32, void* out_y,
                    void* out_proof64) {
    REQUIRE_SRS_CTX(h);
    return kzg_open(reinterpret_cast<KzgSrs*>(h), polys, len, count, (const uint8_t*)z32, (const uint8_t*)gamma32, false, out_y, out_proof64, nullptr);
}
int wsnark_kzg_open_dev(wsnark_kzg_srs_t* h, const void* d_polys, uint64_t len, uint64_t count, const void* z32, const void* gamma32,
                        void* out_y_host, void* out_proof64_host, void* stream) {
    REQUIRE_SRS_CTX(h);
    return kzg_open(reinterpret_cast<KzgSrs*>(h), d_polys, len, count, (const uint8_t*)z32, (const uint8_t*)gamma32, true, out_y_host,
                    out_proof64_host, (hipStream_t)stream);
}
int wsnark_kzg_verify(const void* g1_64, const void* g2_tau_g2_256, const void* commitments, uint64_t count, const void* z32, const void* gamma32,
                      const void* ys, const void* proof64, int* valid) {
    return kzg_verify((const uint8_t*)g1_64, (const uint8_t*)g2_tau_g2_256, (const uint8_t*)commitments, count, (const uint8_t*)z32,
                      (const uint8_t*)gamma32, (const uint8_t*)ys, (const uint8_t*)proof64, valid);
}
int wsnark_pkey_delta_verify(const void* old_pkey, size_t old_len, const void* new_pkey, size_t new_len, const void* seed32,
                             wsnark_pkey_delta_verdict_t* out) {
    REQUIRE_CTX();
    if (!out) return WSNARK_ERR_ARG;
    KeyInput o, n;
    int rc = o.open(old_pkey, old_len);
    if (!rc) rc = n.open(new_pkey, new_len);
    return rc ? rc : pkey_delta_verify_sections(o.S, n.S, (const uint8_t*)seed32, out);
}
int wsnark_pkey_delta_verify_sections(const wsnark_key_sections_t* old_key, const wsnark_key_sections_t* new_key, const void* seed32,
                                      wsnark_pkey_delta_verdict_t* out) {
    REQUIRE_CTX();
    KeyInput o, n;
    if (!out || o.open(old_key) || n.open(new_key)) return WSNARK_ERR_ARG;
    return pkey_delta_verify_sections(o.S, n.S, (const uint8_t*)seed32, out);
}
int wsnark_pkey_delta_verify_file(const char* old_path, const char* new_path, const void* seed32, wsnark_pkey_delta_verdict_t* out) {
    REQUIRE_CTX();
    if (!old_path || !new_path || !out) return WSNARK_ERR_ARG;
    KeyInput o, n;
    int rc = o.open(old_path);
    if (!rc) rc = n.open(new_path);
    return rc ? rc : pkey_delta_verify_sections(o.S, n.S, (const uint8_t*)seed32, out);
}
// ---- a key against its circuit and its powers of tau (pkeycircuit.hip) ----
int wsnark_pkey_circuit_check(const void* pkey, size_t len, const wsnark_powers_t* powers, const wsnark_circuit_t* circuit, const void* vk,
                              size_t vk_len, uint64_t n_inputs, const void* seed32, wsnark_pkey_circuit_verdict_t* out) {
    REQUIRE_CTX();
    if (!out) return WSNARK_ERR_ARG;
    KeyInput in;
    int rc = in.open(pkey, len);
    return rc ? rc : pkey_circuit_check_sections(in.S, powers, circuit, (const uint8_t*)vk, vk_len, n_inputs, (const uint8_t*)seed32, out);
}
int wsnark_pkey_circuit_check_sections(const wsnark_key_sections_t* key, const wsnark_powers_t* powers, const wsnark_circuit_t* circuit,
                                       const void* vk, size_t vk_len, uint64_t n_inputs, const void* seed32,
                                       wsnark_pkey_circuit_verdict_t* out) {
    REQUIRE_CTX();
    KeyInput in;
    if (!out || in.open(key)) return WSNARK_ERR_ARG;
    return pkey_circuit_check_sections(in.S, powers, circuit, (const uint8_t*)vk, vk_len, n_inputs, (const uint8_t*)seed32, out);
}
int wsnark_pkey_circuit_check_file(const char* path, const wsnark_powers_t* powers, const wsnark_circuit_t* circuit, const void* vk,
                                   size_t vk_len, uint64_t n_inputs, const void* seed32, wsnark_pkey_circuit_verdict_t* out) {
    REQUIRE_CTX();
    if (!path || !out) return WSNARK_ERR_ARG;
    KeyInput in;
    int rc = in.open(path);
    return rc ? rc : pkey_circuit_check_sections(in.S, powers, circuit, (const uint8_t*)vk, vk_len, n_inputs, (const uint8_t*)seed32, out);
}
int wsnark_circuit_row_sums(const wsnark_circuit_t* circuit, const void* weights, void* out_public, void* out_private) {
    REQUIRE_CTX();
    return circuit_row_sums(circuit, weights, out_public, out_private);
}
// ---- a witness against its circuit (witcheck.hip) ----
int wsnark_circuit_load(const wsnark_circuit_t* circuit, wsnark_circuit_res_t** out_handle) {
    REQUIRE_CTX();
    if (!out_handle) return WSNARK_ERR_ARG;
    CircuitRes* H = nullptr;
    int rc = circuit_load(circuit, &H);
    if (rc) return rc;
    *out_handle = reinterpret_cast<wsnark_circuit_res_t*>(H);
    return WSNARK_OK;
}
void wsnark_circuit_free(wsnark_circuit_res_t* h) {
    if (!h) return;
    CtxScope scope(circuit_context(reinterpret_cast<const CircuitRes*>(h)));
    circuit_free(reinterpret_cast<CircuitRes*>(h));
}
int wsnark_circuit_info(const wsnark_circuit_res_t* h, uint32_t* n_vars, uint32_t* n_public, uint32_t* domain, uint64_t nnz[3], uint64_t* bytes) {
    if (!h) return WSNARK_ERR_ARG;
    circuit_info(reinterpret_cast<const CircuitRes*>(h), n_vars, n_public, domain, nnz, bytes);
    return WSNARK_OK;
}
int wsnark_witness_check(const wsnark_circuit_t* circuit, const void* witness, size_t witness_len, uint64_t* bad_rows, void* bad_values,
                         uint64_t cap, wsnark_witness_report_t* rep) {
    REQUIRE_CTX();
    return witness_check(circuit, witness, witness_len, bad_rows, bad_values, cap, rep);
}
int wsnark_circuit_witness_check(wsnark_circuit_res_t* h, const void* witness, size_t witness_len, uint64_t* bad_rows, void* bad_values,
                                 uint64_t cap, wsnark_witness_report_t* rep) {
    REQUIRE_CTX();      // (before the handle is looked at: WSNARK_ERR_NOINIT whatever the arguments)
    if (!h) return WSNARK_ERR_ARG;
    CtxScope scope(circuit_context(reinterpret_cast<const CircuitRes*>(h)));
    return circuit_witness_check(reinterpret_cast<CircuitRes*>(h), witness, witness_len, false, bad_rows, bad_values, cap, rep, nullptr);
}
int wsnark_circuit_witness_check_dev(wsnark_circuit_res_t* h, const void* d_witness, size_t witness_len, uint64_t* bad_rows_host,
                                     void* bad_values_host, uint64_t cap, wsnark_witness_report_t* rep, void* stream) {
    REQUIRE_CTX();
    if (!h) return WSNARK_ERR_ARG;
    CtxScope scope(circuit_context(reinterpret_cast<const CircuitRes*>(h)));
    return circuit_witness_check(reinterpret_cast<CircuitRes*>(h), d_witness, witness_len, true, bad_rows_host, bad_values_host, cap, rep,
                                 (hipStream_t)stream);
}
// many witnesses of one resident circuit (witcheck.hip)
int wsnark_circuit_witness_check_batch(wsnark_circuit_res_t* h, const void* witnesses, size_t witness_stride, uint64_t count,
                                       wsnark_witness_verdict_t* verdicts, uint64_t* bad_rows, void* bad_values, uint64_t cap,
                                       wsnark_witness_batch_report_t* rep) {
    REQUIRE_CTX();
    if (!h) return WSNARK_ERR_ARG;
    CtxScope scope(circuit_context(reinterpret_cast<const CircuitRes*>(h)));
    return circuit_witness_check_batch(reinterpret_cast<CircuitRes*>(h), witnesses, witness_stride, count, false, verdicts, bad_rows, bad_values,
                                       cap, rep, nullptr);
}
int wsnark_circuit_witness_check_batch_dev(wsnark_circuit_res_t* h, const void* d_witnesses, size_t witness_stride, uint64_t count,
                                           wsnark_witness_verdict_t* verdicts_host, uint64_t* bad_rows_host, void* bad_values_host, uint64_t cap,
                                           wsnark_witness_batch_report_t* rep, void* stream) {
    REQUIRE_CTX();
    if (!h) return WSNARK_ERR_ARG;
    CtxScope scope(circuit_context(reinterpret_cast<const CircuitRes*>(h)));
    return circuit_witness_check_batch(reinterpret_cast<CircuitRes*>(h), d_witnesses, witness_stride, count, true, verdicts_host, bad_rows_host,
                                       bad_values_host, cap, rep, (hipStream_t)stream);
}
// ---- a circuit in row form (circuitrows.hip) ----
int wsnark_circuit_from_rows_size(const wsnark_rows_t* rows, uint32_t flags, uint32_t* domain, uint64_t lens[3]) {
    return circuit_from_rows_size(rows, flags, domain, lens);
}
int wsnark_circuit_from_rows(const wsnark_rows_t* rows, uint32_t flags, void* out_polsA, uint64_t capA, void* out_polsB, uint64_t capB,
                             void* out_polsC, uint64_t capC, uint32_t* domain, wsnark_rows_report_t* rep) {
    REQUIRE_CTX();
    void* const out[3] = {out_polsA, out_polsB, out_polsC};
    const uint64_t cap[3] = {capA, capB, capC};
    return circuit_from_rows(rows, flags, out, cap, domain, rep);
}
int wsnark_circuit_load_rows(const wsnark_rows_t* rows, uint32_t flags, wsnark_circuit_res_t** out_handle) {
    REQUIRE_CTX();
    if (!out_handle) return WSNARK_ERR_ARG;
    CircuitRes* H = nullptr;
    int rc = circuit_load_rows(rows, flags, &H);
    if (rc) return rc;
    *out_handle = reinterpret_cast<wsnark_circuit_res_t*>(H);
    return WSNARK_OK;
}
int wsnark_pkey_shard_info(const wsnark_pkey_t* h, uint32_t* rank, uint32_t* world, uint64_t* first_signal, uint64_t* n_signals,
                           uint64_t* n_hexps, uint32_t* h_interleave_log) {
    if (!h) return WSNARK_ERR_ARG;
    pkey_shard_info(reinterpret_cast<const ProvingKey*>(h), rank, world, first_signal, n_signals, n_hexps, h_interleave_log);
    return WSNARK_OK;
}
int wsnark_pkey_load_stats(const wsnark_pkey_t* h, double* ms5) {
    if (!h || !ms5) return WSNARK_ERR_ARG;
    pkey_load_stats(reinterpret_cast<const ProvingKey*>(h), ms5);
    return WSNARK_OK;
}
int wsnark_pkey_wait_tables(wsnark_pkey_t* h) {
    REQUIRE_KEY_CTX(h);
    if (!h) return WSNARK_ERR_ARG;
    return pkey_wait_tables(reinterpret_cast<ProvingKey*>(h));
}
int wsnark_pkey_h_msm_dev(wsnark_pkey_t* h, const void* d_h_slice, uint64_t n, void* out96_host, void* stream) {
    REQUIRE_KEY_CTX(h);
    if (!h || !out96_host || (n && !d_h_slice)) return WSNARK_ERR_ARG;
    return pkey_h_msm_dev(reinterpret_cast<ProvingKey*>(h), (const Fe*)d_h_slice, n, (uint8_t*)out96_host, (hipStream_t)stream);
}
int wsnark_groth16_prove_partial(wsnark_pkey_t* h, const void* witness, size_t witness_len, uint32_t rank, uint32_t world,
                                 uint32_t flags, void* out576) {
    REQUIRE_KEY_CTX(h);
    if (!h || !witness || !out576 || !shard_ok(rank, world) || (flags & ~(uint32_t)WSNARK_PARTIAL_SKIP_H)) return WSNARK_ERR_ARG;
    return groth16_prove_partial(reinterpret_cast<ProvingKey*>(h), (const uint8_t*)witness, witness_len, WindowShard{rank, world},
                                 (uint8_t*)out576, (flags & WSNARK_PARTIAL_SKIP_H) != 0);
}
int wsnark_groth16_prove_partial_dev(wsnark_pkey_t* h, const void* d_witness, size_t witness_len, uint32_t rank, uint32_t world,
                                     uint32_t flags, void* out576_host, void* stream) {
    REQUIRE_KEY_CTX(h);
    if (!h || !d_witness || !out576_host || !shard_ok(rank, world) || (flags & ~(uint32_t)WSNARK_PARTIAL_SKIP_H)) return WSNARK_ERR_ARG;
    return groth16_prove_partial_dev(reinterpret_cast<ProvingKey*>(h), (const Fe*)d_witness, witness_len, WindowShard{rank, world},
                                     (uint8_t*)out576_host, (hipStream_t)stream, (flags & WSNARK_PARTIAL_SKIP_H) != 0);
}
int wsnark_groth16_prove_dist(wsnark_pkey_t* h, const void* d_witness, size_t witness_len, const wsnark_comm_t* comm, const void* r32,
                              const void* s32, void* out384_host, void* stream) {
    REQUIRE_KEY_CTX(h);
    if (!h || !d_witness || !comm || !out384_host) return WSNARK_ERR_ARG;
    DistComm cm;
    cm.rank = comm->rank; cm.world = comm->world;
    cm.d_send = (Fe*)comm->d_send; cm.d_recv = (Fe*)comm->d_recv; cm.buf_bytes = comm->buf_bytes;
    cm.all_to_all = comm->all_to_all; cm.all_gather = comm->all_gather; cm.user = comm->user;
    return groth16_prove_dist(reinterpret_cast<ProvingKey*>(h), (const Fe*)d_witness, witness_len, cm, (const uint8_t*)r32, (const uint8_t*)s32,
                              (uint8_t*)out384_host, (hipStream_t)stream);
}
int wsnark_pkey_eval_ab_dev(wsnark_pkey_t* h, const void* d_witness, size_t witness_len, void* d_a_out, void* d_b_out, void* stream) {
    REQUIRE_KEY_CTX(h);
    if (!h || !d_witness || !d_a_out || !d_b_out) return WSNARK_ERR_ARG;
    return pkey_eval_ab_dev(reinterpret_cast<ProvingKey*>(h), (const Fe*)d_witness, witness_len, (Fe*)d_a_out, (Fe*)d_b_out, (hipStream_t)stream);
}
int wsnark_fr_mul_dev(const void* d_a, const void* d_b, void* d_out, uint64_t n, void* stream) {
    REQUIRE_CTX();
    return fr_mul_dev((const Fe*)d_a, (const Fe*)d_b, (Fe*)d_out, n, (hipStream_t)stream);
}
int wsnark_fr_dist_combine_dev(const void* d_e, const void* d_o, void* d_h_out, uint64_t rows, uint64_t cols, uint64_t row0, uint32_t log_n1,
                               uint32_t log_n, void* stream) {
    REQUIRE_CTX();
    return dist_combine_dev((const Fe*)d_e, (const Fe*)d_o, (Fe*)d_h_out, rows, cols, row0, log_n1, log_n, (hipStream_t)stream);
}
int wsnark_groth16_verify(const void* vk, size_t vk_len, const void* inputs, uint64_t n_inputs, const void* proof384, int* valid) {
    if (!vk || !proof384 || !valid || (n_inputs && !inputs)) return WSNARK_ERR_ARG;
    return groth16_verify((const uint8_t*)vk, vk_len, (const uint8_t*)inputs, n_inputs, (const uint8_t*)proof384, valid);
}
// batch verification on the device (pairing.hip); the key stays on the host in both variants
int wsnark_groth16_verify_batch(const void* vk, size_t vk_len, const void* inputs, uint64_t n_inputs, const void* proofs384, uint64_t count,
                                uint8_t* status) {
    REQUIRE_CTX();
    return groth16_verify_batch((const uint8_t*)vk, vk_len, inputs, n_inputs, proofs384, count, status, false, nullptr);
}
int wsnark_groth16_verify_batch_dev(const void* vk, size_t vk_len, const void* d_inputs, uint64_t n_inputs, const void* d_proofs384,
                                    uint64_t count, uint8_t* status_host, void* stream) {
    REQUIRE_CTX();
    return groth16_verify_batch((const uint8_t*)vk, vk_len, d_inputs, n_inputs, d_proofs384, count, status_host, true, (hipStream_t)stream);
}
// compressed points and proofs (pointcodec.hip)
int wsnark_g1_compress(const void* points, uint64_t n, int encoding, void* out, uint8_t* status, uint64_t* n_bad) {
    REQUIRE_CTX();
    return points_codec(1, true, points, n, encoding, 0, out, status, n_bad);
}
int wsnark_g2_compress(const void* points, uint64_t n, int encoding, void* out, uint8_t* status, uint64_t* n_bad) {
    REQUIRE_CTX();
    return points_codec(2, true, points, n, encoding, 0, out, status, n_bad);
}
int wsnark_g1_decompress(const void* in, uint64_t n, int encoding, uint32_t flags, void* out_points, uint8_t* status, uint64_t* n_bad) {
    REQUIRE_CTX();
    return points_codec(1, false, in, n, encoding, flags, out_points, status, n_bad);
}
int wsnark_g2_decompress(const void* in, uint64_t n, int encoding, uint32_t flags, void* out_points, uint8_t* status, uint64_t* n_bad) {
    REQUIRE_CTX();
    return points_codec(2, false, in, n, encoding, flags, out_points, status, n_bad);
}
int wsnark_proof_compress(const void* proofs384, uint64_t count, int encoding, void* out128, uint8_t* status) {
    REQUIRE_CTX();
    return proofs_codec(true, proofs384, count, encoding, out128, status);
}
int wsnark_proof_decompress(const void* proofs128, uint64_t count, int encoding, void* out384, uint8_t* status) {
    REQUIRE_CTX();
    return proofs_codec(false, proofs128, count, encoding, out384, status);
}
int wsnark_groth16_verify_batch_compressed(const void* vk, size_t vk_len, const void* inputs, uint64_t n_inputs, const void* proofs128,
                                           uint64_t count, int encoding, uint8_t* status) {
    REQUIRE_CTX();
    return groth16_verify_batch_compressed((const uint8_t*)vk, vk_len, inputs, n_inputs, proofs128, count, encoding, status, false, nullptr);
}
int wsnark_groth16_verify_batch_compressed_dev(const void* vk, size_t vk_len, const void* d_inputs, uint64_t n_inputs, const void* d_proofs128,
                                               uint64_t count, int encoding, uint8_t* status_host, void* stream) {
    REQUIRE_CTX();
    return groth16_verify_batch_compressed((const uint8_t*)vk, vk_len, d_inputs, n_inputs, d_proofs128, count, encoding, status_host, true,
                                           (hipStream_t)stream);
}
int wsnark_last_blinding(void* r32, void* s32) {
    return last_blinding((uint8_t*)r32, (uint8_t*)s32) ? WSNARK_OK : WSNARK_ERR_ARG;
}
int wsnark_groth16_prove_finish(wsnark_pkey_t* h, const void* partials, uint64_t n_ranks, const void* r32,
                                const void* s32, void* out384) {
    if (!h || !out384 || (n_ranks && !partials)) return WSNARK_ERR_ARG;
    return groth16_prove_finish(reinterpret_cast<ProvingKey*>(h), (const uint8_t*)partials, n_ranks,
                                (const uint8_t*)r32, (const uint8_t*)s32, (uint8_t*)out384);
}

// ---- synthetic-input helpers (no reference counterpart) ----
int wsnark_g1_mul_base_batch(const void* base64, const void* scalars, uint64_t n, void* out_affine) {
    REQUIRE_CTX();
    return g1_mul_base_batch(base64, scalars, n, out_affine);
}
int wsnark_g2_mul_base_batch(const void* base128, const void* scalars, uint64_t n, void* out_affine) {
    REQUIRE_CTX();
    return g2_mul_base_batch(base128, scalars, n, out_affine);
}

// ---- device self-test hooks (tests only; selftest.hip) ----
int wsnark_selftest_field(int which, int impl, int op, const void* a, const void* b, void* out, uint64_t n) {
    REQUIRE_CTX();
    if (n && (!a || !b || !out)) return WSNARK_ERR_ARG;
    return selftest_field(which, impl, op, (const uint8_t*)a, (const uint8_t*)b, (uint8_t*)out, n);
}
int wsnark_selftest_curve(int g, int impl, int op, const void* p, const void* q, void* out, uint64_t n) {
    REQUIRE_CTX();
    if (n && (!p || !q || !out)) return WSNARK_ERR_ARG;
    return selftest_curve(g, impl, op, (const uint8_t*)p, (const uint8_t*)q, (uint8_t*)out, n);
}
int wsnark_selftest_fp12(int impl, int op, const void* a, const void* b, void* out, uint64_t n) {
    REQUIRE_CTX();
    if (n && (!a || !b || !out)) return WSNARK_ERR_ARG;
    return selftest_fp12(impl, op, (const uint8_t*)a, (const uint8_t*)b, (uint8_t*)out, n);
}

int wsnark_selftest_msm_plan(const void* scalars, uint64_t n, uint32_t table_c, uint32_t w_off, uint32_t w_stride, const void* mask,
                             uint32_t* info, uint32_t* bstart, uint32_t* bend, uint64_t cap_buckets, uint32_t* vals, uint64_t cap_vals,
                             uint32_t* tasks, uint64_t cap_tasks, uint32_t* multi, uint64_t cap_multi, uint32_t* hot, uint64_t cap_hot) {
    static_assert(WSNARK_MSM_PLAN_INFO_WORDS == kMsmPlanInfoWords, "info words of the plan hook");
    REQUIRE_CTX();
    if (!info || (n && !scalars) || !shard_ok(w_off, w_stride)) return WSNARK_ERR_ARG;
    if (n > ((uint64_t)1 << 28)) return WSNARK_ERR_SIZE;
    if (table_c && (table_c < 4 || table_c > 22)) return WSNARK_ERR_ARG;
    LaneLock L = acquire_lane(C);
    return selftest_msm_plan(*L, scalars, n, table_c, WindowShard{w_off, w_stride}, (const uint8_t*)mask, info, bstart, bend, cap_buckets,
                             vals, cap_vals, tasks, cap_tasks, multi, cap_multi, hot, cap_hot);
}

int wsnark_selftest_msm_geometry(uint64_t n, uint32_t table_c, uint32_t rank, uint32_t world, uint32_t* words) {
    static_assert(WSNARK_MSM_GEOMETRY_WORDS == kMsmGeometryWords && WSNARK_MSM_TABLE_C_AUTO == kMsmTableAuto, "words of the geometry hook");
    if (!words) return WSNARK_ERR_ARG;
    return selftest_msm_geometry(n, table_c, WindowShard{rank, world}, words);      // (no context: the geometry is host arithmetic)
}

int wsnark_selftest_msm_accumulate(int g, const void* points, uint64_t n_points, const uint32_t* vals, uint64_t n_vals, const uint32_t* tasks,
                                   uint64_t n_tasks, void* out) {
    REQUIRE_CTX();
    return selftest_msm_accumulate(g, points, n_points, vals, n_vals, tasks, n_tasks, out);      // (every argument is checked there)
}

int wsnark_selftest_field29(int which, int impl, int op, const uint32_t* operands, uint32_t* out, uint64_t n) {
    REQUIRE_CTX();
    if (n && (!operands || !out)) return WSNARK_ERR_ARG;
    return selftest_field29(which, impl, op, operands, out, n);
}

int wsnark_peak_probe(int probe, double* gops_per_s) {
    REQUIRE_CTX();
    return peak_probe(probe, gops_per_s);
}

// ---- pinned host buffers ----
int wsnark_host_alloc(size_t bytes, void** out) {
    REQUIRE_CTX();
    if (!out) return WSNARK_ERR_ARG;
    *out = nullptr;
    WS_HIP_CHECK(hipHostMalloc(out, bytes ? bytes : 16, 0));
    return WSNARK_OK;
}
void wsnark_host_free(void* p) {
    if (!p) return;
    if (Context* C = ctx()) (void)hipSetDevice(C->device);
    (void)hipHostFree(p);
}

// ---- measurement switches ----
int wsnark_tuning_set(const char* name, int64_t value) {
    if (!name || !*name) return WSNARK_ERR_ARG;
    tuning_set(name, value == INT64_MIN ? LONG_MIN : (long)value);
    return WSNARK_OK;
}

// ---- timing ----
void wsnark_timing_enable(int on) {
    Context* C = ctx();
    if (C) { C->timer.enabled = on != 0; C->timer.dominant_only = on == 2; }
}
void wsnark_timing_reset(void) {
    Context* C = ctx();
    if (C) C->timer.reset();
}
size_t wsnark_timing_report(char* buf, size_t cap) {
    Context* C = ctx();
    if (!C) return 0;
    (void)hipSetDevice(C->device);
    (void)hipStreamSynchronize(C->stream);
    for (int i = 0; i < C->n_lanes; i++) {
        (void)hipStreamSynchronize(C->lanes[i].stream);
        (void)hipStreamSynchronize(C->lanes[i].stream2);
    }
    C->timer.collect();
    std::string s;
    for (auto& kv : C->timer.acc) {
        char line[256];
        snprintf(line, sizeof line, "%s %.6f %llu\n", kv.first.c_str(), kv.second.first, (unsigned long long)kv.second.second);
        s += line;
    }
    if (buf && cap) {
        size_t k = s.size() < cap - 1 ? s.size() : cap - 1;
        memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return s.size();
}

}  // extern "C"
