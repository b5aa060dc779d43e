/*
 * wsnark_napi.c -- thin N-API addon over the C ABI of libwsnark.so (include/wsnark.h).
 *
 * This is the binding a wasmsnark maintainer would add to replace the worker pool: each JS
 * function maps 1:1 to one C entry point and returns a Promise (napi async work, so the event
 * loop is never blocked), with the reference's byte layouts (Jacobian-Montgomery 96/192 B,
 * plain-form h, ...).  Reference seam: src/bn128.js:102-166 (worker commands), :353-415, :569-720.
 * libwsnark.so (../libwsnark.so next to this addon: the in-tree hipcc build) is dlopen'ed by init();
 * there is no fallback, no path argument and no environment override: if it cannot be loaded or finds no GPU,
 * init() throws.
 */
#define NAPI_VERSION 4
#define _GNU_SOURCE
#include <dlfcn.h>
#include <node_api.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct wsnark_pkey wsnark_pkey_t;
typedef struct wsnark_points wsnark_points_t;
typedef struct wsnark_group wsnark_group_t;
typedef struct wsnark_group_pkey wsnark_group_pkey_t;
typedef struct wsnark_circuit_res wsnark_circuit_res_t;
typedef struct wsnark_kzg_srs wsnark_kzg_srs_t;
static struct {
    void* h;
    int (*init)(int);
    void (*shutdown)(void);
    const char* (*last_error)(void);
    const char* (*device_info)(void);
    int (*g1_msm)(const void*, const void*, uint64_t, void*);
    int (*g2_msm)(const void*, const void*, uint64_t, void*);
    int (*fr_ntt)(void*, uint64_t, int, int);
    int (*calc_h)(const void*, const void*, size_t, const void*, size_t, uint32_t, uint32_t, void*);
    int (*pkey_load)(const void*, size_t, wsnark_pkey_t**);
    void (*pkey_free)(wsnark_pkey_t*);
    int (*pkey_info)(const wsnark_pkey_t*, uint32_t*, uint32_t*, uint32_t*);
    int (*prove)(wsnark_pkey_t*, const void*, size_t, const void*, const void*, void*);
    int (*prove_batch)(wsnark_pkey_t*, const void*, size_t, uint64_t, const void*, const void*, void*, void*, void*);
    int (*last_blinding)(void*, void*);
    int (*verify)(const void*, size_t, const void*, uint64_t, const void*, int*);
    int (*verify_batch)(const void*, size_t, const void*, uint64_t, const void*, uint64_t, uint8_t*);
    int (*host_alloc)(size_t, void**);
    void (*host_free)(void*);
    int (*pkey_load_stats)(const wsnark_pkey_t*, double*);
    int (*pkey_wait_tables)(wsnark_pkey_t*);
    int (*points_load)(int, const void*, uint64_t, wsnark_points_t**);
    void (*points_free)(wsnark_points_t*);
    int (*points_info)(const wsnark_points_t*, int*, uint64_t*, uint32_t*, uint32_t*, uint64_t*);
    int (*points_msm)(wsnark_points_t*, const void*, uint64_t, void*);
    /* several GPUs in this one process (include/wsnark.h: wsnark_group_*) */
    int (*group_create)(const int*, uint32_t, wsnark_group_t**);
    void (*group_free)(wsnark_group_t*);
    int (*group_pkey_load)(wsnark_group_t*, const void*, size_t, wsnark_group_pkey_t**);
    void (*group_pkey_free)(wsnark_group_pkey_t*);
    int (*group_pkey_info)(const wsnark_group_pkey_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, int*);
    int (*group_pkey_wait_tables)(wsnark_group_pkey_t*);
    int (*group_prove)(wsnark_group_pkey_t*, const void*, size_t, const void*, const void*, void*);
    int (*group_last_blinding)(wsnark_group_t*, void*, void*);
    int (*group_g1_msm)(wsnark_group_t*, const void*, const void*, uint64_t, void*);
    int (*group_g2_msm)(wsnark_group_t*, const void*, const void*, uint64_t, void*);
    /* key files: proving_key.bin or the WSNARK64 container (include/wsnark.h: wsnark_pkey_load_file) */
    int (*pkey_load_file)(const char*, uint32_t, uint32_t, uint32_t, wsnark_pkey_t**);
    int (*pkey_file_info)(const char*, uint32_t*, uint32_t*, uint32_t*, uint64_t*, int*);
    int (*group_pkey_load_file)(wsnark_group_t*, const char*, wsnark_group_pkey_t**);
    /* the audit of a key's bytes or of a key file (include/wsnark.h: wsnark_pkey_check, wsnark_pkey_report_t) */
    int (*pkey_check)(const void*, size_t, uint32_t, const void*, void*);
    int (*pkey_check_file)(const char*, uint32_t, const void*, void*);
    /* the phase-2 delta contribution and its check (include/wsnark.h: wsnark_pkey_contribute*, wsnark_pkey_delta_verify*) */
    int (*pkey_contribute)(const void*, size_t, const void*, void*, size_t, void*);
    int (*pkey_contribute_file)(const char*, const char*, const void*, void*);
    int (*pkey_delta_verify)(const void*, size_t, const void*, size_t, const void*, void*);
    int (*pkey_delta_verify_file)(const char*, const char*, const void*, void*);
    /* the first key of a ceremony (include/wsnark.h: wsnark_g{1,2}_ntt, wsnark_pkey_setup_pkey) */
    int (*g1_ntt)(const void*, uint64_t, int, void*);
    int (*g2_ntt)(const void*, uint64_t, int, void*);
    int (*pkey_setup_pkey)(const void*, const void*, void*, size_t, size_t*, void*, void*);
    int (*pkey_setup_size)(const void*, size_t*);
    /* snarkjs' .zkey in and out (include/wsnark.h: wsnark_zkey_*) */
    int (*zkey_info)(const void*, size_t, void*);
    int (*zkey_import)(const void*, size_t, void*, size_t, size_t*, void*, size_t, void*);
    int (*zkey_export)(const void*, size_t, const void*, size_t, uint64_t, void*, size_t, size_t*, void*);
    int (*zkey_export_size)(uint32_t, uint32_t, uint32_t, uint64_t, uint64_t, size_t*);
    /* ... and straight into a resident key (wsnark_pkey_load_zkey*) */
    int (*pkey_load_zkey)(const void*, size_t, wsnark_pkey_t**, void*, size_t, void*);
    int (*pkey_load_zkey_file)(const char*, wsnark_pkey_t**, void*, size_t, void*);
    int (*zkey_vk_len)(const void*, size_t, size_t*);
    int (*zkey_vk_len_file)(const char*, size_t*);
    /* powers of tau (include/wsnark.h: wsnark_g{1,2}_mul_batch, wsnark_powers_contribute, wsnark_powers_check) */
    int (*g1_mul)(const void*, const void*, uint64_t, void*);
    int (*g2_mul)(const void*, const void*, uint64_t, void*);
    int (*powers_contribute)(const void*, const void*, const void*, const void*, void*, void*, void*, void*, void*, void*);
    int (*powers_check)(const void*, uint32_t, const void*, void*);
    /* a key against its circuit and its powers of tau (include/wsnark.h: wsnark_pkey_circuit_check*) */
    int (*pkey_circuit_check)(const void*, size_t, const void*, const void*, const void*, size_t, uint64_t, const void*, void*);
    int (*pkey_circuit_check_file)(const char*, const void*, const void*, const void*, size_t, uint64_t, const void*, void*);
    /* a witness against its circuit (include/wsnark.h: wsnark_circuit_load, wsnark_witness_check, wsnark_circuit_witness_check) */
    int (*circuit_load)(const void*, wsnark_circuit_res_t**);
    void (*circuit_free)(wsnark_circuit_res_t*);
    int (*circuit_info)(const wsnark_circuit_res_t*, uint32_t*, uint32_t*, uint32_t*, uint64_t*, uint64_t*);
    int (*witness_check)(const void*, const void*, size_t, uint64_t*, void*, uint64_t, void*);
    int (*circuit_witness_check)(wsnark_circuit_res_t*, const void*, size_t, uint64_t*, void*, uint64_t, void*);
    int (*circuit_witness_check_batch)(wsnark_circuit_res_t*, const void*, size_t, uint64_t, void*, uint64_t*, void*, uint64_t, void*);
    /* a circuit in row form (include/wsnark.h: wsnark_circuit_from_rows_size, wsnark_circuit_from_rows, wsnark_circuit_load_rows) */
    int (*circuit_from_rows_size)(const void*, uint32_t, uint32_t*, uint64_t*);
    int (*circuit_from_rows)(const void*, uint32_t, void*, uint64_t, void*, uint64_t, void*, uint64_t, uint32_t*, void*);
    int (*circuit_load_rows)(const void*, uint32_t, wsnark_circuit_res_t**);
    /* compressed points and 128-byte proofs (include/wsnark.h: wsnark_g{1,2}_compress / _decompress, wsnark_proof_*, ..._batch_compressed) */
    int (*g1_compress)(const void*, uint64_t, int, void*, uint8_t*, uint64_t*);
    int (*g2_compress)(const void*, uint64_t, int, void*, uint8_t*, uint64_t*);
    int (*g1_decompress)(const void*, uint64_t, int, uint32_t, void*, uint8_t*, uint64_t*);
    int (*g2_decompress)(const void*, uint64_t, int, uint32_t, void*, uint8_t*, uint64_t*);
    int (*proof_compress)(const void*, uint64_t, int, void*, uint8_t*);
    int (*proof_decompress)(const void*, uint64_t, int, void*, uint8_t*);
    int (*verify_batch_compressed)(const void*, size_t, const void*, uint64_t, const void*, uint64_t, int, uint8_t*);
    /* KZG on powers of tau (include/wsnark.h: wsnark_kzg_*, wsnark_fr_poly_eval, wsnark_fr_poly_divide) */
    int (*kzg_srs_load)(const void*, uint64_t, wsnark_kzg_srs_t**);
    void (*kzg_srs_free)(wsnark_kzg_srs_t*);
    int (*kzg_commit)(wsnark_kzg_srs_t*, const void*, uint64_t, uint64_t, int, void*);
    int (*kzg_open)(wsnark_kzg_srs_t*, const void*, uint64_t, uint64_t, const void*, const void*, void*, void*);
    int (*kzg_verify)(const void*, const void*, const void*, uint64_t, const void*, const void*, const void*, const void*, int*);
    int (*poly_eval)(const void*, uint64_t, uint64_t, const void*, void*);
    int (*poly_divide)(const void*, uint64_t, const void*, void*, void*);
    char dir[4096];
} L;

#define CHECK(env, call)                                                        \
    do {                                                                        \
        if ((call) != napi_ok) {                                                \
            napi_throw_error((env), NULL, "wsnark_napi: N-API call failed: " #call); \
            return NULL;                                                        \
        }                                                                       \
    } while (0)

/* The library this addon binds, relative to the addon's own directory: the in-tree hipcc build.  No argument and no environment
 * variable changes it; the test-suite's emulator host is a SEPARATE build of this file (make -C wasmsnark_amd/js emul ->
 * tests/emul/wsnark_napi_emul.node, compiled with another WSNARK_NAPI_LIB_RELPATH) that the product never loads. */
#ifndef WSNARK_NAPI_LIB_RELPATH
#define WSNARK_NAPI_LIB_RELPATH "../../libwsnark.so"
#endif
static int load_lib(char* err, size_t errlen) {
    char path[4200];
    if (L.h) return 0;
    snprintf(path, sizeof path, "%s/%s", L.dir, WSNARK_NAPI_LIB_RELPATH);
    L.h = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
    if (!L.h) { snprintf(err, errlen, "cannot load %s: %s", path, dlerror()); return -1; }
#define SYM(field, name)                                                            \
    *(void**)(&L.field) = dlsym(L.h, name);                                         \
    if (!L.field) { snprintf(err, errlen, "%s lacks symbol %s", path, name); return -1; }
    SYM(init, "wsnark_init") SYM(shutdown, "wsnark_shutdown") SYM(last_error, "wsnark_last_error")
    SYM(device_info, "wsnark_device_info") SYM(g1_msm, "wsnark_g1_msm") SYM(g2_msm, "wsnark_g2_msm")
    SYM(fr_ntt, "wsnark_fr_ntt") SYM(calc_h, "wsnark_calc_h") SYM(pkey_load, "wsnark_pkey_load")
    SYM(pkey_free, "wsnark_pkey_free") SYM(pkey_info, "wsnark_pkey_info") SYM(prove, "wsnark_groth16_prove")
    SYM(last_blinding, "wsnark_last_blinding") SYM(verify, "wsnark_groth16_verify")
    SYM(verify_batch, "wsnark_groth16_verify_batch") SYM(prove_batch, "wsnark_groth16_prove_batch")
    SYM(host_alloc, "wsnark_host_alloc") SYM(host_free, "wsnark_host_free")
    SYM(pkey_load_stats, "wsnark_pkey_load_stats") SYM(pkey_wait_tables, "wsnark_pkey_wait_tables")
    SYM(points_load, "wsnark_points_load") SYM(points_free, "wsnark_points_free") SYM(points_info, "wsnark_points_info") SYM(points_msm, "wsnark_points_msm")
    SYM(group_create, "wsnark_group_create") SYM(group_free, "wsnark_group_free") SYM(group_pkey_load, "wsnark_group_pkey_load")
    SYM(group_pkey_free, "wsnark_group_pkey_free") SYM(group_pkey_info, "wsnark_group_pkey_info")
    SYM(group_pkey_wait_tables, "wsnark_group_pkey_wait_tables") SYM(group_prove, "wsnark_group_prove")
    SYM(group_last_blinding, "wsnark_group_last_blinding") SYM(group_g1_msm, "wsnark_group_g1_msm") SYM(group_g2_msm, "wsnark_group_g2_msm")
    SYM(pkey_load_file, "wsnark_pkey_load_file") SYM(pkey_file_info, "wsnark_pkey_file_info") SYM(group_pkey_load_file, "wsnark_group_pkey_load_file")
    SYM(pkey_check, "wsnark_pkey_check") SYM(pkey_check_file, "wsnark_pkey_check_file")
    SYM(pkey_contribute, "wsnark_pkey_contribute") SYM(pkey_contribute_file, "wsnark_pkey_contribute_file")
    SYM(pkey_delta_verify, "wsnark_pkey_delta_verify") SYM(pkey_delta_verify_file, "wsnark_pkey_delta_verify_file")
    SYM(g1_ntt, "wsnark_g1_ntt") SYM(g2_ntt, "wsnark_g2_ntt") SYM(pkey_setup_pkey, "wsnark_pkey_setup_pkey") SYM(pkey_setup_size, "wsnark_pkey_setup_size")
    SYM(g1_mul, "wsnark_g1_mul_batch") SYM(g2_mul, "wsnark_g2_mul_batch") SYM(powers_contribute, "wsnark_powers_contribute") SYM(powers_check, "wsnark_powers_check")
    SYM(pkey_circuit_check, "wsnark_pkey_circuit_check") SYM(pkey_circuit_check_file, "wsnark_pkey_circuit_check_file")
    SYM(circuit_load, "wsnark_circuit_load") SYM(circuit_free, "wsnark_circuit_free") SYM(circuit_info, "wsnark_circuit_info")
    SYM(witness_check, "wsnark_witness_check") SYM(circuit_witness_check, "wsnark_circuit_witness_check")
    SYM(circuit_witness_check_batch, "wsnark_circuit_witness_check_batch")
    SYM(circuit_from_rows_size, "wsnark_circuit_from_rows_size") SYM(circuit_from_rows, "wsnark_circuit_from_rows")
    SYM(circuit_load_rows, "wsnark_circuit_load_rows")
    SYM(g1_compress, "wsnark_g1_compress") SYM(g2_compress, "wsnark_g2_compress") SYM(g1_decompress, "wsnark_g1_decompress")
    SYM(g2_decompress, "wsnark_g2_decompress") SYM(proof_compress, "wsnark_proof_compress") SYM(proof_decompress, "wsnark_proof_decompress")
    SYM(verify_batch_compressed, "wsnark_groth16_verify_batch_compressed")
    SYM(zkey_info, "wsnark_zkey_info") SYM(zkey_import, "wsnark_zkey_import") SYM(zkey_export, "wsnark_zkey_export") SYM(zkey_export_size, "wsnark_zkey_export_size")
    SYM(pkey_load_zkey, "wsnark_pkey_load_zkey") SYM(pkey_load_zkey_file, "wsnark_pkey_load_zkey_file") SYM(zkey_vk_len, "wsnark_zkey_vk_len") SYM(zkey_vk_len_file, "wsnark_zkey_vk_len_file")
    SYM(kzg_srs_load, "wsnark_kzg_srs_load") SYM(kzg_srs_free, "wsnark_kzg_srs_free") SYM(kzg_commit, "wsnark_kzg_commit") SYM(kzg_open, "wsnark_kzg_open")
    SYM(kzg_verify, "wsnark_kzg_verify") SYM(poly_eval, "wsnark_fr_poly_eval") SYM(poly_divide, "wsnark_fr_poly_divide")
#undef SYM
    return 0;
}

/* ArrayBuffer | Buffer | TypedArray | DataView -> (ptr, len); returns 0 on failure */
static int get_bytes(napi_env env, napi_value v, uint8_t** p, size_t* n) {
    bool is;
    if (napi_is_arraybuffer(env, v, &is) == napi_ok && is) return napi_get_arraybuffer_info(env, v, (void**)p, n) == napi_ok;
    if (napi_is_buffer(env, v, &is) == napi_ok && is) return napi_get_buffer_info(env, v, (void**)p, n) == napi_ok;
    if (napi_is_typedarray(env, v, &is) == napi_ok && is) {
        napi_typedarray_type t; size_t len, off; napi_value ab; void* data;
        if (napi_get_typedarray_info(env, v, &t, &len, &data, &ab, &off) != napi_ok) return 0;
        static const size_t esz[] = {1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8};
        *p = (uint8_t*)data; *n = len * esz[t];
        return 1;
    }
    if (napi_is_dataview(env, v, &is) == napi_ok && is) {
        size_t len, off; napi_value ab; void* data;
        if (napi_get_dataview_info(env, v, &len, &data, &ab, &off) != napi_ok) return 0;
        *p = (uint8_t*)data; *n = len;
        return 1;
    }
    return 0;
}

enum { OP_G1, OP_G2, OP_NTT, OP_CALCH, OP_PROVE, OP_LOADKEY, OP_VERIFY, OP_HASH, OP_WAIT_TABLES,
       OP_GROUP_G1, OP_GROUP_G2, OP_GROUP_LOADKEY, OP_GROUP_PROVE, OP_GROUP_WAIT_TABLES, OP_POINTS_LOAD, OP_POINTS_MSM,
       OP_LOADKEY_FILE, OP_LOADKEY_ZKEY, OP_LOADKEY_ZKEY_FILE, OP_GROUP_LOADKEY_FILE, OP_VERIFY_BATCH, OP_CHECK_KEY, OP_CONTRIBUTE, OP_DELTA_VERIFY, OP_GROUP_NTT, OP_NEW_KEY,
       OP_MUL_POINTS, OP_POWERS_CONTRIBUTE, OP_POWERS_CHECK, OP_CHECK_KEY_CIRCUIT, OP_CIRCUIT_LOAD, OP_WITNESS_CHECK,
       OP_CIRCUIT_WITNESS_CHECK, OP_PROVE_BATCH, OP_CIRCUIT_WITNESS_CHECK_BATCH, OP_CIRCUIT_FROM_ROWS, OP_CIRCUIT_LOAD_ROWS, OP_ZKEY_IMPORT, OP_ZKEY_EXPORT,
       OP_CODEC_POINTS, OP_CODEC_PROOFS, OP_VERIFY_BATCH_COMPRESSED,
       OP_KZG_LOAD, OP_KZG_COMMIT, OP_KZG_OPEN, OP_KZG_VERIFY, OP_POLY_EVAL, OP_POLY_DIVIDE };
/* A group and the keys loaded on it.  The JS side holds them as externals; a key's finalizer must not touch a group that
 * terminate() has already freed (wsnark_group_free frees the keys that are left), so every group handle carries a `live` flag
 * that outlives the group itself and every key handle points at its group's handle. */
/* Lifetime: jobs queued on the libuv pool hold raw pointers into the group, so the library's group must outlive every
 * job that was queued while it was live.  `inflight` counts them (touched on the JS thread only: start_job / job_complete);
 * groupFree / terminate() / the finalizer only mark the group dead (`live` = 0, read by the pool threads) and the LAST job's
 * completion frees it -- at once when nothing is in flight.  A job that reaches the pool after the group died is rejected
 * without entering the library. */
/* Every external this addon hands to JS starts with a tag naming its kind (Node 12 has no napi_type_tag_object): a group key passed
 * where a key handle is expected -- index.js once did that after terminate() -- is refused instead of being read as the other struct. */
#define TAG_KEY 0x77736e4b45593031ull
#define TAG_POINTS 0x77736e5054533031ull
#define TAG_GROUP 0x77736e4752503031ull
#define TAG_GKEY 0x77736e474b593031ull
#define TAG_CIRCUIT 0x77736e4349523031ull
#define TAG_SRS 0x77736e5352533031ull
typedef struct { uint64_t tag; void* p; } handle_t;                 /* a key (wsnark_pkey_t*), a point set (wsnark_points_t*) or a resident circuit */
typedef struct { uint64_t tag; wsnark_group_t* g; int live; int inflight; int refs; } group_ref_t;
typedef struct { uint64_t tag; wsnark_group_pkey_t* k; group_ref_t* gr; } gkey_ref_t;
#define KEY_OBJECT_MARK "wsnarkKeyObject"      /* own property of the object that wraps a key handle: nothing else is unwrapped */
static void* get_handle(napi_env env, napi_value v, uint64_t tag) {
    void* p = NULL;
    napi_valuetype t;
    if (napi_typeof(env, v, &t) != napi_ok) return NULL;
    if (t == napi_object) {      /* the key handle of a .zkey: an object that carries .vk, the handle_t wrapped inside (js_loadkey_zkey) */
        bool ours = false;
        napi_value mark;
        if (napi_create_string_utf8(env, KEY_OBJECT_MARK, NAPI_AUTO_LENGTH, &mark) != napi_ok || napi_has_own_property(env, v, mark, &ours) != napi_ok ||
            !ours || napi_unwrap(env, v, &p) != napi_ok || !p)
            return NULL;
        return *(const uint64_t*)p == tag ? p : NULL;
    }
    if (t != napi_external || napi_get_value_external(env, v, &p) != napi_ok || !p) return NULL;
    return *(const uint64_t*)p == tag ? p : NULL;
}
static void* get_plain(napi_env env, napi_value v, uint64_t tag) {   /* the library pointer inside a key / points handle */
    handle_t* h = (handle_t*)get_handle(env, v, tag);
    return h ? h->p : NULL;
}
static handle_t* new_handle(uint64_t tag, void* p) {
    handle_t* h = (handle_t*)calloc(1, sizeof *h);
    if (h) { h->tag = tag; h->p = p; }
    return h;
}
static void group_ref_drop(group_ref_t* gr) { if (--gr->refs == 0) { gr->tag = 0; free(gr); } }
static void group_release(group_ref_t* gr);
typedef struct {
    int op, rc;
    napi_async_work work;
    napi_deferred deferred;
    napi_ref refs[8];
    int nrefs;
    uint8_t *a, *b, *c, *r32, *s32;
    size_t na, nb, nc;
    uint8_t* in[9];             /* OP_NEW_KEY: tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2, polsA, polsB, polsC; the rows: 3 x (row_ptr, col, coef) */
    size_t nin[9];
    uint32_t u2;
    uint32_t u0, u1;
    int i0, i1;
    wsnark_pkey_t* key;
    group_ref_t* gr;
    gkey_ref_t* gk;
    group_ref_t* gr_used;       /* the group this job runs on (counted in its `inflight`), or NULL */
    wsnark_points_t* pts;
    wsnark_kzg_srs_t* srs;       /* OP_KZG_LOAD: the new handle; OP_KZG_COMMIT, OP_KZG_OPEN: the one summed over */
    wsnark_circuit_res_t* circ;  /* OP_CIRCUIT_LOAD: the new handle; OP_CIRCUIT_WITNESS_CHECK: the one checked against */
    uint64_t cap;               /* the witness checks: entries the two lists hold */
    uint8_t* out;
    size_t nout;
    char* path;                 /* key file (OP_LOADKEY_FILE, OP_GROUP_LOADKEY_FILE): owned by the job */
    char* path2;                /* the second file of OP_CONTRIBUTE (output) / OP_DELTA_VERIFY (new key): owned by the job */
    char err[512];
} job_t;

/* 128-bit digest of a run of bytes: four independent multiply-rotate lanes over 8-byte words, folded with the length.
 * Not cryptographic: it only has to notice that the bytes behind a cached key handle are no longer the bytes that were loaded. */
static void hash_run(const uint8_t* p, size_t n, uint8_t out[16]) {
    uint64_t h[4] = {0x9e3779b97f4a7c15ull, 0xc2b2ae3d27d4eb4full, 0x165667b19e3779f9ull, 0x27d4eb2f165667c5ull};
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
        uint64_t w[4];
        memcpy(w, p + i, 32);
        for (int k = 0; k < 4; k++) {
            h[k] = (h[k] ^ w[k]) * 0xff51afd7ed558ccdull;
            h[k] = (h[k] << 29) | (h[k] >> 35);
        }
    }
    uint64_t tail[4] = {0, 0, 0, 0};
    memcpy(tail, p + i, n - i);
    for (int k = 0; k < 4; k++) h[k] = (h[k] ^ tail[k]) * 0xc4ceb9fe1a85ec53ull;
    uint64_t a = h[0] ^ ((h[1] << 21) | (h[1] >> 43)) ^ (uint64_t)n, b = h[2] ^ ((h[3] << 37) | (h[3] >> 27));
    a = (a ^ (a >> 33)) * 0xff51afd7ed558ccdull; b = (b ^ (b >> 29)) * 0xc4ceb9fe1a85ec53ull;
    a ^= b >> 31; b ^= a >> 27;
    memcpy(out, &a, 8); memcpy(out + 8, &b, 8);
}
/* ... of a whole buffer: the digests of its 4 MiB blocks, digested.  One core streams about 12 GB/s through hash_run -- 50 ms
 * for a 0.6 GB key, longer than the key's load takes -- so the blocks are dealt to up to HASH_THREADS threads (the result does
 * not depend on how many there were). */
#define HASH_BLOCK ((size_t)4 << 20)
#define HASH_THREADS 8
typedef struct { const uint8_t* p; size_t n, nblocks; uint8_t* digests; unsigned first, step; } hash_part_t;
static void* hash_part(void* arg) {
    hash_part_t* h = (hash_part_t*)arg;
    for (size_t b = h->first; b < h->nblocks; b += h->step) {
        const size_t lo = b * HASH_BLOCK, len = h->n - lo < HASH_BLOCK ? h->n - lo : HASH_BLOCK;
        hash_run(h->p + lo, len, h->digests + 16 * b);
    }
    return NULL;
}
static int hash_bytes(const uint8_t* p, size_t n, uint8_t out[16]) {
    const size_t nblocks = n ? (n + HASH_BLOCK - 1) / HASH_BLOCK : 1;
    uint8_t* digests = (uint8_t*)calloc(nblocks, 16);
    if (!digests) return -1;
    unsigned want = nblocks < HASH_THREADS ? (unsigned)nblocks : HASH_THREADS;
    hash_part_t parts[HASH_THREADS];
    pthread_t tid[HASH_THREADS];
    unsigned started = 0;
    for (unsigned t = 0; t < want; t++) parts[t] = (hash_part_t){p, n, nblocks, digests, t, want};
    for (unsigned t = 1; t < want; t++) {
        if (pthread_create(&tid[t], NULL, hash_part, &parts[t]) != 0) break;
        started = t;
    }
    /* (threads that could not be started: their blocks are done here, after this thread's own) */
    hash_part(&parts[0]);
    for (unsigned t = started + 1; t < want; t++) hash_part(&parts[t]);
    for (unsigned t = 1; t <= started; t++) pthread_join(tid[t], NULL);
    uint8_t top[16];
    hash_run(digests, nblocks * 16, top);
    uint64_t a, b;
    memcpy(&a, top, 8); memcpy(&b, top + 8, 8);
    a ^= (uint64_t)n * 0x9e3779b97f4a7c15ull;
    memcpy(out, &a, 8); memcpy(out + 8, &b, 8);
    free(digests);
    return 0;
}

#define PKEY_DELTA_REPORT_BYTES 104      /* sizeof(wsnark_pkey_delta_report_t) */
#define PKEY_DELTA_VERDICT_BYTES 40      /* sizeof(wsnark_pkey_delta_verdict_t) */
#define PKEY_SETUP_REPORT_BYTES 192      /* sizeof(wsnark_pkey_setup_report_t) */
#define POWERS_REPORT_BYTES 192          /* sizeof(wsnark_powers_report_t) */
#define PKEY_CIRCUIT_VERDICT_BYTES 56    /* sizeof(wsnark_pkey_circuit_verdict_t) */
#define WITNESS_REPORT_BYTES 80          /* sizeof(wsnark_witness_report_t) */
#define WITNESS_VERDICT_BYTES 48         /* sizeof(wsnark_witness_verdict_t) */
#define WITNESS_BATCH_REPORT_BYTES 64    /* sizeof(wsnark_witness_batch_report_t) */
#define ROWS_REPORT_BYTES 152            /* sizeof(wsnark_rows_report_t) */
#define ZKEY_INFO_BYTES 56              /* sizeof(wsnark_zkey_info_t) */
#define ZKEY_REPORT_BYTES 136           /* sizeof(wsnark_zkey_report_t) */
#define ZKEY_HEAD_BYTES (16 + ZKEY_REPORT_BYTES)      /* importZkey / exportZkey: u64 length of the key or file, u64 length of the vk, the report */
#define ROWS_HEAD_BYTES (8 + 24 + ROWS_REPORT_BYTES)      /* circuitFromRows: u32 domain, u32 0, lens[3], the report; then the three streams */
/* wsnark_powers_t and wsnark_circuit_t (include/wsnark.h) */
typedef struct {
    uint32_t domain;
    const void* tau_g1; uint64_t tau_g1_len;
    const void* tau_g2; uint64_t tau_g2_len;
    const void* alpha_tau_g1; uint64_t alpha_tau_g1_len;
    const void* beta_tau_g1; uint64_t beta_tau_g1_len;
    const void* beta_g2;
} powers_t;
typedef struct {
    uint32_t n_vars, n_public, domain;
    const void* polsA; uint64_t polsA_len;
    const void* polsB; uint64_t polsB_len;
    const void* polsC; uint64_t polsC_len;
} circuit_t;
/* wsnark_rows_t: the rows' (nVars, nPublic, nConstraints, domain) in u0, u1, i0, u2, flags in i1, the nine arrays in in[0..8] */
typedef struct { const void *row_ptr, *col, *coef; } rows_matrix_t;
typedef struct { uint32_t n_vars, n_public, n_constraints, domain; rows_matrix_t M[3]; } rows_t;
static void job_rows(const job_t* j, rows_t* R) {
    *R = (rows_t){j->u0, j->u1, (uint32_t)j->i0, j->u2, {{j->in[0], j->in[1], j->in[2]}, {j->in[3], j->in[4], j->in[5]}, {j->in[6], j->in[7], j->in[8]}}};
}
static void job_structs(const job_t* j, powers_t* P, circuit_t* K) {
    *P = (powers_t){j->u2, j->in[0], j->nin[0], j->in[1], j->nin[1], j->in[2], j->nin[2], j->in[3], j->nin[3], j->in[4]};
    *K = (circuit_t){j->u0, j->u1, j->u2, j->in[5], j->nin[5], j->in[6], j->nin[6], j->in[7], j->nin[7]};
}
static void job_execute(napi_env env, void* data) {
    (void)env;
    job_t* j = (job_t*)data;
    if (j->gr_used && !__atomic_load_n(&j->gr_used->live, __ATOMIC_ACQUIRE)) {      /* terminate() ran after this job was queued */
        j->rc = -1;
        snprintf(j->err, sizeof j->err, "wsnark: the group was terminated before this call ran");
        return;
    }
    switch (j->op) {
    case OP_G1: j->rc = L.g1_msm(j->a, j->b, j->na / 32, j->out); break;
    case OP_G2: j->rc = L.g2_msm(j->a, j->b, j->na / 32, j->out); break;
    case OP_NTT: memcpy(j->out, j->a, j->na); j->rc = L.fr_ntt(j->out, j->na / 32, j->i0, j->i1); break;
    case OP_CALCH: j->rc = L.calc_h(j->a, j->b, j->nb, j->c, j->nc, j->u0, j->u1, j->out); break;
    case OP_PROVE:   /* out = proof (384 B) | r | s actually used (same pool thread: wsnark_last_blinding is per thread) */
        j->rc = L.prove(j->key, j->a, j->na, j->r32, j->s32, j->out);
        if (!j->rc) j->rc = L.last_blinding(j->out + 384, j->out + 416);
        break;
    case OP_PROVE_BATCH: {   /* out = count proofs (384 B each) | count x (r | s) as used | the report (64 B) */
        const size_t n = j->u0;
        j->rc = L.prove_batch(j->key, j->a, j->na / n, n, j->r32, j->s32, j->out, j->out + 384 * n, j->out + 448 * n);
        break;
    }
    case OP_LOADKEY: j->rc = L.pkey_load(j->a, j->na, &j->key); break;
    case OP_LOADKEY_FILE: j->rc = L.pkey_load_file(j->path, 0, 1, 0, &j->key); break;
    case OP_LOADKEY_ZKEY:
    case OP_LOADKEY_ZKEY_FILE: {   /* out (sized here, from the file's container and section 2 alone: wsnark_zkey_vk_len*): the wsnark_zkey_report_t, the vk */
        size_t vk_len = 0;
        if ((j->rc = j->op == OP_LOADKEY_ZKEY_FILE ? L.zkey_vk_len_file(j->path, &vk_len) : L.zkey_vk_len(j->a, j->na, &vk_len))) break;
        j->nout = ZKEY_REPORT_BYTES + vk_len;
        j->out = (uint8_t*)calloc(j->nout, 1);
        if (!j->out) { j->rc = -1; snprintf(j->err, sizeof j->err, "wsnark: out of memory for the verification key"); return; }
        j->rc = j->op == OP_LOADKEY_ZKEY_FILE ? L.pkey_load_zkey_file(j->path, &j->key, j->out + ZKEY_REPORT_BYTES, vk_len, j->out)
                                              : L.pkey_load_zkey(j->a, j->na, &j->key, j->out + ZKEY_REPORT_BYTES, vk_len, j->out);
        break;
    }
    case OP_GROUP_LOADKEY_FILE: j->rc = L.group_pkey_load_file(j->gr->g, j->path, &j->gk->k); break;
    case OP_VERIFY: j->rc = L.verify(j->a, j->na, j->b, j->nb / 32, j->c, &j->i0); break;
    case OP_VERIFY_BATCH: j->rc = L.verify_batch(j->a, j->na, j->nb ? j->b : NULL, j->u0, j->c, j->nc / 384, j->out); break;
    case OP_VERIFY_BATCH_COMPRESSED:
        j->rc = L.verify_batch_compressed(j->a, j->na, j->nb ? j->b : NULL, j->u0, j->c, j->nc / 128, (int)j->u1, j->out);
        break;
    case OP_CODEC_POINTS: {   /* i0 = g, i1 = 1 compress / 0 decompress, u0 = encoding, u1 = flags; out = the records | a status byte each */
        const size_t in_sz = (j->i1 ? 64 : 32) * (size_t)j->i0, out_sz = (j->i1 ? 32 : 64) * (size_t)j->i0, n = j->na / in_sz;
        uint64_t bad = 0;
        if (j->i1) j->rc = (j->i0 == 1 ? L.g1_compress : L.g2_compress)(j->a, n, (int)j->u0, j->out, j->out + n * out_sz, &bad);
        else j->rc = (j->i0 == 1 ? L.g1_decompress : L.g2_decompress)(j->a, n, (int)j->u0, j->u1, j->out, j->out + n * out_sz, &bad);
        break;
    }
    case OP_CODEC_PROOFS: {   /* i1 = 1 compress / 0 decompress, u0 = encoding; out = the records | a status byte each */
        const size_t in_sz = j->i1 ? 384 : 128, out_sz = j->i1 ? 128 : 384, n = j->na / in_sz;
        j->rc = (j->i1 ? L.proof_compress : L.proof_decompress)(j->a, n, (int)j->u0, j->out, j->out + n * out_sz);
        break;
    }
    case OP_CHECK_KEY:
        j->rc = j->path ? L.pkey_check_file(j->path, j->u0, j->r32, j->out) : L.pkey_check(j->a, j->na, j->u0, j->r32, j->out);
        break;
    case OP_CONTRIBUTE:      /* out = the report (104 B), then -- for key bytes -- the new key */
        j->rc = j->path ? L.pkey_contribute_file(j->path, j->path2, j->r32, j->out)
                        : L.pkey_contribute(j->a, j->na, j->r32, j->out + PKEY_DELTA_REPORT_BYTES, j->na, j->out);
        break;
    case OP_DELTA_VERIFY:
        j->rc = j->path ? L.pkey_delta_verify_file(j->path, j->path2, j->r32, j->out) : L.pkey_delta_verify(j->a, j->na, j->b, j->nb, j->r32, j->out);
        break;
    case OP_ZKEY_IMPORT: {   /* out (sized here, from the file's own header): the head, the vk, proving_key.bin */
        uint8_t info[ZKEY_INFO_BYTES];
        uint64_t pkey_len, vk_len;
        if ((j->rc = L.zkey_info(j->a, j->na, info))) break;
        memcpy(&pkey_len, info + 40, 8); memcpy(&vk_len, info + 48, 8);
        j->nout = ZKEY_HEAD_BYTES + (size_t)vk_len + (size_t)pkey_len;
        j->out = (uint8_t*)calloc(j->nout, 1);
        if (!j->out) { j->rc = -1; snprintf(j->err, sizeof j->err, "wsnark: out of memory for the imported key"); return; }
        size_t len = 0;
        j->rc = L.zkey_import(j->a, j->na, j->out + ZKEY_HEAD_BYTES + vk_len, (size_t)pkey_len, &len, j->out + ZKEY_HEAD_BYTES, (size_t)vk_len, j->out + 16);
        pkey_len = len;
        memcpy(j->out, &pkey_len, 8); memcpy(j->out + 8, &vk_len, 8);
        break;
    }
    case OP_ZKEY_EXPORT: {   /* a = proving_key.bin, b = the vk in the verifier's layout, u0 = nPublic; out: the head, the file */
        uint32_t h[10];
        size_t len = 0;
        if (j->na < 40) { j->rc = -1; snprintf(j->err, sizeof j->err, "wsnark: the key is shorter than its header"); return; }
        memcpy(h, j->a, 40);
        const uint64_t la = (uint64_t)h[4] - h[3], lb = (uint64_t)h[5] - h[4], heads = 4 * (uint64_t)h[0];
        if ((j->rc = L.zkey_export_size(h[0], h[1], h[2], la > heads ? (la - heads) / 36 : 0, lb > heads ? (lb - heads) / 36 : 0, &len))) break;
        j->nout = ZKEY_HEAD_BYTES + len;
        j->out = (uint8_t*)calloc(j->nout, 1);
        if (!j->out) { j->rc = -1; snprintf(j->err, sizeof j->err, "wsnark: out of memory for the file"); return; }
        size_t cap = len;
        j->rc = L.zkey_export(j->a, j->na, j->b, j->nb, j->u0, j->out + ZKEY_HEAD_BYTES, cap, &len, j->out + 16);
        uint64_t l64 = len;
        memcpy(j->out, &l64, 8);
        break;
    }
    case OP_GROUP_NTT: j->rc = (j->i0 == 2 ? L.g2_ntt : L.g1_ntt)(j->a, j->na / (j->i0 == 2 ? 128 : 64), j->i1, j->out); break;
    case OP_NEW_KEY: {       /* out = the report (192 B), IC ((nPublic + 1) x 64 B), the key */
        powers_t P;
        circuit_t K;
        job_structs(j, &P, &K);
        const size_t head = PKEY_SETUP_REPORT_BYTES + ((size_t)j->u1 + 1) * 64;
        j->rc = L.pkey_setup_pkey(&P, &K, j->out + head, j->nout - head, NULL, j->out + PKEY_SETUP_REPORT_BYTES, j->out);
        break;
    }
    case OP_MUL_POINTS: j->rc = (j->i0 == 2 ? L.g2_mul : L.g1_mul)(j->a, j->b, j->nb / 32, j->out); break;
    case OP_POWERS_CONTRIBUTE: {      /* out = the report (192 B), then tau_g1', tau_g2', alpha_tau_g1', beta_tau_g1', beta_g2' */
        powers_t P;
        circuit_t K;
        job_structs(j, &P, &K);
        const size_t n = j->u1;       /* the domain if it is one the library accepts, else 0: nothing is written then */
        uint8_t* o = j->out + POWERS_REPORT_BYTES;
        j->rc = L.powers_contribute(&P, j->r32, j->s32, j->c, o, o + 128 * n, o + 256 * n, o + 320 * n, o + 384 * n, j->out);
        break;
    }
    case OP_POWERS_CHECK: {
        powers_t P;
        circuit_t K;
        job_structs(j, &P, &K);
        j->rc = L.powers_check(&P, j->u0, j->r32, j->out);
        break;
    }
    case OP_CHECK_KEY_CIRCUIT: {      /* b: the verification key's bytes (alfa1 | beta2 | gamma2 | delta2 | IC) or NULL */
        powers_t P;
        circuit_t K;
        job_structs(j, &P, &K);
        const uint64_t n_inputs = j->b ? (j->nb - 448) / 64 - 1 : 0;
        j->rc = j->path ? L.pkey_circuit_check_file(j->path, &P, &K, j->b, j->nb, n_inputs, j->r32, j->out)
                        : L.pkey_circuit_check(j->a, j->na, &P, &K, j->b, j->nb, n_inputs, j->r32, j->out);
        break;
    }
    case OP_CIRCUIT_LOAD: {
        powers_t P;
        circuit_t K;
        job_structs(j, &P, &K);
        j->rc = L.circuit_load(&K, &j->circ);
        break;
    }
    case OP_CIRCUIT_FROM_ROWS: {      /* out = ROWS_HEAD_BYTES, then polsA | polsB | polsC at their lengths */
        rows_t R;
        uint32_t dom = 0;
        uint64_t lens[3];
        job_rows(j, &R);
        if ((j->rc = L.circuit_from_rows_size(&R, (uint32_t)j->i1, &dom, lens))) break;
        j->nout = ROWS_HEAD_BYTES + (size_t)(lens[0] + lens[1] + lens[2]);
        j->out = (uint8_t*)calloc(j->nout, 1);
        if (!j->out) { j->rc = -1; snprintf(j->err, sizeof j->err, "circuitFromRows: out of memory"); return; }
        uint8_t* pols = j->out + ROWS_HEAD_BYTES;
        j->rc = L.circuit_from_rows(&R, (uint32_t)j->i1, pols, lens[0], pols + lens[0], lens[1], pols + lens[0] + lens[1], lens[2], &dom,
                                    j->out + 8 + 24);
        memcpy(j->out, &dom, 4);
        memcpy(j->out + 8, lens, 24);
        break;
    }
    case OP_CIRCUIT_LOAD_ROWS: {
        rows_t R;
        job_rows(j, &R);
        j->rc = L.circuit_load_rows(&R, (uint32_t)j->i1, &j->circ);
        break;
    }
    case OP_WITNESS_CHECK:            /* out = the report (80 B), cap x u64 row indices, cap x 96 B values */
    case OP_CIRCUIT_WITNESS_CHECK: {
        uint64_t* rows = j->cap ? (uint64_t*)(j->out + WITNESS_REPORT_BYTES) : NULL;
        uint8_t* vals = j->cap ? j->out + WITNESS_REPORT_BYTES + 8 * j->cap : NULL;
        if (j->op == OP_WITNESS_CHECK) {
            powers_t P;
            circuit_t K;
            job_structs(j, &P, &K);
            j->rc = L.witness_check(&K, j->a, j->na, rows, vals, j->cap, j->out);
        } else {
            j->rc = L.circuit_witness_check(j->circ, j->a, j->na, rows, vals, j->cap, j->out);
        }
        break;
    }
    case OP_CIRCUIT_WITNESS_CHECK_BATCH: {   /* out = the report (64 B), count verdicts (48 B each), count x cap u64, count x cap x 96 B */
        const size_t n = j->u0;
        uint8_t* ver = j->out + WITNESS_BATCH_REPORT_BYTES;
        uint64_t* rows = j->cap ? (uint64_t*)(ver + WITNESS_VERDICT_BYTES * n) : NULL;
        uint8_t* vals = j->cap ? ver + WITNESS_VERDICT_BYTES * n + 8 * n * j->cap : NULL;
        j->rc = L.circuit_witness_check_batch(j->circ, j->a, j->na / n, n, ver, rows, vals, j->cap, j->out);
        break;
    }
    case OP_WAIT_TABLES: j->rc = L.pkey_wait_tables(j->key); break;
    case OP_GROUP_G1: j->rc = L.group_g1_msm(j->gr->g, j->a, j->b, j->na / 32, j->out); break;
    case OP_GROUP_G2: j->rc = L.group_g2_msm(j->gr->g, j->a, j->b, j->na / 32, j->out); break;
    case OP_GROUP_LOADKEY: j->rc = L.group_pkey_load(j->gr->g, j->a, j->na, &j->gk->k); break;
    case OP_GROUP_PROVE:
        j->rc = L.group_prove(j->gk->k, j->a, j->na, j->r32, j->s32, j->out);
        if (!j->rc) j->rc = L.group_last_blinding(j->gk->gr->g, j->out + 384, j->out + 416);
        break;
    case OP_GROUP_WAIT_TABLES: j->rc = L.group_pkey_wait_tables(j->gk->k); break;
    /* KZG: u0 = len (coefficients per polynomial), na = count x len x 32; r32 = z, s32 = gamma or NULL */
    case OP_KZG_LOAD: j->rc = L.kzg_srs_load(j->a, j->na / 64, &j->srs); break;
    case OP_KZG_COMMIT: j->rc = L.kzg_commit(j->srs, j->a, j->u0, j->na / 32 / j->u0, j->i0, j->out); break;
    case OP_KZG_OPEN: {      /* out = count values | the proof */
        const uint64_t count = j->na / 32 / j->u0;
        j->rc = L.kzg_open(j->srs, j->a, j->u0, count, j->r32, j->s32, j->out, j->out + 32 * count);
        break;
    }
    case OP_KZG_VERIFY:      /* in: g1, g2 | tau g2, commitments, ys, proof */
        j->rc = L.kzg_verify(j->in[0], j->in[1], j->in[2], j->nin[2] / 64, j->r32, j->s32, j->in[3], j->in[4], &j->i0);
        break;
    case OP_POLY_EVAL: j->rc = L.poly_eval(j->a, j->u0, j->na / 32 / j->u0, j->r32, j->out); break;
    case OP_POLY_DIVIDE: j->rc = L.poly_divide(j->a, j->na / 32, j->r32, j->out, j->out + j->na - 32); break;      /* out = q | y */
    case OP_POINTS_LOAD: j->rc = L.points_load(j->i0, j->a, j->na / (j->i0 == 2 ? 128 : 64), &j->pts); break;
    case OP_POINTS_MSM: j->rc = L.points_msm(j->pts, j->a, j->na / 32, j->out); break;
    case OP_HASH:
        if (hash_bytes(j->a, j->na, j->out)) { j->rc = -1; snprintf(j->err, sizeof j->err, "hashBytes: out of memory"); return; }
        break;
    }
    if (j->rc) snprintf(j->err, sizeof j->err, "wsnark error %d: %s", j->rc, L.last_error());
}

/* JS thread.  The group dies now if no job is in flight on it, otherwise with the last of them (job_complete). */
static void group_release(group_ref_t* gr) {
    __atomic_store_n(&gr->live, 0, __ATOMIC_RELEASE);
    if (gr->g && gr->inflight == 0) { L.group_free(gr->g); gr->g = NULL; }
}
static void job_use_group(job_t* j, group_ref_t* gr) { j->gr_used = gr; gr->inflight++; gr->refs++; }
static void job_done_with_group(job_t* j) {
    group_ref_t* gr = j->gr_used;
    if (!gr) return;
    j->gr_used = NULL;
    gr->inflight--;
    if (!gr->live && gr->inflight == 0 && gr->g) { L.group_free(gr->g); gr->g = NULL; }
    group_ref_drop(gr);
}

static void key_finalize(napi_env env, void* data, void* hint) {
    (void)env; (void)hint;
    handle_t* h = (handle_t*)data;
    if (h) { if (h->p) L.pkey_free((wsnark_pkey_t*)h->p); h->tag = 0; free(h); }
}

static void points_finalize(napi_env env, void* data, void* hint) {
    (void)env; (void)hint;
    handle_t* h = (handle_t*)data;
    if (h) { if (h->p) L.points_free((wsnark_points_t*)h->p); h->tag = 0; free(h); }
}
static void circuit_finalize(napi_env env, void* data, void* hint) {
    (void)env; (void)hint;
    handle_t* h = (handle_t*)data;
    if (h) { if (h->p) L.circuit_free((wsnark_circuit_res_t*)h->p); h->tag = 0; free(h); }
}
static void srs_finalize(napi_env env, void* data, void* hint) {
    (void)env; (void)hint;
    handle_t* h = (handle_t*)data;
    if (h) { if (h->p) L.kzg_srs_free((wsnark_kzg_srs_t*)h->p); h->tag = 0; free(h); }
}
static void gkey_finalize(napi_env env, void* data, void* hint) {
    (void)env; (void)hint;
    gkey_ref_t* gk = (gkey_ref_t*)data;
    if (!gk) return;
    if (gk->k && gk->gr->live) L.group_pkey_free(gk->k);      /* (a dead or dying group takes its keys with it) */
    group_ref_drop(gk->gr);
    gk->tag = 0;
    free(gk);
}
static void group_finalize(napi_env env, void* data, void* hint) {
    (void)env; (void)hint;
    group_ref_t* gr = (group_ref_t*)data;
    if (!gr) return;
    group_release(gr);          /* (jobs in flight keep `gr` alive through their own reference and free the group when they finish) */
    group_ref_drop(gr);
}

static void job_complete(napi_env env, napi_status status, void* data) {
    job_t* j = (job_t*)data;
    napi_value res;
    if (status != napi_ok || j->rc) {
        napi_value msg, e;
        napi_create_string_utf8(env, j->rc ? j->err : "async work cancelled", NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, NULL, msg, &e);
        napi_reject_deferred(env, j->deferred, e);
        if ((j->op == OP_GROUP_LOADKEY || j->op == OP_GROUP_LOADKEY_FILE) && j->gk) { group_ref_drop(j->gk->gr); free(j->gk); }
    } else if (j->op == OP_GROUP_LOADKEY || j->op == OP_GROUP_LOADKEY_FILE) {
        napi_create_external(env, j->gk, gkey_finalize, NULL, &res);
        napi_resolve_deferred(env, j->deferred, res);
    } else if (j->op == OP_POINTS_LOAD) {
        napi_create_external(env, new_handle(TAG_POINTS, j->pts), points_finalize, NULL, &res);
        napi_resolve_deferred(env, j->deferred, res);
    } else if (j->op == OP_CIRCUIT_LOAD || j->op == OP_CIRCUIT_LOAD_ROWS) {
        handle_t* h = new_handle(TAG_CIRCUIT, j->circ);
        if (!h || napi_create_external(env, h, circuit_finalize, NULL, &res) != napi_ok) {      /* nothing would ever free the matrices */
            napi_value msg, e;
            L.circuit_free(j->circ);
            free(h);
            napi_create_string_utf8(env, "wsnark_napi: out of memory for the circuit handle", NAPI_AUTO_LENGTH, &msg);
            napi_create_error(env, NULL, msg, &e);
            napi_reject_deferred(env, j->deferred, e);
        } else {
            napi_resolve_deferred(env, j->deferred, res);
        }
    } else if (j->op == OP_KZG_LOAD) {
        handle_t* h = new_handle(TAG_SRS, j->srs);
        if (!h || napi_create_external(env, h, srs_finalize, NULL, &res) != napi_ok) {      /* nothing would ever free the tables */
            napi_value msg, e;
            L.kzg_srs_free(j->srs);
            free(h);
            napi_create_string_utf8(env, "wsnark_napi: out of memory for the reference string's handle", NAPI_AUTO_LENGTH, &msg);
            napi_create_error(env, NULL, msg, &e);
            napi_reject_deferred(env, j->deferred, e);
        } else {
            napi_resolve_deferred(env, j->deferred, res);
        }
    } else if (j->op == OP_VERIFY || j->op == OP_KZG_VERIFY) {
        napi_get_boolean(env, j->i0 != 0, &res);
        napi_resolve_deferred(env, j->deferred, res);
    } else if (j->op == OP_LOADKEY || j->op == OP_LOADKEY_FILE) {
        napi_create_external(env, new_handle(TAG_KEY, j->key), key_finalize, NULL, &res);
        napi_resolve_deferred(env, j->deferred, res);
    } else if (j->op == OP_LOADKEY_ZKEY || j->op == OP_LOADKEY_ZKEY_FILE) {
        /* an OBJECT as the handle (it carries .vk: js/index.js), the handle_t wrapped inside; zkeyOut: the report, the vk's bytes */
        handle_t* h = new_handle(TAG_KEY, j->key);
        napi_value ab, yes;
        void* dst;
        const napi_property_descriptor mark = {KEY_OBJECT_MARK, NULL, NULL, NULL, NULL, NULL, napi_default, NULL};      /* (read-only, not enumerable) */
        napi_property_descriptor marks[1] = {mark};
        if (!h || napi_create_object(env, &res) != napi_ok || napi_get_boolean(env, true, &yes) != napi_ok || ((marks[0].value = yes), 0) ||
            napi_define_properties(env, res, 1, marks) != napi_ok || napi_wrap(env, res, h, key_finalize, NULL, NULL) != napi_ok) {      /* nothing would ever free the key */
            napi_value msg, e;
            L.pkey_free(j->key);
            free(h);
            napi_create_string_utf8(env, "wsnark_napi: cannot create the key handle", NAPI_AUTO_LENGTH, &msg);
            napi_create_error(env, NULL, msg, &e);
            napi_reject_deferred(env, j->deferred, e);
        } else {
            napi_create_arraybuffer(env, j->nout, &dst, &ab);
            memcpy(dst, j->out, j->nout);
            napi_set_named_property(env, res, "zkeyOut", ab);
            napi_resolve_deferred(env, j->deferred, res);
        }
    } else {
        void* dst;
        napi_create_arraybuffer(env, j->nout, &dst, &res);   /* results are fresh ArrayBuffers, as in the reference */
        memcpy(dst, j->out, j->nout);
        napi_resolve_deferred(env, j->deferred, res);
    }
    for (int i = 0; i < j->nrefs; i++) napi_delete_reference(env, j->refs[i]);
    napi_delete_async_work(env, j->work);
    job_done_with_group(j);
    free(j->path); free(j->path2);
    free(j->out);
    free(j);
}

static napi_value start_job(napi_env env, job_t* j, const char* name) {
    napi_value promise, rname;
    if (!L.h) { job_done_with_group(j); free(j->path); free(j->path2); free(j->out); free(j); napi_throw_error(env, NULL, "wsnark_napi: init() has not been called (use buildBn128())"); return NULL; }
    if (napi_create_promise(env, &j->deferred, &promise) != napi_ok || napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &rname) != napi_ok ||
        napi_create_async_work(env, NULL, rname, job_execute, job_complete, j, &j->work) != napi_ok || napi_queue_async_work(env, j->work) != napi_ok) {
        for (int i = 0; i < j->nrefs; i++) napi_delete_reference(env, j->refs[i]);
        job_done_with_group(j);           /* (never queued: nothing will complete it) */
        free(j->path); free(j->path2); free(j->out); free(j);
        napi_throw_error(env, NULL, "wsnark_napi: cannot queue the call");
        return NULL;
    }
    return promise;
}
static int keep(napi_env env, job_t* j, napi_value v) {   /* inputs stay referenced until completion */
    return napi_create_reference(env, v, 1, &j->refs[j->nrefs++]) == napi_ok;
}
#define FAIL(env, j, msg) do { free((j)->path); free((j)->path2); free((j)->out); free(j); napi_throw_type_error((env), NULL, (msg)); return NULL; } while (0)
static char* get_path(napi_env env, napi_value v) {        /* a JS string -> malloc'ed UTF-8 (NULL if it is not a string) */
    size_t n = 0;
    napi_valuetype t;
    if (napi_typeof(env, v, &t) != napi_ok || t != napi_string || napi_get_value_string_utf8(env, v, NULL, 0, &n) != napi_ok) return NULL;
    char* p = (char*)malloc(n + 1);
    if (p && napi_get_value_string_utf8(env, v, p, n + 1, &n) != napi_ok) { free(p); return NULL; }
    return p;
}

/* g1Multiexp(scalars, points) / g2Multiexp(scalars, points) -> Promise<ArrayBuffer 96/192> */
static napi_value msm_common(napi_env env, napi_callback_info info, int op) {
    size_t argc = 2; napi_value argv[2];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = op; j->nout = op == OP_G1 ? 96 : 192; j->out = (uint8_t*)malloc(j->nout);
    if (argc < 2 || !get_bytes(env, argv[0], &j->a, &j->na) || !get_bytes(env, argv[1], &j->b, &j->nb))
        FAIL(env, j, "expected (scalars, points) byte buffers");
    if (j->nb < (j->na / 32) * (op == OP_G1 ? 64 : 128)) FAIL(env, j, "points buffer too short for the number of scalars");
    keep(env, j, argv[0]); keep(env, j, argv[1]);
    return start_job(env, j, op == OP_G1 ? "wsnark_g1_msm" : "wsnark_g2_msm");
}
static napi_value js_g1(napi_env env, napi_callback_info info) { return msm_common(env, info, OP_G1); }
static napi_value js_g2(napi_env env, napi_callback_info info) { return msm_common(env, info, OP_G2); }

/* fft(buf, odd, inverse) -> Promise<ArrayBuffer> (out of place: the input is left untouched) */
static napi_value js_fft(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_NTT;
    if (argc < 1 || !get_bytes(env, argv[0], &j->a, &j->na)) FAIL(env, j, "expected a byte buffer");
    if (argc > 1) napi_get_value_int32(env, argv[1], &j->i0);
    if (argc > 2) { bool b = false; napi_coerce_to_bool(env, argv[2], &argv[2]); napi_get_value_bool(env, argv[2], &b); j->i1 = b; }
    j->nout = j->na; j->out = (uint8_t*)malloc(j->na ? j->na : 1);
    keep(env, j, argv[0]);
    return start_job(env, j, "wsnark_fr_ntt");
}

/* calcH(signals, polsA, polsB, nSignals, domainSize) -> Promise<ArrayBuffer domain*32> */
static napi_value js_calch(napi_env env, napi_callback_info info) {
    size_t argc = 5; napi_value argv[5];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_CALCH;
    if (argc < 5 || !get_bytes(env, argv[0], &j->a, &j->na) || !get_bytes(env, argv[1], &j->b, &j->nb) ||
        !get_bytes(env, argv[2], &j->c, &j->nc) || napi_get_value_uint32(env, argv[3], &j->u0) != napi_ok ||
        napi_get_value_uint32(env, argv[4], &j->u1) != napi_ok)
        FAIL(env, j, "expected (signals, polsA, polsB, nSignals, domainSize)");
    if (j->na < (size_t)j->u0 * 32) FAIL(env, j, "signals shorter than nSignals*32 bytes");
    j->nout = (size_t)j->u1 * 32; j->out = (uint8_t*)malloc(j->nout ? j->nout : 1);
    keep(env, j, argv[0]); keep(env, j, argv[1]); keep(env, j, argv[2]);
    return start_job(env, j, "wsnark_calc_h");
}

/* loadKey(pkey) -> Promise<external handle>; freed by the GC finalizer */
static napi_value js_loadkey(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_LOADKEY;
    if (argc < 1 || !get_bytes(env, argv[0], &j->a, &j->na)) FAIL(env, j, "expected a proving_key.bin byte buffer");
    keep(env, j, argv[0]);
    return start_job(env, j, "wsnark_pkey_load");
}

/* loadKeyFile(path) -> Promise<key handle>: proving_key.bin or the WSNARK64 container, mapped by the library (wsnark_pkey_load_file):
 * the key never exists as a JS buffer -- how keys beyond one ArrayBuffer (4 GiB file format, 2^24 constraints = 7.8 GB) are loaded */
static napi_value js_loadkey_file(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_LOADKEY_FILE;
    if (argc < 1 || !(j->path = get_path(env, argv[0]))) FAIL(env, j, "expected the path of a key file");
    return start_job(env, j, "wsnark_pkey_load_file");
}
/* loadKeyZkey(zkey bytes) / loadKeyZkeyFile(path) -> Promise<key handle>: a snarkjs .zkey straight into a resident key
 * (wsnark_pkey_load_zkey / _file).  The handle is an object every call that takes loadKey's handle takes; its zkeyOut holds the
 * wsnark_zkey_report_t and the verification key in the verifier's layout (js/index.js turns them into .report and .vk) */
static napi_value js_loadkey_zkey(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_LOADKEY_ZKEY;
    if (argc < 1 || !get_bytes(env, argv[0], &j->a, &j->na)) FAIL(env, j, "expected a .zkey byte buffer");
    keep(env, j, argv[0]);
    return start_job(env, j, "wsnark_pkey_load_zkey");
}
static napi_value js_loadkey_zkey_file(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_LOADKEY_ZKEY_FILE;
    if (argc < 1 || !(j->path = get_path(env, argv[0]))) FAIL(env, j, "expected the path of a .zkey file");
    return start_job(env, j, "wsnark_pkey_load_zkey_file");
}
/* keyFileInfo(path) -> {nVars, nPublic, domainSize, fileBytes, format: "proving_key.bin" | "WSNARK64"} (synchronous: reads the header) */
static napi_value js_keyfile_info(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1], o, v;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (!L.h) { napi_throw_error(env, NULL, "wsnark_napi: init() has not been called (use buildBn128())"); return NULL; }
    char* path = argc >= 1 ? get_path(env, argv[0]) : NULL;
    if (!path) { napi_throw_type_error(env, NULL, "expected the path of a key file"); return NULL; }
    uint32_t nv = 0, np = 0, dom = 0; uint64_t nb = 0; int fmt = 0;
    int rc = L.pkey_file_info(path, &nv, &np, &dom, &nb, &fmt);
    free(path);
    if (rc) {
        char msg[600];
        snprintf(msg, sizeof msg, "wsnark error %d: %s", rc, L.last_error());
        napi_throw_error(env, NULL, msg);
        return NULL;
    }
    napi_create_object(env, &o);
    napi_create_uint32(env, nv, &v); napi_set_named_property(env, o, "nVars", v);
    napi_create_uint32(env, np, &v); napi_set_named_property(env, o, "nPublic", v);
    napi_create_uint32(env, dom, &v); napi_set_named_property(env, o, "domainSize", v);
    napi_create_double(env, (double)nb, &v); napi_set_named_property(env, o, "fileBytes", v);
    napi_create_string_utf8(env, fmt == 2 ? "WSNARK64" : "proving_key.bin", NAPI_AUTO_LENGTH, &v); napi_set_named_property(env, o, "format", v);
    return o;
}

/* hashBytes(buf) -> Promise<ArrayBuffer 16>: digest of the WHOLE buffer, computed off the event loop */
static napi_value js_hash(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_HASH; j->nout = 16; j->out = (uint8_t*)malloc(16);
    if (argc < 1 || !get_bytes(env, argv[0], &j->a, &j->na)) FAIL(env, j, "expected a byte buffer");
    keep(env, j, argv[0]);
    return start_job(env, j, "wsnark_hash_bytes");
}

/* waitTables(keyHandle) -> Promise: resolves once the key's fixed-base table rows are built (wsnark_pkey_wait_tables; proofs before
 * that run on the plain sections) */
static napi_value js_wait_tables(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_WAIT_TABLES; j->nout = 1; j->out = (uint8_t*)calloc(1, 1);
    if (argc < 1 || !(j->key = (wsnark_pkey_t*)get_plain(env, argv[0], TAG_KEY))) FAIL(env, j, "expected a key handle");
    keep(env, j, argv[0]);
    return start_job(env, j, "wsnark_pkey_wait_tables");
}

/* prove(keyHandle, witness, r32|null, s32|null) -> Promise<ArrayBuffer 448>: proof (384 B) | r | s used */
static napi_value js_prove(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_PROVE; j->nout = 448; j->out = (uint8_t*)malloc(448);
    if (argc < 2 || !(j->key = (wsnark_pkey_t*)get_plain(env, argv[0], TAG_KEY)) ||
        !get_bytes(env, argv[1], &j->a, &j->na))
        FAIL(env, j, "expected (keyHandle, witness[, r32, s32])");
    keep(env, j, argv[0]); keep(env, j, argv[1]);
    size_t n;
    napi_valuetype t;
    if (argc > 2 && napi_typeof(env, argv[2], &t) == napi_ok && t != napi_null && t != napi_undefined) {
        if (!get_bytes(env, argv[2], &j->r32, &n) || n != 32) FAIL(env, j, "r must be 32 bytes");
        keep(env, j, argv[2]);
    }
    if (argc > 3 && napi_typeof(env, argv[3], &t) == napi_ok && t != napi_null && t != napi_undefined) {
        if (!get_bytes(env, argv[3], &j->s32, &n) || n != 32) FAIL(env, j, "s must be 32 bytes");
        keep(env, j, argv[3]);
    }
    return start_job(env, j, "wsnark_groth16_prove");
}

/* proveBatch(keyHandle, witnesses (count witnesses back to back, equal lengths), count, r32s|null, s32s|null) ->
 * Promise<ArrayBuffer count x 448 + 64>: the proofs (384 B each), then r | s of every proof as used, then wsnark_prove_batch_report_t
 * (include/wsnark.h, wsnark_groth16_prove_batch) */
#define PROVE_BATCH_REPORT_BYTES 64
static napi_value js_prove_batch(napi_env env, napi_callback_info info) {
    size_t argc = 5; napi_value argv[5];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_PROVE_BATCH;
    if (argc < 3 || !(j->key = (wsnark_pkey_t*)get_plain(env, argv[0], TAG_KEY)) || !get_bytes(env, argv[1], &j->a, &j->na) ||
        napi_get_value_uint32(env, argv[2], &j->u0) != napi_ok || j->u0 == 0 || j->u0 > (1u << 16) || j->na % j->u0)
        FAIL(env, j, "expected (keyHandle, witnesses (count x bytes), count in [1, 2^16][, r32s, s32s])");
    keep(env, j, argv[0]); keep(env, j, argv[1]);
    size_t n;
    napi_valuetype t;
    if (argc > 3 && napi_typeof(env, argv[3], &t) == napi_ok && t != napi_null && t != napi_undefined) {
        if (!get_bytes(env, argv[3], &j->r32, &n) || n != 32 * (size_t)j->u0) FAIL(env, j, "r: 32 bytes per proof");
        keep(env, j, argv[3]);
    }
    if (argc > 4 && napi_typeof(env, argv[4], &t) == napi_ok && t != napi_null && t != napi_undefined) {
        if (!get_bytes(env, argv[4], &j->s32, &n) || n != 32 * (size_t)j->u0) FAIL(env, j, "s: 32 bytes per proof");
        keep(env, j, argv[4]);
    }
    j->nout = 448 * (size_t)j->u0 + PROVE_BATCH_REPORT_BYTES;
    j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    return start_job(env, j, "wsnark_groth16_prove_batch");
}

/* codecPoints(g, compress, bytes, encoding, flags) -> Promise<ArrayBuffer>: the n records (compress: 32 g bytes each, else points of
 * 64 g bytes), then n status bytes (include/wsnark.h: wsnark_g{1,2}_compress / _decompress; on the GPU, needs init()) */
static napi_value js_codec_points(napi_env env, napi_callback_info info) {
    size_t argc = 5; napi_value argv[5];
    bool comp = false;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_CODEC_POINTS;
    if (argc < 5 || napi_get_value_int32(env, argv[0], &j->i0) != napi_ok || (j->i0 != 1 && j->i0 != 2) ||
        napi_get_value_bool(env, argv[1], &comp) != napi_ok || !get_bytes(env, argv[2], &j->a, &j->na) ||
        napi_get_value_uint32(env, argv[3], &j->u0) != napi_ok || napi_get_value_uint32(env, argv[4], &j->u1) != napi_ok ||
        j->na == 0 || j->na % ((comp ? 64 : 32) * (size_t)j->i0))
        FAIL(env, j, "expected (g = 1 | 2, compress, bytes (a whole number of records), encoding, flags)");
    j->i1 = comp ? 1 : 0;
    const size_t n = j->na / ((comp ? 64 : 32) * (size_t)j->i0);
    j->nout = n * (comp ? 32 : 64) * (size_t)j->i0 + n;
    j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    keep(env, j, argv[2]);
    return start_job(env, j, "wsnark_points_codec");
}
/* codecProofs(compress, bytes, encoding) -> Promise<ArrayBuffer>: the n records (128 or 384 bytes each), then n status bytes */
static napi_value js_codec_proofs(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    bool comp = false;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_CODEC_PROOFS;
    if (argc < 3 || napi_get_value_bool(env, argv[0], &comp) != napi_ok || !get_bytes(env, argv[1], &j->a, &j->na) ||
        napi_get_value_uint32(env, argv[2], &j->u0) != napi_ok || j->na == 0 || j->na % (comp ? 384 : 128))
        FAIL(env, j, "expected (compress, bytes (a whole number of proofs), encoding)");
    j->i1 = comp ? 1 : 0;
    const size_t n = j->na / (comp ? 384 : 128);
    j->nout = n * (comp ? 128 : 384) + n;
    j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    keep(env, j, argv[1]);
    return start_job(env, j, "wsnark_proofs_codec");
}
/* verifyBatchCompressed(vkBytes, inputBytes (count x nInputs x 32), proofs (count x 128), nInputs, encoding) -> Promise<ArrayBuffer count> */
static napi_value js_verify_batch_compressed(napi_env env, napi_callback_info info) {
    size_t argc = 5; napi_value argv[5];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_VERIFY_BATCH_COMPRESSED;
    if (argc < 5 || !get_bytes(env, argv[0], &j->a, &j->na) || !get_bytes(env, argv[1], &j->b, &j->nb) ||
        !get_bytes(env, argv[2], &j->c, &j->nc) || napi_get_value_uint32(env, argv[3], &j->u0) != napi_ok ||
        napi_get_value_uint32(env, argv[4], &j->u1) != napi_ok || j->nc == 0 || j->nc % 128 || j->nb != (j->nc / 128) * (size_t)j->u0 * 32)
        FAIL(env, j, "expected (vkBytes, inputBytes (count x nInputs x 32), proofs (count x 128), nInputs, encoding)");
    j->nout = j->nc / 128;
    j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    keep(env, j, argv[0]); keep(env, j, argv[1]); keep(env, j, argv[2]);
    return start_job(env, j, "wsnark_groth16_verify_batch_compressed");
}

/* verify(vkBytes, inputBytes, proof384) -> Promise<boolean>   (layouts: include/wsnark.h, wsnark_groth16_verify) */
static napi_value js_verify(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_VERIFY;
    if (argc < 3 || !get_bytes(env, argv[0], &j->a, &j->na) || !get_bytes(env, argv[1], &j->b, &j->nb) ||
        !get_bytes(env, argv[2], &j->c, &j->nc) || j->nc != 384 || j->nb % 32)
        FAIL(env, j, "expected (vkBytes, inputBytes (n x 32), proof384)");
    keep(env, j, argv[0]); keep(env, j, argv[1]); keep(env, j, argv[2]);
    return start_job(env, j, "wsnark_groth16_verify");
}

/* verifyBatch(vkBytes, inputBytes (count x nInputs x 32), proofs (count x 384), nInputs) -> Promise<ArrayBuffer count>: one status
 * byte per proof, 1 valid / 0 invalid / 2 malformed (include/wsnark.h, wsnark_groth16_verify_batch: on the GPU, needs init()) */
static napi_value js_verify_batch(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_VERIFY_BATCH;
    if (argc < 4 || !get_bytes(env, argv[0], &j->a, &j->na) || !get_bytes(env, argv[1], &j->b, &j->nb) ||
        !get_bytes(env, argv[2], &j->c, &j->nc) || napi_get_value_uint32(env, argv[3], &j->u0) != napi_ok ||
        j->nc == 0 || j->nc % 384 || j->nb != (j->nc / 384) * (size_t)j->u0 * 32)
        FAIL(env, j, "expected (vkBytes, inputBytes (count x nInputs x 32), proofs (count x 384), nInputs)");
    j->nout = j->nc / 384;
    j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    keep(env, j, argv[0]); keep(env, j, argv[1]); keep(env, j, argv[2]);
    return start_job(env, j, "wsnark_groth16_verify_batch");
}

/* checkKey(pkeyBytes | path, flags, seed32 | null) -> Promise<ArrayBuffer 248>: the wsnark_pkey_report_t of the audit (include/wsnark.h:
 * wsnark_pkey_check / wsnark_pkey_check_file; index.js turns it into an object).  flags: 1 points, 2 relations, 0 both. */
#define PKEY_REPORT_BYTES 248
static napi_value js_check_key(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_CHECK_KEY;
    if (argc < 2 || (!(j->path = get_path(env, argv[0])) && !get_bytes(env, argv[0], &j->a, &j->na)) ||
        napi_get_value_uint32(env, argv[1], &j->u0) != napi_ok)
        FAIL(env, j, "expected (proving_key.bin bytes | key file path, flags[, seed32])");
    size_t ns = 0;
    if (argc > 2 && get_bytes(env, argv[2], &j->r32, &ns) && ns != 32) FAIL(env, j, "the seed must be 32 bytes");
    j->nout = PKEY_REPORT_BYTES;
    j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    if (!j->path) keep(env, j, argv[0]);
    if (j->r32) keep(env, j, argv[2]);
    return start_job(env, j, "wsnark_pkey_check");
}

/* contributeKey(pkeyBytes | inPath, outPath | null, d32 | null) -> Promise<ArrayBuffer>: the wsnark_pkey_delta_report_t (104 bytes) and,
 * for key bytes, the new key behind it (wsnark_pkey_contribute / _contribute_file).  d32 == null: the library draws d and wipes it. */
static napi_value js_contribute_key(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_CONTRIBUTE;
    if (argc < 1 || (!(j->path = get_path(env, argv[0])) && !get_bytes(env, argv[0], &j->a, &j->na)))
        FAIL(env, j, "expected (proving_key.bin bytes | key file path, outPath | null[, d32])");
    if (j->path && (argc < 2 || !(j->path2 = get_path(env, argv[1])))) FAIL(env, j, "a key file needs the path of the new file");
    size_t ns = 0;
    if (argc > 2 && get_bytes(env, argv[2], &j->r32, &ns) && ns != 32) FAIL(env, j, "the entropy must be 32 bytes");
    j->nout = PKEY_DELTA_REPORT_BYTES + (j->path ? 0 : j->na);
    j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    if (!j->path) keep(env, j, argv[0]);
    if (j->r32) keep(env, j, argv[2]);
    return start_job(env, j, "wsnark_pkey_contribute");
}
/* deltaVerify(oldBytes | oldPath, newBytes | newPath, seed32 | null) -> Promise<ArrayBuffer 40>: the wsnark_pkey_delta_verdict_t */
static napi_value js_delta_verify(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_DELTA_VERIFY;
    if (argc < 2) FAIL(env, j, "expected (old key, new key[, seed32])");
    j->path = get_path(env, argv[0]);
    if (j->path ? !(j->path2 = get_path(env, argv[1])) : (!get_bytes(env, argv[0], &j->a, &j->na) || !get_bytes(env, argv[1], &j->b, &j->nb)))
        FAIL(env, j, "expected two key byte buffers or two key file paths");
    size_t ns = 0;
    if (argc > 2 && get_bytes(env, argv[2], &j->r32, &ns) && ns != 32) FAIL(env, j, "the seed must be 32 bytes");
    j->nout = PKEY_DELTA_VERDICT_BYTES;
    j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    if (!j->path) { keep(env, j, argv[0]); keep(env, j, argv[1]); }
    if (j->r32) keep(env, j, argv[2]);
    return start_job(env, j, "wsnark_pkey_delta_verify");
}

/* groupNtt(group 1 | 2, points, inverse) -> Promise<ArrayBuffer>: the transform over group elements (wsnark_g{1,2}_ntt), out of place */
static napi_value js_group_ntt(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_GROUP_NTT;
    if (argc < 2 || napi_get_value_int32(env, argv[0], &j->i0) != napi_ok || (j->i0 != 1 && j->i0 != 2) || !get_bytes(env, argv[1], &j->a, &j->na) ||
        j->na % (j->i0 == 2 ? 128 : 64))
        FAIL(env, j, "expected (group 1 | 2, a whole number of affine points[, inverse])");
    if (argc > 2) { bool b = false; napi_coerce_to_bool(env, argv[2], &argv[2]); napi_get_value_bool(env, argv[2], &b); j->i1 = b; }
    j->nout = j->na; j->out = (uint8_t*)calloc(j->na ? j->na : 1, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    keep(env, j, argv[1]);
    return start_job(env, j, "wsnark_group_ntt");
}
/* zkeyInfo(zkey) -> ArrayBuffer 56: the wsnark_zkey_info_t of a .zkey (host work only, synchronous) */
static napi_value js_zkey_info(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1], res;
    uint8_t* p; size_t n;
    void* dst;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (!L.h) { napi_throw_error(env, NULL, "wsnark_napi: init() has not been called (use buildBn128())"); return NULL; }
    if (argc < 1 || !get_bytes(env, argv[0], &p, &n)) { napi_throw_type_error(env, NULL, "expected (zkey bytes)"); return NULL; }
    uint8_t out[ZKEY_INFO_BYTES];
    const int rc = L.zkey_info(p, n, out);
    if (rc) {
        char msg[600];
        snprintf(msg, sizeof msg, "wsnark error %d: %s", rc, L.last_error());
        napi_throw_error(env, NULL, msg);
        return NULL;
    }
    CHECK(env, napi_create_arraybuffer(env, sizeof out, &dst, &res));
    memcpy(dst, out, sizeof out);
    return res;
}
/* importZkey(zkey) -> Promise<ArrayBuffer>: u64 key length, u64 vk length, the wsnark_zkey_report_t, the vk (the verifier's plain
 * layout), proving_key.bin (wsnark_zkey_import) */
static napi_value js_import_zkey(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_ZKEY_IMPORT;
    if (argc < 1 || !get_bytes(env, argv[0], &j->a, &j->na)) FAIL(env, j, "expected (zkey bytes)");
    keep(env, j, argv[0]);
    return start_job(env, j, "wsnark_zkey_import");
}
/* exportZkey(pkey, vk bytes, nPublic) -> Promise<ArrayBuffer>: u64 file length, u64 0, the wsnark_zkey_report_t, the .zkey (wsnark_zkey_export) */
static napi_value js_export_zkey(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_ZKEY_EXPORT;
    if (argc < 3 || !get_bytes(env, argv[0], &j->a, &j->na) || !get_bytes(env, argv[1], &j->b, &j->nb) || napi_get_value_uint32(env, argv[2], &j->u0) != napi_ok)
        FAIL(env, j, "expected (proving_key.bin bytes, verification key bytes, nPublic)");
    keep(env, j, argv[0]); keep(env, j, argv[1]);
    return start_job(env, j, "wsnark_zkey_export");
}
/* newKey(nVars, nPublic, domain, [tauG1, tauG2, alphaTauG1, betaTauG1, betaG2, polsA, polsB, polsC]) -> Promise<ArrayBuffer>: the
 * wsnark_pkey_setup_report_t (192 bytes), the nPublic + 1 IC points, then proving_key.bin (wsnark_pkey_setup_pkey) */
static napi_value js_new_key(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4], el;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (!L.h) { napi_throw_error(env, NULL, "wsnark_napi: init() has not been called (use buildBn128())"); return NULL; }
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_NEW_KEY;
    bool is = false;
    if (argc < 4 || napi_get_value_uint32(env, argv[0], &j->u0) != napi_ok || napi_get_value_uint32(env, argv[1], &j->u1) != napi_ok ||
        napi_get_value_uint32(env, argv[2], &j->u2) != napi_ok || napi_is_array(env, argv[3], &is) != napi_ok || !is)
        FAIL(env, j, "expected (nVars, nPublic, domain, [eight byte buffers])");
    for (uint32_t k = 0; k < 8; k++)
        if (napi_get_element(env, argv[3], k, &el) != napi_ok || !get_bytes(env, el, &j->in[k], &j->nin[k])) FAIL(env, j, "newKey: eight byte buffers");
    if (j->nin[4] < 128) FAIL(env, j, "betaG2 must be 128 bytes");
    powers_t P;
    circuit_t K;
    size_t len = 0;
    job_structs(j, &P, &K);
    if (L.pkey_setup_size(&K, &len)) {
        char msg[600];
        snprintf(msg, sizeof msg, "wsnark error: %s", L.last_error());
        free(j);
        napi_throw_error(env, NULL, msg);
        return NULL;
    }
    j->nout = PKEY_SETUP_REPORT_BYTES + ((size_t)j->u1 + 1) * 64 + len;
    j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    keep(env, j, argv[3]);      /* the array keeps its eight buffers alive */
    return start_job(env, j, "wsnark_pkey_setup");
}

/* checkKeyCircuit(pkeyBytes | path, nVars, nPublic, domain, [tauG1, tauG2, alphaTauG1, betaTauG1, betaG2, polsA, polsB, polsC], vkBytes | null,
 * seed32 | null) -> Promise<ArrayBuffer 56>: the wsnark_pkey_circuit_verdict_t (wsnark_pkey_circuit_check / _check_file; index.js turns
 * it into an object).  vkBytes: wsnark_groth16_verify's layout with all the key's IC points. */
static napi_value js_check_key_circuit(napi_env env, napi_callback_info info) {
    size_t argc = 7; napi_value argv[7], el;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_CHECK_KEY_CIRCUIT;
    bool is = false;
    if (argc < 5 || (!(j->path = get_path(env, argv[0])) && !get_bytes(env, argv[0], &j->a, &j->na)) ||
        napi_get_value_uint32(env, argv[1], &j->u0) != napi_ok || napi_get_value_uint32(env, argv[2], &j->u1) != napi_ok ||
        napi_get_value_uint32(env, argv[3], &j->u2) != napi_ok || napi_is_array(env, argv[4], &is) != napi_ok || !is)
        FAIL(env, j, "expected (proving_key.bin bytes | key file path, nVars, nPublic, domain, [eight byte buffers][, vkBytes, seed32])");
    for (uint32_t k = 0; k < 8; k++)
        if (napi_get_element(env, argv[4], k, &el) != napi_ok || !get_bytes(env, el, &j->in[k], &j->nin[k])) FAIL(env, j, "checkKeyCircuit: eight byte buffers");
    if (j->nin[4] < 128) FAIL(env, j, "betaG2 must be 128 bytes");
    if (argc > 5 && get_bytes(env, argv[5], &j->b, &j->nb) && (j->nb < 448 + 64 || (j->nb - 448) % 64)) FAIL(env, j, "vkBytes: alfa1 | beta2 | gamma2 | delta2 | IC points");
    size_t ns = 0;
    if (argc > 6 && get_bytes(env, argv[6], &j->r32, &ns) && ns != 32) FAIL(env, j, "the seed must be 32 bytes");
    j->nout = PKEY_CIRCUIT_VERDICT_BYTES;
    j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    if (!j->path) keep(env, j, argv[0]);
    keep(env, j, argv[4]);      /* the array keeps its eight buffers alive */
    if (j->b) keep(env, j, argv[5]);
    if (j->r32) keep(env, j, argv[6]);
    return start_job(env, j, "wsnark_pkey_circuit_check");
}

/* ---- a witness against its circuit (include/wsnark.h: wsnark_circuit_load, wsnark_witness_check, wsnark_circuit_witness_check) ----
 * the circuit's (nVars, nPublic, domain, [polsA, polsB, polsC]) into u0, u1, u2 and in[5..7], where job_structs reads them */
static int circuit_args(napi_env env, job_t* j, napi_value* argv) {
    napi_value el;
    bool is = false;
    if (napi_get_value_uint32(env, argv[0], &j->u0) != napi_ok || napi_get_value_uint32(env, argv[1], &j->u1) != napi_ok ||
        napi_get_value_uint32(env, argv[2], &j->u2) != napi_ok || napi_is_array(env, argv[3], &is) != napi_ok || !is)
        return 0;
    for (uint32_t k = 0; k < 3; k++)
        if (napi_get_element(env, argv[3], k, &el) != napi_ok || !get_bytes(env, el, &j->in[5 + k], &j->nin[5 + k])) return 0;
    return 1;
}
/* the report and the two lists of `cap` entries behind it; 0 if cap is no count in [0, 2^24] */
static int witness_out(napi_env env, job_t* j, napi_value cap) {
    uint32_t n = 0;
    if (napi_get_value_uint32(env, cap, &n) != napi_ok || n > (1u << 24)) return 0;
    j->cap = n;
    j->nout = WITNESS_REPORT_BYTES + (size_t)n * (8 + 96);
    j->out = (uint8_t*)calloc(j->nout, 1);
    return j->out != NULL;
}
/* loadCircuit(nVars, nPublic, domain, [polsA, polsB, polsC]) -> Promise<handle> */
static napi_value js_circuit_load(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_CIRCUIT_LOAD;
    if (argc < 4 || !circuit_args(env, j, argv)) FAIL(env, j, "expected (nVars, nPublic, domain, [polsA, polsB, polsC])");
    keep(env, j, argv[3]);      /* the array keeps its three buffers alive */
    return start_job(env, j, "wsnark_circuit_load");
}
/* ---- a circuit in row form (include/wsnark.h: wsnark_circuit_from_rows, wsnark_circuit_load_rows) ----
 * (nVars, nPublic, nConstraints, domain, flags, [rowPtrA, colA, coefA, rowPtrB, ..., coefC]); the library has only the pointers, so
 * the arrays' lengths are checked here: row_ptr nConstraints + 1 u64, col row_ptr[nConstraints] u32, coef as many x 32 bytes */
static int rows_args(napi_env env, job_t* j, napi_value* argv) {
    napi_value el;
    bool is = false;
    uint32_t nc = 0, flags = 0;
    if (napi_get_value_uint32(env, argv[0], &j->u0) != napi_ok || napi_get_value_uint32(env, argv[1], &j->u1) != napi_ok ||
        napi_get_value_uint32(env, argv[2], &nc) != napi_ok || nc > 0x7fffffffu || napi_get_value_uint32(env, argv[3], &j->u2) != napi_ok ||
        napi_get_value_uint32(env, argv[4], &flags) != napi_ok || flags > 0x7fffffffu || napi_is_array(env, argv[5], &is) != napi_ok || !is)
        return 0;
    j->i0 = (int)nc; j->i1 = (int)flags;
    for (uint32_t k = 0; k < 9; k++)
        if (napi_get_element(env, argv[5], k, &el) != napi_ok || !get_bytes(env, el, &j->in[k], &j->nin[k])) return 0;
    for (uint32_t m = 0; m < 3; m++) {
        uint64_t nnz;
        if (j->nin[3 * m] != 8 * ((size_t)nc + 1) || ((uintptr_t)j->in[3 * m] & 7) || ((uintptr_t)j->in[3 * m + 1] & 3)) return 0;
        memcpy(&nnz, j->in[3 * m] + 8 * (size_t)nc, 8);
        if (nnz > ((uint64_t)1 << 32) || j->nin[3 * m + 1] != 4 * nnz || j->nin[3 * m + 2] != 32 * nnz) return 0;
    }
    return 1;
}
#define ROWS_ARGS_TEXT "expected (nVars, nPublic, nConstraints, domain, flags, [rowPtr, col, coef] x 3: u64 x (nConstraints + 1), u32 and 32 bytes per entry)"
/* circuitFromRows(...) -> Promise<ArrayBuffer>: u32 domain, u32 0, lens[3] (u64), the wsnark_rows_report_t, polsA | polsB | polsC */
static napi_value js_circuit_from_rows(napi_env env, napi_callback_info info) {
    size_t argc = 6; napi_value argv[6];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_CIRCUIT_FROM_ROWS;
    if (argc < 6 || !rows_args(env, j, argv)) FAIL(env, j, ROWS_ARGS_TEXT);
    keep(env, j, argv[5]);      /* the array keeps its nine buffers alive */
    return start_job(env, j, "wsnark_circuit_from_rows");
}
/* loadCircuitRows(...) -> Promise<handle>: loadCircuit's handle (wsnark_circuit_load_rows) */
static napi_value js_circuit_load_rows(napi_env env, napi_callback_info info) {
    size_t argc = 6; napi_value argv[6];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_CIRCUIT_LOAD_ROWS;
    if (argc < 6 || !rows_args(env, j, argv)) FAIL(env, j, ROWS_ARGS_TEXT);
    keep(env, j, argv[5]);
    return start_job(env, j, "wsnark_circuit_load_rows");
}
/* circuitInfo(handle) -> {nVars, nPublic, domain, nnz: [A, B, C], bytes} */
static napi_value js_circuit_info(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1], o, v, a;
    wsnark_circuit_res_t* c = NULL;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1 || !(c = (wsnark_circuit_res_t*)get_plain(env, argv[0], TAG_CIRCUIT))) { napi_throw_type_error(env, NULL, "expected a circuit handle"); return NULL; }
    uint32_t nv = 0, np = 0, dom = 0;
    uint64_t nnz[3] = {0, 0, 0}, bytes = 0;
    L.circuit_info(c, &nv, &np, &dom, nnz, &bytes);
    napi_create_object(env, &o);
    napi_create_uint32(env, nv, &v); napi_set_named_property(env, o, "nVars", v);
    napi_create_uint32(env, np, &v); napi_set_named_property(env, o, "nPublic", v);
    napi_create_uint32(env, dom, &v); napi_set_named_property(env, o, "domain", v);
    napi_create_array_with_length(env, 3, &a);
    for (uint32_t k = 0; k < 3; k++) { napi_create_double(env, (double)nnz[k], &v); napi_set_element(env, a, k, v); }
    napi_set_named_property(env, o, "nnz", a);
    napi_create_double(env, (double)bytes, &v); napi_set_named_property(env, o, "bytes", v);
    return o;
}
/* circuitFree(handle): the matrices go back now instead of with the garbage collector; the handle is dead afterwards (index.js calls
 * this only when no check on the handle is in flight) */
static napi_value js_circuit_free(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    handle_t* h = argc < 1 ? NULL : (handle_t*)get_handle(env, argv[0], TAG_CIRCUIT);
    if (h && h->p) { L.circuit_free((wsnark_circuit_res_t*)h->p); h->p = NULL; }
    return NULL;
}
/* circuitCheckWitness(handle, witness, cap) -> Promise<ArrayBuffer 80 + cap x 104>: the wsnark_witness_report_t, cap row indices (u64),
 * cap x (a | b | c) */
static napi_value js_circuit_check_witness(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_CIRCUIT_WITNESS_CHECK;
    if (argc < 3 || !(j->circ = (wsnark_circuit_res_t*)get_plain(env, argv[0], TAG_CIRCUIT)) || !get_bytes(env, argv[1], &j->a, &j->na))
        FAIL(env, j, "expected (circuit handle, witness, maxRows)");
    if (!witness_out(env, j, argv[2])) FAIL(env, j, "maxRows: a count of at most 2^24");
    keep(env, j, argv[0]); keep(env, j, argv[1]);
    return start_job(env, j, "wsnark_circuit_witness_check");
}
/* circuitCheckWitnesses(handle, witnesses (count witnesses back to back, equal lengths), count, cap) -> Promise<ArrayBuffer 64 + count x
 * (48 + cap x 104)>: the wsnark_witness_batch_report_t, the verdicts, count x cap row indices (u64), count x cap x (a | b | c)
 * (include/wsnark.h, wsnark_circuit_witness_check_batch) */
static napi_value js_circuit_check_witnesses(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_CIRCUIT_WITNESS_CHECK_BATCH;
    uint32_t cap = 0;
    if (argc < 4 || !(j->circ = (wsnark_circuit_res_t*)get_plain(env, argv[0], TAG_CIRCUIT)) || !get_bytes(env, argv[1], &j->a, &j->na) ||
        napi_get_value_uint32(env, argv[2], &j->u0) != napi_ok || j->u0 == 0 || j->u0 > (1u << 16) || j->na % j->u0)
        FAIL(env, j, "expected (circuit handle, witnesses (count x bytes), count in [1, 2^16], maxRows)");
    if (napi_get_value_uint32(env, argv[3], &cap) != napi_ok || cap > (1u << 24)) FAIL(env, j, "maxRows: a count of at most 2^24");
    j->cap = cap;
    j->nout = WITNESS_BATCH_REPORT_BYTES + (size_t)j->u0 * (WITNESS_VERDICT_BYTES + (size_t)cap * (8 + 96));
    j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    keep(env, j, argv[0]); keep(env, j, argv[1]);
    return start_job(env, j, "wsnark_circuit_witness_check_batch");
}
/* checkWitness(nVars, nPublic, domain, [polsA, polsB, polsC], witness, cap) -> Promise<ArrayBuffer>: the same, load and free included */
static napi_value js_check_witness(napi_env env, napi_callback_info info) {
    size_t argc = 6; napi_value argv[6];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_WITNESS_CHECK;
    if (argc < 6 || !circuit_args(env, j, argv) || !get_bytes(env, argv[4], &j->a, &j->na))
        FAIL(env, j, "expected (nVars, nPublic, domain, [polsA, polsB, polsC], witness, maxRows)");
    if (!witness_out(env, j, argv[5])) FAIL(env, j, "maxRows: a count of at most 2^24");
    keep(env, j, argv[3]); keep(env, j, argv[4]);
    return start_job(env, j, "wsnark_witness_check");
}

/* mulPoints(group 1 | 2, points, scalars) -> Promise<ArrayBuffer>: scalars[i] * points[i] (wsnark_g{1,2}_mul_batch), out of place */
static napi_value js_mul_points(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_MUL_POINTS;
    if (argc < 3 || napi_get_value_int32(env, argv[0], &j->i0) != napi_ok || (j->i0 != 1 && j->i0 != 2) || !get_bytes(env, argv[1], &j->a, &j->na) ||
        !get_bytes(env, argv[2], &j->b, &j->nb) || j->na % (j->i0 == 2 ? 128 : 64) || j->nb % 32 || j->na / (j->i0 == 2 ? 128 : 64) != j->nb / 32)
        FAIL(env, j, "expected (group 1 | 2, a whole number of affine points, as many 32-byte scalars)");
    j->nout = j->na; j->out = (uint8_t*)calloc(j->na ? j->na : 1, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    keep(env, j, argv[1]); keep(env, j, argv[2]);
    return start_job(env, j, "wsnark_mul_batch");
}
/* the five buffers of a transcript (tauG1, tauG2, alphaTauG1, betaTauG1, betaG2) into j->in[0..4], the domain into j->u2 */
static int get_powers(napi_env env, napi_value domain, napi_value arr, job_t* j) {
    bool is = false;
    napi_value el;
    if (napi_get_value_uint32(env, domain, &j->u2) != napi_ok || napi_is_array(env, arr, &is) != napi_ok || !is) return 0;
    for (uint32_t k = 0; k < 5; k++)
        if (napi_get_element(env, arr, k, &el) != napi_ok || !get_bytes(env, el, &j->in[k], &j->nin[k])) return 0;
    return j->nin[4] >= 128;
}
/* contributePowers(domain, [tauG1, tauG2, alphaTauG1, betaTauG1, betaG2], [tau32 | null, alpha32 | null, beta32 | null]) ->
 * Promise<ArrayBuffer>: the wsnark_powers_report_t (192 bytes), then the five parts of the new transcript in that order
 * (wsnark_powers_contribute).  A null secret is drawn by the library and wiped. */
static napi_value js_contribute_powers(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3], el;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_POWERS_CONTRIBUTE;
    bool is = false;
    if (argc < 3 || !get_powers(env, argv[0], argv[1], j) || napi_is_array(env, argv[2], &is) != napi_ok || !is)
        FAIL(env, j, "expected (domain, [five byte buffers, betaG2 of 128 bytes], [three secrets of 32 bytes or null])");
    uint8_t** secret[3] = {&j->r32, &j->s32, &j->c};
    for (uint32_t k = 0; k < 3; k++) {
        size_t ns = 0;
        if (napi_get_element(env, argv[2], k, &el) == napi_ok && get_bytes(env, el, secret[k], &ns) && ns != 32) FAIL(env, j, "a secret must be 32 bytes");
    }
    const uint32_t n = j->u2;
    j->u1 = (n >= 2 && !(n & (n - 1)) && n <= (1u << 24)) ? n : 0;      /* any other domain is rejected before a byte is written */
    j->nout = POWERS_REPORT_BYTES + (size_t)j->u1 * 384 + 128;
    j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    keep(env, j, argv[1]); keep(env, j, argv[2]);      /* the arrays keep their buffers alive */
    return start_job(env, j, "wsnark_powers_contribute");
}
/* checkPowers(domain, [tauG1, tauG2, alphaTauG1, betaTauG1, betaG2], flags, seed32 | null) -> Promise<ArrayBuffer 192>: the
 * wsnark_powers_report_t of the audit (wsnark_powers_check).  flags: 1 points, 2 relations, 0 both. */
static napi_value js_check_powers(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_POWERS_CHECK;
    if (argc < 3 || !get_powers(env, argv[0], argv[1], j) || napi_get_value_uint32(env, argv[2], &j->u0) != napi_ok)
        FAIL(env, j, "expected (domain, [five byte buffers, betaG2 of 128 bytes], flags[, seed32])");
    size_t ns = 0;
    if (argc > 3 && get_bytes(env, argv[3], &j->r32, &ns) && ns != 32) FAIL(env, j, "the seed must be 32 bytes");
    j->nout = POWERS_REPORT_BYTES;
    j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    keep(env, j, argv[1]);
    if (j->r32) keep(env, j, argv[3]);
    return start_job(env, j, "wsnark_powers_check");
}

/* allocPinned(bytes) -> ArrayBuffer over pinned host memory (wsnark_host_alloc): a witness written into it is DMA'd in place,
 * without the staging copy.  Freed by the GC finalizer. */
static void pinned_finalize(napi_env env, void* data, void* hint) {
    (void)env; (void)hint;
    if (data && L.host_free) L.host_free(data);
}
static napi_value js_alloc_pinned(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1], ab;
    double nbytes = 0;
    void* p = NULL;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (!L.h) { napi_throw_error(env, NULL, "wsnark_napi: init() has not been called (use buildBn128())"); return NULL; }
    if (argc < 1 || napi_get_value_double(env, argv[0], &nbytes) != napi_ok || nbytes < 0 || nbytes > 1e12) { napi_throw_type_error(env, NULL, "expected a byte count"); return NULL; }
    int rc = L.host_alloc((size_t)nbytes, &p);
    if (rc || !p) {
        char msg[600];
        snprintf(msg, sizeof msg, "wsnark_host_alloc failed (%d): %s", rc, L.last_error());
        napi_throw_error(env, NULL, msg);
        return NULL;
    }
    if (napi_create_external_arraybuffer(env, p, (size_t)nbytes, pinned_finalize, NULL, &ab) != napi_ok) {
        L.host_free(p);
        napi_throw_error(env, NULL, "wsnark_napi: cannot wrap the pinned buffer");
        return NULL;
    }
    return ab;
}

static napi_value js_keyinfo(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1], o, v;
    wsnark_pkey_t* k = NULL;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1 || !(k = (wsnark_pkey_t*)get_plain(env, argv[0], TAG_KEY))) { napi_throw_type_error(env, NULL, "expected a key handle"); return NULL; }
    uint32_t nv, np, dom;
    L.pkey_info(k, &nv, &np, &dom);
    napi_create_object(env, &o);
    napi_create_uint32(env, nv, &v); napi_set_named_property(env, o, "nVars", v);
    napi_create_uint32(env, np, &v); napi_set_named_property(env, o, "nPublic", v);
    napi_create_uint32(env, dom, &v); napi_set_named_property(env, o, "domainSize", v);
    /* what the load took, phase by phase (wsnark_pkey_load_stats; tableBuild stays 0 until the background build has finished) */
    double ms[5] = {0, 0, 0, 0, 0};
    if (L.pkey_load_stats(k, ms) == 0) {
        static const char* names[5] = {"polsToCsr", "pointsH2d", "masksConvert", "tableBuild", "total"};
        napi_value lo;
        napi_create_object(env, &lo);
        for (int i = 0; i < 5; i++) { napi_create_double(env, ms[i], &v); napi_set_named_property(env, lo, names[i], v); }
        napi_set_named_property(env, o, "loadMs", lo);
    }
    return o;
}

/* ---- resident bases ----
 * loadPoints(group 1|2, points) -> Promise<handle>: the set resident as fixed-base window tables (wsnark_points_load) */
static napi_value js_points_load(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_POINTS_LOAD;
    if (argc < 2 || napi_get_value_int32(env, argv[0], &j->i0) != napi_ok || (j->i0 != 1 && j->i0 != 2) || !get_bytes(env, argv[1], &j->a, &j->na) ||
        j->na == 0 || j->na % (j->i0 == 2 ? 128 : 64))
        FAIL(env, j, "expected (1 | 2, a whole number of affine points)");
    keep(env, j, argv[1]);
    return start_job(env, j, "wsnark_points_load");
}
/* pointsMultiexp(handle, scalars) -> Promise<ArrayBuffer 96/192> */
static napi_value js_points_msm(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    int g = 0;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_POINTS_MSM;
    if (argc < 2 || !(j->pts = (wsnark_points_t*)get_plain(env, argv[0], TAG_POINTS)) || !get_bytes(env, argv[1], &j->a, &j->na))
        FAIL(env, j, "expected (points handle, scalars)");
    L.points_info(j->pts, &g, NULL, NULL, NULL, NULL);
    j->nout = g == 2 ? 192 : 96; j->out = (uint8_t*)malloc(j->nout);
    keep(env, j, argv[0]); keep(env, j, argv[1]);
    return start_job(env, j, "wsnark_points_msm");
}

/* ---- KZG on powers of tau ----
 * a 32-byte scalar argument; null / undefined where the call allows it */
static int get_scalar32(napi_env env, napi_value v, int optional, uint8_t** p) {
    napi_valuetype t;
    size_t n = 0;
    *p = NULL;
    if (optional && napi_typeof(env, v, &t) == napi_ok && (t == napi_null || t == napi_undefined)) return 1;
    return get_bytes(env, v, p, &n) && n == 32;
}
/* kzgLoadSrs(tauG1) -> Promise<handle> */
static napi_value js_kzg_load(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_KZG_LOAD;
    if (argc < 1 || !get_bytes(env, argv[0], &j->a, &j->na) || j->na == 0 || j->na % 64) FAIL(env, j, "expected (a whole number of 64-byte G1 points)");
    keep(env, j, argv[0]);
    return start_job(env, j, "wsnark_kzg_srs_load");
}
/* (polys, len) of kzgCommit / kzgOpen / polyEval: count x len coefficients of 32 bytes */
static int get_polys(napi_env env, napi_value polys, napi_value len, job_t* j) {
    return get_bytes(env, polys, &j->a, &j->na) && napi_get_value_uint32(env, len, &j->u0) == napi_ok && j->u0 != 0 && j->na != 0 &&
           j->na % ((size_t)32 * j->u0) == 0;
}
/* kzgCommit(handle, polys, len, form 0 | 1) -> Promise<ArrayBuffer count x 64> */
static napi_value js_kzg_commit(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_KZG_COMMIT;
    if (argc < 4 || !(j->srs = (wsnark_kzg_srs_t*)get_plain(env, argv[0], TAG_SRS)) || !get_polys(env, argv[1], argv[2], j) ||
        napi_get_value_int32(env, argv[3], &j->i0) != napi_ok)
        FAIL(env, j, "expected (reference string handle, count x len 32-byte coefficients, len, form 0 | 1)");
    j->nout = j->na / 32 / j->u0 * 64; j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    keep(env, j, argv[0]); keep(env, j, argv[1]);
    return start_job(env, j, "wsnark_kzg_commit");
}
/* kzgOpen(handle, polys, len, z32, gamma32 | null) -> Promise<ArrayBuffer count x 32 values | the 64-byte proof> */
static napi_value js_kzg_open(napi_env env, napi_callback_info info) {
    size_t argc = 5; napi_value argv[5];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_KZG_OPEN;
    if (argc < 5 || !(j->srs = (wsnark_kzg_srs_t*)get_plain(env, argv[0], TAG_SRS)) || !get_polys(env, argv[1], argv[2], j) ||
        !get_scalar32(env, argv[3], 0, &j->r32) || !get_scalar32(env, argv[4], 1, &j->s32) || (!j->s32 && j->na / 32 / j->u0 > 1))
        FAIL(env, j, "expected (reference string handle, count x len 32-byte coefficients, len, z (32 bytes), gamma (32 bytes; null for one polynomial))");
    j->nout = j->na / 32 / j->u0 * 32 + 64; j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    keep(env, j, argv[0]); keep(env, j, argv[1]); keep(env, j, argv[3]);
    if (j->s32) keep(env, j, argv[4]);
    return start_job(env, j, "wsnark_kzg_open");
}
/* kzgVerify(g1, g2 | tau g2, commitments, z32, gamma32 | null, ys, proof) -> Promise<boolean>; host only */
static napi_value js_kzg_verify(napi_env env, napi_callback_info info) {
    size_t argc = 7; napi_value argv[7];
    static const int at[5] = {0, 1, 2, 5, 6};
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_KZG_VERIFY;
    int ok = argc >= 7;
    for (int k = 0; ok && k < 5; k++) ok = get_bytes(env, argv[at[k]], &j->in[k], &j->nin[k]);
    if (!ok || j->nin[0] != 64 || j->nin[1] != 256 || j->nin[2] == 0 || j->nin[2] % 64 || j->nin[3] != j->nin[2] / 2 || j->nin[4] != 64 ||
        !get_scalar32(env, argv[3], 0, &j->r32) || !get_scalar32(env, argv[4], 1, &j->s32) || (!j->s32 && j->nin[2] > 64))
        FAIL(env, j, "expected (g1 (64 bytes), g2 | tau g2 (256), count commitments (64 each), z (32), gamma (32; null for one commitment), count values (32 each), proof (64))");
    for (int k = 0; k < 7; k++)
        if (k != 4 || j->s32) keep(env, j, argv[k]);
    return start_job(env, j, "wsnark_kzg_verify");
}
/* polyEval(polys, len, z32) -> Promise<ArrayBuffer count x 32> */
static napi_value js_poly_eval(napi_env env, napi_callback_info info) {
    size_t argc = 3; napi_value argv[3];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_POLY_EVAL;
    if (argc < 3 || !get_polys(env, argv[0], argv[1], j) || !get_scalar32(env, argv[2], 0, &j->r32))
        FAIL(env, j, "expected (count x len 32-byte coefficients, len, z (32 bytes))");
    j->nout = j->na / j->u0; j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    keep(env, j, argv[0]); keep(env, j, argv[2]);
    return start_job(env, j, "wsnark_fr_poly_eval");
}
/* polyDivide(poly, z32) -> Promise<ArrayBuffer (len - 1) x 32 quotient | the 32-byte value> */
static napi_value js_poly_divide(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_POLY_DIVIDE;
    if (argc < 2 || !get_bytes(env, argv[0], &j->a, &j->na) || j->na == 0 || j->na % 32 || !get_scalar32(env, argv[1], 0, &j->r32))
        FAIL(env, j, "expected (len 32-byte coefficients, z (32 bytes))");
    j->nout = j->na; j->out = (uint8_t*)calloc(j->nout, 1);
    if (!j->out) FAIL(env, j, "out of memory");
    keep(env, j, argv[0]); keep(env, j, argv[1]);
    return start_job(env, j, "wsnark_fr_poly_divide");
}

/* ---- several GPUs in this one process ----
 * groupCreate([device, ...]) -> group handle (synchronous: contexts and worker threads are created at once) */
static napi_value js_group_create(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1], res;
    uint32_t n = 0;
    bool is_arr = false;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (!L.h) { napi_throw_error(env, NULL, "wsnark_napi: init() has not been called (use buildBn128())"); return NULL; }
    if (argc < 1 || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, argv[0], &n) != napi_ok || n == 0 || n > 64) {
        napi_throw_type_error(env, NULL, "expected a non-empty array of device ordinals");
        return NULL;
    }
    int devs[64];
    for (uint32_t i = 0; i < n; i++) {
        napi_value e; int32_t d = 0;
        if (napi_get_element(env, argv[0], i, &e) != napi_ok || napi_get_value_int32(env, e, &d) != napi_ok || d < 0) { napi_throw_type_error(env, NULL, "device ordinals must be non-negative integers"); return NULL; }
        devs[i] = d;
    }
    group_ref_t* gr = (group_ref_t*)calloc(1, sizeof *gr);
    int rc = L.group_create(devs, n, &gr->g);
    if (rc) {
        char msg[600];
        snprintf(msg, sizeof msg, "wsnark_group_create failed (%d): %s -- there is no CPU fallback", rc, L.last_error());
        free(gr);
        napi_throw_error(env, NULL, msg);
        return NULL;
    }
    gr->tag = TAG_GROUP; gr->live = 1; gr->refs = 1;
    if (napi_create_external(env, gr, group_finalize, NULL, &res) != napi_ok) { L.group_free(gr->g); free(gr); napi_throw_error(env, NULL, "wsnark_napi: cannot wrap the group"); return NULL; }
    return res;
}
/* groupFree(group): the group is dead from here on (new calls are refused, queued ones are rejected when they reach the pool);
 * its contexts and the keys still loaded on them are freed now, or by the completion of the last call in flight.  Never blocks
 * the event loop behind a running proof.  The handle stays valid as a dead one. */
static napi_value js_group_free(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1], u;
    group_ref_t* gr = NULL;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc >= 1 && (gr = (group_ref_t*)get_handle(env, argv[0], TAG_GROUP)) && gr->live) group_release(gr);
    napi_get_undefined(env, &u);
    return u;
}
static group_ref_t* live_group(napi_env env, napi_value v) {
    group_ref_t* gr = (group_ref_t*)get_handle(env, v, TAG_GROUP);
    return gr && gr->live ? gr : NULL;
}
static gkey_ref_t* live_gkey(napi_env env, napi_value v) {
    gkey_ref_t* gk = (gkey_ref_t*)get_handle(env, v, TAG_GKEY);
    return gk && gk->k && gk->gr->live ? gk : NULL;
}
/* groupMultiexp(group, which, scalars, points) -> Promise<ArrayBuffer 96/192> */
static napi_value js_group_msm(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    int32_t which = 0;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    if (argc < 4 || !(j->gr = live_group(env, argv[0])) || napi_get_value_int32(env, argv[1], &which) != napi_ok ||
        !get_bytes(env, argv[2], &j->a, &j->na) || !get_bytes(env, argv[3], &j->b, &j->nb))
        FAIL(env, j, "expected (group, which, scalars, points)");
    j->op = which ? OP_GROUP_G2 : OP_GROUP_G1; j->nout = which ? 192 : 96; j->out = (uint8_t*)malloc(j->nout);
    if (j->nb < (j->na / 32) * (which ? 128 : 64)) FAIL(env, j, "points buffer too short for the number of scalars");
    keep(env, j, argv[0]); keep(env, j, argv[2]); keep(env, j, argv[3]);
    job_use_group(j, j->gr);
    return start_job(env, j, "wsnark_group_msm");
}
/* groupLoadKey(group, pkey) -> Promise<group key handle> */
static napi_value js_group_loadkey(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_GROUP_LOADKEY;
    if (argc < 2 || !(j->gr = live_group(env, argv[0])) || !get_bytes(env, argv[1], &j->a, &j->na)) FAIL(env, j, "expected (group, proving_key.bin bytes)");
    j->gk = (gkey_ref_t*)calloc(1, sizeof *j->gk);
    j->gk->tag = TAG_GKEY; j->gk->gr = j->gr; j->gr->refs++;
    keep(env, j, argv[0]); keep(env, j, argv[1]);
    job_use_group(j, j->gr);
    return start_job(env, j, "wsnark_group_pkey_load");
}
/* groupLoadKeyFile(group, path) -> Promise<group key handle>: every member reads its own shard's pages of ONE mapping */
static napi_value js_group_loadkey_file(napi_env env, napi_callback_info info) {
    size_t argc = 2; napi_value argv[2];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_GROUP_LOADKEY_FILE;
    if (argc < 2 || !(j->gr = live_group(env, argv[0])) || !(j->path = get_path(env, argv[1]))) FAIL(env, j, "expected (group, path of a key file)");
    j->gk = (gkey_ref_t*)calloc(1, sizeof *j->gk);
    j->gk->tag = TAG_GKEY; j->gk->gr = j->gr; j->gr->refs++;
    keep(env, j, argv[0]);
    job_use_group(j, j->gr);
    return start_job(env, j, "wsnark_group_pkey_load_file");
}
/* groupProve(groupKey, witness, r32|null, s32|null) -> Promise<ArrayBuffer 448>: proof | r | s used */
static napi_value js_group_prove(napi_env env, napi_callback_info info) {
    size_t argc = 4; napi_value argv[4];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_GROUP_PROVE; j->nout = 448; j->out = (uint8_t*)malloc(448);
    if (argc < 2 || !(j->gk = live_gkey(env, argv[0])) || !get_bytes(env, argv[1], &j->a, &j->na)) FAIL(env, j, "expected (groupKey, witness[, r32, s32])");
    keep(env, j, argv[0]); keep(env, j, argv[1]);
    size_t n;
    napi_valuetype t;
    if (argc > 2 && napi_typeof(env, argv[2], &t) == napi_ok && t != napi_null && t != napi_undefined) {
        if (!get_bytes(env, argv[2], &j->r32, &n) || n != 32) FAIL(env, j, "r must be 32 bytes");
        keep(env, j, argv[2]);
    }
    if (argc > 3 && napi_typeof(env, argv[3], &t) == napi_ok && t != napi_null && t != napi_undefined) {
        if (!get_bytes(env, argv[3], &j->s32, &n) || n != 32) FAIL(env, j, "s must be 32 bytes");
        keep(env, j, argv[3]);
    }
    job_use_group(j, j->gk->gr);
    return start_job(env, j, "wsnark_group_prove");
}
static napi_value js_group_wait_tables(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    job_t* j = (job_t*)calloc(1, sizeof *j);
    j->op = OP_GROUP_WAIT_TABLES; j->nout = 1; j->out = (uint8_t*)calloc(1, 1);
    if (argc < 1 || !(j->gk = live_gkey(env, argv[0]))) FAIL(env, j, "expected a group key handle");
    keep(env, j, argv[0]);
    job_use_group(j, j->gk->gr);
    return start_job(env, j, "wsnark_group_pkey_wait_tables");
}
/* groupKeyInfo(groupKey) -> {nVars, nPublic, domainSize, world, distributedCalcH} */
static napi_value js_group_keyinfo(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1], o, v;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    gkey_ref_t* gk = argc >= 1 ? live_gkey(env, argv[0]) : NULL;
    if (!gk) { napi_throw_type_error(env, NULL, "expected a group key handle"); return NULL; }
    uint32_t nv, np, dom, world; int dist;
    L.group_pkey_info(gk->k, &nv, &np, &dom, &world, &dist);
    napi_create_object(env, &o);
    napi_create_uint32(env, nv, &v); napi_set_named_property(env, o, "nVars", v);
    napi_create_uint32(env, np, &v); napi_set_named_property(env, o, "nPublic", v);
    napi_create_uint32(env, dom, &v); napi_set_named_property(env, o, "domainSize", v);
    napi_create_uint32(env, world, &v); napi_set_named_property(env, o, "world", v);
    napi_get_boolean(env, dist != 0, &v); napi_set_named_property(env, o, "distributedCalcH", v);
    return o;
}

/* ---- bin2int / bin2g1 / bin2g2 of the reference (src/bn128.js:319-351, 714-718) in native code ----
 * proofToObject(ArrayBuffer 384) -> {pi_a: [x, y, z], pi_b: [[x0, x1], [y0, y1], [z0, z1]], pi_c: [x, y, z]} of decimal strings */
static void le256_to_decimal(const uint8_t* le, char* out /* >= 80 bytes */) {
    uint32_t w[8];
    char rev[96];
    int n = 0;
    for (int i = 0; i < 8; i++) w[i] = (uint32_t)le[4 * i] | ((uint32_t)le[4 * i + 1] << 8) | ((uint32_t)le[4 * i + 2] << 16) | ((uint32_t)le[4 * i + 3] << 24);
    for (;;) {
        uint64_t rem = 0;
        int nonzero = 0;
        for (int i = 7; i >= 0; i--) {                 /* w /= 10^9 */
            const uint64_t cur = (rem << 32) | w[i];
            w[i] = (uint32_t)(cur / 1000000000u);
            rem = cur % 1000000000u;
            nonzero |= w[i] != 0;
        }
        for (int k = 0; k < 9; k++) { rev[n++] = (char)('0' + rem % 10); rem /= 10; if (!nonzero && rem == 0) break; }
        if (!nonzero) break;
    }
    while (n > 1 && rev[n - 1] == '0') n--;
    for (int i = 0; i < n; i++) out[i] = rev[n - 1 - i];
    out[n] = 0;
}
static napi_value js_proof_to_object(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1];
    uint8_t* p = NULL; size_t n = 0;
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 1 || !get_bytes(env, argv[0], &p, &n) || n != 384) { napi_throw_type_error(env, NULL, "expected the 384 proof bytes"); return NULL; }
    napi_value v[12], o, a, b, c, pair;
    char dec[96];
    for (int i = 0; i < 12; i++) { le256_to_decimal(p + 32 * i, dec); napi_create_string_utf8(env, dec, NAPI_AUTO_LENGTH, &v[i]); }
    napi_create_object(env, &o);
    napi_create_array_with_length(env, 3, &a);
    for (uint32_t i = 0; i < 3; i++) napi_set_element(env, a, i, v[i]);
    napi_create_array_with_length(env, 3, &b);
    for (uint32_t i = 0; i < 3; i++) {
        napi_create_array_with_length(env, 2, &pair);
        napi_set_element(env, pair, 0, v[3 + 2 * i]);
        napi_set_element(env, pair, 1, v[4 + 2 * i]);
        napi_set_element(env, b, i, pair);
    }
    napi_create_array_with_length(env, 3, &c);
    for (uint32_t i = 0; i < 3; i++) napi_set_element(env, c, i, v[9 + i]);
    napi_set_named_property(env, o, "pi_a", a);
    napi_set_named_property(env, o, "pi_b", b);
    napi_set_named_property(env, o, "pi_c", c);
    return o;
}

/* init(device) -> device info string */
static napi_value js_init(napi_env env, napi_callback_info info) {
    size_t argc = 1; napi_value argv[1], s;
    int32_t dev = -1;
    char err[4600];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc > 0) napi_get_value_int32(env, argv[0], &dev);
    if (load_lib(err, sizeof err)) { napi_throw_error(env, NULL, err); return NULL; }
    int rc = L.init(dev);
    if (rc) {
        char msg[600];
        snprintf(msg, sizeof msg, "wsnark_init failed (%d): %s -- there is no CPU fallback", rc, L.last_error());
        napi_throw_error(env, NULL, msg);
        return NULL;
    }
    napi_create_string_utf8(env, L.device_info(), NAPI_AUTO_LENGTH, &s);
    return s;
}
static napi_value js_shutdown(napi_env env, napi_callback_info info) {
    (void)info;
    if (L.h) L.shutdown();
    napi_value u; napi_get_undefined(env, &u);
    return u;
}

static napi_value module_init(napi_env env, napi_value exports) {
    Dl_info di;
    snprintf(L.dir, sizeof L.dir, ".");
    if (dladdr((void*)module_init, &di) && di.dli_fname) {
        snprintf(L.dir, sizeof L.dir, "%s", di.dli_fname);
        char* sl = strrchr(L.dir, '/');
        if (sl) *sl = 0;
    }
    napi_property_descriptor props[] = {
        {"init", NULL, js_init, NULL, NULL, NULL, napi_default, NULL},
        {"shutdown", NULL, js_shutdown, NULL, NULL, NULL, napi_default, NULL},
        {"g1Multiexp", NULL, js_g1, NULL, NULL, NULL, napi_default, NULL},
        {"g2Multiexp", NULL, js_g2, NULL, NULL, NULL, napi_default, NULL},
        {"fft", NULL, js_fft, NULL, NULL, NULL, napi_default, NULL},
        {"calcH", NULL, js_calch, NULL, NULL, NULL, napi_default, NULL},
        {"loadKey", NULL, js_loadkey, NULL, NULL, NULL, napi_default, NULL},
        {"loadKeyFile", NULL, js_loadkey_file, NULL, NULL, NULL, napi_default, NULL},
        {"loadKeyZkey", NULL, js_loadkey_zkey, NULL, NULL, NULL, napi_default, NULL},
        {"loadKeyZkeyFile", NULL, js_loadkey_zkey_file, NULL, NULL, NULL, napi_default, NULL},
        {"keyFileInfo", NULL, js_keyfile_info, NULL, NULL, NULL, napi_default, NULL},
        {"groupLoadKeyFile", NULL, js_group_loadkey_file, NULL, NULL, NULL, napi_default, NULL},
        {"hashBytes", NULL, js_hash, NULL, NULL, NULL, napi_default, NULL},
        {"keyInfo", NULL, js_keyinfo, NULL, NULL, NULL, napi_default, NULL},
        {"allocPinned", NULL, js_alloc_pinned, NULL, NULL, NULL, napi_default, NULL},
        {"prove", NULL, js_prove, NULL, NULL, NULL, napi_default, NULL},
        {"waitTables", NULL, js_wait_tables, NULL, NULL, NULL, napi_default, NULL},
        {"verify", NULL, js_verify, NULL, NULL, NULL, napi_default, NULL},
        {"verifyBatch", NULL, js_verify_batch, NULL, NULL, NULL, napi_default, NULL},
        {"codecPoints", NULL, js_codec_points, NULL, NULL, NULL, napi_default, NULL},
        {"codecProofs", NULL, js_codec_proofs, NULL, NULL, NULL, napi_default, NULL},
        {"verifyBatchCompressed", NULL, js_verify_batch_compressed, NULL, NULL, NULL, napi_default, NULL},
        {"proveBatch", NULL, js_prove_batch, NULL, NULL, NULL, napi_default, NULL},
        {"checkKey", NULL, js_check_key, NULL, NULL, NULL, napi_default, NULL},
        {"contributeKey", NULL, js_contribute_key, NULL, NULL, NULL, napi_default, NULL},
        {"deltaVerify", NULL, js_delta_verify, NULL, NULL, NULL, napi_default, NULL},
        {"groupNtt", NULL, js_group_ntt, NULL, NULL, NULL, napi_default, NULL},
        {"zkeyInfo", NULL, js_zkey_info, NULL, NULL, NULL, napi_default, NULL},
        {"importZkey", NULL, js_import_zkey, NULL, NULL, NULL, napi_default, NULL},
        {"exportZkey", NULL, js_export_zkey, NULL, NULL, NULL, napi_default, NULL},
        {"newKey", NULL, js_new_key, NULL, NULL, NULL, napi_default, NULL},
        {"mulPoints", NULL, js_mul_points, NULL, NULL, NULL, napi_default, NULL},
        {"contributePowers", NULL, js_contribute_powers, NULL, NULL, NULL, napi_default, NULL},
        {"checkPowers", NULL, js_check_powers, NULL, NULL, NULL, napi_default, NULL},
        {"checkKeyCircuit", NULL, js_check_key_circuit, NULL, NULL, NULL, napi_default, NULL},
        {"loadCircuit", NULL, js_circuit_load, NULL, NULL, NULL, napi_default, NULL},
        {"circuitFromRows", NULL, js_circuit_from_rows, NULL, NULL, NULL, napi_default, NULL},
        {"loadCircuitRows", NULL, js_circuit_load_rows, NULL, NULL, NULL, napi_default, NULL},
        {"circuitInfo", NULL, js_circuit_info, NULL, NULL, NULL, napi_default, NULL},
        {"circuitFree", NULL, js_circuit_free, NULL, NULL, NULL, napi_default, NULL},
        {"circuitCheckWitness", NULL, js_circuit_check_witness, NULL, NULL, NULL, napi_default, NULL},
        {"circuitCheckWitnesses", NULL, js_circuit_check_witnesses, NULL, NULL, NULL, napi_default, NULL},
        {"checkWitness", NULL, js_check_witness, NULL, NULL, NULL, napi_default, NULL},
        {"proofToObject", NULL, js_proof_to_object, NULL, NULL, NULL, napi_default, NULL},
        {"kzgLoadSrs", NULL, js_kzg_load, NULL, NULL, NULL, napi_default, NULL},
        {"kzgCommit", NULL, js_kzg_commit, NULL, NULL, NULL, napi_default, NULL},
        {"kzgOpen", NULL, js_kzg_open, NULL, NULL, NULL, napi_default, NULL},
        {"kzgVerify", NULL, js_kzg_verify, NULL, NULL, NULL, napi_default, NULL},
        {"polyEval", NULL, js_poly_eval, NULL, NULL, NULL, napi_default, NULL},
        {"polyDivide", NULL, js_poly_divide, NULL, NULL, NULL, napi_default, NULL},
        {"loadPoints", NULL, js_points_load, NULL, NULL, NULL, napi_default, NULL},
        {"pointsMultiexp", NULL, js_points_msm, NULL, NULL, NULL, napi_default, NULL},
        {"groupCreate", NULL, js_group_create, NULL, NULL, NULL, napi_default, NULL},
        {"groupFree", NULL, js_group_free, NULL, NULL, NULL, napi_default, NULL},
        {"groupMultiexp", NULL, js_group_msm, NULL, NULL, NULL, napi_default, NULL},
        {"groupLoadKey", NULL, js_group_loadkey, NULL, NULL, NULL, napi_default, NULL},
        {"groupProve", NULL, js_group_prove, NULL, NULL, NULL, napi_default, NULL},
        {"groupWaitTables", NULL, js_group_wait_tables, NULL, NULL, NULL, napi_default, NULL},
        {"groupKeyInfo", NULL, js_group_keyinfo, NULL, NULL, NULL, napi_default, NULL},
    };
    CHECK(env, napi_define_properties(env, exports, sizeof props / sizeof props[0], props));
    return exports;
}
NAPI_MODULE(NODE_GYP_MODULE_NAME, module_init)
