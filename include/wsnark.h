/*
 * wsnark.h -- C ABI of libwsnark.so: the MI355X-native replacement for the BN128
 * Groth16 prove hot path of iden3/wasmsnark.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference root, /root/reference in the build container).  The seam is the one the
 * reference itself has: the three worker commands G1_MULTIEXP / G2_MULTIEXP / CALC_H
 * (src/bn128.js:102-166), their host wrappers Bn128.g1_multiexp / g2_multiexp / calcH
 * (src/bn128.js:353-415, 569-578) and Bn128.groth16GenProof (src/bn128.js:580-720).
 * INTEGRATION.md shows the N-API / ctypes bindings over this header.
 *
 * Byte layouts are the reference's (tools/buildpkey.js:57-77, tools/buildwitness.js:36-41):
 *   field element  32 B little-endian; Montgomery form (R = 2^256) unless stated "plain"
 *   G1 affine      64 B  (x, y)                x == 0  => point at infinity
 *   G2 affine      128 B (x.c0, x.c1, y.c0, y.c1)
 *   G1 Jacobian    96 B  (x, y, z)             z == 0  => infinity; canonical (0, 1, 0)
 *   G2 Jacobian    192 B
 *   scalars        32 B raw 256-bit little-endian, NOT required to be < r
 *
 * All functions return 0 on success or a WSNARK_ERR_* code; none throws or aborts.
 * wsnark_last_error() gives a thread-local human-readable message.
 * Input pointers are borrowed for the duration of the call only.
 * "_dev" variants take DEVICE pointers (hipMalloc / torch tensor data_ptr) and a
 * hipStream_t (as void*; NULL = the library's own stream); results that are a single
 * group element are still written to HOST memory.
 *
 * Threading: every entry point may be called from any host thread at any time (the Node addon calls from
 * the libuv pool); each call selects the context's GPU for its thread first.  A context has a few LANES
 * (WSNARK_LANES, default 2): a lane holds everything one call in flight needs besides the read-only key (queues,
 * MSM plans, transform scratch, per-proof buffers), so two proofs -- on one key handle or on two -- or a proof and
 * an MSM overlap on one GPU; further concurrent callers wait for a lane.  There is no process-global mode: sharding
 * parameters are per call.  Unlike the reference's WASM instance (static scratch,
 * non-re-entrant) no caller-side queue is needed.
 * Host buffers are read through a pinned staging ring and are free for reuse when the call returns.
 */
#ifndef WSNARK_H
#define WSNARK_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WSNARK_OK 0
#define WSNARK_ERR_SIZE 1    /* n not a power of two, > 2^28, or inconsistent lengths */
#define WSNARK_ERR_FORMAT 2  /* malformed proving key / pols records / offsets out of range */
#define WSNARK_ERR_HIP 3     /* HIP runtime error, see wsnark_last_error() */
#define WSNARK_ERR_ARG 4     /* NULL pointer or bad handle */
#define WSNARK_ERR_NOINIT 5  /* wsnark_init() not called */

typedef struct wsnark_pkey wsnark_pkey_t;

/* Replaces build() / worker INIT (src/bn128.js:173-265, 55-66): selects the GPU, creates
 * the library stream.  device < 0 => use $LOCAL_RANK or 0.  Idempotent. */
int wsnark_init(int device);
/* Replaces Bn128.terminate() / worker TERMINATE (src/bn128.js:562-566, 167-169). */
void wsnark_shutdown(void);
const char* wsnark_last_error(void);
/* "<device name> <gcn arch> CUs=<n> device=<ordinal>" of the device in use */
const char* wsnark_device_info(void);

/* Worker command G1_MULTIEXP + Bn128.g1_multiexp (src/bn128.js:102-113, 353-383;
 * kernel g1m_multiexp2, src/build_multiexp.js:651-744).  Host pointers.
 * out96 = sum_i scalars[i]*points[i] as Jacobian-Montgomery, affine-normalised
 * ((x, y, 1) or (0, 1, 0)); n == 0 => infinity. */
int wsnark_g1_msm(const void* scalars, const void* points_affine, uint64_t n, void* out96);
/* Worker command G2_MULTIEXP + Bn128.g2_multiexp (src/bn128.js:114-125, 385-415;
 * kernel g2m_multiexp, src/build_multiexp.js:498-580). */
int wsnark_g2_msm(const void* scalars, const void* points_affine, uint64_t n, void* out192);
int wsnark_g1_msm_dev(const void* d_scalars, const void* d_points_affine, uint64_t n, void* out96_host, void* stream);
int wsnark_g2_msm_dev(const void* d_scalars, const void* d_points_affine, uint64_t n, void* out192_host, void* stream);

/* The gather step of Bn128.g1_multiexp / g2_multiexp (src/bn128.js:374-382, 406-414): serial EC
 * sum of `count` Jacobian-Montgomery partial results (any z), host arithmetic, no GPU needed.
 * Used to combine per-GPU partial MSMs after the one all-gather of a sharded run.
 * out = affine-normalised Jacobian-Montgomery. */
int wsnark_g1_sum(const void* jac_points, uint64_t count, void* out96);
int wsnark_g2_sum(const void* jac_points, uint64_t count, void* out192);

/* Multi-GPU alternative to splitting the pairs (the shard is a PER-CALL argument): every rank is given ALL pairs
 * and computes only the Pippenger windows w with w % world == rank; its result is then a partial sum already scaled
 * by 2^(c*w), so the partials of all ranks combine by plain EC addition (all_gather + wsnark_g*_sum) -- the worker
 * split and gather of src/bn128.js:353-415 with GPUs as workers.  (rank 0, world 1) is the whole sum. */
int wsnark_g1_msm_windows(const void* scalars, const void* points_affine, uint64_t n, uint32_t rank, uint32_t world, void* out96);
int wsnark_g2_msm_windows(const void* scalars, const void* points_affine, uint64_t n, uint32_t rank, uint32_t world, void* out192);
int wsnark_g1_msm_windows_dev(const void* d_scalars, const void* d_points_affine, uint64_t n, uint32_t rank, uint32_t world,
                              void* out96_host, void* stream);
int wsnark_g2_msm_windows_dev(const void* d_scalars, const void* d_points_affine, uint64_t n, uint32_t rank, uint32_t world,
                              void* out192_host, void* stream);

/* fft_fft / fft_ifft (src/build_fft.js:159-221), in place on n Montgomery Fr elements.
 * n must be a power of two <= 2^28 (the reference traps otherwise, :137-154);
 * inverse with n == 1 is rejected (the reference never returns, :575-583). */
int wsnark_fr_ntt(void* buf, uint64_t n, int odd, int inverse);
int wsnark_fr_ntt_dev(void* d_buf, uint64_t n, int odd, int inverse, void* stream);
/* Building blocks of the DISTRIBUTED transform (four-step, n = n1 * n2 over the ranks of one node; orchestrated by
 * wasmsnark_amd/dist.py: dist_ntt -- the reference never parallelises a transform, src/bn128.js:126-166 runs CALC_H
 * on one worker).  batch: `count` independent length-n transforms stored back to back (the column step and the row
 * step), same semantics per transform as wsnark_fr_ntt_dev with odd = 0.  dist_scale: element (r, c) of a rank's
 * rows x cols row-major block stands at global position t = (row0 + r) + 2^log_n1 * c of the length-2^log_n vector
 * (cols must be 2^(log_n - log_n1)); `stack` such blocks -- the slices of several vectors that go through the same
 * transform together, one exchange for all of them -- lie one after the other; every element is multiplied by
 *   mode 0: w_n^((row0 + r) * c)  -- the twiddle between the two steps (inverse != 0: the inverse root)
 *   mode 1: w_2n^t                -- the coset pre-scale of odd = 1 (src/build_fft.js:159-187) */
int wsnark_fr_ntt_batch_dev(void* d_buf, uint64_t n, uint64_t count, int inverse, void* stream);
/* The other pieces of a distributed CALC_H (src/bn128.js:126-166), all on device arrays:
 *   pkey_eval_ab : a = A w, b = B w -- the two pol_constructLC calls (src/build_pol.js:62-144, bn128.js:139-145) from a
 *                  device-resident plain witness; `domain` Montgomery elements each
 *   fr_mul       : fft_mulN (src/build_fft.js:461-505), out[i] = a[i] * b[i]
 *   dist_combine : h[t] = fromMontgomery((e[t] - w_2n^-t o[t]) / 2) on a rank's block, t as in dist_scale (the upper
 *                  half of the reference's size-2n inverse transform, bn128.js:160-164; derivation in csrc/calch.hip) */
int wsnark_pkey_eval_ab_dev(wsnark_pkey_t* handle, const void* d_witness, size_t witness_len, void* d_a_out, void* d_b_out, void* stream);
int wsnark_fr_mul_dev(const void* d_a, const void* d_b, void* d_out, uint64_t n, void* stream);
int wsnark_fr_dist_combine_dev(const void* d_e, const void* d_o, void* d_h_out, uint64_t rows, uint64_t cols, uint64_t row0,
                               uint32_t log_n1, uint32_t log_n, void* stream);
int wsnark_fr_dist_scale_dev(void* d_buf, uint64_t stack, uint64_t rows, uint64_t cols, uint64_t row0, uint32_t log_n1, uint32_t log_n,
                             int mode, int inverse, void* stream);
/* fft_toMontgomeryN / fft_fromMontgomeryN (src/build_fft.js:418-458, 507-547) */
int wsnark_fr_to_montgomery(const void* in, void* out, uint64_t n);
int wsnark_fr_from_montgomery(const void* in, void* out, uint64_t n);

/* Worker command CALC_H + Bn128.calcH (src/bn128.js:126-166, 569-578).
 * signals: n_signals x 32 B plain; polsA/polsB: the key's record streams
 * (u32 ncoefs, then ncoefs x (u32 idx, 32 B coef)) per signal (src/build_pol.js:62-144);
 * out_h: domain x 32 B plain. */
int wsnark_calc_h(const void* signals, const void* polsA, size_t lenA, const void* polsB, size_t lenB,
                  uint32_t n_signals, uint32_t domain, void* out_h);

/* Parses proving_key.bin (tools/buildpkey.js:124-240; header read at src/bn128.js:581-604)
 * and makes it device-resident (points as-is, pols transposed to row-major CSR). */
int wsnark_pkey_load(const void* pkey, size_t len, wsnark_pkey_t** out_handle);
void wsnark_pkey_free(wsnark_pkey_t* handle);
int wsnark_pkey_info(const wsnark_pkey_t* handle, uint32_t* n_vars, uint32_t* n_public, uint32_t* domain);
/* How the key's five point sections are resident (no counterpart in the reference, which reads the sections in place:
 * src/bn128.js:592-604).  By default each section is kept as a fixed-base window table -- rows x n points, row w =
 * 2^(c w) * section -- so that a sum is `rows` passes into one bucket set (13 rows, c = 20, at 2^20 pairs; about 6 GB
 * for the five sections).  c_w / rows_w: the A, B1, B2, C tables (nVars pairs); c_h / rows_h: the hExps table
 * (domainSize pairs); bytes: device memory of all five.  Plain sections (WSNARK_KEY_TABLE=0, or tables that do not
 * fit: WSNARK_TABLE_MAX_GB, half of the free memory): c = 0, rows = 1.  Any out pointer may be NULL. */
int wsnark_pkey_table_info(const wsnark_pkey_t* handle, uint32_t* c_w, uint32_t* rows_w, uint32_t* c_h, uint32_t* rows_h,
                           uint64_t* bytes);

/* The table rows beyond the plain sections are built in the BACKGROUND (the context's build queue, lowest stream priority, one key
 * after the other): wsnark_pkey_load* return as soon as the sections are resident (about 30 ms for a 0.59 GB key instead of 214),
 * proofs that start before the build is over (~0.17 s at 2^20) run on the plain sections -- same results, about twice the
 * steady-state time while the build shares the GPU with them (10 % over it on an idle GPU) -- and later ones on the tables.  This call blocks until the handle's tables are
 * built (benchmarks; callers that want the steady state before their first proof).  WSNARK_TABLE_ASYNC=0 makes the load itself wait,
 * as in round 3.  Calls that shard the WINDOWS of a whole key over ranks (wsnark_groth16_prove_partial with world > 1 on a whole
 * key) wait by themselves: their partial sums must mean the same on every rank. */
int wsnark_pkey_wait_tables(wsnark_pkey_t* handle);

/* Wall-clock of the handle's load, in ms: [1] point sections host -> device, [2] infinity masks + conversion to the device
 * field's domain, [0] polsA / polsB -> CSR (header walk on the host, upload, transposition on the GPU), [3] fixed-base table
 * build, [4] the whole call -- what a cold caller waits before its first proof (the reference re-parses the key inside every
 * groth16GenProof call, src/bn128.js:581-604).  With the background build (the default) [4] = [1] + [2] + [0] and [3] is the
 * build's own duration on the GPU (0 until it is over); with WSNARK_TABLE_ASYNC=0 the call waits for it and [4] includes it. */
int wsnark_pkey_load_stats(const wsnark_pkey_t* handle, double* ms5);

/* The same key given as separate host buffers with 64-bit lengths: proving_key.bin addresses its
 * sections with u32 byte offsets (tools/buildpkey.js:133-139), which caps a key at 4 GiB (~2^23
 * constraints); this entry point is the container for larger keys (BASELINE config 5).
 * pointsC holds nVars-nPublic-1 points (signals nPublic+1..), as in the file. */
typedef struct {
    uint32_t n_vars, n_public, domain;
    const void *alfa1, *beta1, *delta1;      /* 64 B each  */
    const void *beta2, *delta2;              /* 128 B each */
    const void* polsA; uint64_t polsA_len;   /* record streams, src/build_pol.js:62-144 */
    const void* polsB; uint64_t polsB_len;
    /* point arrays with the number of BYTES readable behind each pointer; a section shorter than the header
     * implies (nVars x 64, nVars x 64, nVars x 128, (nVars-nPublic-1) x 64, domain x 64) is WSNARK_ERR_FORMAT */
    const void* pointsA;  uint64_t pointsA_len;
    const void* pointsB1; uint64_t pointsB1_len;
    const void* pointsB2; uint64_t pointsB2_len;
    const void* pointsC;  uint64_t pointsC_len;
    const void* pointsH;  uint64_t pointsH_len;
} wsnark_key_sections_t;
int wsnark_pkey_load_sections(const wsnark_key_sections_t* sections, wsnark_pkey_t** out_handle);

/* Multi-GPU: ONE RANK'S SHARE of a key, split by points -- the reference's own worker split (src/bn128.js:353-361:
 * contiguous ranges of the pairs, the remainder to the last worker) with GPUs as workers.  Every rank passes the same
 * (complete) sections and keeps only the points of signals [rank * floor(nVars / world), ...) of A, B1, B2 and C and its
 * share of hExps: 1 / world of the device memory and of the additions of every sum, uniform whatever the window count
 * (wsnark_pkey_table_info reports the shard's own tables).  The two sparse matrices stay complete (CALC_H needs all rows).
 * h_interleave_log = 0: the hExps share is the contiguous range [rank * floor(domain / world), ...): every rank computes
 * the whole h (wsnark_groth16_prove_partial without WSNARK_PARTIAL_SKIP_H).  h_interleave_log = k > 0 (world a power of
 * two, world <= 2^k <= domain): the share is the rank's rows of the 2^k-interleaved layout in which the distributed CALC_H
 * leaves its slice of h -- local element (r, j) = hExps[(rank * 2^k / world + r) + 2^k * j], row-major -- to be summed with
 * wsnark_pkey_h_msm_dev.  On such a handle wsnark_groth16_prove_partial[_dev] must be called with the handle's own (rank,
 * world) and returns the partial sums over the handle's pairs (all windows); wsnark_groth16_prove[_dev] is WSNARK_ERR_ARG;
 * wsnark_groth16_prove_finish works on any handle of the key (it only needs the five fixed points). */
int wsnark_pkey_load_shard(const wsnark_key_sections_t* sections, uint32_t rank, uint32_t world, uint32_t h_interleave_log,
                           wsnark_pkey_t** out_handle);
/* A key FILE (round 6): `path` names the reference's proving_key.bin (tools/buildpkey.js:124-186: u32
 * section offsets, at most 4 GiB) or the WSNARK64 container -- the same sections in the same order behind 64-bit offsets, for keys the
 * reference's format cannot hold (BASELINE config 5, 7.8 GB at 2^24); layout: wasmsnark_amd/csrc/keyfile.hip, written by
 * wasmsnark_amd/formats.py / js/formats.js.  The file is mapped read-only and ONLY the pages of the share asked for are read:
 * (rank, world, h_interleave_log) as in wsnark_pkey_load_shard -- (0, 1, 0) loads the whole key -- so eight ranks read the five point
 * sections once between them (each the two matrices); every range goes back to the kernel as soon as it has been staged, so the
 * load's resident set does not grow with the key.  Replaces the caller-side `fs.readFileSync` + `new Uint32Array(pkey)` of
 * src/bn128.js:580-604 for keys that do not fit one ArrayBuffer.  Errors: WSNARK_ERR_ARG (cannot open), WSNARK_ERR_FORMAT. */
int wsnark_pkey_load_file(const char* path, uint32_t rank, uint32_t world, uint32_t h_interleave_log, wsnark_pkey_t** out_handle);
/* header of a key file without loading it (no GPU needed).  format: 1 = proving_key.bin, 2 = WSNARK64.  Out pointers may be NULL. */
int wsnark_pkey_file_info(const char* path, uint32_t* n_vars, uint32_t* n_public, uint32_t* domain, uint64_t* file_bytes, int* format);
/* ---- the audit of a proving key (csrc/pkeycheck.hip; snarkjs users know the step as `zkey verify`) ----
 * The loaders above never look at a point: a coordinate that is no field element, a point off its curve, a G2 point outside the
 * order-r subgroup or a B2 section that does not match B1 all load, and every later proof is then rejected by every verifier.  These
 * three calls take exactly what wsnark_pkey_load, _load_sections and _load_file take -- the key's BYTES, not a handle: after a load
 * an unreduced coordinate can no longer be seen -- and look at the whole key on the device (no shard parameters).  Nothing calls them
 * unless the host asks: they change no other call.
 *   WSNARK_PKCHECK_POINTS     every point of A, B1, C, hExps (G1) and B2 (G2): x == 0 is infinity by the loaders' own rule (counted in
 *                             infinity[], the rest of its bytes is not read); otherwise every coordinate < q, the curve equation
 *                             (y^2 = x^3 + 3; on the twist x^3 + 3/(9+u)), and for B2 [r] Q == O.  G1 has cofactor 1: no subgroup
 *                             test.  bad[], first_bad[], first_reason[] come from a reduction on the device and do not depend on
 *                             how the sections are cut into chunks.  The five fixed points get the same tests on the host; there
 *                             infinity (x == 0) is itself bad, reason 4, and as for every point it is decided first.
 *   WSNARK_PKCHECK_RELATIONS  with the standard generators G1, G2:   bit 0  e(beta1, G2) = e(G1, beta2)
 *                             bit 1  e(delta1, G2) = e(G1, delta2)    bit 2  e(sum rho_j B1_j, G2) = e(G1, sum rho_j B2_j)
 *                             rho_j: 128 non-zero bits from seed32 and the index j (ChaCha20 block, key = seed, counter = j).  A
 *                             relation is run only if every point it involves passed the point tests (or those were not asked
 *                             for); one that was not run leaves its relations_run bit clear, and then ok = 0.
 *                             seed32 == NULL: 32 bytes from the OS (getrandom), as the blinding values.  Bit 2 is sound with
 *                             probability 1 - 2^-128 over a seed that whoever made the key did NOT know: a fixed or published seed
 *                             gives no soundness.  What the audit cannot see: a permutation applied to B1 and B2 alike, and any
 *                             relation to the circuit (A, C, hExps against the polynomials): both are wsnark_pkey_circuit_check's
 *                             (below), which needs the circuit and the powers of tau the key was built on, not the toxic waste.
 * A bad key is a RESULT: WSNARK_OK with ok = 0.  What the loaders reject (a short section, a bad header, a file that cannot be
 * opened) fails with the loader's code and writes nothing.  Needs wsnark_init (WSNARK_ERR_NOINIT); callable from any thread, each call
 * takes a lane of the context.  Sections are streamed through the staging ring in chunks of WSNARK_PKCHECK_CHUNK points (default
 * 2^18): device memory does not grow with the key, and the file variant hands every staged range back to the kernel. */
enum { WSNARK_PK_A = 0, WSNARK_PK_B1 = 1, WSNARK_PK_B2 = 2, WSNARK_PK_C = 3, WSNARK_PK_H = 4 };      /* sections in report order */
/* why a point is bad; when several apply, the smallest number is reported */
enum { WSNARK_PK_UNREDUCED = 1, WSNARK_PK_OFF_CURVE = 2, WSNARK_PK_OUTSIDE_SUBGROUP = 3, WSNARK_PK_INFINITY = 4 /* fixed points only */ };
#define WSNARK_PKCHECK_POINTS    1u
#define WSNARK_PKCHECK_RELATIONS 2u      /* flags == 0 means both */
typedef struct {
    uint64_t points[5], infinity[5], bad[5];
    uint64_t first_bad[5];               /* smallest index of a bad point, UINT64_MAX if none */
    uint32_t first_reason[5];
    uint32_t fixed_reason[5];            /* alfa1, beta1, delta1, beta2, delta2: 0 = good */
    uint32_t relations_run, relations_bad;   /* bit 0: beta1 ~ beta2, bit 1: delta1 ~ delta2, bit 2: B1 ~ B2 */
    uint32_t ok;                         /* 1 iff nothing is bad and every requested check was run */
    double   ms[4];                      /* upload + point kernels, relation sums, host pairings, whole call */
} wsnark_pkey_report_t;
int wsnark_pkey_check(const void* pkey, size_t len, uint32_t flags, const void* seed32, wsnark_pkey_report_t* out);
int wsnark_pkey_check_sections(const wsnark_key_sections_t* sections, uint32_t flags, const void* seed32, wsnark_pkey_report_t* out);
int wsnark_pkey_check_file(const char* path, uint32_t flags, const void* seed32, wsnark_pkey_report_t* out);
/* ---- the phase-2 contribution to a key's delta, and its check (csrc/pkeydelta.hip; snarkjs: `zkey contribute` / `zkey verify`) ----
 * Nobody should deploy a key whose delta is known to whoever ran the setup.  A contribution by a secret d (non-zero mod r) turns a
 * key with C_j = (.../delta) G1, hExps_i = (tau^i Z(tau)/delta) G1, delta1 = delta G1, delta2 = delta G2 into the same key under
 * delta d:   delta1' = d delta1, delta2' = d delta2 (host)     C'_j = d^-1 C_j, hExps'_i = d^-1 hExps_i (device, one lane per point)
 * and leaves everything else -- header, alfa1, beta1, beta2, polsA, polsB, A, B1, B2 -- byte for byte as it was.  A point with
 * x == 0 is infinity by the loaders' rule and is copied through byte for byte.
 *   wsnark_g{1,2}_scale_batch   out[i] = k * points[i]; affine Montgomery in and out, x == 0 is infinity (copied through); k: 32 bytes
 *                             plain LE, reduced mod r; a result at infinity is written as zeros.  The counterpart of
 *                             wsnark_g{1,2}_mul_base_batch (one base, many scalars): many bases, ONE scalar.  Every input gets the
 *                             audit's two cheap tests (coordinates < q, the curve equation; NOT the G2 subgroup test): a bad point
 *                             fails the call with WSNARK_ERR_FORMAT (wsnark_last_error names the first index), out is then unspecified.
 *   d32                       32 bytes plain little-endian, reduced mod r; d = 0 mod r is WSNARK_ERR_ARG.  d32 == NULL draws the 32
 *                             bytes from the OS (getrandom), as the blinding values: the production case.  The library never returns
 *                             the secret and wipes d, d^-1 and the digit string of d^-1 (volatile stores) before it returns; the
 *                             digits also cross to the device in the kernels' argument blocks, which the runtime owns.  With an
 *                             explicit d32 the call is deterministic.
 *   a bad input is a RESULT   as in the audit: WSNARK_OK with ok = 0 for a C or hExps point with a coordinate >= q or off the curve
 *                             (bad[], first_bad[], first_reason[]: reduced on the device as the audit's, independent of the chunking)
 *                             and for a delta1 or delta2 that fails the audit's fixed-point tests (then no section is looked at and
 *                             the counts stay 0).  With ok = 0 the output buffers are unspecified; the file variant removes its output.
 *   errors                    what the loaders reject (a short section, a bad header, a file that cannot be opened) fails with the
 *                             loader's code before anything is written, as wsnark_pkey_check does; out_cap < len is WSNARK_ERR_SIZE;
 *                             in_path and out_path naming one file is WSNARK_ERR_ARG; before wsnark_init WSNARK_ERR_NOINIT.  A report
 *                             that was not produced is left untouched.
 *   streaming                 C and hExps go through the staging ring in chunks of WSNARK_PKDELTA_CHUNK points (default 2^18, clamped
 *                             to [64, 2^22] as WSNARK_PKCHECK_CHUNK): a chunk goes up, is scaled, and comes down, the next chunk's
 *                             upload beside this chunk's kernel; device memory does not grow with the key.  The file variant maps
 *                             the input read-only, writes the output in the input's format (proving_key.bin or WSNARK64, also above
 *                             4 GiB) and hands every range it has read back to the kernel.  Each call takes a lane of the context;
 *                             nothing else calls these functions and no other entry point changes.
 *                             out_pkey may not overlap pkey unless it IS pkey (in place).
 * wsnark_pkey_delta_verify*: what the next participant runs on (old key, new key).
 *   bit 0  everything but C, hExps, delta1, delta2 is byte-identical: a host memcmp of nVars, nPublic, domainSize, alfa1, beta1,
 *          beta2, both record streams, A, B1, B2.  If the counts or the streams' lengths differ the bit is bad and bits 2, 3 are not run.
 *   bit 1  e(delta1', G2) = e(G1, delta2'); run only if both new points pass the audit's fixed-point tests.
 *   bit 2  e(sum rho_j C'_j, delta2') = e(sum rho_j C_j, delta2)      bit 3  the same for hExps.  rho_j as in the audit (ChaCha20,
 *          key = seed32, counter = the global index j), the SAME for the old and the new point j; the sums run chunk by chunk through
 *          the ordinary G1 MSM, partial sums added on the host.  Run only if bit 1 ran and held -- that is what makes them mean
 *          something: C' = c C and delta2' = c' delta2 pass iff c c' = 1.
 *   bit 4  delta2' != delta2 (a contribution by 1 is none).
 *   seed32 == NULL: 32 bytes from the OS.  As in the audit, bits 2 and 3 are sound with probability 1 - 2^-128 over a seed the
 *   contributor did NOT know; a fixed or published seed gives no soundness.
 *   The check does NOT test individual points -- that is wsnark_pkey_check's job: run the audit on the new key first.  Unreduced
 *   or off-curve bytes do not fault it, they only make the sums meaningless, as in the prover.
 * Out of scope: a transcript of contributions, the proof of knowledge of d that snarkjs stores with each of them, a random
 * beacon, and anything that touches the circuit. */
int wsnark_g1_scale_batch(const void* points, uint64_t n, const void* k32, void* out_affine);
int wsnark_g2_scale_batch(const void* points, uint64_t n, const void* k32, void* out_affine);
typedef struct {
    uint64_t points[2], infinity[2], bad[2];   /* [0] = C, [1] = hExps */
    uint64_t first_bad[2];                      /* UINT64_MAX if none */
    uint32_t first_reason[2];                   /* WSNARK_PK_UNREDUCED / WSNARK_PK_OFF_CURVE */
    uint32_t ok;                                /* 1 iff no bad point and delta1, delta2 passed the audit's fixed-point tests */
    double   ms[3];                             /* device (upload + kernels + download), host (delta1', delta2', copies), whole call */
} wsnark_pkey_delta_report_t;
int wsnark_pkey_contribute(const void* pkey, size_t len, const void* d32, void* out_pkey, size_t out_cap, wsnark_pkey_delta_report_t* rep);
int wsnark_pkey_contribute_sections(const wsnark_key_sections_t* in, const void* d32,
                                    void* out_pointsC, void* out_pointsH, void* out_delta1_64, void* out_delta2_128,
                                    wsnark_pkey_delta_report_t* rep);
int wsnark_pkey_contribute_file(const char* in_path, const char* out_path, const void* d32, wsnark_pkey_delta_report_t* rep);
typedef struct {
    uint32_t checks_run, checks_bad;   /* bits 0..4 as above */
    uint32_t ok;                       /* 1 iff all five ran and none is bad */
    double   ms[3];                    /* sums, pairings, whole call */
} wsnark_pkey_delta_verdict_t;
int wsnark_pkey_delta_verify(const void* old_pkey, size_t old_len, const void* new_pkey, size_t new_len, const void* seed32,
                             wsnark_pkey_delta_verdict_t* out);
int wsnark_pkey_delta_verify_sections(const wsnark_key_sections_t* old_key, const wsnark_key_sections_t* new_key, const void* seed32,
                                      wsnark_pkey_delta_verdict_t* out);
int wsnark_pkey_delta_verify_file(const char* old_path, const char* new_path, const void* seed32, wsnark_pkey_delta_verdict_t* out);
/* ---- the first key of a ceremony from a powers-of-tau transcript (csrc/pkeysetup.hip; snarkjs: `zkey new`) ----
 * The step before the three above.  A key's points are the circuit's columns evaluated "in the exponent" on the Lagrange basis, and
 * L_i(tau) G = (1/n) sum_k w_n^(-ik) (tau^k G) is the inverse transform of the powers: wsnark_fr_ntt with points in place of field
 * elements (no counterpart in the reference, whose FFT is built over frm only).
 *   wsnark_g{1,2}_ntt         forward: out[i] = sum_k w_n^(ik) P_k;   inverse: out[i] = n^-1 sum_k w_n^(-ik) P_k.  w_n is the root
 *                             wsnark_fr_ntt uses (5^((r-1)/2^28) squared down); natural order in and out: this is
 *                             wsnark_fr_ntt(odd = 0, inverse) applied to the discrete logarithms.  points / out: host, n affine
 *                             Montgomery points of 64 (G1) / 128 (G2) bytes; out may be points.  x == 0 is infinity on input; a result
 *                             at infinity is written as zero bytes and every other result is affine and canonical: outputs compare
 *                             byte for byte.  n: a power of two, 1 <= n <= 2^24 (n == 1: the identity), else WSNARK_ERR_SIZE.  Every
 *                             input gets the audit's two cheap tests as in wsnark_g{1,2}_scale_batch (NOT the G2 subgroup test): a
 *                             bad point is WSNARK_ERR_FORMAT (wsnark_last_error names the first index), out is then untouched.
 *                             n/2 log2 n scalar multiplications, one butterfly per lane; needs wsnark_init (WSNARK_ERR_NOINIT) and
 *                             takes a lane of the context. */
int wsnark_g1_ntt(const void* points, uint64_t n, int inverse, void* out);
int wsnark_g2_ntt(const void* points, uint64_t n, int inverse, void* out);
/* wsnark_pkey_setup*: the key of a circuit under delta = 1 and gamma = 1 -- the key wsnark_pkey_contribute is then applied to.
 *   alfa1 = alpha_tau_g1[0], beta1 = beta_tau_g1[0], beta2 as given; delta1, delta2 (and the verification key's gamma2) are the
 *   standard generators.  With L1, L2, aL, bL the INVERSE group transforms of the first n entries of tau_g1, tau_g2, alpha_tau_g1,
 *   beta_tau_g1:   A_j = sum_i a_ji L1_i    B1_j = sum_i b_ji L1_i    B2_j = sum_i b_ji L2_i
 *                  K_j = sum_i a_ji bL_i + sum_i b_ji aL_i + sum_i c_ji L1_i:  C for j > nPublic, IC (the verification key's) for j <= nPublic
 *                  hExps_i = tau_g1[n + i] - tau_g1[i]
 *   polsA and polsB go into the key unchanged; polsC is not part of a proving key and is needed once, here.
 *   column sums               one lane per (signal, sum) walks the signal's records: coefficients are Montgomery in the stream and are
 *                             taken out of Montgomery form on the device; a zero coefficient adds nothing, repeated constraint indices
 *                             simply add, a signal without records is infinity (zero bytes).  A column with more than
 *                             WSNARK_PKSETUP_MSM_MIN records (default 32) has its points gathered and goes through the ordinary MSM
 *                             instead -- a real circuit's constant signal sits in 10^5 rows; the bytes do not depend on the switch.
 *   errors                    what the loaders reject fails before anything is written, the report untouched: nPublic + 1 > nVars
 *                             (WSNARK_ERR_FORMAT), domain not a power of two in [2, 2^24] or the two structs' domains different
 *                             (WSNARK_ERR_SIZE), an array shorter than its domain implies, a truncated record stream or a record
 *                             index >= domain, tau_g1[0] or tau_g2[0] not the generator (WSNARK_ERR_FORMAT); out_cap too small or a
 *                             key beyond proving_key.bin's 4 GiB (WSNARK_ERR_SIZE); before wsnark_init WSNARK_ERR_NOINIT.
 *   a bad power is a RESULT   as in the audit and the contribution: WSNARK_OK with ok = 0 for a power with a coordinate >= q or off
 *                             the curve (per array points / infinity / bad / first_bad / first_reason, reduced on the device; tau_g1
 *                             counts all its 2n entries) and for a beta2 that fails the audit's fixed-point tests.  The outputs are
 *                             then unspecified.
 * Not tested here: whether the powers ARE powers of one tau, and the G2 subgroup test of tau_g2 -- both are wsnark_powers_check's
 * (below): run it on a transcript before a key is built on it.  No .ptau / .r1cs readers (a finished key's .zkey has one: wsnark_zkey_import),
 * no file-to-file variant, one GPU.  Each call takes a lane of the context; nothing
 * else calls these functions and no other entry point changes. */
typedef struct {                 /* what a phase-1 transcript holds for a domain of n = `domain` */
    uint32_t domain;             /* power of two */
    const void* tau_g1;       uint64_t tau_g1_len;        /* 2n x 64 B : tau^k G1, k = 0 .. 2n-1 (hExps needs tau^(n+i)) */
    const void* tau_g2;       uint64_t tau_g2_len;        /*  n x 128 B: tau^k G2 */
    const void* alpha_tau_g1; uint64_t alpha_tau_g1_len;  /*  n x 64 B : alpha tau^k G1 */
    const void* beta_tau_g1;  uint64_t beta_tau_g1_len;   /*  n x 64 B : beta tau^k G1 */
    const void* beta_g2;                                   /*  128 B */
} wsnark_powers_t;
typedef struct {                 /* the circuit in the key's own column form: record streams of src/build_pol.js:62-144 */
    uint32_t n_vars, n_public, domain;
    const void* polsA; uint64_t polsA_len;
    const void* polsB; uint64_t polsB_len;
    const void* polsC; uint64_t polsC_len;                 /* not part of a proving key: needed once, here */
} wsnark_circuit_t;
enum { WSNARK_PW_TAU_G1 = 0, WSNARK_PW_TAU_G2 = 1, WSNARK_PW_ALPHA_TAU_G1 = 2, WSNARK_PW_BETA_TAU_G1 = 3 };      /* arrays in report order */
typedef struct {
    uint64_t points[4], infinity[4], bad[4];
    uint64_t first_bad[4];               /* UINT64_MAX if none */
    uint32_t first_reason[4];            /* WSNARK_PK_UNREDUCED / WSNARK_PK_OFF_CURVE */
    uint32_t beta2_reason;               /* 0 = good */
    uint32_t ok;                         /* 1 iff no bad power and beta2 passed */
    uint32_t msm_columns;                /* column sums that went through the MSM */
    uint32_t reserved;
    double   ms[4];                      /* transforms (with the upload and the input tests), column sums, hExps, whole call */
} wsnark_pkey_setup_report_t;
/* the sections as wsnark_pkey_load_sections reads them: nVars, nVars, nVars (128 B each), nVars - nPublic - 1 and domain points; the
 * five fixed points; out_ic: (nPublic + 1) x 64 B.  out_pointsC may be NULL when nVars == nPublic + 1. */
int wsnark_pkey_setup(const wsnark_powers_t* powers, const wsnark_circuit_t* circuit,
                      void* out_pointsA, void* out_pointsB1, void* out_pointsB2, void* out_pointsC, void* out_pointsH,
                      void* out_alfa1_64, void* out_beta1_64, void* out_delta1_64, void* out_beta2_128, void* out_delta2_128,
                      void* out_ic, wsnark_pkey_setup_report_t* rep);
/* the same key as a whole proving_key.bin in out_pkey[0 .. *out_len); wsnark_pkey_setup_size gives the length without any device work */
int wsnark_pkey_setup_pkey(const wsnark_powers_t* powers, const wsnark_circuit_t* circuit, void* out_pkey, size_t out_cap, size_t* out_len,
                           void* out_ic, wsnark_pkey_setup_report_t* rep);
int wsnark_pkey_setup_size(const wsnark_circuit_t* circuit, size_t* out_len);
/* ---- a key against its circuit and its powers of tau (csrc/pkeycircuit.hip; snarkjs: `zkey verify <r1cs> <ptau> <zkey>`) ----
 * Is this the key of THIS circuit on THIS transcript?  Before the first contribution wsnark_pkey_setup and a byte compare answer
 * that, at the price of four group transforms; afterwards C and hExps are scaled by an unknown 1/delta and only a replay of every
 * wsnark_pkey_delta_verify would.  This check needs neither: with rho_j = ChaCha20(seed32, counter j) for signal j < nVars (the audit's
 * generator), u_M = (rows of matrix M) . rho and c(x) = fromMontgomery(iNTT(x)),
 *     sum_j rho_j A_j = sum_i u_A,i L_i(tau) G = sum_k c(u_A)_k tau^k G
 * -- a transform over the FIELD, not the group.  Split by public and private signal (p_M: columns j <= nPublic, v_M: j > nPublic,
 * u_M = p_M + v_M; one walk of every row, lc_split_kernel), n = domain, np = nPublic, rho'_i = the generator at counter nVars + i:
 *   bit 0  the key's nVars, nPublic and domainSize equal the circuit's, and its polsA and polsB are the circuit's byte for byte (host
 *          memcmp).  If the COUNTS differ the bit is bad and nothing else runs.
 *   bit 1  alfa1 == alpha_tau_g1[0], beta1 == beta_tau_g1[0], beta2 == beta_g2 (bytes)
 *   bit 2  e(delta1, G2) = e(G1, delta2); run only if both pass the audit's fixed-point tests
 *   bit 3  sum_j rho_j A_j  == sum_k c(u_A)_k tau_g1[k]      (equality of the normalised sums, no pairing)
 *   bit 4  sum_j rho_j B1_j == sum_k c(u_B)_k tau_g1[k]      bit 5  sum_j rho_j B2_j == sum_k c(u_B)_k tau_g2[k]
 *   bit 6  e(sum_{j>np} rho_j C_j, delta2) = e(K_v, G2),  K_v = sum_k [c(v_A)_k beta_tau_g1[k] + c(v_B)_k alpha_tau_g1[k] + c(v_C)_k tau_g1[k]];
 *          point k of the C section is signal np + 1 + k and is weighted by THAT rho.  nVars == np + 1: two points at infinity, holds.
 *   bit 7  e(sum_i rho'_i hExps_i, delta2) = e(sum_i rho'_i tau_g1[n + i] - sum_i rho'_i tau_g1[i], G2)
 *          Bits 6 and 7 run only if bit 2 ran and held: that is what makes them mean something.
 *   bit 8  vk given: n_inputs == nPublic, and the vk's alfa1, beta2, delta2 are the key's (after conversion to Montgomery form)
 *   bit 9  vk given: e(sum_{j<=np} rho_j IC_j, gamma2) = e(K_p, G2), K_p as K_v over p_A, p_B, p_C; run only if n_inputs == nPublic and
 *          the vk's gamma2 and IC points pass the audit's fixed-point tests.
 *   vk: the layout wsnark_groth16_verify reads (plain: alfa1 | beta2 | gamma2 | delta2 | IC[0 .. n_inputs]); NULL: bits 8 and 9 are not
 *   requested.  ok = 1 iff every requested bit ran and none is bad; a bit that did not run stays clear in checks_run.
 *   seed32 == NULL: 32 bytes from the OS.  Each relation is sound with probability 1 - 2^-128 over a seed the key's author did NOT
 *   know; a fixed or published seed gives no soundness.
 *   The check does NOT test individual points: that is wsnark_pkey_check's job on the key and wsnark_powers_check's on the transcript.
 *   Unreduced or off-curve bytes do not fault it, they only make the sums meaningless.  It cannot tell whether the circuit is the
 *   intended one, nor who contributed.
 *   streaming   key sections and transcript arrays go through the staging ring in chunks of WSNARK_PKCIRCUIT_CHUNK points (default
 *               2^18, clamped to [64, 2^22]; no verdict depends on it).  The three CSR matrices and the six domain-length vectors are
 *               resident for the call (the nVars weights only while the row sums run), everything else is bounded by the chunk; the
 *               sums are the ordinary MSMs, partial sums added on the host.  The file variant maps the key read-only and hands every
 *               staged range back.  Each call takes one lane; no other entry point changes.
 *   errors      what the loaders and wsnark_pkey_setup reject fails with their code before anything is written, the verdict untouched
 *               (a short section or array, a truncated stream, a record index >= domain, a domain that is no power of two in
 *               [2, 2^24], the two structs' domains differing, tau_g1[0] / tau_g2[0] not the generators); a NULL pointer WSNARK_ERR_ARG;
 *               a vk shorter than n_inputs + 1 IC points WSNARK_ERR_SIZE; before wsnark_init WSNARK_ERR_NOINIT.  A wrong key is a
 *               RESULT: WSNARK_OK with ok = 0.
 * wsnark_circuit_row_sums: the building block -- the six vectors themselves for caller-given weights (nVars x 32 B plain, any 256-bit
 *   value): out_public = p_A | p_B | p_C, out_private = v_A | v_B | v_C, 3 x domain x 32 B each, Montgomery and canonical. */
typedef struct {
    uint32_t checks_run, checks_bad;   /* bits 0..9 as above */
    uint32_t ok, reserved;
    double   ms[5];                    /* matrices (CSR + row sums + transforms), key-side sums, transcript-side sums, pairings, whole call */
} wsnark_pkey_circuit_verdict_t;
int wsnark_pkey_circuit_check(const void* pkey, size_t len, const wsnark_powers_t* powers, const wsnark_circuit_t* circuit,
                              const void* vk, size_t vk_len, uint64_t n_inputs, const void* seed32, wsnark_pkey_circuit_verdict_t* out);
int wsnark_pkey_circuit_check_sections(const wsnark_key_sections_t* key, const wsnark_powers_t* powers, const wsnark_circuit_t* circuit,
                                       const void* vk, size_t vk_len, uint64_t n_inputs, const void* seed32,
                                       wsnark_pkey_circuit_verdict_t* out);
int wsnark_pkey_circuit_check_file(const char* path, const wsnark_powers_t* powers, const wsnark_circuit_t* circuit,
                                   const void* vk, size_t vk_len, uint64_t n_inputs, const void* seed32, wsnark_pkey_circuit_verdict_t* out);
int wsnark_circuit_row_sums(const wsnark_circuit_t* circuit, const void* weights, void* out_public, void* out_private);
/* ---- a witness against its circuit: which constraints fail (csrc/witcheck.hip; snarkjs: `wtns check <r1cs> <wtns>`) ----
 * wsnark_groth16_prove evaluates a = A.w and b = B.w and takes a o b on the domain as C.w: a proving key holds no C matrix, so a witness
 * that breaks a constraint proves like any other, and every verifier rejects the proof without saying why.  This is the step between
 * the witness generator and the prover: row i is bad iff (A_i.w)(B_i.w) != C_i.w mod r.
 *   wsnark_circuit_load           the circuit's three matrices resident as row-major CSR on the calling thread's device (the loaders'
 *                                 transposition); wsnark_circuit_info reads the counts, the three record counts and the device bytes
 *                                 back (any out pointer may be NULL); wsnark_circuit_free(NULL) is ignored.  The handle is read-only
 *                                 after the load.
 *   wsnark_circuit_witness_check  witness: host, nVars x 32 B plain LE, any 256-bit values -- signals >= r are reduced mod r for the
 *                                 check, as the prover reduces them, and counted in `unreduced`.  witness_len < nVars x 32 is
 *                                 WSNARK_ERR_SIZE; a longer buffer is accepted and only nVars signals are read, as in
 *                                 wsnark_groth16_prove.  One lane per row (lc_check_kernel): a wavefront's 64 verdicts leave as one word
 *                                 of a bad-row bitmask, the count and the smallest bad index are reduced on the device.
 *   bad_rows / bad_values         cap x u64, ascending, the SMALLEST bad indices; cap x 96 B, a | b | c of that row, plain LE and
 *                                 canonical.  listed = min(bad, cap) entries are written, the rest is left as it was.  cap == 0: both
 *                                 may be NULL.  The bitmask (domain / 8 bytes) comes to the host only when bad > 0 && cap > 0; a good
 *                                 witness costs one small download.
 *   wsnark_circuit_witness_check_dev   the witness already on the handle's device: d_witness is memory of THAT device (the one
 *                                 wsnark_circuit_load ran on), 16-byte aligned -- the kernels read whole 32-byte elements; a
 *                                 misaligned pointer is WSNARK_ERR_ARG; stream: the queue d_witness is ready on, a queue of that same
 *                                 device (NULL = the lane's own).  The lists and the report are host memory; the call returns when they are written.
 *   wsnark_witness_check          load, check and free in one call: the same report and lists, the matrices' time in ms[0].
 *   A bad witness is a RESULT: WSNARK_OK with ok = 0.
 *   errors      what wsnark_circuit_row_sums rejects of a circuit is rejected with the same codes (nPublic + 1 > nVars, a truncated
 *               stream, a record index >= domain: WSNARK_ERR_FORMAT; a domain that is no power of two in [2, 2^24]: WSNARK_ERR_SIZE); a
 *               NULL circuit, handle, witness or report, or cap > 0 with a NULL list: WSNARK_ERR_ARG; before wsnark_init
 *               WSNARK_ERR_NOINIT.  On every error the report and the lists are left untouched.
 *   threads     each call takes a lane; the bitmask, the counters and the witness copy belong to the call, not to the handle: two
 *               threads may check two witnesses on one handle at once.
 *   Out of scope: group (multi-GPU) handles; readers of .r1cs / .wtns files; whether the circuit's A and B are a given key's (that is
 *   bit 0 of wsnark_pkey_circuit_check); no wsnark_groth16_prove* entry point changes. */
typedef struct wsnark_circuit_res wsnark_circuit_res_t;      /* a circuit's three matrices resident as row-major CSR */
int  wsnark_circuit_load(const wsnark_circuit_t* circuit, wsnark_circuit_res_t** out_handle);
void wsnark_circuit_free(wsnark_circuit_res_t* handle);       /* NULL is ignored */
int  wsnark_circuit_info(const wsnark_circuit_res_t* h, uint32_t* n_vars, uint32_t* n_public, uint32_t* domain,
                         uint64_t nnz[3], uint64_t* bytes);   /* any out pointer may be NULL */
typedef struct {
    uint64_t rows;                  /* = domain */
    uint64_t bad;                   /* rows with (A_i.w)(B_i.w) != C_i.w mod r */
    uint64_t first_bad;             /* UINT64_MAX if none */
    uint64_t listed;                /* min(bad, cap): entries written to bad_rows / bad_values */
    uint64_t unreduced;             /* signals >= r (they are reduced mod r for the check, as the prover reduces them) */
    uint64_t first_unreduced;       /* UINT64_MAX if none */
    uint32_t one_ok;                /* witness[0] == 1 */
    uint32_t ok;                    /* 1 iff bad == 0, one_ok, and no signal of index <= nPublic is >= r
                                       (wsnark_groth16_verify rejects such a public input) */
    double   ms[3];                 /* matrices (0 on a resident circuit), device (upload + kernels + download), whole call */
} wsnark_witness_report_t;
int wsnark_witness_check(const wsnark_circuit_t* circuit, const void* witness, size_t witness_len,
                         uint64_t* bad_rows, void* bad_values, uint64_t cap, wsnark_witness_report_t* rep);
int wsnark_circuit_witness_check(wsnark_circuit_res_t* h, const void* witness, size_t witness_len,
                                 uint64_t* bad_rows, void* bad_values, uint64_t cap, wsnark_witness_report_t* rep);
int wsnark_circuit_witness_check_dev(wsnark_circuit_res_t* h, const void* d_witness, size_t witness_len,
                                     uint64_t* bad_rows_host, void* bad_values_host, uint64_t cap,
                                     wsnark_witness_report_t* rep, void* stream);
/* ---- many witnesses against ONE resident circuit in one call (csrc/witcheck.hip) ----
 * The batch counterpart of wsnark_circuit_witness_check, beside wsnark_groth16_prove_batch: N calls of the single check are N memsets,
 * 2 N launches of a handful of workgroups and N synchronising downloads; this is one memset, two launches and one download per pass.
 * THE CONTRACT: for every i, verdicts[i] and witness i's lists are field for field what
 *   wsnark_circuit_witness_check(h, witnesses + i * witness_stride, nVars * 32, rows_i, values_i, cap, &r)
 * reports: bad, first_bad, unreduced, first_unreduced, listed, one_ok, ok; bad_rows[i * cap .. i * cap + listed_i) ascending, the
 * SMALLEST bad indices of witness i; bad_values[(i * cap) * 96 ..) a | b | c of those rows, plain LE and canonical.  Signals >= r are
 * reduced for the check and counted.  List entries beyond listed_i are left as they were.  Nothing in a result depends on the launch
 * geometry or on the pass size.
 *   witnesses     count witnesses, witness i at witnesses + i * witness_stride; only its first nVars signals are read.
 *                 witness_stride < nVars * 32: WSNARK_ERR_SIZE.  count == 0: WSNARK_OK, nothing is touched.  count > 2^16:
 *                 WSNARK_ERR_SIZE.
 *   lists         bad_rows: count x cap u64; bad_values: count x cap x 96 B.  cap == 0: both may be NULL.
 *   rep           may be NULL.
 *   _dev          the witnesses are memory of the handle's device, ready on `stream` (NULL = the lane's own queue), and are read in
 *                 place; pointer and stride are multiples of 16, else WSNARK_ERR_ARG.  The verdicts, lists and report are host
 *                 memory; the call returns when they are written.
 *   passes        a host batch goes through the staging ring in passes of `chunk` witnesses under a fixed byte budget
 *                 (WITCHECK_BATCH_CHUNK, through wsnark_tuning_set or the environment, read per call); a device batch is read in place
 *                 and the chunk only bounds the masks, the counters and the lists.  A pass costs one memset, two launches and one
 *                 download of chunk x 48 B; with cap > 0 and bad witnesses in it, one gather of THEIR bitmasks (one launch, one
 *                 download) and one launch and one download for all listed rows of the pass -- whatever the number of bad witnesses.
 *                 count == 1 is handed to the single check (chunk = 1): the one shape a pass of its own lost to it.
 *   domains < 64  every witness takes one whole wavefront of lc_check_batch_kernel, lanes domain .. 63 idle: no ballot word and no
 *                 counter is shared by two witnesses.
 *   A bad witness is a RESULT: WSNARK_OK with ok = 0 in its verdict.
 *   errors        a NULL handle, witnesses or verdicts, or cap > 0 with a NULL list: WSNARK_ERR_ARG; before wsnark_init
 *                 WSNARK_ERR_NOINIT.  On every error the verdicts, the lists and the report are left untouched (they are written last).
 *   threads       everything a call writes on the device belongs to the lane it holds: two threads may run batches on one handle at
 *                 once.  Each path waits for its queue before the lane goes back.
 *   Out of scope: group handles; whether the circuit is a given key's (bit 0 of wsnark_pkey_circuit_check). */
typedef struct {                    /* one per witness: the fields of wsnark_witness_report_t that belong to a witness */
    uint64_t bad, first_bad;        /* first_bad: UINT64_MAX if none */
    uint64_t unreduced, first_unreduced;
    uint64_t listed;                /* min(bad, cap) */
    uint32_t one_ok, ok;
} wsnark_witness_verdict_t;
typedef struct {
    uint64_t count, rows;           /* rows = domain */
    uint64_t good;                  /* witnesses with ok = 1 */
    uint64_t first_not_ok;          /* smallest i with ok = 0, UINT64_MAX if none */
    uint32_t chunk, reserved;       /* witnesses per pass */
    double   ms[3];                 /* 0 (the circuit is resident), device (upload + kernels + download), whole call */
} wsnark_witness_batch_report_t;
int wsnark_circuit_witness_check_batch(wsnark_circuit_res_t* h, const void* witnesses, size_t witness_stride, uint64_t count,
                                       wsnark_witness_verdict_t* verdicts, uint64_t* bad_rows, void* bad_values, uint64_t cap,
                                       wsnark_witness_batch_report_t* rep);
int wsnark_circuit_witness_check_batch_dev(wsnark_circuit_res_t* h, const void* d_witnesses, size_t witness_stride, uint64_t count,
                                           wsnark_witness_verdict_t* verdicts_host, uint64_t* bad_rows_host, void* bad_values_host,
                                           uint64_t cap, wsnark_witness_batch_report_t* rep, void* stream);
/* ---- circuits in ROW form: column streams and the resident CSR from constraints (csrc/circuitrows.hip) ----
 * wsnark_circuit_t holds a circuit in the proving key's own column form, which only a key (A and B) or wasmsnark_amd/synth.py emits.
 * Every front end produces constraints row by row: this is the way in.  A matrix is CSR over the constraints as given.
 *   wsnark_circuit_from_rows_size   host work only (no wsnark_init needed): *domain and lens[M] = 4 * n_vars + 36 * (nnz_M [+ n_public
 *                                 + 1 for A with WSNARK_ROWS_PUBLIC_ROWS]).  Records are kept as given -- nothing is merged or dropped.
 *   wsnark_circuit_from_rows      the three record streams of wsnark_circuit_t.  THE CONTRACT, byte for byte: for every signal in index
 *                                 order `u32 ncoefs`, then its records (u32 row, 32 B coefficient) with ASCENDING row; equal rows (a
 *                                 signal listed twice in one constraint) keep the order in which the input lists them.  The coefficient
 *                                 is (c mod r) R mod r, canonical; a coefficient that is 0 mod r stays as a record with zero bytes.
 *                                 Nothing in the output depends on launch geometry, tile size or the arrival order of atomics.
 *   the scheme                    entries go up through the staging ring; per matrix a STABLE least-significant-digit radix sort of
 *                                 (signal, entry index) pairs by signal, 6 bits per pass and as many passes as n_vars has bits / 6:
 *                                 a pass ranks a tile's entries in LDS (one run of consecutive entries per lane, counters per (digit,
 *                                 lane), one scan in digit-major order) and adds the scanned per-(digit, tile) bases.  No order comes
 *                                 from an atomic, and a column with 10^6 records costs what 10^6 columns with one record cost.  The
 *                                 emit stages 256 sorted records of 9 words in LDS and stores them with 32-bit stores in output order;
 *                                 a signal's header comes from two binary searches in the sorted pairs (the position IS the offset).
 *                                 ROWS_TILE (wsnark_tuning_set or WSNARK_ROWS_TILE, read per call): entries per tile, a multiple of
 *                                 256 in [256, 4096], default 2048; any other value is WSNARK_ERR_ARG.  No byte depends on it.
 *   wsnark_circuit_load_rows      the handle wsnark_circuit_load returns, built directly: row_ptr / col / coef go up, one kernel puts
 *                                 the coefficients into the resident form (c R^2) and appends the public rows; no transposition.  Every
 *                                 wsnark_circuit_witness_check* and wsnark_circuit_info result on it is field for field that of the
 *                                 handle loaded from the streams wsnark_circuit_from_rows writes.
 *   rep                           nnz: records written per matrix (the public rows included); unreduced: input coefficients >= r;
 *                                 zero: input coefficients that reduce to 0; empty_signals: signals without a record; max_column: the
 *                                 longest column; ms: upload, kernels, download, whole call, by the host clock between waits for
 *                                 the queue (whole call: with the one device allocation the call makes and frees; the download goes
 *                                 into the caller's memory as it is, pageable or pinned).
 *   errors      nothing is written on any of them, the report is left untouched: a NULL struct, array or output WSNARK_ERR_ARG (also
 *               unknown flag bits); n_public + 1 > n_vars, row_ptr[0] != 0 or decreasing, a col >= n_vars WSNARK_ERR_FORMAT (the last
 *               one found on the device by a min-reduction: wsnark_last_error names the matrix and the smallest entry index); a domain
 *               that is no power of two, below the total rows or outside [2, 2^24], a matrix of 2^32 records or more, n_vars > 2^30, a
 *               capacity below lens[M] WSNARK_ERR_SIZE; before wsnark_init WSNARK_ERR_NOINIT.
 *   threads     each call takes one lane; scratch belongs to the call.
 *   Out of scope: readers of .r1cs and snarkjs JSON files (a front end packs its constraints into wsnark_rows_t:
 *   wasmsnark_amd/formats.py rows_from_constraints; a .zkey and a .wtns have their readers below); merging repeated signals of a row; group (multi-GPU) handles; no other entry
 *   point changes. */
typedef struct {                      /* one matrix, CSR over the constraints as given */
    const uint64_t* row_ptr;          /* n_constraints + 1 entries, row_ptr[0] == 0, non-decreasing */
    const uint32_t* col;              /* row_ptr[n_constraints] signal indices */
    const void*     coef;             /* as many x 32 B, PLAIN little-endian, any 256-bit value: reduced mod r */
} wsnark_rows_matrix_t;
typedef struct {
    uint32_t n_vars, n_public, n_constraints;
    uint32_t domain;                  /* 0 = the smallest power of two >= max(total rows, 2); else a power of two >= total rows */
    wsnark_rows_matrix_t A, B, C;
} wsnark_rows_t;
#define WSNARK_ROWS_PUBLIC_ROWS 1u    /* append the nPublic + 1 input-binding rows: row n_constraints + i of A = {signal i: 1}, B and C empty */
typedef struct {
    uint64_t nnz[3], unreduced[3], zero[3], empty_signals[3], max_column[3];
    double   ms[4];                   /* upload, kernels, download, whole call */
} wsnark_rows_report_t;
int wsnark_circuit_from_rows_size(const wsnark_rows_t* rows, uint32_t flags, uint32_t* domain, uint64_t lens[3]);
int wsnark_circuit_from_rows(const wsnark_rows_t* rows, uint32_t flags, void* out_polsA, uint64_t capA, void* out_polsB, uint64_t capB,
                             void* out_polsC, uint64_t capC, uint32_t* domain, wsnark_rows_report_t* rep);
int wsnark_circuit_load_rows(const wsnark_rows_t* rows, uint32_t flags, wsnark_circuit_res_t** out_handle);
/* ---- snarkjs' .zkey in and out; the H basis change (csrc/zkey.hip) ----
 * What circom / snarkjs / rapidsnark users hold is a .zkey and a .wtns, not proving_key.bin and witness.bin.  Two sections of a .zkey
 * are in another FORM than the key's: the coefficients are one flat list of (matrix, constraint, signal, value) records in row order
 * with A and B interleaved (the key wants one column stream per matrix), and H holds the odd Lagrange points of the doubled domain,
 * N_i = (L^{2n}_{2i+1}(tau) / delta) G1, where CALC_H's sum wants hExps_k = (tau^k (tau^n - 1) / delta) G1.  With n = domainSize, w_n
 * the root wsnark_fr_ntt uses, w_2n^2 = w_n:
 *       hExps_k = (-2 w_2n^k) sum_i w_n^(ik) N_i              N_i = sum_k w_n^(-ik) (-(2n)^-1 w_2n^(-k)) hExps_k
 * -- a group transform and one scalar per point, the latter BEHIND the stages on the way in and IN FRONT of them on the way out, where
 * it carries the inverse's 1/n as well.  The layout of the container, the sections, the points (proving_key.bin's own: sections
 * 5 - 8 and the fixed points are copied byte for byte) and the coefficient values (c R^2 mod r in a .zkey, c R mod r in a key) is
 * README.md's "zkey" section.
 *   wsnark_g1_h_basis          points / out: host, n points of 64 B as in wsnark_g1_ntt (out may be points); to_lagrange = 0: N -> hExps,
 *                              1: hExps -> N.  n a power of two in [2, 2^24], else WSNARK_ERR_SIZE.  Every input gets the audit's two
 *                              cheap tests; a bad point is WSNARK_ERR_FORMAT, wsnark_last_error names the first index, out untouched.
 *                              Outputs are canonical affine, infinity as zero bytes.  The points stay on the device from upload to
 *                              download: load, stages, twist are wsnark_g1_ntt's and wsnark_g1_mul_batch's kernels.
 *   wsnark_zkey_info           host only, no wsnark_init: the header's numbers, records per matrix, contributions, the length of the
 *                              proving_key.bin (may be 2^32 or more: then only the sections variant imports it) and of the vk.
 *   wsnark_zkey_import         the key as proving_key.bin in out_pkey[0 .. *out_len) and the verification key in out_vk (the layout
 *                              wsnark_groth16_verify reads, plain: alfa1 | beta2 | gamma2 | delta2 | IC[0 .. nPublic]).
 *   wsnark_zkey_import_sections the same key as twelve separate buffers for keys past 4 GiB, in this order with their capacities:
 *                              polsA, polsB, then wsnark_pkey_setup's pointsA, pointsB1, pointsB2, pointsC, pointsH, alfa1, beta1,
 *                              delta1, beta2, delta2 (IC goes into out_vk).  pointsC may be NULL when nVars == nPublic + 1.
 *     streams                  every signal's records have ascending constraint, equal constraints keep file order, a zero value
 *                              stays as a record, a value >= r is reduced and counted.  The nPublic + 1 input-binding rows are
 *                              already records of section 4: nothing is appended.  One kernel reads the 44-byte records, takes the
 *                              value out of one Montgomery factor and partitions STABLY by matrix (a block scan of the matrix flag
 *                              plus scanned per-tile bases; no order comes from an atomic); the stable radix sort and the emit are
 *                              wsnark_circuit_from_rows'.  Where a matrix's records are not non-decreasing in constraint (snarkjs
 *                              always writes them so), passes over the constraint bits run first: the result is that of the file
 *                              stably sorted by constraint.  ROWS_TILE as above; no byte depends on it.
 *     validation               before anything is written, WSNARK_ERR_FORMAT with a text that names it: bad magic, version or
 *                              protocol (PLONK and FFLONK ids included), n8q or n8r != 32, q or r not BN128's, nPublic + 1 > nVars, a
 *                              section size that does not match its counts, a truncated file, a required section (1 - 9) missing or
 *                              any section present twice, matrix > 1, signal >= nVars, constraint >= domainSize (the last two
 *                              found on the device by a min-reduction), a bad point of H (unreduced or off the curve, with its
 *                              index).  Unknown section types are skipped; sections may come in any order.  WSNARK_ERR_SIZE: a
 *                              domainSize that is no power of two in [2, 2^24], a capacity that is too small, a key past 4 GiB in the
 *                              proving_key.bin variant.  On every error the outputs and the report are untouched.
 *     NOT audited              sections 3 and 5 - 8 and the fixed points are copied, not tested: that is wsnark_pkey_check's job, to be
 *                              run on the imported key before it is trusted.
 *   wsnark_zkey_export*        sections 1 - 10 in numeric order.  Section 4 by ascending constraint; inside a constraint matrix 0's records
 *                              by ascending signal (equal signals in stream order), then matrix 1's: one stable sort by constraint
 *                              of the two streams' records, then an emit that multiplies by R and stores the 44-byte records
 *                              with 32-bit stores in output order.  gamma2 and IC come from vk (the verifier's layout, n_inputs =
 *                              nPublic, else WSNARK_ERR_ARG; vk == NULL is WSNARK_ERR_ARG).  Section 10 is 64 zero bytes and n = 0: the
 *                              circuit hash is over data a key does not hold, so `snarkjs zkey verify` rejects the file while
 *                              provers take it.  wsnark_zkey_export_size: the length, host only.
 *   rep                        records / unreduced / zero per matrix; sorted: 1 iff every matrix's records were already in constraint
 *                              order (always 1 on export); the H array's points / infinity / bad / first_bad / first_reason; ms:
 *                              parse + upload, coefficients, H basis, download, whole call.
 *   Each call takes one lane; before wsnark_init WSNARK_ERR_NOINIT (not wsnark_zkey_info and _export_size).  No other entry point
 *   changes.  Out of scope: .r1cs and .ptau readers, a faithful section 10, other protocols, groups (multi-GPU). */
typedef struct {
    uint32_t n_vars, n_public, domain, n_coeffs;
    uint64_t records[2];                 /* section 4's records of matrix 0 (A) and 1 (B) */
    uint32_t n_contributions, reserved;
    uint64_t pkey_len;                   /* the proving_key.bin this key makes */
    uint64_t vk_len;                     /* 448 + 64 (nPublic + 1) */
} wsnark_zkey_info_t;
typedef struct {
    uint64_t records[2], unreduced[2], zero[2];
    uint32_t sorted, reserved;
    uint64_t h_points, h_infinity, h_bad;
    uint64_t h_first_bad;                /* UINT64_MAX if none */
    uint32_t h_first_reason, reserved2;
    double   ms[5];                      /* parse + upload, coefficients, H basis, download, whole call */
} wsnark_zkey_report_t;
int wsnark_g1_h_basis(const void* points, uint64_t n, int to_lagrange, void* out);
int wsnark_zkey_info(const void* zkey, size_t len, wsnark_zkey_info_t* out);
int wsnark_zkey_import(const void* zkey, size_t len, void* out_pkey, size_t cap, size_t* out_len,
                       void* out_vk, size_t vk_cap, wsnark_zkey_report_t* rep);
int wsnark_zkey_import_sections(const void* zkey, size_t len, void* const out[12], const uint64_t caps[12],
                                void* out_vk, size_t vk_cap, wsnark_zkey_report_t* rep);
int wsnark_zkey_export(const void* pkey, size_t len, const void* vk, size_t vk_len, uint64_t n_inputs,
                       void* out_zkey, size_t cap, size_t* out_len, wsnark_zkey_report_t* rep);
int wsnark_zkey_export_sections(const wsnark_key_sections_t* key, const void* vk, size_t vk_len, uint64_t n_inputs,
                                void* out_zkey, size_t cap, size_t* out_len, wsnark_zkey_report_t* rep);
int wsnark_zkey_export_size(uint32_t n_vars, uint32_t n_public, uint32_t domain, uint64_t nnzA, uint64_t nnzB, size_t* out_len);
/* ---- a .zkey straight into a resident proving key (csrc/zkey.hip: zkey_load; the seam in csrc/prove.hip) ----
 * prove(zkey, wtns) without the way through proving_key.bin: what wsnark_zkey_import followed by wsnark_pkey_load computes, with nothing
 * of the key coming back to the host except the verification key.
 *   handle       a whole-key wsnark_pkey_t (rank 0 of 1): every call that takes wsnark_pkey_load's handle takes this one with the same
 *                results -- _info, _table_info, _wait_tables, _load_stats, _shard_info, wsnark_groth16_prove[_dev], _prove_batch[_dev],
 *                wsnark_pkey_eval_ab_dev, _prove_partial*, _prove_finish, wsnark_pkey_free.  The tables are built in the background as
 *                for any load; WSNARK_KEY_TABLE, _TABLE_MAX_GB and _TABLE_ASYNC apply.  _load_stats: [0] the coefficients, [1] parse +
 *                upload, [2] masks + conversion, [3] the table build, [4] the call from the first allocation on.
 *   points       sections 5 - 8 go through the staging ring into row 0 of the handle's tables (C behind its nPublic + 1 infinities);
 *                section 9 into H's, where the basis change above runs in place (N -> hExps), its scratch freed before the call returns.
 *   coefficients the 44-byte records go up as they are.  The import's count / test and STABLE partition by matrix run on them, with the
 *                value kept as the file stores it, c R^2 mod r -- what the resident matrices hold (a value >= r is reduced and counted,
 *                no Montgomery factor is taken off).  A matrix's partition then IS col[] (the signal) and coef[] of the prover's
 *                row-major CSR: snarkjs writes the records by ascending constraint.  Where a matrix's records are not non-decreasing in
 *                constraint the import's stable radix passes over the constraint bits run first.  row_ptr[k], k = 0 .. domainSize, is
 *                the number of records with constraint < k: one lane per k, a binary search, plain stores.  No order comes from an
 *                atomic: inside a row the entries are in file order.  Rows without records, a matrix without records and nCoeffs = 0
 *                give valid matrices.
 *   out_vk       wsnark_groth16_verify's layout, as wsnark_zkey_import writes it; NULL with vk_cap == 0: not wanted.  Its length,
 *                448 + 64 (nPublic + 1), comes from wsnark_zkey_vk_len / _vk_len_file: host only, no wsnark_init, read from the container
 *                and section 2 ALONE -- wsnark_zkey_info gives it too, but counts section 4's records on the host, which would fault
 *                the largest section of a mapped file into the process.  Their errors are the container's, with the texts above.
 *   rep          wsnark_zkey_report_t as on import, or NULL; ms: parse + upload, coefficients, H basis, 0 (nothing is downloaded), the
 *                whole call up to "proofs may start".
 *   errors       wsnark_zkey_import's, codes and texts, the "zkey import:" prefix of two of them included (the container, the sizes, matrix > 1, signal >= nVars and constraint >=
 *                domainSize with the record, a bad H point with its index); WSNARK_ERR_SIZE: a domainSize that is no power of two in
 *                [2, 2^24], vk_cap too small; WSNARK_ERR_ARG: a file that cannot be opened, zkey / path / out_handle NULL;
 *                WSNARK_ERR_NOINIT before wsnark_init.  On every error *out_handle, out_vk and rep are untouched and nothing stays
 *                allocated.
 *   _file        the file is mapped read-only; the sections are found by type, in any order, unknown types skipped; every range is
 *                staged in pieces (WSNARK_POLS_PIECE_KB) and handed back to the kernel piece by piece, so the process never holds the
 *                key: keys past 4 GiB, up to domainSize 2^24.  An empty or too short file is the container's "truncated file".
 *   NOT audited  as on import: sections 3 and 5 - 8 and the fixed points are taken as they are (wsnark_pkey_check on imported bytes is
 *                the audit); H gets the two cheap tests of its basis change.  The .zkey reading has still not met a file written by
 *                snarkjs: the model file of the tests follows README.md's "zkey" section.  Out of scope: shards, groups (multi-GPU). */
int wsnark_pkey_load_zkey(const void* zkey, size_t len, wsnark_pkey_t** out_handle,
                          void* out_vk, size_t vk_cap, wsnark_zkey_report_t* rep);
int wsnark_pkey_load_zkey_file(const char* path, wsnark_pkey_t** out_handle,
                               void* out_vk, size_t vk_cap, wsnark_zkey_report_t* rep);
int wsnark_zkey_vk_len(const void* zkey, size_t len, size_t* out_len);
int wsnark_zkey_vk_len_file(const char* path, size_t* out_len);
/* ---- powers of tau: contribute to a transcript, audit one (csrc/pwtau.hip; snarkjs: `powersoftau contribute` / `powersoftau verify`) ----
 * Phase 1 itself: the transcript wsnark_pkey_setup builds a key on.  A contribution by secrets t, a, b (non-zero mod r) turns the
 * transcript of (tau, alpha, beta) into the one of (t tau, a alpha, b beta):
 *   tau_g1'[k] = t^k tau_g1[k], k < 2n      tau_g2'[k] = t^k tau_g2[k], k < n
 *   alpha_tau_g1'[k] = a t^k alpha_tau_g1[k]      beta_tau_g1'[k] = b t^k beta_tau_g1[k]      beta_g2' = b beta_g2 (host curve)
 * -- a DIFFERENT scalar for every point: the third shape beside wsnark_g{1,2}_mul_base_batch (one base, many scalars) and
 * wsnark_g{1,2}_scale_batch (many bases, one scalar).
 *   wsnark_g{1,2}_mul_batch   out[i] = scalars[i] * points[i].  points / out: host, n affine Montgomery points of 64 (G1) / 128 (G2)
 *                             bytes, x == 0 is infinity and is copied through byte for byte; scalars: n x 32 bytes plain LE, NOT
 *                             required to be below r: reduced mod r.  A result at infinity (a scalar that is 0 mod r) is written as
 *                             zero bytes, every other result is affine and canonical: outputs compare byte for byte.  out may be
 *                             points.  Every input gets the audit's two cheap tests as in wsnark_g{1,2}_scale_batch (coordinates < q,
 *                             the curve equation; NOT the G2 subgroup test): a bad point is WSNARK_ERR_FORMAT (wsnark_last_error
 *                             names the first index and the count), out is then untouched.  n == 0: WSNARK_OK, nothing is touched;
 *                             n > 2^24: WSNARK_ERR_SIZE; a NULL pointer: WSNARK_ERR_ARG; before wsnark_init WSNARK_ERR_NOINIT.
 *                             Points, scalars and results stream through the staging ring in chunks of WSNARK_PWTAU_CHUNK points
 *                             (default 2^18, clamped to [64, 2^22]): device memory does not grow with n.  Each call takes a lane.
 *                             The kernel's chain: fixed signed 4-bit windows over a per-lane table of the point's multiples
 *                             1 .. 8, every lane adding at the same steps.
 *   tau32, alpha32, beta32    32 bytes plain little-endian each, reduced mod r; a secret that is 0 mod r is WSNARK_ERR_ARG.  NULL
 *                             draws the 32 bytes from the OS (getrandom): the production case.  The library never returns a secret
 *                             and wipes t, a, b and the table of t^(2^j) (volatile stores) before it returns; the device buffer
 *                             of the scalars c t^k is overwritten on its queue before the call returns, on every exit path; the
 *                             table of t^(2^j) and c also cross to the device in a kernel's argument block, which the runtime owns.
 *                             With three explicit secrets the call is deterministic.
 *   outputs                   out_tau_g1: 2n x 64 B, out_tau_g2: n x 128 B, out_alpha_tau_g1, out_beta_tau_g1: n x 64 B,
 *                             out_beta_g2_128.  An output may BE its input (in place); any other overlap is not allowed.
 *   errors                    what the loaders reject fails before anything is written, the report untouched: a NULL array, output
 *                             or report (WSNARK_ERR_ARG), domain not a power of two in [2, 2^24] (WSNARK_ERR_SIZE), an array shorter
 *                             than its domain implies (WSNARK_ERR_FORMAT); before wsnark_init WSNARK_ERR_NOINIT.
 *   a bad power is a RESULT   as in wsnark_pkey_setup: WSNARK_OK with ok = 0, per array points / infinity / bad / first_bad /
 *                             first_reason reduced on the device, independent of the chunking; a beta_g2 that fails the audit's
 *                             fixed-point tests is beta2_reason (then no array is looked at).  A power at infinity (x == 0) has no
 *                             place in a transcript: it is counted in infinity[] and makes ok = 0.  With ok = 0 the outputs are
 *                             unspecified.  relations_run and relations_bad stay 0.
 * wsnark_powers_check: the audit.  flags: WSNARK_PWCHECK_POINTS, WSNARK_PWCHECK_RELATIONS, 0 = both (as wsnark_pkey_check).
 *   points     every entry of the four arrays: coordinates < q, the curve equation; tau_g2 also the order-r subgroup test of the key
 *              audit (WSNARK_PK_OUTSIDE_SUBGROUP) -- the test wsnark_pkey_setup leaves out; beta_g2 the fixed-point tests; infinity
 *              counted as above.
 *   relations  rho_k as in the key audit (ChaCha20, key = seed32, counter = the global index k), T2 = tau_g2[1]:
 *     bit 0  tau_g1[0] and tau_g2[0] are the standard generators (byte compare)
 *     bit 1  e(sum_{k<2n-1} rho_k tau_g1[k+1], G2) = e(sum rho_k tau_g1[k], T2)
 *     bit 2  e(tau_g1[1], sum_{k<n-1} rho_k tau_g2[k]) = e(G1, sum rho_k tau_g2[k+1])
 *     bit 3  e(sum_{k<n-1} rho_k alpha_tau_g1[k+1], G2) = e(sum rho_k alpha_tau_g1[k], T2)      bit 4  the same for beta_tau_g1
 *     bit 5  e(beta_tau_g1[0], G2) = e(G1, beta_g2)
 *              Bits 1 and 2 together say that both arrays are the consecutive powers of ONE tau (bit 2's k = 0 term ties T2 to
 *              tau_g1[1]).  Each bit is two sums over the SAME rho against one array at offsets k and k + 1, by the ordinary MSMs chunk
 *              by chunk, and two host Miller loops.  A relation runs only if every point it involves passed the point tests (or they
 *              were not asked for); one that did not run leaves its relations_run bit clear, and then ok = 0.
 *              seed32 == NULL: 32 bytes from the OS.  As in the key audit the sums are sound with probability 1 - 2^-128 over a seed
 *              the transcript's author did NOT know; a fixed or published seed gives no soundness at all.
 *   The audit cannot tell WHO contributed, nor whether a transcript descends from an earlier one: that needs each contributor's proof
 *   of knowledge, which -- like a random beacon, .ptau readers and writers, file-to-file variants and more than one GPU -- is out of
 *   scope here.  Errors as for the contribution; flags with unknown bits: WSNARK_ERR_ARG.  Nothing else calls these functions and
 *   no other entry point changes. */
int wsnark_g1_mul_batch(const void* points, const void* scalars, uint64_t n, void* out_affine);
int wsnark_g2_mul_batch(const void* points, const void* scalars, uint64_t n, void* out_affine);
#define WSNARK_PWCHECK_POINTS    1u
#define WSNARK_PWCHECK_RELATIONS 2u      /* flags == 0 means both */
typedef struct {
    uint64_t points[4], infinity[4], bad[4];   /* WSNARK_PW_TAU_G1 .. WSNARK_PW_BETA_TAU_G1 */
    uint64_t first_bad[4];               /* UINT64_MAX if none */
    uint32_t first_reason[4];            /* WSNARK_PK_UNREDUCED / WSNARK_PK_OFF_CURVE / WSNARK_PK_OUTSIDE_SUBGROUP (tau_g2, the audit) */
    uint32_t beta2_reason;               /* 0 = good */
    uint32_t relations_run, relations_bad;   /* bits 0..5 as above; the contribution leaves both 0 */
    uint32_t ok;                         /* 1 iff nothing is bad or at infinity and every requested check was run */
    double   ms[4];                      /* contribution: device, host, 0, whole call; audit: points, relation sums, pairings, whole call */
} wsnark_powers_report_t;
int wsnark_powers_contribute(const wsnark_powers_t* in, const void* tau32, const void* alpha32, const void* beta32,
                             void* out_tau_g1, void* out_tau_g2, void* out_alpha_tau_g1, void* out_beta_tau_g1,
                             void* out_beta_g2_128, wsnark_powers_report_t* rep);
int wsnark_powers_check(const wsnark_powers_t* powers, uint32_t flags, const void* seed32, wsnark_powers_report_t* rep);
/* which share a handle holds: (0, 1, 0, nVars, domain, 0) for a whole key.  Any out pointer may be NULL. */
int wsnark_pkey_shard_info(const wsnark_pkey_t* handle, uint32_t* rank, uint32_t* world, uint64_t* first_signal,
                           uint64_t* n_signals, uint64_t* n_hexps, uint32_t* h_interleave_log);
/* sum_i h[i] * hExps_local[i] over the handle's resident hExps share (n must equal its n_hexps; d_h_slice: device, plain
 * form, in the share's layout) -- the H call of src/bn128.js:614 for one rank.  out96: Jacobian-Montgomery, normalised. */
int wsnark_pkey_h_msm_dev(wsnark_pkey_t* handle, const void* d_h_slice, uint64_t n, void* out96_host, void* stream);

/* Bn128.groth16GenProof (src/bn128.js:580-720).  witness: nVars x 32 B plain
 * (tools/buildwitness.js:36-41); witness_len < nVars * 32 is WSNARK_ERR_SIZE, a LONGER buffer is accepted and only its first
 * nVars signals are read -- exactly what the reference does with an over-long signals buffer (it walks nSignals records,
 * src/bn128.js:607-620).  r32 / s32: the two 32-byte blinding values the reference
 * draws from crypto.randomBytes (src/bn128.js:642-661); NULL => drawn from the OS CSPRNG.
 * out384 = pi_a (x, y, z) 96 B | pi_b (x.c0, x.c1, y.c0, y.c1, z.c0, z.c1) 192 B |
 * pi_c 96 B: affine, PLAIN (non-Montgomery) little-endian, i.e. exactly the integers
 * bin2g1/bin2g2 print (src/bn128.js:329-351, 706-718); infinity = (0, 1, 0). */
int wsnark_groth16_prove(wsnark_pkey_t* handle, const void* witness, size_t witness_len, const void* r32,
                         const void* s32, void* out384);
/* same, witness already on the device */
int wsnark_groth16_prove_dev(wsnark_pkey_t* handle, const void* d_witness, size_t witness_len, const void* r32,
                             const void* s32, void* out384_host, void* stream);

/* Host buffers the GPU can read in place (no counterpart in the reference, whose inputs live in the WASM heap).  A witness --
 * or the scalars / points of an MSM -- that is WRITTEN into such a buffer is DMA'd straight from it, chunk by chunk; any other
 * host pointer is first copied into the library's pinned staging ring by worker threads (about as fast as the link, but it
 * costs host cores and a second pass over the bytes).  The Node addon hands these out as external ArrayBuffers
 * (Bn128.allocInput).  Needs wsnark_init; free with wsnark_host_free (NULL is ignored). */
int wsnark_host_alloc(size_t bytes, void** out);
void wsnark_host_free(void* p);

/* Bn128.groth16Verify (src/bn128.js:722-791; pairing bn128_pairingEq4, src/bn128/build_bn128.js:265-1374): native host
 * arithmetic, no GPU and no wsnark_init needed.  Checks e(A,B) e(-IC(inputs),gamma2) e(-C,delta2) e(-alfa1,beta2) == 1.
 *   vk     : alfa1 (64 B) | beta2 (128 B) | gamma2 (128 B) | delta2 (128 B) | IC[0 .. n_inputs] (64 B each) -- the points
 *            of verification_key.json as affine PLAIN (non-Montgomery) little-endian integers, G2 as (x.c0, x.c1, y.c0, y.c1)
 *   inputs : n_inputs x 32 B plain little-endian public signals; one >= r gives *valid = 0 like the reference (:772)
 *   proof384: what wsnark_groth16_prove writes (pi_a | pi_b | pi_c with their z coordinates).  The z coordinates are IGNORED,
 *            as the reference's setG1Affine / setG2Affine do (src/bn128.js:741-760): (x, y) is the point.  Consequence: a proof
 *            with a component at infinity -- printed (0, 1, 0); reachable only with r = s = 0 on degenerate witnesses -- is read
 *            as the point (0, 1), which is not on the curve, and is therefore always INVALID here
 * Returns WSNARK_OK with *valid = 1 / 0; WSNARK_ERR_FORMAT if a coordinate is not a reduced field element,
 * WSNARK_ERR_SIZE if vk holds fewer than n_inputs + 1 IC points.  Unlike the reference, which makes no such test (its
 * verdict on malformed points is an accident of its Miller loop), a point that is not on its curve, or a G2 point outside
 * the order-r subgroup, makes the proof invalid (*valid = 0).  Like the reference (src/bn128.js:741-760 force z = 1) the z
 * coordinates of the proof are ignored: (x, y) is the point. */
int wsnark_groth16_verify(const void* vk, size_t vk_len, const void* inputs, uint64_t n_inputs, const void* proof384, int* valid);

/* MANY proofs against ONE key, on the device (csrc/pairing.hip): status[i] is what wsnark_groth16_verify(vk, vk_len, inputs_i,
 * n_inputs, proof_i, &v) says about proof i -- 1 = valid, 0 = invalid, 2 = malformed (a coordinate of proof i, its z
 * coordinates included, is not a reduced field element: the case in which the single call returns WSNARK_ERR_FORMAT).  Every rule
 * of the single call holds per proof (z ignored; an input >= r is invalid, not an error; an off-curve point or a G2 point outside
 * the order-r subgroup is invalid before anything is paired).
 * vk: the single call's layout, in HOST memory in both variants.  inputs: count x n_inputs x 32 bytes (proof i's public signals
 * one after the other), proofs384: count x 384 bytes, each record as wsnark_groth16_prove writes it; host memory (staged through
 * the upload ring) or, for _dev, device memory read on `stream` (NULL = the lane's queue).  status: count bytes, host memory.
 * What the key alone decides is decided once per call, on the host: an unreduced key coordinate is WSNARK_ERR_FORMAT for the call,
 * fewer IC points than n_inputs + 1 WSNARK_ERR_SIZE (nothing is written); a key point that fails its curve / subgroup test makes
 * every status 0 (2 for a malformed proof).  count == 0 is WSNARK_OK and touches nothing; count > 2^24 is WSNARK_ERR_SIZE.
 * Unlike the single call these need wsnark_init (WSNARK_ERR_NOINIT otherwise); callable from any thread, each call takes a lane of
 * the context like an MSM does.  Both return when status has been written. */
int wsnark_groth16_verify_batch(const void* vk, size_t vk_len, const void* inputs, uint64_t n_inputs, const void* proofs384, uint64_t count,
                                uint8_t* status);
int wsnark_groth16_verify_batch_dev(const void* vk, size_t vk_len, const void* d_inputs, uint64_t n_inputs, const void* d_proofs384,
                                    uint64_t count, uint8_t* status_host, void* stream);

/* ---- compressed points and 128-byte proofs (csrc/pointcodec.hip): NO reference counterpart ----
 * The reference speaks proofs only as 384-byte records; every other Groth16 stack on this curve hands points around compressed: x and
 * one bit that names the root y of y^2 = x^3 + b (b = 3 on G1, 3 / (9 + u) on the twist).  32 bytes per G1 point, 64 per G2 point,
 * 128 per proof.  q < 2^254, so the top two bits of x are free for flags.  "Larger" root: the one whose PLAIN value is > (q - 1) / 2; on
 * G2 decided on y.c1 if that is not zero, else on y.c0 (the same as y > -y with c1 compared before c0).
 *   WSNARK_ENC_LE  x little-endian; G2 is x.c0 | x.c1; flags in the top two bits of the LAST byte: 0x80 = y is the larger root,
 *                  0x40 = infinity (every other bit zero); both set is malformed.           (ark-serialize's compressed mode, BN254)
 *   WSNARK_ENC_BE  x big-endian; G2 is x.c1 | x.c0; flags in the top two bits of the FIRST byte: 0b10 = smaller root, 0b11 = larger
 *                  root, 0b01 = infinity (every other bit zero); 0b00 ("uncompressed") is malformed here.  (gnark-crypto's bn254 marshal)
 *   G1 = (1, 2):  01 00 .. 00 (LE),  80 00 .. 00 01 (BE);   -G1:  01 00 .. 00 80 (LE),  C0 00 .. 00 01 (BE);   infinity:  00 .. 00 40 (LE),
 *   40 00 .. 00 (BE).
 * NOT VERIFIED against either library: both layouts were written from knowledge of them; no file written by arkworks or gnark was
 * available.  The statement above is the contract, and the tests pin it.
 *
 * Points (host memory both ways; streamed through the staging ring in chunks, so device memory does not grow with n):
 *   compress    points: n affine points in key format (Montgomery words, 64 / 128 bytes, every word of x zero = infinity, the loaders'
 *               rule) -> out: n x 32 / 64 bytes; status[i]: 0 = ok, 1 = a coordinate >= q, and that record is all zero.  The curve
 *               equation is NOT tested (that is wsnark_pkey_check's job): any reduced (x, y) is compressed.
 *   decompress  in: n x 32 / 64 bytes -> out_points: n affine points in key format (infinity: all zero); status[i] one of WSNARK_DEC_*;
 *               the smallest number wins when several reasons apply; a point whose status is not 0 is written as all zero bytes.
 *               flags: 0, or WSNARK_DEC_SUBGROUP (G2 only: the audit's [r] Q == O chain; ignored on G1, whose curve has prime order).
 *   *n_bad: how many statuses are not 0, counted on the device.
 * Proofs: a compressed proof is A | B | C at 32 + 64 + 32 bytes, the order in which both libraries write one; the 384-byte record is
 * wsnark_groth16_prove's (plain little-endian integers).  status[i] has wsnark_groth16_verify_batch's meaning:
 *   proof_compress     1 = written; 2 = one of the twelve words (z included) is not a reduced field element: a zero record.  The z
 *                      words are otherwise ignored, as the verifiers ignore them; a component with x = 0 is written as infinity.
 *   proof_decompress   1 = written, with z = 1 (z.c0 = 1, z.c1 = 0 for B); 2 = a malformed point; 0 = a point without a y, or one
 *                      encoded as infinity (no verifier accepts a proof with a component at infinity).  0 and 2: a zero record.
 *                      B's subgroup membership is not tested here: the verifiers test it.
 *   verify_batch_compressed[_dev]   status[i] is exactly what wsnark_groth16_verify_batch says about the decompressed proof i: a proof
 *                      with a malformed point is 2, one with a point without a y or at infinity is 0.  The proofs are decompressed on
 *                      the device into the records the batch verifier's first kernel reads; nothing returns to the host in between.
 *                      vk, inputs, count == 0, count > 2^24, the key-level outcomes, lanes and threads: as wsnark_groth16_verify_batch.
 *                      _dev: d_inputs and d_proofs128 (16-byte aligned) in device memory, read on `stream` (NULL: the lane's queue).
 * Every call here needs wsnark_init (WSNARK_ERR_NOINIT), returns WSNARK_ERR_ARG for an encoding that is not WSNARK_ENC_*, for an
 * undefined flag and for a NULL pointer, WSNARK_OK without touching anything for n == 0 / count == 0, and leaves its outputs untouched
 * on any error.
 * Out of scope: readers of arkworks or gnark KEY files; a compressed key container; square roots in Fr; a host-only path without
 * wsnark_init; group (multi-GPU) handles; provers that emit compressed proofs directly (wsnark_proof_compress on their output is the
 * path). */
enum { WSNARK_ENC_LE = 1, WSNARK_ENC_BE = 2 };
enum { WSNARK_DEC_OK = 0, WSNARK_DEC_MALFORMED = 1, WSNARK_DEC_NO_POINT = 2, WSNARK_DEC_OUTSIDE_SUBGROUP = 3 };
enum { WSNARK_DEC_SUBGROUP = 1 };      /* flags of the decompress calls */
int wsnark_g1_compress(const void* points, uint64_t n, int encoding, void* out, uint8_t* status, uint64_t* n_bad);
int wsnark_g2_compress(const void* points, uint64_t n, int encoding, void* out, uint8_t* status, uint64_t* n_bad);
int wsnark_g1_decompress(const void* in, uint64_t n, int encoding, uint32_t flags, void* out_points, uint8_t* status, uint64_t* n_bad);
int wsnark_g2_decompress(const void* in, uint64_t n, int encoding, uint32_t flags, void* out_points, uint8_t* status, uint64_t* n_bad);
int wsnark_proof_compress(const void* proofs384, uint64_t count, int encoding, void* out128, uint8_t* status);
int wsnark_proof_decompress(const void* proofs128, uint64_t count, int encoding, void* out384, uint8_t* status);
int wsnark_groth16_verify_batch_compressed(const void* vk, size_t vk_len, const void* inputs, uint64_t n_inputs, const void* proofs128,
                                           uint64_t count, int encoding, uint8_t* status);
int wsnark_groth16_verify_batch_compressed_dev(const void* vk, size_t vk_len, const void* d_inputs, uint64_t n_inputs, const void* d_proofs128,
                                               uint64_t count, int encoding, uint8_t* status_host, void* stream);

/* ---- many witnesses of ONE key in one call (csrc/provebatch.hip): NO reference counterpart ----
 * The reference's groth16GenProof takes one witness (src/bn128.js:580-720); a proving service holds one small circuit (2^10 .. 2^16
 * constraints) and many witnesses, and a single proof of that size leaves most of the device idle.
 * THE CONTRACT: out384s[i] (count x 384 bytes) is byte for byte what wsnark_groth16_prove(handle, witness_i, nVars*32, r_i, s_i, out)
 * writes.  Every rule of the single call holds per proof: witness values are raw 256-bit and may be >= r; the key's points at
 * infinity (x == 0) are honoured; infinity prints as (0, 1, 0).
 *   witnesses      witness i starts at witnesses + i * witness_stride; only its first nVars signals are read.  witness_stride <
 *                  nVars*32 is WSNARK_ERR_SIZE.  _dev: memory of the handle's device, pointer and stride multiples of 16, ready on
 *                  `stream` (NULL: the lane's own queue)
 *   r32s, s32s     count x 32 bytes each, HOST memory in both variants; either may be NULL: its values are then drawn from the OS
 *                  CSPRNG, one independent draw per proof
 *   out_rs64s      (may be NULL) count x 64 bytes, host: r_i | s_i as used -- the batch's counterpart of wsnark_last_blinding
 *   rep            (may be NULL) see below
 * count == 0 is WSNARK_OK and touches nothing; count > 2^16 is WSNARK_ERR_SIZE; a NULL handle, witnesses or out is
 * WSNARK_ERR_ARG, as is a handle that holds a points shard or an interleaved hExps slice (whole keys only, no group handles);
 * WSNARK_ERR_NOINIT before wsnark_init.  On every error the outputs and the report are left untouched.
 * The batch path: per pass of `chunk` proofs (as many as keep the pass's scratch under a fixed budget; switch BATCH_CHUNK) one
 * upload, a = A.w and b = B.w of all proofs in one launch, CALC_H over the stack of proofs, the five sums of every proof against
 * row 0 of the key's resident sections (one workgroup per (proof, sum, window), windows of BATCH_WINDOW bits in [4, 8], default 8),
 * the proof assembly on the device, one download of chunk x 384 bytes.  r, s and rs cross to the device in a buffer that is
 * overwritten on the call's queue before the call returns, on every exit path.  It does not wait for the key's table build.
 * Routing: a key whose domain is above BATCH_MAX_DOMAIN (at most 2^16), or a call with fewer than BATCH_MIN proofs, loops the single
 * prover instead -- same contract, same outputs, report.batched = 0.  The switches are read per call (wsnark_tuning_set /
 * WSNARK_<name>), so one process can run both paths.
 * wsnark_last_blinding: the batch kernels leave the calling thread's record alone; the loop over the single prover overwrites it with
 * the last proof's r | s, as that prover always does.  Callers of this entry point read out_rs64s, which is the same on both routes.
 * _dev and the stride: every witness is read as 16-byte aligned field elements (the single prover's contract for a device witness,
 * which the loop route hands witness i to as it is), hence pointer AND stride are multiples of 16.
 * Memory: a pass's scratch (at most 2 GiB) belongs to the lane the call held and is kept, grow-only, until the context goes.
 * Each call takes one lane of the key's context; two threads may run batches on one handle at once. */
typedef struct {
    uint64_t count;        /* proofs asked for */
    uint64_t batched;      /* proofs that went through the batch kernels (0: the call looped the single prover) */
    uint32_t chunk;        /* proofs per pass over the kernels */
    uint32_t window_bits;  /* of the batch sums */
    double   ms[5];        /* upload, CALC_H, the five sums, assembly (device time, summed over the passes); whole call (host clock) */
} wsnark_prove_batch_report_t;
int wsnark_groth16_prove_batch(wsnark_pkey_t* handle, const void* witnesses, size_t witness_stride, uint64_t count,
                               const void* r32s, const void* s32s, void* out384s, void* out_rs64s,
                               wsnark_prove_batch_report_t* rep);
int wsnark_groth16_prove_batch_dev(wsnark_pkey_t* handle, const void* d_witnesses, size_t witness_stride, uint64_t count,
                                   const void* r32s, const void* s32s, void* out384s_host, void* out_rs64s_host,
                                   wsnark_prove_batch_report_t* rep, void* stream);

/* The two 32-byte blinding values of the last proof assembled by the CALLING THREAD (wsnark_groth16_prove[_dev] or
 * _prove_finish), whether injected or drawn from the OS CSPRNG: the reference keeps them the same way, "for tests",
 * as this._pr / this._ps (src/bn128.js:662-664).  WSNARK_ERR_ARG if this thread has not proved yet. */
int wsnark_last_blinding(void* r32_out, void* s32_out);

/* Multi-GPU proving (one process per GPU; windows sharded as in wsnark_g1_msm_windows, rank / world per call).
 * prove_partial runs CALC_H and the five MSMs on this rank's windows and writes ONE 576-byte record:
 * A | B1 | C | H (4 x 96 B G1) | B2 (192 B G2), Jacobian-Montgomery -- the reference's per-worker
 * partial results (src/bn128.js:374-382, 406-414) for all five sums at once.  After a single
 * all_gather of these records, prove_finish (host arithmetic only) sums them and assembles the proof
 * exactly as wsnark_groth16_prove does (src/bn128.js:671-718).
 * flags: WSNARK_PARTIAL_SKIP_H leaves CALC_H and the H sum to the caller (the record's H slot is infinity): the ranks then
 * compute h with the distributed four-step transform and each sums its own slice of h against its slice of the H points
 * (wasmsnark_amd/dist.py: DistProver) instead of every rank repeating the whole CALC_H. */
#define WSNARK_PARTIAL_SKIP_H 1u
int wsnark_groth16_prove_partial(wsnark_pkey_t* handle, const void* witness, size_t witness_len, uint32_t rank,
                                 uint32_t world, uint32_t flags, void* out576);
int wsnark_groth16_prove_partial_dev(wsnark_pkey_t* handle, const void* d_witness, size_t witness_len, uint32_t rank,
                                     uint32_t world, uint32_t flags, void* out576_host, void* stream);
int wsnark_groth16_prove_finish(wsnark_pkey_t* handle, const void* partials, uint64_t n_ranks, const void* r32,
                                const void* s32, void* out384);

/* ONE CALL per proof and rank for the whole multi-GPU prover (csrc/dist.hip): the rank's partial sums over its points shard,
 * CALC_H on the distributed four-step transform (three all-to-alls per proof), the H sum over the rank's hExps share, one
 * all-gather of the 576-byte records and the host-side assembly -- no host language between the kernels.  The library links
 * no collectives library: the host passes its transport as two callbacks (torch.distributed on RCCL in
 * wasmsnark_amd/dist.py; MPI, a thread pool, ... elsewhere):
 *   d_send / d_recv  two device buffers of buf_bytes >= 3 * 32 * domain / world each, owned by the host side
 *   all_to_all(user, bytes_per_rank, stream)   block q (bytes_per_rank bytes) of d_send goes to rank q, block q of d_recv comes
 *                    from rank q; must be ORDERED ON `stream` (the library's kernels that fill d_send were enqueued on it and
 *                    the ones that read d_recv follow on it) -- enqueue it there, or synchronise it; return 0 on success
 *   all_gather(user, send, recv, bytes)        host memory: recv = the `bytes`-byte records of all ranks in rank order
 * handle: the rank's points shard with h_interleave_log = floor(log2(domain) / 2) (wsnark_pkey_load_shard); world must be a
 * power of two <= 2^floor(log2(domain) / 2).  world == 1: callbacks may be NULL (the exchange is the identity).
 * Collectives per proof, posted by EVERY rank in the same order whatever happens on it: all_gather (80-byte records: the
 * rank's preflight status, which of r / s it was given, the blinding bytes -- rank 0's draw when r32 / s32 are NULL -- before
 * the GPU work, so that the host's key-only scalar multiplications run under it), three all_to_all, all_gather (592-byte
 * records: the 576 bytes of partial sums + the rank's status).  EVERY RANK MUST PASS THE SAME r32 / s32 (all NULL, or the
 * same bytes): ranks that disagree all return WSNARK_ERR_ARG.  A rank that fails locally still posts the exchanges its peers
 * are waiting in and reports through the last gather: every rank then returns an error, nobody is left in a collective
 * (what remains the transport's job: a callback that itself fails or hangs on one rank).
 * stream: the queue d_witness is ready on (NULL: the library's own). */
typedef struct {
    uint32_t rank, world;
    void* d_send;
    void* d_recv;
    uint64_t buf_bytes;
    int (*all_to_all)(void* user, uint64_t bytes_per_rank, void* stream);
    int (*all_gather)(void* user, const void* send, void* recv, uint64_t bytes);
    void* user;
} wsnark_comm_t;
int wsnark_groth16_prove_dist(wsnark_pkey_t* handle, const void* d_witness, size_t witness_len, const wsnark_comm_t* comm,
                              const void* r32, const void* s32, void* out384_host, void* stream);

/* ---- resident bases (round 5; csrc/fixedbase.hip): NO reference counterpart ----
 * The reference's g1_multiexp / g2_multiexp (src/bn128.js:353-415) take the points with every call.  A caller that sums over the
 * SAME bases repeatedly can make them resident once -- as fixed-base window tables, the layout a resident proving key's sections
 * have: rows x n points, row w = 2^(c w) * P, c = log2 n (13 rows and 13 x the bytes at 2^20) -- and then pays neither the points'
 * H2D copy nor the per-window plans and the host's doubling chain: every sum is one bucket set and one reduction tail.
 *   group: 1 = G1 (64-byte affine Montgomery points), 2 = G2 (128-byte); x == 0 is infinity, as everywhere.
 *   wsnark_points_msm[_dev]: n must be the set's size (one raw 256-bit scalar per point); out = the Jacobian-Montgomery triple
 *   (96 / 192 bytes, affine-normalised) that wsnark_g{1,2}_msm returns for the same pairs. */
typedef struct wsnark_points wsnark_points_t;
int wsnark_points_load(int group, const void* points, uint64_t n, wsnark_points_t** out_handle);
void wsnark_points_free(wsnark_points_t* handle);
int wsnark_points_info(const wsnark_points_t* handle, int* group, uint64_t* n, uint32_t* window_bits, uint32_t* rows, uint64_t* table_bytes);
int wsnark_points_msm(wsnark_points_t* handle, const void* scalars, uint64_t n, void* out);
int wsnark_points_msm_dev(wsnark_points_t* handle, const void* d_scalars, uint64_t n, void* out_host, void* stream);

/* ---- KZG commitments on a powers-of-tau transcript: commit, open, verify (csrc/kzg.hip): NO reference counterpart ----
 * The tau_g1 array of a transcript (wsnark_powers_t) is also the structured reference string of the KZG scheme that snarkjs' PLONK and
 * FFLONK, gnark's PLONK and halo2-KZG use on this curve: C = sum_k f[k] tau^k G commits to f, pi = commit((f - f(z)) / (X - z)) opens
 * it at z, and two pairings check the opening.  The sums are the resident-bases sums above, the transform is wsnark_fr_ntt's; the
 * division by (X - z) and the fold of several polynomials under a challenge are kernels of their own (DESIGN.md "KZG").
 *   Scalars -- coefficients, z, gamma, y -- are 32-byte plain little-endian integers; inputs may be any 256-bit value and are taken
 *   mod r, outputs are canonical.  A polynomial is len coefficients, lowest degree first; count polynomials are stored back to back.
 *   G1 points are 64-byte affine Montgomery points, x == 0 is infinity; a result at infinity is 64 zero bytes and every other result
 *   is affine and canonical: results compare byte for byte.
 *   wsnark_kzg_srs_load: tau_g1[k] = tau^k g1, k < n, n in [1, 2^24], on the host; they become resident as wsnark_points_load makes
 *     them (window tables where they fit).  Every power gets the audit's two cheap tests: a coordinate >= q, a point off the curve
 *     or one at infinity is WSNARK_ERR_FORMAT, and wsnark_last_error names the first index.  tau_g1[0] is the commitment generator
 *     and need not be the standard one.  Whether the points ARE the powers of one tau is wsnark_powers_check's question, not this
 *     call's.  The handle is read-only after the load: any number of threads may commit and open on it at once.
 *   wsnark_fr_poly_eval: out_y[i] = f_i(z).  wsnark_fr_poly_divide: out_q = (f - f(z)) / (X - z), len - 1 coefficients (none for
 *     len == 1), out_y32 = f(z); _dev: d_poly and d_q resident and NOT overlapping, the value still goes to the host.  len in
 *     [1, 2^24]; z = 0 and z >= r are ordinary inputs.
 *   wsnark_kzg_commit: out[i] = sum_k f_i[k] tau_g1[k], len <= n.  form 0: coefficients.  form 1: len evaluations on the size-len
 *     domain of wsnark_fr_ntt (len a power of two): the call runs the inverse transform first.  For len < n the sum runs over the
 *     first len points or, padded with zeros, over the whole table, whichever was measured faster (KZG_PAD_PCT); same bytes.
 *   wsnark_kzg_open: out_y[i] = f_i(z) for every polynomial, and ONE proof pi = commit(q), q the quotient of F = sum_i gamma^i f_i
 *     at z.  count == 1 ignores gamma, which may then be NULL.  gamma is the caller's Fiat-Shamir challenge.
 *   wsnark_kzg_verify: with C = sum gamma^i C_i and y = sum gamma^i y_i it checks e(C - y g1 + z pi, g2) == e(pi, tau g2) on the
 *     host (the curve and pairing of wsnark_groth16_verify); it needs no wsnark_init.  g2_tau_g2_256 = g2 | tau g2, 128 bytes each.
 *     An unreduced coordinate is WSNARK_ERR_FORMAT; an off-curve point, a G2 point outside the subgroup, g1, g2 or tau g2 at infinity
 *     give *valid = 0; pi or a C_i at infinity is legal (a constant polynomial's proof is infinity).
 *   Errors: NULL pointers or a NULL handle WSNARK_ERR_ARG; len == 0, len > n, len > 2^24, count > 65535, count x len > 2^28, a len that is no
 *     power of two with form 1: WSNARK_ERR_SIZE; count == 0: WSNARK_OK and nothing is touched; every call but wsnark_kzg_verify
 *     before wsnark_init: WSNARK_ERR_NOINIT.  On every error the outputs are left untouched.  Each call takes a lane.
 *   Out of scope: G2 commitments; openings of one polynomial at several points; a batch verifier with a single verdict; Fiat-Shamir
 *     transcripts; readers of .ptau, halo2 or gnark SRS files; group (multi-GPU) and sharded handles. */
typedef struct wsnark_kzg_srs wsnark_kzg_srs_t;
int wsnark_kzg_srs_load(const void* tau_g1, uint64_t n, wsnark_kzg_srs_t** out_handle);
void wsnark_kzg_srs_free(wsnark_kzg_srs_t* handle);      /* NULL ignored */
int wsnark_kzg_srs_info(const wsnark_kzg_srs_t* handle, uint64_t* n, uint64_t* table_bytes);
int wsnark_fr_poly_eval(const void* polys, uint64_t len, uint64_t count, const void* z32, void* out_y);
int wsnark_fr_poly_divide(const void* poly, uint64_t len, const void* z32, void* out_q, void* out_y32);
int wsnark_fr_poly_divide_dev(const void* d_poly, uint64_t len, const void* z32, void* d_q, void* out_y32_host, void* stream);
int wsnark_kzg_commit(wsnark_kzg_srs_t* handle, const void* polys, uint64_t len, uint64_t count, int form, void* out_commitments);
int wsnark_kzg_commit_dev(wsnark_kzg_srs_t* handle, const void* d_polys, uint64_t len, uint64_t count, int form, void* out_commitments_host,
                          void* stream);
int wsnark_kzg_open(wsnark_kzg_srs_t* handle, const void* polys, uint64_t len, uint64_t count, const void* z32, const void* gamma32,
                    void* out_y, void* out_proof64);
int wsnark_kzg_open_dev(wsnark_kzg_srs_t* handle, const void* d_polys, uint64_t len, uint64_t count, const void* z32, const void* gamma32,
                        void* out_y_host, void* out_proof64_host, void* stream);
int wsnark_kzg_verify(const void* g1_64, const void* g2_tau_g2_256, const void* commitments, uint64_t count, const void* z32,
                      const void* gamma32, const void* ys, const void* proof64, int* valid);

/* ---- several GPUs in ONE process (csrc/group.hip; round 5) ----
 * The reference's host is one process that starts W workers (src/bn128.js:173-265, `build()`), cuts every multi-exponentiation
 * into W contiguous ranges of the pairs, posts one to each worker and adds the partial results (:353-415), and runs the five
 * sums of a proof that way (:607-622).  A group is that arrangement with GPUs as the workers, for hosts that are ONE process
 * (the Node.js drop-in): one context and one host thread per device, the transport between the devices inside the library
 * (device-to-device copies ordered by events for the distributed CALC_H's three exchanges; the 576-byte records gathered in
 * host memory).  Hosts that run one process per GPU keep using wsnark_groth16_prove_dist with their own transport.
 *   wsnark_group_create      devices[n]: HIP device ordinals (the same ordinal may appear more than once: two contexts on one
 *                            GPU -- how the path is tested on a single-GPU box).  Independent of wsnark_init.
 *   wsnark_group_pkey_load*  one POINTS SHARD of the key per device (wsnark_pkey_load_shard: pairs [g floor(n/N), ...), all
 *                            fixed-base table rows of that range, 1 / N of the key's memory each; the two matrices complete)
 *   wsnark_group_prove       = wsnark_groth16_prove over the group: same inputs, same 384 bytes.  CALC_H runs on the
 *                            distributed four-step transform when N is a power of two <= 2^floor(log2(domain) / 2)
 *                            (wsnark_group_pkey_info reports which), otherwise complete on every device.
 *   wsnark_group_g{1,2}_msm  = wsnark_g{1,2}_msm with the reference's split of the pairs over the devices
 * Calls on one group are serialised (one collective at a time); different groups are independent.
 * OWNERSHIP: a group owns its keys.  wsnark_group_free waits for the group's call in flight, then frees the group AND every key
 * handle still loaded on it: those handles are invalid afterwards and must not be passed to wsnark_group_pkey_free (the Python and
 * Node hosts forget them when the group dies).  The caller must not free a group while another thread may still START a call on
 * it (the Node addon counts its queued jobs and defers the free to the last one). */
typedef struct wsnark_group wsnark_group_t;
typedef struct wsnark_group_pkey wsnark_group_pkey_t;
int wsnark_group_create(const int* devices, uint32_t n, wsnark_group_t** out_group);
void wsnark_group_free(wsnark_group_t* group);
uint32_t wsnark_group_size(const wsnark_group_t* group);
int wsnark_group_pkey_load(wsnark_group_t* group, const void* pkey, size_t len, wsnark_group_pkey_t** out_handle);
int wsnark_group_pkey_load_sections(wsnark_group_t* group, const wsnark_key_sections_t* ks, wsnark_group_pkey_t** out_handle);
/* the same from a key file (wsnark_pkey_load_file): ONE read-only mapping, every member reads its own shard's pages */
int wsnark_group_pkey_load_file(wsnark_group_t* group, const char* path, wsnark_group_pkey_t** out_handle);
void wsnark_group_pkey_free(wsnark_group_pkey_t* handle);
int wsnark_group_pkey_info(const wsnark_group_pkey_t* handle, uint32_t* n_vars, uint32_t* n_public, uint32_t* domain, uint32_t* world,
                           int* distributed_calc_h);
int wsnark_group_pkey_wait_tables(wsnark_group_pkey_t* handle);
int wsnark_group_prove(wsnark_group_pkey_t* handle, const void* witness, size_t witness_len, const void* r32, const void* s32,
                       void* out384);
int wsnark_group_last_blinding(wsnark_group_t* group, void* r32, void* s32);     /* = wsnark_last_blinding for the group's last proof */
int wsnark_group_g1_msm(wsnark_group_t* group, const void* scalars, const void* points, uint64_t n, void* out96);
int wsnark_group_g2_msm(wsnark_group_t* group, const void* scalars, const void* points, uint64_t n, void* out192);

/* ---- synthetic-input helpers: NO reference counterpart ----
 * out[i] = scalars[i] * base (affine Montgomery in and out; infinity written as all-zero bytes).
 * The reference ships no proving key (its test/data/proving_key.bin is absent), so benches and
 * tests build valid synthetic keys from known toxic waste with these (wasmsnark_amd/synth.py). */
int wsnark_g1_mul_base_batch(const void* base64, const void* scalars, uint64_t n, void* out_affine);
int wsnark_g2_mul_base_batch(const void* base128, const void* scalars, uint64_t n, void* out_affine);

/* A whole synthetic circuit + trusted setup from KNOWN toxic waste, on the host (csrc/synth.hip): the multiplication-chain
 * R1CS SURVEY.md section 8d C4 specifies (style 0 = 1-3 non-zeros per COLUMN of A and B, every variable present; style 1 =
 * 1-2 terms per ROW, ~40 % of the variables absent from A resp. B; style 2 = bit decompositions: groups of 14 free bits with their
 * booleanity rows b (b - 1) = 0, a recomposition row and a product row -- 87.5 % of the witness is 0 / 1), its witness, its polsA / polsB record streams
 * (tools/buildpkey.js:79-89), the discrete logarithm of every key point (feed them to wsnark_g{1,2}_mul_base_batch) and
 * the discrete logarithms of the proof for given r, s -- the closed form the full-size parity tests compare against.
 * key_scalars group 1: alfa1, beta1, delta1, A[nVars], B1[nVars], C[nVars-nPublic-1], hExps[domain], IC[nPublic+1];
 * group 2: beta2, delta2, gamma2, B2[nVars]; 32-byte plain little-endian each.  expected: a | b | c, 32 B plain each. */
typedef struct wsnark_synth wsnark_synth_t;
typedef struct {
    uint32_t n_vars, n_public, domain;
    uint64_t nnz_a, nnz_b, absent_a, absent_b;   /* non-zeros; variables that never occur in A resp. B */
    uint64_t pols_a_len, pols_b_len;             /* bytes of the record streams */
    uint64_t n_g1_scalars, n_g2_scalars;
} wsnark_synth_info_t;
int wsnark_synth_new(uint32_t log_domain, uint32_t n_public, uint64_t circuit_seed, uint64_t setup_seed, int style,
                     wsnark_synth_t** out);
void wsnark_synth_free(wsnark_synth_t* h);
int wsnark_synth_info(const wsnark_synth_t* h, wsnark_synth_info_t* out);
int wsnark_synth_witness(const wsnark_synth_t* h, void* out_plain);
int wsnark_synth_pols(const wsnark_synth_t* h, int which, void* out, uint64_t cap);
int wsnark_synth_key_scalars(const wsnark_synth_t* h, int group, void* out);
int wsnark_synth_expected(const wsnark_synth_t* h, const void* r32, const void* s32, void* out96);

/* ---- device self-test hooks (tests/test_gpu_primitives.py): NO reference counterpart ----
 * The reference tests its field and group primitives directly (test/f1.js:296-400, test/bn128.js:84-185); here they
 * are __device__ code reached only through whole kernels, so these two entry points run ONE LANE PER VECTOR through
 * the device arithmetic itself.  Inputs and outputs are in the reference's formats; the conversion to the kernels'
 * internal representation and back is part of what is tested.
 *   which: 0 = Fq, 1 = Fr (32-byte elements), 2 = Fq2 (64-byte)
 *   impl : 0 = radix-2^29 lazy field (MSM / NTT kernels), 1 = saturated 4 x 64 field on the device (light kernels),
 *          2 = the host field (what proof assembly uses; runs on the CPU)
 *   op   : WSNARK_ST_* below; out is n x 32 (64 for Fq2) bytes. */
enum {
    WSNARK_ST_MUL = 0, WSNARK_ST_SQR = 1, WSNARK_ST_ADD = 2, WSNARK_ST_SUB = 3, WSNARK_ST_NEG = 4,
    WSNARK_ST_TOMONT = 5, WSNARK_ST_FROMMONT = 6,
    WSNARK_ST_SUB_WEAK = 7,      /* (a - b) through the uncorrected difference feeding a product     */
    WSNARK_ST_ADD_LAZY_MUL = 8,  /* (a + b) * b with the carry-free sum as a direct product operand  */
    WSNARK_ST_NEG_WEAK_MUL = 9,  /* (-a) * b through the 2p - a form                                 */
    WSNARK_ST_MUL2ADD = 10,      /* a*a + b*b with one Montgomery reduction                          */
    WSNARK_ST_MULSUB2 = 11,      /* (a - b)*a - b*a: fused, first operand an uncorrected difference   */
    WSNARK_ST_EQ = 12,           /* out = 1 if a == b else 0 (zero test of the strict difference)    */
    WSNARK_ST_EQ_WEAK = 13,      /* the same through the uncorrected difference                      */
    WSNARK_ST_INVERSE = 14,      /* 1/a (a != 0): impl 2 = the host's inversion (proof assembly), impl 0 / 1 (Fq, Fr) = the DEVICE's Fermat
                                    inversion a^(p-2) on that field -- what the table build's normalisation runs (msm_table_norm_kernel) */
    WSNARK_ST_SQR_WEAK = 15,     /* (a - b)^2 with the uncorrected difference as the operand of the squaring        */
    WSNARK_ST_MUL_WEAK_A = 16,   /* (a - b) * b with the uncorrected difference as the FIRST operand of the product */
    WSNARK_ST_MULSUB2_WEAK_B = 17, /* a*(a - b) - b*a: fused, second operand an uncorrected difference              */
    /* square roots (the reference's f1m_sqrt / f1m_isSquare, src/build_f1m.js:809-897): `which` 0 (Fq: a^((q+1)/4), q = 3 mod 4) and
       2 (Fq2: the complex method, two exponentiations and no inversion); b is ignored.  `which` 1 (Fr) is WSNARK_ERR_ARG: Tonelli-Shanks
       over a field of 2-adicity 28 has no user here.  impl 0 = the device's radix-2^29 field, 2 = the host's. */
    WSNARK_ST_SQRT = 18,         /* Fq: the root whose PLAIN value is even, as the reference picks it (build_f1m.js:871-875); Fq2: the
                                    not-larger root (WSNARK_ENC_* below: "larger").  A non-square: every output byte 0xFF.  sqrt(0) = 0 */
    WSNARK_ST_IS_SQUARE = 19     /* out = 1 if a is a square (0 is one), else 0                                          */
};
int wsnark_selftest_field(int which, int impl, int op, const void* a, const void* b, void* out, uint64_t n);
/*   g: 1 or 2; impl: 0 = radix-2^29 curve of the accumulation kernels, 1 = saturated-field curve on the device,
 *   2 = host curve, 3 = (G1 only) the radix-2^29 variant of the reduction-tail kernels (inlined products), 4 = (G2 only) the
 *   reduction-tail variant with the quadratic extension's two components on two adjacent lanes (two lanes per vector).
 *   p, q: n Jacobian-Montgomery points (96 / 192 B, any z; z == 0 = infinity); out: n affine-normalised
 *   Jacobian-Montgomery points ((x, y, 1) or (0, 1, 0)) like every group element this ABI returns.
 *   op: 0 = p + q (full addition), 1 = 2p, 2 = -p, 3 = p (normalisation only), 4 = p + q as a MIXED addition
 *   (q must be affine: z == 1, or infinity), 5 = p - q as a mixed addition with the negate flag,
 *   6 = p + q + q and 7 = p + q - q as two mixed additions of the ACCUMULATION LOOP's lazy form (x kept "wide" between
 *   them, field29.h) followed by its narrowing, 8 = timesScalar (src/build_timesscalar.js:20-80): q's bytes are NOT a point
 *   but a little-endian scalar in bytes [0, 64) and its length -- 32 or 64 -- in byte 64 (impl 0-3),
 *   10 and 11 (9 is not an operation) = the reduction tail's straight-path addition (curve.h / curve_pair.h: add_fast), which refuses
 *   what is not the sum of two finite, distinct, non-opposite points: 10 = the accumulator after the call (p + q where it accepts, p
 *   where it refuses), 11 = q where it accepts, infinity where it refuses,
 *   12 - 15 = one step of the ACCUMULATION LOOP's fast half as msm.hip takes it (q affine: z == 1, or infinity): q at infinity is
 *   refused by the loop's own test, every other q goes to the straight-path mixed addition (curve.h), which refuses a q that may be
 *   equal or opposite to p -- a cheap necessary test, so a refusal of another pair is allowed -- without touching the accumulator:
 *   12 = madd_fast(p, q): the accumulator after the step, narrowed (p + q where it accepts, p unchanged where it refuses),
 *   13 = the same step: q where it accepts, infinity where it refuses; 14 / 15 = the same two for mmadd_fast, the affine + affine
 *   form of a task's second entry: every p must be affine with z == 1, any other p is WSNARK_ERR_ARG.  impl 0-3; the tails' paired
 *   and lane-split curves (impl 4, 5, 6) do not have these functions: WSNARK_ERR_ARG.
 *   impl 5 (g = 1) and 6 (g = 2): the lane-split tail curves (one point on two / four lanes), ops 0, 1, 3, 10, 11. */
int wsnark_selftest_curve(int g, int impl, int op, const void* p, const void* q, void* out, uint64_t n);
/* The radix-2^29 field (csrc/field29.h) on RAW limbs, one lane per case: the operand bounds its contracts allow cannot be reached
 * through the packed 32-byte form (8p, 10p and 16p do not fit it, a carry-free sum's limbs are not tight, and to_internal turns every
 * input into an ordinary representative below 2p), so here the nine 29-bit limbs of every operand (value = sum v[i] 2^(29 i); the top
 * limb takes the rest) reach the function under test exactly as given, and the result's limbs come back as returned.
 *   which   : 0 = Fq, 1 = Fr
 *   impl    : 0 = device Field29<P> (the noinline products: mad_chain.h on the GPU), 3 = device Field29I<P> (Fq only: the inlined
 *             products and mul2add_inl of the reduction tails), 2 = the same functions run on the host (the C bodies)
 *   operands: n x arity(op) x 9 uint32_t (the extension's ops: arity x 18, (c0, c1)); nothing is reduced or converted on the way in
 *   out     : n x 9 uint32_t (the extension's ops: 18), nothing canonicalised; predicates write 0 or 1 in limb 0; ops that return the
 *             32-byte form write its eight 32-bit words and 0 in the ninth
 * Unknown which / impl / op: WSNARK_ERR_ARG.  n <= 2^20. */
enum {
    WSNARK_F29_MUL = 0,            /* 2: mul(a, b)                                                   */
    WSNARK_F29_SQR = 1,            /* 1: sqr(a)                                                      */
    WSNARK_F29_MUL_INL = 2,        /* 2: mul_inl(a, b)                                               */
    WSNARK_F29_MUL2ADD = 3,        /* 4: mul2add(a, b, c, d) = a b + c d                             */
    WSNARK_F29_MUL2ADD_INL = 4,    /* 4: mul2add_inl(a, b, c, d)                                     */
    WSNARK_F29_MUL4ADD = 5,        /* 8: mul4add(a, ..., h) = a b + c d + e f + g h                  */
    WSNARK_F29_MULSUB2 = 6,        /* 4: mulsub2(a, b, c, d) = a b - c d                             */
    WSNARK_F29_ADD = 7,            /* 2 */
    WSNARK_F29_SUB = 8,            /* 2 */
    WSNARK_F29_NEG = 9,            /* 1 */
    WSNARK_F29_SUB_WEAK = 10,      /* 2: a - b + 2p                                                  */
    WSNARK_F29_SUB_WEAK4 = 11,     /* 2: a - b + 4p                                                  */
    WSNARK_F29_SUB_WEAK8 = 12,     /* 2: a - b + 8p                                                  */
    WSNARK_F29_NEG_WEAK = 13,      /* 1: 2p - a                                                      */
    WSNARK_F29_NEG_WEAK4 = 14,     /* 1: 4p - a                                                      */
    WSNARK_F29_ADD_NR = 15,        /* 2: a + b, carries propagated, no reduction                     */
    WSNARK_F29_ADD_LAZY_MUL = 16,  /* 3: mul(add_lazy(a, b), c): the carry-free sum is valid inside a product only */
    WSNARK_F29_FOLD8 = 17,         /* 1 */
    WSNARK_F29_FOLD16 = 18,        /* 1 */
    WSNARK_F29_FOLD4TO2 = 19,      /* 1 */
    WSNARK_F29_COND_SUB_2P = 20,   /* 1 */
    WSNARK_F29_NARROW = 21,        /* 1 */
    WSNARK_F29_CANONICAL = 22,     /* 1 */
    WSNARK_F29_X3_WIDE = 23,       /* 3: x3_wide(rr, ppp, q) = rr - ppp - 2q + 6p                    */
    WSNARK_F29_SUB_WIDE = 24,      /* 2: a - b + 8p                                                  */
    WSNARK_F29_IS_ZERO = 25,       /* 1, predicate */
    WSNARK_F29_IS_ZERO_WEAK = 26,  /* 1, predicate */
    WSNARK_F29_IS_ZERO_WIDE = 27,  /* 1, predicate */
    WSNARK_F29_MAYBE_ZERO_WEAK = 28, /* 1, predicate (maybe_kp(a, 3)) */
    WSNARK_F29_MAYBE_ZERO_WIDE = 29, /* 1, predicate (maybe_kp(a, 9)) */
    WSNARK_F29_PACK_UNPACK = 30,   /* 1: pack(unpack(x)); x = eight 32-bit words, the ninth is ignored; out = eight words */
    WSNARK_F29_PACKED_IS_ZERO = 31,/* 1, predicate on eight 32-bit words                             */
    WSNARK_F29_TO_INTERNAL = 32,   /* 1: to_internal(x) of a raw 256-bit x (eight words)             */
    WSNARK_F29_FROM_INTERNAL = 33, /* 1: from_internal(a); out = eight words                         */
    WSNARK_F29_DBL = 34,           /* 1 */
    WSNARK_F29_EQ = 35,            /* 2, predicate */
    WSNARK_F29_FP2_MUL = 36,       /* 2 x 18: Fp2T<Fq29>::mul(a, b)            (which 0, impl 0 or 2) */
    WSNARK_F29_FP2_SQR = 37,       /* 1 x 18: Fp2T<Fq29>::sqr(a)                                      */
    WSNARK_F29_FP2_MULSUB2 = 38    /* 4 x 18: Fp2T<Fq29>::mulsub2(a, b, c, d) = a b - c d             */
};
int wsnark_selftest_field29(int which, int impl, int op, const uint32_t* operands, uint32_t* out, uint64_t n);
/* The Fp12 arithmetic of the batch verifier (csrc/fp12.h), one lane per element.
 * op 0 = a * b, 1 = a^2, 2 = 1 / a, 3 = a^(p^2), 4 = final exponentiation of a (the shipped path: easy part by inversion,
 * conjugation and Frobenius, then the hard exponent), 5 = final exponentiation by the plain exponent (p^12 - 1)/r;
 * impl 0 = the device Fp12 of pairing.hip, 2 = the host Fp12 of the single-proof verifier (ops 2-5 there by plain exponentiation:
 * the yardstick).  a, b, out: n x 384 bytes, twelve PLAIN little-endian Fq values, coefficient i of w^i = (c0, c1); n <= 2^16. */
int wsnark_selftest_fp12(int impl, int op, const void* a, const void* b, void* out, uint64_t n);
/* What the MSM's grouping pass and task planner (csrc/msm.hip: presort_*, msm_plan_emit*) write for a scalar vector, read back without
 * running a point kernel (tests/grouping_patterns.py holds the model it is compared with).
 *   scalars : n x 32 bytes, raw 256-bit little-endian values (host)
 *   table_c : 0 = a per-window plan; else a flat fixed-base table plan of that window width (4 .. 22)
 *   w_off, w_stride : the window shard (rank, world of the *_msm_windows entry points); 0, 1 = every window
 *   mask    : optional, n bytes (host): the plain plan is built first, then its masked variant as the prover builds one -- pairs with
 *             mask[i] == 0 left out -- and the variant is what is returned
 *   info    : WSNARK_MSM_PLAN_INFO_WORDS words, always written on WSNARK_OK and on WSNARK_ERR_SIZE: [0] c, [1] windows of the whole
 *             scalar, [2] owned windows, [3] w_off, [4] w_stride, [5] NB = 2^(c-1), [6] buckets, [7] flat, [8] task cap lmax,
 *             [9] hot-bucket threshold, [10] low bucket bits per bin, [11] index bits of a 4-byte entry, [12] bins, [13] 4-byte entries,
 *             [14] the one-pass scatter ran, [15] partial slots, [16] multi-task buckets, [17] tasks, [18] hot buckets, [19] hot slices,
 *             [20] length of vals (the end of the last bin), [21] threads per workgroup of the per-bin sort, [22] n, [23] 0.
 *             All zero for n == 0 and for a shard that owns no window.
 *   bstart, bend : info[6] words each (cap_buckets);  vals : info[20] words (cap_vals): index | sign << 31, table plans: window * n + i;
 *   tasks : info[17] x (dst, start, len), dst = bucket or 0x80000000 | partial slot (cap_tasks);
 *   multi : info[16] x (bucket, first_partial, ntasks) (cap_multi);
 *   hot   : info[18] x (bucket, first_partial, ntasks, task_base, rem_index, start, rem, slice_base) (cap_hot).
 * Capacities count records.  An array passed as NULL is not written: a first call with every array NULL returns the sizes.  An array
 * whose capacity is too small fails the call with WSNARK_ERR_SIZE before any array is written.  The call waits for the queue; it
 * leaves nothing behind that a later sum reads (every sum builds its own plan). */
#define WSNARK_MSM_PLAN_INFO_WORDS 24
int wsnark_selftest_msm_plan(const void* scalars, uint64_t n, uint32_t table_c, uint32_t w_off, uint32_t w_stride, const void* mask,
                             uint32_t* info, uint32_t* bstart, uint32_t* bend, uint64_t cap_buckets, uint32_t* vals, uint64_t cap_vals,
                             uint32_t* tasks, uint64_t cap_tasks, uint32_t* multi, uint64_t cap_multi, uint32_t* hot, uint64_t cap_hot);
/* The geometry the MSM's host driver decides for a plan (csrc/msm.hip: msm_plan_geometry) -- the sum's shape, the grouping pass, the
 * reduction tail --, from the size, the shard, the table's window width and the library's switches alone.  Pure host arithmetic: no
 * device, no wsnark_init (tests/golden/msm_geometry.json pins the production shapes and both sides of every rule).
 *   n        : pairs
 *   table_c  : 0 = a per-window plan; 4 .. 22 = a flat fixed-base table plan of that window width; WSNARK_MSM_TABLE_C_AUTO = a table
 *              plan of the width the library gives a resident key of n pairs (msm_table_window; WSNARK_TABLE_C overrides)
 *   rank, world : the window shard; 0, 1 = every window
 *   words    : WSNARK_MSM_GEOMETRY_WORDS words.
 *              the sum's shape: [0] n, [1] c, [2] windows of the whole scalar, [3] owned windows, [4] w_off, [5] w_stride, [6] NB = 2^(c-1),
 *                [7] buckets, [8] flat, [9] task cap lmax, [10] hot-bucket threshold, [11] capacity of the task list;
 *              the grouping pass: [12] low bucket bits per bin, [13] index bits of an entry, [14] bins, [15] threads of the per-bin sort (0:
 *                msm_plan_finish sets it), [16] bins per bucket set, [17] scalars per workgroup, [18] its threads, [19] the plan has a grouping pass (1), [20] 4-byte entries;
 *              the reduction tail: [21] pieces, [22] buckets per piece, [23] pieces per group, [24] groups, [25] buckets per chunk,
 *                [26] chunks folded by the second level (1: none), [27] their product m, [28] chunk pairs per piece, [29] pairs the trees
 *                see J, [30] ceil(log2 J), [31] rows per piece, [32] rows per group that reach the host, [33] rows folded on the GPU.
 *              All zero on an error, for n == 0 and for a shard that owns no window.
 * Returns what msm_plan_geometry returns: WSNARK_ERR_SIZE (n > 2^28, n x owned windows >= 2^32, table rows x n >= 2^31, more bins
 * than the grouping pass has counters for), WSNARK_ERR_ARG (world == 0, a width outside 2 .. 22). */
#define WSNARK_MSM_GEOMETRY_WORDS 34
#define WSNARK_MSM_TABLE_C_AUTO 0xFFFFFFFFu
int wsnark_selftest_msm_geometry(uint64_t n, uint32_t table_c, uint32_t rank, uint32_t world, uint32_t* words);
/* The MSM's accumulation kernel (csrc/msm.hip: msm_accumulate, the __global__ function every sum launches) on tasks the caller wrote,
 * so that a test decides which entry meets which running sum (tests/accumulate_patterns.py holds the model of the loop's branches).
 *   g       : 1 or 2
 *   points  : n_points affine points in the reference's Montgomery format (64 / 128 B, as wsnark_g{1,2}_multiexp takes them; an
 *             all-zero record is infinity), brought to the device form by the conversion every sum uses
 *   vals    : n_vals words index | sign << 31, exactly what the grouping pass writes (sign: the point is subtracted)
 *   tasks   : n_tasks x (start, len): task t sums vals[start .. start + len); ranges may overlap; len 0 gives infinity
 *   out     : n_tasks affine-normalised Jacobian-Montgomery points ((x, y, 1) or (0, 1, 0); 96 / 192 B) like every group element this
 *             ABI returns
 * Task t is stored to bucket t when t is even and to partial slot t when t is odd, so both stores of the kernel run; the task count
 * sits in device memory and the grid is whole workgroups of 256, as a sum's.  Both result arrays carry a workgroup of extra slots and
 * are pre-filled with a byte pattern: a slot that no task names and does not hold the pattern afterwards, or a named slot that still
 * does, fails the call with WSNARK_ERR_FORMAT (wsnark_last_error names the slot).  Everything is checked on the host BEFORE anything is
 * launched: an index >= n_points, start + len > n_vals, n_points or n_vals > 2^20, n_tasks > 2^16, g not 1 or 2, a null pointer
 * with a non-zero count: WSNARK_ERR_ARG, and out is not written.  The hook allocates and frees its own buffers, waits for the queue
 * and leaves nothing behind that a later sum reads. */
int wsnark_selftest_msm_accumulate(int g, const void* points, uint64_t n_points, const uint32_t* vals, uint64_t n_vals, const uint32_t* tasks,
                                   uint64_t n_tasks, void* out);

/* ---- measurement hooks (bench.py) ---- */
/* A/B switches of the library (queue arrangement of a proof, reduction-tail geometry, ...; the names are the WSNARK_<name>
 * environment variables DESIGN.md lists, without the prefix): an override set here wins over the environment and is read by
 * every later call, so that one process can time several settings on one resident key.  value == INT64_MIN forgets the
 * override.  Results never depend on these switches -- only the schedule does. */
int wsnark_tuning_set(const char* name, int64_t value);
/* per-kernel HIP-event timing on the stream the kernels are launched on: 0 = off, 1 = every kernel,
 * 2 = only the dominant kernel (msm_accumulate_*), for timed regions where the brackets themselves must
 * stay out of the way */
void wsnark_timing_enable(int on);
void wsnark_timing_reset(void);
/* writes "name total_ms launches\n" lines; returns bytes needed (excluding NUL) */
size_t wsnark_timing_report(char* buf, size_t cap);
/* The integer roofline's peak, measured on the device in use (about 10 ms each): probe 0 = a dependent chain of the
 * library's own radix-2^29 Montgomery product on every lane, 8 x 256 lanes per CU (Gmodmul/s: what a kernel of nothing
 * but products reaches); 1 = the same with the inlined product body; 2 = eight independent v_mad_u64_u32 chains per lane
 * (Gmad/s: the raw 32x32+64 multiply-add issue rate).  3, 4 = traffic calibration kernels for the
 * FETCH_SIZE counter (run under rocprofv3 --pmc by tools/gpu_session.sh): 3 = 2^25 pseudo-random 64-byte point gathers out
 * of a 1 GiB table (the accumulation kernel's access pattern; 2 GiB of known bytes per launch, kernel
 * `probe_gather64_kernel`), 4 = a 16-B-per-lane streaming read of the same 1 GiB (`probe_stream16_kernel`); both return
 * GB/s of those known bytes.  5 = one field inversion per lane (the library's Fermat inversion on the radix-2^29 product,
 * every lane busy): G inversions/s -- what a lane-parallel batch inversion costs per batch. */
int wsnark_peak_probe(int probe, double* gops_per_s);

#ifdef __cplusplus
}
#endif
#endif
