// pkeydelta.hip -- the phase-2 contribution to a Groth16 proving key (wsnark_pkey_contribute* / wsnark_pkey_delta_verify*,
// wsnark_g{1,2}_scale_batch; include/wsnark.h).
//
// A key holds C_j = (.../delta) G1, hExps_i = (tau^i Z(tau)/delta) G1, delta1 = delta G1, delta2 = delta G2.  A contribution by d
// replaces delta by delta d:   delta1' = d delta1, delta2' = d delta2 (host curve, two multiplications),
//                              C'_j = d^-1 C_j, hExps'_i = d^-1 hExps_i (device, one multiplication per point),
// everything else byte for byte as it was.  The device work is the opposite shape of mul_base_kernel (one base, a scalar per lane,
// divergent): here every lane has its own base and the whole launch shares ONE scalar.
//
//   scale_points_kernel<C>: one lane per point (reference format in and out).  The scalar never comes from memory: the host recodes
//     it once into non-adjacent form (digits -1, 0, 1; on average 1/3 of them non-zero: ~85 additions behind the 253 doublings
//     instead of ~127) and passes the two digit masks in the argument block, so the loop's branches are scalar branches and no
//     wavefront diverges on them.  A negative digit is madd's negate flag.  The chain itself is keybytes.h's naf_chain.
//     Before the chain each lane classifies its point with the audit's own code (keybytes.h: pk_classify -- infinity by the loaders'
//     rule, every coordinate < q, the curve equation); counts and the first bad index are reduced by the audit's pk_reduce and read
//     by its pk_decode.  An infinity point is copied through.
//     Products per finite point on G1 (counted from curve.h's formulas, squarings as products, the fused Y3 as two): input tests
//     2 + 3, chain 253 x 9 (dbl) + ~85 x 11 (madd), normalisation 24 + 363 / 4 + 5, output 2: ~3350.
//   normalisation: ONE inversion per workgroup (keybytes.h: block_inverse): a product tree over the 256 lanes' ZZ ZZZ in LDS (8
//     levels up), wavefront 0 inverts the root while the other three wait, 8 levels down give every lane its own inverse.
//
//   streaming: a section goes through the staging ring in chunks of PKDELTA_CHUNK points (default 2^18); chunk k + 1 is staged on
//     the lane's copy queue while chunk k's kernel runs on its first queue, and chunk k's result comes down into one of two pinned
//     buffers that the host empties while chunk k + 1 runs.  Device memory: 4 x 64 B x chunk, whatever the key's size.
//
//   wsnark_pkey_delta_verify: what the NEXT participant checks -- the new key is the old one under a new delta.  bit 0: a memcmp of
//     everything a contribution must not touch; bit 1: e(delta1', G2) = e(G1, delta2'); bits 2, 3: with rho_j the audit's (ChaCha20,
//     the global index) e(sum rho_j C'_j, delta2') = e(sum rho_j C_j, delta2), and the same for hExps, by the ordinary MSMs chunk by
//     chunk (keybytes.h: RhoSum) and two host Miller loops each (same_pairing); bit 4: delta2' != delta2.
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "keybytes.h"

namespace wsnark {

using namespace hostpair;

// ---- device ----
// (the scalar in non-adjacent form, the chain over its digits, the shared inversion and the affine result: keybytes.h)
template <class C>
__global__ __launch_bounds__(256) void scale_points_kernel(const typename C::AffP* __restrict__ pts, uint64_t n, uint64_t base, ScaleDigits D,
                                                             typename C::El curve_b, typename C::AffP* __restrict__ out, PkAcc* __restrict__ acc) {
    typedef typename C::Field F;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int st = 0;               // pk_reduce's states: 0 good, 1 unreduced, 2 off the curve, 4 infinity
    bool live = false;        // a good finite point and a non-zero scalar: this lane runs the chain
    typename C::Aff P = typename C::Aff{F::zero(), F::zero()};
    if (i < n) {
        st = pk_classify<C>(pts[i], curve_b, &P);
        live = st == 0 && D.top >= 0;
    }
    pk_reduce(st, base + i, acc);

    // the chain starts as P itself (finite: x != 0 was decided above)
    typename C::Pt a = C::infinity();
    if (live) {
        a = typename C::Pt{P.x, P.y, F::one(), F::one()};
        naf_chain<C>(a, P, D.nz[0], D.nz[1], D.nz[2], D.nz[3], D.neg[0], D.neg[1], D.neg[2], D.neg[3], D.top);
    }
    const bool fin = live && !C::is_inf(a);

    // one inversion per workgroup (blockDim.x == 256): every lane arrives, a lane with nothing to normalise passes 1
    const typename C::El inv = block_inverse<F>(fin ? F::mul(a.zz, a.zzz) : F::one());
    if (i < n) out[i] = st == 4 ? pts[i] : affine_result<C>(a, fin, inv, 1);      // infinity: copied through byte for byte
}

// ---- host ----
namespace {
template <class C> const char* scale_name() {
    return sizeof(typename C::AffP) == 64 ? "scale_points_g1_shared_inv" : "scale_points_g2_shared_inv";
}

// where a scaled chunk goes: caller memory, or a file
struct Sink {
    uint8_t* mem = nullptr;
    int fd = -1;
    uint64_t off = 0;
    int put(uint64_t at, const uint8_t* p, size_t n) const {
        if (mem) { memcpy(mem + at, p, n); return WS_OK; }
        size_t done = 0;
        while (done < n) {
            const ssize_t r = pwrite(fd, p + done, n - done, (off_t)(off + at + done));
            if (r < 0) {
                if (errno == EINTR) continue;
                set_last_error(std::string("key file: write failed: ") + strerror(errno));
                return WS_ERR_ARG;
            }
            done += (size_t)r;
        }
        return WS_OK;
    }
};

// two of everything a chunk in flight needs; the pending download of the chunk before
struct ScaleRing {
    hipStream_t s = nullptr, sc = nullptr;
    DevBuf d_in[2], d_out[2];
    uint8_t* pin[2] = {nullptr, nullptr};
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
    unsigned k = 0;
    struct { bool on = false; const Sink* sink = nullptr; uint64_t at = 0; size_t bytes = 0; int b = 0; } pend;
    int init(hipStream_t s_, hipStream_t sc_, size_t bytes) {
        s = s_; sc = sc_;
        for (int b = 0; b < 2; b++) {
            WS_HIP_CHECK(d_in[b].alloc(bytes));
            WS_HIP_CHECK(d_out[b].alloc(bytes));
            WS_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&pin[b]), bytes ? bytes : 16, 0));
            WS_HIP_CHECK(hipEventCreateWithFlags(&ev_up[b], hipEventDisableTiming));
            WS_HIP_CHECK(hipEventCreateWithFlags(&ev_done[b], hipEventDisableTiming));
        }
        return WS_OK;
    }
    int drain() {
        if (!pend.on) return WS_OK;
        pend.on = false;
        WS_HIP_CHECK(hipEventSynchronize(ev_done[pend.b]));
        return pend.sink->put(pend.at, pin[pend.b], pend.bytes);
    }
    ~ScaleRing() {      // (also the error paths: nothing may still read or write the buffers)
        if (sc) (void)hipStreamSynchronize(sc);
        if (s) (void)hipStreamSynchronize(s);
        for (int b = 0; b < 2; b++) {
            if (pin[b]) (void)hipHostFree(pin[b]);
            if (ev_up[b]) (void)hipEventDestroy(ev_up[b]);
            if (ev_done[b]) (void)hipEventDestroy(ev_done[b]);
        }
    }
};

// sink[at ..] = k * src[0 .. n), chunk by chunk.  The last chunk's download is still pending when this returns (R.drain()).
template <class C>
int scale_stream(Context* X, ScaleRing& R, const uint8_t* src, uint64_t n, uint64_t chunk, const ScaleDigits& D, const typename C::El& cb,
                 const Sink& sink, PkAcc* d_acc, void (*release)(const void*, size_t)) {
    typedef typename C::AffP AffP;
    const size_t psz = sizeof(AffP);
    int rc;
    for (uint64_t lo = 0; lo < n; lo += chunk) {
        const uint64_t m = std::min<uint64_t>(chunk, n - lo);
        const int b = (int)(R.k++ & 1);
        // buffers b were last used by the chunk before the previous one: its download has been waited for (drain below, one lap ago),
        // so its kernel has read d_in[b], the copy has read d_out[b], and the host has emptied pin[b]
        if ((rc = stage_chunk(R.d_in[b].p, src + lo * psz, (size_t)m * psz, R.sc, release))) return rc;
        WS_HIP_CHECK(hipEventRecord(R.ev_up[b], R.sc));
        WS_HIP_CHECK(hipStreamWaitEvent(R.s, R.ev_up[b], 0));
        X->timer.begin(scale_name<C>(), R.s);
        hipLaunchKernelGGL(scale_points_kernel<C>, dim3(ceil_div_u64(m, 256)), dim3(256), 0, R.s, R.d_in[b].as<AffP>(), m, lo, D, cb,
                           R.d_out[b].as<AffP>(), d_acc);
        WS_HIP_CHECK(hipGetLastError());
        X->timer.end(R.s);
        WS_HIP_CHECK(hipMemcpyAsync(R.pin[b], R.d_out[b].p, (size_t)m * psz, hipMemcpyDeviceToHost, R.s));
        WS_HIP_CHECK(hipEventRecord(R.ev_done[b], R.s));
        if ((rc = R.drain())) return rc;      // the chunk before: its kernel ran while this one was staged
        R.pend.on = true; R.pend.sink = &sink; R.pend.at = lo * psz; R.pend.bytes = (size_t)m * psz; R.pend.b = b;
    }
    return WS_OK;
}

template <class C>
int scale_batch(const void* points, uint64_t n, const void* k32, void* out) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (n == 0) return WS_OK;
    if (!points || !k32 || !out) return WS_ERR_ARG;
    if (n > ((uint64_t)1 << 28)) return WS_ERR_SIZE;
    typename C::El cb;
    int rc = curve_b(&cb);
    if (rc) return rc;
    ScaleDigits D;
    naf_digits(load_scalar((const uint8_t*)k32), &D);
    const uint64_t chunk = key_chunk("PKDELTA_CHUNK");
    PkAcc h_acc;
    {
        LaneLock L = acquire_lane(X);
        DevBuf d_acc;
        WS_HIP_CHECK(d_acc.alloc(sizeof(PkAcc)));
        WS_HIP_CHECK(hipMemsetAsync(d_acc.p, 0, sizeof(PkAcc), L->stream));
        ScaleRing R;
        if ((rc = R.init(L->stream, L->stream_copy, (size_t)std::min<uint64_t>(chunk, n) * sizeof(typename C::AffP)))) return rc;
        Sink sink;
        sink.mem = (uint8_t*)out;
        if ((rc = scale_stream<C>(X, R, (const uint8_t*)points, n, chunk, D, cb, sink, d_acc.as<PkAcc>(), nullptr))) return rc;
        if ((rc = R.drain())) return rc;
        WS_HIP_CHECK(hipMemcpyAsync(&h_acc, d_acc.p, sizeof h_acc, hipMemcpyDeviceToHost, L->stream));
        WS_HIP_CHECK(hipStreamSynchronize(L->stream));
    }
    uint64_t inf, bad, first;
    uint32_t reason;
    pk_decode(h_acc, &inf, &bad, &first, &reason);
    if (bad) {
        set_last_error("scale_batch: " + std::to_string(bad) + " point(s) unreduced or off the curve, the first at index " + std::to_string(first));
        return WS_ERR_FORMAT;
    }
    return WS_OK;
}

// the secret of one contribution: d, and the digits of d^-1; wiped when it goes
struct Secret {
    Fe d;
    ScaleDigits inv_digits;
    ~Secret() { wipe(this, sizeof *this); }
};
// everything that can fail before a byte is written
int contribute_prepare(const KeySections& S, const uint8_t* d32, Secret* K) {
    if (!ctx()) return WS_ERR_NOINIT;
    int rc = key_shape_check(S);
    if (rc) return rc;
    uint8_t raw[32];
    if ((rc = draw_seed(d32, raw))) return rc;
    K->d = load_scalar(raw);
    wipe(raw, sizeof raw);
    if (Fr::is_zero(K->d)) { set_last_error("contribution: d = 0 mod r"); return WS_ERR_ARG; }
    Fe dinv = Fr::from_mont(Fr::inv(Fr::to_mont(K->d)));
    naf_digits(dinv, &K->inv_digits);
    wipe(&dinv, sizeof dinv);
    return WS_OK;
}

int contribute_run(const KeySections& S, const Secret& K, const Sink& outC, const Sink& outH, uint8_t* out_d1, uint8_t* out_d2,
                   wsnark_pkey_delta_report_t* rep) {
    Context* X = ctx();
    const auto t_begin = Clock::now();
    wsnark_pkey_delta_report_t R;
    memset(&R, 0, sizeof R);
    const KeyCounts all = key_counts(S);
    const uint64_t counts[2] = {all[WSNARK_PK_C], all[WSNARK_PK_H]};
    for (int k = 0; k < 2; k++) { R.points[k] = counts[k]; R.first_bad[k] = UINT64_MAX; }

    // delta1' = d delta1, delta2' = d delta2: the host curve of proof assembly
    auto t0 = Clock::now();
    G1A d1;
    G2A d2;
    const bool fixed_ok = fixed_g1(S.delta1, true, &d1) == 0 && fixed_g2(S.delta2, true, &d2) == 0;
    if (fixed_ok) {
        G1::Pt p1 = G1::mul_bytes(G1::Pt{d1.x, d1.y, Fq::one(), Fq::one()}, reinterpret_cast<const uint8_t*>(&K.d), 32);
        G2::Pt p2 = G2::mul_bytes(G2::Pt{d2.x, d2.y, Fq2::one(), Fq2::one()}, reinterpret_cast<const uint8_t*>(&K.d), 32);
        const Jac<Fq> j1 = G1::to_affine_jac(p1);       // (d != 0 mod r and both points have order r: never infinity)
        const Jac<Fq2> j2 = G2::to_affine_jac(p2);
        memcpy(out_d1, &j1, 64);
        memcpy(out_d2, &j2, 128);
        wipe(&p1, sizeof p1);
        wipe(&p2, sizeof p2);
    }
    double ms_host = ms_since(t0), ms_dev = 0;

    PkAcc h_acc[2];
    memset(h_acc, 0, sizeof h_acc);
    if (fixed_ok) {
        t0 = Clock::now();
        G1R29::El cb;
        int rc = curve_b(&cb);
        if (rc) return rc;
        const uint64_t chunk = key_chunk("PKDELTA_CHUNK");
        LaneLock L = acquire_lane(X);
        DevBuf d_acc;
        WS_HIP_CHECK(d_acc.alloc(sizeof h_acc));
        WS_HIP_CHECK(hipMemsetAsync(d_acc.p, 0, sizeof h_acc, L->stream));
        ScaleRing ring;
        const uint64_t cap = key_chunk_cap(chunk, std::max(counts[0], counts[1]));
        if ((rc = ring.init(L->stream, L->stream_copy, (size_t)cap * 64))) return rc;
        if ((rc = scale_stream<G1R29>(X, ring, S.Cpts, counts[0], chunk, K.inv_digits, cb, outC, d_acc.as<PkAcc>(), S.release))) return rc;
        if ((rc = scale_stream<G1R29>(X, ring, S.H, counts[1], chunk, K.inv_digits, cb, outH, d_acc.as<PkAcc>() + 1, S.release))) return rc;
        if ((rc = ring.drain())) return rc;
        WS_HIP_CHECK(hipMemcpyAsync(h_acc, d_acc.p, sizeof h_acc, hipMemcpyDeviceToHost, L->stream));
        WS_HIP_CHECK(hipStreamSynchronize(L->stream));
        ms_dev = ms_since(t0);
    }
    bool ok = fixed_ok;
    for (int k = 0; k < 2; k++) {
        pk_decode(h_acc[k], &R.infinity[k], &R.bad[k], &R.first_bad[k], &R.first_reason[k]);
        ok = ok && R.bad[k] == 0;
    }
    R.ok = ok ? 1 : 0;
    R.ms[0] = ms_dev;
    R.ms[1] = ms_host;
    R.ms[2] = ms_since(t_begin);
    *rep = R;
    return WS_OK;
}
}  // namespace

// the kernel alone, on points that are already on the device (pkeysetup.hip: the 1/n of an inverse group transform)
template <class C>
static int scale_dev(Context* X, const void* d_in, uint64_t n, const ScaleDigits& D, void* d_out, PkAcc* d_acc, hipStream_t s) {
    typedef typename C::AffP AffP;
    typename C::El cb;
    const int rc = curve_b(&cb);
    if (rc) return rc;
    X->timer.begin(scale_name<C>(), s);
    hipLaunchKernelGGL(scale_points_kernel<C>, dim3(ceil_div_u64(n, 256)), dim3(256), 0, s, reinterpret_cast<const AffP*>(d_in), n, (uint64_t)0, D, cb,
                       reinterpret_cast<AffP*>(d_out), d_acc);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    return WS_OK;
}
int g1_scale_dev(Context* X, const void* d_in, uint64_t n, const ScaleDigits& D, void* d_out, PkAcc* d_acc, hipStream_t s) {
    return scale_dev<G1R29>(X, d_in, n, D, d_out, d_acc, s);
}
int g2_scale_dev(Context* X, const void* d_in, uint64_t n, const ScaleDigits& D, void* d_out, PkAcc* d_acc, hipStream_t s) {
    return scale_dev<G2R29>(X, d_in, n, D, d_out, d_acc, s);
}

int g1_scale_batch(const void* points, uint64_t n, const void* k32, void* out) { return scale_batch<G1R29>(points, n, k32, out); }
int g2_scale_batch(const void* points, uint64_t n, const void* k32, void* out) { return scale_batch<G2R29>(points, n, k32, out); }

int pkey_contribute_sections(const KeySections& S, const uint8_t* d32, uint8_t* out_pointsC, uint8_t* out_pointsH, uint8_t* out_delta1,
                             uint8_t* out_delta2, wsnark_pkey_delta_report_t* rep) {
    if (!rep || !out_pointsH || !out_delta1 || !out_delta2 || (!out_pointsC && (uint64_t)S.n_vars > (uint64_t)S.n_public + 1)) return WS_ERR_ARG;
    Secret K;
    int rc = contribute_prepare(S, d32, &K);
    if (rc) return rc;
    Sink sc, sh;
    sc.mem = out_pointsC;
    sh.mem = out_pointsH;
    return contribute_run(S, K, sc, sh, out_delta1, out_delta2, rep);
}

// the key's image: a copy of the input with the four parts overwritten
int pkey_contribute_bytes(const KeySections& S, const uint8_t* pkey, size_t len, const uint8_t* d32, uint8_t* out, size_t out_cap,
                          wsnark_pkey_delta_report_t* rep) {
    int rc;
    if (out_cap < len) { set_last_error("contribution: the output buffer is smaller than the key"); return WS_ERR_SIZE; }
    Secret K;
    if ((rc = contribute_prepare(S, d32, &K))) return rc;
    if (out != pkey) memcpy(out, pkey, len);
    Sink sc, sh;
    sc.mem = out + (S.Cpts - pkey);
    sh.mem = out + (S.H - pkey);
    uint8_t d1[64], d2[128];
    rc = contribute_run(S, K, sc, sh, d1, d2, rep);
    if (rc == WS_OK && rep->ok) {
        memcpy(out + (S.delta1 - pkey), d1, 64);
        memcpy(out + (S.delta2 - pkey), d2, 128);
    }
    return rc;
}

int pkey_contribute_file(const KeySections& S, const KeyFile& F, const char* in_path, const char* out_path, const uint8_t* d32,
                         wsnark_pkey_delta_report_t* rep) {
    int rc;
    struct stat si, so;
    if (strcmp(in_path, out_path) == 0 ||
        (fstat(F.fd, &si) == 0 && stat(out_path, &so) == 0 && si.st_dev == so.st_dev && si.st_ino == so.st_ino)) {
        set_last_error("contribution: the input and the output are the same file");
        return WS_ERR_ARG;
    }
    Secret K;
    if ((rc = contribute_prepare(S, d32, &K))) return rc;
    const int fd = open(out_path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd < 0) { set_last_error(std::string("key file: cannot create ") + out_path + ": " + strerror(errno)); return WS_ERR_ARG; }
    struct Closer {
        int fd; const char* path; bool keep;
        ~Closer() { close(fd); if (!keep) unlink(path); }
    } closer{fd, out_path, false};
    // everything but C and hExps as it is, in pieces that go back to the kernel as soon as they are written
    const KeyCounts counts = key_counts(S);
    uint64_t skip[2][2] = {{(uint64_t)(S.Cpts - F.base), counts[WSNARK_PK_C] * 64}, {(uint64_t)(S.H - F.base), counts[WSNARK_PK_H] * 64}};
    if (skip[1][0] < skip[0][0]) std::swap(skip[0], skip[1]);
    Sink whole;
    whole.fd = fd;
    const auto t_copy = Clock::now();
    uint64_t at = 0;
    for (int k = 0; k <= 2; k++) {
        const uint64_t end = k < 2 ? skip[k][0] : (uint64_t)F.len;
        for (; at < end;) {
            const size_t piece = (size_t)std::min<uint64_t>(end - at, (uint64_t)16 << 20);
            if ((rc = whole.put(at, F.base + at, piece))) return rc;
            if (S.release) S.release(F.base + at, piece);
            at += piece;
        }
        if (k < 2) at = std::max(at, skip[k][0] + skip[k][1]);
    }
    if (ftruncate(fd, (off_t)F.len) != 0) { set_last_error(std::string("key file: cannot size the output: ") + strerror(errno)); return WS_ERR_ARG; }
    const double ms_copy = ms_since(t_copy);
    Sink sc, sh;
    sc.fd = sh.fd = fd;
    sc.off = (uint64_t)(S.Cpts - F.base);
    sh.off = (uint64_t)(S.H - F.base);
    uint8_t d1[64], d2[128];
    wsnark_pkey_delta_report_t R;
    if ((rc = contribute_run(S, K, sc, sh, d1, d2, &R))) return rc;
    if (R.ok) {
        if ((rc = whole.put((uint64_t)(S.delta1 - F.base), d1, 64)) || (rc = whole.put((uint64_t)(S.delta2 - F.base), d2, 128))) return rc;
        closer.keep = true;
    }
    R.ms[1] += ms_copy;
    R.ms[2] += ms_copy;
    *rep = R;
    return WS_OK;
}

int pkey_delta_verify_sections(const KeySections& O, const KeySections& N, const uint8_t* seed32, wsnark_pkey_delta_verdict_t* out) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (!out) return WS_ERR_ARG;
    int rc;
    if ((rc = key_shape_check(O)) || (rc = key_shape_check(N))) return rc;
    uint8_t seed[32];
    if ((rc = draw_seed(seed32, seed))) return rc;
    const auto t_begin = Clock::now();
    wsnark_pkey_delta_verdict_t V;
    memset(&V, 0, sizeof V);

    // bit 0: what a contribution must not touch
    const bool same_shape = O.n_vars == N.n_vars && O.n_public == N.n_public && O.domain == N.domain && O.lenA == N.lenA && O.lenB == N.lenB;
    V.checks_run |= 1;
    {
        bool same = same_shape;
        auto cmp = [&](const uint8_t* a, const uint8_t* b, uint64_t n) {
            for (uint64_t at = 0; same && at < n; at += (uint64_t)16 << 20) {      // in pieces: a mapped file gets its pages back
                const size_t piece = (size_t)std::min<uint64_t>(n - at, (uint64_t)16 << 20);
                same = memcmp(a + at, b + at, piece) == 0;
                if (O.release) O.release(a + at, piece);
                if (N.release) N.release(b + at, piece);
            }
        };
        if (same) {
            const uint64_t nv = O.n_vars;
            cmp(O.alfa1, N.alfa1, 64); cmp(O.beta1, N.beta1, 64); cmp(O.beta2, N.beta2, 128);
            cmp(O.polsA, N.polsA, O.lenA); cmp(O.polsB, N.polsB, O.lenB);
            cmp(O.A, N.A, nv * 64); cmp(O.B1, N.B1, nv * 64); cmp(O.B2, N.B2, nv * 128);
        }
        if (!same) V.checks_bad |= 1;
    }
    // bit 4: a contribution by 1 is none
    V.checks_run |= 16;
    if (memcmp(O.delta2, N.delta2, 128) == 0) V.checks_bad |= 16;
    // bit 1: the new delta1 and delta2 hold the same logarithm
    G1A n1;
    G2A n2, o2;
    double ms_pair = 0;
    if (fixed_g1(N.delta1, true, &n1) == 0 && fixed_g2(N.delta2, true, &n2) == 0) {
        const auto t0 = Clock::now();
        V.checks_run |= 2;
        if (!same_log(n1, n2)) V.checks_bad |= 2;
        ms_pair += ms_since(t0);
    }
    // bits 2, 3: only behind a delta2' that is what delta1' is -- and only over sections of one length
    double ms_sums = 0;
    if (same_shape && (V.checks_run & 2) && !(V.checks_bad & 2)) {
        const auto t0 = Clock::now();
        fixed_g2(O.delta2, false, &o2);
        const KeyCounts all = key_counts(O);
        const uint64_t counts[2] = {all[WSNARK_PK_C], all[WSNARK_PK_H]};
        const uint8_t* src[2][2] = {{O.Cpts, N.Cpts}, {O.H, N.H}};
        G1A sums[2][2];
        {
            const uint64_t chunk = key_chunk("PKDELTA_CHUNK");
            const uint64_t cap = key_chunk_cap(chunk, std::max(counts[0], counts[1]));
            LaneLock L = acquire_lane(X);
            hipStream_t s = L->stream;
            DevBuf d_pts, d_rho;
            WS_HIP_CHECK(d_pts.alloc((size_t)cap * 64));
            WS_HIP_CHECK(d_rho.alloc((size_t)cap * 32));
            for (int sec = 0; sec < 2; sec++) {
                RhoSum<Fq> part[2];
                for (uint64_t lo = 0; lo < counts[sec]; lo += chunk) {
                    const uint64_t n = std::min<uint64_t>(chunk, counts[sec] - lo);
                    if ((rc = pkcheck_rho_dev(d_rho.as<Fe>(), n, lo, seed, s))) return rc;      // the SAME rho_j for the old and the new point j
                    for (int which = 0; which < 2; which++) {
                        if ((rc = stage_chunk(d_pts.p, src[sec][which] + lo * 64, (size_t)n * 64, s, (which ? N : O).release))) return rc;
                        if ((rc = part[which].add(*L, d_rho.as<Fe>(), d_pts.as<Affine<Fq>>(), n, s))) return rc;
                    }
                }
                WS_HIP_CHECK(hipStreamSynchronize(s));
                for (int which = 0; which < 2; which++) sums[sec][which] = part[which].finish();
            }
        }
        ms_sums = ms_since(t0);
        const auto t1 = Clock::now();
        for (int sec = 0; sec < 2; sec++) {
            V.checks_run |= 4u << sec;
            if (!same_pairing(sums[sec][1], n2, sums[sec][0], o2)) V.checks_bad |= 4u << sec;      // (the new sum, the old sum)
        }
        ms_pair += ms_since(t1);
    }
    wipe(seed, sizeof seed);
    V.ok = (V.checks_run == 31 && V.checks_bad == 0) ? 1 : 0;
    V.ms[0] = ms_sums;
    V.ms[1] = ms_pair;
    V.ms[2] = ms_since(t_begin);
    *out = V;
    return WS_OK;
}

}  // namespace wsnark
