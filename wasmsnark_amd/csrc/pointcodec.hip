// pointcodec.hip -- compressed points and 128-byte proofs (wsnark_g1/g2_compress, _decompress, wsnark_proof_compress / _decompress,
// wsnark_groth16_verify_batch_compressed[_dev]; include/wsnark.h has the two encodings byte by byte).
//
// One lane per point on the radix-2^29 field, as the light kernels of pkeycheck.hip:
//   compress     x == 0 (every word): infinity by the loaders' rule; a coordinate word string >= q: status 1, a zero record; else
//                the plain x with the two flag bits in its top byte.  The sign is "y is the larger root" (field.h: ws_gt_half; on G2
//                decided on y.c1, on y.c0 if that is zero).  The curve equation is NOT tested: that is the audit's job (pkeycheck.hip).
//   decompress   the flags and the range of x (WSNARK_DEC_MALFORMED), y = sqrt(x^3 + b) (none: WSNARK_DEC_NO_POINT; field.h, fp2.h: one
//                windowed chain on G1, two on G2, no inversion), the root the sign bit names, and on request the audit's [r] Q == O
//                chain on G2 (WSNARK_DEC_OUTSIDE_SUBGROUP).  The smallest reason wins, as in the audit; a bad point is written as zeros.
// Both read and write records at a stride, so the same kernels serve arrays of points (stride = the record) and the three points of a
// proof (strides 128 and 384).  Arrays stream through the staging ring in chunks of CODEC_CHUNK points (default 2^18): device memory
// does not grow with n.  Bad points are counted on the device (keybytes.h: pk_reduce).
// Proofs: A | B | C at 32 + 64 + 32 bytes <-> the prover's 384-byte record of plain integers; decompression writes z = 1.  The
// compressed verifier decompresses on the device into the very records verify_prepare_kernel (pairing.hip) reads -- a proof whose
// decompression failed is a zero record, which no curve equation accepts -- and the batch verifier runs on them unchanged.
#include <string.h>

#include <vector>

#include "fp12.h"
#include "keybytes.h"

namespace wsnark {

typedef Curve<Fq29> G1k;                    // products as calls, as in pkeycheck.hip
typedef G2R29 G2k;

// the records of one launch: record i is read at in + i in_stride + in_off and written at out + i out_stride + out_off
struct CodecIO {
    const uint8_t* in;
    uint64_t in_stride, in_off;
    uint8_t* out;
    uint64_t out_stride, out_off;
    uint8_t* status;                        // one byte per record at status[i st_stride + st_off]
    uint64_t st_stride, st_off;
    int raw;                                // 1: infinity is reported as 4 (the proof kernels need it); 0: as WSNARK_DEC_OK
};
struct CodecConsts {
    F29 to_int;                             // 2^522 mod q as a plain integer: plain x -> internal with one product (fp12.h)
};

__device__ inline Fe cd_rev(const Fe& x) {      // little-endian words <-> 32 big-endian bytes
    return Fe{{__builtin_bswap64(x.l[3]), __builtin_bswap64(x.l[2]), __builtin_bswap64(x.l[1]), __builtin_bswap64(x.l[0])}};
}
__device__ inline Fe cd_zero() { return Fe{{0, 0, 0, 0}}; }
// a stored coordinate word (key format: Montgomery; plain: the integer itself) <-> the field's internal form / the plain integer
__device__ inline F29 cd_load(const Fe& w, int plain, const CodecConsts& K) {
    return plain ? Fq29::mul(Fq29::unpack(w), K.to_int) : Fq29::to_internal(w);
}
__device__ inline Fe cd_store(const F29& a, int plain) { return plain ? Fq29::plain(a) : Fq29::from_internal(a); }
__device__ inline Fe cd_plain_of(const Fe& w, int plain) {      // x R 2^5 2^-261 = x
    return plain ? w : Fq29::pack(Fq29::canonical(Fq29::mul(Fq29::unpack(w), Fq29::from_words(32, 0, 0, 0))));
}

// One point (NE = 1: G1, 2: G2 words per coordinate) -> its record.  0 good, 1 a coordinate >= q, 4 infinity (the record then says so)
template <int NE>
__device__ inline int codec_encode(const Fe* __restrict__ pt, int enc, int plain, Fe* rec) {
    const uint64_t q[4] = {FqParams::P0, FqParams::P1, FqParams::P2, FqParams::P3};
    Fe x[NE], y[NE];
    bool inf = true, big = false;
    for (int k = 0; k < NE; k++) { x[k] = pt[k]; inf = inf && pk_zero(x[k]); }
    uint64_t f;                             // the two flag bits, as they sit in the top byte
    if (inf) {
        for (int k = 0; k < NE; k++) x[k] = cd_zero();
        f = 1;
    } else {
        for (int k = 0; k < NE; k++) y[k] = pt[NE + k];
        for (int k = 0; k < NE; k++) big = big || pk_ge(x[k], q) || pk_ge(y[k], q);
        if (big) {
            for (int k = 0; k < NE; k++) rec[k] = cd_zero();
            return 1;
        }
        for (int k = 0; k < NE; k++) x[k] = cd_plain_of(x[k], plain);
        // the larger root: decided on the last non-zero component (c1 before c0)
        const Fe ys = (NE == 2 && !pk_zero(y[NE - 1])) ? y[NE - 1] : y[0];
        const bool larger = ws_gt_half<FqParams>(cd_plain_of(ys, plain));
        f = enc == WSNARK_ENC_LE ? (larger ? 2 : 0) : (larger ? 3 : 2);
    }
    x[NE - 1].l[3] |= f << 62;
    for (int k = 0; k < NE; k++) rec[k] = enc == WSNARK_ENC_BE ? cd_rev(x[NE - 1 - k]) : x[k];
    return inf ? 4 : 0;
}

// One record -> its point in the field's internal form.  0 good, 1 .. 3 = WSNARK_DEC_*, 4 infinity
template <class C>
__device__ inline int codec_decode(const Fe* __restrict__ rec, int enc, uint32_t flags, const CodecConsts& K,
                                   const typename C::El& curve_b, typename C::Aff* P) {
    typedef typename C::Field F;
    constexpr int NE = (int)(sizeof(typename F::Packed) / 32);
    const uint64_t q[4] = {FqParams::P0, FqParams::P1, FqParams::P2, FqParams::P3};
    Fe w[NE];                               // the components of x, little-endian words
    for (int k = 0; k < NE; k++) w[k] = enc == WSNARK_ENC_BE ? cd_rev(rec[NE - 1 - k]) : rec[k];
    const uint32_t f = (uint32_t)(w[NE - 1].l[3] >> 62);
    w[NE - 1].l[3] &= ~((uint64_t)3 << 62);
    const bool le = enc == WSNARK_ENC_LE;
    if (le ? f == 3 : f == 0) return WSNARK_DEC_MALFORMED;
    if (f == 1) {
        bool zero = true;
        for (int k = 0; k < NE; k++) zero = zero && pk_zero(w[k]);
        return zero ? 4 : WSNARK_DEC_MALFORMED;
    }
    const bool sign = le ? f == 2 : f == 3;
    bool big = false;
    for (int k = 0; k < NE; k++) big = big || pk_ge(w[k], q);
    if (big) return WSNARK_DEC_MALFORMED;
    if constexpr (NE == 1) P->x = cd_load(w[0], 1, K);
    else P->x = typename F::El{cd_load(w[0], 1, K), cd_load(w[1], 1, K)};
    typename F::El y;
    if (!F::sqrt(F::add(F::mul(F::sqr(P->x), P->x), curve_b), &y)) return WSNARK_DEC_NO_POINT;
    P->y = F::is_larger(y) != sign ? F::neg(y) : y;
    if constexpr (NE == 2) {
        if (flags & WSNARK_DEC_SUBGROUP) {      // the audit's chain (pkeycheck.hip, mode 0)
            typename C::Pt a = C::infinity();
#pragma unroll 1
            for (int bit = 253; bit >= 0; bit--) {
                a = C::dbl(a);
                if ((word4(FrParams::P0, FrParams::P1, FrParams::P2, FrParams::P3, bit >> 6) >> (bit & 63)) & 1) C::madd(a, *P, false);
            }
            if (!C::is_inf(a)) return WSNARK_DEC_OUTSIDE_SUBGROUP;
        }
    }
    return 0;
}

template <int NE>
__global__ __launch_bounds__(256) void codec_compress_kernel(CodecIO io, uint64_t n, int enc, int plain, PkAcc* __restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int st = 0;
    if (i < n) {
        Fe rec[NE];
        st = codec_encode<NE>(reinterpret_cast<const Fe*>(io.in + i * io.in_stride + io.in_off), enc, plain, rec);
        Fe* o = reinterpret_cast<Fe*>(io.out + i * io.out_stride + io.out_off);
        for (int k = 0; k < NE; k++) o[k] = rec[k];
        io.status[i * io.st_stride + io.st_off] = (uint8_t)((st == 4 && !io.raw) ? 0 : st);
    }
    pk_reduce(st, i, acc);
}

template <class C, int THREADS>
__global__ __launch_bounds__(THREADS) void codec_decompress_kernel(CodecIO io, uint64_t n, int enc, uint32_t flags, int plain, CodecConsts K,
                                                                     typename C::El curve_b, PkAcc* __restrict__ acc) {
    typedef typename C::Field F;
    constexpr int NE = (int)(sizeof(typename F::Packed) / 32);
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int st = 0;
    if (i < n) {
        typename C::Aff P;
        st = codec_decode<C>(reinterpret_cast<const Fe*>(io.in + i * io.in_stride + io.in_off), enc, flags, K, curve_b, &P);
        Fe* o = reinterpret_cast<Fe*>(io.out + i * io.out_stride + io.out_off);
        if (st != 0) {
            for (int k = 0; k < 2 * NE; k++) o[k] = cd_zero();
        } else if constexpr (NE == 1) {
            o[0] = cd_store(P.x, plain);
            o[1] = cd_store(P.y, plain);
        } else {
            o[0] = cd_store(P.x.c0, plain);
            o[1] = cd_store(P.x.c1, plain);
            o[2] = cd_store(P.y.c0, plain);
            o[3] = cd_store(P.y.c1, plain);
        }
        io.status[i * io.st_stride + io.st_off] = (uint8_t)((st == 4 && !io.raw) ? 0 : st);
    }
    pk_reduce(st, i, acc);
}

// a proof's three point results (raw: 0 good, 1 .. 3, 4 infinity) -> its status, with the batch verifier's meaning: 2 malformed,
// 0 a point without y or at infinity, 1 written; z = 1 behind a good proof, a zero record behind any other
__global__ __launch_bounds__(256) void proof_decompress_finish_kernel(const uint8_t* __restrict__ st3, uint64_t n, Fe* __restrict__ proofs,
                                                                        uint8_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t a = st3[3 * i], b = st3[3 * i + 1], c = st3[3 * i + 2];
    const uint8_t st = (a == 1 || b == 1 || c == 1) ? 2 : (a | b | c) ? 0 : 1;
    Fe* o = proofs + i * 12;
    if (st != 1) {
        for (int k = 0; k < 12; k++) o[k] = cd_zero();
    } else {
        const Fe one = Fe{{1, 0, 0, 0}};
        o[2] = one; o[7] = one; o[8] = cd_zero(); o[11] = one;
    }
    status[i] = st;
}
// the other way: 2 for a proof with an unreduced word (all twelve, z included), else 1; a zero record behind a malformed proof
__global__ __launch_bounds__(256) void proof_compress_finish_kernel(const Fe* __restrict__ proofs, uint64_t n, Fe* __restrict__ out,
                                                                      uint8_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t q[4] = {FqParams::P0, FqParams::P1, FqParams::P2, FqParams::P3};
    bool big = false;
    for (int k = 0; k < 12; k++) big = big || pk_ge(proofs[i * 12 + k], q);
    if (big)
        for (int k = 0; k < 4; k++) out[i * 4 + k] = cd_zero();
    status[i] = big ? 2 : 1;
}

// ---- host ----
namespace {
bool enc_ok(int enc) { return enc == WSNARK_ENC_LE || enc == WSNARK_ENC_BE; }
int codec_consts(CodecConsts* K) {
    const PairConsts* PC = nullptr;
    if (int rc = pairing_consts(&PC)) return rc;
    K->to_int = PC->to_int;
    return WS_OK;
}
// one launch of either direction on records that are on the device
int launch_compress(Context* X, int g, const CodecIO& io, uint64_t n, int enc, int plain, PkAcc* d_acc, hipStream_t s) {
    X->timer.begin(g == 1 ? "g1_compress" : "g2_compress", s);
    if (g == 1) hipLaunchKernelGGL(codec_compress_kernel<1>, dim3(ceil_div_u64(n, 256)), dim3(256), 0, s, io, n, enc, plain, d_acc);
    else hipLaunchKernelGGL(codec_compress_kernel<2>, dim3(ceil_div_u64(n, 256)), dim3(256), 0, s, io, n, enc, plain, d_acc);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    return WS_OK;
}
int launch_decompress(Context* X, int g, const CodecIO& io, uint64_t n, int enc, uint32_t flags, int plain, PkAcc* d_acc, hipStream_t s) {
    CodecConsts K;
    G1k::El b1;
    G2k::El b2;
    int rc;
    if ((rc = codec_consts(&K)) || (rc = pk_curve_b(&b1, &b2))) return rc;
    X->timer.begin(g == 1 ? "g1_decompress" : "g2_decompress", s);
    if (g == 1)
        hipLaunchKernelGGL((codec_decompress_kernel<G1k, 256>), dim3(ceil_div_u64(n, 256)), dim3(256), 0, s, io, n, enc, flags, plain, K, b1, d_acc);
    else
        hipLaunchKernelGGL((codec_decompress_kernel<G2k, 64>), dim3(ceil_div_u64(n, 64)), dim3(64), 0, s, io, n, enc, flags, plain, K, b2, d_acc);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    return WS_OK;
}
}  // namespace

// arrays of points, host memory both ways, chunk by chunk.  compress: in = points (64 g bytes), out = records (32 g bytes)
int points_codec(int g, bool compress, const void* in, uint64_t n, int enc, uint32_t flags, void* out, uint8_t* status, uint64_t* n_bad) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (n == 0) return WS_OK;
    if (!in || !out || !status || !n_bad || !enc_ok(enc) || (flags & ~(uint32_t)WSNARK_DEC_SUBGROUP)) return WS_ERR_ARG;
    const size_t pt = (size_t)64 * g, rec = (size_t)32 * g, in_sz = compress ? pt : rec, out_sz = compress ? rec : pt;
    const uint64_t chunk = key_chunk("CODEC_CHUNK"), cap = key_chunk_cap(chunk, n);
    // (the outputs are the caller's only once every chunk has gone through: an error leaves them as they were)
    std::vector<uint8_t> h_out((size_t)n * out_sz), h_st(n);
    PkAcc h_acc;
    {
        LaneLock L = acquire_lane(X);
        hipStream_t s = L->stream;
        Slab S;
        uint8_t *d_in, *d_out, *d_st;
        PkAcc* d_acc;
        S.add(&d_in, cap * in_sz);
        S.add(&d_out, cap * out_sz);
        S.add(&d_st, cap);
        S.add(&d_acc, sizeof(PkAcc));
        WS_HIP_CHECK(S.alloc());
        WS_HIP_CHECK(hipMemsetAsync(d_acc, 0, sizeof(PkAcc), s));
        for (uint64_t lo = 0; lo < n; lo += chunk) {
            const uint64_t m = std::min<uint64_t>(chunk, n - lo);
            int rc = upload_staged(d_in, (const uint8_t*)in + lo * in_sz, (size_t)m * in_sz, s);
            if (rc) return rc;
            const CodecIO io = {d_in, in_sz, 0, d_out, out_sz, 0, d_st, 1, 0, 0};
            rc = compress ? launch_compress(X, g, io, m, enc, 0, d_acc, s) : launch_decompress(X, g, io, m, enc, flags, 0, d_acc, s);
            if (rc) return rc;
            WS_HIP_CHECK(hipMemcpyAsync(h_out.data() + lo * out_sz, d_out, (size_t)m * out_sz, hipMemcpyDeviceToHost, s));
            WS_HIP_CHECK(hipMemcpyAsync(h_st.data() + lo, d_st, m, hipMemcpyDeviceToHost, s));
            WS_HIP_CHECK(hipStreamSynchronize(s));
        }
        WS_HIP_CHECK(hipMemcpyAsync(&h_acc, d_acc, sizeof h_acc, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));
    }
    memcpy(out, h_out.data(), h_out.size());
    memcpy(status, h_st.data(), n);
    *n_bad = h_acc.bad;
    return WS_OK;
}

// count proofs on the device: d_in128 -> d_out384 (plain integers, z = 1), d_status (1 / 0 / 2); d_st3: 3 count bytes of scratch
static int proofs_decompress_dev(Context* X, const uint8_t* d_in128, uint64_t count, int enc, uint8_t* d_out384, uint8_t* d_st3, PkAcc* d_acc,
                                 uint8_t* d_status, hipStream_t s) {
    const uint64_t in_off[3] = {0, 32, 96}, out_off[3] = {0, 96, 288};
    for (int k = 0; k < 3; k++) {
        const CodecIO io = {d_in128, 128, in_off[k], d_out384, 384, out_off[k], d_st3, 3, (uint64_t)k, 1};
        // (B's subgroup membership is the verifier's test, not the codec's: a proof is not a key)
        if (int rc = launch_decompress(X, k == 1 ? 2 : 1, io, count, enc, 0, 1, d_acc, s)) return rc;
    }
    X->timer.begin("proof_decompress_finish", s);
    hipLaunchKernelGGL(proof_decompress_finish_kernel, dim3(ceil_div_u64(count, 256)), dim3(256), 0, s, (const uint8_t*)d_st3, count,
                       reinterpret_cast<Fe*>(d_out384), d_status);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    return WS_OK;
}

int proofs_codec(bool compress, const void* in, uint64_t count, int enc, void* out, uint8_t* status) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (count == 0) return WS_OK;
    if (!in || !out || !status || !enc_ok(enc)) return WS_ERR_ARG;
    const size_t in_sz = compress ? 384 : 128, out_sz = compress ? 128 : 384;
    const uint64_t chunk = key_chunk("CODEC_CHUNK"), cap = key_chunk_cap(chunk, count);
    std::vector<uint8_t> h_out((size_t)count * out_sz), h_st(count);
    LaneLock L = acquire_lane(X);
    hipStream_t s = L->stream;
    Slab S;
    uint8_t *d_in, *d_out, *d_st3, *d_st;
    PkAcc* d_acc;
    S.add(&d_in, cap * in_sz);
    S.add(&d_out, cap * out_sz);
    S.add(&d_st3, cap * 3);
    S.add(&d_st, cap);
    S.add(&d_acc, sizeof(PkAcc));
    WS_HIP_CHECK(S.alloc());
    WS_HIP_CHECK(hipMemsetAsync(d_acc, 0, sizeof(PkAcc), s));
    for (uint64_t lo = 0; lo < count; lo += chunk) {
        const uint64_t m = std::min<uint64_t>(chunk, count - lo);
        int rc = upload_staged(d_in, (const uint8_t*)in + lo * in_sz, (size_t)m * in_sz, s);
        if (rc) return rc;
        if (compress) {
            const uint64_t in_off[3] = {0, 96, 288}, out_off[3] = {0, 32, 96};
            for (int k = 0; k < 3; k++) {
                const CodecIO io = {d_in, 384, in_off[k], d_out, 128, out_off[k], d_st3, 3, (uint64_t)k, 1};
                if ((rc = launch_compress(X, k == 1 ? 2 : 1, io, m, enc, 1, d_acc, s))) return rc;
            }
            hipLaunchKernelGGL(proof_compress_finish_kernel, dim3(ceil_div_u64(m, 256)), dim3(256), 0, s, reinterpret_cast<const Fe*>(d_in), m,
                               reinterpret_cast<Fe*>(d_out), d_st);
            WS_HIP_CHECK(hipGetLastError());
        } else if ((rc = proofs_decompress_dev(X, d_in, m, enc, d_out, d_st3, d_acc, d_st, s))) {
            return rc;
        }
        WS_HIP_CHECK(hipMemcpyAsync(h_out.data() + lo * out_sz, d_out, (size_t)m * out_sz, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipMemcpyAsync(h_st.data() + lo, d_st, m, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));
    }
    memcpy(out, h_out.data(), h_out.size());
    memcpy(status, h_st.data(), count);
    return WS_OK;
}

// status[i] = what the batch verifier says about the decompressed proof i; 2 where decompression found a malformed point
int groth16_verify_batch_compressed(const uint8_t* vk, size_t vk_len, const void* inputs, uint64_t n_inputs, const void* proofs128, uint64_t count,
                                    int enc, uint8_t* status_host, bool on_device, hipStream_t stream) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (count == 0) return WS_OK;
    if (!vk || !proofs128 || !status_host || !enc_ok(enc)) return WS_ERR_ARG;
    // the batch verifier's own conditions, before any work (pairing.hip: groth16_verify_batch)
    if (vk_len < 512 || n_inputs > (vk_len - 448) / 64 - 1) { set_last_error("verification key has fewer IC points than inputs + 1"); return WS_ERR_SIZE; }
    if (count > ((uint64_t)1 << 24)) { set_last_error("verify_batch: more than 2^24 proofs in one call"); return WS_ERR_SIZE; }
    if (n_inputs && !inputs) return WS_ERR_ARG;
    Slab S;
    uint8_t *d_in128 = nullptr, *d_p384, *d_st3, *d_pre, *d_inputs = nullptr;
    PkAcc* d_acc;
    if (!on_device) {
        S.add(&d_in128, (size_t)count * 128);
        S.add(&d_inputs, (size_t)count * n_inputs * 32);
    }
    S.add(&d_p384, (size_t)count * 384);
    S.add(&d_st3, (size_t)count * 3);
    S.add(&d_pre, count);
    S.add(&d_acc, sizeof(PkAcc));
    WS_HIP_CHECK(S.alloc());
    std::vector<uint8_t> pre(count), st(count);
    {
        LaneLock L = acquire_lane(X);
        hipStream_t s = stream ? stream : L->stream;
        int rc;
        if (!on_device) {
            if ((rc = upload_staged(d_in128, proofs128, (size_t)count * 128, s))) return rc;
            if (n_inputs && (rc = upload_staged(d_inputs, inputs, (size_t)count * n_inputs * 32, s))) return rc;
        }
        WS_HIP_CHECK(hipMemsetAsync(d_acc, 0, sizeof(PkAcc), s));
        if ((rc = proofs_decompress_dev(X, on_device ? (const uint8_t*)proofs128 : d_in128, count, enc, d_p384, d_st3, d_acc, d_pre, s))) return rc;
        WS_HIP_CHECK(hipMemcpyAsync(pre.data(), d_pre, count, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));      // (the verifier takes a lane of its own: the records are complete before it starts)
    }
    const int rc = groth16_verify_batch(vk, vk_len, on_device ? inputs : (const void*)d_inputs, n_inputs, d_p384, count, st.data(), true, stream);
    if (rc) return rc;
    for (uint64_t i = 0; i < count; i++) status_host[i] = pre[i] == 2 ? 2 : st[i];
    return WS_OK;
}

}  // namespace wsnark
