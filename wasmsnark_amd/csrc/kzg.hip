// kzg.hip -- KZG commitments on a powers-of-tau transcript: commit to a polynomial, open it at a point, check the opening
// (wsnark_kzg_srs_load, wsnark_kzg_commit, wsnark_kzg_open, wsnark_kzg_verify, wsnark_fr_poly_eval, wsnark_fr_poly_divide;
// include/wsnark.h).  The sums are the resident-bases sums of fixedbase.hip, the transform of form 1 is ntt.hip's, the pairing is the
// host pairing of fp12_host.h.  What is new here is the division of a polynomial by (X - z) on the device, and the fold of several
// polynomials under a challenge.
//
// The division.  With Q[len] = 0 and Q[k] = f[k] + z Q[k + 1] -- Horner's rule from the top -- the quotient is q[k - 1] = Q[k] and
// the value is y = Q[0].  Q is a suffix scan of a linear recurrence: for any run [a, b) of coefficients,
//     Q[a] = H(a, b) + z^(b - a) Q[b],      H(a, b) = sum_{a <= k < b} f[k] z^(k - a)   (the run's own Horner value),
// so runs combine like numbers under the operator (v, m) o (v', m') = (v + m v', m m'), and with runs of EQUAL length every
// multiplier of a scan step is one power of z that the host computes once per call (KzPowers: z, z^(SEG 2^j), z^(256 SEG 2^j)).
// Three plain launches; the launches are the only synchronisation between workgroups (no flag is waited for, no grid barrier):
//   kz_tile_kernel      a workgroup takes a tile of 256 SEG consecutive coefficients (zeros behind the polynomial's end), lane l
//                       the SEG coefficients [l SEG, (l + 1) SEG) of it: its Horner value, then the scan of the 256 values with
//                       multiplier z^SEG (kz_suffix_scan): lane l holds Q at the start of its run as if nothing followed the
//                       tile.  These 256 values are stored (the division only: 32 / SEG bytes per coefficient); lane 0's is the
//                       tile's value H(tile).
//   kz_carry_kernel     ONE workgroup per polynomial scans the tile values with multiplier z^(256 SEG): lane l takes G = ceil(tiles
//                       / 256) consecutive tile values -- a Horner pass of its own, so the second launch stays one workgroup
//                       however long the polynomial --, the 256 group values are scanned with multiplier z^(256 SEG G), and the
//                       lane replays its group: the carry Q[end of tile] that enters each tile, and y.  It also writes the 256
//                       powers (z^SEG)^(l + 1) the third launch needs (lane l multiplies the z^(SEG 2^j) of the set bits of l + 1).
//   kz_quotient_kernel  the tile again: lane l takes Q at the end of its run from its neighbour's stored value and the tile's
//                       carry, Q[end of run l] = I[l + 1] + (z^SEG)^(255 - l) carry -- one product, no second scan --, replays
//                       its run from there, q stored.
// Global loads and stores are coalesced: a tile passes through LDS (element e of the tile at slot e + e / SEG: the run of a lane
// starts (SEG + 1) slots after its neighbour's), lane l of a wavefront loads and stores elements 256 i + l.  (The second launch's
// lanes stride through the tile values by G elements: one value per 256 SEG coefficients.)
// Products per coefficient: 1 + 8 / SEG in the first launch (the scan's eight steps per lane are shared by SEG coefficients),
// 1 + 1 / SEG in the third; bytes: 32 + 32 / SEG, then 64 + 32 / SEG.  All values are PLAIN: z and its powers are in Montgomery form,
// so that the Montgomery product of a power and a plain value is the plain product -- no conversion pass on either side.
// SEG: KZG_SEG, default 4, within [1, 6] (LDS: 256 (SEG + 2) x 32 B, 48 KiB at 4); no result depends on it.
// wsnark_fr_poly_eval is the first two launches with the polynomial's index as the grid's second dimension.
//
// The fold.  F[k] = sum_i gamma^i f_i[k]: one lane per coefficient, Horner over i from the last polynomial down, neighbouring
// lanes read neighbouring coefficients of the same polynomial.
#include <string.h>

#include <memory>

#include "keybytes.h"

namespace wsnark {

using namespace hostpair;

// ---- device ----
constexpr uint32_t KZ_LANES = 256;
constexpr long KZ_SEG_DEFAULT = 4, KZ_SEG_MAX = 6;

struct KzPowers {      // Montgomery form
    Fe z;
    Fe lane[8];        // z^(SEG 2^j): the scan over a tile's 256 runs
    Fe tile;           // z^(256 SEG): one tile value to the next
    Fe group[8];       // z^(256 SEG G 2^j): the scan over the 256 groups of G tile values
};

// I[l] = sum_{j >= l} v[j] m^(j - l) over the workgroup's 256 lanes, pw[s] = m^(2^s); buf: 256 elements of LDS, which hold I when
// the function returns (every lane arrives; the caller synchronises before it writes buf again)
__device__ __forceinline__ Fe kz_suffix_scan(Fe v, const Fe* __restrict__ pw, Fe* buf) {
    const unsigned l = threadIdx.x;
    buf[l] = v;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const unsigned d = 1u << s;
        if (l + d < KZ_LANES) v = Fr::add(v, Fr::mul(pw[s], buf[l + d]));
        __syncthreads();
        buf[l] = v;
        __syncthreads();
    }
    return v;
}

// the tile [base, base + 256 seg) of f into LDS, reduced mod r, zeros from len on; lane l loads elements 256 i + l
__device__ __forceinline__ void kz_load_tile(const Fe* __restrict__ f, uint64_t len, uint64_t base, uint32_t seg, Fe* tile) {
    for (uint32_t i = 0; i < seg; i++) {
        const uint32_t e = i * KZ_LANES + threadIdx.x;
        const uint64_t k = base + e;
        tile[e + e / seg] = k < len ? Fr::reduce_full(f[k]) : Fe{{0, 0, 0, 0}};
    }
    __syncthreads();
}
// H of the lane's run: its seg coefficients from the top
__device__ __forceinline__ Fe kz_run_value(const Fe* tile, uint32_t seg, const Fe& z) {
    const Fe* run = tile + threadIdx.x * (seg + 1);
    Fe acc = run[seg - 1];
    for (uint32_t j = seg - 1; j-- > 0;) acc = Fr::add(run[j], Fr::mul(z, acc));
    return acc;
}

// tilevals[poly][tile] = H(tile); runvals (may be null; one polynomial): the scan's 256 values of every tile; grid (tiles,
// polynomials); dynamic LDS: 256 (seg + 2) elements
__global__ __launch_bounds__(256) void kz_tile_kernel(const Fe* __restrict__ polys, uint64_t len, uint32_t seg, KzPowers W, Fe* __restrict__ tilevals,
                                                       Fe* __restrict__ runvals) {
    WS_DYN_SMEM(Fe, sm);
    Fe* tile = sm + KZ_LANES;
    kz_load_tile(polys + (uint64_t)blockIdx.y * len, len, (uint64_t)blockIdx.x * KZ_LANES * seg, seg, tile);
    const Fe v = kz_suffix_scan(kz_run_value(tile, seg, W.z), W.lane, sm);
    if (runvals) runvals[(uint64_t)blockIdx.x * KZ_LANES + threadIdx.x] = v;
    if (threadIdx.x == 0) tilevals[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = v;
}

// carries[t] = Q[end of tile t] (carries may be null: the value alone), ys[poly] = Q[0], lanepow[l] = (z^SEG)^(l + 1) (may be null);
// one workgroup per polynomial, lane l the tile values [l G, (l + 1) G)
__global__ __launch_bounds__(256) void kz_carry_kernel(const Fe* __restrict__ tilevals, uint32_t ntiles, uint32_t G, KzPowers W, Fe* __restrict__ carries,
                                                        Fe* __restrict__ ys, Fe* __restrict__ lanepow) {
    __shared__ Fe buf[KZ_LANES];
    const Fe* V = tilevals + (uint64_t)blockIdx.x * ntiles;
    const unsigned l = threadIdx.x;
    const uint32_t lo = l * G;
    Fe acc = Fe{{0, 0, 0, 0}};
    for (uint32_t j = G; j-- > 0;) {
        const uint32_t t = lo + j;
        acc = Fr::add(t < ntiles ? V[t] : Fe{{0, 0, 0, 0}}, Fr::mul(W.tile, acc));
    }
    acc = kz_suffix_scan(acc, W.group, buf);
    if (l == 0) ys[blockIdx.x] = acc;
    if (carries) {
        acc = l == KZ_LANES - 1 ? Fe{{0, 0, 0, 0}} : buf[l + 1];      // Q at the end of the lane's group
        for (uint32_t j = G; j-- > 0;) {
            const uint32_t t = lo + j;
            if (t < ntiles) {
                carries[t] = acc;
                acc = Fr::add(V[t], Fr::mul(W.tile, acc));
            }
        }
    }
    if (lanepow && blockIdx.x == 0) {
        const unsigned m = l + 1;
        Fe p = W.tile;                                                // m == 256
        bool started = false;
#pragma unroll
        for (int j = 0; j < 8; j++)
            if ((m >> j) & 1) { p = started ? Fr::mul(p, W.lane[j]) : W.lane[j]; started = true; }
        lanepow[l] = p;
    }
}

// q[k - 1] = Q[k], 1 <= k < len, for the tile's k; runvals: kz_tile_kernel's, carries and lanepow: kz_carry_kernel's; dynamic LDS:
// 256 (seg + 1) elements
__global__ __launch_bounds__(256) void kz_quotient_kernel(const Fe* __restrict__ f, uint64_t len, uint32_t seg, KzPowers W, const Fe* __restrict__ runvals,
                                                           const Fe* __restrict__ carries, const Fe* __restrict__ lanepow, Fe* __restrict__ q) {
    WS_DYN_SMEM(Fe, tile);
    const unsigned l = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * KZ_LANES * seg;
    kz_load_tile(f, len, base, seg, tile);
    // Q at the end of the lane's run: the 255 - l runs above it in the tile, then the tile's carry behind (z^SEG)^(255 - l)
    Fe acc = carries[blockIdx.x];
    if (l < KZ_LANES - 1) acc = Fr::add(runvals[(uint64_t)blockIdx.x * KZ_LANES + l + 1], Fr::mul(lanepow[KZ_LANES - 2 - l], acc));
    Fe* run = tile + l * (seg + 1);
    for (uint32_t j = seg; j-- > 0;) {
        acc = Fr::add(run[j], Fr::mul(W.z, acc));
        run[j] = acc;
    }
    __syncthreads();
    for (uint32_t i = 0; i < seg; i++) {
        const uint32_t e = i * KZ_LANES + l;
        const uint64_t k = base + e;
        if (k >= 1 && k < len) q[k - 1] = tile[e + e / seg];
    }
}

// out[k] = sum_i gamma^i polys[i][k], reduced
__global__ __launch_bounds__(256) void kz_fold_kernel(const Fe* __restrict__ polys, uint64_t len, uint64_t count, Fe gamma, Fe* __restrict__ out) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= len) return;
    Fe acc = Fr::reduce_full(polys[(count - 1) * len + k]);
    for (uint64_t i = count - 1; i-- > 0;) acc = Fr::add(Fr::reduce_full(polys[i * len + k]), Fr::mul(gamma, acc));
    out[k] = acc;
}

// ---- host ----
struct KzgSrs {
    Context* owner = nullptr;
    uint64_t n = 0;
    ResidentPoints* pts = nullptr;
    ~KzgSrs() { if (pts) points_free(pts); }
};
Context* kzg_context(const KzgSrs* S) { return S ? S->owner : nullptr; }
void kzg_srs_free(KzgSrs* S) { delete S; }
void kzg_srs_info(const KzgSrs* S, uint64_t* n, uint64_t* bytes) {
    if (n) *n = S->n;
    if (bytes) points_info(S->pts, nullptr, nullptr, nullptr, nullptr, bytes);
}

namespace {
constexpr uint64_t KZ_MAX_LEN = (uint64_t)1 << 24;

uint32_t kz_seg() { return (uint32_t)std::min<long>(std::max<long>(tuning_get("KZG_SEG", KZ_SEG_DEFAULT), 1), KZ_SEG_MAX); }
uint32_t kz_tiles(uint64_t len, uint32_t seg) { return ceil_div_u64(len, (uint64_t)KZ_LANES * seg); }
size_t kz_lds(uint32_t seg) { return (size_t)KZ_LANES * (seg + 2) * sizeof(Fe); }

// tile values per lane of the second launch
uint32_t kz_group(uint32_t tiles) { return (tiles + KZ_LANES - 1) / KZ_LANES; }
KzPowers kz_powers(const Fe& z, uint32_t seg, uint64_t len) {
    KzPowers W;
    W.z = Fr::to_mont(z);
    W.lane[0] = Fr::pow_u64(W.z, seg);
    for (int j = 1; j < 8; j++) W.lane[j] = Fr::sqr(W.lane[j - 1]);
    W.tile = Fr::sqr(W.lane[7]);
    W.group[0] = Fr::pow_u64(W.tile, kz_group(kz_tiles(len, seg)));
    for (int j = 1; j < 8; j++) W.group[j] = Fr::sqr(W.group[j - 1]);
    return W;
}

// the lane's scratch of one call, pieces of L.kzg_ws
struct KzWs {
    Fe *F = nullptr, *q = nullptr, *tilevals = nullptr, *carries = nullptr, *ys = nullptr, *runvals = nullptr, *lanepow = nullptr;
    // ncar: the tiles of a division (0: none): its carries, its 256 scan values per tile, the 256 lane powers
    int carve(Lane& L, uint64_t nF, uint64_t nq, uint64_t ntv, uint64_t ncar, uint64_t nys) {
        const uint64_t want[7] = {nF, nq, ntv, ncar, nys, ncar * KZ_LANES, ncar ? KZ_LANES : 0};
        Fe** at[7] = {&F, &q, &tilevals, &carries, &ys, &runvals, &lanepow};
        size_t total = 0;
        for (uint64_t w : want) total += Slab::up256((size_t)std::max<uint64_t>(w, 1) * sizeof(Fe));
        WS_HIP_CHECK(L.kzg_ws.reserve(total));
        size_t off = 0;
        for (int i = 0; i < 7; i++) {
            *at[i] = reinterpret_cast<Fe*>(L.kzg_ws.as<uint8_t>() + off);
            off += Slab::up256((size_t)std::max<uint64_t>(want[i], 1) * sizeof(Fe));
        }
        return WS_OK;
    }
};

// d_ys[i] = f_i(z) for count polynomials stored back to back; d_tilevals: count x tiles elements
int kz_eval_dev(Context* X, const Fe* d_polys, uint64_t len, uint64_t count, const KzPowers& W, uint32_t seg, Fe* d_tilevals, Fe* d_ys, hipStream_t s) {
    const uint32_t tiles = kz_tiles(len, seg);
    X->timer.begin("kzg_tile", s);
    hipLaunchKernelGGL(kz_tile_kernel, dim3(tiles, (uint32_t)count), dim3(KZ_LANES), kz_lds(seg), s, d_polys, len, seg, W, d_tilevals, (Fe*)nullptr);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    X->timer.begin("kzg_carry", s);
    hipLaunchKernelGGL(kz_carry_kernel, dim3((uint32_t)count), dim3(KZ_LANES), 0, s, d_tilevals, tiles, kz_group(tiles), W, (Fe*)nullptr, d_ys, (Fe*)nullptr);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    return WS_OK;
}
// the three launches: d_q[0 .. len - 1) and d_y[0]; d_q must not overlap d_f; ws: carved for this division's tiles
int kz_divide_dev(Context* X, const Fe* d_f, uint64_t len, const KzPowers& W, uint32_t seg, const KzWs& ws, Fe* d_y, Fe* d_q, hipStream_t s) {
    const uint32_t tiles = kz_tiles(len, seg);
    X->timer.begin("kzg_tile", s);
    hipLaunchKernelGGL(kz_tile_kernel, dim3(tiles, 1), dim3(KZ_LANES), kz_lds(seg), s, d_f, len, seg, W, ws.tilevals, len > 1 ? ws.runvals : (Fe*)nullptr);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    X->timer.begin("kzg_carry", s);
    hipLaunchKernelGGL(kz_carry_kernel, dim3(1), dim3(KZ_LANES), 0, s, ws.tilevals, tiles, kz_group(tiles), W, ws.carries, d_y, ws.lanepow);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    if (len > 1) {
        X->timer.begin("kzg_quotient", s);
        hipLaunchKernelGGL(kz_quotient_kernel, dim3(tiles), dim3(KZ_LANES), kz_lds(seg) - KZ_LANES * sizeof(Fe), s, d_f, len, seg, W, ws.runvals, ws.carries,
                           ws.lanepow, d_q);
        WS_HIP_CHECK(hipGetLastError());
        X->timer.end(s);
    }
    return WS_OK;
}

// The sum over the first len powers, len < n: over the prefix of the points by a per-window plan, or -- the scalars padded with
// zeros -- over the whole set through its window tables.  KZG_PAD_PCT: the padded sum from len >= pct / 100 of n on (0: always,
// above 100: never).  The default is the measured crossover at n = 2^20 (tools/kzg_bench.py, profiles/kzg_bench.json): the padded
// sum wins at n / 2 (1.29 against 1.55 ms), the prefix sum at n / 4 and below (1.00 against 1.23 ms).  The group element, and so the
// bytes, are the same.
bool kz_pad(uint64_t len, uint64_t n) {
    const long pct = std::min<long>(std::max<long>(tuning_get("KZG_PAD_PCT", 50), 0), 101);
    return len * 100 >= (uint64_t)pct * n;
}
// out64 = sum_k d_coef[k] tau_g1[k], k < len; d_pad: n elements of scratch that d_coef is not part of
int kz_commit_one(Lane& L, KzgSrs* S, const Fe* d_coef, uint64_t len, Fe* d_pad, uint8_t* out64, hipStream_t s) {
    Jac<Fq> j;
    int rc;
    if (len < S->n && kz_pad(len, S->n)) {
        WS_HIP_CHECK(hipMemcpyAsync(d_pad, d_coef, (size_t)len * sizeof(Fe), hipMemcpyDeviceToDevice, s));
        WS_HIP_CHECK(hipMemsetAsync(d_pad + len, 0, (size_t)(S->n - len) * sizeof(Fe), s));
        rc = points_msm_lane(L, S->pts, d_pad, S->n, &j, s);
    } else {
        rc = points_msm_lane(L, S->pts, d_coef, len, &j, s);
    }
    if (rc) return rc;
    if (Fq::is_zero(j.z)) memset(out64, 0, 64);
    else memcpy(out64, &j, 64);
    return WS_OK;
}

int kz_len_check(const char* who, uint64_t len, uint64_t n, uint64_t count) {
    if (len == 0 || len > KZ_MAX_LEN || len > n) {
        set_last_error(std::string(who) + ": len must be in [1, min(n, 2^24)]");
        return WS_ERR_SIZE;
    }
    if (count > 65535 || count > ((uint64_t)1 << 28) / len) {      // (the polynomial's index is the grid's second dimension)
        set_last_error(std::string(who) + ": count > 65535 or count x len > 2^28");
        return WS_ERR_SIZE;
    }
    return WS_OK;
}
// the caller's polynomials on the device: as they are, or staged into the lane's input buffer
int kz_inputs(Lane& L, const void* polys, uint64_t elems, bool on_device, hipStream_t s, const Fe** out) {
    *out = (const Fe*)polys;
    if (on_device) return WS_OK;
    WS_HIP_CHECK(L.host_in[0].reserve((size_t)elems * sizeof(Fe)));
    *out = L.host_in[0].as<Fe>();
    return upload_staged(L.host_in[0].p, polys, (size_t)elems * sizeof(Fe), s);
}
}  // namespace

int kzg_srs_load(const void* tau_g1, uint64_t n, KzgSrs** out) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (!tau_g1 || !out) return WS_ERR_ARG;
    if (n == 0 || n > KZ_MAX_LEN) { set_last_error("kzg_srs_load: n must be in [1, 2^24]"); return WS_ERR_SIZE; }
    // the audit's two cheap tests on every power: reduced coordinates, on the curve (G1 has cofactor 1); no infinity
    PkAcc h_acc;
    memset(&h_acc, 0, sizeof h_acc);
    {
        int rc;
        const uint64_t chunk = key_chunk("PWTAU_CHUNK");
        LaneLock L = acquire_lane(X);
        hipStream_t s = L->stream;
        DevBuf d_pts, d_acc;
        WS_HIP_CHECK(d_pts.alloc((size_t)key_chunk_cap(chunk, n) * 64));
        WS_HIP_CHECK(d_acc.alloc(sizeof h_acc));
        WS_HIP_CHECK(hipMemsetAsync(d_acc.p, 0, sizeof h_acc, s));
        for (uint64_t lo = 0; lo < n; lo += chunk) {
            const uint64_t m = std::min<uint64_t>(chunk, n - lo);
            if ((rc = stage_chunk(d_pts.p, (const uint8_t*)tau_g1 + lo * 64, (size_t)m * 64, s, nullptr))) return rc;
            if ((rc = pkcheck_g1_dev(X, d_pts.p, m, lo, d_acc.as<PkAcc>(), s))) return rc;
            WS_HIP_CHECK(hipStreamSynchronize(s));      // (the chunk buffer is written again)
        }
        WS_HIP_CHECK(hipMemcpyAsync(&h_acc, d_acc.p, sizeof h_acc, hipMemcpyDeviceToHost, s));
        WS_HIP_CHECK(hipStreamSynchronize(s));
    }
    uint64_t inf, bad, first;
    uint32_t reason;
    pk_decode(h_acc, &inf, &bad, &first, &reason);
    if (inf) {      // (the counters index bad points only: the first infinity is found here, x == 0)
        static const uint8_t zero[32] = {0};
        for (uint64_t i = 0; i < n && i < first; i++)
            if (!memcmp((const uint8_t*)tau_g1 + i * 64, zero, 32)) { first = i; reason = WSNARK_PK_INFINITY; break; }
    }
    if (bad || inf) {
        const char* why = reason == WSNARK_PK_INFINITY ? "at infinity" : reason == WSNARK_PK_UNREDUCED ? "unreduced" : "off the curve";
        set_last_error("kzg_srs_load: " + std::to_string(bad + inf) + " bad power(s), the first at index " + std::to_string(first) + " (" + why + ")");
        return WS_ERR_FORMAT;
    }
    std::unique_ptr<KzgSrs> S(new KzgSrs());
    S->owner = X;
    S->n = n;
    const int rc = points_load(0, tau_g1, n, &S->pts);
    if (rc) return rc;
    *out = S.release();
    return WS_OK;
}

int fr_poly_eval(const void* polys, uint64_t len, uint64_t count, const uint8_t* z32, void* out_y) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (count == 0) return WS_OK;
    if (!polys || !z32 || !out_y) return WS_ERR_ARG;
    int rc;
    if ((rc = kz_len_check("fr_poly_eval", len, KZ_MAX_LEN, count))) return rc;
    const uint32_t seg = kz_seg();
    const KzPowers W = kz_powers(load_scalar(z32), seg, len);
    LaneLock L = acquire_lane(X);
    hipStream_t s = L->stream;
    const Fe* d_polys;
    KzWs ws;
    if ((rc = kz_inputs(*L, polys, count * len, false, s, &d_polys))) return rc;
    if ((rc = ws.carve(*L, 0, 0, count * kz_tiles(len, seg), 0, count))) return rc;
    if ((rc = kz_eval_dev(X, d_polys, len, count, W, seg, ws.tilevals, ws.ys, s))) return rc;
    std::vector<Fe> ys(count);
    WS_HIP_CHECK(hipMemcpyAsync(ys.data(), ws.ys, (size_t)count * sizeof(Fe), hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    memcpy(out_y, ys.data(), (size_t)count * sizeof(Fe));
    return WS_OK;
}

int fr_poly_divide(const void* poly, uint64_t len, const uint8_t* z32, void* q, void* out_y32, bool on_device, hipStream_t s) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (!poly || !z32 || !out_y32 || (len > 1 && !q)) return WS_ERR_ARG;
    int rc;
    if ((rc = kz_len_check("fr_poly_divide", len, KZ_MAX_LEN, 1))) return rc;
    const uint32_t seg = kz_seg(), tiles = kz_tiles(len, seg);
    const KzPowers W = kz_powers(load_scalar(z32), seg, len);
    LaneLock L = acquire_lane(X);
    if (!s) s = L->stream;
    const Fe* d_f;
    KzWs ws;
    if ((rc = kz_inputs(*L, poly, len, on_device, s, &d_f))) return rc;
    if ((rc = ws.carve(*L, 0, on_device ? 0 : len, tiles, tiles, 1))) return rc;
    Fe* d_q = on_device ? (Fe*)q : ws.q;
    if ((rc = kz_divide_dev(X, d_f, len, W, seg, ws, ws.ys, d_q, s))) return rc;
    Fe y;
    WS_HIP_CHECK(hipMemcpyAsync(&y, ws.ys, sizeof y, hipMemcpyDeviceToHost, s));
    if (!on_device && len > 1) WS_HIP_CHECK(hipMemcpyAsync(q, d_q, (size_t)(len - 1) * sizeof(Fe), hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    memcpy(out_y32, &y, sizeof y);
    return WS_OK;
}

int kzg_commit(KzgSrs* S, const void* polys, uint64_t len, uint64_t count, int form, bool on_device, void* out_commitments, hipStream_t s) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (!S) return WS_ERR_ARG;
    if (count == 0) return WS_OK;
    if (!polys || !out_commitments || (form != 0 && form != 1)) return WS_ERR_ARG;
    int rc;
    if ((rc = kz_len_check("kzg_commit", len, S->n, count))) return rc;
    if (form == 1 && (len & (len - 1))) { set_last_error("kzg_commit: evaluation form needs a power-of-two len"); return WS_ERR_SIZE; }
    LaneLock L = acquire_lane(X);
    if (!s) s = L->stream;
    const Fe* d_polys;
    KzWs ws;
    if ((rc = kz_inputs(*L, polys, count * len, on_device, s, &d_polys))) return rc;
    if ((rc = ws.carve(*L, form == 1 ? len : 0, S->n, 0, 0, 0))) return rc;
    std::vector<uint8_t> held((size_t)count * 64);
    for (uint64_t i = 0; i < count; i++) {
        const Fe* d_coef = d_polys + i * len;
        if (form == 1) {      // evaluations on the domain of wsnark_fr_ntt: the inverse transform works on Montgomery form
            if ((rc = fr_map_dev(d_coef, ws.F, len, 1, s))) return rc;
            if (len > 1 && (rc = ntt_dev(*L, ws.F, len, 0, 1, s))) return rc;
            if ((rc = fr_map_dev(ws.F, ws.F, len, 0, s))) return rc;
            d_coef = ws.F;
        }
        if ((rc = kz_commit_one(*L, S, d_coef, len, ws.q, held.data() + i * 64, s))) return rc;
    }
    memcpy(out_commitments, held.data(), held.size());
    return WS_OK;
}

int kzg_open(KzgSrs* S, const void* polys, uint64_t len, uint64_t count, const uint8_t* z32, const uint8_t* gamma32, bool on_device, void* out_y,
             void* out_proof64, hipStream_t s) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (!S) return WS_ERR_ARG;
    if (count == 0) return WS_OK;
    if (!polys || !z32 || !out_y || !out_proof64 || (count > 1 && !gamma32)) return WS_ERR_ARG;
    int rc;
    if ((rc = kz_len_check("kzg_open", len, S->n, count))) return rc;
    const uint32_t seg = kz_seg(), tiles = kz_tiles(len, seg);
    const KzPowers W = kz_powers(load_scalar(z32), seg, len);
    LaneLock L = acquire_lane(X);
    if (!s) s = L->stream;
    const Fe* d_polys;
    KzWs ws;
    if ((rc = kz_inputs(*L, polys, count * len, on_device, s, &d_polys))) return rc;
    // F: the fold, then (the division has read it) the padded quotient; ys: the count values, then the fold's own
    if ((rc = ws.carve(*L, std::max(len, S->n), len, count * tiles, tiles, count + 1))) return rc;
    const Fe* d_F = d_polys;
    if (count > 1) {
        if ((rc = kz_eval_dev(X, d_polys, len, count, W, seg, ws.tilevals, ws.ys, s))) return rc;
        X->timer.begin("kzg_fold", s);
        hipLaunchKernelGGL(kz_fold_kernel, dim3(ceil_div_u64(len, KZ_LANES)), dim3(KZ_LANES), 0, s, d_polys, len, count, Fr::to_mont(load_scalar(gamma32)), ws.F);
        WS_HIP_CHECK(hipGetLastError());
        X->timer.end(s);
        d_F = ws.F;
    }
    // (one polynomial: the division's y is the value asked for)
    if ((rc = kz_divide_dev(X, d_F, len, W, seg, ws, count > 1 ? ws.ys + count : ws.ys, ws.q, s))) return rc;
    std::vector<Fe> ys(count);
    WS_HIP_CHECK(hipMemcpyAsync(ys.data(), ws.ys, (size_t)count * sizeof(Fe), hipMemcpyDeviceToHost, s));
    uint8_t proof[64];
    memset(proof, 0, sizeof proof);      // (a constant polynomial: the quotient is zero, the proof infinity)
    if (len > 1 && (rc = kz_commit_one(*L, S, ws.q, len - 1, ws.F, proof, s))) return rc;
    WS_HIP_CHECK(hipStreamSynchronize(s));
    memcpy(out_y, ys.data(), (size_t)count * sizeof(Fe));
    memcpy(out_proof64, proof, sizeof proof);
    return WS_OK;
}

// ---- the check, on the host ----
namespace {
// one G1 input: WS_ERR_FORMAT for an unreduced coordinate; *ok cleared for a point off the curve, or at infinity where that is not legal
int kz_g1_in(const uint8_t* p, bool inf_legal, G1A* out, bool* ok) {
    const uint32_t why = fixed_g1(p, true, out);
    if (why == WSNARK_PK_UNREDUCED) { set_last_error("kzg_verify: an unreduced coordinate"); return WS_ERR_FORMAT; }
    if (why == WSNARK_PK_INFINITY ? !inf_legal : why != 0) *ok = false;
    return WS_OK;
}
int kz_g2_in(const uint8_t* p, G2A* out, bool* ok) {
    const uint32_t why = fixed_g2(p, true, out);
    if (why == WSNARK_PK_UNREDUCED) { set_last_error("kzg_verify: an unreduced coordinate"); return WS_ERR_FORMAT; }
    if (why) *ok = false;
    return WS_OK;
}
G1::Pt kz_pt(const G1A& a) { return a.inf ? G1::infinity() : G1::Pt{a.x, a.y, Fq::one(), Fq::one()}; }
G1::Pt kz_mul(const G1::Pt& p, const Fe& k) { return G1::mul_bytes(p, reinterpret_cast<const uint8_t*>(&k), 32); }
}  // namespace

int kzg_verify(const uint8_t* g1_64, const uint8_t* g2_pair256, const uint8_t* commitments, uint64_t count, const uint8_t* z32,
               const uint8_t* gamma32, const uint8_t* ys, const uint8_t* proof64, int* valid) {
    if (count == 0) return WS_OK;
    if (!g1_64 || !g2_pair256 || !commitments || !z32 || !ys || !proof64 || !valid || (count > 1 && !gamma32)) return WS_ERR_ARG;
    int rc;
    bool ok = true;
    G1A g1, pi;
    G2A g2, tau2;
    if ((rc = kz_g1_in(g1_64, false, &g1, &ok)) || (rc = kz_g1_in(proof64, true, &pi, &ok)) || (rc = kz_g2_in(g2_pair256, &g2, &ok)) ||
        (rc = kz_g2_in(g2_pair256 + 128, &tau2, &ok)))
        return rc;
    std::vector<G1A> Cs(count);
    for (uint64_t i = 0; i < count; i++)
        if ((rc = kz_g1_in(commitments + i * 64, true, &Cs[i], &ok))) return rc;
    if (!ok) { *valid = 0; return WS_OK; }
    // C = sum gamma^i C_i and y = sum gamma^i y_i, Horner from the last pair down
    const Fe gamma = count > 1 ? load_scalar(gamma32) : Fe{{0, 0, 0, 0}}, gamma_m = Fr::to_mont(gamma);
    G1::Pt C = kz_pt(Cs[count - 1]);
    Fe y = load_scalar(ys + (count - 1) * 32);
    for (uint64_t i = count - 1; i-- > 0;) {
        C = G1::add(kz_mul(C, gamma), kz_pt(Cs[i]));
        y = Fr::add(load_scalar(ys + i * 32), Fr::mul(gamma_m, y));
    }
    // e(C - y g1 + z pi, g2) == e(pi, tau g2)
    const G1::Pt lhs = G1::add(G1::add(C, G1::neg(kz_mul(kz_pt(g1), y))), kz_mul(kz_pt(pi), load_scalar(z32)));
    const Jac<Fq> j = G1::to_affine_jac(lhs);
    *valid = same_pairing(G1A{j.x, j.y, Fq::is_zero(j.z)}, g2, pi, tau2) ? 1 : 0;
    return WS_OK;
}

}  // namespace wsnark
