// pairing.hip -- batch Groth16 verification on the device (wsnark_groth16_verify_batch, include/wsnark.h).
//
// Same check and same verdicts, proof by proof, as the host verifier (verify.hip; its header has the pairing and why any bilinear
// non-degenerate pairing gives the same verdict):
//     e(A, B) * e(-IC(x), gamma2) * e(-C, delta2) * e(-alfa1, beta2) == 1
// with the plain ate pairing f_{T,Q}(P)^((p^12-1)/r), T = p - r, on Fp12 = Fq2[w]/(w^6 - xi) (fp12.h).
//
// Per CALL, on the host, with the host verifier's own code (fp12_host.h): the key's range / curve / subgroup checks; the line
// coefficients (lambda', lambda' x_T' - y_T') of every Miller step of gamma2 and of delta2 -- the key fixes them, so per proof their
// lines cost "evaluate at P, multiply into f" with no slope --; and the Miller value of (-alfa1, beta2), one Fp12 constant.
// Per PROOF, one lane, three kernels:
//   verify_prepare   range checks of the proof's twelve numbers (status 2) and of the inputs (>= r: status 0), curve equations of
//                    A, B, C, [r] B == O, IC(x) = IC[0] + sum x_i IC[i+1] as ONE double-and-add chain over the bits of all inputs
//                    (254 doublings + a mixed addition per set bit instead of a chain per input), its affine form
//   verify_miller    ONE accumulator f for the three proof-dependent pairings: per bit of T one squaring of f, the line of B's
//                    doubling (B's multiples in Jacobian coordinates: the line is scaled by an element of Fq2, which the final
//                    exponentiation kills -- no inversion anywhere in the loop) and the two stored lines; then f * m(-alfa1, beta2)
//   verify_finalexp  f^((p^6-1)(p^2+1)) by one inversion, one conjugation and one p^2-Frobenius, then the hard part through the
//                    curve's parameter x on cyclotomic squarings (fp12.h: f12d_hard_bn), and the comparison with 1
//                    (WSNARK_VERIFY_PLAIN_EXP=1: the host's 2790-bit exponent instead, the cross-check; =2: the hard part by
//                    square-and-multiply over its 761 bits)
// A lane whose status is decided in the first kernel leaves the later ones at once; lanes never exchange anything, so a proof's
// result depends on no neighbour.  An Fp12 value lives in the lane's private memory (fp12.h says why).
#include <string.h>

#include <vector>

#include "../../include/wsnark.h"
#include "internal.h"
#include "fp12.h"
#include "fp12_host.h"

namespace wsnark {

using namespace hostpair;

static const uint8_t kPending = 255;      // status of a proof that is still to be paired (device-internal)

// ---- host: constants ----
static Fe pk_internal(const Fe& mont) { return Fq29::pack(Fq29::canonical(Fq29::to_internal(mont))); }   // reference format -> internal, stored
struct PairConstsHost {
    PairConsts K;
    int rc = WS_OK;
    PairConstsHost() {
        const Fe one = Fq::one(), nine = Fq::to_mont(Fe{{9, 0, 0, 0}});
        const F2 xi = F2{nine, one};
        const F2 g1 = f2_pow(xi, kExpXiSixth, kExpXiSixthBits);                  // xi^((p^2-1)/6): in Fq
        // self-check: w^(p^2), by exponentiation in the host Fp12, is gamma w
        F12 w = f12_one();
        w.c[0] = Fq2::zero();
        w.c[1] = Fq2::one();
        const F12 wp = f12_pow(w, kExpP2, kExpP2Bits);
        bool ok = Fq::is_zero(g1.c1) && Fq2::eq(wp.c[1], g1);
        for (int i = 0; i < 6; i++) ok = ok && (i == 1 || Fq2::is_zero(wp.c[i]));
        if (!ok) { rc = WS_ERR_FORMAT; return; }
        Fe g = g1.c0;
        for (int k = 0; k < 5; k++) { K.gamma[k] = Fq29::to_internal(g); g = Fq::mul(g, g1.c0); }
        K.to_int = Fq29::unpack(Fq::to_mont(Fq::to_mont(Fe{{1024, 0, 0, 0}})));   // 2^10 2^512 mod p, read as a plain integer
        const F2 b2 = Fq2::mul(F2{Fq::to_mont(Fe{{3, 0, 0, 0}}), Fq::zero()}, Fq2::inv(xi));      // the twist's 3 / xi
        K.b2[0] = Fq29::to_internal(b2.c0);
        K.b2[1] = Fq29::to_internal(b2.c1);
        for (int i = 0; i < kExpHardWords; i++) K.hard[i] = kExpHard[i];
        for (int i = 0; i < 44; i++) K.plain[i] = kFinalExp[i];
        const Fe q = Fq::modulus(), r = Fr::modulus();
        for (int i = 0; i < 4; i++) { K.q[i] = q.l[i]; K.r[i] = r.l[i]; }
        K.ate[0] = kAteLoop[0];
        K.ate[1] = kAteLoop[1];
        // the p-Frobenius: gamma_1 = xi^((p-1)/6) in Fq2; self-check w^p == gamma_1 w by exponentiation
        const F2 h1 = f2_pow(xi, kExpXiSixthP, kExpXiSixthPBits);
        const F12 wq = f12_pow(w, q.l, 254);
        ok = Fq2::eq(wq.c[1], h1);
        for (int i = 0; i < 6; i++) ok = ok && (i == 1 || Fq2::is_zero(wq.c[i]));
        if (!ok) { rc = WS_ERR_FORMAT; return; }
        F2 h = h1;
        for (int k = 0; k < 5; k++) { K.gamma1[k][0] = Fq29::to_internal(h.c0); K.gamma1[k][1] = Fq29::to_internal(h.c1); h = Fq2::mul(h, h1); }
        K.bn_x = kBnX[0];
    }
};
int pairing_consts(const PairConsts** out) {
    static const PairConstsHost H;        // (immutable after its thread-safe construction)
    if (H.rc) { set_last_error("pairing: the Frobenius self-check (w^p, w^(p^2) by exponentiation against the table) failed"); return H.rc; }
    *out = &H.K;
    return WS_OK;
}

// ---- device ----
typedef Curve<Fq29> G1d;                  // products as calls (code size; the kernels are latency chains, not issue bound)
typedef G2R29 G2d;

__device__ inline bool ge_words(const Fe& x, const uint64_t* m) {        // x >= m
    for (int i = 3; i >= 0; i--) {
        if (x.l[i] > m[i]) return true;
        if (x.l[i] < m[i]) return false;
    }
    return true;
}
__device__ inline F29 load_plain(const Fe& x, const PairConsts* K) { return Fq29::mul(Fq29::unpack(x), K->to_int); }

// per proof, written by verify_prepare: xA yA | xIC yIC' | xC yC' | xB.c0 xB.c1 yB.c0 yB.c1, internal form packed (y' = -y), and
// whether IC(x) is infinity (its pairing is 1)
static const int kPtWords = 10;

__global__ __launch_bounds__(64) void verify_prepare_kernel(const Fe* __restrict__ proofs, const Fe* __restrict__ inputs, uint32_t n_inputs,
                                                              const Fe* __restrict__ ic, const uint8_t* __restrict__ ic_inf,
                                                              const PairConsts* __restrict__ K, int key_ok, uint32_t count,
                                                              uint8_t* __restrict__ status, Fe* __restrict__ pts, uint8_t* __restrict__ ic_is_inf) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const Fe* pr = proofs + (size_t)i * 12;
    bool reduced = true;
#pragma unroll 1
    for (int k = 0; k < 12; k++) reduced = reduced && !ge_words(pr[k], K->q);
    if (!reduced) { status[i] = 2; return; }
    if (!key_ok) { status[i] = 0; return; }
    typedef Fq29 F;
    // curve equations (the z coordinates, words 2, 7, 8, 11, are ignored: (x, y) is the point)
    const F29 three = F::add(F::dbl(F::one()), F::one());
    const F29 xA = load_plain(pr[0], K), yA = load_plain(pr[1], K), xC = load_plain(pr[9], K), yC = load_plain(pr[10], K);
    bool ok = F::eq(F::sqr(yA), F::add(F::mul(F::sqr(xA), xA), three)) && F::eq(F::sqr(yC), F::add(F::mul(F::sqr(xC), xC), three));
    const F2d xB = F2d{load_plain(pr[3], K), load_plain(pr[4], K)}, yB = F2d{load_plain(pr[5], K), load_plain(pr[6], K)};
    const F2d b2 = F2d{K->b2[0], K->b2[1]};
    ok = ok && Fq2d::eq(Fq2d::sqr(yB), Fq2d::add(Fq2d::mul(Fq2d::sqr(xB), xB), b2));
    const Fe* in = inputs + (size_t)i * n_inputs;
#pragma unroll 1
    for (uint32_t k = 0; k < n_inputs; k++) ok = ok && !ge_words(in[k], K->r);
    if (!ok) { status[i] = 0; return; }
    {   // [r] B == O  (full additions: no coordinate value stands for infinity here)
        const G2d::Pt Bp = G2d::Pt{xB, yB, Fq2d::one(), Fq2d::one()};
        G2d::Pt acc = G2d::infinity();
#pragma unroll 1
        for (int bit = 253; bit >= 0; bit--) {
            acc = G2d::dbl(acc);
            if ((K->r[bit >> 6] >> (bit & 63)) & 1) acc = G2d::add(acc, Bp);
        }
        if (!G2d::is_inf(acc)) { status[i] = 0; return; }
    }
    // IC(x): one chain over the bits of all inputs
    G1d::Pt acc = G1d::infinity();
#pragma unroll 1
    for (int bit = 253; bit >= 0; bit--) {
        acc = G1d::dbl(acc);
#pragma unroll 1
        for (uint32_t k = 0; k < n_inputs; k++) {
            if (((in[k].l[bit >> 6] >> (bit & 63)) & 1) && !ic_inf[k + 1])
                G1d::madd(acc, G1d::Aff{F::unpack(ic[2 * (k + 1)]), F::unpack(ic[2 * (k + 1) + 1])}, false);
        }
    }
    if (!ic_inf[0]) G1d::madd(acc, G1d::Aff{F::unpack(ic[0]), F::unpack(ic[1])}, false);
    Fe* o = pts + (size_t)i * kPtWords;
    const bool inf = G1d::is_inf(acc);
    ic_is_inf[i] = inf ? 1 : 0;
    if (inf) {
        o[2] = F::pack(F::zero());
        o[3] = F::pack(F::zero());
    } else {
        const Jac<F> j = G1d::to_affine_jac(acc);
        o[2] = F::pack(j.x);
        o[3] = F::pack(F::neg(j.y));
    }
    o[0] = F::pack(xA); o[1] = F::pack(yA);
    o[4] = F::pack(xC); o[5] = F::pack(F::neg(yC));
    o[6] = F::pack(xB.c0); o[7] = F::pack(xB.c1); o[8] = F::pack(yB.c0); o[9] = F::pack(yB.c1);
    status[i] = kPending;
}

// one stored line (lambda', c3 = lambda' x_T' - y_T') at P = (x, y): l0 = y, l1 = -lambda' x, l3 = c3;  nx = -x
__device__ inline void stored_line(F12d* f, const Fe* __restrict__ t, const F29& nx, const F29& y) {
    const F2d lam = F2d{Fq29::unpack(t[0]), Fq29::unpack(t[1])}, l3 = F2d{Fq29::unpack(t[2]), Fq29::unpack(t[3])};
    const F2d l0 = F2d{y, Fq29::zero()}, l1 = f2d_scale(lam, nx);
    f12d_mul_line(f, f, &l0, &l1, &l3);
}

// lines: per Miller step (a doubling, or the addition after it on a set bit of T) four words for gamma2 then four for delta2
__global__ __launch_bounds__(64) void verify_miller_kernel(const uint8_t* __restrict__ status, const Fe* __restrict__ pts,
                                                             const uint8_t* __restrict__ ic_is_inf, const Fe* __restrict__ lines,
                                                             int gamma_on, int delta_on, const Fe* __restrict__ m_ab,
                                                             const PairConsts* __restrict__ K, uint32_t count, Fe* __restrict__ f_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count || status[i] != kPending) return;
    typedef Fq29 B;
    typedef Fq2d F;
    const Fe* p = pts + (size_t)i * kPtWords;
    const F29 nxA = B::neg(B::unpack(p[0])), yA = B::unpack(p[1]);
    const F29 nxI = B::neg(B::unpack(p[2])), yI = B::unpack(p[3]);
    const F29 nxC = B::neg(B::unpack(p[4])), yC = B::unpack(p[5]);
    const F2d xQ = F2d{B::unpack(p[6]), B::unpack(p[7])}, yQ = F2d{B::unpack(p[8]), B::unpack(p[9])};
    const bool with_gamma = gamma_on && !ic_is_inf[i];
    F2d X = xQ, Y = yQ, Z = F::one();
    F12d f;
    f12d_set_one(&f);
    uint32_t step = 0;
#pragma unroll 1
    for (int bit = 125; bit >= 0; bit--) {
        f12d_sqr(&f, &f);
        {   // T <- 2T; the tangent at T, scaled by 2 Y Z^3
            const F2d A = F::sqr(X), Bq = F::sqr(Y), Cq = F::sqr(Bq);
            const F2d S = F::dbl(F::dbl(F::mul(X, Bq)));
            const F2d M = F::add(F::dbl(A), A);
            const F2d Z2 = F::sqr(Z);
            const F2d Z3 = F::dbl(F::mul(Y, Z));
            const F2d l0 = f2d_scale(F::mul(Z3, Z2), yA), l1 = f2d_scale(F::mul(M, Z2), nxA), l3 = F::sub(F::mul(M, X), F::dbl(Bq));
            const F2d X3 = F::sub(F::sqr(M), F::dbl(S));
            Y = F::sub(F::mul(M, F::sub(S, X3)), F::dbl(F::dbl(F::dbl(Cq))));
            X = X3;
            Z = Z3;
            f12d_mul_line(&f, &f, &l0, &l1, &l3);
        }
        if (with_gamma) stored_line(&f, lines + (size_t)step * 8, nxI, yI);
        if (delta_on) stored_line(&f, lines + (size_t)step * 8 + 4, nxC, yC);
        step++;
        if ((K->ate[bit >> 6] >> (bit & 63)) & 1) {
            {   // T <- T + Q; the chord through T and Q, scaled by Z3 = Z (x_Q Z^2 - X)
                const F2d Z2 = F::sqr(Z);
                const F2d H = F::sub(F::mul(xQ, Z2), X), R = F::sub(F::mul(yQ, F::mul(Z2, Z)), Y);
                const F2d Z3 = F::mul(Z, H), HH = F::sqr(H);
                const F2d HHH = F::mul(H, HH), V = F::mul(X, HH);
                const F2d l0 = f2d_scale(Z3, yA), l1 = f2d_scale(R, nxA), l3 = F::sub(F::mul(R, xQ), F::mul(Z3, yQ));
                const F2d X3 = F::sub(F::sub(F::sqr(R), HHH), F::dbl(V));
                Y = F::sub(F::mul(R, F::sub(V, X3)), F::mul(Y, HHH));
                X = X3;
                Z = Z3;
                f12d_mul_line(&f, &f, &l0, &l1, &l3);
            }
            if (with_gamma) stored_line(&f, lines + (size_t)step * 8, nxI, yI);
            if (delta_on) stored_line(&f, lines + (size_t)step * 8 + 4, nxC, yC);
            step++;
        }
    }
    {   // the key's own pairing
        F12d m;
#pragma unroll 1
        for (int k = 0; k < 6; k++) m.c[k] = F2d{B::unpack(m_ab[2 * k]), B::unpack(m_ab[2 * k + 1])};
        f12d_mul(&f, &f, &m);
    }
    Fe* o = f_out + (size_t)i * 12;
#pragma unroll 1
    for (int k = 0; k < 6; k++) { o[2 * k] = B::pack(f.c[k].c0); o[2 * k + 1] = B::pack(f.c[k].c1); }
}

__global__ __launch_bounds__(64) void verify_finalexp_kernel(uint8_t* __restrict__ status, const Fe* __restrict__ f_in,
                                                               const PairConsts* __restrict__ K, int plain, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count || status[i] != kPending) return;
    const Fe* p = f_in + (size_t)i * 12;
    F12d f, e;
#pragma unroll 1
    for (int k = 0; k < 6; k++) f.c[k] = F2d{Fq29::unpack(p[2 * k]), Fq29::unpack(p[2 * k + 1])};
    f12d_final_exp(&e, &f, K, plain);
    status[i] = f12d_is_one(&e) ? 1 : 0;
}

// ---- host: one call ----
namespace {
struct KeyPrep {
    bool key_ok = true;
    bool gamma_on = false, delta_on = false;
    std::vector<Fe> ic;            // 2 words per IC point, internal form
    std::vector<uint8_t> ic_inf;
    std::vector<Fe> lines;         // 8 words per Miller step
    Fe m_ab[12];
};
size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// everything that depends on the key alone; WS_ERR_FORMAT for an unreduced key coordinate
int prepare_key(const uint8_t* vk, uint64_t n_inputs, KeyPrep* P) {
    G1A alfa1;
    G2A beta2, gamma2, delta2;
    if (!load_g1(vk, false, &alfa1) || !load_g2(vk + 64, false, &beta2) || !load_g2(vk + 192, false, &gamma2) || !load_g2(vk + 320, false, &delta2)) {
        set_last_error("verify: a coordinate is not a reduced field element");
        return WS_ERR_FORMAT;
    }
    std::vector<G1A> icp(n_inputs + 1);
    for (uint64_t i = 0; i <= n_inputs; i++)
        if (!load_g1(vk + 448 + i * 64, false, &icp[i])) { set_last_error("verify: IC coordinate not reduced"); return WS_ERR_FORMAT; }
    P->key_ok = g1_ok(alfa1) && g2_ok(beta2) && g2_ok(gamma2) && g2_ok(delta2);
    for (uint64_t i = 0; P->key_ok && i <= n_inputs; i++) P->key_ok = g1_ok(icp[i]);
    if (!P->key_ok) return WS_OK;
    P->ic.resize(2 * (n_inputs + 1));
    P->ic_inf.resize(n_inputs + 1);
    for (uint64_t i = 0; i <= n_inputs; i++) {
        P->ic_inf[i] = icp[i].inf ? 1 : 0;
        P->ic[2 * i] = pk_internal(icp[i].x);
        P->ic[2 * i + 1] = pk_internal(icp[i].y);
    }
    // the line coefficients do not depend on P: any finite P records them
    const G1A gen = G1A{Fq::one(), Fq::to_mont(Fe{{2, 0, 0, 0}}), false};
    std::vector<F2> lg, ld;
    F12 m;
    if (!miller_ate(gamma2, gen, &m, &lg) || !miller_ate(delta2, gen, &m, &ld)) { P->key_ok = false; return WS_OK; }
    P->gamma_on = !lg.empty();       // (a key point at infinity pairs to 1: no lines)
    P->delta_on = !ld.empty();
    const size_t steps = P->gamma_on ? lg.size() / 2 : ld.size() / 2;
    if (P->gamma_on && P->delta_on && lg.size() != ld.size()) { P->key_ok = false; return WS_OK; }
    P->lines.assign(steps * 8 + 8, Fe{{0, 0, 0, 0}});
    for (size_t s = 0; s < steps; s++) {
        if (P->gamma_on) { P->lines[8 * s] = pk_internal(lg[2 * s].c0); P->lines[8 * s + 1] = pk_internal(lg[2 * s].c1);
                           P->lines[8 * s + 2] = pk_internal(lg[2 * s + 1].c0); P->lines[8 * s + 3] = pk_internal(lg[2 * s + 1].c1); }
        if (P->delta_on) { P->lines[8 * s + 4] = pk_internal(ld[2 * s].c0); P->lines[8 * s + 5] = pk_internal(ld[2 * s].c1);
                           P->lines[8 * s + 6] = pk_internal(ld[2 * s + 1].c0); P->lines[8 * s + 7] = pk_internal(ld[2 * s + 1].c1); }
    }
    G1A na = alfa1;
    na.y = Fq::neg(na.y);
    if (!miller_ate(beta2, na, &m)) { P->key_ok = false; return WS_OK; }
    for (int k = 0; k < 6; k++) { P->m_ab[2 * k] = pk_internal(m.c[k].c0); P->m_ab[2 * k + 1] = pk_internal(m.c[k].c1); }
    return WS_OK;
}
}  // namespace

int groth16_verify_batch(const uint8_t* vk, size_t vk_len, const void* inputs, uint64_t n_inputs, const void* proofs384, uint64_t count,
                         uint8_t* status_host, bool on_device, hipStream_t s) {
    Context* X = ctx();
    if (!X) return WS_ERR_NOINIT;
    if (count == 0) return WS_OK;
    if (!vk || !proofs384 || !status_host) return WS_ERR_ARG;
    // (compared without the multiplication, like the single call: (n_inputs + 1) * 64 wraps for n_inputs near 2^58)
    if (vk_len < 512 || n_inputs > (vk_len - 448) / 64 - 1) { set_last_error("verification key has fewer IC points than inputs + 1"); return WS_ERR_SIZE; }
    if (count > ((uint64_t)1 << 24)) { set_last_error("verify_batch: more than 2^24 proofs in one call"); return WS_ERR_SIZE; }
    if (n_inputs && !inputs) return WS_ERR_ARG;
    const PairConsts* K = nullptr;
    int rc = pairing_consts(&K);
    if (rc) return rc;
    KeyPrep P;
    if ((rc = prepare_key(vk, n_inputs, &P))) return rc;
    const uint32_t n = (uint32_t)count, n_in = (uint32_t)n_inputs;

    LaneLock L = acquire_lane(X);
    if (!s) s = L->stream;
    const Fe* d_proofs = (const Fe*)proofs384;
    const Fe* d_inputs = (const Fe*)inputs;
    if (!on_device) {
        WS_HIP_CHECK(L->host_in[0].reserve((size_t)n * 384));
        if ((rc = upload_staged(L->host_in[0].p, proofs384, (size_t)n * 384, s))) return rc;
        d_proofs = L->host_in[0].as<Fe>();
        if (n_in) {
            WS_HIP_CHECK(L->host_in[1].reserve((size_t)n * n_in * 32));
            if ((rc = upload_staged(L->host_in[1].p, inputs, (size_t)n * n_in * 32, s))) return rc;
            d_inputs = L->host_in[1].as<Fe>();
        }
    }
    // one workspace: constants | IC | IC flags | lines | m_ab | points | IC(x) flags | Miller values | status
    std::vector<uint8_t> head;
    auto put = [&](const void* p, size_t bytes) { const size_t o = head.size(); head.resize(align256(o + (bytes ? bytes : 1))); if (bytes) memcpy(head.data() + o, p, bytes); return o; };
    const size_t o_k = put(K, sizeof *K), o_ic = put(P.ic.data(), P.ic.size() * 32), o_icf = put(P.ic_inf.data(), P.ic_inf.size());
    const size_t o_ln = put(P.lines.data(), P.lines.size() * 32), o_m = put(P.m_ab, sizeof P.m_ab);
    const size_t o_pts = head.size(), o_inf = o_pts + align256((size_t)n * kPtWords * 32), o_f = o_inf + align256(n);
    const size_t o_st = o_f + align256((size_t)n * 384), total = o_st + align256(n);
    WS_HIP_CHECK(L->verify_ws.reserve(total));
    uint8_t* ws = L->verify_ws.as<uint8_t>();
    WS_HIP_CHECK(hipMemcpyAsync(ws, head.data(), head.size(), hipMemcpyHostToDevice, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));        // (`head` is pageable and leaves scope; the copy is a few tens of kilobytes)
    const PairConsts* d_K = (const PairConsts*)(ws + o_k);
    uint8_t* d_status = ws + o_st;
    const dim3 grid(ceil_div_u64(n, 64)), block(64);
    const int plain = (int)tuning_get("VERIFY_PLAIN_EXP", 0);      // 0 shipped; 1 plain exponent; 2 hard part bit by bit

    X->timer.begin("verify_prepare", s);
    hipLaunchKernelGGL(verify_prepare_kernel, grid, block, 0, s, d_proofs, d_inputs, n_in, (const Fe*)(ws + o_ic), (const uint8_t*)(ws + o_icf), d_K,
                       P.key_ok ? 1 : 0, n, d_status, (Fe*)(ws + o_pts), ws + o_inf);
    WS_HIP_CHECK(hipGetLastError());
    X->timer.end(s);
    if (P.key_ok) {
        X->timer.begin("verify_miller", s);
        hipLaunchKernelGGL(verify_miller_kernel, grid, block, 0, s, (const uint8_t*)d_status, (const Fe*)(ws + o_pts), (const uint8_t*)(ws + o_inf),
                           (const Fe*)(ws + o_ln), P.gamma_on ? 1 : 0, P.delta_on ? 1 : 0, (const Fe*)(ws + o_m), d_K, n, (Fe*)(ws + o_f));
        WS_HIP_CHECK(hipGetLastError());
        X->timer.end(s);
        X->timer.begin(plain == 1 ? "verify_finalexp_plain" : plain == 2 ? "verify_finalexp_bits" : "verify_finalexp", s);
        hipLaunchKernelGGL(verify_finalexp_kernel, grid, block, 0, s, d_status, (const Fe*)(ws + o_f), d_K, plain, n);
        WS_HIP_CHECK(hipGetLastError());
        X->timer.end(s);
    }
    WS_HIP_CHECK(hipMemcpyAsync(status_host, d_status, n, hipMemcpyDeviceToHost, s));
    WS_HIP_CHECK(hipStreamSynchronize(s));
    return WS_OK;
}

}  // namespace wsnark
