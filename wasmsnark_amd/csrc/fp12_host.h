// fp12_host.h -- the HOST pairing arithmetic of the Groth16 verifier: Fp12 = Fp2[w]/(w^6 - xi) as one flat degree-6 extension,
// the affine ate Miller loop and the plain final exponentiation, on the saturated host field (field.h / fp2.h).
// Moved here unchanged from verify.hip so that three users share ONE copy: wsnark_groth16_verify (verify.hip, the pinned
// single-proof verifier), the batch verifier's per-key preparation (pairing.hip: key checks, the line tables of the key's fixed
// G2 points, the Miller value of (-alfa1, beta2)) and the yardstick of the device Fp12 self-test (selftest.hip, impl 2).
// The formulas and the argument why any pairing gives the same verdict are at the top of verify.hip.
#pragma once
#include <string.h>

#include <vector>

#include "curve.h"
#include "pairing_consts.h"

namespace wsnark {
namespace hostpair {

typedef Fe2 F2;   // Fq2 element, Montgomery form

struct F12 {
    F2 c[6];      // sum c[i] w^i,  w^6 = xi
};

inline F2 f2_mul_xi(const F2& a) {          // (a0 + a1 u)(9 + u) = (9 a0 - a1) + (9 a1 + a0) u
    Fe a0_2 = Fq::dbl(a.c0), a0_4 = Fq::dbl(a0_2), a0_8 = Fq::dbl(a0_4), a0_9 = Fq::add(a0_8, a.c0);
    Fe a1_2 = Fq::dbl(a.c1), a1_4 = Fq::dbl(a1_2), a1_8 = Fq::dbl(a1_4), a1_9 = Fq::add(a1_8, a.c1);
    return F2{Fq::sub(a0_9, a.c1), Fq::add(a1_9, a.c0)};
}
inline F12 f12_one() {
    F12 r;
    for (auto& x : r.c) x = Fq2::zero();
    r.c[0] = Fq2::one();
    return r;
}
inline bool f12_is_one(const F12& a) {
    if (!Fq2::eq(a.c[0], Fq2::one())) return false;
    for (int i = 1; i < 6; i++) if (!Fq2::is_zero(a.c[i])) return false;
    return true;
}
inline F12 f12_mul(const F12& a, const F12& b) {
    F2 lo[6], hi[5];
    for (auto& x : lo) x = Fq2::zero();
    for (auto& x : hi) x = Fq2::zero();
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            const F2 t = Fq2::mul(a.c[i], b.c[j]);
            if (i + j < 6) lo[i + j] = Fq2::add(lo[i + j], t);
            else hi[i + j - 6] = Fq2::add(hi[i + j - 6], t);
        }
    F12 r;
    for (int k = 0; k < 6; k++) r.c[k] = k < 5 ? Fq2::add(lo[k], f2_mul_xi(hi[k])) : lo[k];
    return r;
}
// a * (l0 + l1 w + l3 w^3): the line's three non-zero coefficients
inline F12 f12_mul_line(const F12& a, const F2& l0, const F2& l1, const F2& l3) {
    F2 lo[6], hi[5];
    for (auto& x : lo) x = Fq2::zero();
    for (auto& x : hi) x = Fq2::zero();
    const F2* L[3] = {&l0, &l1, &l3};
    const int deg[3] = {0, 1, 3};
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 3; j++) {
            const F2 t = Fq2::mul(a.c[i], *L[j]);
            const int k = i + deg[j];
            if (k < 6) lo[k] = Fq2::add(lo[k], t);
            else hi[k - 6] = Fq2::add(hi[k - 6], t);
        }
    F12 r;
    for (int k = 0; k < 6; k++) r.c[k] = k < 5 ? Fq2::add(lo[k], f2_mul_xi(hi[k])) : lo[k];
    return r;
}

// (p^12 - 1) / r, little-endian 64-bit words (2790 bits)
static const uint64_t kFinalExp[44] = {
    0x86964b64ca86f120ull, 0x40a4efb7e54523a4ull, 0x837fa97896e84abbull, 0x361102b6b9b2b918ull,
    0xc0de81def35692daull, 0xbe04c7e8a6c3c760ull, 0xd766f9c9d570bb7full, 0xc230974d83561841ull,
    0x5bba1668c3be69a3ull, 0x7f3811c410526294ull, 0x29baee7ddadda71cull, 0xbf813b8d145da900ull,
    0x641bbadf423f9a2cull, 0xa80bb4ea44eacc5eull, 0xcd65664814fde37cull, 0x4a0364b9580291d2ull,
    0xee93dfb10826f0ddull, 0x6b42db8dc5514724ull, 0xbb10cf430b0f3785ull, 0x40494e406f804216ull,
    0x55cfe107acf3aafbull, 0x2088ec80e0ebae87ull, 0x846a3ed011a337a0ull, 0x48a45a4a1e3a5195ull,
    0xe5664568dfc50e16ull, 0xab6a41294c0cc4ebull, 0x82d0d602d268c7daull, 0x6668449aed3cc48aull,
    0x5062cd0fb2015dfcull, 0x7f2940a8b1ddb3d1ull, 0x77f5b63a2a226448ull, 0xfef0781361e443aeull,
    0xf977870e88d5c6c8ull, 0x790364a61f676baaull, 0x5887e72eceaddea3ull, 0x1377e563a09a1b70ull,
    0x0c54efee1bd8c3b2ull, 0x3ec3d15ad524d8f7ull, 0xdaf15466b2383a5dull, 0xe1e30a73bb94fec0ull,
    0x6a1c71015f3f7be2ull, 0x842d43bf6369b1ffull, 0x20fddadf107d20bcull, 0x0000002f4b6dc970ull,
};
inline F12 final_exponentiation(const F12& f) {
    F12 acc = f12_one();
    bool started = false;
    for (int i = 44 * 64 - 1; i >= 0; i--) {
        if (started) acc = f12_mul(acc, acc);
        if ((kFinalExp[i >> 6] >> (i & 63)) & 1) { acc = started ? f12_mul(acc, f) : f; started = true; }
    }
    return acc;
}

static const uint64_t kAteLoop[2] = {0xf83e9682e87cfd46ull, 0x6f4d8248eeb859fbull};   // T = p - r (127 bits; bit 126 is the leading one)
struct G1A { Fe x, y; bool inf; };      // affine, Montgomery
struct G2A { F2 x, y; bool inf; };

// f_{T,Q}(P) for T = p - r, affine steps on the twist.  Returns false if a step degenerates (Q not of order r).
// lines (optional): receives, per doubling / addition step in loop order, the two P-independent numbers of that step's line,
// (lambda', lambda' x_T' - y_T'): the batch verifier uploads them for the key's fixed G2 points (pairing.hip)
inline bool miller_ate(const G2A& Q, const G1A& P, F12* out, std::vector<F2>* lines = nullptr) {
    *out = f12_one();
    if (Q.inf || P.inf) return true;                          // e(O, .) = e(., O) = 1
    const uint64_t* T = kAteLoop;
    const F2 xP = F2{P.x, Fq::zero()}, yP = F2{P.y, Fq::zero()};
    F2 tx = Q.x, ty = Q.y;
    F12 f = f12_one();
    for (int i = 125; i >= 0; i--) {                          // bit 126 is the leading one
        // doubling step: lambda = 3 x^2 / (2 y)
        if (Fq2::is_zero(ty)) return false;
        const F2 x2 = Fq2::sqr(tx);
        const F2 lam = Fq2::mul(Fq2::add(Fq2::dbl(x2), x2), Fq2::inv(Fq2::dbl(ty)));
        f = f12_mul(f, f);
        f = f12_mul_line(f, yP, Fq2::neg(Fq2::mul(lam, xP)), Fq2::sub(Fq2::mul(lam, tx), ty));
        if (lines) { lines->push_back(lam); lines->push_back(Fq2::sub(Fq2::mul(lam, tx), ty)); }
        const F2 nx = Fq2::sub(Fq2::sqr(lam), Fq2::dbl(tx));
        ty = Fq2::sub(Fq2::mul(lam, Fq2::sub(tx, nx)), ty);
        tx = nx;
        if ((T[i >> 6] >> (i & 63)) & 1) {
            // addition step with Q: lambda = (yT - yQ) / (xT - xQ)
            const F2 dx = Fq2::sub(tx, Q.x);
            if (Fq2::is_zero(dx)) return false;
            const F2 l2 = Fq2::mul(Fq2::sub(ty, Q.y), Fq2::inv(dx));
            f = f12_mul_line(f, yP, Fq2::neg(Fq2::mul(l2, xP)), Fq2::sub(Fq2::mul(l2, Q.x), Q.y));
            if (lines) { lines->push_back(l2); lines->push_back(Fq2::sub(Fq2::mul(l2, Q.x), Q.y)); }
            const F2 ax = Fq2::sub(Fq2::sub(Fq2::sqr(l2), tx), Q.x);
            ty = Fq2::sub(Fq2::mul(l2, Fq2::sub(Q.x, ax)), Q.y);
            tx = ax;
        }
    }
    *out = f;
    return true;
}

// plain 32-byte LE integers -> Montgomery; false if a coordinate is >= q
inline bool load_fq(const uint8_t* p, Fe* out) {
    Fe v;
    memcpy(&v, p, 32);
    const Fe red = Fq::reduce_full(v);
    if (!Fq::eq(red, v)) return false;
    *out = Fq::to_mont(v);
    return true;
}
// (x, y[, z]) plain coordinates; the z of a proof element must be a reduced field element but is otherwise ignored
// (the reference forces z = 1).  Key points (no z): (0, 0) stands for infinity, as in proving keys.
inline bool load_g1(const uint8_t* p, bool has_z, G1A* out) {
    Fe z = Fq::one();
    if (!load_fq(p, &out->x) || !load_fq(p + 32, &out->y) || (has_z && !load_fq(p + 64, &z))) return false;
    out->inf = !has_z && Fq::is_zero(out->x) && Fq::is_zero(out->y);
    return true;
}
inline bool load_g2(const uint8_t* p, bool has_z, G2A* out) {
    F2 z = Fq2::one();
    if (!load_fq(p, &out->x.c0) || !load_fq(p + 32, &out->x.c1) || !load_fq(p + 64, &out->y.c0) || !load_fq(p + 96, &out->y.c1)) return false;
    if (has_z && (!load_fq(p + 128, &z.c0) || !load_fq(p + 160, &z.c1))) return false;
    out->inf = !has_z && Fq2::is_zero(out->x) && Fq2::is_zero(out->y);
    return true;
}
// y^2 == x^3 + 3 (G1 has cofactor 1: on the curve is in the group)
inline bool g1_ok(const G1A& P) {
    if (P.inf) return true;
    const Fe three = Fq::to_mont(Fe{{3, 0, 0, 0}});
    return Fq::eq(Fq::sqr(P.y), Fq::add(Fq::mul(Fq::sqr(P.x), P.x), three));
}
// on the twist y^2 == x^3 + 3/(9 + u) (src/bn128/build_bn128.js:79-90) AND in the order-r subgroup: [r] Q == O
inline bool g2_ok(const G2A& Q) {
    if (Q.inf) return true;
    static const F2 b2 = Fq2::mul(F2{Fq::to_mont(Fe{{3, 0, 0, 0}}), Fq::zero()}, Fq2::inv(F2{Fq::to_mont(Fe{{9, 0, 0, 0}}), Fq::one()}));
    if (!Fq2::eq(Fq2::sqr(Q.y), Fq2::add(Fq2::mul(Fq2::sqr(Q.x), Q.x), b2))) return false;
    const Fe r = Fr::modulus();
    const G2::Pt rq = G2::mul_bytes(G2::Pt{Q.x, Q.y, Fq2::one(), Fq2::one()}, reinterpret_cast<const uint8_t*>(&r), 32);
    return G2::is_inf(rq);
}

// ---- yardsticks of the device Fp12 self-test (selftest.hip, impl 2) and the first-use check of the Frobenius table ----
// a^e by plain MSB-first square-and-multiply, e given as little-endian 64-bit words (e > 0)
inline F12 f12_pow(const F12& a, const uint64_t* e, int bits) {
    F12 acc = f12_one();
    bool started = false;
    for (int i = bits - 1; i >= 0; i--) {
        if (started) acc = f12_mul(acc, acc);
        if ((e[i >> 6] >> (i & 63)) & 1) { acc = started ? f12_mul(acc, a) : a; started = true; }
    }
    return acc;
}
inline F2 f2_pow(const F2& a, const uint64_t* e, int bits) {
    F2 acc = Fq2::one();
    for (int i = bits - 1; i >= 0; i--) {
        acc = Fq2::sqr(acc);
        if ((e[i >> 6] >> (i & 63)) & 1) acc = Fq2::mul(acc, a);
    }
    return acc;
}
// twelve PLAIN little-endian Fq values (coefficient i of w^i = (c0, c1)) <-> F12; values are taken mod q
inline F12 f12_from_plain(const uint8_t* p) {
    F12 r;
    for (int i = 0; i < 6; i++) {
        Fe a, b;
        memcpy(&a, p + 64 * i, 32);
        memcpy(&b, p + 64 * i + 32, 32);
        r.c[i] = F2{Fq::to_mont(Fq::reduce_full(a)), Fq::to_mont(Fq::reduce_full(b))};
    }
    return r;
}
inline void f12_to_plain(const F12& a, uint8_t* p) {
    for (int i = 0; i < 6; i++) {
        const Fe x = Fq::from_mont(a.c[i].c0), y = Fq::from_mont(a.c[i].c1);
        memcpy(p + 64 * i, &x, 32);
        memcpy(p + 64 * i + 32, &y, 32);
    }
}

}  // namespace hostpair
}  // namespace wsnark
