// fp12.h -- Fp12 = Fq2[w]/(w^6 - xi), xi = 9 + u, on the DEVICE field (radix-2^29 Montgomery, field29.h; Fq2 on one lane, fp2.h):
// the arithmetic of the batch verifier's Miller loop and final exponentiation (pairing.hip) and of wsnark_selftest_fp12.
// The same flat degree-6 extension as the host verifier's (fp12_host.h), so values compare coefficient by coefficient.
//
// One lane holds one element; an element is 12 x 9 = 108 words and lives in the lane's PRIVATE memory, not in registers: every
// function here takes pointers, is a real (non-inlined) device function and walks the coefficients in ROLLED loops, so that what
// is live in VGPRs is one column accumulator and the two Fq2 operands of the product in flight (DESIGN.md "pairing.hip" has the
// register / scratch figures and what that costs).  All stored coefficients are strict ([0, 2p), field29.h): every sum and
// difference here is the corrected form, so any stored value may be either operand of a product.
//   products per operation (Fq2 products; one is two fused double products of the base field):
//     mul 36 (+ 5 by xi, additions only)    sqr 15 + 6 squarings    mul_line 18    frob2 5 x 2 base products
//     inv = 1 mul + Fp6 inverse (9 products, 3 squarings, one Fq2 inverse = one Fermat inversion of the base field) + 1 mul
#pragma once
#include "curve.h"
#include "pairing_consts.h"

namespace wsnark {

typedef Fp2T<Fq29> Fq2d;
typedef Fq2d::El F2d;            // Fe2T<F29>: 18 words
struct F12d {
    F2d c[6];                    // sum c[i] w^i
};

// what the device needs besides its operands: computed on the host at first use (pairing.hip: pairing_consts), one upload per call
struct PairConsts {
    F29 gamma[5];                // xi^(k (p^2 - 1)/6), k = 1..5, internal form: (c w^k)^(p^2) = gamma[k-1] c w^k
    F29 to_int;                  // 2^522 mod p as a plain integer: plain x -> internal x 2^261 with one product
    uint64_t hard[kExpHardWords];        // (p^4 - p^2 + 1) / r
    uint64_t plain[44];                  // (p^12 - 1) / r, the host verifier's exponent
    uint64_t q[4], r[4];                 // the two primes (range checks, the subgroup test)
    uint64_t ate[2];                     // T = p - r, the Miller loop's 127 bits
    F29 b2[2];                           // 3 / xi, the twist's constant, internal form
    F29 gamma1[5][2];                    // xi^(k (p - 1)/6) in Fq2, k = 1..5: (c w^k)^p = conj(c) gamma1[k-1] w^k
    uint64_t bn_x;                       // the curve's parameter x (63 bits)
};

#if defined(__HIP_DEVICE_COMPILE__) && !defined(WSNARK_EMUL)
#define WS_F12_FN static __device__ __attribute__((noinline))
#else
#define WS_F12_FN __device__ inline
#endif

// (a0 + a1 u)(9 + u) = (9 a0 - a1) + (9 a1 + a0) u
__device__ inline F2d f2d_mul_xi(const F2d& a) {
    typedef Fq29 B;
    const F29 a0_8 = B::dbl(B::dbl(B::dbl(a.c0))), a1_8 = B::dbl(B::dbl(B::dbl(a.c1)));
    return F2d{B::sub(B::add(a0_8, a.c0), a.c1), B::add(B::add(a1_8, a.c1), a.c0)};
}
// an Fq2 element times one of the base field
__device__ inline F2d f2d_scale(const F2d& a, const F29& s) { return F2d{Fq29::mul(a.c0, s), Fq29::mul(a.c1, s)}; }

__device__ inline void f12d_set_one(F12d* r) {
#pragma unroll 1
    for (int i = 0; i < 6; i++) r->c[i] = Fq2d::zero();
    r->c[0] = Fq2d::one();
}
__device__ inline bool f12d_is_one(const F12d* a) {
    bool ok = Fq2d::eq(a->c[0], Fq2d::one());
#pragma unroll 1
    for (int i = 1; i < 6; i++) ok = ok && Fq2d::is_zero(a->c[i]);
    return ok;
}
// columns 0..10 of a product folded with w^6 = xi
__device__ inline void f12d_fold(F12d* r, const F2d* col) {
#pragma unroll 1
    for (int k = 0; k < 5; k++) r->c[k] = Fq2d::add(col[k], f2d_mul_xi(col[k + 6]));
    r->c[5] = col[5];
}
// r = a b (r may be a or b)
WS_F12_FN void f12d_mul(F12d* r, const F12d* a, const F12d* b) {
    F2d col[11];
#pragma unroll 1
    for (int k = 0; k < 11; k++) col[k] = Fq2d::zero();
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
        const F2d ai = a->c[i];
#pragma unroll 1
        for (int j = 0; j < 6; j++) col[i + j] = Fq2d::add(col[i + j], Fq2d::mul(ai, b->c[j]));
    }
    f12d_fold(r, col);
}
// r = a^2: the 15 mixed products once, doubled, plus the 6 squares
WS_F12_FN void f12d_sqr(F12d* r, const F12d* a) {
    F2d col[11];
#pragma unroll 1
    for (int k = 0; k < 11; k++) col[k] = Fq2d::zero();
#pragma unroll 1
    for (int i = 0; i < 5; i++) {
        const F2d ai = a->c[i];
#pragma unroll 1
        for (int j = i + 1; j < 6; j++) col[i + j] = Fq2d::add(col[i + j], Fq2d::mul(ai, a->c[j]));
    }
#pragma unroll 1
    for (int k = 0; k < 11; k++) col[k] = Fq2d::dbl(col[k]);
#pragma unroll 1
    for (int i = 0; i < 6; i++) col[2 * i] = Fq2d::add(col[2 * i], Fq2d::sqr(a->c[i]));
    f12d_fold(r, col);
}
// r = a (l0 + l1 w + l3 w^3): a Miller line has three non-zero coefficients (r may be a)
WS_F12_FN void f12d_mul_line(F12d* r, const F12d* a, const F2d* l0, const F2d* l1, const F2d* l3) {
    F2d col[11];
#pragma unroll 1
    for (int k = 0; k < 11; k++) col[k] = Fq2d::zero();
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
        const F2d ai = a->c[i];
        col[i] = Fq2d::add(col[i], Fq2d::mul(ai, *l0));
        col[i + 1] = Fq2d::add(col[i + 1], Fq2d::mul(ai, *l1));
        col[i + 3] = Fq2d::add(col[i + 3], Fq2d::mul(ai, *l3));
    }
    f12d_fold(r, col);
}
// a^(p^6): w -> -w, the coefficients (in Fq2, fixed by p^2) stay
__device__ inline void f12d_conj(F12d* r, const F12d* a) {
#pragma unroll 1
    for (int i = 0; i < 6; i++) r->c[i] = (i & 1) ? Fq2d::neg(a->c[i]) : a->c[i];
}
// a^(p^2): coefficient k times gamma^k, gamma = xi^((p^2 - 1)/6) in Fq
WS_F12_FN void f12d_frob2(F12d* r, const F12d* a, const PairConsts* K) {
    r->c[0] = a->c[0];
#pragma unroll 1
    for (int i = 1; i < 6; i++) r->c[i] = f2d_scale(a->c[i], K->gamma[i - 1]);
}
// 1 / a (0 for a = 0): a^-1 = conj(a) / N, N = a conj(a) in Fp6 = Fq2[v]/(v^3 - xi), v = w^2 (the even coefficients)
WS_F12_FN void f12d_inv(F12d* r, const F12d* a) {
    typedef Fq2d F;
    F12d cj, n;
    f12d_conj(&cj, a);
    f12d_mul(&n, a, &cj);
    const F2d n0 = n.c[0], n1 = n.c[2], n2 = n.c[4];
    const F2d A = F::sub(F::sqr(n0), f2d_mul_xi(F::mul(n1, n2)));
    const F2d B = F::sub(f2d_mul_xi(F::sqr(n2)), F::mul(n0, n1));
    const F2d C = F::sub(F::sqr(n1), F::mul(n0, n2));
    const F2d t = F::add(F::mul(n0, A), f2d_mul_xi(F::add(F::mul(n2, B), F::mul(n1, C))));
    const F2d ti = F::inv(t);
#pragma unroll 1
    for (int i = 0; i < 6; i++) n.c[i] = F::zero();
    n.c[0] = F::mul(A, ti);
    n.c[2] = F::mul(B, ti);
    n.c[4] = F::mul(C, ti);
    f12d_mul(r, &cj, &n);
}
// a^p: the coefficients conjugated in Fq2, coefficient k times gamma_1^k, gamma_1 = xi^((p - 1)/6) in Fq2 (r may be a)
WS_F12_FN void f12d_frob1(F12d* r, const F12d* a, const PairConsts* K) {
    r->c[0] = F2d{a->c[0].c0, Fq29::neg(a->c[0].c1)};
#pragma unroll 1
    for (int i = 1; i < 6; i++) {
        const F2d g = F2d{K->gamma1[i - 1][0], K->gamma1[i - 1][1]};
        r->c[i] = Fq2d::mul(F2d{a->c[i].c0, Fq29::neg(a->c[i].c1)}, g);
    }
}
// (x + y s)^2 in Fq4 = Fq2[s]/(s^2 - xi): even part (x + y)(x + xi y) - x y - xi x y, odd part 2 x y
__device__ inline void f4d_sqr(const F2d& x, const F2d& y, F2d* even, F2d* odd) {
    typedef Fq2d F;
    const F2d t = F::mul(x, y);
    *even = F::sub(F::sub(F::mul(F::add(x, y), F::add(f2d_mul_xi(y), x)), t), f2d_mul_xi(t));
    *odd = F::dbl(t);
}
// r = a^2 for a in the cyclotomic subgroup (a^(p^6 + 1) = 1 and a^(p^4 - p^2 + 1) = 1: everything after the easy part of the
// final exponentiation): Granger-Scott's squaring, three squarings in Fq4 = 6 Fq2 products instead of 15 + 6 squarings.  In the
// tower Fp12 = Fp6[w]/(w^2 - v), Fp6 = Fq2[v]/(v^3 - xi), v = w^2, the element is (a0 + a2 v + a4 v^2) + (a1 + a3 v + a5 v^2) w and
// the three Fq4 elements are (a0, a3), (a1, a4), (a2, a5).  (r may be a)
WS_F12_FN void f12d_cyc_sqr(F12d* r, const F12d* a) {
    typedef Fq2d F;
    F2d t0, t1, t2, t3, t4, t5;
    f4d_sqr(a->c[0], a->c[3], &t0, &t1);
    f4d_sqr(a->c[1], a->c[4], &t2, &t3);
    f4d_sqr(a->c[2], a->c[5], &t4, &t5);
    const F2d x5 = f2d_mul_xi(t5);
    const F2d z0 = a->c[0], z1 = a->c[3], z2 = a->c[1], z3 = a->c[4], z4 = a->c[2], z5 = a->c[5];
    auto minus = [](const F2d& t, const F2d& z) { const F2d d = F::sub(t, z); return F::add(F::dbl(d), t); };   // 3 t - 2 z
    auto plus = [](const F2d& t, const F2d& z) { const F2d d = F::add(t, z); return F::add(F::dbl(d), t); };    // 3 t + 2 z
    r->c[0] = minus(t0, z0);
    r->c[3] = plus(t1, z1);
    r->c[1] = plus(x5, z2);
    r->c[4] = minus(t4, z3);
    r->c[2] = minus(t2, z4);
    r->c[5] = plus(t3, z5);
}
// r = a^e, plain MSB-first square-and-multiply over the little-endian words of e (e > 0; r must not be a); cyc: a is in the
// cyclotomic subgroup and the squarings are Granger-Scott's
WS_F12_FN void f12d_pow(F12d* r, const F12d* a, const uint64_t* e, int bits, bool cyc) {
    bool started = false;
#pragma unroll 1
    for (int i = bits - 1; i >= 0; i--) {
        if (started) {
            if (cyc) f12d_cyc_sqr(r, r);
            else f12d_sqr(r, r);
        }
        if ((e[i >> 6] >> (i & 63)) & 1) {
            if (started) f12d_mul(r, r, a);
            else { *r = *a; started = true; }
        }
    }
}
// r = f^((p^4 - p^2 + 1)/r) for f in the cyclotomic subgroup, through the curve's parameter x (p and r are polynomials in x):
//   (p^4 - p^2 + 1)/r = p^3 + (6 x^2 + 1) p^2 + (-36 x^3 - 18 x^2 - 12 x + 1) p + (-36 x^3 - 30 x^2 - 18 x - 2)
// (tools/gen_pairing_consts.py asserts the identity), evaluated the way Scott, Benger, Charlemagne, Dominguez Perez and Kachisa
// arrange it ("On the final exponentiation for calculating pairings on ordinary elliptic curves", Pairing 2009): with
// fx = f^x, fx2 = fx^x, fx3 = fx2^x and inversion = conjugation in this subgroup,
//   y0 = f^p f^(p^2) f^(p^3), y1 = 1/f, y2 = fx2^(p^2), y3 = 1/fx^p, y4 = 1/(fx fx2^p), y5 = 1/fx2, y6 = 1/(fx3 fx3^p),
//   result = y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36  by the addition chain below: 3 x 62 squarings and 3 x 28 products for the powers
// of x, then 13 products, 4 squarings and 7 Frobenius maps instead of 760 squarings and 380 products.
WS_F12_FN void f12d_hard_bn(F12d* r, const F12d* f, const PairConsts* K) {
    F12d fx, fx2, fx3, t0, t1, y;
    f12d_pow(&fx, f, &K->bn_x, kBnXBits, true);
    f12d_pow(&fx2, &fx, &K->bn_x, kBnXBits, true);
    f12d_pow(&fx3, &fx2, &K->bn_x, kBnXBits, true);
    f12d_frob1(&y, &fx3, K);
    f12d_mul(&y, &y, &fx3);
    f12d_conj(&y, &y);                   // y6
    f12d_cyc_sqr(&t0, &y);
    f12d_frob1(&y, &fx2, K);
    f12d_mul(&y, &y, &fx);
    f12d_conj(&y, &y);                   // y4
    f12d_mul(&t0, &t0, &y);
    f12d_conj(&y, &fx2);                 // y5
    f12d_mul(&t0, &t0, &y);
    f12d_frob1(&t1, &fx, K);
    f12d_conj(&t1, &t1);                 // y3
    f12d_mul(&t1, &t1, &y);
    f12d_mul(&t1, &t1, &t0);
    f12d_frob2(&y, &fx2, K);             // y2
    f12d_mul(&t0, &t0, &y);
    f12d_cyc_sqr(&t1, &t1);
    f12d_mul(&t1, &t1, &t0);
    f12d_cyc_sqr(&t1, &t1);
    f12d_conj(&y, f);                    // y1
    f12d_mul(&t0, &t1, &y);
    f12d_frob1(&y, f, K);
    f12d_frob2(&fx, f, K);
    f12d_mul(&y, &y, &fx);
    f12d_frob1(&fx, &fx, K);
    f12d_mul(&y, &y, &fx);               // y0
    f12d_mul(&t1, &t1, &y);
    f12d_cyc_sqr(&t0, &t0);
    f12d_mul(r, &t0, &t1);
}
// r = f^((p^12 - 1)/r).  mode 1: the host verifier's plain exponent, bit by bit (the cross-check).  Otherwise the split form
// (p^12 - 1)/r = (p^6 - 1)(p^2 + 1) * hard:  t = conj(f) / f,  u = t^(p^2) t,  r = u^hard, the hard part through the curve's
// parameter (mode 0, shipped) or by square-and-multiply over its 761 bits (mode 2, the record of the intermediate step)
WS_F12_FN void f12d_final_exp(F12d* r, const F12d* f, const PairConsts* K, int mode) {
    if (mode == 1) {
        f12d_pow(r, f, K->plain, 44 * 64, false);
        return;
    }
    F12d t, u;
    f12d_inv(&u, f);
    f12d_conj(&t, f);
    f12d_mul(&t, &t, &u);
    f12d_frob2(&u, &t, K);
    f12d_mul(&u, &u, &t);
    if (mode == 2) f12d_pow(r, &u, K->hard, kExpHardBits, false);
    else f12d_hard_bn(r, &u, K);
}

// twelve PLAIN little-endian Fq values <-> the internal form (values >= q are taken mod q: the product reduces them)
__device__ inline void f12d_load_plain(F12d* r, const Fe* p, const PairConsts* K) {
#pragma unroll 1
    for (int i = 0; i < 6; i++) r->c[i] = F2d{Fq29::mul(Fq29::unpack(p[2 * i]), K->to_int), Fq29::mul(Fq29::unpack(p[2 * i + 1]), K->to_int)};
}
__device__ inline Fe f29_to_plain(const F29& a) {
    F29 one = Fq29::zero();
    one.v[0] = 1;
    return Fq29::pack(Fq29::canonical(Fq29::mul(a, one)));      // a 2^-261, canonical
}
__device__ inline void f12d_store_plain(Fe* p, const F12d* a) {
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
        p[2 * i] = f29_to_plain(a->c[i].c0);
        p[2 * i + 1] = f29_to_plain(a->c[i].c1);
    }
}

}  // namespace wsnark
