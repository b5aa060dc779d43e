// field.h -- 256-bit Montgomery prime-field arithmetic for BN128 (Fq, Fr), R = 2^256.
//
// One element = 4 x u64 limbs, little-endian, exactly the 32-byte layout of the
// reference (8 x u32 LE; /root/reference tools/buildpkey.js:57-77).  Every
// operation returns the canonical representative in [0,p) like the reference's
// f1m_* (src/build_f1m.js:67-113, 235-436), so intermediate arrays are
// bit-comparable with the reference.
//
// Replaces: f1m_mul/frm_mul, f1m_square,
// f1m_add/sub/neg, to/fromMontgomery, inverse.
//
// Shared by device kernels (one element per lane, limbs in VGPRs; the multiplier
// works on 32-bit half-limbs so each partial product is one v_mad_u64_u32) and by
// the host-side proof assembly (64-bit limbs with unsigned __int128).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#if defined(__HIP_DEVICE_COMPILE__)
#define WS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define WS_HD __host__ __device__ inline
#endif
#else
#define WS_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__) || defined(WSNARK_FORCE_32BIT_MUL)
#define WS_MUL32 1
#else
#define WS_MUL32 0
#endif

namespace wsnark {

struct alignas(16) Fe {
    uint64_t l[4];
};

// ---- parameters (src/bn128/build_bn128.js:19-20; constants SURVEY.md section 8) ----
struct FqParams {
    static constexpr uint64_t P0 = 0x3c208c16d87cfd47ull, P1 = 0x97816a916871ca8dull,
                              P2 = 0xb85045b68181585dull, P3 = 0x30644e72e131a029ull;
    static constexpr uint64_t NP = 0x87d20782e4866389ull;  // -p^-1 mod 2^64
    static constexpr uint64_t R0 = 0xd35d438dc58f0d9dull, R1 = 0x0a78eb28f5c70b3dull,   // 2^256 mod p
                              R2_ = 0x666ea36f7879462cull, R3 = 0x0e0a77c19a07df2full;
    static constexpr uint64_t RR0 = 0xf32cfc5b538afa89ull, RR1 = 0xb5e71911d44501fbull,  // 2^512 mod p
                              RR2 = 0x47ab1eff0a417ff6ull, RR3 = 0x06d89f71cab8351full;
};
struct FrParams {
    static constexpr uint64_t P0 = 0x43e1f593f0000001ull, P1 = 0x2833e84879b97091ull,
                              P2 = 0xb85045b68181585dull, P3 = 0x30644e72e131a029ull;
    static constexpr uint64_t NP = 0xc2e1f593efffffffull;
    static constexpr uint64_t R0 = 0xac96341c4ffffffbull, R1 = 0x36fc76959f60cd29ull,
                              R2_ = 0x666ea36f7879462eull, R3 = 0x0e0a77c19a07df2full;
    static constexpr uint64_t RR0 = 0x1bb8e645ae216da7ull, RR1 = 0x53fe3ab1e35c59e3ull,
                              RR2 = 0x8c49833d53bb8085ull, RR3 = 0x0216d0b17f4e44a5ull;
};

WS_HD uint64_t ws_addc(uint64_t a, uint64_t b, uint64_t cin, uint64_t* cout) {
    unsigned __int128 s = (unsigned __int128)a + b + cin;
    *cout = (uint64_t)(s >> 64);
    return (uint64_t)s;
}
WS_HD uint64_t ws_subb(uint64_t a, uint64_t b, uint64_t bin, uint64_t* bout) {
    unsigned __int128 d = (unsigned __int128)a - b - bin;
    *bout = (uint64_t)(d >> 64) & 1;
    return (uint64_t)d;
}


// 8 x 32-bit CIOS Montgomery product: every partial product is one 32x32+64 multiply-add
// (v_mad_u64_u32 on gfx950).  Deliberately a real (non-inlined) device function taking its
// operands by value in VGPRs: the curve formulas call it 10-40 times per group operation, and
// one ~5 KiB body keeps the kernels inside the instruction cache (and the build in minutes).
#if WS_MUL32
template <class P>
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __attribute__((noinline))
#else
inline
#endif
Fe mont_mul32(Fe a, Fe b) {
    const uint32_t p[8] = {(uint32_t)P::P0, (uint32_t)(P::P0 >> 32), (uint32_t)P::P1, (uint32_t)(P::P1 >> 32),
                           (uint32_t)P::P2, (uint32_t)(P::P2 >> 32), (uint32_t)P::P3, (uint32_t)(P::P3 >> 32)};
    const uint32_t np32 = (uint32_t)P::NP;
    uint32_t x[8], y[8], t[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        x[2 * i] = (uint32_t)a.l[i]; x[2 * i + 1] = (uint32_t)(a.l[i] >> 32);
        y[2 * i] = (uint32_t)b.l[i]; y[2 * i + 1] = (uint32_t)(b.l[i] >> 32);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) t[j] = 0;
    uint32_t t8 = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            c = (uint64_t)x[j] * y[i] + t[j] + c;
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        uint32_t top = t8 + (uint32_t)c;   // p < 2^254: never overflows
        uint32_t m = t[0] * np32;
        c = ((uint64_t)m * p[0] + t[0]) >> 32;
#pragma unroll
        for (int j = 1; j < 8; j++) {
            c = (uint64_t)m * p[j] + t[j] + c;
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += top;
        t[7] = (uint32_t)c;
        t8 = (uint32_t)(c >> 32);
    }
    Fe r;
#pragma unroll
    for (int i = 0; i < 4; i++) r.l[i] = (uint64_t)t[2 * i] | ((uint64_t)t[2 * i + 1] << 32);
    // final conditional subtraction -> canonical representative
    uint64_t bw = 0;
    Fe s;
    s.l[0] = ws_subb(r.l[0], P::P0, bw, &bw);
    s.l[1] = ws_subb(r.l[1], P::P1, bw, &bw);
    s.l[2] = ws_subb(r.l[2], P::P2, bw, &bw);
    s.l[3] = ws_subb(r.l[3], P::P3, bw, &bw);
    return bw ? r : s;
}
#endif

// ---- square roots for a modulus p = 3 (mod 4): Fq (p mod 8 = 7).  Not Fr: p = 1 (mod 4) there, and Tonelli-Shanks over a field of
// 2-adicity 28 has no user.  Replaces the reference's f1m_sqrt / f1m_isSquare (src/build_f1m.js:809-897) for Fq. ----
#ifndef WS_SQRT_WINDOW
#define WS_SQRT_WINDOW 4      // bits per window of the chain below
#endif
// a^((p-3)/4) by fixed windows over a per-lane table of the powers a^1 .. a^(2^W - 1): the exponent (p >> 2, 252 bits) is a
// compile-time constant with the same bits on every lane, so the loop over its windows never diverges, and every table index is a
// constant (the table stays in registers).  W = 4: 14 products for the table, then 248 squarings and one product per non-zero window
// below the top one (56 of 62) -- 318 products, against about 380 for the bit-by-bit ladder of inv().
// With w = a^((p-3)/4):  a w is the candidate root a^((p+1)/4);  a w^2 = a^((p-1)/2) = +-1 is the quadratic character, so for a != 0
// the inverse of the candidate is +-w and no root ever needs an inversion of its own (fp2.h: sqrt).
template <class F, class P>
WS_HD typename F::El ws_pow_pm3_4(const typename F::El& a) {
    static_assert((P::P0 & 3) == 3, "the chain's exponent is (p - 3) / 4: p = 3 (mod 4) only");
    typedef typename F::El El;
    constexpr int W = WS_SQRT_WINDOW, N = 1 << W;
    static_assert(W >= 2 && W <= 4, "window of 2, 3 or 4 bits");
    constexpr int kBits = 252, kWindows = (kBits + W - 1) / W;
    const uint64_t e[4] = {(P::P0 >> 2) | (P::P1 << 62), (P::P1 >> 2) | (P::P2 << 62), (P::P2 >> 2) | (P::P3 << 62), P::P3 >> 2};
    El t[N];
    t[1] = a;
#pragma unroll
    for (int k = 2; k < N; k++) t[k] = (k & 1) ? F::mul(t[k - 1], a) : F::sqr(t[k / 2]);
    El acc = F::one();
#pragma unroll 1
    for (int j = kWindows - 1; j >= 0; j--) {
        const int o = j * W;
        uint32_t d = (uint32_t)(e[o >> 6] >> (o & 63));
        if ((o & 63) + W > 64 && (o >> 6) < 3) d |= (uint32_t)(e[(o >> 6) + 1] << (64 - (o & 63)));
        d &= (uint32_t)(N - 1);
        if (j != kWindows - 1) {
#pragma unroll
            for (int k = 0; k < W; k++) acc = F::sqr(acc);
        }
        if (d == 0) continue;
        El m = t[1];
        switch (d) {      // (a branch on a value every lane shares: the index of each table read is a constant)
#define WS_SQRT_CASE(k) case k: m = t[(k) < N ? (k) : 1]; break;
            WS_SQRT_CASE(2) WS_SQRT_CASE(3) WS_SQRT_CASE(4) WS_SQRT_CASE(5) WS_SQRT_CASE(6) WS_SQRT_CASE(7) WS_SQRT_CASE(8)
            WS_SQRT_CASE(9) WS_SQRT_CASE(10) WS_SQRT_CASE(11) WS_SQRT_CASE(12) WS_SQRT_CASE(13) WS_SQRT_CASE(14) WS_SQRT_CASE(15)
#undef WS_SQRT_CASE
            default: break;
        }
        acc = (j == kWindows - 1) ? m : F::mul(acc, m);
    }
    return acc;
}
// plain value v (canonical, NOT Montgomery) > (p - 1) / 2: the "larger" of the two roots v, p - v
template <class P>
WS_HD bool ws_gt_half(const Fe& v) {
    const uint64_t h[4] = {(P::P0 >> 1) | (P::P1 << 63), (P::P1 >> 1) | (P::P2 << 63), (P::P2 >> 1) | (P::P3 << 63), P::P3 >> 1};   // (p - 1) / 2
    for (int i = 3; i >= 0; i--) {
        if (v.l[i] > h[i]) return true;
        if (v.l[i] < h[i]) return false;
    }
    return false;
}

template <class P>
struct Field {
    typedef Fe El;
    typedef Fe Packed;                             // global-memory form == register form here
    static constexpr bool kInternalDomain = false;
    static constexpr bool kHasSqrt = (P::P0 & 3) == 3;      // sqrt / is_square below: p = 3 (mod 4), Fq
    WS_HD static Fe unpack(const Fe& x) { return x; }
    WS_HD static Fe pack(const Fe& x) { return x; }
    WS_HD static Fe to_internal(const Fe& x) { return x; }
    WS_HD static Fe from_internal(const Fe& x) { return x; }
    WS_HD static Fe canonical(const Fe& x) { return x; }
    WS_HD static Fe zero() { return Fe{{0, 0, 0, 0}}; }
    WS_HD static Fe one() { return Fe{{P::R0, P::R1, P::R2_, P::R3}}; }   // Montgomery 1
    WS_HD static Fe rsq() { return Fe{{P::RR0, P::RR1, P::RR2, P::RR3}}; }
    WS_HD static Fe modulus() { return Fe{{P::P0, P::P1, P::P2, P::P3}}; }

    WS_HD static bool is_zero(const Fe& a) { return (a.l[0] | a.l[1] | a.l[2] | a.l[3]) == 0; }
    WS_HD static bool eq(const Fe& a, const Fe& b) {
        return ((a.l[0] ^ b.l[0]) | (a.l[1] ^ b.l[1]) | (a.l[2] ^ b.l[2]) | (a.l[3] ^ b.l[3])) == 0;
    }

    // t - p if t >= p (t < 2p assumed)
    WS_HD static Fe reduce_once(const Fe& t) {
        uint64_t bw = 0;
        Fe s;
        s.l[0] = ws_subb(t.l[0], P::P0, bw, &bw);
        s.l[1] = ws_subb(t.l[1], P::P1, bw, &bw);
        s.l[2] = ws_subb(t.l[2], P::P2, bw, &bw);
        s.l[3] = ws_subb(t.l[3], P::P3, bw, &bw);
        Fe r;
        r.l[0] = bw ? t.l[0] : s.l[0];
        r.l[1] = bw ? t.l[1] : s.l[1];
        r.l[2] = bw ? t.l[2] : s.l[2];
        r.l[3] = bw ? t.l[3] : s.l[3];
        return r;
    }

    // build_f1m.js:67-84 (p < 2^254, so a+b never carries out of 256 bits)
    WS_HD static Fe add(const Fe& a, const Fe& b) {
        uint64_t c = 0;
        Fe t;
        t.l[0] = ws_addc(a.l[0], b.l[0], c, &c);
        t.l[1] = ws_addc(a.l[1], b.l[1], c, &c);
        t.l[2] = ws_addc(a.l[2], b.l[2], c, &c);
        t.l[3] = ws_addc(a.l[3], b.l[3], c, &c);
        return reduce_once(t);
    }
    WS_HD static Fe dbl(const Fe& a) { return add(a, a); }
    WS_HD static Fe add_lazy(const Fe& a, const Fe& b) { return add(a, b); }   // (no lazy form for the saturated limbs)
    static constexpr bool kHasMul2Add = false;
    WS_HD static Fe sub_weak(const Fe& a, const Fe& b) { return sub(a, b); }
    WS_HD static bool is_zero_weak(const Fe& a) { return is_zero(a); }
    WS_HD static Fe mulsub2(const Fe& a, const Fe& b, const Fe& c, const Fe& d) { return sub(mul(a, b), mul(c, d)); }
    WS_HD static Fe mul_inl(const Fe& a, const Fe& b) { return mul(a, b); }
    // (the "wide" forms of the radix-2^29 field, field29.h: strict here)
    WS_HD static Fe x3_wide(const Fe& rr, const Fe& ppp, const Fe& q) { return sub(sub(rr, ppp), dbl(q)); }
    WS_HD static Fe sub_wide(const Fe& a, const Fe& b) { return sub(a, b); }
    WS_HD static bool is_zero_wide(const Fe& a) { return is_zero(a); }
    WS_HD static Fe narrow(const Fe& a) { return a; }
    // the accumulation loop's cheap tests (curve.h: madd_fast; field29.h has the forms that matter): "may be zero" must hold for every
    // zero, "packed_is_zero" is is_zero on the stored form
    WS_HD static bool maybe_zero_wide(const Fe& a) { return is_zero(a); }
    WS_HD static bool maybe_zero_weak(const Fe& a) { return is_zero(a); }
    WS_HD static bool packed_is_zero(const Fe& a) { return is_zero(a); }
    WS_HD static void keep(Fe&) {}
    WS_HD static Fe sub_weak4(const Fe& a, const Fe& b) { return sub(a, b); }
    // (the lazily reduced butterfly sums of field29.h: strict here)
    WS_HD static Fe add_nr(const Fe& a, const Fe& b) { return add(a, b); }
    WS_HD static Fe sub_weak8(const Fe& a, const Fe& b) { return sub(a, b); }
    WS_HD static Fe fold8(const Fe& a) { return a; }
    WS_HD static Fe fold16(const Fe& a) { return a; }
    WS_HD static Fe fold4to2(const Fe& a) { return a; }
    WS_HD static Fe neg_weak(const Fe& a) { return neg(a); }
    WS_HD static Fe neg_weak4(const Fe& a) { return neg(a); }

    // build_f1m.js:86-100
    WS_HD static Fe sub(const Fe& a, const Fe& b) {
        uint64_t bw = 0;
        Fe t;
        t.l[0] = ws_subb(a.l[0], b.l[0], bw, &bw);
        t.l[1] = ws_subb(a.l[1], b.l[1], bw, &bw);
        t.l[2] = ws_subb(a.l[2], b.l[2], bw, &bw);
        t.l[3] = ws_subb(a.l[3], b.l[3], bw, &bw);
        uint64_t m = (uint64_t)0 - bw;   // all ones if borrowed
        uint64_t c = 0;
        Fe r;
        r.l[0] = ws_addc(t.l[0], P::P0 & m, c, &c);
        r.l[1] = ws_addc(t.l[1], P::P1 & m, c, &c);
        r.l[2] = ws_addc(t.l[2], P::P2 & m, c, &c);
        r.l[3] = ws_addc(t.l[3], P::P3 & m, c, &c);
        return r;
    }
    // build_f1m.js:102-113
    WS_HD static Fe neg(const Fe& a) {
        uint64_t bw = 0;
        Fe t;
        t.l[0] = ws_subb(P::P0, a.l[0], bw, &bw);
        t.l[1] = ws_subb(P::P1, a.l[1], bw, &bw);
        t.l[2] = ws_subb(P::P2, a.l[2], bw, &bw);
        t.l[3] = ws_subb(P::P3, a.l[3], bw, &bw);
        uint64_t nz = is_zero(a) ? 0 : ~(uint64_t)0;
        t.l[0] &= nz; t.l[1] &= nz; t.l[2] &= nz; t.l[3] &= nz;
        return t;
    }
    // conditional negate (sign != 0 -> -a)
    WS_HD static Fe cneg(const Fe& a, bool sign) { return sign ? neg(a) : a; }

    // Montgomery product a*b*2^-256 mod p, canonical (build_f1m.js:235-436).
    WS_HD static Fe mul(const Fe& a, const Fe& b) {
#if WS_MUL32
        return mont_mul32<P>(a, b);
#else
        const uint64_t p[4] = {P::P0, P::P1, P::P2, P::P3};
        uint64_t t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
        for (int i = 0; i < 4; i++) {
            unsigned __int128 c;
            c = (unsigned __int128)a.l[0] * b.l[i] + t0; t0 = (uint64_t)c; c >>= 64;
            c += (unsigned __int128)a.l[1] * b.l[i] + t1; t1 = (uint64_t)c; c >>= 64;
            c += (unsigned __int128)a.l[2] * b.l[i] + t2; t2 = (uint64_t)c; c >>= 64;
            c += (unsigned __int128)a.l[3] * b.l[i] + t3; t3 = (uint64_t)c; c >>= 64;
            uint64_t t5 = (uint64_t)c + t4;
            uint64_t m = t0 * P::NP;
            c = (unsigned __int128)m * p[0] + t0; c >>= 64;
            c += (unsigned __int128)m * p[1] + t1; t0 = (uint64_t)c; c >>= 64;
            c += (unsigned __int128)m * p[2] + t2; t1 = (uint64_t)c; c >>= 64;
            c += (unsigned __int128)m * p[3] + t3; t2 = (uint64_t)c; c >>= 64;
            c += t5; t3 = (uint64_t)c; t4 = (uint64_t)(c >> 64);
        }
        return reduce_once(Fe{{t0, t1, t2, t3}});
#endif
    }
    WS_HD static Fe sqr(const Fe& a) { return mul(a, a); }   // build_f1m.js:439-736

    WS_HD static Fe to_mont(const Fe& a) { return mul(a, rsq()); }              // build_f1m.js:749-759
    WS_HD static Fe from_mont(const Fe& a) { return mul(a, Fe{{1, 0, 0, 0}}); } // build_f1m.js:761-770

    // a^(p-2): unique inverse, equal to the reference's ext-Euclid result (build_f1m.js:772-782)
    WS_HD static Fe inv(const Fe& a) {
        const uint64_t e[4] = {P::P0 - 2, P::P1, P::P2, P::P3};
        Fe acc = one(), base = a;
        for (int i = 0; i < 256; i++) {
            if ((e[i >> 6] >> (i & 63)) & 1) acc = mul(acc, base);
            base = sqr(base);
        }
        return acc;
    }
    WS_HD static Fe pow_u64(const Fe& a, uint64_t e) {
        Fe acc = one(), base = a;
        while (e) {
            if (e & 1) acc = mul(acc, base);
            base = sqr(base);
            e >>= 1;
        }
        return acc;
    }
    // ---- square roots (p = 3 mod 4 only: Fq; ws_pow_pm3_4 above has the chain) ----
    WS_HD static Fe pow_pm3_4(const Fe& a) { return ws_pow_pm3_4<Field<P>, P>(a); }
    // *root = a^((p+1)/4); true iff a is a square (0 included: sqrt(0) = 0), and then *root squared is a.  Which of the two roots
    // comes out is the chain's business: callers pick by parity (the reference, build_f1m.js:871-875) or by is_larger
    WS_HD static bool sqrt(const Fe& a, Fe* root) {
        *root = mul(pow_pm3_4(a), a);
        return eq(sqr(*root), a);
    }
    WS_HD static bool is_square(const Fe& a) { Fe r; return sqrt(a, &r); }
    // the plain (non-Montgomery) canonical value, and whether it is > (p - 1) / 2
    WS_HD static Fe plain(const Fe& a) { return from_mont(a); }
    WS_HD static bool is_larger(const Fe& a) { return ws_gt_half<P>(plain(a)); }
    // a / 2: (a + p) / 2 for an odd representative
    WS_HD static Fe halve(const Fe& a) {
        const uint64_t m = (uint64_t)0 - (a.l[0] & 1);
        uint64_t c = 0;
        Fe t;
        t.l[0] = ws_addc(a.l[0], P::P0 & m, c, &c);
        t.l[1] = ws_addc(a.l[1], P::P1 & m, c, &c);
        t.l[2] = ws_addc(a.l[2], P::P2 & m, c, &c);
        t.l[3] = ws_addc(a.l[3], P::P3 & m, c, &c);      // (p < 2^254: no carry out)
        return Fe{{(t.l[0] >> 1) | (t.l[1] << 63), (t.l[1] >> 1) | (t.l[2] << 63), (t.l[2] >> 1) | (t.l[3] << 63), t.l[3] >> 1}};
    }

    // reduce an arbitrary 256-bit integer mod p (plain domain): 2^256 / p < 6
    WS_HD static Fe reduce_full(const Fe& a) {
        Fe t = a;
        for (int k = 0; k < 6; k++) {
            uint64_t bw = 0;
            Fe s;
            s.l[0] = ws_subb(t.l[0], P::P0, bw, &bw);
            s.l[1] = ws_subb(t.l[1], P::P1, bw, &bw);
            s.l[2] = ws_subb(t.l[2], P::P2, bw, &bw);
            s.l[3] = ws_subb(t.l[3], P::P3, bw, &bw);
            if (!bw) t = s;
        }
        return t;
    }
};

typedef Field<FqParams> Fq;
typedef Field<FrParams> Fr;

}  // namespace wsnark
