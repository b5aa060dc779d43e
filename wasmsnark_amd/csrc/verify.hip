// verify.hip -- native Groth16 verification on the host.
//
// Replaces /root/reference src/bn128.js:722-791 (Bn128.groth16Verify) and the pairing it calls,
// bn128_pairingEq4 (src/bn128/build_bn128.js:265-1374: prepareG1/prepareG2, Miller loop, final exponentiation over the
// Fp2 / Fp6 / Fp12 tower of build_f2m.js / build_f3m.js).  Same check, same verdicts:
//     e(A, B) * e(-IC(inputs), gamma2) * e(-C, delta2) * e(-alfa1, beta2) == 1,      false if an input is >= r (:772)
// The verdict of a pairing-product equation does not depend on WHICH bilinear non-degenerate pairing on G1 x G2 is
// used, so this build does not restate the reference's optimal-ate code with its Frobenius tables.  It evaluates the
// plain ate pairing  a(Q, P) = f_{T,Q}(P)^((p^12-1)/r),  T = t - 1 = p - r  (127 bits),  with
//   * Fp12 = Fp2[w]/(w^6 - xi), xi = 9 + u (one flat degree-6 extension; w^2 = v, v^3 = xi is the reference's tower),
//   * the untwist (x', y') -> (x' w^2, y' w^3) of the D-type twist  y^2 = x^3 + 3/xi  (build_bn128.js:79-90),
//   * affine Miller steps: the line through the untwisted points evaluated at P = (xP, yP) is
//         l = yP - lambda' xP * w + (lambda' xT' - yT') * w^3                  (three non-zero coefficients)
//     where lambda' is the slope on the twist; vertical lines lie in a proper subfield and vanish in the final
//     exponentiation,
//   * ONE final exponentiation of the product of the four Miller values by plain square-and-multiply with the
//     2790-bit exponent (p^12 - 1)/r: no Frobenius constants anywhere.
// Host arithmetic (field.h / fp2.h, the same headers the proof assembly uses); ~30 ms per verification on one core.
// "Same verdict under any pairing" holds for points of G1 x G2 only: for a B on the twist but outside the order-r
// subgroup, or for off-curve coordinates, neither this map nor the reference's is bilinear and the two could disagree
// (ADVICE r2).  The reference makes no such checks (its verdict on malformed points is an accident of its Miller loop);
// here every proof and key point must satisfy its curve equation and every G2 point must be killed by r, otherwise the
// proof is INVALID (*valid = 0) before any pairing is evaluated.  Like the reference (setG1Affine / setG2Affine force
// z = 1, src/bn128.js:741-760) the z coordinates of the proof are ignored: (x, y) is the point, so the (0, 1, 0) a
// prover prints for infinity is the off-curve point (0, 1) and makes the proof invalid.
#include <string.h>

#include "../../include/wsnark.h"
#include "internal.h"
#include "fp12_host.h"

namespace wsnark {
using namespace hostpair;   // F12, the Miller loop, the point loaders and checks: fp12_host.h (moved there unchanged)

// vk: alfa1 (64 B) | beta2 (128 B) | gamma2 (128 B) | delta2 (128 B) | IC[0 .. n_inputs] (64 B each); all affine, PLAIN LE.
int groth16_verify(const uint8_t* vk, size_t vk_len, const uint8_t* inputs, uint64_t n_inputs, const uint8_t* proof384, int* valid) {
    *valid = 0;
    // (compared without the multiplication: (n_inputs + 1) * 64 wraps for n_inputs near 2^58)
    if (vk_len < 512 || n_inputs > (vk_len - 448) / 64 - 1) { set_last_error("verification key has fewer IC points than inputs + 1"); return WS_ERR_SIZE; }
    G1A alfa1, A, C;
    G2A beta2, gamma2, delta2, B;
    if (!load_g1(vk, false, &alfa1) || !load_g2(vk + 64, false, &beta2) || !load_g2(vk + 192, false, &gamma2) ||
        !load_g2(vk + 320, false, &delta2) || !load_g1(proof384, true, &A) || !load_g2(proof384 + 96, true, &B) ||
        !load_g1(proof384 + 288, true, &C)) {
        set_last_error("verify: a coordinate is not a reduced field element");
        return WS_ERR_FORMAT;
    }
    // malformed points: invalid, before anything is paired (see the header)
    if (!g1_ok(alfa1) || !g1_ok(A) || !g1_ok(C) || !g2_ok(beta2) || !g2_ok(gamma2) || !g2_ok(delta2) || !g2_ok(B)) return WS_OK;
    // IC(inputs) = IC[0] + sum input_i * IC[i+1]   (src/bn128.js:765-777; an input >= r makes the proof invalid, :772)
    G1::Pt acc = G1::infinity();
    for (uint64_t i = 0; i <= n_inputs; i++) {
        G1A ic;
        if (!load_g1(vk + 448 + i * 64, false, &ic)) { set_last_error("verify: IC coordinate not reduced"); return WS_ERR_FORMAT; }
        if (!g1_ok(ic)) return WS_OK;
        G1::Pt pt = ic.inf ? G1::infinity() : G1::Pt{ic.x, ic.y, Fq::one(), Fq::one()};
        if (i > 0) {
            Fe s;
            memcpy(&s, inputs + (i - 1) * 32, 32);
            if (!Fr::eq(Fr::reduce_full(s), s)) return WS_OK;                       // >= r: invalid, not an error
            pt = G1::mul_bytes(pt, reinterpret_cast<const uint8_t*>(&s), 32);
        }
        acc = G1::add(acc, pt);
    }
    const Jac<Fq> icj = G1::to_affine_jac(acc);
    G1A IC{icj.x, icj.y, Fq::is_zero(icj.z)};
    auto neg = [](G1A p) { p.y = Fq::neg(p.y); return p; };
    F12 f = f12_one(), m;
    const G1A Ps[4] = {A, neg(IC), neg(C), neg(alfa1)};
    const G2A Qs[4] = {B, gamma2, delta2, beta2};
    for (int k = 0; k < 4; k++) {
        if (!miller_ate(Qs[k], Ps[k], &m)) return WS_OK;      // a G2 point outside the order-r subgroup: invalid
        f = f12_mul(f, m);
    }
    *valid = f12_is_one(final_exponentiation(f)) ? 1 : 0;
    return WS_OK;
}

}  // namespace wsnark
