// g2_points_bn254.hpp -- the arithmetic of decoding and validating BN254 G2 points, __host__ __device__ like the field and group headers it builds
// on: the Fq2 square root with arkworks' sign rule, the curve equation of the twist, psi, and the subgroup test [r]P = O.  The kernels are in
// msm_kernels_g2_points.hpp; tools/g2_points_check.cpp runs the same functions on the CPU with every limb-range assumption asserted
// (-DFP_BOUNDS_CHECK), against the Python law (tests/test_g2_points_cpu.py).
//
// The square root (p = 3 mod 4) works on the norm, in Fq, with TWO Fq exponentiations and no inversion -- a third of the multiplications of the
// two Fq2 exponentiations of the "complex" method, and a window table of 7 Fq entries (63 registers) instead of 7 Fq2 entries (126):
//   a = a0 + a1 u,  N = a0^2 + a1^2 (a is a square of Fq2 <=> N is one of Fq),  s = N^((p+1)/4), checked: s^2 == N
//   d = (a0 + s) / 2  (d = 0 only when a1 = 0: then d = (a0 - s) / 2 = a0),     t = d^((p-3)/4),  w = d t,  h = a1 t / 2
//   w^2 == d  (d a square: t^2 = 1/d)    : y = w + h u        since y0^2 = d, 2 y0 y1 = a1 and then y0^2 - y1^2 = a0 follows from d (d - a0) = a1^2 / 4
//   otherwise (t^2 = -1/d, w^2 = -d)     : y = h - w u        the root built on the other d' = (a0 - s) / 2 = -a1^2 / (4 d): sqrt(d') = a1 t / 2
//   y^2 == a is then verified exactly on canonical values whatever branch produced y, and the sign picked by ark-ff 0.4's order of Fq2.
// Both exponents are constants: the 3-bit windows and their branches are wave-uniform (k_decompress's scheme).
//
// The subgroup test is the relation [x+1]P + psi([x]P) + psi^2([x]P) = psi^3([2x]P) (x the BN parameter, 63 bits of weight 28), which on the twist
// holds exactly for the points of order r: 62 doublings and 27 mixed additions for [x]P, then a doubling, a mixed and three additions, all with the COMPLETE
// XYZZ formulas of ec_g2_bn254.hpp -- the inputs are adversarial (small-order points, points whose multiples meet) -- and decided projectively.
// psi acts on an XYZZ record coordinate-wise: x = X / ZZ, y = Y / ZZZ and conjugation is a ring map, so psi(X, Y, ZZ, ZZZ) =
// (conj(X) PSI_X, conj(Y) PSI_Y, conj(ZZ), conj(ZZZ)); the identity (ZZ exactly zero) is passed through untouched.
//
// Value bounds (multiples of p per component, k = 0.0059; the product rules are those of fp2_bn254.hpp) are written at each call.
#pragma once
#include "ec_g2_bn254.hpp"

namespace bn254 {

#include "g2_points_constants.inc"

// packed words < p ?
FP_HD bool words_lt_p(const uint32_t w[8]) {
    bool lt = false;
#pragma unroll
    for (int k = 7; k >= 0; k--) {
        if (w[k] != G2P_PW[k]) {
            lt = w[k] < G2P_PW[k];
            break;
        }
    }
    return lt;
}
// packed standard-form words > (p-1)/2 ?  (v > p - v; 0 is not)
FP_HD bool words_gt_half(const uint32_t w[8]) {
    bool gt = false;
#pragma unroll
    for (int k = 7; k >= 0; k--) {
        if (w[k] != G2P_HALF[k]) {
            gt = w[k] > G2P_HALF[k];
            break;
        }
    }
    return gt;
}
// a == b (mod p), any normalised operands (< 128p): one multiplication by one each, then canonical limbs
FP_HD bool fp_equal(const fp& a, const fp& b) {
    const fp ca = fp_canonical(a), cb = fp_canonical(b);
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) d |= ca.v[i] ^ cb.v[i];
    return d == 0;
}

// a^e in Fq for a constant 252-bit exponent whose top 3-bit window is not zero (both exponents here: asserted by the generator).  a normalised, < 5p;
// result < 1.1p.  Fixed 3-bit windows, most significant first: a^1 .. a^7 in registers, three squarings per window and one multiplication unless
// the window is zero.  The window value is a constant of the exponent: wave-uniform.
FP_HD fp fp_pow_const252(const fp& a, const uint32_t (&EXP)[8]) {
    fp tab[7];
    tab[0] = a;                                // < 5
    tab[1] = fp_sqr(tab[0]);                   // 25k + 1 < 1.15
    tab[2] = fp_mul(tab[1], tab[0]);           // < 1.04
    tab[3] = fp_sqr(tab[1]);                   // < 1.01
    tab[4] = fp_mul(tab[3], tab[0]);           // < 1.03
    tab[5] = fp_sqr(tab[2]);                   // < 1.01
    tab[6] = fp_mul(tab[5], tab[0]);           // < 1.03
    auto window = [&](int k) -> uint32_t {  // bits [3k, 3k+3) of the exponent
        const int b = 3 * k, i = b >> 5;
        const uint64_t lo = EXP[i], hi = i < 7 ? EXP[i + 1] : 0u;
        return (uint32_t)(((hi << 32) | lo) >> (b & 31)) & 7u;
    };
    // y * tab[d - 1], d in 1..7 and uniform: a switch over seven call sites.  (Selecting the entry first -- k_decompress's form -- is turned into an
    // indexed read of tab by the compiler, which puts the table into scratch memory: 256 bytes per lane.)
    auto times_entry = [&](const fp& y, uint32_t d) {
        switch (d) {
            case 1: return fp_mul(y, tab[0]);
            case 2: return fp_mul(y, tab[1]);
            case 3: return fp_mul(y, tab[2]);
            case 4: return fp_mul(y, tab[3]);
            case 5: return fp_mul(y, tab[4]);
            case 6: return fp_mul(y, tab[5]);
            default: return fp_mul(y, tab[6]);
        }
    };
    fp y = times_entry(fp_one(), window(83));                         // the top window is not zero
#pragma unroll 1
    for (int k = 82; k >= 0; k--) {
        y = fp_sqr(fp_sqr(fp_sqr(y)));                                // (5^2 k + 1 at the first step, then) < 1.01
        const uint32_t d = window(k);
        if (d) y = times_entry(y, d);                                 // 1.01 * 5k + 1 < 1.03
    }
    return y;
}

// Square root of a in Fq2 with the sign asked for (want_larger: the root that is the larger of (y, -y) in ark-ff 0.4's order -- c1 first, then c0,
// as standard-form integers; 0 is never larger).  a: components normalised, < 4p.  Returns false when a is not a square; y then is unspecified.
// y: components canonical (internal domain).
FP_HD bool g2_sqrt_signed(const fp2& a, bool want_larger, fp2& y) {
    const fp nrm = fp_add(fp_sqr(a.c0), fp_sqr(a.c1));               // 2 (16k + 1) < 2.2
    const fp s = fp_pow_const252(nrm, G2P_EXP_ROOT);                  // < 1.1
    if (!fp_equal(fp_sqr(s), nrm)) return false;                      // N no square of Fq <=> a no square of Fq2
    const fp inv2 = fp_const(G2P_INV2);
    fp d = fp_mul(fp_add(a.c0, s), inv2);                             // 5.1 * 1k + 1 < 1.04
    if (fp_is_zero_lt2p(d)) d = fp_mul(fp_sub<3>(a.c0, s), inv2);     // s < 2p;  a0 + 3p - s < 7;  < 1.05   (a1 = 0, s = -a0: the other d is a0)
    const fp t = fp_pow_const252(d, G2P_EXP_T);                       // < 1.1
    const fp w = fp_mul(d, t);                                        // < 1.01
    const fp h = fp_mul(fp_mul(a.c1, t), inv2);                       // 4 * 1.1k + 1 < 1.03, then < 1.01
    fp2 r;
    if (fp_equal(fp_sqr(w), d)) r = fp2{w, h};
    else r = fp2{h, fp_neg<3>(w)};                                    // 3p - w < 3
    const fp2 r2 = fp2_sqr<5>(r);                                     // r.c1 <= 3p;  4 * 6.1k + 1 < 1.15
    if (!fp_equal(r2.c0, a.c0) || !fp_equal(r2.c1, a.c1)) return false;  // (cannot happen for a square a: the exact check the contract asks for)
    fp c0 = fp_canonical(r.c0), c1 = fp_canonical(r.c1);
    uint32_t ws[8];
    fp_to_std(ws, c1);
    uint32_t nz = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) nz |= ws[k];
    if (!nz) fp_to_std(ws, c0);                                       // c1 = 0: c0 decides
    if (words_gt_half(ws) != want_larger) {                           // -y, component-wise: p - c, and 0 stays 0
        if (!fp_is_zero_exact(c0)) c0 = fp_reduce_lt2p(fp_neg<2>(c0));
        if (!fp_is_zero_exact(c1)) c1 = fp_reduce_lt2p(fp_neg<2>(c1));
    }
    y = fp2{c0, c1};
    return true;
}

// x^3 + b on the twist.  x components < 1.01p.  Result components < 2.1p.
FP_HD fp2 g2_rhs(const fp2& x) {
    const fp2 x2 = fp2_sqr<3>(x);                                     // x.c1 < 2p;  2.02 * 3.02k + 1 < 1.04
    const fp2 x3 = fp2_mul<3>(x2, x);                                 // x.c1 < 2p;  1.04 * 3.02k + 1 < 1.02
    return fp2_add(x3, fp2{fp_const(G2P_B_C0), fp_const(G2P_B_C1)});  // < 2.02
}

// conj(a) * c for a coordinate a with a.c1 < (K-1)p and a < Kp, c a canonical constant: components < K * 3k + 1
template <int K>
FP_HD fp2 g2_conj_mul(const fp2& a, const uint32_t (&c0)[9], const uint32_t (&c1)[9]) {
    const fp2 ca{a.c0, fp_normalize(fp_neg_raw_k<K>(a.c1))};         // < K
    return fp2_mul<3>(ca, fp2{fp_const(c0), fp_const(c1)});          // c.c1 < 2p
}
// conj(a) for ZZ / ZZZ (< 4.2): the u component 6p - a1 goes through one multiplication by one, back below 1.04
FP_HD fp2 g2_conj_small(const fp2& a) { return fp2{a.c0, fp_mul(fp_neg_raw_k<6>(a.c1), fp_one())}; }

// psi and -psi of an XYZZ record within the bounds of ec_g2_bn254.hpp (X < 12, Y < 8, ZZ, ZZZ < 4.2); the results are within them as well.
// The identity (ZZ exactly zero) stays the exact identity.
template <bool NEG>
FP_HD xyzz2 g2_psi(const xyzz2& p) {
    if (xyzz2_is_identity(p)) return p;
    return xyzz2{g2_conj_mul<13>(p.x, G2P_PSI_X_C0, G2P_PSI_X_C1),                                   // 13 * 3k + 1 < 1.24
                 NEG ? g2_conj_mul<9>(p.y, G2P_NPSI_Y_C0, G2P_NPSI_Y_C1) : g2_conj_mul<9>(p.y, G2P_PSI_Y_C0, G2P_PSI_Y_C1),  // 9 * 3k + 1 < 1.16
                 g2_conj_small(p.zz), g2_conj_small(p.zzz)};
}

// The same value, opaque to the optimiser (no instruction is emitted).  The mixed additions of the loops below all add the SAME point; left visible,
// that loop invariance makes the compiler hoist and interleave the addition's arithmetic on it -- the doubling of its cold same-point path first
// of all -- until the kernel spills to scratch memory (tens of KB per lane with the compiler this was written against); with the operand
// redefined in front of each addition the kernels need none.  tests/test_g2_points_cpu.py asserts that from the compiler's resource remarks;
// the register counts are in DESIGN.md section 9b.
FP_HD affine2 g2p_opaque(const affine2& p) {
    affine2 q = p;
#if defined(__HIP_DEVICE_COMPILE__)
    fp* c[4] = {&q.x.c0, &q.x.c1, &q.y.c0, &q.y.c1};
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int i = 0; i < 9; i++) asm volatile("" : "+v"(c[k]->v[i]));
#endif
    return q;
}

// [r]P == O for a point P ON THE TWIST (checked by the caller), not the identity; p within the affine bounds (x, y canonical).
// Shared by k_g2_decompress<true> and k_g2_validate.  The scalar is a constant: the double-and-add branch is wave-uniform.
// psi is a homomorphism, so the relation's three psi terms are evaluated as psi(xP + psi(xP - psi([2x]P))): two points live at a time.
FP_HD bool g2_in_subgroup(const affine2& p) {
    xyzz2 xp{p.x, p.y, fp2_one(), fp2_one()};
#pragma unroll 1
    for (int b = 61; b >= 0; b--) {  // bit 62 is the top one
        xp = xyzz2_dbl(xp);
        if ((G2P_X >> b) & 1ull) xyzz2_madd(xp, g2p_opaque(p));
    }
    xyzz2 t = g2_psi<true>(xyzz2_dbl(xp));           // -psi([2x]P)
#pragma unroll 1
    for (int j = 0; j < 3; j++) {
        if (j == 2) xyzz2_madd(xp, g2p_opaque(p));    // [x + 1]P
        t = xyzz2_add(xp, t);
        if (j < 2) t = g2_psi<false>(t);
    }
    return xyzz2_is_identity(t);                      // (the complete formulas write the identity as an exact zero ZZ)
}

}  // namespace bn254
