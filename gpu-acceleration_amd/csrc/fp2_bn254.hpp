// fp2_bn254.hpp -- Fq2 = Fq[u] / (u^2 + 1) on the lazily reduced 9 x 29-bit field of fp_bn254.hpp (BN254 G2 coordinates).
//
// Value discipline: a component is NORMALISED as in fp_bn254.hpp; its value bound is a multiple of p written next to every call (ec_g2_bn254.hpp).
//   fp2_mul<K>(a, b) : c0 = a0*b0 + a1*(K*p - b1), c1 = a0*b1 + a1*b0, each ONE fp_mul_add (one Montgomery reduction for two products).
//                      Needs b1 < (K-1)p.  Output components < A*(2B+1)*k + 1 (A, B: bounds of a, b; k = p / 2^261 = 0.0059).
//                      486 limb products -- what Karatsuba's three fp_mul cost -- but no subtraction AFTER a product: the outputs stay below
//                      ~1.5p instead of the (pad + product) of Karatsuba's v2 - v0 - v1, which would make every later pad grow.
//   fp2_sqr<K>(a)    : c0 = (a0 + a1) * (a0 + K*p - a1), c1 = (2 a0) * a1: two fp_mul (324 products).  Needs a1 < (K-1)p.
//                      Output components < 2A(2A+1)k + 1 for K = A + 1.
//   fp2_add / fp2_dbl: component-wise, value = sum.   fp2_sub<K>(a, b) = a + K*p - b, needs b < (K-1)p.
// The subtraction pads of fp_bn254.hpp stop at 12p; the G2 formulas need up to 16p, so this header spells its own pads K*p (K <= FP2_MAX_PAD)
// with limbs 0..7 >= 2^29 - 1 (a normalised subtrahend never borrows), generated at compile time from FP29_P.
#pragma once
#include "fp_bn254.hpp"

namespace bn254 {

constexpr int FP2_MAX_PAD = 18;
struct fp2_pad_table {
    uint32_t v[FP2_MAX_PAD + 1][9];
};
constexpr fp2_pad_table fp2_make_pads() {
    fp2_pad_table t{};
    for (int k = 2; k <= FP2_MAX_PAD; k++) {
        uint64_t c = 0;
        uint32_t n[9] = {};
        for (int i = 0; i < 8; i++) {
            const uint64_t s = (uint64_t)k * FP29_P[i] + c;
            n[i] = (uint32_t)(s & FP_MASK);
            c = s >> FP_LIMB_BITS;
        }
        n[8] = (uint32_t)((uint64_t)k * FP29_P[8] + c);
        t.v[k][0] = n[0] + (1u << FP_LIMB_BITS);
        for (int i = 1; i < 8; i++) t.v[k][i] = n[i] + (1u << FP_LIMB_BITS) - 1u;
        t.v[k][8] = n[8] - 1u;
    }
    return t;
}
constexpr fp2_pad_table FP2_PAD = fp2_make_pads();

struct fp2 {
    fp c0, c1;
};

FP_HD fp2 fp2_zero() { return fp2{fp_zero(), fp_zero()}; }
FP_HD fp2 fp2_one() { return fp2{fp_one(), fp_zero()}; }
FP_HD bool fp2_is_zero_exact(const fp2& a) { return fp_is_zero_exact(a.c0) && fp_is_zero_exact(a.c1); }
// a == 0 in Fq2 for components that are normalised and < 2p (outputs of fp2_mul / fp2_sqr with small operands qualify: see the bounds at the call)
FP_HD bool fp2_is_zero_lt2p(const fp2& a) { return fp_is_zero_lt2p(a.c0) && fp_is_zero_lt2p(a.c1); }
// a == 0 in Fq2 for ANY normalised components (< 128p): one multiplication by one per component brings them below 2p (cold paths only)
FP_HD bool fp2_is_zero_any(const fp2& a) { return fp_is_zero_lt2p(fp_mul(a.c0, fp_one())) && fp_is_zero_lt2p(fp_mul(a.c1, fp_one())); }

// K*p - b (limb-wise, NOT normalised: limbs 0..7 < 2^30) and a + K*p - b (normalised)
template <int K>
FP_HD fp fp_neg_raw_k(const fp& b) {
    static_assert(K >= 2 && K <= FP2_MAX_PAD, "pad multiple out of table");
    fp r;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        FP_ASSERT(b.v[i] <= FP2_PAD.v[K][i], "fp2 pad: subtrahend limb exceeds the pad (b >= (K-1)p or not normalised)");
        r.v[i] = FP2_PAD.v[K][i] - b.v[i];
    }
    return r;
}
template <int K>
FP_HD fp fp_sub_raw_k(const fp& a, const fp& b) {
    fp r = fp_neg_raw_k<K>(b);
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] += a.v[i];
    return r;
}
template <int K>
FP_HD fp fp_sub_k(const fp& a, const fp& b) { return fp_normalize(fp_sub_raw_k<K>(a, b)); }

FP_HD fp2 fp2_add(const fp2& a, const fp2& b) { return fp2{fp_add(a.c0, b.c0), fp_add(a.c1, b.c1)}; }
FP_HD fp2 fp2_dbl(const fp2& a) { return fp2{fp_dbl(a.c0), fp_dbl(a.c1)}; }
template <int K>
FP_HD fp2 fp2_sub(const fp2& a, const fp2& b) { return fp2{fp_sub_k<K>(a.c0, b.c0), fp_sub_k<K>(a.c1, b.c1)}; }
template <int K>
FP_HD fp2 fp2_neg(const fp2& b) { return fp2{fp_normalize(fp_neg_raw_k<K>(b.c0)), fp_normalize(fp_neg_raw_k<K>(b.c1))}; }

// (a0 + a1 u)(b0 + b1 u) = (a0 b0 - a1 b1) + (a0 b1 + a1 b0) u.  The raw K*p - b1 is the second factor of its product, whose first factor a1 is
// normalised: fp_bn254.hpp's RAW rule keeps the shared column accumulator below 2^64.
template <int K>
FP_HD fp2 fp2_mul(const fp2& a, const fp2& b) {
    return fp2{fp_mul_add(a.c0, b.c0, a.c1, fp_neg_raw_k<K>(b.c1)), fp_mul_add(a.c0, b.c1, a.c1, b.c0)};
}
// (a0 + a1 u)^2 = (a0 + a1)(a0 - a1) + 2 a0 a1 u   (a0 - a1 raw: one factor of an fp_mul whose other factor is normalised)
template <int K>
FP_HD fp2 fp2_sqr(const fp2& a) { return fp2{fp_mul(fp_add(a.c0, a.c1), fp_sub_raw_k<K>(a.c0, a.c1)), fp_mul(fp_dbl(a.c0), a.c1)}; }
// by an Fq element (component-wise)
FP_HD fp2 fp2_mul_fp(const fp2& a, const fp& s) { return fp2{fp_mul(a.c0, s), fp_mul(a.c1, s)}; }

}  // namespace bn254
