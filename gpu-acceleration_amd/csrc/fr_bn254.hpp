// fr_bn254.hpp -- BN254 SCALAR-field (Fr) arithmetic for gfx950 and the host: 9 limbs of 29 bits, lazily reduced, Montgomery radix
// R' = 2^261.  The shape of fp_bn254.hpp (profiles/NOTES_r1.md: a multiplication is 162 back-to-back v_mad_u64_u32 and no carry
// instruction) over the other modulus; fp_bn254.hpp itself is left alone, its macros (FP_HD, FP_ASSERT, fp_mad) are used.
//
// Two readings of nine limbs:   raw(x): the limbs spell the integer x;   rep(x) = raw(x * 2^261 mod r): the INTERNAL form.
// fr_mul(A, B) = A*B*2^-261, so rep(x) * rep(y) -> rep(xy), and raw(x) * rep(y) -> raw(xy): every conversion (standard words in, arkworks
// R = 2^256 Montgomery words in or out, 1/n, coset powers) is ONE multiplication by a constant the host prepares.
//
// Value discipline: NORMALISED = all nine limbs < 2^29 (so the value is < 2^261 ~ 169 r).
//   fr_mul     inputs normalised AND A*B < (2^261 - r) * 2^261; output normalised, value < A*B/2^261 + r.  Normalised operands alone are NOT
//              enough: the result is (A*B + m*r) / 2^261 with m up to 2^261 - 1, so (2^261 - 1)^2 gives about 169.86 r >= 2^261 (169.28 r) and
//              the top limb leaves 29 bits (asserted below; tools/fr_bounds_check.cpp holds the case).  Sufficient forms, the ones the code uses:
//              both operands < 168.78 r; or one operand <= 2^261 - r (~168.28 r: anything < 168 r, a canonical or < 2r table entry, any 256-bit
//              word < 5.3 r) and the other merely normalised.  Column bound: 9*2^58 + 9*2^58 + carry < 2^63.
//              With one operand < 2r (canonical table entries are < r) and the other < 2^261: output < 2r + r = 3r; with the other < 84r: < 2r.
//   fr_add     limb-wise + ripple; the sum must stay < 2^261 (asserted on the top limb)
//   fr_sub<K>  A + K*r - B; B normalised and B < (K-1)*r
//   fr_reduce_lt2r  canonical representative of a normalised value < 2r
// The butterflies of ntt_bn254.hpp carry their bounds in comments; -DFP_BOUNDS_CHECK (host builds: tools/ntt_check.cpp) asserts all of them.
#pragma once
#include "fp_bn254.hpp"

namespace bn254 {

#include "fr29_constants.inc"

struct fr {
    uint32_t v[9];
};

FP_HD fr fr_const(const uint32_t (&t)[9]) { return fr{{t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]}}; }
FP_HD fr fr_zero() { return fr{{0, 0, 0, 0, 0, 0, 0, 0, 0}}; }
FP_HD fr fr_one() { return fr_const(FR29_ONE); }  // rep(1)
FP_HD fr fr_raw_one() {                           // raw(1): fr_mul(rep(x), raw(1)) = raw(x)
    fr r = fr_zero();
    r.v[0] = 1;
    return r;
}
FP_HD bool fr_is_zero_exact(const fr& a) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) d |= a.v[i];
    return d == 0;
}

// carry propagation: limbs 0..7 back below 2^29 (input limbs + carry < 2^32); the value must be < 2^261
FP_HD fr fr_normalize(const fr& a) {
    fr r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        FP_ASSERT((uint64_t)a.v[i] + c < (1ull << 32), "fr normalize: limb + carry overflows 32 bits");
        uint32_t t = a.v[i] + c;
        r.v[i] = t & FP_MASK;
        c = t >> FP_LIMB_BITS;
    }
    FP_ASSERT((uint64_t)a.v[8] + c < (1ull << 29), "fr normalize: top limb leaves 29 bits (value >= 2^261)");
    r.v[8] = a.v[8] + c;
    return r;
}
FP_HD fr fr_add(const fr& a, const fr& b) {
    fr r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = a.v[i] + b.v[i];
    return fr_normalize(r);
}
// a + K*r - b.  FR29_PAD[K] spells K*r with limbs 0..7 >= 2^29 - 1 and the top limb >= that of any normalised value < (K-1)*r
template <int K>
FP_HD fr fr_sub(const fr& a, const fr& b) {
    static_assert(K >= 2 && K <= FR29_MAX_PAD, "pad multiple out of table");
    fr r;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        FP_ASSERT(b.v[i] <= FR29_PAD[K][i], "fr_sub: subtrahend limb exceeds the pad (b >= (K-1)r or not normalised)");
        r.v[i] = a.v[i] + (FR29_PAD[K][i] - b.v[i]);
    }
    return fr_normalize(r);
}

// Montgomery product a*b*2^-261 (mod r), product scanning as fp_mul: 162 multiply-adds, one shift + mask per column
FP_HD fr fr_mul(const fr& a, const fr& b) {
    uint64_t acc = 0;
    uint32_t m[9];
    fr r;
#if defined(FP_BOUNDS_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
    for (int i = 0; i < 9; i++) FP_ASSERT(a.v[i] <= FP_MASK && b.v[i] <= FP_MASK, "fr_mul: operand not normalised");
#endif
#pragma unroll
    for (int k = 0; k < 9; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) acc = fp_mad(a.v[i], b.v[k - i], acc);
#pragma unroll
        for (int i = 0; i < k; i++) acc = fp_mad(m[i], FR29_R[k - i], acc);
        m[k] = ((uint32_t)acc * FR29_INV) & FP_MASK;
        acc = fp_mad(m[k], FR29_R[0], acc);
        acc >>= FP_LIMB_BITS;
    }
#pragma unroll
    for (int k = 9; k < 17; k++) {
#pragma unroll
        for (int i = k - 8; i <= 8; i++) acc = fp_mad(a.v[i], b.v[k - i], acc);
#pragma unroll
        for (int i = k - 8; i <= 8; i++) acc = fp_mad(m[i], FR29_R[k - i], acc);
        r.v[k - 9] = (uint32_t)acc & FP_MASK;
        acc >>= FP_LIMB_BITS;
    }
    FP_ASSERT(acc < (1ull << 29), "fr_mul: result not normalised");
    r.v[8] = (uint32_t)acc;
    return r;
}

// canonical representative in [0, r) of a normalised value < 2r
FP_HD fr fr_reduce_lt2r(const fr& a) {
    fr t;
    int32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        int32_t d = (int32_t)a.v[i] - (int32_t)FR29_R[i] + borrow;
        t.v[i] = (uint32_t)d & FP_MASK;
        borrow = d >> 29;  // arithmetic: 0 or -1
    }
    fr r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = borrow ? a.v[i] : t.v[i];
#if defined(FP_BOUNDS_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
    {
        int32_t b2 = 0;  // the result is < r: r - result does not borrow ... result - r does
        for (int i = 0; i < 9; i++) b2 = ((int32_t)r.v[i] - (int32_t)FR29_R[i] + b2) >> 29;
        FP_ASSERT(b2 == -1, "fr_reduce_lt2r: input was >= 2r");
    }
#endif
    return r;
}
// same domain, value in [0, r): what is stored as 8 words (tables, the array between two passes).  Any normalised input.
FP_HD fr fr_canonical(const fr& a) { return fr_reduce_lt2r(fr_mul(a, fr_one())); }

// 8 x 32-bit words <-> 9 x 29-bit limbs (any 256-bit pattern unpacks to a normalised value < 2^256)
FP_HD fr fr_unpack(const uint32_t w[8]) {
    fr r;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int bit = 29 * i, lo = bit >> 5, sh = bit & 31;
        uint64_t two = (uint64_t)w[lo] | ((lo + 1 < 8) ? ((uint64_t)w[lo + 1] << 32) : 0ull);
        r.v[i] = (uint32_t)(two >> sh) & FP_MASK;
    }
    return r;
}
// value must be < 2^256 and normalised
FP_HD void fr_pack(uint32_t w[8], const fr& a) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int i = (32 * j) / 29, sh = 32 * j - 29 * i;
        uint64_t two = (uint64_t)a.v[i] | ((uint64_t)a.v[i + 1] << 29);
        if (i + 2 < 9) two |= (uint64_t)a.v[i + 2] << 58;
        w[j] = (uint32_t)(two >> sh);
    }
}
// plain integer words (any 256-bit pattern, read modulo r) -> rep, < 2r
FP_HD fr fr_from_std(const uint32_t w[8]) { return fr_mul(fr_unpack(w), fr_const(FR29_IN_STD)); }
// rep (normalised) -> canonical plain integer words
FP_HD void fr_to_std(uint32_t w[8], const fr& a) { fr_pack(w, fr_reduce_lt2r(fr_mul(a, fr_raw_one()))); }

// a^e for a 32-bit exponent (a: rep, normalised, < 84r; result < 2r).  e = 0 gives rep(1).
__host__ __device__ inline fr fr_pow_u32(const fr& a, uint32_t e) {
    fr acc = fr_one(), b = a;
    while (e) {
        if (e & 1u) acc = fr_mul(acc, b);
        b = fr_mul(b, b);
        e >>= 1;
    }
    return acc;
}
// a^(r-2) (Fermat); a: rep, normalised, < 84r as fr_pow_u32 (the squares fall 84r -> 42.7r -> 11.8r -> < 2r, every product has a factor < 2r);
// result < 2r; a != 0 mod r (0 gives 0)
__host__ __device__ inline fr fr_inv(const fr& a) {
    fr acc = fr_one(), b = a;
    for (int i = 0; i < 254; i++) {
        if ((FR_EXP_RM2[i >> 5] >> (i & 31)) & 1u) acc = fr_mul(acc, b);
        b = fr_mul(b, b);
    }
    return acc;
}

}  // namespace bn254
