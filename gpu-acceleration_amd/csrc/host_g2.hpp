// host_g2.hpp -- host-side (CPU) BN254 G2 arithmetic of the PRODUCT: Fq2 = Fq[u] / (u^2 + 1) over hostg1::Fq (R = 2^256 Montgomery), Jacobian
// addition / doubling on the twist (a = 0), affine conversion and the canonical Z = 1 form.  What finishes a G2 MSM after the GPU has produced its
// bit sums (the Horner chain of host_finish.hpp) and what msm_bn254_g2_combine folds with.
//
// C-ABI word order of an Fq2 element: c0 (8 words), c1 (8 words); of a Jacobian point: X.c0 X.c1 Y.c0 Y.c1 Z.c0 Z.c1 (48 words).
#pragma once
#include "host_g1.hpp"

namespace hostg2 {

using hostg1::Fq;

struct Fq2 {
    Fq c0, c1;
};

inline Fq2 zero() { return Fq2{Fq{{0, 0, 0, 0}}, Fq{{0, 0, 0, 0}}}; }
inline Fq2 one() { return Fq2{hostg1::ONE, Fq{{0, 0, 0, 0}}}; }
inline bool is_zero(const Fq2& a) { return hostg1::is_zero(a.c0) && hostg1::is_zero(a.c1); }
inline Fq2 add(const Fq2& a, const Fq2& b) { return Fq2{hostg1::add(a.c0, b.c0), hostg1::add(a.c1, b.c1)}; }
inline Fq2 sub(const Fq2& a, const Fq2& b) { return Fq2{hostg1::sub(a.c0, b.c0), hostg1::sub(a.c1, b.c1)}; }
inline Fq2 dbl(const Fq2& a) { return add(a, a); }
inline Fq2 mul(const Fq2& a, const Fq2& b) {  // Karatsuba: three Fq products
    const Fq v0 = hostg1::mul(a.c0, b.c0), v1 = hostg1::mul(a.c1, b.c1);
    const Fq s = hostg1::mul(hostg1::add(a.c0, a.c1), hostg1::add(b.c0, b.c1));
    return Fq2{hostg1::sub(v0, v1), hostg1::sub(hostg1::sub(s, v0), v1)};
}
inline Fq2 sqr(const Fq2& a) {  // (a0 + a1)(a0 - a1) + 2 a0 a1 u
    return Fq2{hostg1::mul(hostg1::add(a.c0, a.c1), hostg1::sub(a.c0, a.c1)), hostg1::dbl(hostg1::mul(a.c0, a.c1))};
}
inline Fq2 inv(const Fq2& a) {  // (a0 - a1 u) / (a0^2 + a1^2)
    const Fq t = hostg1::inv(hostg1::add(hostg1::sqr(a.c0), hostg1::sqr(a.c1)));
    return Fq2{hostg1::mul(a.c0, t), hostg1::sub(Fq{{0, 0, 0, 0}}, hostg1::mul(a.c1, t))};
}
inline Fq2 from_mont(const Fq2& a) { return Fq2{hostg1::from_mont(a.c0), hostg1::from_mont(a.c1)}; }
inline Fq2 load_words(const uint32_t* w) { return Fq2{hostg1::load_words(w), hostg1::load_words(w + 8)}; }
inline void store_words(uint32_t* w, const Fq2& a) {
    hostg1::store_words(w, a.c0);
    hostg1::store_words(w + 8, a.c1);
}

// Jacobian point on the twist, identity <=> Z == 0 (written as (1, 1, 0), as the G1 side writes (R, R, 0))
struct Jac {
    Fq2 x, y, z;
};
inline Jac identity() { return Jac{one(), one(), zero()}; }
inline bool is_identity(const Jac& p) { return is_zero(p.z); }

inline Jac jdbl(const Jac& p) {  // dbl-2009-l
    if (is_identity(p)) return p;
    const Fq2 a = sqr(p.x), b = sqr(p.y), c = sqr(b);
    const Fq2 d = dbl(sub(sub(sqr(add(p.x, b)), a), c));
    const Fq2 e = add(dbl(a), a);
    const Fq2 f = sqr(e);
    const Fq2 x3 = sub(f, dbl(d));
    const Fq2 c8 = dbl(dbl(dbl(c)));
    const Fq2 y3 = sub(mul(e, sub(d, x3)), c8);
    const Fq2 z3 = dbl(mul(p.y, p.z));
    return Jac{x3, y3, z3};
}
inline Jac jadd(const Jac& p, const Jac& q) {  // add-2007-bl, complete
    if (is_identity(p)) return q;
    if (is_identity(q)) return p;
    const Fq2 z1z1 = sqr(p.z), z2z2 = sqr(q.z);
    const Fq2 u1 = mul(p.x, z2z2), u2 = mul(q.x, z1z1);
    const Fq2 s1 = mul(mul(p.y, q.z), z2z2), s2 = mul(mul(q.y, p.z), z1z1);
    const Fq2 h = sub(u2, u1), rr = sub(s2, s1);
    if (is_zero(h)) return is_zero(rr) ? jdbl(p) : identity();
    const Fq2 i = sqr(dbl(h));
    const Fq2 j = mul(h, i);
    const Fq2 r = dbl(rr);
    const Fq2 v = mul(u1, i);
    const Fq2 x3 = sub(sub(sqr(r), j), dbl(v));
    const Fq2 y3 = sub(mul(r, sub(v, x3)), dbl(mul(s1, j)));
    const Fq2 z3 = dbl(mul(mul(p.z, q.z), h));
    return Jac{x3, y3, z3};
}
// the Z = 1 representative (Montgomery words); p must not be the identity
inline Jac normalize(const Jac& p) {
    const Fq2 zi = inv(p.z), zi2 = sqr(zi);
    return Jac{mul(p.x, zi2), mul(p.y, mul(zi2, zi)), one()};
}
// canonical affine, standard form; returns true for the identity (x = y = 0)
inline bool to_affine_std(const Jac& p, Fq2& x, Fq2& y) {
    if (is_identity(p)) {
        x = zero();
        y = zero();
        return true;
    }
    const Jac a = normalize(p);
    x = from_mont(a.x);
    y = from_mont(a.y);
    return false;
}
inline Jac load_jac(const uint32_t* w) { return Jac{load_words(w), load_words(w + 16), load_words(w + 32)}; }
inline void store_jac(uint32_t* w, const Jac& p) {
    store_words(w, p.x);
    store_words(w + 16, p.y);
    store_words(w + 32, p.z);
}

// 64-byte image of ark-serialize 0.4 G2Affine::serialize_compressed (msm_bn254_g2_compress): x.c0 | x.c1, 32 bytes each, little-endian standard
// form; byte 63 bit 7 = y is the larger of (y, -y), bit 6 = the point at infinity (then everything else is zero).  ark-ff 0.4 orders a quadratic
// extension by c1 first, then c0, each as a standard-form integer: y > -y <=> y.c1 > (p-1)/2, or y.c1 == 0 and y.c0 > (p-1)/2 (0 is not larger).
// xy: 32 words x.c0 x.c1 y.c0 y.c1 (mont: R = 2^256 Montgomery words, else standard form).
inline void compress_point(const uint32_t* xy, bool mont, bool infinity, uint8_t out[64]) {
    static constexpr uint64_t HALF[4] = {0x9e10460b6c3e7ea3ULL, 0xcbc0b548b438e546ULL, 0xdc2822db40c0ac2eULL, 0x183227397098d014ULL};  // (p-1)/2
    uint32_t w[16] = {};
    if (infinity) {
        w[15] = 1u << 30;
    } else {
        Fq2 x = load_words(xy), y = load_words(xy + 16);
        if (mont) x = from_mont(x), y = from_mont(y);
        store_words(w, x);
        const Fq& key = hostg1::is_zero(y.c1) ? y.c0 : y.c1;
        bool larger = false;
        for (int k = 3; k >= 0; k--)
            if (key.l[k] != HALF[k]) {
                larger = key.l[k] > HALF[k];
                break;
            }
        if (larger) w[15] |= 1u << 31;
    }
    std::memcpy(out, w, 64);
}

}  // namespace hostg2

// The G2 counterpart of HostG1 (host_g1.hpp)
struct HostG2 {
    using Jac = hostg2::Jac;
    using F = hostg2::Fq2;
    static constexpr size_t JAC_WORDS = 48;  // X, Y, Z, each c0 c1
    static constexpr size_t AFF_WORDS = 32;  // x, y
    static Jac identity() { return hostg2::identity(); }
    static bool is_identity(const Jac& p) { return hostg2::is_identity(p); }
    static Jac jdbl(const Jac& p) { return hostg2::jdbl(p); }
    static Jac jadd(const Jac& p, const Jac& q) { return hostg2::jadd(p, q); }
    static Jac normalize(const Jac& p) { return hostg2::normalize(p); }
    static bool to_affine_std(const Jac& p, F& x, F& y) { return hostg2::to_affine_std(p, x, y); }
    static F from_mont(const F& a) { return hostg2::from_mont(a); }
    static Jac load_jac(const uint32_t* w) { return hostg2::load_jac(w); }
    static void store_jac(uint32_t* w, const Jac& p) { hostg2::store_jac(w, p); }
    static void store_words(uint32_t* w, const F& a) { hostg2::store_words(w, a); }
};
