// ec_g2_bn254.hpp -- BN254 G2 (the sextic twist y^2 = x^3 + 3/(9+u) over Fq2) group law for gfx950: the formulas of ec_bn254.hpp over fp2.
//
// Same family as G1 (EFD shortw/xyzz, a = 0: madd-2008-s, add-2008-s, dbl-2008-s-1); the twist's b never enters an addition or a doubling.
// Identity: ZZ == 0 (both components exactly zero; an all-zero record is the identity too).  Complete: P + P, P + (-P) and identity operands are
// decided projectively.  P == 0 (same x) is read off ZZ3 = ZZ1 * PP, a product of bound < 2p that is zero exactly when PP, i.e. P, is (ZZ1 != 0);
// R == 0 is only tested on that cold path.
//
// Value bounds (multiples of p per component; fp2_bn254.hpp gives the product rules; k = 0.0059):
//   affine operand   x < 1 (canonical), y <= 2 (y or the negation 2p - y: exactly 2p for a zero component of y, which fp2_neg<2> does not reduce)
//   XYZZ everywhere  X < 12, Y < 8, ZZ < 4.2, ZZZ < 4.2  -- every function below re-establishes these
// Every fp2_mul<K>(a, b) needs b.c1 < (K-1)p, every fp2_sub<K>(a, b) b < (K-1)p; the bounds are written at each call.  (The rule is sufficient, not
// tight: a K*p pad takes a subtrahend limb by limb up to about K*p - 2^232, so only an operand within 3e-7 p of the top of its range can tell a pad
// that is one p too small -- tools/g2_bounds_check.cpp puts operands there.)
#pragma once
#include "fp2_bn254.hpp"

namespace bn254 {

struct affine2 {  // internal Montgomery domain per component; infinity is carried out of band
    fp2 x, y;
};
struct xyzz2 {
    fp2 x, y, zz, zzz;
};

FP_HD xyzz2 xyzz2_identity() { return xyzz2{fp2_one(), fp2_one(), fp2_zero(), fp2_zero()}; }
FP_HD bool xyzz2_is_identity(const xyzz2& p) { return fp2_is_zero_exact(p.zz); }

// 2P, dbl-2008-s-1 (a = 0).  Input within the XYZZ bounds (or an affine point with ZZ = ZZZ = 1).  (y != 0 on G2: no 2-torsion)
FP_HD xyzz2 xyzz2_dbl(const xyzz2& p) {
    if (xyzz2_is_identity(p)) return p;
    const fp2 u = fp2_dbl(p.y);                          // < 16
    const fp2 v = fp2_sqr<17>(u);                        // 32 * 33k + 1 < 7.3
    const fp2 w = fp2_mul<17>(v, u);                     // 7.3 * 33k + 1 < 2.5
    const fp2 s = fp2_mul<13>(v, p.x);                   // 7.3 * 25k + 1 < 2.1
    const fp2 xx = fp2_sqr<13>(p.x);                     // 24 * 25k + 1 < 4.6
    const fp2 m = fp2_add(fp2_dbl(xx), xx);              // < 13.8
    const fp2 x3 = fp2_sub<6>(fp2_sqr<15>(m), fp2_dbl(s));  // m^2 < 27.6 * 28.6k + 1 < 5.7, 2s < 4.2;  x3 < 11.6
    const fp2 y3 = fp2_sub<3>(fp2_mul<17>(m, fp2_sub<13>(s, x3)),   // s - x3 < 15.1;  m * (s - x3) < 13.8 * 31.2k + 1 < 3.6
                              fp2_mul<9>(w, p.y));                  // w * y < 2.5 * 17k + 1 < 1.3;  y3 < 6.6
    return xyzz2{x3, y3, fp2_mul<6>(v, p.zz), fp2_mul<6>(w, p.zzz)};  // 7.3 * 9.4k + 1 < 1.5, < 1.2
}

// acc += (q.x, q.y)  madd-2008-s, complete.  q within the affine bounds.
FP_HD void xyzz2_madd(xyzz2& acc, const affine2& q) {
    if (xyzz2_is_identity(acc)) {
        acc = xyzz2{q.x, q.y, fp2_one(), fp2_one()};
        return;
    }
    const fp2 u2 = fp2_mul<6>(q.x, acc.zz);       // 1 * 9.4k + 1 < 1.06
    const fp2 s2 = fp2_mul<6>(q.y, acc.zzz);      // 2 * 9.4k + 1 < 1.12
    const fp2 pp_ = fp2_sub<13>(u2, acc.x);       // P: x < 12;  P < 14.1
    const fp2 r = fp2_sub<9>(s2, acc.y);          // R: y < 8;   R < 10.2
    const fp2 pp = fp2_sqr<16>(pp_);              // 28.2 * 30.1k + 1 < 6  (c1: 2 * 14.1^2 k + 1 < 3.4)
    const fp2 zz3 = fp2_mul<7>(acc.zz, pp);       // 4.2 * 13k + 1 < 1.4  (< 2p: the zero test below is exact)
    if (fp2_is_zero_lt2p(zz3)) {                  // P == 0: same x
        if (fp2_is_zero_any(r)) acc = xyzz2_dbl(xyzz2{q.x, q.y, fp2_one(), fp2_one()});  // same point
        else acc = xyzz2_identity();                                                   // opposite points
        return;
    }
    const fp2 ppp = fp2_mul<16>(pp, pp_);         // 6 * 29.2k + 1 < 2.1
    const fp2 qv = fp2_mul<13>(pp, acc.x);        // 6 * 25k + 1 < 1.9
    const fp2 x3 = fp2_sub<7>(fp2_sqr<12>(r), fp2_add(ppp, fp2_dbl(qv)));  // r^2 < 20.3 * 22.2k + 1 < 3.7, ppp + 2 qv < 5.9;  x3 < 10.7
    const fp2 y3 = fp2_sub<3>(fp2_mul<15>(r, fp2_sub<12>(qv, x3)),         // qv - x3 < 13.9;  r * () < 10.2 * 28.8k + 1 < 2.8
                              fp2_mul<9>(ppp, acc.y));                     // 2.1 * 17k + 1 < 1.3;  y3 < 5.8
    acc.x = x3;
    acc.y = y3;
    acc.zz = zz3;
    acc.zzz = fp2_mul<4>(acc.zzz, ppp);           // 4.2 * 5.2k + 1 < 1.2
}

// a + b, add-2008-s, complete.  Both within the XYZZ bounds.
FP_HD xyzz2 xyzz2_add(const xyzz2& a, const xyzz2& b) {
    if (xyzz2_is_identity(a)) return b;
    if (xyzz2_is_identity(b)) return a;
    const fp2 u1 = fp2_mul<13>(b.zz, a.x);        // 4.2 * 25k + 1 < 1.7
    const fp2 u2 = fp2_mul<13>(a.zz, b.x);
    const fp2 s1 = fp2_mul<9>(b.zzz, a.y);        // 4.2 * 17k + 1 < 1.5
    const fp2 s2 = fp2_mul<9>(a.zzz, b.y);
    const fp2 pp_ = fp2_sub<3>(u2, u1);           // < 4.7
    const fp2 r = fp2_sub<3>(s2, s1);             // < 4.5
    const fp2 pp = fp2_sqr<6>(pp_);               // 9.4 * 10.4k + 1 < 1.6
    const fp2 zz3 = fp2_mul<3>(fp2_mul<6>(a.zz, b.zz), pp);  // zz1 zz2 < 4.2 * 9.4k + 1 < 1.3;  zz3 < 1.3 * 4.2k + 1 < 1.04
    if (fp2_is_zero_lt2p(zz3)) {
        if (fp2_is_zero_any(r)) return xyzz2_dbl(a);
        return xyzz2_identity();
    }
    const fp2 ppp = fp2_mul<6>(pp, pp_);          // 1.6 * 10.4k + 1 < 1.1
    const fp2 qv = fp2_mul<3>(pp, u1);            // 1.6 * 4.4k + 1 < 1.05
    const fp2 x3 = fp2_sub<5>(fp2_sqr<6>(r), fp2_add(ppp, fp2_dbl(qv)));  // r^2 < 9 * 10k + 1 < 1.6, ppp + 2 qv < 3.2;  x3 < 6.6
    const fp2 y3 = fp2_sub<3>(fp2_mul<10>(r, fp2_sub<8>(qv, x3)),         // x3 >= 1.8 (5p - 3.2p): qv - x3 < 1.05 + 8 - 1.8 < 7.3 (< 9: fp2_mul<10>);  r * () < 4.5 * 17.3k + 1 < 1.5
                              fp2_mul<3>(ppp, s1));                       // 1.1 * 4k + 1 < 1.03;  y3 < 4.6
    const fp2 zzz3 = fp2_mul<3>(fp2_mul<6>(a.zzz, b.zzz), ppp);          // < 1.3, then 1.3 * 3.2k + 1 < 1.03
    return xyzz2{x3, y3, zz3, zzz3};
}

}  // namespace bn254
