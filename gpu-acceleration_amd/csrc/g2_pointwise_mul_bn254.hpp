// g2_pointwise_mul_bn254.hpp -- BN254 G2 element-wise scalar multiplication, out[i] = k_i * Q_i: n different points of G2, each with a scalar
// of its own (or one scalar for all of them), n points out -- the G2 half of an UPDATE of an existing setup (the tauG2 section and betaG2 of a
// powers-of-tau contribution, deltaG2 of a phase-2 contribution, a re-randomised G2 base set).  pointwise_mul_bn254.hpp over Fq2: the per-lane
// routines, __host__ __device__ throughout: tools/g2_pointwise_mul_check.cpp runs them on the CPU with -DFP_BOUNDS_CHECK; the kernel is
// msm_kernels_g2_pointwise.hpp, the host side msm_g2_pointwise.inc.  The scalar side -- pm_scalar_canonical, pm_split, pm_split_host, PmSplit,
// pm_shl -- is the G1 call's, used as it is: on G2 phi2(x, y) = (beta^2 x, y) = lambda * (x, y) with the lambda of the G1 split
// (msm_kernels_g2.hpp; the G2 MSM relies on it).
//
// Shape.  One lane per point; the FB_GROUP lanes of a workgroup share two FIELD inversions, in Fq: 1 / z = conj(z) / N(z), N = z.c0^2 + z.c1^2
// (u^2 = -1, and -1 is no square modulo p: N != 0 for z != 0), so fixed_base_bn254.hpp's product tree inverts the 256 norms unchanged.  Per lane:
//   1. the point as canonical internal-domain components (one multiplication per component, whichever form the words have);
//   2. the scalar as the canonical integer k < r, k = k1 + lambda * k2, |k1|, |k2| < 2^126 (the G1 routines);
//   3. three affine points: P1 = (x, +-y) = sign(k1) * Q, P2 = (beta^2 x, +-y) = sign(k2) * lambda * Q, S = P1 + P2.  Only x, beta^2 x, y and S
//      are kept (five fp2 = 90 registers): y2 is +-y1, so the two sign bits of the split stand for the second and third y, and the operand's y
//      is negated on its way into the addition (fp2_neg<2> of the CANONICAL y, both components normalised: fixed_base_g2_bn254.hpp's warning).
//      The slope of S has the denominator (beta^2 - 1) x.  For a point of G2 x != 0: a point (0, y) is fixed by phi2, so (lambda - 1) Q = O,
//      and lambda != 1 mod r forces Q = O.  lambda != +-1 also gives P1 != +-P2: the plain chord formula holds.  x = 0 can only come from
//      invalid input and enters the inversion as 1, as in G1;
//   4. a joint (Shamir) ladder over the PM_LADDER_BITS = 126 positions, top down: xyzz2_dbl, then xyzz2_madd of the entry the two bits select,
//      if any (ec_g2_bn254.hpp: both complete, so there is no special case here);
//   5. the shared inversion of N(ZZZ) and canonical words out (fb2_store_output).
// The bits are read by SHIFTING the halves, the table entry is chosen by selects: no lane makes a data-dependent memory access.  The twist's
// cofactor is not 1: reading a scalar modulo r and the endomorphism are only right IN G2, so for words that are no curve point, components of
// p or above, or a twist point outside G2 a lane computes a meaningless point -- without disturbing its neighbours (x = 0 enters the first
// inversion as 1, ZZZ = 0 mod p leaves the second one flagged).
//
// Count per point, in the project's units (an fp2_mul or fp2_sqr is two field multiplications: two fp_mul_add resp. two fp_mul) and in limb
// products (fp2_mul 486, fp2_sqr 324, fp_mul 162, fp_sqr 126, as DESIGN.md 9j counts them):
//   xyzz2_dbl    3 fp2_sqr + 6 fp2_mul = 18 units, 3 888 limb products          xyzz2_madd   2 fp2_sqr + 8 fp2_mul = 20 units, 4 536
//   fixed part   4 (point) + 2 (beta^2 x) + 2 (norm) + 2 (1 / den) + 2 + 2 + 2 + 4 (l, l^2, sy, canonical S) + 2 + 2 (norm, 1 / ZZZ)
//                + 2 + 2 + 2 + 2 + 4 (t, t^2, x, y, out) + 2 * 3 (tree) = 42 units
//   126 * 18 + 126 * 20 + 42 = 4 830 units per point, 126 * 18 + 94.5 * 20 + 42 = 4 200 with one scalar (a wavefront skips the additions that no
//   lane needs); in limb products 126 * (3 888 + 4 536) = 1.06 M against G1's 126 * (8 + 9) * 162 = 0.35 M (3.06 x).
#pragma once
#include "fixed_base_g2_bn254.hpp"
#include "pointwise_mul_bn254.hpp"

namespace pmk {

// beta^2 = -beta - 1 (mod p) in standard form: the constant of msm_kernels_g2.hpp (k_g2_convert), which that header keeps in its own namespace
// next to the G2 MSM's kernels; tests/test_g2_pointwise_mul_cpu.py holds both against beta of tests/golden/glv_constants.json
constexpr uint32_t PM2_BETA2_STD[8] = {0x77fffffeu, 0x57634731u, 0xacdb5c4fu, 0xd4f263f1u, 0xa0d48bacu, 0x59e26bceu, 0x00000000u, 0x00000000u};

using Pm2Plan = PmPlan;  // == msm_pointwise_g2_plan_t: the same four words
inline Pm2Plan pm2_plan() { return Pm2Plan{FB_GROUP, PM_LADDER_BITS, PM_TABLE_POINTS, 0}; }

struct Pm2Lane {  // what a lane keeps in registers: x, beta^2 x, y (canonical: P1 = (x, +-y), P2 = (bx, +-y) by s.neg1, s.neg2), S = (sx, sy) canonical
    fp2 x, bx, y, sx, sy;
    PmSplit s;
};

// one component of a record (8 words, 16-byte aligned) as a canonical internal-domain value; c: FP29_IN_STD or FP29_IN_MONT
FP_HD fp pm2_load_component(const uint32_t* p, const fp& c) {
    return fp_reduce_lt2p(fp_mul(fb2_load_fp8(p), c));  // < 2^256 * p / 2^261 + p < 1.04
}
// the point of a record (32 words x.c0 x.c1 y.c0 y.c1; Montgomery words, standard form with bases_std): every component canonical
FP_HD affine2 pm2_load_point(const uint32_t* rec, bool bases_std) {
    const fp c = bases_std ? fp_const(FP29_IN_STD) : fp_const(FP29_IN_MONT);
    return affine2{fp2{pm2_load_component(rec, c), pm2_load_component(rec + 8, c)}, fp2{pm2_load_component(rec + 16, c), pm2_load_component(rec + 24, c)}};
}
// +-y of the canonical y: y < 1, 2p - y <= 2 with both components normalised (exactly 2p for a zero component: ec_g2_bn254.hpp's affine bound)
FP_HD fp2 pm2_signed_y(const fp2& y, uint32_t negate) {
    const fp2 ny = fp2_neg<2>(y);  // y < 1 = (2 - 1)
    fp2 r;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        r.c0.v[i] = negate ? ny.c0.v[i] : y.c0.v[i];
        r.c1.v[i] = negate ? ny.c1.v[i] : y.c1.v[i];
    }
    return r;
}
// the denominator of S's slope, beta^2 x - x: x canonical, so each component < bx + 2 < 3
FP_HD fp2 pm2_slope_den(const Pm2Lane& t) { return fp2_sub<2>(t.bx, t.x); }

// x, beta^2 x and y of the point a (canonical); returns the NORM of the denominator of S's slope, the Fq element the workgroup inverts:
// 2 * (3^2 k + 1) < 2.2 -- a leaf of the product tree: every node above it is a product of two values < 3, so < 1.06.
// x_zero: the words were no point of G2 and the denominator is 0.
FP_HD fp pm2_table_begin(Pm2Lane& t, const affine2& a, bool& x_zero) {
    const fp b2 = fp_from_std(PM2_BETA2_STD);                                            // < 1.01
    t.x = a.x;
    t.bx = fp2{fp_reduce_lt2p(fp_mul(a.x.c0, b2)), fp_reduce_lt2p(fp_mul(a.x.c1, b2))};  // 1 * 1.01k + 1 < 1.01: canonical after the reduction
    t.y = a.y;
    x_zero = fp2_is_zero_exact(a.x);
    return fb2_norm(pm2_slope_den(t));
}
// S = P1 + P2 by the chord: l = (y2 - y1) / (bx - x), sx = l^2 - x - bx, sy = l (x - sx) - y1; ni = 1 / N(bx - x), < 2
FP_HD void pm2_table_finish(Pm2Lane& t, const fp& ni) {
    const fp2 id = fb2_inv_from_norm(pm2_slope_den(t), ni);              // den < 3: 3 * 2k + 1 < 1.04 and (6p - c1 raw, c1 < 5) 6 * 2k + 1 < 1.08
    const fp2 y1 = pm2_signed_y(t.y, t.s.neg1), y2 = pm2_signed_y(t.y, t.s.neg2);  // <= 2
    const fp2 l = fp2_mul<3>(fp2_sub<4>(y2, y1), id);                    // y1 <= 2 < 3: the difference < 6;  id.c1 < 2;  6 * 3.16k + 1 < 1.12
    const fp2 x3 = fp2_sub<3>(fp2_sqr<3>(l), fp2_add(t.x, t.bx));        // l.c1 < 2: l^2 < 2.24 * 3.24k + 1 < 1.05;  x + bx < 2;  x3 < 4.05
    t.sx = fp2{fp_canonical(x3.c0), fp_canonical(x3.c1)};
    const fp2 m = fp2_mul<4>(l, fp2_sub<2>(t.x, t.sx));                  // sx < 1: x - sx < 3;  1.12 * 7k + 1 < 1.05
    const fp2 y3 = fp2_sub<4>(m, y1);                                    // y1 <= 2 < 3;  < 5.05
    t.sy = fp2{fp_canonical(y3.c0), fp_canonical(y3.c1)};
}

// the entry sel = 1 (P1), 2 (P2) or 3 (S), by selects: x canonical, y <= 2
FP_HD affine2 pm2_select(const Pm2Lane& t, uint32_t sel) {
    const fp2 ys = pm2_signed_y(t.y, sel == 1u ? t.s.neg1 : t.s.neg2);
    affine2 q;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        q.x.c0.v[i] = sel == 1u ? t.x.c0.v[i] : sel == 2u ? t.bx.c0.v[i] : t.sx.c0.v[i];
        q.x.c1.v[i] = sel == 1u ? t.x.c1.v[i] : sel == 2u ? t.bx.c1.v[i] : t.sx.c1.v[i];
        q.y.c0.v[i] = sel == 3u ? t.sy.c0.v[i] : ys.c0.v[i];
        q.y.c1.v[i] = sel == 3u ? t.sy.c1.v[i] : ys.c1.v[i];
    }
    return q;
}
// |k1| * P1 + |k2| * P2: the joint ladder over PM_LADDER_BITS positions, most significant first.  Every accumulator is within ec_g2_bn254.hpp's
// XYZZ bounds (X < 12, Y < 8, ZZ, ZZZ < 4.2): both functions re-establish them from an operand with x < 1, y <= 2.
FP_HD xyzz2 pm2_ladder(const Pm2Lane& t) {
    uint32_t k1[4] = {t.s.k1[0], t.s.k1[1], t.s.k1[2], t.s.k1[3]}, k2[4] = {t.s.k2[0], t.s.k2[1], t.s.k2[2], t.s.k2[3]};
    pm_shl(k1, 128 - PM_LADDER_BITS);  // bit 125 to the top of the fourth word
    pm_shl(k2, 128 - PM_LADDER_BITS);
    xyzz2 acc = xyzz2_identity();
#pragma nounroll
    for (uint32_t j = 0; j < PM_LADDER_BITS; j++) {
        acc = xyzz2_dbl(acc);
        const uint32_t sel = (k1[3] >> 31) | ((k2[3] >> 31) << 1);
        pm_shl(k1, 1);
        pm_shl(k2, 1);
        if (sel) xyzz2_madd(acc, pm2_select(t, sel));
    }
    return acc;
}

// ---- the phases of a lane, a shared inversion between them (k_pm2_mul of msm_kernels_g2_pointwise.hpp; tools/g2_pointwise_mul_check.cpp) ----
// phase 1: the scalar (unless the halves came with the launch: t.s is set then and `scalar` is not read), the point, x, beta^2 x, y; returns
// the norm of the slope's denominator
template <bool UNIFORM>
FP_HD fp pm2_lane_begin(Pm2Lane& t, const uint32_t* base_rec, const uint32_t* scalar, uint32_t flags, bool& x_zero) {
    if (!UNIFORM) {
        const uint4* q = reinterpret_cast<const uint4*>(scalar);
        const uint4 a = q[0], b = q[1];
        uint32_t k[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        pm_scalar_canonical(k, (flags & PM_F_IN_MONT) != 0);
        t.s = pm_split(k);
    }
    return pm2_table_begin(t, pm2_load_point(base_rec, (flags & PM_F_BASES_STD) != 0), x_zero);
}
// phase 2: S and the ladder; ni = 1 / (what phase 1 returned)
FP_HD xyzz2 pm2_lane_finish(Pm2Lane& t, const fp& ni) {
    pm2_table_finish(t, ni);
    return pm2_ladder(t);
}
// the identity, or (words that were no point) a ZZZ the shared inversion must not meet.  Every ZZ and ZZZ a ladder leaves is a product
// (xyzz2_dbl: < 1.5, xyzz2_madd: < 1.4), the literal 1 or the literal 0: below 2p, the test is exact
FP_HD bool pm2_is_identity(const xyzz2& p) { return fp2_is_zero_lt2p(p.zz) || fp2_is_zero_lt2p(p.zzz); }
// what a lane gives the second inversion: N(ZZZ) < 2.3 (fb2_norm)
FP_HD fp pm2_out_norm(const xyzz2& p) { return fb2_norm(p.zzz); }
// the output record from ni = 1 / N(ZZZ), < 2
FP_HD void pm2_store_output(uint32_t* out_xy, uint8_t* out_inf, const xyzz2& p, const fp& ni, bool identity, bool out_std) {
    fp2 iz = fp2_zero();
    if (!identity) iz = fb2_inv_from_norm(p.zzz, ni);  // ZZZ < 4.2: iz < 1.08
    fb2_store_output(out_xy, out_inf, p, iz, identity, out_std);
}

}  // namespace pmk
