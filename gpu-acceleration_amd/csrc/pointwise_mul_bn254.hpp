// pointwise_mul_bn254.hpp -- BN254 G1 element-wise scalar multiplication, out[i] = k_i * P_i: n different points, each with a scalar of its own
// (or one scalar for all of them), n points out -- what an UPDATE of an existing setup consists of (a powers-of-tau contribution, a phase-2
// contribution, a re-randomised base set).  The per-lane routines, __host__ __device__ throughout: tools/pointwise_mul_check.cpp runs them on
// the CPU with -DFP_BOUNDS_CHECK; the kernels are msm_kernels_pointwise.hpp, the host side msm_pointwise.inc.
//
// Shape.  One lane per point; the FB_GROUP lanes of a workgroup share two field inversions (fixed_base_bn254.hpp's product tree).  Per lane:
//   1. the point as canonical internal-domain coordinates (one multiplication per coordinate, whichever form the words have);
//   2. the scalar as the canonical integer k < r (one fr_mul by a constant and the final reduction, for both input forms);
//   3. k = k1 + lambda * k2, |k1|, |k2| < 2^126 (glv::split);
//   4. three affine points in registers: P1 = (x, +-y) = sign(k1) * P, P2 = (beta x, +-y) = sign(k2) * lambda * P, S = P1 + P2.  The slope of
//      S has the denominator beta x - x = (beta - 1) x, never zero for a curve point (3 is a non-residue modulo p: y^2 = 3 has no solution,
//      so no point has x = 0) -- P1 is never +-P2 and the plain chord formula holds; the denominators of a workgroup are inverted together;
//   5. a joint (Shamir) ladder over the PM_LADDER_BITS = 126 bit positions, top down: xyzz_dbl, then xyzz_madd of the entry the two bits
//      select, if any (ec_bn254.hpp: both complete, so k1 = +-k2, a half of zero and an accumulator that meets a table entry need no case);
//   6. the shared inversion of ZZZ and canonical words out (fb_store_output).
// The scalars' bits are read by SHIFTING the halves (static register indices), the table entry is chosen by selects: no lane makes a
// data-dependent memory access, and a lane whose words are no curve point computes a meaningless point without disturbing its neighbours
// (x = 0 enters the first inversion as 1, ZZZ = 0 mod p leaves the second one flagged).
//
// Count (field multiplications; a squaring counts as one, and so does a fused multiply-add, which has 1.5 times the limb products): 126
// doublings of 8 (xyzz_dbl) and up to 126 additions of 9 (xyzz_madd) -- a wavefront executes the addition whenever ANY of its lanes needs
// it, so the per-element form pays all 126 and the one-scalar form the 3/4 of them its bits ask for on average -- plus 2 (point) + 1 (beta x)
// + 4 (S) + 2 * 3 (the two inversions) + 6 (output) = 19: 2 161 per point resp. about 1 878.
#pragma once
#include "fixed_base_bn254.hpp"
#include "glv_bn254.hpp"

namespace pmk {

using namespace fbk;

constexpr uint32_t PM_LADDER_BITS = (uint32_t)glv::HALF_BITS;  // 126
constexpr uint32_t PM_TABLE_POINTS = 3;                        // P1, P2, P1 + P2
constexpr uint32_t PM_F_IN_MONT = 2u, PM_F_OUT_STD = 8u, PM_F_BASES_STD = 16u;  // == MSM_NTT_IN_MONT, MSM_FB_OUT_STD, MSM_PM_BASES_STD

struct PmPlan {  // == msm_pointwise_plan_t
    uint32_t inv_group, ladder_bits, table_points, reserved;
};
inline PmPlan pm_plan() { return PmPlan{FB_GROUP, PM_LADDER_BITS, PM_TABLE_POINTS, 0}; }

struct PmSplit {  // the halves of a scalar as sign and magnitude; a kernel argument in the one-scalar form
    uint32_t k1[4], k2[4];
    uint32_t neg1, neg2;
};
struct PmLane {  // what a lane keeps in registers: P1 = (x, y1), P2 = (bx, y2), S = (sx, sy), all affine (x canonical, y < 2), and the halves
    fp x, bx, y1, y2, sx, sy;
    PmSplit s;
};

// any 256-bit pattern -> the canonical integer below r it stands for: the words are k (read modulo r), or arkworks Fr.0 words k * 2^256 mod r.
// fr_mul(w, f) = w * f * 2^-261 with f = raw(2^261 mod r) resp. raw(2^5)
FP_HD void pm_scalar_canonical(uint32_t k[8], bool in_mont) {
    fr f = fr_one();
    if (in_mont) {
        f = fr_zero();
        f.v[0] = 32;
    }
    fr_pack(k, fr_reduce_lt2r(fr_mul(fr_unpack(k), f)));  // < 2^256 * r / 2^261 + r < 2r
}
// k < r -> the halves
FP_HD PmSplit pm_split(const uint32_t (&k)[8]) {
    PmSplit s;
    bool n1, n2;
    const bool ok = glv::split(k, s.k1, n1, s.k2, n2);
    FP_ASSERT(ok, "pointwise: a half of the split exceeds 126 bits");
    (void)ok;
    s.neg1 = n1 ? 1u : 0u;
    s.neg2 = n2 ? 1u : 0u;
    return s;
}
// the halves of ONE scalar for all points, made on the host: k_std is any 256-bit pattern in standard form
inline PmSplit pm_split_host(const uint32_t k_std[8]) {
    uint32_t k[8];
    for (int i = 0; i < 8; i++) k[i] = k_std[i];
    pm_scalar_canonical(k, false);
    return pm_split(k);
}

// the point of a record (16 words, 16-byte aligned; Montgomery words, standard form with bases_std) as canonical internal-domain coordinates
FP_HD affine pm_load_point(const uint32_t* rec, bool bases_std) {
    const uint4* q = reinterpret_cast<const uint4*>(rec);
    const uint4 a = q[0], b = q[1], e = q[2], f = q[3];
    const uint32_t wx[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, wy[8] = {e.x, e.y, e.z, e.w, f.x, f.y, f.z, f.w};
    const fp c = bases_std ? fp_const(FP29_IN_STD) : fp_const(FP29_IN_MONT);
    return affine{fp_reduce_lt2p(fp_mul(fp_unpack(wx), c)), fp_reduce_lt2p(fp_mul(fp_unpack(wy), c))};  // < 2^256 * p / 2^261 + p < 1.04
}

// P1 and P2 of the point a (canonical) under the signs of t.s; returns the denominator of S's slope, beta x - x (< 3; a leaf of the product
// tree: every node above it is a product of two values < 3, so < 1.06).  x_zero: the words were no curve point and the denominator is 0.
FP_HD fp pm_table_begin(PmLane& t, const affine& a, bool& x_zero) {
    t.x = a.x;
    t.bx = fp_reduce_lt2p(fp_mul(a.x, fp_from_std(glv::BETA_STD)));  // < 1.01
    const fp ny = fp_neg<2>(a.y);                                    // y < 1: 2p - y <= 2
#pragma unroll
    for (int i = 0; i < 9; i++) {
        t.y1.v[i] = t.s.neg1 ? ny.v[i] : a.y.v[i];
        t.y2.v[i] = t.s.neg2 ? ny.v[i] : a.y.v[i];
    }
    x_zero = fp_is_zero_exact(a.x);
    return fp_sub<2>(t.bx, t.x);                                     // x < 1;  < 3
}
// S = P1 + P2 by the chord: l = (y2 - y1) / (bx - x), sx = l^2 - x - bx, sy = l (x - sx) - y1; id = 1 / (bx - x), < 2
FP_HD void pm_table_finish(PmLane& t, const fp& id) {
    const fp l = fp_mul(fp_sub<4>(t.y2, t.y1), id);             // y1 <= 2: the difference < 6;  l < 6 * 2k + 1 < 1.08
    const fp x3 = fp_sub<3>(fp_sqr(l), fp_add(t.x, t.bx));      // l^2 < 1.01, x + bx < 2;  x3 < 4.01
    t.sx = fp_canonical(x3);
    t.sy = fp_reduce_lt2p(fp_mul_add(l, fp_sub<2>(t.x, t.sx), fp_neg<4>(t.y1), fp_one()));  // l (x + 2p - sx) + (4p - y1) * 1: (1.08 * 3 + 4)k + 1 < 1.05
}

// the entry sel = 1 (P1), 2 (P2) or 3 (S), by selects
FP_HD affine pm_select(const PmLane& t, uint32_t sel) {
    affine q;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        q.x.v[i] = sel == 1u ? t.x.v[i] : sel == 2u ? t.bx.v[i] : t.sx.v[i];
        q.y.v[i] = sel == 1u ? t.y1.v[i] : sel == 2u ? t.y2.v[i] : t.sy.v[i];
    }
    return q;
}
FP_HD void pm_shl(uint32_t (&k)[4], uint32_t by) {  // by in 1 .. 31
    k[3] = (k[3] << by) | (k[2] >> (32 - by));
    k[2] = (k[2] << by) | (k[1] >> (32 - by));
    k[1] = (k[1] << by) | (k[0] >> (32 - by));
    k[0] <<= by;
}
// |k1| * P1 + |k2| * P2: the joint ladder over PM_LADDER_BITS positions, most significant first
FP_HD xyzz pm_ladder(const PmLane& t) {
    uint32_t k1[4] = {t.s.k1[0], t.s.k1[1], t.s.k1[2], t.s.k1[3]}, k2[4] = {t.s.k2[0], t.s.k2[1], t.s.k2[2], t.s.k2[3]};
    pm_shl(k1, 128 - PM_LADDER_BITS);  // bit 125 to the top of the fourth word
    pm_shl(k2, 128 - PM_LADDER_BITS);
    xyzz acc = xyzz_identity();
#pragma nounroll
    for (uint32_t j = 0; j < PM_LADDER_BITS; j++) {
        acc = xyzz_dbl(acc);
        const uint32_t sel = (k1[3] >> 31) | ((k2[3] >> 31) << 1);
        pm_shl(k1, 1);
        pm_shl(k2, 1);
        if (sel) xyzz_madd(acc, pm_select(t, sel));
    }
    return acc;
}

// ---- the phases of a lane, a shared inversion between them (k_pm_mul of msm_kernels_pointwise.hpp; tools/pointwise_mul_check.cpp) ----
// phase 1: the scalar (unless the halves came with the launch: t.s is set then and `scalar` is not read), the point, P1 and P2
template <bool UNIFORM>
FP_HD fp pm_lane_begin(PmLane& t, const uint32_t* base_rec, const uint32_t* scalar, uint32_t flags, bool& x_zero) {
    if (!UNIFORM) {
        const uint4* q = reinterpret_cast<const uint4*>(scalar);
        const uint4 a = q[0], b = q[1];
        uint32_t k[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        pm_scalar_canonical(k, (flags & PM_F_IN_MONT) != 0);
        t.s = pm_split(k);
    }
    return pm_table_begin(t, pm_load_point(base_rec, (flags & PM_F_BASES_STD) != 0), x_zero);
}
// phase 2: S and the ladder
FP_HD xyzz pm_lane_finish(PmLane& t, const fp& id) {
    pm_table_finish(t, id);
    return pm_ladder(t);
}
// the identity, or (words that were no curve point) a ZZZ the shared inversion must not meet
FP_HD bool pm_is_identity(const xyzz& p) { return fp_is_zero_lt2p(p.zz) || fp_is_zero_lt2p(p.zzz); }

}  // namespace pmk
