// g2_fft_bn254.hpp -- the discrete Fourier transform over BN254 G2 POINTS, out[j] = sum_i w^(ij) * Q_i (and its inverse, with n^-1), in place on
// affine records of 32 words: what turns the tauG2 section tau^j * H of a powers-of-tau file into L_i(tau) * H when nobody knows tau.
// g1_fft_bn254.hpp over Fq2: the per-butterfly routines, __host__ __device__ throughout: tools/g2_fft_check.cpp runs them on the CPU with
// -DFP_BOUNDS_CHECK; the kernels are msm_kernels_g2_fft.hpp, the host side msm_g1_fft.inc (one body for both groups).
//
// Shape.  The G1 transform's, stage for stage: a bit-reversal sweep of the records, then log_n stages, one launch each, one lane per butterfly,
// decimation in time (the operand that meets the twiddle must be affine before the ladder starts).  The index arithmetic does not know the group:
// GfStage, GfPair, gf_pair and gf_rev are g1_fft_bn254.hpp's, used as they are; so is the twiddle table (n / 2 standard-form powers of w, one
// table for both groups and both directions; the inverse reads entry n/2 - t and swaps its outputs, which gf_pair already does).  Per lane:
//   1. T = w * B: pm2_lane_begin<false> on B's record and the twiddle, the shared inversion of the NORMS of the slopes' denominators,
//      pm2_lane_finish -- the routines of g2_pointwise_mul_bn254.hpp as they are.  The first stage has every twiddle 1 and runs no ladder: T = B;
//   2. A' = A + T and B' = A - T: two complete mixed additions xyzz2_madd of the affine A, to T and to -T = (X, 8p - Y, ZZ, ZZZ).  A == T doubles,
//      A == -T cancels, T = identity (a flagged B, or w * B = O for words that are no point of G2) copies A: the complete formula decides, no
//      case here.  A flagged A is the identity operand: the two sums are then T and -T, chosen by selects after the additions;
//   3. ONE shared inversion for the 2 * FB_GROUP results of a workgroup, in Fq: the lane enters N(ZZZ_A') * N(ZZZ_B') (pm2_out_norm; an identity
//      enters as 1) and un-multiplies, 1 / N(ZZZ_A') = inv * N(ZZZ_B') and the other way round;
//   4. canonical words and the flag of both results (pm2_store_output: 1 / ZZZ = conj(ZZZ) / N).
// No other lane touches a butterfly's two records or flag bytes: the stage is in place.  Every address is a function of the lane's index alone.
//
// The bound on -T.  ec_g2_bn254.hpp promises Y < 8 for every XYZZ value, and a negation 9p - Y of such a Y would leave that range (<= 9).  What
// a ladder LEAVES is narrower: its last step is xyzz2_dbl (y3 < 6.6), xyzz2_madd (y3 < 5.8), or the set of an empty accumulator from a table
// entry (y <= 2); the first stage's T is a record's canonical y (< 1).  So T.y < 6.6 < 7 = (8 - 1): fp2_neg<8> takes it, and -T.y = 8p - T.y <= 8p,
// with 8p itself only for a component of y that is exactly zero (the case ec_g2_bn254.hpp's affine bound "y <= 2" names).  xyzz2_madd reads the
// accumulator's Y in fp2_sub<9>(s2, acc.y) and as the second factor of fp2_mul<9>(ppp, acc.y): the 9p pad takes a normalised subtrahend limb by
// limb up to about 9p - 2^232 (the remark on pads in ec_g2_bn254.hpp), so <= 8p is inside, and the value bounds written there (R < 10.2,
// 2.1 * 17k + 1) are computed for 8.  X, ZZ and ZZZ of -T are T's.  tools/g2_fft_check.cpp asserts T.y < 7p, -T.y <= 8p and the XYZZ bounds of
// both sums in every butterfly it runs, next to the limb-wise pad checks of -DFP_BOUNDS_CHECK.
//
// The leaf of the product tree.  N(ZZZ) = c0^2 + c1^2 < 2 * (4.2^2 k + 1) < 2.3 (fb2_norm); the product of two: 2.3 * 2.3 k + 1 < 1.04, below the
// 2.2 of the leaf that pm2_table_begin enters, so every node above it stays < 1.06 as there.  inv = 1 / (Ns * Nd) < 2 (what the tree hands every
// leaf); 1 / Ns = inv * Nd: 2 * 2.3 k + 1 < 1.03 < 2, what pm2_store_output asks of its ni.
//
// Count per butterfly, in the units of g2_pointwise_mul_bn254.hpp (an fp2_mul or fp2_sqr is two): the ladder and its table 4 830 - 19 = 4 811 (no
// norm, no 1 / ZZZ, no output and no second tree there: 2 + 2 + 12 + 3), + 4 (A) + 2 * 20 (the additions) + 2 * 2 (the norms) + 1 (the product)
// + 3 (the tree) + 2 (un-multiply) + 2 * (2 + 12) (1 / ZZZ and the output, twice) = 4 893 against 4 830 for the point alone, 1.3 % more; the
// first stage 82.  In limb products: 126 * (3 888 + 4 536) + 2 * 4 536 for the two additions, 1.070 M against 1.061 M, 0.9 % more.
// Later stages do not skip their w = 1 butterflies (one in 2^(s-1)): the ladder runs on the scalar 1 there.
#pragma once
#include "g1_fft_bn254.hpp"
#include "g2_pointwise_mul_bn254.hpp"

namespace gfk {

using Gf2Plan = GfPlan;  // == msm_g2_fft_plan_t: the same four fields; gf_plan(log_n) is the plan of both groups (one table)

// element `item` of batch * n of the bit-reversal sweep: swaps the 128-byte record and the flag byte with its partner's when it is the lower of
// the pair
FP_HD void gf2_bitrev_one(uint32_t* xy, uint8_t* inf, uint64_t item, uint32_t log_n) {
    const uint64_t arr = item >> log_n;
    const uint32_t i = (uint32_t)(item & (((uint64_t)1 << log_n) - 1)), r = gf_rev(i, log_n);  // r < n
    if (i >= r) return;
    uint4* p = reinterpret_cast<uint4*>(xy + ((arr << log_n) + i) * FB2_REC_WORDS);
    uint4* q = reinterpret_cast<uint4*>(xy + ((arr << log_n) + r) * FB2_REC_WORDS);
#pragma unroll
    for (int w = 0; w < 8; w++) {
        const uint4 t = p[w];
        p[w] = q[w];
        q[w] = t;
    }
    const uint8_t f = inf[(arr << log_n) + i];
    inf[(arr << log_n) + i] = inf[(arr << log_n) + r];
    inf[(arr << log_n) + r] = f;
}

// ---- the phases of a lane, a shared inversion between them (k_gf2_stage of msm_kernels_g2_fft.hpp; tools/g2_fft_check.cpp) ----
// phase 1 of a ladder stage: B's record and the twiddle (8 standard-form words) -> x, beta^2 x, y; returns the norm of the denominator of S's
// slope (< 2.2)
FP_HD fp gf2_lane_begin(Pm2Lane& t, const uint32_t* b_rec, const uint32_t* tw, const GfStage& st, bool& x_zero) {
    return pm2_lane_begin<false>(t, b_rec, tw, st.flags & GF_F_IN_STD, x_zero);  // (PM_F_IN_MONT clear: the table is in standard form)
}
// phase 1 of the first stage: T = B
FP_HD xyzz2 gf2_lane_plain(const uint32_t* b_rec, const GfStage& st) {
    return fb2_from_affine(pm2_load_point(b_rec, (st.flags & GF_F_IN_STD) != 0));  // x, y canonical
}
// -T: Y < 7 in (the header's remark: a ladder leaves < 6.6, the first stage < 1), <= 8 out; X, ZZ, ZZZ as they are
FP_HD xyzz2 gf2_neg(const xyzz2& T) { return xyzz2{T.x, fp2_neg<8>(T.y), T.zz, T.zzz}; }
// r = pick ? v : r, by selects
FP_HD void gf2_pick(fp2& r, const fp2& v, bool pick) {
#pragma unroll
    for (int i = 0; i < 9; i++) {
        r.c0.v[i] = pick ? v.c0.v[i] : r.c0.v[i];
        r.c1.v[i] = pick ? v.c1.v[i] : r.c1.v[i];
    }
}
// phase 2: sum = A + T, diff = A - T.  T: X < 12, Y < 6.6, ZZ, ZZZ < 4.2, or the identity (ZZ == 0).  a: x, y canonical (pm2_load_point).
FP_HD void gf2_butterfly(const xyzz2& T, const affine2& a, bool a_inf, xyzz2& sum, xyzz2& diff) {
    const xyzz2 nT = gf2_neg(T);  // Y <= 8: what xyzz2_madd accepts for an accumulator (the header's remark)
    sum = T;
    diff = nT;
    xyzz2_madd(sum, a);   // x < 1, y < 1
    xyzz2_madd(diff, a);
    // a flagged A: 0 + T and 0 - T (whatever its words gave above is dropped)
    gf2_pick(sum.x, T.x, a_inf), gf2_pick(sum.y, T.y, a_inf), gf2_pick(sum.zz, T.zz, a_inf), gf2_pick(sum.zzz, T.zzz, a_inf);
    gf2_pick(diff.x, nT.x, a_inf), gf2_pick(diff.y, nT.y, a_inf), gf2_pick(diff.zz, nT.zz, a_inf), gf2_pick(diff.zzz, nT.zzz, a_inf);
}
// phase 3: what the lane puts into the shared inversion: N(ZZZ_sum) * N(ZZZ_diff), an identity as 1 (each < 2.3: the product < 1.04, a leaf
// below pm2_table_begin's 2.2)
FP_HD fp gf2_inv_enter(const xyzz2& sum, bool sum_id, const xyzz2& diff, bool diff_id, fp& ns, fp& nd) {
    ns = sum_id ? fp_one() : pm2_out_norm(sum);
    nd = diff_id ? fp_one() : pm2_out_norm(diff);
    return fp_mul(ns, nd);
}
// phase 4: inv = 1 / (ns * nd) (< 2) -> 1 / ns = inv * nd, 1 / nd = inv * ns (2 * 2.3k + 1 < 1.03: the ni < 2 of pm2_store_output), and the
// two records
FP_HD void gf2_lane_store(uint32_t* xy, uint8_t* inf, const GfPair& p, const xyzz2& sum, bool sum_id, const xyzz2& diff, bool diff_id, const fp& inv,
                          const fp& ns, const fp& nd, bool out_std) {
    pm2_store_output(xy + p.out_sum * FB2_REC_WORDS, inf + p.out_sum, sum, fp_mul(inv, nd), sum_id, out_std);
    pm2_store_output(xy + p.out_diff * FB2_REC_WORDS, inf + p.out_diff, diff, fp_mul(inv, ns), diff_id, out_std);
}

}  // namespace gfk
