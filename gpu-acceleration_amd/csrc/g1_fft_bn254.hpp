// g1_fft_bn254.hpp -- the discrete Fourier transform over BN254 G1 POINTS, out[j] = sum_i w^(ij) * P_i (and its inverse, with n^-1), in place on
// affine records: what turns a powers-of-tau output tau^j * G into the Lagrange basis L_i(tau) * G when nobody knows tau.  The per-butterfly
// routines, __host__ __device__ throughout: tools/g1_fft_check.cpp runs them on the CPU with -DFP_BOUNDS_CHECK; the kernels are
// msm_kernels_g1_fft.hpp, the host side msm_g1_fft.inc.
//
// Shape.  Radix 2, decimation in time: a bit-reversal sweep of the records, then log_n stages, one launch each, one lane per butterfly, the
// points affine Montgomery records between the stages (the caller's arrays are the working storage).  Decimation in time because the operand that
// meets the twiddle must be AFFINE before the ladder starts (pointwise_mul_bn254.hpp builds P, lambda P, P + lambda P from an affine point): here
// it is B as loaded; in decimation in frequency it would be A - B, an inversion earlier.  Stage s = 1 .. log_n, half = 2^(s-1); butterfly b of
// an array: g = b / half, j = b % half, A at g * 2^s + j, B at A + half, twiddle w_n^t with t = j * n / 2^s < n / 2.  Per lane:
//   1. T = w * B: pm_lane_begin on B's record and the twiddle (a standard-form scalar), the shared inversion of the slopes' denominators,
//      pm_lane_finish -- the routines of pointwise_mul_bn254.hpp as they are.  The first stage has every twiddle 1 and runs no ladder: T = B;
//   2. A' = A + T and B' = A - T: two complete mixed additions xyzz_madd of the affine A, to T and to -T = (X, -Y, ZZ, ZZZ).  A == T doubles,
//      A == -T cancels, T = identity (a flagged B, or w * B = 0 for words that are no point of the group) copies A: the complete formula decides,
//      no case here.  A flagged A is the identity operand: the two sums are then T and -T, chosen by selects after the additions;
//   3. ONE shared inversion for the 2 * FB_GROUP results of a workgroup: the lane enters the product ZZZ_A' * ZZZ_B' (an identity enters as 1)
//      and un-multiplies, 1 / ZZZ_A' = inv * ZZZ_B' and the other way round;
//   4. canonical words and the flag of both results (fb_store_output).
// No other lane touches a butterfly's two records or flag bytes: the stage is in place.  Every address is a function of the lane's index alone.
//
// One table serves both directions.  It holds w^t for t < n / 2 in standard form; the inverse transform needs w^(-t) = -w^(n/2 - t) for t > 0
// (w^(n/2) = -1): it reads entry n/2 - t and SWAPS the butterfly's two outputs (A - T' = A + w^(-t) B goes to A's place); t = 0 is w^0 either way.
//
// Count per butterfly (field multiplications, the conventions of pointwise_mul_bn254.hpp): the ladder and its table 2 161 - 6 - 3 = 2 152 (no
// output and no second inversion there), + 2 (A) + 2 * 9 (the additions) + 1 (the product) + 3 (the tree) + 2 (un-multiply) + 2 * 6 (output)
// = 2 190 against 2 161 for the point alone, 1.3 % more.  The inversion by the product: 6 per butterfly and one fp_inv and 17 barriers per
// workgroup; two calls of fb_batch_inverse would be 6 as well, with a second fp_inv (335 dependent multiplications on ONE lane while 255 wait)
// and 17 more barriers -- so the product.
// Later stages do not skip their w = 1 butterflies (one in 2^(s-1)): the ladder runs on the scalar 1 there.
#pragma once
#include "pointwise_mul_bn254.hpp"

namespace gfk {

using namespace pmk;

constexpr uint32_t GF_MAX_LOG2 = 28;                            // r - 1 has 28 factors of two
constexpr uint32_t GF_F_INVERSE = 1u;                           // == MSM_NTT_INVERSE
constexpr uint32_t GF_F_OUT_STD = PM_F_OUT_STD, GF_F_IN_STD = PM_F_BASES_STD;  // == MSM_FB_OUT_STD, MSM_PM_BASES_STD

struct GfPlan {  // == msm_g1_fft_plan_t
    uint16_t stages, ladder_stages;
    uint32_t inv_group;
    uint64_t table_bytes;
};
// entries of the twiddle table of a size: n / 2 powers of w, none where no stage runs a ladder
FP_HD uint64_t gf_table_entries(uint32_t log_n) { return log_n >= 2 ? (uint64_t)1 << (log_n - 1) : 0; }
inline GfPlan gf_plan(uint32_t log_n) {
    return GfPlan{(uint16_t)log_n, (uint16_t)(log_n ? log_n - 1 : 0), FB_GROUP, gf_table_entries(log_n) * 32};
}

struct GfStage {  // a kernel argument: the stage s of a transform of 2^log_n points
    uint32_t log_n, s, flags;  // flags: GF_F_INVERSE; GF_F_IN_STD: the records are standard-form words (first stage); GF_F_OUT_STD (last stage)
};
struct GfPair {  // where butterfly `item` of a launch reads and writes
    uint64_t a, b;      // records (and flag bytes) of A and B
    uint64_t out_sum, out_diff;  // where A + T and A - T go: a, b, or b, a for a swapped inverse butterfly
    uint64_t tw;        // entry of the twiddle table (0 in the first stage)
};
// item < batch * n / 2 (n >= 2): array item / (n / 2), butterfly item % (n / 2)
FP_HD GfPair gf_pair(uint64_t item, const GfStage& st) {
    const uint32_t k = st.log_n, s = st.s;
    const uint64_t half_n = (uint64_t)1 << (k - 1), arr = item >> (k - 1), b = item & (half_n - 1);
    const uint64_t half = (uint64_t)1 << (s - 1), g = b >> (s - 1), j = b & (half - 1);
    GfPair p;
    p.a = (arr << k) + (g << s) + j;  // < batch * n
    p.b = p.a + half;                 // g * 2^s + j + half < (g + 1) * 2^s <= n: inside the array
    const uint64_t t = j << (k - s);  // < half * n / 2^s = n / 2
    const bool swap = (st.flags & GF_F_INVERSE) != 0 && t != 0;
    p.tw = swap ? half_n - t : t;     // in 1 .. n/2 - 1 resp. 0 .. n/2 - 1: inside the table
    p.out_sum = swap ? p.b : p.a;
    p.out_diff = swap ? p.a : p.b;
    return p;
}
// the k low bits of i reversed (k in 1 .. 32)
FP_HD uint32_t gf_rev(uint32_t i, uint32_t k) {
    i = (i >> 16) | (i << 16);
    i = ((i & 0xFF00FF00u) >> 8) | ((i & 0x00FF00FFu) << 8);
    i = ((i & 0xF0F0F0F0u) >> 4) | ((i & 0x0F0F0F0Fu) << 4);
    i = ((i & 0xCCCCCCCCu) >> 2) | ((i & 0x33333333u) << 2);
    i = ((i & 0xAAAAAAAAu) >> 1) | ((i & 0x55555555u) << 1);
    return i >> (32 - k);
}
// element `item` of batch * n of the bit-reversal sweep: swaps the record and the flag byte with its partner's when it is the lower of the pair
FP_HD void gf_bitrev_one(uint32_t* xy, uint8_t* inf, uint64_t item, uint32_t log_n) {
    const uint64_t arr = item >> log_n;
    const uint32_t i = (uint32_t)(item & (((uint64_t)1 << log_n) - 1)), r = gf_rev(i, log_n);  // r < n
    if (i >= r) return;
    uint4* p = reinterpret_cast<uint4*>(xy + ((arr << log_n) + i) * 16);
    uint4* q = reinterpret_cast<uint4*>(xy + ((arr << log_n) + r) * 16);
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const uint4 t = p[w];
        p[w] = q[w];
        q[w] = t;
    }
    const uint8_t f = inf[(arr << log_n) + i];
    inf[(arr << log_n) + i] = inf[(arr << log_n) + r];
    inf[(arr << log_n) + r] = f;
}

// ---- the phases of a lane, a shared inversion between them (k_gf_stage of msm_kernels_g1_fft.hpp; tools/g1_fft_check.cpp) ----
// phase 1 of a ladder stage: B's record and the twiddle (8 standard-form words) -> P1, P2; returns the denominator of S's slope (< 3)
FP_HD fp gf_lane_begin(PmLane& t, const uint32_t* b_rec, const uint32_t* tw, const GfStage& st, bool& x_zero) {
    return pm_lane_begin<false>(t, b_rec, tw, st.flags & GF_F_IN_STD, x_zero);  // (PM_F_IN_MONT clear: the table is in standard form)
}
// phase 1 of the first stage: T = B
FP_HD xyzz gf_lane_plain(const uint32_t* b_rec, const GfStage& st) {
    return xyzz_from_affine(pm_load_point(b_rec, (st.flags & GF_F_IN_STD) != 0));  // x, y canonical
}
// phase 2: sum = A + T, diff = A - T.  T: X < 7, Y <= 2 (a ladder ends in xyzz_dbl or xyzz_madd: Y < 1.42; an accumulator that was only ever
// set from a table entry holds its y <= 2; the first stage's y < 1), ZZ, ZZZ < 2, or the identity (ZZ == 0).  a: x, y canonical (pm_load_point).
FP_HD void gf_butterfly(const xyzz& T, const affine& a, bool a_inf, xyzz& sum, xyzz& diff) {
    const xyzz nT{T.x, fp_neg<3>(T.y), T.zz, T.zzz};  // Y <= 2: 3p - Y <= 3 (< 5, the bound of XYZZ)
    sum = T;
    diff = nT;
    xyzz_madd(sum, a);   // x < 1, y < 1
    xyzz_madd(diff, a);
#pragma unroll
    for (int i = 0; i < 9; i++) {  // a flagged A: 0 + T and 0 - T (whatever its words gave above is dropped)
        sum.x.v[i] = a_inf ? T.x.v[i] : sum.x.v[i];
        sum.y.v[i] = a_inf ? T.y.v[i] : sum.y.v[i];
        sum.zz.v[i] = a_inf ? T.zz.v[i] : sum.zz.v[i];
        sum.zzz.v[i] = a_inf ? T.zzz.v[i] : sum.zzz.v[i];
        diff.x.v[i] = a_inf ? nT.x.v[i] : diff.x.v[i];
        diff.y.v[i] = a_inf ? nT.y.v[i] : diff.y.v[i];
        diff.zz.v[i] = a_inf ? nT.zz.v[i] : diff.zz.v[i];
        diff.zzz.v[i] = a_inf ? nT.zzz.v[i] : diff.zzz.v[i];
    }
}
// phase 3: what the lane puts into the shared inversion: ZZZ_sum * ZZZ_diff, an identity as 1 (ZZZ < 2: the product < 1.03, a leaf below 2)
FP_HD fp gf_inv_enter(const xyzz& sum, bool sum_id, const xyzz& diff, bool diff_id, fp& zs, fp& zd) {
    zs = sum_id ? fp_one() : sum.zzz;
    zd = diff_id ? fp_one() : diff.zzz;
    return fp_mul(zs, zd);
}
// phase 4: inv = 1 / (zs * zd) (< 2) -> 1 / zs = inv * zd, 1 / zd = inv * zs (< 1.03), and the two records
FP_HD void gf_lane_store(uint32_t* xy, uint8_t* inf, const GfPair& p, const xyzz& sum, bool sum_id, const xyzz& diff, bool diff_id, const fp& inv,
                         const fp& zs, const fp& zd, bool out_std) {
    fb_store_output(xy + p.out_sum * 16, inf + p.out_sum, sum, fp_mul(inv, zd), sum_id, out_std);
    fb_store_output(xy + p.out_diff * 16, inf + p.out_diff, diff, fp_mul(inv, zs), diff_id, out_std);
}

}  // namespace gfk
