// msm_kernels_g2_pointwise.hpp -- the kernel of the G2 element-wise scalar multiplication (g2_pointwise_mul_bn254.hpp has the routines and the
// reasoning):
//   k_pm2_mul<false>  one lane per point: scalar -> halves, x, beta^2 x, y, the shared inversion of the norms of the slopes' denominators, S, the
//                     joint ladder over Fq2, the shared inversion of the norms of ZZZ, canonical words out
//   k_pm2_mul<true>   the same body with the halves of ONE scalar as a launch argument: the ladder's column sequence is wave-uniform
// Both inversions are fb_batch_inverse of msm_kernels_fixed_base.hpp over the same 18 KB of LDS, in Fq: every lane of the workgroup reaches
// both.  One kernel per call and no scratch array (unlike k_fb2_accumulate): the ladder is long enough to carry the two one-lane fp_inv.
#pragma once
#include "msm_kernels_fixed_base.hpp"
#include "g2_pointwise_mul_bn254.hpp"

namespace pmk {

// out[i] = k_i * Q_i resp. k * Q_i for i < n (n <= 2^30 per launch); flags: PM_F_IN_MONT, PM_F_OUT_STD, PM_F_BASES_STD.  inf_mask may be null.
// out_xy may BE bases and out_inf may BE inf_mask (a lane reads its own record before it writes it; no other lane touches it): those four
// carry no __restrict__.
template <bool UNIFORM>
__global__ void __launch_bounds__(FB_GROUP) k_pm2_mul(const uint32_t* bases, const uint8_t* inf_mask, const uint32_t* __restrict__ scalars, PmSplit uni,
                                                     uint32_t n, uint32_t flags, uint32_t* out_xy, uint8_t* out_inf) {
    __shared__ uint32_t tree[FB_TREE_WORDS];
    const uint32_t i = blockIdx.x * FB_GROUP + threadIdx.x;
    const bool live = i < n;
    const bool idle = !live || (inf_mask != nullptr && inf_mask[i] != 0);  // a flagged base: the identity whatever the scalar
    Pm2Lane t;
    t.s = uni;
    fp den = fp_one();
    bool x_zero = false;
    if (!idle) den = pm2_lane_begin<UNIFORM>(t, bases + (size_t)i * FB2_REC_WORDS, scalars + (size_t)i * 8, flags, x_zero);
    const fp ni = fb_batch_inverse(tree, den, idle || x_zero);
    xyzz2 acc = xyzz2_identity();
    if (!idle) acc = pm2_lane_finish(t, ni);
    const bool identity = pm2_is_identity(acc);
    fp nrm = fp_one();
    if (!identity) nrm = pm2_out_norm(acc);
    const fp nz = fb_batch_inverse(tree, nrm, identity);
    if (live) pm2_store_output(out_xy + (size_t)i * FB2_REC_WORDS, out_inf + i, acc, nz, identity, (flags & PM_F_OUT_STD) != 0);
}

}  // namespace pmk
