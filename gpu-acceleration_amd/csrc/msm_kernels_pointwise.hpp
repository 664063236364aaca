// msm_kernels_pointwise.hpp -- the kernel of the G1 element-wise scalar multiplication (pointwise_mul_bn254.hpp has the routines and the
// reasoning):
//   k_pm_mul<false>  one lane per point: scalar -> halves, P1, P2, the shared inversion of the slopes' denominators, S, the joint ladder, the
//                    shared inversion of ZZZ, canonical words out
//   k_pm_mul<true>   the same body with the halves of ONE scalar as a launch argument: the ladder's column sequence is wave-uniform, no lane
//                    waits for another's addition
// Both inversions are fb_batch_inverse of msm_kernels_fixed_base.hpp over the same 18 KB of LDS: every lane of the workgroup reaches both.
#pragma once
#include "msm_kernels_fixed_base.hpp"
#include "pointwise_mul_bn254.hpp"

namespace pmk {

// out[i] = k_i * P_i resp. k * P_i for i < n (n <= 2^30 per launch); flags: PM_F_IN_MONT, PM_F_OUT_STD, PM_F_BASES_STD.  inf_mask may be null.
// out_xy may BE bases and out_inf may BE inf_mask (a lane reads its own record before it writes it; no other lane touches it): those four
// carry no __restrict__.
template <bool UNIFORM>
__global__ void __launch_bounds__(FB_GROUP) k_pm_mul(const uint32_t* bases, const uint8_t* inf_mask, const uint32_t* __restrict__ scalars, PmSplit uni,
                                                    uint32_t n, uint32_t flags, uint32_t* out_xy, uint8_t* out_inf) {
    __shared__ uint32_t tree[FB_TREE_WORDS];
    const uint32_t i = blockIdx.x * FB_GROUP + threadIdx.x;
    const bool live = i < n;
    const bool idle = !live || (inf_mask != nullptr && inf_mask[i] != 0);  // a flagged base: the identity whatever the scalar
    PmLane t;
    t.s = uni;
    fp den = fp_one();
    bool x_zero = false;
    if (!idle) den = pm_lane_begin<UNIFORM>(t, bases + (size_t)i * 16, scalars + (size_t)i * 8, flags, x_zero);
    const fp id = fb_batch_inverse(tree, den, idle || x_zero);
    xyzz acc = xyzz_identity();
    if (!idle) acc = pm_lane_finish(t, id);
    const bool identity = pm_is_identity(acc);
    const fp iz = fb_batch_inverse(tree, acc.zzz, identity);
    if (live) fb_store_output(out_xy + (size_t)i * 16, out_inf + i, acc, iz, identity, (flags & PM_F_OUT_STD) != 0);
}

}  // namespace pmk
