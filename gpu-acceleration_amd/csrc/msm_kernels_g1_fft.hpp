// msm_kernels_g1_fft.hpp -- the kernels of the G1 group transform (g1_fft_bn254.hpp has the routines and the reasoning):
//   k_gf_bitrev        one lane per record: the lower index of a pair (i, rev(i)) swaps the two 64-byte records and their flag bytes
//   k_gf_stage<true>   one lane per butterfly (A, B, w): T = w * B by the ladder of pointwise_mul_bn254.hpp (the shared inversion of the slopes'
//                      denominators in its middle), A + T and A - T, the shared inversion of the products ZZZ * ZZZ, canonical words out
//   k_gf_stage<false>  the same body without the ladder and its inversion, T = B: the first stage, every twiddle 1
// Both inversions are fb_batch_inverse of msm_kernels_fixed_base.hpp over the same 18 KB of LDS: every lane of the workgroup reaches both.
#pragma once
#include "msm_kernels_fixed_base.hpp"
#include "g1_fft_bn254.hpp"

namespace gfk {

// records first .. first + count of batch * n (count <= 2^30 per launch)
__global__ void __launch_bounds__(FB_GROUP) k_gf_bitrev(uint32_t* xy, uint8_t* inf, uint32_t log_n, uint64_t first, uint32_t count) {
    const uint32_t l = blockIdx.x * FB_GROUP + threadIdx.x;
    if (l < count) gf_bitrev_one(xy, inf, first + l, log_n);
}

// butterflies first .. first + count of batch * n / 2 (count <= 2^30 per launch) of stage st.s, in place: a lane reads its two records and flag
// bytes before it writes them, and no other lane touches them.  tw: n / 2 standard-form powers of w (not read by the first stage).
template <bool LADDER>
__global__ void __launch_bounds__(FB_GROUP) k_gf_stage(uint32_t* xy, uint8_t* inf, const uint32_t* __restrict__ tw, GfStage st, uint64_t first,
                                                      uint32_t count) {
    __shared__ uint32_t tree[FB_TREE_WORDS];
    const uint32_t l = blockIdx.x * FB_GROUP + threadIdx.x;
    const bool live = l < count;
    GfPair p{};
    bool a_inf = true, b_inf = true;
    if (live) {
        p = gf_pair(first + l, st);
        a_inf = inf[p.a] != 0;
        b_inf = inf[p.b] != 0;
    }
    const bool idle = !live || b_inf;  // a flagged B: T is the identity whatever the twiddle
    xyzz T = xyzz_identity();
    if (LADDER) {
        PmLane t;
        fp den = fp_one();
        bool x_zero = false;
        if (!idle) den = gf_lane_begin(t, xy + p.b * 16, tw + p.tw * 8, st, x_zero);
        const fp id = fb_batch_inverse(tree, den, idle || x_zero);
        if (!idle) T = pm_lane_finish(t, id);
    } else if (!idle) {
        T = gf_lane_plain(xy + p.b * 16, st);
    }
    xyzz sum = xyzz_identity(), diff = xyzz_identity();
    if (live) gf_butterfly(T, pm_load_point(xy + p.a * 16, (st.flags & GF_F_IN_STD) != 0), a_inf, sum, diff);
    const bool sum_id = pm_is_identity(sum), diff_id = pm_is_identity(diff);
    fp zs, zd;
    const fp prod = gf_inv_enter(sum, sum_id, diff, diff_id, zs, zd);
    const fp inv = fb_batch_inverse(tree, prod, false);
    if (live) gf_lane_store(xy, inf, p, sum, sum_id, diff, diff_id, inv, zs, zd, (st.flags & GF_F_OUT_STD) != 0);
}

}  // namespace gfk
