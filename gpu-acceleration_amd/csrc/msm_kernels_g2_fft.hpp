// msm_kernels_g2_fft.hpp -- the kernels of the G2 group transform (g2_fft_bn254.hpp has the routines and the reasoning):
//   k_gf2_bitrev        one lane per record: the lower index of a pair (i, rev(i)) swaps the two 128-byte records and their flag bytes
//   k_gf2_stage<true>   one lane per butterfly (A, B, w): T = w * B by the ladder of g2_pointwise_mul_bn254.hpp (the shared inversion of the norms
//                       of the slopes' denominators in its middle), A + T and A - T, the shared inversion of the products N(ZZZ) * N(ZZZ),
//                       canonical words out
//   k_gf2_stage<false>  the same body without the ladder and its inversion, T = B: the first stage, every twiddle 1
// Both inversions are fb_batch_inverse of msm_kernels_fixed_base.hpp over the same 18 KB of LDS, in Fq: every lane of the workgroup reaches
// both.  No scratch array: a stage is one kernel, as k_pm2_mul is.
#pragma once
#include "msm_kernels_fixed_base.hpp"
#include "g2_fft_bn254.hpp"

namespace gfk {

// records first .. first + count of batch * n (count <= 2^30 per launch)
__global__ void __launch_bounds__(FB_GROUP) k_gf2_bitrev(uint32_t* xy, uint8_t* inf, uint32_t log_n, uint64_t first, uint32_t count) {
    const uint32_t l = blockIdx.x * FB_GROUP + threadIdx.x;
    if (l < count) gf2_bitrev_one(xy, inf, first + l, log_n);
}

// butterflies first .. first + count of batch * n / 2 (count <= 2^30 per launch) of stage st.s, in place: a lane reads its two records and flag
// bytes before it writes them, and no other lane touches them.  tw: n / 2 standard-form powers of w (not read by the first stage).
template <bool LADDER>
__global__ void __launch_bounds__(FB_GROUP) k_gf2_stage(uint32_t* xy, uint8_t* inf, const uint32_t* __restrict__ tw, GfStage st, uint64_t first,
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
    xyzz2 T = xyzz2_identity();
    if (LADDER) {
        Pm2Lane t;
        fp den = fp_one();
        bool x_zero = false;
        if (!idle) den = gf2_lane_begin(t, xy + p.b * FB2_REC_WORDS, tw + p.tw * 8, st, x_zero);
        const fp ni = fb_batch_inverse(tree, den, idle || x_zero);
        if (!idle) T = pm2_lane_finish(t, ni);
    } else if (!idle) {
        T = gf2_lane_plain(xy + p.b * FB2_REC_WORDS, st);
    }
    xyzz2 sum = xyzz2_identity(), diff = xyzz2_identity();
    if (live) gf2_butterfly(T, pm2_load_point(xy + p.a * FB2_REC_WORDS, (st.flags & GF_F_IN_STD) != 0), a_inf, sum, diff);
    const bool sum_id = pm2_is_identity(sum), diff_id = pm2_is_identity(diff);
    fp ns, nd;
    const fp prod = gf2_inv_enter(sum, sum_id, diff, diff_id, ns, nd);
    const fp inv = fb_batch_inverse(tree, prod, false);
    if (live) gf2_lane_store(xy, inf, p, sum, sum_id, diff, diff_id, inv, ns, nd, (st.flags & GF_F_OUT_STD) != 0);
}

}  // namespace gfk
