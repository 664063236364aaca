// msm_kernels_fixed_base.hpp -- the kernels of the G1 fixed-base batch multiplication (fixed_base_bn254.hpp has the routines and the reasoning):
//   k_fb_window_bases  one workgroup: lane j doubles P c*j times (a serial chain, once per (base, c)); the group normalises the W records T_j[1]
//   k_fb_table_level   c-1 launches: level L doubles every window's table with one mixed addition per new entry, normalised by the workgroup's
//                      shared inversion and stored as affine records
//   k_fb_mul           one lane per scalar: recode, at most W mixed additions from the table, the shared inversion, canonical words out
// All three end in fb_batch_inverse: the lanes keep their XYZZ accumulators in registers, only ZZZ goes through LDS (18 KB per workgroup).
#pragma once
#include "fixed_base_bn254.hpp"

namespace fbk {

// 1 / zzz of every lane of the workgroup (1 for an identity); t: FB_TREE_WORDS words of LDS.  Must be reached by all FB_GROUP lanes.
__device__ __forceinline__ fp fb_batch_inverse(uint32_t* t, const fp& zzz, bool identity) {
    const uint32_t lane = threadIdx.x;
    fb_inv_enter(t, lane, zzz, identity);
    for (uint32_t s = FB_GROUP / 2; s >= 1; s >>= 1) {  // uniform
        __syncthreads();
        if (lane < s) fb_inv_up(t, s, lane);
    }
    __syncthreads();
    if (lane == 0) fb_inv_root(t);
    for (uint32_t s = 1; s < FB_GROUP; s <<= 1) {
        __syncthreads();
        if (lane < s) fb_inv_down(t, s, lane);
    }
    __syncthreads();
    return fb_inv_leave(t, lane);
}

// T_j[1] = 2^(c j) * P for j < W <= FB_MAX_WINDOWS <= FB_GROUP: the first record of every window
__global__ void __launch_bounds__(FB_GROUP) k_fb_window_bases(FbBase base, uint32_t c, uint32_t W, uint32_t* __restrict__ table) {
    __shared__ uint32_t tree[FB_TREE_WORDS];
    const uint32_t j = threadIdx.x;
    const bool live = j < W;
    xyzz acc = xyzz_identity();
    if (live) acc = fb_window_base(affine{fp_from_mont256(base.w), fp_from_mont256(base.w + 8)}, c, j);
    const fp iz = fb_batch_inverse(tree, acc.zzz, !live);
    if (live) fb_store_record(table + fb_table_index(j, 1, c) * FB_REC_WORDS, fb_to_affine(acc, iz));
}

// level L of every window's table (fb_table_step): entries lanes, one mixed addition each; launched for L = 1 .. c-1 in turn.
// (table is read and written, at different records: no __restrict__)
__global__ void __launch_bounds__(FB_GROUP) k_fb_table_level(uint32_t* table, uint32_t c, uint32_t L, uint32_t entries) {
    __shared__ uint32_t tree[FB_TREE_WORDS];
    const uint32_t e = blockIdx.x * FB_GROUP + threadIdx.x;
    const bool live = e < entries;
    xyzz acc = xyzz_identity();
    size_t dst = 0;
    if (live) acc = fb_table_step(table, c, L, e, dst);
    const bool identity = xyzz_is_identity(acc);  // (d * 2^(c j) is never a multiple of r: live entries are points)
    const fp iz = fb_batch_inverse(tree, acc.zzz, identity);
    if (live) fb_store_record(table + dst * FB_REC_WORDS, fb_to_affine(acc, iz));
}

// out[i] = k_i * P for i < n (n <= 2^30 per launch); flags: FB_F_IN_MONT, FB_F_OUT_STD
__global__ void __launch_bounds__(FB_GROUP) k_fb_mul(const uint32_t* __restrict__ table, uint32_t c, uint32_t W, const uint32_t* __restrict__ scalars,
                                                    uint32_t n, uint32_t flags, uint32_t* __restrict__ out_xy, uint8_t* __restrict__ out_inf) {
    __shared__ uint32_t tree[FB_TREE_WORDS];
    const uint32_t i = blockIdx.x * FB_GROUP + threadIdx.x;
    const bool live = i < n;
    xyzz acc = xyzz_identity();
    if (live) {
        const uint4* q = reinterpret_cast<const uint4*>(scalars + (size_t)i * 8);
        const uint4 a = q[0], b = q[1];
        uint32_t k[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        if (flags & FB_F_IN_MONT) fb_scalar_from_mont(k);
        acc = fb_mul_point(table, c, W, k);
    }
    const bool identity = xyzz_is_identity(acc);
    const fp iz = fb_batch_inverse(tree, acc.zzz, identity);
    if (live) fb_store_output(out_xy + (size_t)i * 16, out_inf + i, acc, iz, identity, (flags & FB_F_OUT_STD) != 0);
}

}  // namespace fbk
