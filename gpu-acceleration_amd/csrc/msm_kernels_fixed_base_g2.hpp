// msm_kernels_fixed_base_g2.hpp -- the kernels of the G2 fixed-base batch multiplication (fixed_base_g2_bn254.hpp has the routines and the reasoning):
//   k_fb2_window_bases  one workgroup: lane j doubles Q c*j times (a serial chain, once per (base, c)); the group normalises the W records T_j[1]
//   k_fb2_table_level   c-1 launches: level L doubles every window's table with one mixed addition per new entry, stored as affine2 records
//   k_fb2_accumulate    one lane per scalar: recode, at most W mixed additions from the table, the XYZZ sum into the scratch array
//   k_fb2_normalise     one lane per chain of G points of the scratch array: Fq arithmetic only, canonical words out
// The two table kernels run once per base and end in the G1 product tree over the NORMS of ZZZ (fb_batch_inverse of
// msm_kernels_fixed_base.hpp, called as it is: leaves < 2.3 instead of < 2, so a node is below 2.3^2 k + 1 < 1.04 and the root's inverse below 2).
#pragma once
#include "fixed_base_g2_bn254.hpp"
#include "msm_kernels_fixed_base.hpp"

namespace fbk {

// T_j[1] = 2^(c j) * Q for j < W <= FB_MAX_WINDOWS <= FB_GROUP: the first record of every window
__global__ void __launch_bounds__(FB_GROUP) k_fb2_window_bases(Fb2Base base, uint32_t c, uint32_t W, uint32_t* __restrict__ table) {
    __shared__ uint32_t tree[FB_TREE_WORDS];
    const uint32_t j = threadIdx.x;
    const bool live = j < W;
    xyzz2 acc = xyzz2_identity();
    if (live) acc = fb2_window_base(fb2_base_affine(base.w), c, j);
    const fp ni = fb_batch_inverse(tree, live ? fb2_norm(acc.zzz) : fp_one(), !live);
    if (live) fb2_store_record(table + fb_table_index(j, 1, c) * FB2_REC_WORDS, fb2_to_affine(acc, fb2_inv_from_norm(acc.zzz, ni)));
}

// level L of every window's table (fb2_table_step): entries lanes, one mixed addition each; launched for L = 1 .. c-1 in turn.
// (table is read and written, at different records: no __restrict__)
__global__ void __launch_bounds__(FB_GROUP) k_fb2_table_level(uint32_t* table, uint32_t c, uint32_t L, uint32_t entries) {
    __shared__ uint32_t tree[FB_TREE_WORDS];
    const uint32_t e = blockIdx.x * FB_GROUP + threadIdx.x;
    const bool live = e < entries;
    xyzz2 acc = xyzz2_identity();
    size_t dst = 0;
    if (live) acc = fb2_table_step(table, c, L, e, dst);
    const bool identity = xyzz2_is_identity(acc);  // (d * 2^(c j) is never a multiple of r: live entries are points)
    const fp ni = fb_batch_inverse(tree, identity ? fp_one() : fb2_norm(acc.zzz), identity);
    if (live && !identity) fb2_store_record(table + dst * FB2_REC_WORDS, fb2_to_affine(acc, fb2_inv_from_norm(acc.zzz, ni)));
}

// scratch[.., i] = k_i * Q as XYZZ for i < n (n <= stride, the columns of the scratch array); flags: FB_F_IN_MONT
__global__ void __launch_bounds__(FB2_BLOCK) k_fb2_accumulate(const uint32_t* __restrict__ table, uint32_t c, uint32_t W,
                                                             const uint32_t* __restrict__ scalars, uint32_t n, uint32_t flags,
                                                             uint32_t* __restrict__ scratch, uint32_t stride) {
    const uint32_t i = blockIdx.x * FB2_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint4* q = reinterpret_cast<const uint4*>(scalars + (size_t)i * 8);
    const uint4 a = q[0], b = q[1];
    uint32_t k[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    if (flags & FB_F_IN_MONT) fb_scalar_from_mont(k);
    fb2_scratch_put(scratch, stride, i, fb2_mul_point(table, c, W, k));
}

// out[i] = the affine point of scratch[.., i] for i < n: lane t owns the chain fb2_chain_first(t, G) of G points; flags: FB_F_OUT_STD.
// (scratch is read and written -- the prefix slots -- by the lane that owns the point: no __restrict__)
__global__ void __launch_bounds__(FB2_BLOCK) k_fb2_normalise(uint32_t* scratch, uint32_t stride, uint32_t n, uint32_t G, uint32_t flags,
                                                            uint32_t* __restrict__ out_xy, uint8_t* __restrict__ out_inf) {
    const size_t first = fb2_chain_first((size_t)blockIdx.x * FB2_BLOCK + threadIdx.x, G);
    if (first >= n) return;
    const fp inv = fp_inv(fb2_chain_up(scratch, stride, first, G, n));  // < 1.02 in, < 2 out
    fb2_chain_down(scratch, stride, first, G, n, inv, out_xy, out_inf, (flags & FB_F_OUT_STD) != 0);
}

}  // namespace fbk
