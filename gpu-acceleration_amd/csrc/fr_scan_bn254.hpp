// fr_scan_bn254.hpp -- scans over the BN254 scalar field made in HBM: the value of a polynomial at z, its quotient by X - z (Horner's recurrence,
// a SUFFIX scan: the proof of a KZG opening is the MSM of that quotient) and the running product (a PREFIX scan: the grand product Z of PLONK and
// halo2).  The per-lane routines and the combine steps (__host__ __device__) and the kernels that run them.  tools/fr_scan_check.cpp runs the
// SAME routines on the CPU, the lanes of a workgroup emulated in a loop, under -DFP_BOUNDS_CHECK.
//
// Shape.  Lane t of a workgroup of FSC_BLOCK = 256 lanes owns the chain of G CONSECUTIVE elements (block * 256 + t) * G + s, s < G: a lane reads
// 32 G = 256 bytes at G = 8, two whole 128-byte lines that nobody else touches, so every fetched line is used.  A workgroup covers B = 256 G
// consecutive elements.  Three launches, none of which waits for another workgroup:
//   1 k_fsc_*_aggregate  a lane folds its chain (polynomial: Horner, acc = c + z acc from the top; product: p = p x from the bottom), the 256 lane
//                        values are combined in 8 steps, and the workgroup's aggregate goes to a scratch array (9 limbs, 36 bytes per block)
//   2 k_fsc_*_blocks     ONE workgroup walks the aggregates in rounds of 256 and replaces each by its block's carry-in: what the scan has
//                        gathered when it enters the block.  It writes the remainder / the value / the total.  An evaluation stops here.
//   3 k_fsc_*_apply      a workgroup repeats launch 1 with its carry-in injected into the lane the scan enters by (255 / 0), which gives every lane
//                        ITS carry-in; the lane then repeats its chain from there and writes the elements of its own chain.
// The combine step k takes the value of the lane 2^k further on (polynomial) or back (product).  Every chain has the same length, elements at or
// above n count as 0 (polynomial) or 1 (product), and a carry-in is injected BEFORE the steps instead of being spread after them, so the multiplier
// of step k is the same for all lanes: z^(G 2^k) in launches 1 and 3, z^(B 2^k) in launch 2.  The steps reach across the wavefronts of a
// workgroup (lane 63 takes lane 64's value in step 0), so the values change hands through LDS, two buffers of 256 x 9 words and one barrier per
// step, not through wavefront shuffles: a shuffle scan needs a second, lane-dependent multiplier z^(G (64 - lane)) to bring the other wavefronts in.
//
// In place.  A lane reads and writes the elements of its own chain only, and reads element i (again) before it writes element i: the quotient
// q[i] = S[i + 1] is the carry the lane holds when it arrives at i.  Everything from other lanes or blocks arrives through LDS or the scratch
// array.  So d_quot == d_coeffs and d_out == d_in need no copy, and no workgroup reads or writes a neighbour's range.
//
// Forms (fr_bn254.hpp: raw / rep).  Polynomial: the words are added AS LOADED, raw(c f) with f = 1 or 2^256, and multiplied by rep(z), which keeps
// the form; the store multiplies by post = rep(2^(256 (out_mont - in_mont))), canonical, which also reduces.  Product: x = word * pre with
// pre = rep(2^261 / f) is rep(element), products stay rep, the store multiplies by raw(f_out).  No element pays a separate conversion pass.
//
// Bounds (values in units of r; 2^261 ~ 169 r; fr_mul(A, B) < A B / 169 + 1, valid while both operands < 168.78).  A loaded word < 5.3.
//   polynomial chain    acc' = word + acc * z, z < 2: acc < 84 gives the product < 2, so acc' < 7.3
//   combine step        v' = v + other * m, m < 2, other < 84: the product < 2, so a value grows by < 2 per step
//   launch 1 / 3        a lane's value < 7.3 (lane 255 of launch 3 starts from a carry-in < 43.3: the same); after 8 steps < 23.3
//   launch 2            an aggregate < 23.3, plus carry * z^B < 2 in lane 255: < 25.3; after 8 steps < 41.3: carry-ins and the round's carry < 41.3
//   stores              value * post, value < 41.3, post < 1: < 41.3 / 169 + 1 < 2: fr_reduce_lt2r gives the canonical words
//   product             x = word * pre < 5.3 * 2 / 169 + 1 < 2; every product of two values < 2 is < 2 * 2 / 169 + 1 < 2; stores value * out < 2
//   host arguments      every power of z is a product of two values < 2: < 2
// No operand of an fr_mul here exceeds 41.3, far below the limit of 168.78.
#pragma once
#include "fr_vectors_bn254.hpp"

namespace fsck {

using namespace frvk;

constexpr uint32_t FSC_BLOCK = 256;      // lanes of a workgroup of every kernel here
constexpr uint32_t FSC_STEPS = 8;        // combine steps over the lanes of a workgroup
constexpr uint32_t FSC_CHAIN = 8;        // elements of one lane's chain
constexpr uint32_t FSC_CHAIN_SMALL = 1;  // hooks build only (msm_test_fr_scan_set_chain): a block is 256 elements, launch 2 takes a second round from 2^16 + 1 elements on
constexpr uint32_t FSC_MAX_LOG2 = 36;    // a call covers at most 2^36 elements
constexpr uint32_t FSC_AGG_WORDS = 9;    // a block's aggregate / carry-in in the scratch array: nine limbs, normalised
constexpr uint32_t FSC_EXCLUSIVE = 32;   // == MSM_FR_SCAN_EXCLUSIVE
static_assert(FSC_BLOCK == 1u << FSC_STEPS, "the combine steps cover a workgroup");

struct FscPlan {  // == msm_fr_scan_plan_t
    uint32_t chain;          // elements per lane
    uint32_t block_points;   // elements per workgroup
    uint32_t eval_launches;  // kernel launches of an evaluation
    uint32_t div_launches;   // ... of a division or a running product
    uint64_t blocks;         // workgroups of launches 1 and 3 for n
    uint64_t scratch_bytes;  // aggregates kept on the context for n
};
inline bool fsc_chain_ok(uint32_t G) { return G == FSC_CHAIN || G == FSC_CHAIN_SMALL; }
NTT_HD size_t fsc_blocks(size_t n, uint32_t G) { return (n + (size_t)FSC_BLOCK * G - 1) / ((size_t)FSC_BLOCK * G); }
inline FscPlan fsc_plan(size_t n, uint32_t G = FSC_CHAIN) {
    const size_t nb = fsc_blocks(n, G);
    return FscPlan{G, FSC_BLOCK * G, 2, 3, nb, (uint64_t)nb * FSC_AGG_WORDS * 4};
}

NTT_HD fr fsc_load9(const uint32_t* p, size_t i) {
    fr a;
#pragma unroll
    for (int k = 0; k < 9; k++) a.v[k] = p[i * FSC_AGG_WORDS + k];
    return a;
}
NTT_HD void fsc_store9(uint32_t* p, size_t i, const fr& a) {
#pragma unroll
    for (int k = 0; k < 9; k++) p[i * FSC_AGG_WORDS + k] = a.v[k];
}
NTT_HD void fsc_bound(const fr& a, uint32_t top) {  // a < top * 2^232 (r ~ 12.1 * 2^250: 84 r < 2^28 * 2^232); host builds under FP_BOUNDS_CHECK only
    FP_ASSERT(a.v[8] < top, "fr scan: a value leaves the bound its comment states");
    (void)a, (void)top;
}
constexpr uint32_t FSC_TOP_84 = 1u << 28;  // v[8] < 2^28: the value < 2^260 ~ 84.6 r

// ---- the polynomial: suffix sums S[j] = sum_{i >= j} c[i] z^(i - j) ---------------------------------------------------------------------------
struct FscPoly {
    fr z;                       // rep(z), < 2
    fr pw[2 * FSC_STEPS];       // z^(G 2^k): steps of launches 1 and 3 are pw[k], k < 8; launch 2 injects with pw[8] = z^B and steps with pw[8 + k]
    fr post;                    // canonical
};
inline FscPoly fsc_poly_args(const fr& z, uint32_t G, uint32_t flags) {
    FscPoly a;
    a.z = z;
    a.pw[0] = frv_pow_u64(z, G);
    for (uint32_t k = 1; k < 2 * FSC_STEPS; k++) a.pw[k] = fr_mul(a.pw[k - 1], a.pw[k - 1]);
    a.post = frv_lincomb_args(fr_one(), fr_one(), fr_one(), flags).post;
    return a;
}
// the chain of the lane whose first element is `first`, from the top: acc = S at the element behind the chain on entry, S[first] on return
template <uint32_t G>
NTT_HD fr fsc_poly_chain(const FscPoly& a, const uint32_t* in, size_t n, size_t first, fr acc) {
    for (uint32_t s = G; s-- > 0;) {
        const size_t i = first + s;
        if (i < n) {
            fsc_bound(acc, FSC_TOP_84);
            acc = fr_add(frv_load(in, i), fr_mul(acc, a.z));  // acc < 84, z < 2: < 5.3 + 2
        }
    }
    return acc;
}
// one combine step: mine + other * m (other: the value of the lane 2^k further on, < 84; m < 2)
NTT_HD fr fsc_poly_combine(const fr& mine, const fr& other, const fr& m) {
    fsc_bound(other, FSC_TOP_84);
    return fr_add(mine, fr_mul(other, m));  // grows by < 2
}
// the same chain once more, writing q[i] = S[i + 1] for its own elements
template <uint32_t G>
NTT_HD void fsc_poly_apply(const FscPoly& a, const uint32_t* in, uint32_t* out, size_t n, size_t first, fr acc) {
    for (uint32_t s = G; s-- > 0;) {
        const size_t i = first + s;
        if (i < n) {
            fsc_bound(acc, FSC_TOP_84);
            const fr w = frv_load(in, i);          // (out may be in: this lane alone touches element i, and reads it before it writes it)
            frv_store(out, i, fr_mul(acc, a.post));  // acc < 43.3, post < 1: < 2
            if (s) acc = fr_add(w, fr_mul(acc, a.z));  // < 7.3
        }
    }
}
// the value that leaves launch 2: S[0] in the output form
NTT_HD void fsc_poly_result(const FscPoly& a, uint32_t* out, const fr& s0) {
    fsc_bound(s0, FSC_TOP_84);
    frv_store(out, 0, fr_mul(s0, a.post));  // < 41.3 / 169 + 1
}

// ---- the running product: P[i] = prod_{j <= i} x[j] ------------------------------------------------------------------------------------------
struct FscProduct {
    fr pre;   // word * pre = rep(element)
    fr out;   // canonical; rep(x) * out = the words of x in the output form
    uint32_t exclusive;
};
inline FscProduct fsc_product_args(uint32_t flags) {
    return FscProduct{ntt_factor_in(flags), fr_canonical(frv_out_factor(flags)), (flags & FSC_EXCLUSIVE) ? 1u : 0u};
}
template <uint32_t G>
NTT_HD fr fsc_product_chain(const FscProduct& a, const uint32_t* in, size_t n, size_t first, fr run) {
    for (uint32_t s = 0; s < G; s++) {
        const size_t i = first + s;
        if (i < n) run = fr_mul(run, fr_mul(frv_load(in, i), a.pre));  // x < 5.3 * 2 / 169 + 1 < 2; run < 2: < 2
    }
    return run;
}
NTT_HD fr fsc_product_combine(const fr& mine, const fr& other) { return fr_mul(other, mine); }  // both < 2: < 2
template <uint32_t G>
NTT_HD void fsc_product_apply(const FscProduct& a, const uint32_t* in, uint32_t* out, size_t n, size_t first, fr run) {
    for (uint32_t s = 0; s < G; s++) {
        const size_t i = first + s;
        if (i < n) {
            const fr x = fr_mul(frv_load(in, i), a.pre);  // (out may be in: as above)
            if (a.exclusive) frv_store(out, i, fr_mul(run, a.out));  // run < 2, out < 1: < 2
            run = fr_mul(run, x);
            if (!a.exclusive) frv_store(out, i, fr_mul(run, a.out));
        }
    }
}
NTT_HD void fsc_product_result(const FscProduct& a, uint32_t* out, const fr& total) { frv_store(out, 0, fr_mul(total, a.out)); }

#if defined(__HIPCC__) && !defined(NTT_NO_KERNELS)
constexpr uint32_t FSC_LDS_WORDS = 2 * FSC_BLOCK * 9;  // two buffers of 256 values: 18 KiB

// The 8 combine steps over the 256 lanes of a workgroup.  SUFFIX: lane t takes lane t + 2^k (polynomial), else lane t - 2^k (product).  Step k
// writes buffer k & 1 and reads it behind ONE barrier: a lane that is a step ahead writes the other buffer, and nobody is two steps ahead of
// a lane that has not passed the barrier between.  Every lane of the workgroup must call this.
template <bool SUFFIX, class Step>
__device__ inline fr fsc_wg_scan(fr v, uint32_t* lds, Step step) {
    const uint32_t t = threadIdx.x;
#pragma unroll 1
    for (uint32_t k = 0; k < FSC_STEPS; k++) {
        uint32_t* buf = lds + (k & 1u) * (FSC_BLOCK * 9);
        const uint32_t d = 1u << k;
        ntt_lds_put(buf, t, v);
        __syncthreads();
        if (SUFFIX ? t + d < FSC_BLOCK : t >= d) v = step(v, ntt_lds_get(buf, SUFFIX ? t + d : t - d), k);
    }
    return v;
}
// after the steps: every lane's value to buffer 0 (last read in step 6; every lane has passed the barrier of step 7), so that a lane can take its
// neighbour's.  The caller puts a barrier behind its reads before the buffers are written again.
__device__ inline void fsc_wg_publish(const fr& v, uint32_t* lds) {
    ntt_lds_put(lds, threadIdx.x, v);
    __syncthreads();
}

// ---- launch 1 -----------------------------------------------------------------------------------------------------------------------------------
template <uint32_t G>
__global__ void __launch_bounds__(FSC_BLOCK) k_fsc_poly_aggregate(const FscPoly a, const uint32_t* in, size_t n, uint32_t* agg) {
    __shared__ uint32_t lds[FSC_LDS_WORDS];
    const size_t first = ((size_t)blockIdx.x * FSC_BLOCK + threadIdx.x) * G;
    fr v = fsc_poly_chain<G>(a, in, n, first, fr_zero());
    v = fsc_wg_scan<true>(v, lds, [&](const fr& mine, const fr& other, uint32_t k) { return fsc_poly_combine(mine, other, a.pw[k]); });
    if (threadIdx.x == 0) fsc_store9(agg, blockIdx.x, v);
}
template <uint32_t G>
__global__ void __launch_bounds__(FSC_BLOCK) k_fsc_product_aggregate(const FscProduct a, const uint32_t* in, size_t n, uint32_t* agg) {
    __shared__ uint32_t lds[FSC_LDS_WORDS];
    const size_t first = ((size_t)blockIdx.x * FSC_BLOCK + threadIdx.x) * G;
    fr v = fsc_product_chain<G>(a, in, n, first, fr_one());
    v = fsc_wg_scan<false>(v, lds, [&](const fr& mine, const fr& other, uint32_t) { return fsc_product_combine(mine, other); });
    if (threadIdx.x == FSC_BLOCK - 1) fsc_store9(agg, blockIdx.x, v);
}

// ---- launch 2: one workgroup; agg[b] becomes the carry-in of block b ------------------------------------------------------------------------------
__global__ void __launch_bounds__(FSC_BLOCK) k_fsc_poly_blocks(const FscPoly a, uint32_t* agg, size_t nb, uint32_t* d_result) {
    __shared__ uint32_t lds[FSC_LDS_WORDS];
    const uint32_t t = threadIdx.x;
    fr carry = fr_zero();  // S at the first element behind the round's blocks
    for (size_t round = (nb + FSC_BLOCK - 1) / FSC_BLOCK; round-- > 0;) {
        const size_t b = round * FSC_BLOCK + t;
        fr v = b < nb ? fsc_load9(agg, b) : fr_zero();
        if (t == FSC_BLOCK - 1) v = fsc_poly_combine(v, carry, a.pw[FSC_STEPS]);
        v = fsc_wg_scan<true>(v, lds, [&](const fr& mine, const fr& other, uint32_t k) { return fsc_poly_combine(mine, other, a.pw[FSC_STEPS + k]); });
        fsc_wg_publish(v, lds);
        const fr next = t + 1 < FSC_BLOCK ? ntt_lds_get(lds, t + 1) : carry;
        carry = ntt_lds_get(lds, 0);
        if (b < nb) fsc_store9(agg, b, next);
        __syncthreads();
    }
    if (t == 0 && d_result) fsc_poly_result(a, d_result, carry);
}
__global__ void __launch_bounds__(FSC_BLOCK) k_fsc_product_blocks(const FscProduct a, uint32_t* agg, size_t nb, uint32_t* d_result) {
    __shared__ uint32_t lds[FSC_LDS_WORDS];
    const uint32_t t = threadIdx.x;
    fr carry = fr_one();  // the product of everything before the round's blocks
    const size_t rounds = (nb + FSC_BLOCK - 1) / FSC_BLOCK;
    for (size_t round = 0; round < rounds; round++) {
        const size_t b = round * FSC_BLOCK + t;
        fr v = b < nb ? fsc_load9(agg, b) : fr_one();
        if (t == 0) v = fsc_product_combine(v, carry);
        v = fsc_wg_scan<false>(v, lds, [&](const fr& mine, const fr& other, uint32_t) { return fsc_product_combine(mine, other); });
        fsc_wg_publish(v, lds);
        const fr before = t ? ntt_lds_get(lds, t - 1) : carry;
        carry = ntt_lds_get(lds, FSC_BLOCK - 1);
        if (b < nb) fsc_store9(agg, b, before);
        __syncthreads();
    }
    if (t == 0 && d_result) fsc_product_result(a, d_result, carry);
}

// ---- launch 3 -----------------------------------------------------------------------------------------------------------------------------------
template <uint32_t G>
__global__ void __launch_bounds__(FSC_BLOCK) k_fsc_poly_apply(const FscPoly a, const uint32_t* in, uint32_t* out, size_t n, const uint32_t* agg) {
    __shared__ uint32_t lds[FSC_LDS_WORDS];
    const uint32_t t = threadIdx.x;
    const size_t first = ((size_t)blockIdx.x * FSC_BLOCK + t) * G;
    const fr carry = fsc_load9(agg, blockIdx.x);
    fr v = fsc_poly_chain<G>(a, in, n, first, t == FSC_BLOCK - 1 ? carry : fr_zero());
    v = fsc_wg_scan<true>(v, lds, [&](const fr& mine, const fr& other, uint32_t k) { return fsc_poly_combine(mine, other, a.pw[k]); });
    fsc_wg_publish(v, lds);  // every lane has read its chain: from here on the lanes write
    fsc_poly_apply<G>(a, in, out, n, first, t + 1 < FSC_BLOCK ? ntt_lds_get(lds, t + 1) : carry);
}
template <uint32_t G>
__global__ void __launch_bounds__(FSC_BLOCK) k_fsc_product_apply(const FscProduct a, const uint32_t* in, uint32_t* out, size_t n, const uint32_t* agg) {
    __shared__ uint32_t lds[FSC_LDS_WORDS];
    const uint32_t t = threadIdx.x;
    const size_t first = ((size_t)blockIdx.x * FSC_BLOCK + t) * G;
    const fr carry = fsc_load9(agg, blockIdx.x);
    fr v = fsc_product_chain<G>(a, in, n, first, t == 0 ? carry : fr_one());
    v = fsc_wg_scan<false>(v, lds, [&](const fr& mine, const fr& other, uint32_t) { return fsc_product_combine(mine, other); });
    fsc_wg_publish(v, lds);
    fsc_product_apply<G>(a, in, out, n, first, t ? ntt_lds_get(lds, t - 1) : carry);
}
#endif

}  // namespace fsck
