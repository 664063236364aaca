// fixed_base_bn254.hpp -- BN254 G1 fixed-base batch multiplication, out[i] = k_i * P: the plan, the digit recoding, the window table of one base and
// the batch inversion (Montgomery's trick over one workgroup) that both the table build and the multiplication end with.  __host__ __device__
// throughout: tools/fixed_base_check.cpp runs the same routines on the CPU with -DFP_BOUNDS_CHECK; the kernels are msm_kernels_fixed_base.hpp.
//
// Shape.  A scalar is read as a 256-bit INTEGER k (no reduction modulo r: P has order r, so k * P = (k mod r) * P) and cut into W = ceil(257 / c)
// signed digits d_j in [-2^(c-1), 2^(c-1)], k = sum d_j * 2^(c j); the 257th bit takes the carry of the top window.  The table holds
// T_j[d] = d * 2^(c j) * P for d = 1 .. 2^(c-1) as affine records (16 words: x, y canonical in the internal domain, what load_affine reads), so a
// product is at most W mixed additions xyzz_madd(acc, +-T_j[|d_j|]) (ec_bn254.hpp: complete; the sign goes through the raw negation of y) and a
// zero digit costs nothing.
//
// Batch inversion.  The FB_GROUP lanes of a workgroup keep their accumulators in registers and put ZZZ into a product tree in LDS (a heap of
// 2 * FB_GROUP nodes, limb-major): FB_GROUP - 1 multiplications up, ONE fp_inv of the root, 2 * (FB_GROUP - 1) multiplications down, 3 per
// point and 2 * log2(FB_GROUP) levels deep -- prefix products in tree order (a serial prefix chain would leave one lane to do 3 * FB_GROUP
// dependent multiplications).  An identity (ZZ == 0) enters as 1 and leaves flagged.  From iz = 1 / ZZZ:
//     t = iz * ZZ = ZZ / ZZZ,   1 / ZZ = t^2  (ZZ^2 / ZZZ^2 = ZZ^2 / ZZ^3),   x = X * t^2,   y = Y * iz          -- 3M + 1S, exact.
// Bounds (multiples of p, ec_bn254.hpp): leaves are ZZZ < 2 or 1; every node is a product of two values < 2, so < 1.03; fp_inv takes and gives < 2.
#pragma once
#include "ec_bn254.hpp"
#include "fr_bn254.hpp"

namespace fbk {

using namespace bn254;

constexpr uint32_t FB_GROUP = 256;     // lanes of a workgroup = points that share one field inversion
constexpr uint32_t FB_C_MIN = 4, FB_C_MAX = 16;
constexpr uint32_t FB_C_DEFAULT = 12;  // the fastest of the sweep 6, 8, 10, 12 at n = 2^20 (profiles/fixed_base_timing_mi355x.txt)
constexpr uint32_t FB_BITS = 257;      // signed digits of a 256-bit integer may carry one bit out
constexpr uint32_t FB_MAX_WINDOWS = (FB_BITS + FB_C_MIN - 1) / FB_C_MIN;  // 65
constexpr uint32_t FB_REC_WORDS = 16;  // an affine table record
constexpr uint32_t FB_TREE_WORDS = 2 * FB_GROUP * 9;                      // the product tree of one workgroup (18 KB)
constexpr uint32_t FB_F_IN_MONT = 2u, FB_F_OUT_STD = 8u;                  // == MSM_NTT_IN_MONT, MSM_FB_OUT_STD of include/msm_hip.h

struct FbPlan {  // == msm_fixed_base_plan_t
    uint32_t window_bits, num_windows;
    uint64_t table_entries, table_bytes;
    uint32_t inv_group, reserved;
};
struct FbBase {  // the base as arkworks Montgomery words (x, y), a kernel argument
    uint32_t w[16];
};

FP_HD uint32_t fb_num_windows(uint32_t c) { return (FB_BITS + c - 1) / c; }
// false: window_bits is neither 0 (the default) nor in FB_C_MIN .. FB_C_MAX
inline bool fb_plan(uint32_t window_bits, FbPlan& p) {
    const uint32_t c = window_bits ? window_bits : FB_C_DEFAULT;
    if (c < FB_C_MIN || c > FB_C_MAX) return false;
    p.window_bits = c;
    p.num_windows = fb_num_windows(c);
    p.table_entries = (uint64_t)p.num_windows << (c - 1);
    p.table_bytes = p.table_entries * FB_REC_WORDS * 4;
    p.inv_group = FB_GROUP;
    p.reserved = 0;
    return true;
}

// arkworks Fr.0 words (k * 2^256 mod r, any 256-bit pattern) -> the canonical integer k: one fr_mul by raw(2^5), w * 2^5 * 2^-261 = w * 2^-256
FP_HD void fb_scalar_from_mont(uint32_t k[8]) {
    fr f = fr_zero();
    f.v[0] = 32;
    fr_pack(k, fr_reduce_lt2r(fr_mul(fr_unpack(k), f)));  // < 2^256 * 32 / 2^261 + r < 2r
}
// the next signed digit of k (least significant first); k is shifted right by c (static indices only: the words stay in registers)
FP_HD int32_t fb_next_digit(uint32_t k[8], uint32_t c, uint32_t& carry) {
    const uint32_t H = 1u << (c - 1), v = (k[0] & (2u * H - 1u)) + carry;
#pragma unroll
    for (int i = 0; i < 7; i++) k[i] = (k[i] >> c) | (k[i + 1] << (32 - c));  // c in 4 .. 16
    k[7] >>= c;
    carry = v > H ? 1u : 0u;  // v == H stays a positive digit: |d| <= 2^(c-1)
    return carry ? (int32_t)v - (int32_t)(2u * H) : (int32_t)v;
}
// record of T_j[d], d in 1 .. 2^(c-1)
FP_HD size_t fb_table_index(uint32_t j, uint32_t d, uint32_t c) { return ((size_t)j << (c - 1)) + (d - 1); }

FP_HD affine fb_load_affine(const uint32_t* rec) {  // 16-byte aligned
    const uint4* q = reinterpret_cast<const uint4*>(rec);
    const uint4 a = q[0], b = q[1], e = q[2], f = q[3];
    const uint32_t wx[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, wy[8] = {e.x, e.y, e.z, e.w, f.x, f.y, f.z, f.w};
    return affine{fp_unpack(wx), fp_unpack(wy)};
}
FP_HD void fb_store_words8(uint32_t* p, const uint32_t w[8]) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// an affine point (internal domain, < 128p) as a table record
FP_HD void fb_store_record(uint32_t* rec, const affine& a) {
    uint32_t w[8];
    fp_pack(w, fp_canonical(a.x));
    fb_store_words8(rec, w);
    fp_pack(w, fp_canonical(a.y));
    fb_store_words8(rec + 8, w);
}

// k * P from the table; k is consumed
FP_HD xyzz fb_mul_point(const uint32_t* table, uint32_t c, uint32_t W, uint32_t k[8]) {
    xyzz acc = xyzz_identity();
    uint32_t carry = 0;
    for (uint32_t j = 0; j < W; j++) {
        const int32_t d = fb_next_digit(k, c, carry);
        if (d == 0) continue;
        affine a = fb_load_affine(table + fb_table_index(j, (uint32_t)(d < 0 ? -d : d), c) * FB_REC_WORDS);
        if (d < 0) a.y = fp_neg_raw<2>(a.y);  // y canonical: 2p - y, raw (xyzz_madd)
        xyzz_madd(acc, a);
    }
    FP_ASSERT(carry == 0, "fixed base: the top window carries out (W * c < 257)");
    return acc;
}
// 2^(c j) * P: the base of window j
FP_HD xyzz fb_window_base(const affine& p, uint32_t c, uint32_t j) {
    xyzz acc = xyzz_from_affine(p);
    for (uint32_t i = 0; i < c * j; i++) acc = xyzz_dbl(acc);
    return acc;
}
// The table of window j grows level by level from T_j[1] = 2^(c j) * P: level L = 1 .. c-1 makes the 2^(L-1) entries d in (2^(L-1), 2^L] as
// T_j[d - 2^(L-1)] + T_j[2^(L-1)], ONE mixed addition of two records of earlier levels (d = 2^L adds the record to itself: the complete formula
// doubles).  A level reads entries <= 2^(L-1) and writes entries above: no lane of a launch reads what another writes.
FP_HD uint32_t fb_level_entries(uint32_t W, uint32_t L) { return W << (L - 1); }
// item e < fb_level_entries(W, L) of level L: the sum, and the index of the record it becomes
FP_HD xyzz fb_table_step(const uint32_t* table, uint32_t c, uint32_t L, uint32_t e, size_t& dst) {
    const uint32_t half = 1u << (L - 1), j = e >> (L - 1), t = (e & (half - 1u)) + 1u;  // t in 1 .. 2^(L-1)
    xyzz acc = xyzz_from_affine(fb_load_affine(table + fb_table_index(j, t, c) * FB_REC_WORDS));
    xyzz_madd(acc, fb_load_affine(table + fb_table_index(j, half, c) * FB_REC_WORDS));
    dst = fb_table_index(j, half + t, c);
    return acc;
}

// ---- the product tree: node v of 1 .. 2G-1, leaves G .. 2G-1, limb-major so that neighbouring lanes touch neighbouring banks ----
FP_HD void fb_node_put(uint32_t* t, uint32_t node, const fp& v) {
#pragma unroll
    for (int i = 0; i < 9; i++) t[(uint32_t)i * (2 * FB_GROUP) + node] = v.v[i];
}
FP_HD fp fb_node_get(const uint32_t* t, uint32_t node) {
    fp r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = t[(uint32_t)i * (2 * FB_GROUP) + node];
    return r;
}
// the phases, each by `lane`, a barrier between them (fb_batch_inverse of msm_kernels_fixed_base.hpp; fb_batch_inverse_host below)
FP_HD void fb_inv_enter(uint32_t* t, uint32_t lane, const fp& zzz, bool identity) { fb_node_put(t, FB_GROUP + lane, identity ? fp_one() : zzz); }
FP_HD void fb_inv_up(uint32_t* t, uint32_t s, uint32_t lane) {  // level of s nodes, lane < s
    const uint32_t v = s + lane;
    fb_node_put(t, v, fp_mul(fb_node_get(t, 2 * v), fb_node_get(t, 2 * v + 1)));
}
FP_HD void fb_inv_root(uint32_t* t) { fb_node_put(t, 1, fp_inv(fb_node_get(t, 1))); }
FP_HD void fb_inv_down(uint32_t* t, uint32_t s, uint32_t lane) {  // node v holds 1 / (its product): 1 / left = that * right, 1 / right = that * left
    const uint32_t v = s + lane;
    const fp iv = fb_node_get(t, v), l = fb_node_get(t, 2 * v), r = fb_node_get(t, 2 * v + 1);
    fb_node_put(t, 2 * v, fp_mul(iv, r));
    fb_node_put(t, 2 * v + 1, fp_mul(iv, l));
}
FP_HD fp fb_inv_leave(const uint32_t* t, uint32_t lane) { return fb_node_get(t, FB_GROUP + lane); }

// x = X / ZZ, y = Y / ZZZ from iz = 1 / ZZZ (internal domain, < 2p)
FP_HD affine fb_to_affine(const xyzz& p, const fp& iz) {
    const fp t = fp_mul(iz, p.zz);
    return affine{fp_mul(p.x, fp_sqr(t)), fp_mul(p.y, iz)};
}
// the output record of one point: canonical standard or arkworks Montgomery words, all zero for the identity
FP_HD void fb_store_output(uint32_t* out_xy, uint8_t* out_inf, const xyzz& p, const fp& iz, bool identity, bool out_std) {
    uint32_t wx[8] = {0, 0, 0, 0, 0, 0, 0, 0}, wy[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!identity) {
        const affine a = fb_to_affine(p, iz);
        if (out_std) {
            fp_to_std(wx, a.x);
            fp_to_std(wy, a.y);
        } else {
            fp_to_mont256(wx, a.x);
            fp_to_mont256(wy, a.y);
        }
    }
    fb_store_words8(out_xy, wx);
    fb_store_words8(out_xy + 8, wy);
    *out_inf = identity ? 1 : 0;
}

// the phases in the kernels' order for one group on the host: iz[l] = 1 / zzz[l], or 1 where identity[l].  t: FB_TREE_WORDS words.
inline void fb_batch_inverse_host(uint32_t* t, const fp* zzz, const bool* identity, fp* iz) {
    for (uint32_t l = 0; l < FB_GROUP; l++) fb_inv_enter(t, l, zzz[l], identity[l]);
    for (uint32_t s = FB_GROUP / 2; s >= 1; s >>= 1)
        for (uint32_t l = 0; l < s; l++) fb_inv_up(t, s, l);
    fb_inv_root(t);
    for (uint32_t s = 1; s < FB_GROUP; s <<= 1)
        for (uint32_t l = 0; l < s; l++) fb_inv_down(t, s, l);
    for (uint32_t l = 0; l < FB_GROUP; l++) iz[l] = fb_inv_leave(t, l);
}

}  // namespace fbk
