// fixed_base_g2_bn254.hpp -- BN254 G2 fixed-base batch multiplication, out[i] = k_i * Q for one base Q of the order-r subgroup of the twist: the
// plan, the window table of affine2 records, the product, and the normalisation of a chunk of XYZZ results by chain inversions.  __host__
// __device__ throughout: tools/fixed_base_g2_check.cpp runs the same routines on the CPU with -DFP_BOUNDS_CHECK; the kernels are
// msm_kernels_fixed_base_g2.hpp.  The digit recoding, the scalar conversion and the level scheme of the table are fixed_base_bn254.hpp's, used
// as they are (fb_next_digit, fb_scalar_from_mont, fb_num_windows, fb_table_index, fb_level_entries).
//
// Shape.  As in G1 a scalar is read as a 256-bit INTEGER and cut into W = ceil(257 / c) signed digits; the twist's cofactor is not 1, so
// k * Q = (k mod r) * Q only holds because the host has checked [r]Q = O (msm_fixed_base_g2.inc).  The table holds T_j[d] = d * 2^(c j) * Q for
// d = 1 .. 2^(c-1) as records of 32 words (x.c0 x.c1 y.c0 y.c1, canonical, internal domain), so a product is at most W mixed additions
// xyzz2_madd(acc, +-T_j[|d_j|]) (ec_g2_bn254.hpp: complete).  The operand is read from the table in front of every addition, so it is never
// loop-invariant (the trap of DESIGN.md 9b).  -T is (x, 2p - y) with both components of y NORMALISED (fp2_neg<2>, what k_g2_accumulate does): a
// raw negation may not meet the raw K*p - b.c1 inside fp2_mul, and the identity path of xyzz2_madd stores the operand.
//
// Two kernels per chunk.  A G2 accumulator is 72 registers, so the multiplication kernel leaves no room to hide a one-lane field inversion behind
// other workgroups; it stores its XYZZ result into a scratch array instead (fb2_scratch_*: word-major, word w of point i at scratch[w * stride + i],
// so the lanes of a wave touch neighbouring addresses), and a second kernel of Fq arithmetic only normalises:
//   1 / ZZZ = conj(ZZZ) / N,  N = ZZZ.c0^2 + ZZZ.c1^2 in Fq  (u^2 = -1; N != 0 for ZZZ != 0 because -1 is no square modulo p)
// EACH LANE runs Montgomery's trick over a chain of inv_group points of its own: prefix products up (one multiplication per point, the prefix parked
// in the ninth slot of the point's scratch record), ONE fp_inv, two multiplications per point down.  No barrier, no LDS, no private array.  Lane l
// of wave w owns the points (w * inv_group + s) * 64 + l for s < inv_group: at every step of the chain a wave reads and writes 64 neighbouring points.
// An identity (ZZ == 0; xyzz2_identity writes ZZZ == 0 with it, which is what the way up looks at) enters the chain as 1 and leaves flagged.
// From iz = 1 / ZZZ, as in G1:  t = ZZ * iz,  x = X * t^2,  y = Y * iz.
//
// Bounds (multiples of p per component, k = 0.0059; XYZZ records within ec_g2_bn254.hpp's X < 12, Y < 8, ZZ, ZZZ < 4.2) are written at each call.
#pragma once
#include "ec_g2_bn254.hpp"
#include "fixed_base_bn254.hpp"

namespace fbk {

constexpr uint32_t FB2_C_DEFAULT = 12;    // the fastest of the sweep 8, 10, 11, 12 at n = 2^20 although its 5.8 MB exceed the 4 MB of L2 of one XCD (profiles/fixed_base_g2_timing_mi355x.txt)
constexpr uint32_t FB2_REC_WORDS = 32;    // an affine2 table record, and an output record
constexpr uint32_t FB2_BLOCK = 256;       // lanes of a workgroup of k_fb2_accumulate / k_fb2_normalise
constexpr uint32_t FB2_WAVE = 64;         // lanes whose chains interleave
constexpr uint32_t FB2_INV_GROUP = 8;     // points of one chain = points that share one field inversion: the fastest of 8, 16, 32 (same file)
constexpr uint32_t FB2_SLOT_WORDS = 81;   // a scratch record: X Y ZZ ZZZ (8 x 9 limbs) and the chain's prefix product (9 limbs)
constexpr uint32_t FB2_PREFIX_WORD = 72;
constexpr uint32_t FB2_CHUNK = 1u << 18;  // points per pass through the scratch array (85 MB) and per staging step of the host-pointer call
static_assert(FB2_CHUNK % (FB2_WAVE * 32) == 0, "a chunk is whole waves of chains for every inv_group up to 32");

struct Fb2Plan {  // == msm_fixed_base_g2_plan_t
    uint32_t window_bits, num_windows;
    uint64_t table_entries, table_bytes;
    uint32_t inv_group, chunk_points;
    uint64_t scratch_bytes;
};
struct Fb2Base {  // the base as arkworks Montgomery words (x.c0, x.c1, y.c0, y.c1), a kernel argument
    uint32_t w[32];
};

// false: window_bits is neither 0 (the default) nor in FB_C_MIN .. FB_C_MAX
inline bool fb2_plan(uint32_t window_bits, Fb2Plan& p) {
    const uint32_t c = window_bits ? window_bits : FB2_C_DEFAULT;
    if (c < FB_C_MIN || c > FB_C_MAX) return false;
    p.window_bits = c;
    p.num_windows = fb_num_windows(c);
    p.table_entries = (uint64_t)p.num_windows << (c - 1);
    p.table_bytes = p.table_entries * FB2_REC_WORDS * 4;
    p.inv_group = FB2_INV_GROUP;
    p.chunk_points = FB2_CHUNK;
    p.scratch_bytes = (uint64_t)FB2_CHUNK * FB2_SLOT_WORDS * 4;
    return true;
}

FP_HD fp fb2_load_fp8(const uint32_t* p) {  // 16-byte aligned
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    return fp_unpack(w);
}
FP_HD affine2 fb2_load_affine(const uint32_t* rec) {
    return affine2{fp2{fb2_load_fp8(rec), fb2_load_fp8(rec + 8)}, fp2{fb2_load_fp8(rec + 16), fb2_load_fp8(rec + 24)}};
}
// an affine point (internal domain, components < 128p) as a table record
FP_HD void fb2_store_record(uint32_t* rec, const affine2& a) {
    const fp* c[4] = {&a.x.c0, &a.x.c1, &a.y.c0, &a.y.c1};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t w[8];
        fp_pack(w, fp_canonical(*c[k]));
        fb_store_words8(rec + 8 * k, w);
    }
}
// the base's Montgomery words as an affine operand: components canonical
FP_HD affine2 fb2_base_affine(const uint32_t w[32]) {
    return affine2{fp2{fp_reduce_lt2p(fp_from_mont256(w)), fp_reduce_lt2p(fp_from_mont256(w + 8))},            // fp_mul gives < 1.01: below 2p
                   fp2{fp_reduce_lt2p(fp_from_mont256(w + 16)), fp_reduce_lt2p(fp_from_mont256(w + 24))}};
}
FP_HD xyzz2 fb2_from_affine(const affine2& a) { return xyzz2{a.x, a.y, fp2_one(), fp2_one()}; }

// k * Q from the table; k is consumed
FP_HD xyzz2 fb2_mul_point(const uint32_t* table, uint32_t c, uint32_t W, uint32_t k[8]) {
    xyzz2 acc = xyzz2_identity();
    uint32_t carry = 0;
    for (uint32_t j = 0; j < W; j++) {
        const int32_t d = fb_next_digit(k, c, carry);
        if (d == 0) continue;
        affine2 a = fb2_load_affine(table + fb_table_index(j, (uint32_t)(d < 0 ? -d : d), c) * FB2_REC_WORDS);  // x, y canonical: < 1
        if (d < 0) a.y = fp2_neg<2>(a.y);  // 2p - y < 2, normalised
        xyzz2_madd(acc, a);
    }
    FP_ASSERT(carry == 0, "fixed base G2: the top window carries out (W * c < 257)");
    return acc;
}
// 2^(c j) * Q: the base of window j
FP_HD xyzz2 fb2_window_base(const affine2& q, uint32_t c, uint32_t j) {
    xyzz2 acc = fb2_from_affine(q);
    for (uint32_t i = 0; i < c * j; i++) acc = xyzz2_dbl(acc);
    return acc;
}
// item e < fb_level_entries(W, L) of level L (fixed_base_bn254.hpp's scheme): T_j[t] + T_j[2^(L-1)], and the index of the record it becomes.
// t == 2^(L-1) adds the record to itself: the complete formula doubles.
FP_HD xyzz2 fb2_table_step(const uint32_t* table, uint32_t c, uint32_t L, uint32_t e, size_t& dst) {
    const uint32_t half = 1u << (L - 1), j = e >> (L - 1), t = (e & (half - 1u)) + 1u;  // t in 1 .. 2^(L-1)
    xyzz2 acc = fb2_from_affine(fb2_load_affine(table + fb_table_index(j, t, c) * FB2_REC_WORDS));
    xyzz2_madd(acc, fb2_load_affine(table + fb_table_index(j, half, c) * FB2_REC_WORDS));
    dst = fb_table_index(j, half + t, c);
    return acc;
}

// N = ZZZ.c0^2 + ZZZ.c1^2:  2 * (4.2^2 k + 1) < 2.3
FP_HD fp fb2_norm(const fp2& zzz) { return fp_add(fp_sqr(zzz.c0), fp_sqr(zzz.c1)); }
// 1 / ZZZ = conj(ZZZ) * ni from ni = 1 / N (< 2):  4.2 * 2k + 1 < 1.05 and (6p - c1, raw: one factor of a product whose other one is normalised) 6 * 2k + 1 < 1.08
FP_HD fp2 fb2_inv_from_norm(const fp2& zzz, const fp& ni) { return fp2{fp_mul(zzz.c0, ni), fp_mul(fp_neg_raw_k<6>(zzz.c1), ni)}; }
// x = X / ZZ, y = Y / ZZZ from iz = 1 / ZZZ (< 1.08)
FP_HD affine2 fb2_to_affine(const xyzz2& p, const fp2& iz) {
    const fp2 t = fp2_mul<3>(p.zz, iz);       // iz.c1 < 2p;  4.2 * 3.2k + 1 < 1.08
    const fp2 t2 = fp2_sqr<3>(t);             // t.c1 < 2p;   2.2 * 3.2k + 1 < 1.05
    return affine2{fp2_mul<3>(p.x, t2),       // t2.c1 < 2p;  12 * 3.1k + 1 < 1.23
                   fp2_mul<3>(p.y, iz)};      // 8 * 3.2k + 1 < 1.16
}
FP_HD void fb2_store_component(uint32_t* out, const fp& v, bool out_std) {  // internal, < 128p -> 8 canonical words
    uint32_t w[8];
    if (out_std) fp_to_std(w, v);
    else fp_to_mont256(w, v);
    fb_store_words8(out, w);
}
// the output record of one point: canonical standard or arkworks Montgomery words, all zero for the identity
FP_HD void fb2_store_output(uint32_t* out_xy, uint8_t* out_inf, const xyzz2& p, const fp2& iz, bool identity, bool out_std) {
    if (identity) {
        const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        fb_store_words8(out_xy, z), fb_store_words8(out_xy + 8, z), fb_store_words8(out_xy + 16, z), fb_store_words8(out_xy + 24, z);
    } else {
        const affine2 a = fb2_to_affine(p, iz);
        fb2_store_component(out_xy, a.x.c0, out_std), fb2_store_component(out_xy + 8, a.x.c1, out_std);
        fb2_store_component(out_xy + 16, a.y.c0, out_std), fb2_store_component(out_xy + 24, a.y.c1, out_std);
    }
    *out_inf = identity ? 1 : 0;
}

// ---- the scratch array of one chunk: FB2_SLOT_WORDS rows of `stride` words, point i in column i ----
FP_HD void fb2_scratch_put_fp(uint32_t* s, size_t stride, size_t i, uint32_t word, const fp& v) {
#pragma unroll
    for (int k = 0; k < 9; k++) s[(size_t)(word + k) * stride + i] = v.v[k];
}
FP_HD fp fb2_scratch_get_fp(const uint32_t* s, size_t stride, size_t i, uint32_t word) {
    fp r;
#pragma unroll
    for (int k = 0; k < 9; k++) r.v[k] = s[(size_t)(word + k) * stride + i];
    return r;
}
FP_HD void fb2_scratch_put(uint32_t* s, size_t stride, size_t i, const xyzz2& p) {
    const fp* c[8] = {&p.x.c0, &p.x.c1, &p.y.c0, &p.y.c1, &p.zz.c0, &p.zz.c1, &p.zzz.c0, &p.zzz.c1};
#pragma unroll
    for (int k = 0; k < 8; k++) fb2_scratch_put_fp(s, stride, i, 9u * k, *c[k]);
}
FP_HD fp2 fb2_scratch_get_zzz(const uint32_t* s, size_t stride, size_t i) {
    return fp2{fb2_scratch_get_fp(s, stride, i, 54), fb2_scratch_get_fp(s, stride, i, 63)};
}
FP_HD xyzz2 fb2_scratch_get(const uint32_t* s, size_t stride, size_t i) {
    return xyzz2{fp2{fb2_scratch_get_fp(s, stride, i, 0), fb2_scratch_get_fp(s, stride, i, 9)},
                 fp2{fb2_scratch_get_fp(s, stride, i, 18), fb2_scratch_get_fp(s, stride, i, 27)},
                 fp2{fb2_scratch_get_fp(s, stride, i, 36), fb2_scratch_get_fp(s, stride, i, 45)}, fb2_scratch_get_zzz(s, stride, i)};
}

// ---- one lane's chain: the points first + s * FB2_WAVE for s < G that lie below n (n <= stride) ----
FP_HD size_t fb2_chain_first(size_t lane_global, uint32_t G) { return (lane_global / FB2_WAVE) * ((size_t)FB2_WAVE * G) + lane_global % FB2_WAVE; }
FP_HD size_t fb2_chain_lanes(size_t n, uint32_t G) { return (n + (size_t)FB2_WAVE * G - 1) / ((size_t)FB2_WAVE * G) * FB2_WAVE; }
// the way up: every point's prefix slot gets the product of the norms in front of it; returns the product of all (1 for an empty chain)
FP_HD fp fb2_chain_up(uint32_t* s, size_t stride, size_t first, uint32_t G, size_t n) {
    fp run = fp_one();
    for (uint32_t st = 0; st < G; st++) {
        const size_t i = first + (size_t)st * FB2_WAVE;
        if (i >= n) break;
        const fp2 zzz = fb2_scratch_get_zzz(s, stride, i);
        fb2_scratch_put_fp(s, stride, i, FB2_PREFIX_WORD, run);
        if (!fp2_is_zero_exact(zzz)) run = fp_mul(run, fb2_norm(zzz));  // 1.02 * 2.3k + 1 < 1.02
    }
    return run;
}
// the way down from inv = 1 / (the product): every point of the chain leaves as its output record
FP_HD void fb2_chain_down(const uint32_t* s, size_t stride, size_t first, uint32_t G, size_t n, fp inv, uint32_t* out_xy, uint8_t* out_inf,
                          bool out_std) {
    for (uint32_t st = G; st-- > 0;) {
        const size_t i = first + (size_t)st * FB2_WAVE;
        if (i >= n) continue;
        const xyzz2 p = fb2_scratch_get(s, stride, i);
        const bool identity = xyzz2_is_identity(p);
        FP_ASSERT(identity == fp2_is_zero_exact(p.zzz), "fixed base G2: ZZ and ZZZ disagree about the identity");
        fp2 iz = fp2_zero();
        if (!identity) {
            const fp nrm = fb2_norm(p.zzz);                                                    // < 2.3
            const fp ni = fp_mul(inv, fb2_scratch_get_fp(s, stride, i, FB2_PREFIX_WORD));      // 2 * 1.02k + 1 < 1.02
            inv = fp_mul(inv, nrm);                                                            // 2 * 2.3k + 1 < 1.03
            iz = fb2_inv_from_norm(p.zzz, ni);
        }
        fb2_store_output(out_xy + i * FB2_REC_WORDS, out_inf + i, p, iz, identity, out_std);
    }
}

}  // namespace fbk
