/*
 * msm_hip_testhooks.h -- test, benchmark and calibration hooks of the MI355X BN254 G1 MSM engine.
 *
 * NOT part of the product ABI: these symbols exist only in libmsm_hip_hooks.so, a second build of the same sources with
 * -DMSM_HIP_TEST_HOOKS (make -C gpu-acceleration_amd/csrc hooks).  That library also contains the complete engine
 * (include/msm_hip.h), so a hooks context runs exactly the kernels the product runs.  Users: tests/, bench.py (input
 * generation, multiplier calibration), tools/.
 */
#ifndef MSM_HIP_TESTHOOKS_H
#define MSM_HIP_TESTHOOKS_H
#include "msm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- synthetic inputs: counterpart of test_utils::generate_random_bases_and_scalars
 *      (metal_msm.rs:698-731).  Base i is k_i*G with k_i = SplitMix64 stream (seed, i) reduced below r,
 *      scalar i likewise from scalar_seed; both written to DEVICE memory (Montgomery bases). ------- */
int32_t msm_bn254_g1_generate_device(msm_ctx *ctx, uint64_t base_seed, uint64_t scalar_seed, size_t n,
                                     void *d_bases_mont_out, void *d_scalars_out);
/* the same k_i / s_i streams on the host (8 words each), for closed-form checks */
int32_t msm_bn254_generate_scalars_host(uint64_t seed, size_t n, int nonzero, uint32_t *out);

/* ---- device-math unit-test hooks: counterpart of the reference's test_* kernels (SURVEY C10,
 *      e.g. mont_mul_cios.metal:8-15, jacobian_add_2007_bl.metal:8-40).  Host arrays in/out. ------ */
#define MSM_OP_FP_ADD 0u
#define MSM_OP_FP_SUB 1u
#define MSM_OP_FP_MONT_MUL 2u
#define MSM_OP_FP_TO_MONT 3u
#define MSM_OP_FP_FROM_MONT 4u
#define MSM_OP_FP_INV 5u
int32_t msm_test_fp_op(msm_ctx *ctx, uint32_t op, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n);
#define MSM_OP_G1_MADD 0u /* a: Jacobian(24) + b: affine Montgomery(16) -> Jacobian(24) */
#define MSM_OP_G1_ADD 1u  /* a: Jacobian(24) + b: Jacobian(24)          -> Jacobian(24) */
#define MSM_OP_G1_DBL 2u  /* a: Jacobian(24)                            -> Jacobian(24) */
#define MSM_OP_G1_ADD_WIDE 3u /* as ADD, computed by 8 cooperating lanes (csrc/ec_wide.hpp, the reduction-tree path) */
#define MSM_OP_G1_MADD_M256 4u     /* as MADD, b's arkworks words gathered as they are (fp_unpack_shl5 + xyzz_madd_m32: k_accumulate_pieces<.., M256>) */
#define MSM_OP_G1_MADD_M256_NEG 5u /* a - b by the same path (the digit's sign applied to S2) */
int32_t msm_test_g1_op(msm_ctx *ctx, uint32_t op, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n);
/* the G1 group law of csrc/ec_bn254.hpp / csrc/ec_wide.hpp on RAW limb records: n elements, no conversion and no reduction on the way in or out
 * (msm_test_g1_op above only ever hands the law freshly reduced operands).  A record is 9 limbs of 29 bits per coordinate (one u32 word per limb,
 * least significant first; value = sum limb_i * 2^(29 i)), internal Montgomery domain (x * 2^261 mod p, plus any multiple of p the bounds of
 * ec_bn254.hpp allow: X < 7p, Y < 5p, ZZ, ZZZ < 2p; affine x < p, y < 2p).  XYZZ record: X Y ZZ ZZZ (36 words, the layout of store_xyzz); affine
 * record: x y (18 words); the M256 operations take b as 16 words, x then y, ANY 32-bit values (the caller's R = 2^256 words as they are).  The
 * identity is ZZ == 0 with every limb zero.  The caller picks the representative the device computes on and reads back exactly the limbs it stored.
 * An input limb >= 2^29 is MSM_ERR_BAD_ARG (the 16-word b of the M256 operations is exempt); the bounds above are the caller's to keep. */
#define MSM_OP_G1_RAW_MADD 0u          /* a: XYZZ record (36) + b: affine record (18) -> 36, xyzz_madd */
#define MSM_OP_G1_RAW_MADD_NEG_RAW 1u  /* a - b: the kernel applies fp_neg_raw<2> to the y it loaded, then xyzz_madd (a negative digit in k_accumulate_pieces) */
#define MSM_OP_G1_RAW_MADD_M256 2u     /* a: 36 + b: 16 words -> 36, xyzz_madd_m32 on fp_unpack_shl5 of the words */
#define MSM_OP_G1_RAW_MADD_M256_NEG 3u /* a - b by the same path */
#define MSM_OP_G1_RAW_ADD 4u           /* a: 36 + b: 36 -> 36, xyzz_add */
#define MSM_OP_G1_RAW_DBL 5u           /* a: 36 -> 36, xyzz_dbl */
#define MSM_OP_G1_RAW_ADD_WIDE_LDS 6u  /* as ADD by eight lanes per pair, records staged in LDS and added in place (lds_tree_wide's call) */
#define MSM_OP_G1_RAW_ADD_WIDE_HBM 7u  /* as ADD by eight lanes per pair, records in global memory, distinct output (k_pair_level_wide's call) */
int32_t msm_test_g1_raw_op(msm_ctx *ctx, uint32_t op, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n);
/* the root-and-sign routine of k_g2_decompress on arbitrary Fq2 values (curve points whose y has a zero component cannot be constructed in closed
 * form: this is how the c1 = 0 / c0 = 0 branches of the sign rule get tested).  a_std: n x 16 standard-form words (c0, c1; canonical);
 * want_larger: n bytes (non-zero: the root that is the larger of (y, -y), see msm_bn254_g2_compress); out_std: n x 16 standard-form words of the
 * root (zero when there is none); ok: n bytes, 1 = a is a square. */
int32_t msm_test_g2_sqrt(msm_ctx *ctx, const uint32_t *a_std, const uint8_t *want_larger, uint32_t *out_std, uint8_t *ok, size_t n);
/* the G2 group law of csrc/ec_g2_bn254.hpp on RAW limb records: n elements, one device lane each, no conversion and no reduction on the way in or
 * out.  A record is 9 limbs of 29 bits per Fq component (one u32 word per limb, least significant first; value = sum limb_i * 2^(29 i)), internal
 * Montgomery domain (x * 2^261 mod p, plus any multiple of p the bounds of ec_g2_bn254.hpp allow: X < 12p, Y < 8p, ZZ, ZZZ < 4.2p; affine x < p,
 * y < 2p).  XYZZ record: X.c0 X.c1 Y.c0 Y.c1 ZZ.c0 ZZ.c1 ZZZ.c0 ZZZ.c1 (72 words); affine record: x.c0 x.c1 y.c0 y.c1 (36 words).  The identity is
 * ZZ == 0 with every limb zero.  The caller picks the representative the device computes on and reads back exactly the limbs it produced.
 * An input limb >= 2^29 is MSM_ERR_BAD_ARG (the bounds above are the caller's to keep: the device asserts nothing). */
#define MSM_OP_G2_MADD 0u /* a: XYZZ record (72) + b: affine record (36) -> XYZZ record (72) */
#define MSM_OP_G2_ADD 1u  /* a: 72 + b: 72 -> 72 */
#define MSM_OP_G2_DBL 2u  /* a: 72 -> 72 */
int32_t msm_test_g2_op(msm_ctx *ctx, uint32_t op, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n);
/* the scalar field Fr of csrc/fr_bn254.hpp on RAW limb records: n elements, one device lane each, no conversion and no reduction on the way in or
 * out.  a, b and out hold n x 9 words: 9 limbs of 29 bits (one u32 word per limb, least significant first; value = sum limb_i * 2^(29 i)), ANY
 * representative the value discipline of fr_bn254.hpp allows for the operation.  Where a function reads or writes 8 words (32-bit words of a
 * 256-bit pattern), word 8 is ignored on input and written as 0 on output.  b is read by MUL, ADD, SUB<K> (a second record) and POW_U32 (the
 * exponent in b[i][0], words 1..8 ignored); the other operations take b == NULL.  The caller picks the representative the device computes on and
 * reads back exactly the limbs it stored.  A limb >= 2^29 in an operand that must be normalised is MSM_ERR_BAD_ARG (a of NORMALIZE, UNPACK and
 * FROM_STD takes any 32-bit words); the value bounds are the caller's to keep: the device asserts nothing. */
#define MSM_OP_FR_RAW_MUL 0u          /* fr_mul(a, b): a * b * 2^-261, needs a * b < (2^261 - r) * 2^261 */
#define MSM_OP_FR_RAW_ADD 1u          /* fr_add(a, b): a + b < 2^261 */
#define MSM_OP_FR_RAW_SUB2 2u         /* fr_sub<2>(a, b): a + 2r - b, b < r */
#define MSM_OP_FR_RAW_SUB3 3u         /* fr_sub<3>: b < 2r (the butterflies) */
#define MSM_OP_FR_RAW_SUB7 4u         /* fr_sub<7>: b < 6r */
#define MSM_OP_FR_RAW_SUB8 5u         /* fr_sub<8>: b < 7r, the last row of the pad table */
#define MSM_OP_FR_RAW_NORMALIZE 6u    /* fr_normalize(a): limbs 0..7 + carry < 2^32, value < 2^261 */
#define MSM_OP_FR_RAW_REDUCE_LT2R 7u  /* fr_reduce_lt2r(a): a < 2r */
#define MSM_OP_FR_RAW_CANONICAL 8u    /* fr_canonical(a): any normalised a */
#define MSM_OP_FR_RAW_UNPACK 9u       /* fr_unpack(a[0..7]) */
#define MSM_OP_FR_RAW_PACK 10u        /* fr_pack(out[0..7], a): a < 2^256 */
#define MSM_OP_FR_RAW_FROM_STD 11u    /* fr_from_std(a[0..7]) */
#define MSM_OP_FR_RAW_TO_STD 12u      /* fr_to_std(out[0..7], a): any normalised a */
#define MSM_OP_FR_RAW_POW_U32 13u     /* fr_pow_u32(a, b[0]): a < 84r */
#define MSM_OP_FR_RAW_INV 14u         /* fr_inv(a): a < 84r */
int32_t msm_test_fr_raw_op(msm_ctx *ctx, uint32_t op, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n);
/* the base field Fq of csrc/fp_bn254.hpp and Fq2 of csrc/fp2_bn254.hpp on RAW limb records: n elements, one device lane each, one function per
 * launch, no conversion and no reduction on the way in or out.  A record is 9 words for Fq (9 limbs of 29 bits, one u32 word per limb, least
 * significant first; value = sum limb_i * 2^(29 i)) and 18 words (c0, c1) for Fq2; ANY representative the value discipline of the two headers
 * allows for the operation.  `in` holds n elements of ARITY records one after the other, `out` n records.  op = kind | K << 8, K the pad multiple
 * where the function is a template over one (0 elsewhere); the instantiated (kind, K) are those of csrc/ outside the hooks files, any other is
 * MSM_ERR_BAD_ARG.  A limb >= 2^29 in an operand that must be normalised is MSM_ERR_BAD_ARG before anything runs (the operand of NORMALIZE and
 * the 8-word inputs take any 32-bit words); the value bounds are the caller's to keep: the device asserts nothing.  Where a function reads or
 * writes 8 words (a 256-bit pattern) word 8 is ignored on input and written as 0 on output.  RAW values (fp_sub_raw / fp_neg_raw) never cross
 * this interface: each way the product consumes one is a composite kind on normalised operands. */
#define MSM_OP_FQ_RAW_MUL 0u                /* fp_mul(a, b): needs a * b < (2^261 - p) * 2^261 */
#define MSM_OP_FQ_RAW_SQR 1u                /* fp_sqr(a) */
#define MSM_OP_FQ_RAW_MUL_ADD 2u            /* fp_mul_add(a, b, c, d): needs a * b + c * d < (2^261 - p) * 2^261 */
#define MSM_OP_FQ_RAW_ADD 3u                /* fp_add(a, b): a + b < 2^261 */
#define MSM_OP_FQ_RAW_DBL 4u                /* fp_dbl(a) */
#define MSM_OP_FQ_RAW_SUB 5u                /* fp_sub<K>(a, b): a + K p - b, b < (K-1) p;  K = 2 .. 8 */
#define MSM_OP_FQ_RAW_NEG 6u                /* fp_neg<K>(a): K p - a;  K = 2, 3, 4, 6 */
#define MSM_OP_FQ_RAW_SUB_B_2C 7u           /* fp_sub_b_2c(a, b, c): a + 5p - b - 2c, b + 2c < 4p */
#define MSM_OP_FQ_RAW_NORMALIZE 8u          /* fp_normalize(a): limbs + carry < 2^32, value < 2^261 */
#define MSM_OP_FQ_RAW_REDUCE_LT2P 9u        /* fp_reduce_lt2p(a): a < 2p */
#define MSM_OP_FQ_RAW_CANONICAL 10u         /* fp_canonical(a) */
#define MSM_OP_FQ_RAW_INV 11u               /* fp_inv(a): a < 2p */
#define MSM_OP_FQ_RAW_IS_ZERO_LT2P 12u      /* fp_is_zero_lt2p(a): 0 or 1 in word 0, the other words 0 */
#define MSM_OP_FQ_RAW_UNPACK 13u            /* fp_unpack(a[0..7]) */
#define MSM_OP_FQ_RAW_UNPACK_SHL5 14u       /* fp_unpack_shl5(a[0..7]) */
#define MSM_OP_FQ_RAW_FROM_MONT256 15u      /* fp_from_mont256(a[0..7]) */
#define MSM_OP_FQ_RAW_FROM_STD 16u          /* fp_from_std(a[0..7]) */
#define MSM_OP_FQ_RAW_PACK 17u              /* fp_pack(out[0..7], a): a < 2^256 */
#define MSM_OP_FQ_RAW_TO_MONT256 18u        /* fp_to_mont256(out[0..7], a) */
#define MSM_OP_FQ_RAW_TO_STD 19u            /* fp_to_std(out[0..7], a) */
#define MSM_OP_FQ_RAW_MUL_NEG_RAW2 20u      /* fp_mul(fp_neg_raw<2>(a), b): the y of a negative digit into S2 (a < p) */
#define MSM_OP_FQ_RAW_NORMALIZE_NEG_RAW2 21u /* fp_normalize(fp_neg_raw<2>(a)): xyzz_madd's identity branch */
#define MSM_OP_FQ_RAW_SUB6_NEG_RAW4 22u     /* fp_sub<6>(fp_neg_raw<4>(a), b): the raw minuend of xyzz_madd_m32 */
#define MSM_OP_FQ_RAW_Y3 23u                /* fp_mul_add(r, fp_sub_raw<8>(q, x3), fp_neg_raw<K>(y), ppp), records r q x3 y ppp;  K = 3, 6 */
int32_t msm_test_fq_raw_op(msm_ctx *ctx, uint32_t op, const uint32_t *in, uint32_t *out, size_t n);
#define MSM_OP_FQ2_RAW_MUL 0u               /* fp2_mul<K>(a, b): b.c1 < (K-1) p */
#define MSM_OP_FQ2_RAW_SQR 1u               /* fp2_sqr<K>(a): a.c1 < (K-1) p */
#define MSM_OP_FQ2_RAW_SUB 2u               /* fp2_sub<K>(a, b) */
#define MSM_OP_FQ2_RAW_NEG 3u               /* fp2_neg<K>(a) */
#define MSM_OP_FQ2_RAW_ADD 4u               /* fp2_add(a, b) */
#define MSM_OP_FQ2_RAW_DBL 5u               /* fp2_dbl(a) */
#define MSM_OP_FQ2_RAW_MUL_FP 6u            /* fp2_mul_fp(a, s): s one Fq record (9 words) */
#define MSM_OP_FQ2_RAW_IS_ZERO_LT2P 7u      /* fp2_is_zero_lt2p(a): 0 or 1 in word 0, the other words 0 */
#define MSM_OP_FQ2_RAW_IS_ZERO_ANY 8u       /* fp2_is_zero_any(a): likewise */
#define MSM_OP_FQ2_RAW_NEG_RAW6_MUL_ONE 9u  /* fp_mul(fp_neg_raw_k<6>(a.ci), fp_one()) per component: g2_conj_small (a.ci < 5p) */
#define MSM_OP_FQ2_RAW_NEG_RAW6_MUL_FP 10u  /* fp_mul(fp_neg_raw_k<6>(a.ci), s) per component, s one Fq record: fb2_inv_from_norm */
#define MSM_OP_FQ2_RAW_CONJ 11u             /* {a.c0, fp_normalize(fp_neg_raw_k<K>(a.c1))}: the operand g2_conj_mul<K> builds;  K = 9, 13 */
int32_t msm_test_fq2_raw_op(msm_ctx *ctx, uint32_t op, const uint32_t *in, uint32_t *out, size_t n);
/* signed/unsigned digit decomposition of the planner's choice, digits[w*n + i] as int32 */
int32_t msm_test_decompose(msm_ctx *ctx, const uint32_t *scalars, size_t n, uint32_t window_bits, int32_t *digits);

/* ---- integer-multiplier calibration --------------------------------------------
 * Runs two saturating micro-kernels on the context's device (4 wavefronts per SIMD, dependent chains, ~1 ms each) and
 * reports what THIS device sustains, per second over the whole chip, lane level:
 *   *mad_per_s     v_mad_u64_u32 operations (the instruction the field multiplication is made of)
 *   *fp_mul_per_s  9 x 29-bit Montgomery multiplications (fp_mul of csrc/fp_bn254.hpp, 171 multiplier instructions each)
 * bench.py prices k_accumulate against these instead of a datasheet figure. */
int32_t msm_calibrate(msm_ctx *ctx, double *mad_per_s, double *fp_mul_per_s);

/* ---- stage-level parity (counterpart of the reference's per-kernel tests: tests/cuzk/transpose.rs:6-118,
 *      smvp.rs:119-303, pbpr.rs:26-247).  Runs the whole pipeline once on host inputs (as msm_bn254_g1, single shot) and
 *      copies the intermediates of every stage back.  All output pointers are nullable; sizes follow msm_plan(n, ...)
 *      with W = num_windows, nb = num_buckets, nv = virtual_points, kb = log2(nb):
 *        digits      W x nv     bucket index | negate << 31, 0xFFFFFFFF = skipped (zero digit / base at infinity)
 *        offsets     W*nb + 1   exclusive prefix of the bucket sizes (CSC column pointer)
 *        sorted      W x nv     first offsets[W*nb] entries valid: virtual point index | negate << 31, grouped by bucket
 *        buckets     W*nb x 24  bucket sums, Jacobian Montgomery words (bucket b of window w holds the digit magnitude b + 1; in the TOP
 *                               window, when t = msm_plan_t.top_digit_bits < kb, the magnitude (b mod 2^t) + 1, the index bits above
 *                               t being low bits of the point index)
 *        bit_sums    W x (kb+1) x 24   Q_{w,u} (u < kb: buckets whose index has bit u set) and Q_{w,kb} = all buckets
 *      With MSM_FLAG_WINDOW_TABLE in the context's flags the RESIDENT path runs (upload + window table, then the resident
 *      pipeline): V = msm_plan_t.bucket_arrays arrays instead of W windows -- offsets V*nb + 1, buckets V*nb x 24, sorted entries are
 *      TABLE indices j*nv + i (window j of the group, virtual point i).  Arrays of more than 2^17 buckets are reduced as
 *      P = 2^(kb-16) pseudo-windows of 2^16 buckets: bit_sums then is (V*P) x 17 x 24 (Q_u over the index INSIDE the slice, u < 16,
 *      and the slice's plain sum).
 *      sort_path (nullable) receives 2 = two-level LDS sort, 1 = tiled LDS histogram, 0 = global-atomic fallback;
 *      big_items (nullable) the number of (region, batch) items of oversized sort regions handed to k_big_place. */
int32_t msm_test_stage_dump(msm_ctx *ctx, const uint32_t *bases_xy, uint32_t base_form, const uint8_t *inf_mask,
                            const uint32_t *scalars, size_t n, uint32_t *digits, uint32_t *offsets, uint32_t *sorted,
                            uint32_t *buckets_jacobian_mont, uint32_t *bit_sums_jacobian_mont, uint32_t *sort_path,
                            uint32_t *big_items, uint32_t out_jacobian_mont[24]);

/* ---- a call that FAILS between its sort and its accumulation (the piece-sort histogram and the bin cursors used to be cleaned by
 *      the accumulation of the call that used them, so such a failure left them dirty for the next call on the context).  Runs the
 *      decomposition, the sort and the piece plan of an n-point MSM on `scalars` (host, n x 8 words) and then returns MSM_ERR_HIP as a
 *      failed copy / event wait in front of the accumulation would: the flag words, the list counters, the piece histogram and its cursors
 *      are left exactly as that failure leaves them.  The next call on the context must be right. */
int32_t msm_test_abandon_after_sort(msm_ctx *ctx, const uint32_t *scalars, size_t n);

/* ---- probes of the bucket reduction's dependent chain (tools/wide_level_probe.py -> profiles/r6_wide_level_breakdown.txt).
 *      msm_probe_wide_level: ONE workgroup of `threads` threads runs `iters` pairwise levels e[i] += e[i + m/2] over m XYZZ records in LDS.
 *        mode 0: eight lanes per addition (the body of lds_tree_wide), loop bracketed only
 *        mode 1: the same with shader-cycle marks inside the addition of wavefront 0 (needs m/2 <= threads/8)
 *        mode 2: one lane per addition (xyzz_add, the form of k_pair_level)
 *      out[0] shader cycles of the loop, out[1] constant-rate (100 MHz) ticks of the loop, out[2 + k] (mode 1) cycles between mark k - 1 and
 *      mark k summed over the levels: 1 operands loaded, 2 stage-1 product, 3 exchange + P / R, 4 squares, 5 special-case vote,
 *      6 exchange + stage-3 operands, 7 stage-3 product, 8 exchange + X3 + stage-4 operands, 9 stage-4 product, 10 exchange + Y3,
 *      11 result stored, 12 loop left, 13 barrier passed.
 *      msm_probe_launch_chain: `launches` dependent launches back to back on the context's stream -- k_pair_level_wide over n_adds additions
 *      each, or an empty kernel (n_adds = 0) -- microseconds per launch by hipEvents. */
int32_t msm_probe_wide_level(msm_ctx *ctx, uint32_t threads, uint32_t m, uint32_t iters, uint32_t mode, long long out[18]);
int32_t msm_probe_launch_chain(msm_ctx *ctx, uint32_t n_adds, uint32_t launches, double *us_per_launch);
/* `launches` dependent launches of an EMPTY kernel of blocks x threads with lds_kb of static LDS per workgroup (0, 1 or 36): what the
 * dispatch of a large grid costs when every workgroup leaves at once (k_combine_pieces on uniform scalars) */
int32_t msm_probe_empty_launch(msm_ctx *ctx, uint32_t blocks, uint32_t threads, uint32_t lds_kb, uint32_t launches, double *us_per_launch);
/* k_reduce_bits_wide of the 2^20 shape (8 windows x 16 bit sums = 128 workgroups) on synthetic row / column sums with parts switched off:
 * parts bit 0 = staging (HBM -> LDS), bit 1 = the LDS tree, bit 2 = the XYZZ -> Jacobian -> R = 2^256 conversion; 7 = the kernel as the product runs it */
int32_t msm_probe_reduce_bits(msm_ctx *ctx, uint32_t parts, uint32_t launches, double *us_per_launch);
/* the list counters the last sort chain / accumulation left on the device: out[0] long-list entries, out[1] mid-list entries (buckets of 3 .. 7
 * pieces k_combine_pieces folds), out[2] pieces, out[3] partial-sum slots, out[4] buckets of exactly two pieces (listed apart) */
int32_t msm_test_get_list_counts(msm_ctx *ctx, uint32_t out[5]);
/* the tile size (log2 of the elements a workgroup holds in LDS) of the transforms that follow on this context: 4 or 10, the two sizes the
 * kernels are instantiated for; 0 = back to the plan of msm_bn254_fr_ntt_plan.  With 4, 2^12 elements are a three-pass transform. */
int32_t msm_test_ntt_set_tile_log2(msm_ctx *ctx, uint32_t tile_log2);
/* the chain (elements per lane) of the scalar-field scans that follow on this context: 1 or 8, the two lengths the kernels are instantiated
 * for; 0 = back to the plan of msm_bn254_fr_scan_plan.  With 1 a workgroup covers 256 elements, and the launch that walks the workgroups'
 * aggregates needs a second round from 2^16 + 1 elements on. */
int32_t msm_test_fr_scan_set_chain(msm_ctx *ctx, uint32_t chain);

#ifdef __cplusplus
}
#endif
#endif /* MSM_HIP_TESTHOOKS_H */
