// msm_testhooks_fq_raw.hpp -- the base field Fq (fp_bn254.hpp) and Fq2 (fp2_bn254.hpp) on RAW limb records, one function per element: what the
// kernels k_test_fq_raw / k_test_fq2_raw of the hooks build (msm_test_fq_raw_op, msm_test_fq2_raw_op) and the host program
// tools/fq_bounds_check.cpp (the same headers with -DFP_BOUNDS_CHECK) BOTH call.  Hooks build and tools only: never part of libmsm_hip.so.
//
// An element is ARITY records one after the other (Fq: 9 words, Fq2: 18 words c0 c1; the Fq operand of the two *_FP kinds of Fq2 is 9 words),
// the result one record.  The words are loaded as the caller wrote them, the one function is called, the limbs it returned are stored: no
// conversion and no reduction on the way in or out.  A RAW value (fp_sub_raw / fp_neg_raw: limbs up to 2^29 + 2^30) is never stored, so every way
// the product consumes one is a composite kind whose operands are all normalised.
// An operation is kind | K << 8, K the pad multiple the function is a template over (0 where it is none).  MSM_FQ_RAW_OPS / MSM_FQ2_RAW_OPS list
// every (kind, K) that is instantiated: exactly the instantiations of csrc/ outside the hooks files (tests/test_fq_ops_cpu.py compares).
#pragma once
#include "fp2_bn254.hpp"
#include "../../include/msm_hip_testhooks.h"

#define MSM_FQ_RAW_OPS(X)                                                                                                                        \
    X(MSM_OP_FQ_RAW_MUL, 0) X(MSM_OP_FQ_RAW_SQR, 0) X(MSM_OP_FQ_RAW_MUL_ADD, 0) X(MSM_OP_FQ_RAW_ADD, 0) X(MSM_OP_FQ_RAW_DBL, 0)                 \
    X(MSM_OP_FQ_RAW_SUB, 2) X(MSM_OP_FQ_RAW_SUB, 3) X(MSM_OP_FQ_RAW_SUB, 4) X(MSM_OP_FQ_RAW_SUB, 5) X(MSM_OP_FQ_RAW_SUB, 6)                     \
    X(MSM_OP_FQ_RAW_SUB, 7) X(MSM_OP_FQ_RAW_SUB, 8)                                                                                              \
    X(MSM_OP_FQ_RAW_NEG, 2) X(MSM_OP_FQ_RAW_NEG, 3) X(MSM_OP_FQ_RAW_NEG, 4) X(MSM_OP_FQ_RAW_NEG, 6)                                             \
    X(MSM_OP_FQ_RAW_SUB_B_2C, 0) X(MSM_OP_FQ_RAW_NORMALIZE, 0) X(MSM_OP_FQ_RAW_REDUCE_LT2P, 0) X(MSM_OP_FQ_RAW_CANONICAL, 0)                    \
    X(MSM_OP_FQ_RAW_INV, 0) X(MSM_OP_FQ_RAW_IS_ZERO_LT2P, 0) X(MSM_OP_FQ_RAW_UNPACK, 0) X(MSM_OP_FQ_RAW_UNPACK_SHL5, 0)                         \
    X(MSM_OP_FQ_RAW_FROM_MONT256, 0) X(MSM_OP_FQ_RAW_FROM_STD, 0) X(MSM_OP_FQ_RAW_PACK, 0) X(MSM_OP_FQ_RAW_TO_MONT256, 0)                       \
    X(MSM_OP_FQ_RAW_TO_STD, 0) X(MSM_OP_FQ_RAW_MUL_NEG_RAW2, 0) X(MSM_OP_FQ_RAW_NORMALIZE_NEG_RAW2, 0) X(MSM_OP_FQ_RAW_SUB6_NEG_RAW4, 0)        \
    X(MSM_OP_FQ_RAW_Y3, 3) X(MSM_OP_FQ_RAW_Y3, 6)

#define MSM_FQ2_RAW_OPS(X)                                                                                                                       \
    X(MSM_OP_FQ2_RAW_MUL, 3) X(MSM_OP_FQ2_RAW_MUL, 4) X(MSM_OP_FQ2_RAW_MUL, 6) X(MSM_OP_FQ2_RAW_MUL, 7) X(MSM_OP_FQ2_RAW_MUL, 9)                \
    X(MSM_OP_FQ2_RAW_MUL, 10) X(MSM_OP_FQ2_RAW_MUL, 13) X(MSM_OP_FQ2_RAW_MUL, 15) X(MSM_OP_FQ2_RAW_MUL, 16) X(MSM_OP_FQ2_RAW_MUL, 17)           \
    X(MSM_OP_FQ2_RAW_SQR, 3) X(MSM_OP_FQ2_RAW_SQR, 5) X(MSM_OP_FQ2_RAW_SQR, 6) X(MSM_OP_FQ2_RAW_SQR, 12) X(MSM_OP_FQ2_RAW_SQR, 13)              \
    X(MSM_OP_FQ2_RAW_SQR, 15) X(MSM_OP_FQ2_RAW_SQR, 16) X(MSM_OP_FQ2_RAW_SQR, 17)                                                               \
    X(MSM_OP_FQ2_RAW_SUB, 2) X(MSM_OP_FQ2_RAW_SUB, 3) X(MSM_OP_FQ2_RAW_SUB, 4) X(MSM_OP_FQ2_RAW_SUB, 5) X(MSM_OP_FQ2_RAW_SUB, 6)                \
    X(MSM_OP_FQ2_RAW_SUB, 7) X(MSM_OP_FQ2_RAW_SUB, 8) X(MSM_OP_FQ2_RAW_SUB, 9) X(MSM_OP_FQ2_RAW_SUB, 12) X(MSM_OP_FQ2_RAW_SUB, 13)              \
    X(MSM_OP_FQ2_RAW_NEG, 2) X(MSM_OP_FQ2_RAW_NEG, 8)                                                                                            \
    X(MSM_OP_FQ2_RAW_ADD, 0) X(MSM_OP_FQ2_RAW_DBL, 0) X(MSM_OP_FQ2_RAW_MUL_FP, 0) X(MSM_OP_FQ2_RAW_IS_ZERO_LT2P, 0)                             \
    X(MSM_OP_FQ2_RAW_IS_ZERO_ANY, 0) X(MSM_OP_FQ2_RAW_NEG_RAW6_MUL_ONE, 0) X(MSM_OP_FQ2_RAW_NEG_RAW6_MUL_FP, 0)                                 \
    X(MSM_OP_FQ2_RAW_CONJ, 9) X(MSM_OP_FQ2_RAW_CONJ, 13)

namespace fqraw {
using namespace bn254;

// records an element of `kind` holds (Fq), 0 = unknown kind
constexpr uint32_t fq_arity(uint32_t kind) {
    switch (kind) {
        case MSM_OP_FQ_RAW_MUL: case MSM_OP_FQ_RAW_ADD: case MSM_OP_FQ_RAW_SUB: case MSM_OP_FQ_RAW_MUL_NEG_RAW2: case MSM_OP_FQ_RAW_SUB6_NEG_RAW4: return 2;
        case MSM_OP_FQ_RAW_SUB_B_2C: return 3;
        case MSM_OP_FQ_RAW_MUL_ADD: return 4;
        case MSM_OP_FQ_RAW_Y3: return 5;
        default: return kind <= MSM_OP_FQ_RAW_Y3 ? 1 : 0;
    }
}
// the one record is 8 words of 32 bits (any values) and an ignored ninth
constexpr bool fq_words_in(uint32_t kind) { return kind >= MSM_OP_FQ_RAW_UNPACK && kind <= MSM_OP_FQ_RAW_FROM_STD; }
// the operand need not be normalised (fp_normalize exists for such limbs)
constexpr bool fq_any_limbs(uint32_t kind) { return kind == MSM_OP_FQ_RAW_NORMALIZE || fq_words_in(kind); }
// words an element of `kind` holds (Fq2), 0 = unknown kind
constexpr uint32_t fq2_words(uint32_t kind) {
    switch (kind) {
        case MSM_OP_FQ2_RAW_MUL: case MSM_OP_FQ2_RAW_SUB: case MSM_OP_FQ2_RAW_ADD: return 36;
        case MSM_OP_FQ2_RAW_MUL_FP: case MSM_OP_FQ2_RAW_NEG_RAW6_MUL_FP: return 27;
        default: return kind <= MSM_OP_FQ2_RAW_CONJ ? 18 : 0;
    }
}

FP_HD fp load9(const uint32_t* p) { return fp{{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]}}; }
FP_HD void store9(uint32_t* p, const fp& a) {
#pragma unroll
    for (int k = 0; k < 9; k++) p[k] = a.v[k];
}
FP_HD fp2 load18(const uint32_t* p) { return fp2{load9(p), load9(p + 9)}; }
FP_HD void store18(uint32_t* p, const fp2& a) { store9(p, a.c0), store9(p + 9, a.c1); }
FP_HD fp flag9(bool f) {
    fp r = fp_zero();
    r.v[0] = f ? 1u : 0u;
    return r;
}

// one element of the Fq operation KIND | K << 8: in = fq_arity(KIND) x 9 words, out = 9 words
template <uint32_t KIND, int K>
FP_HD void fq_eval(const uint32_t* in, uint32_t* out) {
    if constexpr (KIND >= MSM_OP_FQ_RAW_UNPACK && KIND <= MSM_OP_FQ_RAW_FROM_STD) {
        uint32_t w[8];
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = in[k];
        if constexpr (KIND == MSM_OP_FQ_RAW_UNPACK) store9(out, fp_unpack(w));
        else if constexpr (KIND == MSM_OP_FQ_RAW_UNPACK_SHL5) store9(out, fp_unpack_shl5(w));
        else if constexpr (KIND == MSM_OP_FQ_RAW_FROM_MONT256) store9(out, fp_from_mont256(w));
        else store9(out, fp_from_std(w));
    } else if constexpr (KIND >= MSM_OP_FQ_RAW_PACK && KIND <= MSM_OP_FQ_RAW_TO_STD) {
        uint32_t w[8];
        const fp a = load9(in);
        if constexpr (KIND == MSM_OP_FQ_RAW_PACK) fp_pack(w, a);
        else if constexpr (KIND == MSM_OP_FQ_RAW_TO_MONT256) fp_to_mont256(w, a);
        else fp_to_std(w, a);
#pragma unroll
        for (int k = 0; k < 8; k++) out[k] = w[k];
        out[8] = 0;
    } else {
        const fp a = load9(in);
        fp r;
        if constexpr (KIND == MSM_OP_FQ_RAW_MUL) r = fp_mul(a, load9(in + 9));
        else if constexpr (KIND == MSM_OP_FQ_RAW_SQR) r = fp_sqr(a);
        else if constexpr (KIND == MSM_OP_FQ_RAW_MUL_ADD) r = fp_mul_add(a, load9(in + 9), load9(in + 18), load9(in + 27));
        else if constexpr (KIND == MSM_OP_FQ_RAW_ADD) r = fp_add(a, load9(in + 9));
        else if constexpr (KIND == MSM_OP_FQ_RAW_DBL) r = fp_dbl(a);
        else if constexpr (KIND == MSM_OP_FQ_RAW_SUB) r = fp_sub<K>(a, load9(in + 9));
        else if constexpr (KIND == MSM_OP_FQ_RAW_NEG) r = fp_neg<K>(a);
        else if constexpr (KIND == MSM_OP_FQ_RAW_SUB_B_2C) r = fp_sub_b_2c(a, load9(in + 9), load9(in + 18));
        else if constexpr (KIND == MSM_OP_FQ_RAW_NORMALIZE) r = fp_normalize(a);
        else if constexpr (KIND == MSM_OP_FQ_RAW_REDUCE_LT2P) r = fp_reduce_lt2p(a);
        else if constexpr (KIND == MSM_OP_FQ_RAW_CANONICAL) r = fp_canonical(a);
        else if constexpr (KIND == MSM_OP_FQ_RAW_INV) r = fp_inv(a);
        else if constexpr (KIND == MSM_OP_FQ_RAW_IS_ZERO_LT2P) r = flag9(fp_is_zero_lt2p(a));
        else if constexpr (KIND == MSM_OP_FQ_RAW_MUL_NEG_RAW2) r = fp_mul(fp_neg_raw<2>(a), load9(in + 9));       // the y of a negative digit into S2
        else if constexpr (KIND == MSM_OP_FQ_RAW_NORMALIZE_NEG_RAW2) r = fp_normalize(fp_neg_raw<2>(a));          // xyzz_madd's identity branch
        else if constexpr (KIND == MSM_OP_FQ_RAW_SUB6_NEG_RAW4) r = fp_sub<6>(fp_neg_raw<4>(a), load9(in + 9));   // xyzz_madd_m32's raw minuend
        else {
            static_assert(KIND == MSM_OP_FQ_RAW_Y3, "unknown Fq kind");  // the Y3 of the additions: r, q, x3, y, ppp
            r = fp_mul_add(a, fp_sub_raw<8>(load9(in + 9), load9(in + 18)), fp_neg_raw<K>(load9(in + 27)), load9(in + 36));
        }
        store9(out, r);
    }
}

// one element of the Fq2 operation KIND | K << 8: in = fq2_words(KIND) words, out = 18 words
template <uint32_t KIND, int K>
FP_HD void fq2_eval(const uint32_t* in, uint32_t* out) {
    const fp2 a = load18(in);
    fp2 r;
    if constexpr (KIND == MSM_OP_FQ2_RAW_MUL) r = fp2_mul<K>(a, load18(in + 18));
    else if constexpr (KIND == MSM_OP_FQ2_RAW_SQR) r = fp2_sqr<K>(a);
    else if constexpr (KIND == MSM_OP_FQ2_RAW_SUB) r = fp2_sub<K>(a, load18(in + 18));
    else if constexpr (KIND == MSM_OP_FQ2_RAW_NEG) r = fp2_neg<K>(a);
    else if constexpr (KIND == MSM_OP_FQ2_RAW_ADD) r = fp2_add(a, load18(in + 18));
    else if constexpr (KIND == MSM_OP_FQ2_RAW_DBL) r = fp2_dbl(a);
    else if constexpr (KIND == MSM_OP_FQ2_RAW_MUL_FP) r = fp2_mul_fp(a, load9(in + 18));
    else if constexpr (KIND == MSM_OP_FQ2_RAW_IS_ZERO_LT2P) r = fp2{flag9(fp2_is_zero_lt2p(a)), fp_zero()};
    else if constexpr (KIND == MSM_OP_FQ2_RAW_IS_ZERO_ANY) r = fp2{flag9(fp2_is_zero_any(a)), fp_zero()};
    else if constexpr (KIND == MSM_OP_FQ2_RAW_NEG_RAW6_MUL_ONE) r = fp2{fp_mul(fp_neg_raw_k<6>(a.c0), fp_one()), fp_mul(fp_neg_raw_k<6>(a.c1), fp_one())};  // g2_conj_small, per component
    else if constexpr (KIND == MSM_OP_FQ2_RAW_NEG_RAW6_MUL_FP) {  // fb2_inv_from_norm's second component, per component
        const fp s = load9(in + 18);
        r = fp2{fp_mul(fp_neg_raw_k<6>(a.c0), s), fp_mul(fp_neg_raw_k<6>(a.c1), s)};
    } else {
        static_assert(KIND == MSM_OP_FQ2_RAW_CONJ, "unknown Fq2 kind");  // the operand g2_conj_mul<K> builds
        r = fp2{a.c0, fp_normalize(fp_neg_raw_k<K>(a.c1))};
    }
    store18(out, r);
}

}  // namespace fqraw
