// msm_testhooks.inc -- test, benchmark and calibration hooks (include/msm_hip_testhooks.h).  Compiled only into
// libmsm_hip_hooks.so (-DMSM_HIP_TEST_HOOKS); the product library libmsm_hip.so does not contain any of this.
#include "../../include/msm_hip_testhooks.h"
#include "msm_testhooks_kernels.hpp"

namespace {

int32_t ensure_pow2_table(msm_ctx* c) {
    if (c->pow2_ready) return MSM_OK;
    using namespace hostg1;
    std::vector<uint32_t> tab((size_t)msmk::SCALAR_BITS * 16);
    Jac g{ONE, dbl(ONE), ONE};  // (1, 2) -- SH/constants.metal:121-174
    for (int j = 0; j < msmk::SCALAR_BITS; j++) {
        Fq zi = inv(g.z), zi2 = sqr(zi);
        Fq x = mul(g.x, zi2), y = mul(g.y, mul(zi2, zi));  // Montgomery affine
        store_words(&tab[(size_t)j * 16], x);
        store_words(&tab[(size_t)j * 16 + 8], y);
        g = jdbl(g);
    }
    int32_t rc = ensure(c, c->pow2, tab.size() * 4);
    if (rc) return rc;
    DevTmp raw;  // freed on every exit path
    HIPCHK(c, hipMalloc(&raw.p, tab.size() * 4));
    HIPCHK(c, hipMemcpyAsync(raw.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    msmk::k_convert_bases<<<grid1(2 * (size_t)msmk::SCALAR_BITS, 64), 64, 0, c->stream>>>((const uint32_t*)raw.p, (uint32_t*)c->pow2.p,
                                                                                     (uint32_t)msmk::SCALAR_BITS, 1u, 0u);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pow2_ready = true;
    return MSM_OK;
}

}  // namespace

extern "C" {

int32_t msm_bn254_g1_generate_device(msm_ctx* c, uint64_t base_seed, uint64_t scalar_seed, size_t n, void* d_bases_out,
                                     void* d_scalars_out) {
    if (!c) return MSM_ERR_BAD_ARG;
    if (n == 0) return fail(c, MSM_ERR_EMPTY, "Empty input");
    if (n > 0x7FFFFFFFull) return fail(c, MSM_ERR_BAD_ARG, "n too large");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    int32_t rc;
    if (d_bases_out) {
        if ((rc = ensure_pow2_table(c))) return rc;
        msmk::k_gen_bases<<<grid1(n, 128), 128, 0, c->stream>>>(base_seed, (uint32_t)n, (const uint32_t*)c->pow2.p,
                                                             (uint32_t*)d_bases_out);
    }
    if (d_scalars_out) msmk::k_gen_scalars<<<grid1(n, 256), 256, 0, c->stream>>>(scalar_seed, (uint32_t)n, (uint32_t*)d_scalars_out);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return MSM_OK;
}

int32_t msm_bn254_generate_scalars_host(uint64_t seed, size_t n, int nonzero, uint32_t* out) {
    if (!out) return MSM_ERR_BAD_ARG;
    for (size_t i = 0; i < n; i++) msmk::gen_scalar(seed, i, nonzero != 0, out + i * 8);
    return MSM_OK;
}

// ---- device-math unit-test hooks --------------------------------------------------------------------
static int32_t run_test_kernel(msm_ctx* c, bool g1, uint32_t op, const uint32_t* a, size_t a_words, const uint32_t* b,
                               size_t b_words, uint32_t* out, size_t out_words, size_t n) {
    if (!c || !a || !out) return MSM_ERR_BAD_ARG;
    if (n == 0) return MSM_ERR_EMPTY;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    DevTmp ta, tb_, tout;  // freed on every exit path
    HIPCHK(c, hipMalloc(&ta.p, n * a_words * 4));
    HIPCHK(c, hipMalloc(&tout.p, n * out_words * 4));
    HIPCHK(c, hipMemcpy(ta.p, a, n * a_words * 4, hipMemcpyHostToDevice));
    if (b) {
        HIPCHK(c, hipMalloc(&tb_.p, n * b_words * 4));
        HIPCHK(c, hipMemcpy(tb_.p, b, n * b_words * 4, hipMemcpyHostToDevice));
    }
    void *da = ta.p, *db = tb_.p, *dout = tout.p;
    if (g1 && op == MSM_OP_G1_ADD_WIDE) msmk::k_test_g1_wide<<<grid1(n, 8), 64, 0, c->stream>>>((uint32_t*)da, (uint32_t*)db, (uint32_t*)dout, (uint32_t)n);
    else if (g1) msmk::k_test_g1<<<grid1(n, 64), 64, 0, c->stream>>>(op, (uint32_t*)da, (uint32_t*)db, (uint32_t*)dout, (uint32_t)n);
    else msmk::k_test_fp<<<grid1(n, 64), 64, 0, c->stream>>>(op, (uint32_t*)da, (uint32_t*)db, (uint32_t*)dout, (uint32_t)n);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpy(out, dout, n * out_words * 4, hipMemcpyDeviceToHost));
    return MSM_OK;
}
int32_t msm_test_fp_op(msm_ctx* c, uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
    if (op > MSM_OP_FP_INV) return MSM_ERR_BAD_ARG;
    if (op <= MSM_OP_FP_MONT_MUL && !b) return MSM_ERR_BAD_ARG;
    return run_test_kernel(c, false, op, a, 8, op <= MSM_OP_FP_MONT_MUL ? b : nullptr, 8, out, 8, n);
}
int32_t msm_test_g1_op(msm_ctx* c, uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
    if (op > MSM_OP_G1_MADD_M256_NEG) return MSM_ERR_BAD_ARG;
    if (op != MSM_OP_G1_DBL && !b) return MSM_ERR_BAD_ARG;
    const bool affine_b = op == MSM_OP_G1_MADD || op == MSM_OP_G1_MADD_M256 || op == MSM_OP_G1_MADD_M256_NEG;
    return run_test_kernel(c, true, op, a, 24, op == MSM_OP_G1_DBL ? nullptr : b, affine_b ? 16 : 24, out, 24, n);
}
// the root-and-sign routine of k_g2_decompress (msm_kernels_g2_points.hpp g2_sqrt_signed) on arbitrary Fq2 values
int32_t msm_test_g2_sqrt(msm_ctx* c, const uint32_t* a_std, const uint8_t* want_larger, uint32_t* out_std, uint8_t* ok, size_t n) {
    if (!c || !a_std || !want_larger || !out_std || !ok) return MSM_ERR_BAD_ARG;
    if (n == 0) return MSM_ERR_EMPTY;
    if (n > 0x7FFFFFFFull) return fail(c, MSM_ERR_BAD_ARG, "n too large");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    DevTmp ta, tw, tout, tok;  // freed on every exit path
    HIPCHK(c, hipMalloc(&ta.p, n * 64));
    HIPCHK(c, hipMalloc(&tw.p, n));
    HIPCHK(c, hipMalloc(&tout.p, n * 64));
    HIPCHK(c, hipMalloc(&tok.p, n));
    HIPCHK(c, hipMemcpy(ta.p, a_std, n * 64, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(tw.p, want_larger, n, hipMemcpyHostToDevice));
    msmk::k_g2_test_sqrt<<<grid1(n, 256), 256, 0, c->stream>>>((const uint32_t*)ta.p, (const uint8_t*)tw.p, (uint32_t)n, (uint32_t*)tout.p, (uint8_t*)tok.p);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpy(out_std, tout.p, n * 64, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(ok, tok.p, n, hipMemcpyDeviceToHost));
    return MSM_OK;
}
// the G2 group law on raw limb records (msmk::k_test_g2): alloc / copy / launch / sync as run_test_kernel
int32_t msm_test_g2_op(msm_ctx* c, uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
    if (!c || !a || !out) return MSM_ERR_BAD_ARG;
    if (op > MSM_OP_G2_DBL) return fail(c, MSM_ERR_BAD_ARG, "unknown G2 op %u", op);
    if (op != MSM_OP_G2_DBL && !b) return MSM_ERR_BAD_ARG;
    if (n == 0) return MSM_ERR_EMPTY;
    if (n > 0x7FFFFFFFull / msmk::XW2) return fail(c, MSM_ERR_BAD_ARG, "n too large");
    const size_t a_words = msmk::XW2, b_words = op == MSM_OP_G2_MADD ? 36 : op == MSM_OP_G2_ADD ? (size_t)msmk::XW2 : 0;
    // a limb of 2^29 or more could overflow a column accumulator of the multiplication: a malformed test is refused, not run
    for (size_t i = 0; i < n * a_words; i++)
        if (a[i] > bn254::FP_MASK) return fail(c, MSM_ERR_BAD_ARG, "a: word %zu of record %zu is not a 29-bit limb", i % a_words, i / a_words);
    for (size_t i = 0; i < n * b_words; i++)
        if (b[i] > bn254::FP_MASK) return fail(c, MSM_ERR_BAD_ARG, "b: word %zu of record %zu is not a 29-bit limb", i % b_words, i / b_words);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    DevTmp ta, tb_, tout;  // freed on every exit path
    HIPCHK(c, hipMalloc(&ta.p, n * a_words * 4));
    HIPCHK(c, hipMalloc(&tout.p, n * a_words * 4));
    HIPCHK(c, hipMemcpy(ta.p, a, n * a_words * 4, hipMemcpyHostToDevice));
    if (b_words) {
        HIPCHK(c, hipMalloc(&tb_.p, n * b_words * 4));
        HIPCHK(c, hipMemcpy(tb_.p, b, n * b_words * 4, hipMemcpyHostToDevice));
    }
    const uint32_t *da = (const uint32_t*)ta.p, *db = (const uint32_t*)tb_.p;
    uint32_t* dout = (uint32_t*)tout.p;
    if (op == MSM_OP_G2_MADD) msmk::k_test_g2<MSM_OP_G2_MADD><<<grid1(n, 64), 64, 0, c->stream>>>(da, db, dout, (uint32_t)n);
    else if (op == MSM_OP_G2_ADD) msmk::k_test_g2<MSM_OP_G2_ADD><<<grid1(n, 64), 64, 0, c->stream>>>(da, db, dout, (uint32_t)n);
    else msmk::k_test_g2<MSM_OP_G2_DBL><<<grid1(n, 64), 64, 0, c->stream>>>(da, db, dout, (uint32_t)n);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpy(out, dout, n * a_words * 4, hipMemcpyDeviceToHost));
    return MSM_OK;
}
// the G1 group law on raw limb records (msmk::k_test_g1_raw and the two eight-lane kernels): checks, alloc / copy / launch / sync as msm_test_g2_op
int32_t msm_test_g1_raw_op(msm_ctx* c, uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
    if (!c || !a || !out) return MSM_ERR_BAD_ARG;
    if (op > MSM_OP_G1_RAW_ADD_WIDE_HBM) return fail(c, MSM_ERR_BAD_ARG, "unknown raw G1 op %u", op);
    if (op != MSM_OP_G1_RAW_DBL && !b) return MSM_ERR_BAD_ARG;
    if (n == 0) return MSM_ERR_EMPTY;
    if (n > 0x7FFFFFFFull / msmk::XW) return fail(c, MSM_ERR_BAD_ARG, "n too large");
    const bool m256 = op == MSM_OP_G1_RAW_MADD_M256 || op == MSM_OP_G1_RAW_MADD_M256_NEG;
    const size_t a_words = msmk::XW;
    const size_t b_words = op == MSM_OP_G1_RAW_DBL ? 0 : m256 ? 16 : op <= MSM_OP_G1_RAW_MADD_NEG_RAW ? 18 : (size_t)msmk::XW;
    // a limb of 2^29 or more could overflow a column accumulator of the multiplication: a malformed test is refused, not run
    // (the 16 words of the M256 operations are not limbs: fp_unpack_shl5 takes any 256 bits)
    for (size_t i = 0; i < n * a_words; i++)
        if (a[i] > bn254::FP_MASK) return fail(c, MSM_ERR_BAD_ARG, "a: word %zu of record %zu is not a 29-bit limb", i % a_words, i / a_words);
    for (size_t i = 0; !m256 && i < n * b_words; i++)
        if (b[i] > bn254::FP_MASK) return fail(c, MSM_ERR_BAD_ARG, "b: word %zu of record %zu is not a 29-bit limb", i % b_words, i / b_words);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    DevTmp ta, tb_, tout;  // freed on every exit path
    HIPCHK(c, hipMalloc(&ta.p, n * a_words * 4));
    HIPCHK(c, hipMalloc(&tout.p, n * a_words * 4));
    HIPCHK(c, hipMemcpy(ta.p, a, n * a_words * 4, hipMemcpyHostToDevice));
    if (b_words) {
        HIPCHK(c, hipMalloc(&tb_.p, n * b_words * 4));
        HIPCHK(c, hipMemcpy(tb_.p, b, n * b_words * 4, hipMemcpyHostToDevice));
    }
    const uint32_t *da = (const uint32_t*)ta.p, *db = (const uint32_t*)tb_.p;
    uint32_t* dout = (uint32_t*)tout.p;
#define MSM_G1_RAW(OP) msmk::k_test_g1_raw<OP><<<grid1(n, 64), 64, 0, c->stream>>>(da, db, dout, (uint32_t)n)
    switch (op) {
        case MSM_OP_G1_RAW_MADD: MSM_G1_RAW(MSM_OP_G1_RAW_MADD); break;
        case MSM_OP_G1_RAW_MADD_NEG_RAW: MSM_G1_RAW(MSM_OP_G1_RAW_MADD_NEG_RAW); break;
        case MSM_OP_G1_RAW_MADD_M256: MSM_G1_RAW(MSM_OP_G1_RAW_MADD_M256); break;
        case MSM_OP_G1_RAW_MADD_M256_NEG: MSM_G1_RAW(MSM_OP_G1_RAW_MADD_M256_NEG); break;
        case MSM_OP_G1_RAW_ADD: MSM_G1_RAW(MSM_OP_G1_RAW_ADD); break;
        case MSM_OP_G1_RAW_DBL: MSM_G1_RAW(MSM_OP_G1_RAW_DBL); break;
        case MSM_OP_G1_RAW_ADD_WIDE_LDS: msmk::k_test_g1_raw_wide_lds<<<grid1(n, 8), 64, 0, c->stream>>>(da, db, dout, (uint32_t)n); break;
        default: msmk::k_test_g1_raw_wide_hbm<<<grid1(n, 8), 64, 0, c->stream>>>(da, db, dout, (uint32_t)n); break;
    }
#undef MSM_G1_RAW
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpy(out, dout, n * a_words * 4, hipMemcpyDeviceToHost));
    return MSM_OK;
}
// the scalar field on raw limb records (msmk::k_test_fr_raw): checks, alloc / copy / launch / sync as msm_test_g1_raw_op
int32_t msm_test_fr_raw_op(msm_ctx* c, uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
    if (!c || !a || !out) return MSM_ERR_BAD_ARG;
    if (op > MSM_OP_FR_RAW_INV) return fail(c, MSM_ERR_BAD_ARG, "unknown raw Fr op %u", op);
    const bool b_limbs = op <= MSM_OP_FR_RAW_SUB8, b_read = b_limbs || op == MSM_OP_FR_RAW_POW_U32;
    if (b_read && !b) return MSM_ERR_BAD_ARG;
    if (n == 0) return MSM_ERR_EMPTY;
    if (n > 0x7FFFFFFFull / 9) return fail(c, MSM_ERR_BAD_ARG, "n too large");
    // a limb of 2^29 or more could overflow a column accumulator of the multiplication: a malformed test is refused, not run
    // (fr_normalize exists for such limbs, and the 8 words of fr_unpack / fr_from_std are not limbs: any 256 bits)
    const bool a_limbs = op != MSM_OP_FR_RAW_NORMALIZE && op != MSM_OP_FR_RAW_UNPACK && op != MSM_OP_FR_RAW_FROM_STD;
    for (size_t i = 0; a_limbs && i < n * 9; i++)
        if (a[i] > bn254::FP_MASK) return fail(c, MSM_ERR_BAD_ARG, "a: word %zu of record %zu is not a 29-bit limb", i % 9, i / 9);
    for (size_t i = 0; b_limbs && i < n * 9; i++)
        if (b[i] > bn254::FP_MASK) return fail(c, MSM_ERR_BAD_ARG, "b: word %zu of record %zu is not a 29-bit limb", i % 9, i / 9);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    DevTmp ta, tb_, tout;  // freed on every exit path
    HIPCHK(c, hipMalloc(&ta.p, n * 36));
    HIPCHK(c, hipMalloc(&tout.p, n * 36));
    HIPCHK(c, hipMemcpy(ta.p, a, n * 36, hipMemcpyHostToDevice));
    if (b_read) {
        HIPCHK(c, hipMalloc(&tb_.p, n * 36));
        HIPCHK(c, hipMemcpy(tb_.p, b, n * 36, hipMemcpyHostToDevice));
    }
    const uint32_t *da = (const uint32_t*)ta.p, *db = (const uint32_t*)tb_.p;
    uint32_t* dout = (uint32_t*)tout.p;
#define MSM_FR_RAW(OP) \
    case OP: msmk::k_test_fr_raw<OP><<<grid1(n, 64), 64, 0, c->stream>>>(da, db, dout, (uint32_t)n); break
    switch (op) {
        MSM_FR_RAW(MSM_OP_FR_RAW_MUL);
        MSM_FR_RAW(MSM_OP_FR_RAW_ADD);
        MSM_FR_RAW(MSM_OP_FR_RAW_SUB2);
        MSM_FR_RAW(MSM_OP_FR_RAW_SUB3);
        MSM_FR_RAW(MSM_OP_FR_RAW_SUB7);
        MSM_FR_RAW(MSM_OP_FR_RAW_SUB8);
        MSM_FR_RAW(MSM_OP_FR_RAW_NORMALIZE);
        MSM_FR_RAW(MSM_OP_FR_RAW_REDUCE_LT2R);
        MSM_FR_RAW(MSM_OP_FR_RAW_CANONICAL);
        MSM_FR_RAW(MSM_OP_FR_RAW_UNPACK);
        MSM_FR_RAW(MSM_OP_FR_RAW_PACK);
        MSM_FR_RAW(MSM_OP_FR_RAW_FROM_STD);
        MSM_FR_RAW(MSM_OP_FR_RAW_TO_STD);
        MSM_FR_RAW(MSM_OP_FR_RAW_POW_U32);
        MSM_FR_RAW(MSM_OP_FR_RAW_INV);
    }
#undef MSM_FR_RAW
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpy(out, dout, n * 36, hipMemcpyDeviceToHost));
    return MSM_OK;
}
// Fq and Fq2 on raw limb records (msmk::k_test_fq_raw / k_test_fq2_raw): checks, alloc / copy / launch / sync as msm_test_fr_raw_op.  in_words,
// out_words: the words of an element; limbs_from: the first word of an element that must be a 29-bit limb (in_words: none)
static int32_t run_fq_raw(msm_ctx* c, bool fq2, uint32_t op, const uint32_t* in, uint32_t* out, size_t n, size_t in_words, size_t out_words,
                          size_t limbs_from) {
    if (n == 0) return MSM_ERR_EMPTY;
    if (n > 0x7FFFFFFFull / 45) return fail(c, MSM_ERR_BAD_ARG, "n too large");
    // a limb of 2^29 or more could overflow a column accumulator of the multiplication: a malformed test is refused, not run
    for (size_t i = 0; i < n * in_words; i++)
        if (i % in_words >= limbs_from && in[i] > bn254::FP_MASK)
            return fail(c, MSM_ERR_BAD_ARG, "in: word %zu of element %zu is not a 29-bit limb", i % in_words, i / in_words);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    DevTmp tin, tout;  // freed on every exit path
    HIPCHK(c, hipMalloc(&tin.p, n * in_words * 4));
    HIPCHK(c, hipMalloc(&tout.p, n * out_words * 4));
    HIPCHK(c, hipMemcpy(tin.p, in, n * in_words * 4, hipMemcpyHostToDevice));
    const uint32_t* din = (const uint32_t*)tin.p;
    uint32_t* dout = (uint32_t*)tout.p;
#define MSM_FQ_RAW(KIND, K) \
    case (KIND) | ((uint32_t)(K) << 8): msmk::k_test_fq_raw<KIND, K><<<grid1(n, 64), 64, 0, c->stream>>>(din, dout, (uint32_t)n); break;
#define MSM_FQ2_RAW(KIND, K) \
    case (KIND) | ((uint32_t)(K) << 8): msmk::k_test_fq2_raw<KIND, K><<<grid1(n, 64), 64, 0, c->stream>>>(din, dout, (uint32_t)n); break;
    if (fq2) {
        switch (op) { MSM_FQ2_RAW_OPS(MSM_FQ2_RAW) }
    } else {
        switch (op) { MSM_FQ_RAW_OPS(MSM_FQ_RAW) }
    }
#undef MSM_FQ_RAW
#undef MSM_FQ2_RAW
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpy(out, dout, n * out_words * 4, hipMemcpyDeviceToHost));
    return MSM_OK;
}
int32_t msm_test_fq_raw_op(msm_ctx* c, uint32_t op, const uint32_t* in, uint32_t* out, size_t n) {
    if (!c || !in || !out) return MSM_ERR_BAD_ARG;
    bool known = false;
#define MSM_FQ_RAW(KIND, K) known = known || op == ((KIND) | ((uint32_t)(K) << 8));
    MSM_FQ_RAW_OPS(MSM_FQ_RAW)
#undef MSM_FQ_RAW
    if (!known) return fail(c, MSM_ERR_BAD_ARG, "unknown raw Fq op %u (kind %u, K %u)", op, op & 0xFFu, op >> 8);
    const uint32_t kind = op & 0xFFu;
    const size_t in_words = (size_t)fqraw::fq_arity(kind) * 9;
    return run_fq_raw(c, false, op, in, out, n, in_words, 9, fqraw::fq_any_limbs(kind) ? in_words : 0);
}
int32_t msm_test_fq2_raw_op(msm_ctx* c, uint32_t op, const uint32_t* in, uint32_t* out, size_t n) {
    if (!c || !in || !out) return MSM_ERR_BAD_ARG;
    bool known = false;
#define MSM_FQ2_RAW(KIND, K) known = known || op == ((KIND) | ((uint32_t)(K) << 8));
    MSM_FQ2_RAW_OPS(MSM_FQ2_RAW)
#undef MSM_FQ2_RAW
    if (!known) return fail(c, MSM_ERR_BAD_ARG, "unknown raw Fq2 op %u (kind %u, K %u)", op, op & 0xFFu, op >> 8);
    return run_fq_raw(c, true, op, in, out, n, fqraw::fq2_words(op & 0xFFu), 18, 0);
}
int32_t msm_calibrate(msm_ctx* c, double* mad_per_s, double* fp_mul_per_s) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    int32_t rc;
    if ((rc = ensure(c, c->flags, 64))) return rc;
    hipDeviceProp_t prop;
    HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
    const unsigned blocks = (unsigned)prop.multiProcessorCount * 4u * 4u;  // 256-thread blocks: 4 wavefronts on each of a CU's 4 SIMDs
    struct Ev {
        hipEvent_t e = nullptr;
        ~Ev() {
            if (e) (void)hipEventDestroy(e);
        }
    } ev0, ev1;
    HIPCHK(c, hipEventCreate(&ev0.e));
    HIPCHK(c, hipEventCreate(&ev1.e));
    hipEvent_t e0 = ev0.e, e1 = ev1.e;
    double out[2] = {0, 0};
    for (uint32_t what = 0; what < 2; what++) {
        const uint32_t iters = what == 0 ? 500u : 100u;  // ~1 ms each
        const double ops_per_thread = what == 0 ? 64.0 * iters : 4.0 * iters;
        msmk::k_calibrate<<<blocks, 256, 0, c->stream>>>(what, iters / 10, (uint32_t*)c->flags.p + 15);  // warm-up
        HIPCHK(c, hipEventRecord(e0, c->stream));
        msmk::k_calibrate<<<blocks, 256, 0, c->stream>>>(what, iters, (uint32_t*)c->flags.p + 15);
        HIPCHK(c, hipEventRecord(e1, c->stream));
        HIPCHK(c, hipEventSynchronize(e1));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
        out[what] = ops_per_thread * (double)blocks * 256.0 / ((double)ms * 1e-3);
    }
    HIPCHK(c, hipGetLastError());
    if (mad_per_s) *mad_per_s = out[0];
    if (fp_mul_per_s) *fp_mul_per_s = out[1];
    return MSM_OK;
}

// ---- probes of the reduction's dependent chain (VERDICT r5 item 1a; tools/wide_level_probe.py) -----------------
namespace {
int32_t probe_records(msm_ctx* c, size_t nrec, DevTmp& buf) {
    // nrec pseudo-random XYZZ records: normalised limbs, values below p (top limb < 2^21); not curve points -- the arithmetic does not care,
    // and two random values never meet the special cases (equal x, identity)
    std::vector<uint32_t> h(nrec * msmk::XW);
    uint64_t st = 0xB2540006ull;
    for (size_t i = 0; i < h.size(); i++) h[i] = (uint32_t)msmk::splitmix64(st) & ((i % 9 == 8) ? 0x1FFFFFu : bn254::FP_MASK);
    HIPCHK(c, hipMalloc(&buf.p, h.size() * 4));
    HIPCHK(c, hipMemcpy(buf.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    return MSM_OK;
}
}  // namespace
int32_t msm_probe_wide_level(msm_ctx* c, uint32_t threads, uint32_t m, uint32_t iters, uint32_t mode, long long out[18]) {
    if (!c || !out || threads == 0 || threads > 512 || threads % 64 || m < 2 || m > msmk::WIDE_TREE_MAX || (m & 1) || iters == 0 || mode > 2) return MSM_ERR_BAD_ARG;
    if (mode == 1 && m / 2 > threads / msmk::WIDE_LANES) return MSM_ERR_BAD_ARG;  // marks: one addition per group and level
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    DevTmp rec, res;
    int32_t rc = probe_records(c, m, rec);
    if (rc) return rc;
    HIPCHK(c, hipMalloc(&res.p, 18 * 8));
    HIPCHK(c, hipMemset(res.p, 0, 18 * 8));
    for (int rep = 0; rep < 2; rep++) {  // (the second run's numbers are kept: instruction cache warm)
        if (mode == 0) msmk::k_probe_wide_level<false><<<1, threads, 0, c->stream>>>((const uint32_t*)rec.p, m, iters, (long long*)res.p);
        else if (mode == 1) msmk::k_probe_wide_level<true><<<1, threads, 0, c->stream>>>((const uint32_t*)rec.p, m, iters, (long long*)res.p);
        else msmk::k_probe_scalar_level<<<1, threads, 0, c->stream>>>((const uint32_t*)rec.p, m, iters, (long long*)res.p);
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpy(out, res.p, 18 * 8, hipMemcpyDeviceToHost));
    return MSM_OK;
}
int32_t msm_probe_launch_chain(msm_ctx* c, uint32_t n_adds, uint32_t launches, double* us_per_launch) {
    if (!c || !us_per_launch || launches == 0 || n_adds > (1u << 20)) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    DevTmp rec, outb;
    int32_t rc;
    if (n_adds) {
        if ((rc = probe_records(c, 2 * (size_t)n_adds, rec))) return rc;
        HIPCHK(c, hipMalloc(&outb.p, (size_t)n_adds * XB));
    }
    struct Ev {
        hipEvent_t e = nullptr;
        ~Ev() {
            if (e) (void)hipEventDestroy(e);
        }
    } ev0, ev1;
    HIPCHK(c, hipEventCreate(&ev0.e));
    HIPCHK(c, hipEventCreate(&ev1.e));
    const msmk::pair_job ja{(const uint32_t*)rec.p, (uint32_t*)outb.p, n_adds, 1}, jb{nullptr, nullptr, 0, 1};
    for (int rep = 0; rep < 2; rep++) {
        HIPCHK(c, hipEventRecord(ev0.e, c->stream));
        for (uint32_t k = 0; k < launches; k++) {
            if (n_adds) msmk::k_pair_level_wide<<<grid1((size_t)n_adds * msmk::WIDE_LANES, 256), 256, 0, c->stream>>>(ja, jb);
            else msmk::k_probe_empty<<<1, 64, 0, c->stream>>>(nullptr);
        }
        HIPCHK(c, hipEventRecord(ev1.e, c->stream));
        HIPCHK(c, hipEventSynchronize(ev1.e));
    }
    HIPCHK(c, hipGetLastError());
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev0.e, ev1.e));
    *us_per_launch = (double)ms * 1e3 / launches;
    return MSM_OK;
}

int32_t msm_probe_empty_launch(msm_ctx* c, uint32_t blocks, uint32_t threads, uint32_t lds_kb, uint32_t launches, double* us_per_launch) {
    if (!c || !us_per_launch || !blocks || !threads || threads > 1024 || launches == 0) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    struct Ev {
        hipEvent_t e = nullptr;
        ~Ev() {
            if (e) (void)hipEventDestroy(e);
        }
    } ev0, ev1;
    HIPCHK(c, hipEventCreate(&ev0.e));
    HIPCHK(c, hipEventCreate(&ev1.e));
    for (int rep = 0; rep < 2; rep++) {
        HIPCHK(c, hipEventRecord(ev0.e, c->stream));
        for (uint32_t k = 0; k < launches; k++) {
            if (lds_kb >= 36) msmk::k_probe_empty_lds<9216><<<blocks, threads, 0, c->stream>>>(nullptr);
            else if (lds_kb > 0) msmk::k_probe_empty_lds<256><<<blocks, threads, 0, c->stream>>>(nullptr);
            else msmk::k_probe_empty<<<blocks, threads, 0, c->stream>>>(nullptr);
        }
        HIPCHK(c, hipEventRecord(ev1.e, c->stream));
        HIPCHK(c, hipEventSynchronize(ev1.e));
    }
    HIPCHK(c, hipGetLastError());
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev0.e, ev1.e));
    *us_per_launch = (double)ms * 1e3 / launches;
    return MSM_OK;
}
// k_reduce_bits_wide on synthetic row / column sums of the 2^20 shape (8 windows, 256 row sums, 128 column sums each: 128 workgroups), with
// parts of it switched off (msmk::k_reduce_bits_wide<PARTS>): microseconds per launch, dependent launches back to back
int32_t msm_probe_reduce_bits(msm_ctx* c, uint32_t parts, uint32_t launches, double* us_per_launch) {
    if (!c || !us_per_launch || launches == 0 || parts > 7) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    const uint32_t W = 8, kb = 15, kb_lo = 7, n_lo = 128, n_hi = 256;
    DevTmp rec, fl;
    int32_t rc;
    if ((rc = probe_records(c, (size_t)W * (n_lo + n_hi), rec))) return rc;
    HIPCHK(c, hipMalloc(&fl.p, 64));
    HIPCHK(c, hipMemset(fl.p, 0, 64));
    uint32_t *q_dev = nullptr, *f_dev = nullptr;
    HIPCHK(c, hipHostGetDevicePointer((void**)&q_dev, c->results[PointSide<HostG1>::RESULT].pinned, 0));
    HIPCHK(c, hipHostGetDevicePointer((void**)&f_dev, c->h_flags, 0));
    const uint32_t *Rp = (const uint32_t*)rec.p, *Cp = Rp + (size_t)W * n_hi * msmk::XW;
    struct Ev {
        hipEvent_t e = nullptr;
        ~Ev() {
            if (e) (void)hipEventDestroy(e);
        }
    } ev0, ev1;
    HIPCHK(c, hipEventCreate(&ev0.e));
    HIPCHK(c, hipEventCreate(&ev1.e));
    for (int rep = 0; rep < 2; rep++) {
        HIPCHK(c, hipEventRecord(ev0.e, c->stream));
        for (uint32_t k = 0; k < launches; k++) {
#define MSM_PROBE_RB(P) msmk::k_reduce_bits_wide<P><<<W * (kb + 1), 512, 0, c->stream>>>(Rp, Cp, q_dev, n_hi, n_lo, kb_lo, kb, (uint32_t*)fl.p, f_dev, 0u)
            switch (parts) {
                case 7: MSM_PROBE_RB(7); break;
                case 6: MSM_PROBE_RB(6); break;
                case 5: MSM_PROBE_RB(5); break;
                case 4: MSM_PROBE_RB(4); break;
                case 3: MSM_PROBE_RB(3); break;
                case 2: MSM_PROBE_RB(2); break;
                case 1: MSM_PROBE_RB(1); break;
                default: MSM_PROBE_RB(0); break;
            }
#undef MSM_PROBE_RB
        }
        HIPCHK(c, hipEventRecord(ev1.e, c->stream));
        HIPCHK(c, hipEventSynchronize(ev1.e));
    }
    HIPCHK(c, hipGetLastError());
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, ev0.e, ev1.e));
    *us_per_launch = (double)ms * 1e3 / launches;
    return MSM_OK;
}
// the list counters the LAST sort chain / accumulation of this context left on the device: [0] long-list entries, [1] mid-list entries
// (buckets of 3 .. 7 pieces k_combine_pieces folds), [2] pieces, [3] partial-sum slots, [4] two-piece buckets
static_assert(msmk::FLAG_MID2 == msmk::FLAG_LONG + 4, "msm_test_get_list_counts copies five consecutive flag words");
int32_t msm_test_get_list_counts(msm_ctx* c, uint32_t out[5]) {
    if (!c || !out) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    if (!c->flags.p) return MSM_ERR_STATE;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, (const uint32_t*)c->flags.p + msmk::FLAG_LONG, 20, hipMemcpyDeviceToHost));
    return MSM_OK;
}

int32_t msm_test_decompose(msm_ctx* c, const uint32_t* scalars, size_t n, uint32_t window_bits, int32_t* digits) {
    if (!c || !scalars || !digits) return MSM_ERR_BAD_ARG;
    if (n == 0) return MSM_ERR_EMPTY;
    msm_plan_t pl;
    if (make_plan(n, window_bits ? window_bits : c->cfg.window_bits, c->cfg.flags | MSM_FLAG_NO_GLV, &pl, c->knobs.glv_max)) return MSM_ERR_BAD_ARG;  // plain 254-bit digits
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    DevTmp ts, td;
    size_t out_bytes = (size_t)pl.num_windows * n * 4;
    HIPCHK(c, hipMalloc(&ts.p, n * 32));
    HIPCHK(c, hipMalloc(&td.p, out_bytes));
    void *ds = ts.p, *dd = td.p;
    HIPCHK(c, hipMemcpy(ds, scalars, n * 32, hipMemcpyHostToDevice));
    if (pl.signed_digits)
        msmk::k_decompose_plain<true><<<grid1(n, 256), 256, 0, c->stream>>>((uint32_t*)ds, (uint32_t)n, pl.window_bits,
                                                                         pl.num_windows, (int32_t*)dd);
    else
        msmk::k_decompose_plain<false><<<grid1(n, 256), 256, 0, c->stream>>>((uint32_t*)ds, (uint32_t)n, pl.window_bits,
                                                                          pl.num_windows, (int32_t*)dd);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpy(digits, dd, out_bytes, hipMemcpyDeviceToHost));
    return MSM_OK;
}

// the whole pipeline once, then every stage's intermediates back to the host (see include/msm_hip_testhooks.h)
int32_t msm_test_stage_dump(msm_ctx* c, const uint32_t* bases_xy, uint32_t base_form, const uint8_t* inf_mask, const uint32_t* scalars,
                            size_t n, uint32_t* digits, uint32_t* offsets, uint32_t* sorted, uint32_t* buckets_jac, uint32_t* bit_sums,
                            uint32_t* sort_path, uint32_t* big_items, uint32_t out_jac[24]) {
    int32_t rc = check_common(c, bases_xy, scalars, n);
    if (rc) return rc;
    if (base_form != MSM_FORM_STD && base_form != MSM_FORM_MONT) return fail(c, MSM_ERR_BAD_ARG, "unknown base_form %u", base_form);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t st = c->stream;
    PipeState ps;
    if ((rc = ensure(c, c->scalars, n * 32))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->scalars.p, scalars, n * 32, hipMemcpyHostToDevice, st));
    if (c->cfg.flags & MSM_FLAG_WINDOW_TABLE) {
        // the resident path with its window table: upload (+ table build), then the resident pipeline on the whole set
        c->resident_n = 0;
        if ((rc = upload_resident_locked(c, bases_xy, base_form, inf_mask, n))) return rc;
        HIPCHK(c, hipStreamSynchronize(st));
        c->resident_n = n;
        c->resident_has_inf = inf_mask != nullptr;
        PipelineOpts ro;
        ro.extra_flags = c->resident_glv ? 0u : MSM_FLAG_NO_GLV, ro.ps_out = &ps;
        ro.table_c = c->table_f > 1 ? c->table_c : 0u, ro.table_f = c->table_f;
        rc = run_pipeline(c, (const uint32_t*)c->rbases.p, inf_mask ? (const uint8_t*)c->rinf.p : nullptr, (const uint32_t*)c->scalars.p, n, st,
                          out_jac, nullptr, nullptr, ro);
    } else {
        const bool glv = plan_glv(c, n);
        if ((rc = ensure(c, c->bases, n * 64))) return rc;
        if ((rc = ensure(c, c->ibases, (glv ? 2 : 1) * n * 64))) return rc;
        if (inf_mask && (rc = ensure(c, c->inf, n))) return rc;
        HIPCHK(c, hipMemcpyAsync(c->bases.p, bases_xy, n * 64, hipMemcpyHostToDevice, st));
        if (inf_mask) HIPCHK(c, hipMemcpyAsync(c->inf.p, inf_mask, n, hipMemcpyHostToDevice, st));
        HostInput in;  // the product's own coordinate half: arkworks words are gathered as they are, standard form is converted
        in.kind = base_form == MSM_FORM_MONT ? KIND_MONT : KIND_STD;
        const BaseSrc src = launch_convert(in, c->bases.p, n, (uint32_t*)c->ibases.p, nullptr, glv, st);
        PipelineOpts ro;
        ro.ps_out = &ps;
        rc = run_pipeline(c, src, inf_mask ? (const uint8_t*)c->inf.p : nullptr, (const uint32_t*)c->scalars.p, n, st, out_jac, nullptr, nullptr, ro);
    }
    if (rc) return rc;
    // every intermediate buffer survives the pipeline (the reduction reads the buckets, it does not overwrite them)
    if (digits) {  // always handed out as 32-bit codes, rows of ps.n entries
        const SortGeom& sg = ps.sg;
        if (sg.d16) {
            std::vector<uint16_t> h((size_t)ps.W * sg.drow);
            HIPCHK(c, hipMemcpy(h.data(), c->digits.p, h.size() * 2, hipMemcpyDeviceToHost));
            for (uint32_t w = 0; w < ps.W; w++)
                for (size_t i = 0; i < ps.n; i++) digits[(size_t)w * ps.n + i] = msmk::digit16_widen(h[(size_t)w * sg.drow + i]);
        } else {
            HIPCHK(c, hipMemcpy(digits, c->digits.p, ps.pairs * 4, hipMemcpyDeviceToHost));
        }
    }
    if (offsets) HIPCHK(c, hipMemcpy(offsets, c->offsets.p, (ps.tb + 1) * 4, hipMemcpyDeviceToHost));
    if (sorted) HIPCHK(c, hipMemcpy(sorted, c->sorted.p, ps.pairs * 4, hipMemcpyDeviceToHost));
    if (buckets_jac) {
        DevTmp t;
        HIPCHK(c, hipMalloc(&t.p, ps.tb * 96));
        msmk::k_dump_xyzz_as_jacobian<<<grid1(ps.tb, 64), 64, 0, st>>>((const uint32_t*)c->buckets.p, (uint32_t)ps.tb, (uint32_t*)t.p);
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpy(buckets_jac, t.p, ps.tb * 96, hipMemcpyDeviceToHost));
    }
    if (bit_sums) std::memcpy(bit_sums, c->results[PointSide<HostG1>::RESULT].taken.data(), (size_t)ps.rW * (ps.rkb + 1) * 96);  // (pseudo-)windows x (rkb + 1): what finish_sync took out of the pairs
    if (sort_path) *sort_path = c->last_sort_path;
    if (big_items) {
        *big_items = 0;
        if (c->last_sort_path == 2 && c->big.p) HIPCHK(c, hipMemcpy(big_items, c->big.p, 4, hipMemcpyDeviceToHost));
    }
    return MSM_OK;
}

int32_t msm_test_abandon_after_sort(msm_ctx* c, const uint32_t* scalars, size_t n) {
    int32_t rc = check_common(c, scalars, scalars, n);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t st = c->stream;
    PipeState ps;
    if ((rc = ensure(c, c->scalars, n * 32))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->scalars.p, scalars, n * 32, hipMemcpyHostToDevice, st));
    if ((rc = pipe_prepare(c, n, st, &ps))) return rc;
    if ((rc = enqueue_digits_sort(c, ps, nullptr, (const uint32_t*)c->scalars.p, 0, st, true))) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    return fail(c, MSM_ERR_HIP, "test hook: the call was abandoned between its sort and its accumulation");
}

int32_t msm_test_ntt_set_tile_log2(msm_ctx* c, uint32_t tile_log2) {
    if (!c) return MSM_ERR_BAD_ARG;
    if (tile_log2 != 0 && tile_log2 != nttk::NTT_TILE_SMALL_LOG2 && tile_log2 != nttk::NTT_TILE_LOG2)
        return fail(c, MSM_ERR_BAD_ARG, "tile_log2 = %u: 0, %u or %u", tile_log2, nttk::NTT_TILE_SMALL_LOG2, nttk::NTT_TILE_LOG2);
    std::lock_guard<std::mutex> lk(c->mu);
    int32_t rc = ntt_state(c);
    if (rc) return rc;
    c->ntt->forced_tile = tile_log2;
    return MSM_OK;
}

int32_t msm_test_fr_scan_set_chain(msm_ctx* c, uint32_t chain) {
    if (!c) return MSM_ERR_BAD_ARG;
    if (chain != 0 && !fsck::fsc_chain_ok(chain))
        return fail(c, MSM_ERR_BAD_ARG, "chain = %u: 0, %u or %u", chain, fsck::FSC_CHAIN_SMALL, fsck::FSC_CHAIN);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    int32_t rc = fr_scan_state(c);
    if (rc) return rc;
    c->fr_scan->forced_chain = chain;
    return MSM_OK;
}

}  // extern "C"
