// msm_fr_scan.inc -- scans over the scalar field behind the C ABI: msm_bn254_fr_scan_plan (host only), msm_bn254_fr_poly_eval_device,
// msm_bn254_fr_poly_div_linear_device, msm_bn254_fr_poly_div_linear, msm_bn254_fr_running_product_device.  Included by msm_hip.hip after
// msm_fr_vectors.inc; the per-lane routines, the combine steps and the kernels are fr_scan_bn254.hpp.
//
// Per context (msm_ctx::fr_scan, made on first use): ONE grow-on-demand array of block aggregates, 36 bytes per workgroup of the call (about
// 5 MB at 2^28 elements), shared by all streams the context is used with.  So, as the transforms do and the Fr vectors do not, every call leaves
// an event behind and a call on ANOTHER stream waits for it first.  Every constant (the powers of z, the changes of form) travels by value.
// A call checks everything and allocates before it enqueues anything: a failed call has written nothing.

struct FrScanState {
    DevBuf agg;                 // the aggregates of launch 1, turned into carry-ins by launch 2
    hipEvent_t ev = nullptr;    // behind the latest call
    hipStream_t last_stream = nullptr;
    bool used = false;
    uint32_t forced_chain = 0;  // hooks: msm_test_fr_scan_set_chain
};

static_assert(sizeof(msm_fr_scan_plan_t) == sizeof(fsck::FscPlan) && sizeof(fsck::FscPlan) == 32, "fr_scan_bn254.hpp mirrors the header's struct");
static_assert(MSM_FR_SCAN_EXCLUSIVE == fsck::FSC_EXCLUSIVE, "fr_scan_bn254.hpp mirrors the header's flag");
static_assert((MSM_FR_SCAN_EXCLUSIVE & (MSM_NTT_INVERSE | MSM_NTT_IN_MONT | MSM_NTT_OUT_MONT | MSM_FB_OUT_STD | MSM_PM_BASES_STD)) == 0,
              "the flag is a bit of its own");

namespace {

void fr_scan_release(msm_ctx* c) {
    FrScanState* s = c->fr_scan;
    if (!s) return;
    release(s->agg);
    if (s->ev) (void)hipEventDestroy(s->ev);
    delete s;
    c->fr_scan = nullptr;
}

int32_t fr_scan_state(msm_ctx* c) {
    if (c->fr_scan) return MSM_OK;
    FrScanState* s = new (std::nothrow) FrScanState();
    if (!s) return fail(c, MSM_ERR_OOM, "out of host memory");
    hipError_t e = hipEventCreateWithFlags(&s->ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        delete s;
        return fail(c, MSM_ERR_HIP, "hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
    }
    c->fr_scan = s;
    return MSM_OK;
}

uint32_t fr_scan_chain(const msm_ctx* c) { return c->fr_scan && c->fr_scan->forced_chain ? c->fr_scan->forced_chain : fsck::FSC_CHAIN; }

enum FrScanOp { FSC_OP_EVAL, FSC_OP_DIV, FSC_OP_PRODUCT };

template <uint32_t G>
void fr_scan_launch(FrScanOp op, const fsck::FscPoly& pa, const fsck::FscProduct& qa, const uint32_t* d_in, uint32_t* d_out, size_t n,
                    uint32_t* d_result, uint32_t* agg, hipStream_t st) {
    using namespace fsck;
    const size_t nb = fsc_blocks(n, G);
    const dim3 grid((unsigned)nb);
    if (op == FSC_OP_PRODUCT) {
        k_fsc_product_aggregate<G><<<grid, FSC_BLOCK, 0, st>>>(qa, d_in, n, agg);
        k_fsc_product_blocks<<<1, FSC_BLOCK, 0, st>>>(qa, agg, nb, d_result);
        k_fsc_product_apply<G><<<grid, FSC_BLOCK, 0, st>>>(qa, d_in, d_out, n, agg);
    } else {
        k_fsc_poly_aggregate<G><<<grid, FSC_BLOCK, 0, st>>>(pa, d_in, n, agg);
        k_fsc_poly_blocks<<<1, FSC_BLOCK, 0, st>>>(pa, agg, nb, d_result);
        if (op == FSC_OP_DIV) k_fsc_poly_apply<G><<<grid, FSC_BLOCK, 0, st>>>(pa, d_in, d_out, n, agg);
    }
}

// the whole call on st; the context's mutex is held and the arguments are checked
int32_t fr_scan_enqueue(msm_ctx* c, FrScanOp op, const uint32_t* z_std, const uint32_t* d_in, uint32_t* d_out, size_t n, uint32_t* d_result,
                        uint32_t flags, hipStream_t st) {
    using namespace fsck;
    int32_t rc;
    if ((rc = fr_scan_state(c))) return rc;
    FrScanState* s = c->fr_scan;
    const uint32_t G = fr_scan_chain(c);
    if ((rc = ensure(c, s->agg, (size_t)fsc_plan(n, G).scratch_bytes))) return rc;
    if (s->used && s->last_stream != st) HIPCHK(c, hipStreamWaitEvent(st, s->ev, 0));
    FscPoly pa{};
    FscProduct qa{};
    if (op == FSC_OP_PRODUCT) qa = fsc_product_args(flags);
    else pa = fsc_poly_args(fr_from_std(z_std), G, flags);
    if (G == FSC_CHAIN_SMALL) fr_scan_launch<FSC_CHAIN_SMALL>(op, pa, qa, d_in, d_out, n, d_result, (uint32_t*)s->agg.p, st);
    else fr_scan_launch<FSC_CHAIN>(op, pa, qa, d_in, d_out, n, d_result, (uint32_t*)s->agg.p, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(s->ev, st));
    s->used = true;
    s->last_stream = st;
    return MSM_OK;
}

}  // namespace

extern "C" {

int32_t msm_bn254_fr_scan_plan(size_t n, msm_fr_scan_plan_t* out) {
    if (!out) return fail(nullptr, MSM_ERR_BAD_ARG, "NULL out pointer");
    if (n == 0) return fail(nullptr, MSM_ERR_EMPTY, "Empty input");
    if (n > ((size_t)1 << fsck::FSC_MAX_LOG2)) return fail(nullptr, MSM_ERR_BAD_ARG, "n = %zu exceeds 2^%u elements", n, fsck::FSC_MAX_LOG2);
    const fsck::FscPlan p = fsck::fsc_plan(n);
    memcpy(out, &p, sizeof p);
    return MSM_OK;
}

int32_t msm_bn254_fr_poly_eval_device(msm_ctx* c, const void* d_coeffs, size_t n, const uint32_t* z_std, void* d_value, uint32_t flags,
                                      void* hip_stream) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!d_coeffs || !z_std || !d_value) return fail(c, MSM_ERR_BAD_ARG, "NULL coefficient, point or value pointer");
    int32_t rc = frv_check(c, flags, MSM_NTT_IN_MONT | MSM_NTT_OUT_MONT, n, {d_coeffs, d_value}, true);
    if (rc) return rc;
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_poly_eval_device");
    return fr_scan_enqueue(c, FSC_OP_EVAL, z_std, (const uint32_t*)d_coeffs, nullptr, n, (uint32_t*)d_value, flags,
                           hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int32_t msm_bn254_fr_poly_div_linear_device(msm_ctx* c, const void* d_coeffs, size_t n, const uint32_t* z_std, void* d_quot, void* d_rem,
                                            uint32_t flags, void* hip_stream) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!d_coeffs || !z_std || !d_quot) return fail(c, MSM_ERR_BAD_ARG, "NULL coefficient, point or quotient pointer");
    int32_t rc = frv_check(c, flags, MSM_NTT_IN_MONT | MSM_NTT_OUT_MONT, n, {d_coeffs, d_quot, d_rem}, true);
    if (rc) return rc;
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_poly_div_linear_device");
    return fr_scan_enqueue(c, FSC_OP_DIV, z_std, (const uint32_t*)d_coeffs, (uint32_t*)d_quot, n, (uint32_t*)d_rem, flags,
                           hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int32_t msm_bn254_fr_poly_div_linear(msm_ctx* c, const uint32_t* coeffs, size_t n, const uint32_t* z_std, uint32_t* quot, uint32_t* rem,
                                     uint32_t flags) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!coeffs || !z_std || !quot) return fail(c, MSM_ERR_BAD_ARG, "NULL coefficient, point or quotient pointer");
    int32_t rc = frv_check(c, flags, MSM_NTT_IN_MONT | MSM_NTT_OUT_MONT, n, {}, false);
    if (rc) return rc;
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_poly_div_linear");
    const size_t bytes = n * 32;
    HostPin pin_i, pin_o;
    if (!c->no_host_pin) {
        pin_i.pin(coeffs, bytes);
        if (quot != coeffs) pin_o.pin(quot, bytes);
    }
    DevTmp io;  // the n elements and, behind them, the remainder (freed on every way out)
    HIPCHK(c, hipMalloc(&io.p, bytes + 32));
    uint32_t* d_rem = (uint32_t*)io.p + n * 8;
    if ((rc = h2d(c, io.p, coeffs, bytes, c->stream))) return rc;
    if ((rc = fr_scan_enqueue(c, FSC_OP_DIV, z_std, (const uint32_t*)io.p, (uint32_t*)io.p, n, d_rem, flags, c->stream))) return rc;
    HIPCHK(c, hipMemcpyAsync(quot, io.p, bytes, hipMemcpyDeviceToHost, c->stream));
    uint32_t r8[8];
    HIPCHK(c, hipMemcpyAsync(r8, d_rem, 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (rem) memcpy(rem, r8, 32);
    return MSM_OK;
}

int32_t msm_bn254_fr_running_product_device(msm_ctx* c, const void* d_in, void* d_out, size_t n, void* d_total, uint32_t flags,
                                            void* hip_stream) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!d_in || !d_out) return fail(c, MSM_ERR_BAD_ARG, "NULL input or output pointer");
    int32_t rc = frv_check(c, flags, MSM_NTT_IN_MONT | MSM_NTT_OUT_MONT | MSM_FR_SCAN_EXCLUSIVE, n, {d_in, d_out, d_total}, true);
    if (rc) return rc;
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_running_product_device");
    return fr_scan_enqueue(c, FSC_OP_PRODUCT, nullptr, (const uint32_t*)d_in, (uint32_t*)d_out, n, (uint32_t*)d_total, flags,
                           hip_stream ? (hipStream_t)hip_stream : c->stream);
}

}  // extern "C"
