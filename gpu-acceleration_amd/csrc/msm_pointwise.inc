// msm_pointwise.inc -- the element-wise scalar multiplication of both groups behind the C ABI: msm_bn254_g1_pointwise_mul_plan (host only),
// msm_bn254_g1_pointwise_mul_device, msm_bn254_g1_scale_device, msm_bn254_g1_pointwise_mul and the same four with _g2_.  Included by msm_hip.hip
// after msm_fr_vectors.inc; the routines are pointwise_mul_bn254.hpp / g2_pointwise_mul_bn254.hpp, the kernels msm_kernels_pointwise.hpp /
// msm_kernels_g2_pointwise.hpp.  The host side is one body per call, over PointwiseSide<G>: the record width, the staging step, the kernel and
// the names of the ranges are all that differ between the groups.
//
// The device forms keep nothing on the context (the idiom of msm_fr_vectors.inc): no table, no scratch array, no event -- a call is one kernel
// launch per 2^30 points, and the halves of _scale_device's one scalar travel by value with it.  So two calls on two streams do not wait for
// each other.  Only the host-pointer form has state (msm_ctx::pointwise, per group, made by its first call): the staging arrays, which the kernel
// updates IN PLACE -- the bases go up into the array the products come down from.

static_assert(sizeof(msm_pointwise_plan_t) == sizeof(pmk::PmPlan) && sizeof(pmk::PmPlan) == 16, "pointwise_mul_bn254.hpp mirrors the header's struct");
static_assert(sizeof(msm_pointwise_g2_plan_t) == sizeof(pmk::Pm2Plan) && sizeof(pmk::Pm2Plan) == 16, "g2_pointwise_mul_bn254.hpp mirrors the header's struct");
static_assert(MSM_FB_OUT_STD == pmk::PM_F_OUT_STD && MSM_NTT_IN_MONT == pmk::PM_F_IN_MONT && MSM_PM_BASES_STD == pmk::PM_F_BASES_STD,
              "pointwise_mul_bn254.hpp mirrors the header's constants (both groups' kernels read these)");

struct PointwiseState {
    DevBuf io_k, io_xy, io_inf;
};

namespace {

constexpr size_t PM_LAUNCH_MAX = (size_t)1 << 30;  // points per launch (a multiple of 16: the chunks' arrays stay aligned)

// A group's side of the call: words per affine record, points the host-pointer call stages at a time, the kernels, the names of the ranges
// (KERNEL_ONE is named first: template kernels land in the code object in the order the host code names them, profiles/host_share_resource_usage.txt)
template <class G>
struct PointwiseSide;
template <>
struct PointwiseSide<HostG1> {
    static constexpr size_t WORDS = 16;
    static constexpr size_t STAGE_MAX = (size_t)1 << 20;
    static constexpr const char* RANGE_DEVICE = "msm_bn254_g1_pointwise_mul_device";
    static constexpr const char* RANGE_SCALE = "msm_bn254_g1_scale_device";
    static constexpr const char* RANGE_HOST = "msm_bn254_g1_pointwise_mul";
    static constexpr auto KERNEL_ONE = pmk::k_pm_mul<true>, KERNEL_EACH = pmk::k_pm_mul<false>;  // one scalar for all points / a scalar per point
};
template <>
struct PointwiseSide<HostG2> {
    static constexpr size_t WORDS = 32;
    static constexpr size_t STAGE_MAX = (size_t)1 << 19;  // (128 + 32 + 1 bytes each: 85 MB)
    static constexpr const char* RANGE_DEVICE = "msm_bn254_g2_pointwise_mul_device";
    static constexpr const char* RANGE_SCALE = "msm_bn254_g2_scale_device";
    static constexpr const char* RANGE_HOST = "msm_bn254_g2_pointwise_mul";
    static constexpr auto KERNEL_ONE = pmk::k_pm2_mul<true>, KERNEL_EACH = pmk::k_pm2_mul<false>;  // one scalar for all points / a scalar per point
};

void pointwise_release(msm_ctx* c) {
    for (PointwiseState*& s : c->pointwise) {
        if (!s) continue;
        for (DevBuf* b : {&s->io_k, &s->io_xy, &s->io_inf}) release(*b);
        delete s;
        s = nullptr;
    }
}

int32_t pointwise_plan(void* out, const pmk::PmPlan& p) {
    if (!out) return fail(nullptr, MSM_ERR_BAD_ARG, "NULL out pointer");
    memcpy(out, &p, sizeof p);
    return MSM_OK;
}

// what the device forms check; scalars: the device array (per-element form) or the host words (one scalar)
int32_t pointwise_check(msm_ctx* c, const void* d_bases, const void* d_inf, const void* scalars, const void* d_scalars, size_t n, uint32_t flags,
                        uint32_t allowed, const void* d_out_xy, const void* d_out_inf) {
    if (!d_bases || !scalars || !d_out_xy || !d_out_inf) return fail(c, MSM_ERR_BAD_ARG, "NULL base, scalar or output pointer");
    if (flags & ~allowed)
        return fail(c, MSM_ERR_BAD_ARG, "flags = 0x%x: only 0x%x is taken here (MSM_NTT_IN_MONT = 2, MSM_FB_OUT_STD = 8, MSM_PM_BASES_STD = 16)", flags, allowed);
    if (((uintptr_t)d_bases | (uintptr_t)d_inf | (uintptr_t)d_scalars | (uintptr_t)d_out_xy | (uintptr_t)d_out_inf) & 15u)
        return fail(c, MSM_ERR_BAD_ARG, "the arrays must be 16-byte aligned");
    if (n == 0) return fail(c, MSM_ERR_EMPTY, "Empty input");
    return MSM_OK;
}

// out[i] = k_i * P_i (uni null) or k * P_i (the halves of k) on st, a launch per PM_LAUNCH_MAX points
template <class G>
int32_t pointwise_enqueue(msm_ctx* c, const uint32_t* d_bases, const uint8_t* d_inf, const uint32_t* d_scalars, const pmk::PmSplit* uni, size_t n,
                          uint32_t flags, uint32_t* d_out_xy, uint8_t* d_out_inf, hipStream_t st) {
    using PW = PointwiseSide<G>;
    const auto kernel = uni ? PW::KERNEL_ONE : PW::KERNEL_EACH;
    for (size_t at = 0; at < n; at += PM_LAUNCH_MAX) {
        const size_t cnt = n - at < PM_LAUNCH_MAX ? n - at : PM_LAUNCH_MAX;
        kernel<<<grid1(cnt, pmk::FB_GROUP), pmk::FB_GROUP, 0, st>>>(d_bases + at * PW::WORDS, d_inf ? d_inf + at : nullptr, uni ? nullptr : d_scalars + at * 8,
                                                                    uni ? *uni : pmk::PmSplit{}, (uint32_t)cnt, flags, d_out_xy + at * PW::WORDS,
                                                                    d_out_inf + at);
    }
    HIPCHK(c, hipGetLastError());
    return MSM_OK;
}

template <class G>
int32_t pointwise_mul_device(msm_ctx* c, const void* d_bases_xy, const void* d_inf_mask, const void* d_scalars, size_t n, uint32_t flags, void* d_out_xy,
                             void* d_out_inf, void* hip_stream) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int32_t rc = pointwise_check(c, d_bases_xy, d_inf_mask, d_scalars, d_scalars, n, flags, MSM_NTT_IN_MONT | MSM_FB_OUT_STD | MSM_PM_BASES_STD, d_out_xy,
                                 d_out_inf);
    if (rc) return rc;
    DeviceGuard g(c->device);
    Range r_(PointwiseSide<G>::RANGE_DEVICE);
    return pointwise_enqueue<G>(c, (const uint32_t*)d_bases_xy, (const uint8_t*)d_inf_mask, (const uint32_t*)d_scalars, nullptr, n, flags,
                                (uint32_t*)d_out_xy, (uint8_t*)d_out_inf, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

template <class G>
int32_t pointwise_scale_device(msm_ctx* c, const void* d_bases_xy, const void* d_inf_mask, const uint32_t* k_std, size_t n, uint32_t flags, void* d_out_xy,
                               void* d_out_inf, void* hip_stream) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int32_t rc = pointwise_check(c, d_bases_xy, d_inf_mask, k_std, nullptr, n, flags, MSM_FB_OUT_STD | MSM_PM_BASES_STD, d_out_xy, d_out_inf);
    if (rc) return rc;
    DeviceGuard g(c->device);
    Range r_(PointwiseSide<G>::RANGE_SCALE);
    const pmk::PmSplit uni = pmk::pm_split_host(k_std);
    return pointwise_enqueue<G>(c, (const uint32_t*)d_bases_xy, (const uint8_t*)d_inf_mask, nullptr, &uni, n, flags, (uint32_t*)d_out_xy,
                                (uint8_t*)d_out_inf, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

template <class G>
int32_t pointwise_mul_host(msm_ctx* c, const uint32_t* bases_xy, uint32_t base_form, const uint8_t* inf_mask, const uint32_t* scalars, size_t n,
                           uint32_t flags, uint32_t* out_xy, uint8_t* out_inf) {
    using PW = PointwiseSide<G>;
    constexpr size_t WORDS = PW::WORDS, BYTES = WORDS * 4;
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!bases_xy || !scalars || !out_xy || !out_inf) return fail(c, MSM_ERR_BAD_ARG, "NULL base, scalar or output pointer");
    if (base_form != MSM_FORM_STD && base_form != MSM_FORM_MONT) return fail(c, MSM_ERR_BAD_ARG, "base_form = %u: MSM_FORM_STD or MSM_FORM_MONT", base_form);
    if (flags & ~(MSM_NTT_IN_MONT | MSM_FB_OUT_STD))
        return fail(c, MSM_ERR_BAD_ARG, "flags = 0x%x: MSM_NTT_IN_MONT and / or MSM_FB_OUT_STD (base_form names the form of the bases)", flags);
    if (n == 0) return fail(c, MSM_ERR_EMPTY, "Empty input");
    DeviceGuard g(c->device);
    Range r_(PW::RANGE_HOST);
    PointwiseState*& s = c->pointwise[PointSide<G>::RESULT];
    if (!s) {
        s = new (std::nothrow) PointwiseState();
        if (!s) return fail(c, MSM_ERR_OOM, "out of host memory");
    }
    int32_t rc;
    const size_t stage = n < PW::STAGE_MAX ? n : PW::STAGE_MAX;
    if ((rc = ensure(c, s->io_k, stage * 32))) return rc;
    if ((rc = ensure(c, s->io_xy, stage * BYTES))) return rc;
    if ((rc = ensure(c, s->io_inf, stage))) return rc;
    HostPin pin_b, pin_k, pin_xy;
    if (!c->no_host_pin) {
        pin_b.pin(bases_xy, n * BYTES);
        pin_k.pin(scalars, n * 32);
        if (out_xy != bases_xy) pin_xy.pin(out_xy, n * BYTES);
    }
    const uint32_t kflags = flags | (base_form == MSM_FORM_STD ? MSM_PM_BASES_STD : 0u);
    for (size_t at = 0; at < n; at += stage) {  // one stream: a chunk's copies out are behind its kernel and in front of the next chunk's copies in
        const size_t cnt = n - at < stage ? n - at : stage;
        if ((rc = h2d(c, s->io_xy.p, bases_xy + at * WORDS, cnt * BYTES, c->stream))) return rc;
        if ((rc = h2d(c, s->io_k.p, scalars + at * 8, cnt * 32, c->stream))) return rc;
        if (inf_mask && (rc = h2d(c, s->io_inf.p, inf_mask + at, cnt, c->stream))) return rc;
        if ((rc = pointwise_enqueue<G>(c, (const uint32_t*)s->io_xy.p, inf_mask ? (const uint8_t*)s->io_inf.p : nullptr, (const uint32_t*)s->io_k.p, nullptr,
                                       cnt, kflags, (uint32_t*)s->io_xy.p, (uint8_t*)s->io_inf.p, c->stream)))
            return rc;
        HIPCHK(c, hipMemcpyAsync(out_xy + at * WORDS, s->io_xy.p, cnt * BYTES, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(out_inf + at, s->io_inf.p, cnt, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MSM_OK;
}

}  // namespace

extern "C" {

int32_t msm_bn254_g1_pointwise_mul_plan(msm_pointwise_plan_t* out) { return pointwise_plan(out, pmk::pm_plan()); }
int32_t msm_bn254_g2_pointwise_mul_plan(msm_pointwise_g2_plan_t* out) { return pointwise_plan(out, pmk::pm2_plan()); }

int32_t msm_bn254_g1_pointwise_mul_device(msm_ctx* c, const void* d_bases_xy, const void* d_inf_mask, const void* d_scalars, size_t n, uint32_t flags,
                                          void* d_out_xy, void* d_out_inf, void* hip_stream) {
    return pointwise_mul_device<HostG1>(c, d_bases_xy, d_inf_mask, d_scalars, n, flags, d_out_xy, d_out_inf, hip_stream);
}
int32_t msm_bn254_g2_pointwise_mul_device(msm_ctx* c, const void* d_bases_xy, const void* d_inf_mask, const void* d_scalars, size_t n, uint32_t flags,
                                          void* d_out_xy, void* d_out_inf, void* hip_stream) {
    return pointwise_mul_device<HostG2>(c, d_bases_xy, d_inf_mask, d_scalars, n, flags, d_out_xy, d_out_inf, hip_stream);
}

int32_t msm_bn254_g1_scale_device(msm_ctx* c, const void* d_bases_xy, const void* d_inf_mask, const uint32_t* k_std, size_t n, uint32_t flags,
                                  void* d_out_xy, void* d_out_inf, void* hip_stream) {
    return pointwise_scale_device<HostG1>(c, d_bases_xy, d_inf_mask, k_std, n, flags, d_out_xy, d_out_inf, hip_stream);
}
int32_t msm_bn254_g2_scale_device(msm_ctx* c, const void* d_bases_xy, const void* d_inf_mask, const uint32_t* k_std, size_t n, uint32_t flags,
                                  void* d_out_xy, void* d_out_inf, void* hip_stream) {
    return pointwise_scale_device<HostG2>(c, d_bases_xy, d_inf_mask, k_std, n, flags, d_out_xy, d_out_inf, hip_stream);
}

int32_t msm_bn254_g1_pointwise_mul(msm_ctx* c, const uint32_t* bases_xy, uint32_t base_form, const uint8_t* inf_mask, const uint32_t* scalars, size_t n,
                                   uint32_t flags, uint32_t* out_xy, uint8_t* out_inf) {
    return pointwise_mul_host<HostG1>(c, bases_xy, base_form, inf_mask, scalars, n, flags, out_xy, out_inf);
}
int32_t msm_bn254_g2_pointwise_mul(msm_ctx* c, const uint32_t* bases_xy, uint32_t base_form, const uint8_t* inf_mask, const uint32_t* scalars, size_t n,
                                   uint32_t flags, uint32_t* out_xy, uint8_t* out_inf) {
    return pointwise_mul_host<HostG2>(c, bases_xy, base_form, inf_mask, scalars, n, flags, out_xy, out_inf);
}

}  // extern "C"
