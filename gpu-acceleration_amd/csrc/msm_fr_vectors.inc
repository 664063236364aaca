// msm_fr_vectors.inc -- the scalars of a setup made in HBM, behind the C ABI: msm_bn254_fr_vector_plan (host only), msm_bn254_fr_powers_device,
// msm_bn254_fr_batch_inverse_device, msm_bn254_fr_batch_inverse, msm_bn254_fr_lagrange_device, msm_bn254_fr_lincomb_device.  Included by
// msm_hip.hip after msm_fixed_base.inc; the per-lane routines and the kernels are fr_vectors_bn254.hpp.
//
// Nothing is kept on the context: every constant a kernel needs (the scale, the powers base^(2^k), the change of form) is prepared on the host
// and travels BY VALUE with the launch, no table, no scratch array, no event.  So two calls on two streams do not wait for each other, and a
// call is one kernel launch.  The host-pointer form of the inversion stages through an allocation of its own that it frees before it returns.

static_assert(sizeof(msm_fr_vector_plan_t) == sizeof(frvk::FrvPlan) && sizeof(frvk::FrvPlan) == 16, "fr_vectors_bn254.hpp mirrors the header's struct");

namespace {

uint32_t frv_group(const msm_ctx* c) { return frvk::frv_group_ok(c->knobs.frv_inv_group) ? c->knobs.frv_inv_group : frvk::FRV_INV_GROUP; }

// what every call here checks: the flags it takes, the count, and (device forms) the alignment of its arrays
int32_t frv_check(msm_ctx* c, uint32_t flags, uint32_t allowed, size_t n, std::initializer_list<const void*> arrays, bool device) {
    if (flags & ~allowed) return fail(c, MSM_ERR_BAD_ARG, "flags = 0x%x: only 0x%x is taken here (MSM_NTT_IN_MONT = 2, MSM_NTT_OUT_MONT = 4)", flags, allowed);
    uintptr_t bits = 0;
    for (const void* p : arrays) bits |= (uintptr_t)p;
    if (device && (bits & 15u)) return fail(c, MSM_ERR_BAD_ARG, "the arrays must be 16-byte aligned");
    if (n == 0) return fail(c, MSM_ERR_EMPTY, "Empty input");
    if (n > ((size_t)1 << frvk::FRV_MAX_LOG2)) return fail(c, MSM_ERR_BAD_ARG, "n = %zu exceeds 2^%u elements", n, frvk::FRV_MAX_LOG2);
    return MSM_OK;
}

template <uint32_t G>
void frv_launch_inverse(const frvk::FrvInverse& a, const uint32_t* d_in, uint32_t* d_out, size_t n, hipStream_t st) {
    frvk::k_frv_batch_inverse<G><<<grid1(frvk::frv_chain_lanes(n, G), frvk::FRV_BLOCK), frvk::FRV_BLOCK, 0, st>>>(a, d_in, d_out, n);
}
int32_t frv_enqueue_inverse(msm_ctx* c, const uint32_t* d_in, uint32_t* d_out, size_t n, uint32_t flags, hipStream_t st) {
    const frvk::FrvInverse a = frvk::frv_inverse_args(flags);
    switch (frv_group(c)) {
        case 4: frv_launch_inverse<4>(a, d_in, d_out, n, st); break;
        case 16: frv_launch_inverse<16>(a, d_in, d_out, n, st); break;
        case 32: frv_launch_inverse<32>(a, d_in, d_out, n, st); break;
        default: frv_launch_inverse<8>(a, d_in, d_out, n, st); break;
    }
    HIPCHK(c, hipGetLastError());
    return MSM_OK;
}

}  // namespace

extern "C" {

int32_t msm_bn254_fr_vector_plan(msm_fr_vector_plan_t* out) {
    if (!out) return fail(nullptr, MSM_ERR_BAD_ARG, "NULL out pointer");
    const frvk::FrvPlan p = frvk::frv_plan();
    memcpy(out, &p, sizeof p);
    return MSM_OK;
}

int32_t msm_bn254_fr_powers_device(msm_ctx* c, const uint32_t* base_std, const uint32_t* scale_std, uint64_t first, void* d_out, size_t n,
                                   uint32_t flags, void* hip_stream) {
    using namespace frvk;
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!base_std || !d_out) return fail(c, MSM_ERR_BAD_ARG, "NULL base or output pointer");
    int32_t rc = frv_check(c, flags, MSM_NTT_OUT_MONT, n, {d_out}, true);
    if (rc) return rc;
    if (first + n < first) return fail(c, MSM_ERR_BAD_ARG, "first + n exceeds 64 bits");
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_powers_device");
    const FrvPowers a = frv_powers_args(fr_from_std(base_std), scale_std ? fr_from_std(scale_std) : fr_one(), first, flags);
    k_frv_powers<<<grid1(frv_powers_lanes(n), FRV_BLOCK), FRV_BLOCK, 0, hip_stream ? (hipStream_t)hip_stream : c->stream>>>(a, (uint32_t*)d_out, n);
    HIPCHK(c, hipGetLastError());
    return MSM_OK;
}

int32_t msm_bn254_fr_batch_inverse_device(msm_ctx* c, const void* d_in, void* d_out, size_t n, uint32_t flags, void* hip_stream) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!d_in || !d_out) return fail(c, MSM_ERR_BAD_ARG, "NULL input or output pointer");
    int32_t rc = frv_check(c, flags, MSM_NTT_IN_MONT | MSM_NTT_OUT_MONT, n, {d_in, d_out}, true);
    if (rc) return rc;
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_batch_inverse_device");
    return frv_enqueue_inverse(c, (const uint32_t*)d_in, (uint32_t*)d_out, n, flags, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int32_t msm_bn254_fr_batch_inverse(msm_ctx* c, const uint32_t* in, uint32_t* out, size_t n, uint32_t flags) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!in || !out) return fail(c, MSM_ERR_BAD_ARG, "NULL input or output pointer");
    int32_t rc = frv_check(c, flags, MSM_NTT_IN_MONT | MSM_NTT_OUT_MONT, n, {}, false);
    if (rc) return rc;
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_batch_inverse");
    const size_t bytes = n * 32;
    HostPin pin_i, pin_o;
    if (!c->no_host_pin) {
        pin_i.pin(in, bytes);
        if (out != in) pin_o.pin(out, bytes);
    }
    DevTmp io;  // (freed on every way out: the context keeps nothing of this call)
    HIPCHK(c, hipMalloc(&io.p, bytes));
    if ((rc = h2d(c, io.p, in, bytes, c->stream))) return rc;
    if ((rc = frv_enqueue_inverse(c, (const uint32_t*)io.p, (uint32_t*)io.p, n, flags, c->stream))) return rc;
    HIPCHK(c, hipMemcpyAsync(out, io.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MSM_OK;
}

int32_t msm_bn254_fr_lagrange_device(msm_ctx* c, const uint32_t* tau_std, uint32_t log_n, void* d_out, uint32_t flags, void* hip_stream) {
    using namespace frvk;
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!tau_std || !d_out) return fail(c, MSM_ERR_BAD_ARG, "NULL tau or output pointer");
    if (log_n > NTT_MAX_LOG2) return fail(c, MSM_ERR_BAD_ARG, "log_n = %u: r - 1 has 28 factors of two", log_n);
    int32_t rc = frv_check(c, flags, MSM_NTT_OUT_MONT, (size_t)1 << log_n, {d_out}, true);
    if (rc) return rc;
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_lagrange_device");
    const FrvLagrange a = frv_lagrange_args(fr_from_std(tau_std), log_n, flags);
    constexpr uint32_t G = FRV_INV_GROUP;
    const size_t n = (size_t)1 << log_n;
    k_frv_lagrange<G><<<grid1(frv_chain_lanes(n, G), FRV_BLOCK), FRV_BLOCK, 0, hip_stream ? (hipStream_t)hip_stream : c->stream>>>(a, (uint32_t*)d_out, n);
    HIPCHK(c, hipGetLastError());
    return MSM_OK;
}

int32_t msm_bn254_fr_lincomb_device(msm_ctx* c, const void* d_a, const uint32_t* ka_std, const void* d_b, const uint32_t* kb_std, const void* d_c,
                                    const uint32_t* kc_std, void* d_out, size_t n, uint32_t flags, void* hip_stream) {
    using namespace frvk;
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!d_a || !d_out) return fail(c, MSM_ERR_BAD_ARG, "NULL first operand or output pointer");
    int32_t rc = frv_check(c, flags, MSM_NTT_IN_MONT | MSM_NTT_OUT_MONT, n, {d_a, d_b, d_c, d_out}, true);
    if (rc) return rc;
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_lincomb_device");
    auto coef = [](const uint32_t* k) { return k ? fr_from_std(k) : fr_one(); };
    const FrvLincomb k = frv_lincomb_args(coef(ka_std), coef(kb_std), coef(kc_std), flags);
    k_frv_lincomb<<<grid1(n, FRV_BLOCK), FRV_BLOCK, 0, hip_stream ? (hipStream_t)hip_stream : c->stream>>>(k, (const uint32_t*)d_a, (const uint32_t*)d_b,
                                                                                                        (const uint32_t*)d_c, (uint32_t*)d_out, n);
    HIPCHK(c, hipGetLastError());
    return MSM_OK;
}

}  // extern "C"
