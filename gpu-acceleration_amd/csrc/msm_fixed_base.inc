// msm_fixed_base.inc -- the G1 fixed-base batch multiplication behind the C ABI: msm_bn254_g1_fixed_base_plan (host only),
// msm_bn254_g1_fixed_base_mul_device, msm_bn254_g1_fixed_base_mul.  Included by msm_hip.hip after msm_r1cs.inc; the routines are
// fixed_base_bn254.hpp, the kernels msm_kernels_fixed_base.hpp.
//
// Per context (msm_ctx::fixed_base, made by the first call): the window table of the latest (base, c) and the
// staging arrays of the host-pointer call.  A call only ENQUEUES -- the table build too, on the call's stream; the table is shared by all streams
// a context is used with, so every call leaves an event behind and a call on ANOTHER stream waits for it first (the idiom of msm_ntt.inc).

static_assert(sizeof(msm_fixed_base_plan_t) == sizeof(fbk::FbPlan), "fixed_base_bn254.hpp mirrors the header's struct");
static_assert(MSM_FB_OUT_STD == fbk::FB_F_OUT_STD && MSM_NTT_IN_MONT == fbk::FB_F_IN_MONT, "fixed_base_bn254.hpp mirrors the header's constants");

struct FixedBaseState {
    DevBuf table, io_k, io_xy, io_inf;
    fbk::FbBase base{};  // Montgomery words of the base the table was built from
    uint32_t c = 0;      // 0: no table
    hipEvent_t ev = nullptr;  // behind the latest call
    hipStream_t last_stream = nullptr;
    bool used = false;
};

namespace {

constexpr size_t FB_LAUNCH_MAX = (size_t)1 << 30;  // points per launch (a multiple of 16: the chunks' arrays stay aligned)
constexpr size_t FB_STAGE_MAX = (size_t)1 << 20;   // points the host-pointer call stages at a time

void fixed_base_release(msm_ctx* c) {
    FixedBaseState* s = c->fixed_base;
    if (!s) return;
    for (DevBuf* b : {&s->table, &s->io_k, &s->io_xy, &s->io_inf}) release(*b);
    if (s->ev) (void)hipEventDestroy(s->ev);
    delete s;
    c->fixed_base = nullptr;
}

// arguments both forms share; the base comes back as Montgomery words
int32_t fixed_base_check(msm_ctx* c, const uint32_t* base_xy, uint32_t base_form, const void* scalars, size_t n, uint32_t window_bits,
                         uint32_t flags, const void* out_xy, const void* out_inf, fbk::FbPlan& plan, fbk::FbBase& base) {
    using namespace hostg1;
    if (!base_xy || !scalars || !out_xy || !out_inf) return fail(c, MSM_ERR_BAD_ARG, "NULL base, scalar or output pointer");
    if (base_form != MSM_FORM_STD && base_form != MSM_FORM_MONT) return fail(c, MSM_ERR_BAD_ARG, "base_form = %u: MSM_FORM_STD or MSM_FORM_MONT", base_form);
    if (flags & ~(MSM_NTT_IN_MONT | MSM_FB_OUT_STD)) return fail(c, MSM_ERR_BAD_ARG, "flags = 0x%x: MSM_NTT_IN_MONT and / or MSM_FB_OUT_STD", flags);
    if (!fbk::fb_plan(window_bits, plan)) return fail(c, MSM_ERR_BAD_ARG, "window_bits = %u: 0 or %u..%u", window_bits, fbk::FB_C_MIN, fbk::FB_C_MAX);
    if (n == 0) return fail(c, MSM_ERR_EMPTY, "Empty input");
    Fq x = load_words(base_xy), y = load_words(base_xy + 8);
    if (geq_mod(x) || geq_mod(y)) return fail(c, MSM_ERR_INVALID_DATA, "a coordinate of the base is not below p");
    if (base_form == MSM_FORM_STD) x = to_mont(x), y = to_mont(y);
    const Fq three = add(ONE, dbl(ONE));
    if (!is_zero(sub(sqr(y), add(mul(sqr(x), x), three)))) return fail(c, MSM_ERR_INVALID_DATA, "the base is not on the curve y^2 = x^3 + 3");
    store_words(base.w, x);
    store_words(base.w + 8, y);
    return MSM_OK;
}

int32_t fixed_base_state(msm_ctx* c) {
    if (c->fixed_base) return MSM_OK;
    FixedBaseState* s = new (std::nothrow) FixedBaseState();
    if (!s) return fail(c, MSM_ERR_OOM, "out of host memory");
    hipError_t e = hipEventCreateWithFlags(&s->ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        delete s;
        return fail(c, MSM_ERR_HIP, "hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
    }
    c->fixed_base = s;
    return MSM_OK;
}

// the table if (base, c) changed, then the products, on st; the context's mutex is held
int32_t fixed_base_enqueue(msm_ctx* c, const fbk::FbPlan& plan, const fbk::FbBase& base, const uint32_t* d_scalars, size_t n, uint32_t flags,
                           uint32_t* d_out_xy, uint8_t* d_out_inf, hipStream_t st) {
    using namespace fbk;
    FixedBaseState* s = c->fixed_base;
    if (s->used && s->last_stream != st) HIPCHK(c, hipStreamWaitEvent(st, s->ev, 0));
    const uint32_t cw = plan.window_bits, W = plan.num_windows;
    if (s->c != cw || memcmp(&s->base, &base, sizeof base) != 0) {
        const size_t need = (size_t)plan.table_bytes;
        if (s->table.cap < need) {
            if (s->used) HIPCHK(c, hipEventSynchronize(s->ev));  // an earlier call may still read the table that is freed
            s->c = 0;
            int32_t rc = ensure(c, s->table, need);
            if (rc) return rc;
        }
        s->c = 0;
        uint32_t* table = (uint32_t*)s->table.p;
        k_fb_window_bases<<<dim3(1), FB_GROUP, 0, st>>>(base, cw, W, table);
        for (uint32_t L = 1; L < cw; L++)
            k_fb_table_level<<<grid1(fb_level_entries(W, L), FB_GROUP), FB_GROUP, 0, st>>>(table, cw, L, fb_level_entries(W, L));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(s->ev, st));  // (the table is in flight: a failure below must not leave it unguarded)
        s->used = true;
        s->last_stream = st;
        s->base = base;
        s->c = cw;
    }
    for (size_t at = 0; at < n; at += FB_LAUNCH_MAX) {
        const size_t cnt = n - at < FB_LAUNCH_MAX ? n - at : FB_LAUNCH_MAX;
        k_fb_mul<<<grid1(cnt, FB_GROUP), FB_GROUP, 0, st>>>((const uint32_t*)s->table.p, cw, W, d_scalars + at * 8, (uint32_t)cnt, flags,
                                                            d_out_xy + at * 16, d_out_inf + at);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(s->ev, st));
    s->used = true;
    s->last_stream = st;
    return MSM_OK;
}

}  // namespace

extern "C" {

int32_t msm_bn254_g1_fixed_base_plan(uint32_t window_bits, msm_fixed_base_plan_t* out) {
    if (!out) return fail(nullptr, MSM_ERR_BAD_ARG, "NULL out pointer");
    fbk::FbPlan p;
    if (!fbk::fb_plan(window_bits, p)) return fail(nullptr, MSM_ERR_BAD_ARG, "window_bits = %u: 0 or %u..%u", window_bits, fbk::FB_C_MIN, fbk::FB_C_MAX);
    memcpy(out, &p, sizeof p);
    return MSM_OK;
}

int32_t msm_bn254_g1_fixed_base_mul_device(msm_ctx* c, const uint32_t* base_xy, uint32_t base_form, const void* d_scalars, size_t n,
                                           uint32_t window_bits, uint32_t flags, void* d_out_xy, void* d_out_inf, void* hip_stream) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    fbk::FbPlan plan;
    fbk::FbBase base;
    int32_t rc = fixed_base_check(c, base_xy, base_form, d_scalars, n, window_bits, flags, d_out_xy, d_out_inf, plan, base);
    if (rc) return rc;
    if (((uintptr_t)d_scalars | (uintptr_t)d_out_xy | (uintptr_t)d_out_inf) & 15u) return fail(c, MSM_ERR_BAD_ARG, "the arrays must be 16-byte aligned");
    DeviceGuard g(c->device);
    Range r_("msm_bn254_g1_fixed_base_mul_device");
    if ((rc = fixed_base_state(c))) return rc;
    return fixed_base_enqueue(c, plan, base, (const uint32_t*)d_scalars, n, flags, (uint32_t*)d_out_xy, (uint8_t*)d_out_inf,
                              hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int32_t msm_bn254_g1_fixed_base_mul(msm_ctx* c, const uint32_t* base_xy, uint32_t base_form, const uint32_t* scalars, size_t n,
                                    uint32_t window_bits, uint32_t flags, uint32_t* out_xy, uint8_t* out_inf) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    fbk::FbPlan plan;
    fbk::FbBase base;
    int32_t rc = fixed_base_check(c, base_xy, base_form, scalars, n, window_bits, flags, out_xy, out_inf, plan, base);
    if (rc) return rc;
    DeviceGuard g(c->device);
    Range r_("msm_bn254_g1_fixed_base_mul");
    if ((rc = fixed_base_state(c))) return rc;
    FixedBaseState* s = c->fixed_base;
    HostPin pin_k, pin_xy;
    if (!c->no_host_pin) {
        pin_k.pin(scalars, n * 32);
        pin_xy.pin(out_xy, n * 64);
    }
    const size_t stage = n < FB_STAGE_MAX ? n : FB_STAGE_MAX;
    if ((rc = ensure(c, s->io_k, stage * 32))) return rc;
    if ((rc = ensure(c, s->io_xy, stage * 64))) return rc;
    if ((rc = ensure(c, s->io_inf, stage))) return rc;
    for (size_t at = 0; at < n; at += stage) {  // one stream: a chunk's copies out are behind its kernel and in front of the next chunk's copy in
        const size_t cnt = n - at < stage ? n - at : stage;
        if ((rc = h2d(c, s->io_k.p, scalars + at * 8, cnt * 32, c->stream))) return rc;
        if ((rc = fixed_base_enqueue(c, plan, base, (const uint32_t*)s->io_k.p, cnt, flags, (uint32_t*)s->io_xy.p, (uint8_t*)s->io_inf.p, c->stream)))
            return rc;
        HIPCHK(c, hipMemcpyAsync(out_xy + at * 16, s->io_xy.p, cnt * 64, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(out_inf + at, s->io_inf.p, cnt, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MSM_OK;
}

}  // extern "C"
