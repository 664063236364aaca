// msm_fixed_base.inc -- the fixed-base batch multiplication of both groups behind the C ABI: msm_bn254_g1_fixed_base_plan (host only),
// msm_bn254_g1_fixed_base_mul_device, msm_bn254_g1_fixed_base_mul and the same three with _g2_.  Included by msm_hip.hip after msm_r1cs.inc; the
// routines are fixed_base_bn254.hpp / fixed_base_g2_bn254.hpp, the kernels msm_kernels_fixed_base.hpp / msm_kernels_fixed_base_g2.hpp.
//
// Shared between the groups, over FixedBaseSide<G>: the argument checks, the state with its event, the plan call, the device form and the staging
// loop of the host-pointer form.  Per group: the curve check of the base, G2's subgroup check, and the enqueue (one kernel per launch for G1;
// for G2 the products go through a scratch array and a chunk is two kernels).
//
// Per context and group (msm_ctx::fixed_base / fixed_base_g2, made by the first call; two objects, so a setup that alternates G1 and G2 queries
// rebuilds neither table): the window table of the latest (base, c), the staging arrays of the host-pointer call and, for G2, the XYZZ scratch
// array of one chunk.  A call only ENQUEUES -- the table build too, on the call's stream; table and scratch are shared by all streams a context
// is used with, so every call leaves an event behind and a call on ANOTHER stream waits for it first (the idiom of msm_ntt.inc).
// The G2 base is checked on the host: on the twist every call, and [r]Q = O (host_g2.hpp's jdbl / jadd, 254 doublings) whenever it is not the
// base the table was built from -- the twist's cofactor is not 1, and reading k as (k mod r) is only right in the subgroup.

static_assert(sizeof(msm_fixed_base_plan_t) == sizeof(fbk::FbPlan), "fixed_base_bn254.hpp mirrors the header's struct");
static_assert(sizeof(msm_fixed_base_g2_plan_t) == sizeof(fbk::Fb2Plan) && sizeof(fbk::Fb2Plan) == 40, "fixed_base_g2_bn254.hpp mirrors the header's struct");
static_assert(MSM_FB_OUT_STD == fbk::FB_F_OUT_STD && MSM_NTT_IN_MONT == fbk::FB_F_IN_MONT, "fixed_base_bn254.hpp mirrors the header's constants");

struct FixedBaseCommon {
    DevBuf table, io_k, io_xy, io_inf;
    uint32_t c = 0;           // 0: no table
    hipEvent_t ev = nullptr;  // behind the latest call
    hipStream_t last_stream = nullptr;
    bool used = false;
};
struct FixedBaseState : FixedBaseCommon {
    fbk::FbBase base{};  // Montgomery words of the base the table was built from
};
struct FixedBaseG2State : FixedBaseCommon {
    DevBuf scratch;
    fbk::Fb2Base base{};     // Montgomery words of the base the table was built from
    bool have_base = false;  // `base` has passed the subgroup check (it stays so when its table is dropped)
};

namespace {

constexpr size_t FB_LAUNCH_MAX = (size_t)1 << 30;  // points per launch (a multiple of 16: the chunks' arrays stay aligned)

// A group's side of the shared bodies: its plan, base and state, words per affine record, points the host-pointer call stages at a time
template <class G>
struct FixedBaseSide;
template <>
struct FixedBaseSide<HostG1> {
    using Plan = fbk::FbPlan;
    using Base = fbk::FbBase;
    using State = FixedBaseState;
    static constexpr size_t WORDS = 16;
    static constexpr const char* RANGE_DEVICE = "msm_bn254_g1_fixed_base_mul_device";
    static constexpr const char* RANGE_HOST = "msm_bn254_g1_fixed_base_mul";
    static bool plan(uint32_t window_bits, Plan& p) { return fbk::fb_plan(window_bits, p); }
    static State*& state(msm_ctx* c) { return c->fixed_base; }
    static size_t stage_max(const Plan&) { return (size_t)1 << 20; }
};
template <>
struct FixedBaseSide<HostG2> {
    using Plan = fbk::Fb2Plan;
    using Base = fbk::Fb2Base;
    using State = FixedBaseG2State;
    static constexpr size_t WORDS = 32;
    static constexpr const char* RANGE_DEVICE = "msm_bn254_g2_fixed_base_mul_device";
    static constexpr const char* RANGE_HOST = "msm_bn254_g2_fixed_base_mul";
    static bool plan(uint32_t window_bits, Plan& p) { return fbk::fb2_plan(window_bits, p); }
    static State*& state(msm_ctx* c) { return c->fixed_base_g2; }
    static size_t stage_max(const Plan& p) { return p.chunk_points; }  // a staging step is one chunk of the scratch array
};

void fixed_base_release(msm_ctx* c) {
    if (c->fixed_base_g2) release(c->fixed_base_g2->scratch);
    for (FixedBaseCommon* s : std::initializer_list<FixedBaseCommon*>{c->fixed_base, c->fixed_base_g2}) {
        if (!s) continue;
        for (DevBuf* b : {&s->table, &s->io_k, &s->io_xy, &s->io_inf}) release(*b);
        if (s->ev) (void)hipEventDestroy(s->ev);
    }
    delete c->fixed_base;
    delete c->fixed_base_g2;
    c->fixed_base = nullptr;
    c->fixed_base_g2 = nullptr;
}

// ---- per group: the base on its curve (it comes back as Montgomery words), in its group ----

int32_t fixed_base_on_curve(msm_ctx* c, const uint32_t* base_xy, uint32_t base_form, fbk::FbBase& base) {
    using namespace hostg1;
    Fq x = load_words(base_xy), y = load_words(base_xy + 8);
    if (geq_mod(x) || geq_mod(y)) return fail(c, MSM_ERR_INVALID_DATA, "a coordinate of the base is not below p");
    if (base_form == MSM_FORM_STD) x = to_mont(x), y = to_mont(y);
    const Fq three = add(ONE, dbl(ONE));
    if (!is_zero(sub(sqr(y), add(mul(sqr(x), x), three)))) return fail(c, MSM_ERR_INVALID_DATA, "the base is not on the curve y^2 = x^3 + 3");
    store_words(base.w, x);
    store_words(base.w + 8, y);
    return MSM_OK;
}

// 3 / (9 + u), Montgomery form
const hostg2::Fq2& fixed_base_g2_twist_b() {
    static const hostg2::Fq2 b = [] {
        using namespace hostg1;
        const Fq three = add(ONE, dbl(ONE));
        return hostg2::mul(hostg2::Fq2{three, Fq{{0, 0, 0, 0}}}, hostg2::inv(hostg2::Fq2{add(dbl(dbl(dbl(ONE))), ONE), ONE}));
    }();
    return b;
}
int32_t fixed_base_on_curve(msm_ctx* c, const uint32_t* base_xy, uint32_t base_form, fbk::Fb2Base& base) {
    using namespace hostg2;
    Fq2 x = load_words(base_xy), y = load_words(base_xy + 16);
    if (hostg1::geq_mod(x.c0) || hostg1::geq_mod(x.c1) || hostg1::geq_mod(y.c0) || hostg1::geq_mod(y.c1))
        return fail(c, MSM_ERR_INVALID_DATA, "a component of the base is not below p (curve check)");
    if (base_form == MSM_FORM_STD) {
        x = Fq2{hostg1::to_mont(x.c0), hostg1::to_mont(x.c1)};
        y = Fq2{hostg1::to_mont(y.c0), hostg1::to_mont(y.c1)};
    }
    if (!is_zero(sub(sqr(y), add(mul(sqr(x), x), fixed_base_g2_twist_b()))))
        return fail(c, MSM_ERR_INVALID_DATA, "the base is not on the curve y^2 = x^3 + 3/(9+u)");
    store_words(base.w, x);
    store_words(base.w + 16, y);
    return MSM_OK;
}

// [r]Q == O for a point of the twist (Montgomery words)
bool fixed_base_g2_in_subgroup(const fbk::Fb2Base& base) {
    static constexpr uint64_t R_ORDER[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
    const hostg2::Jac q{hostg2::load_words(base.w), hostg2::load_words(base.w + 16), hostg2::one()};
    hostg2::Jac acc = hostg2::identity();
    for (int b = 253; b >= 0; b--) {
        acc = hostg2::jdbl(acc);
        if ((R_ORDER[b >> 6] >> (b & 63)) & 1ull) acc = hostg2::jadd(acc, q);
    }
    return hostg2::is_identity(acc);
}
int32_t fixed_base_in_group(msm_ctx*, const FixedBaseState&, const fbk::FbBase&) { return MSM_OK; }  // the curve's order is r
// the subgroup check of a base the state has not seen
int32_t fixed_base_in_group(msm_ctx* c, const FixedBaseG2State& s, const fbk::Fb2Base& base) {
    if (!(s.have_base && memcmp(&s.base, &base, sizeof base) == 0) && !fixed_base_g2_in_subgroup(base))
        return fail(c, MSM_ERR_INVALID_DATA, "the base is on the twist but not in G2: [r]Q is not the identity (subgroup check)");
    return MSM_OK;
}

// ---- per group: the table if (base, c) changed, then the products, on st; the context's mutex is held ----

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

// G2: the products chunk by chunk through the scratch array
int32_t fixed_base_enqueue(msm_ctx* c, const fbk::Fb2Plan& plan, const fbk::Fb2Base& base, const uint32_t* d_scalars, size_t n, uint32_t flags,
                           uint32_t* d_out_xy, uint8_t* d_out_inf, hipStream_t st) {
    using namespace fbk;
    FixedBaseG2State* s = c->fixed_base_g2;
    if (s->used && s->last_stream != st) HIPCHK(c, hipStreamWaitEvent(st, s->ev, 0));
    const uint32_t cw = plan.window_bits, W = plan.num_windows;
    const uint32_t G = c->knobs.fb2_inv_group ? c->knobs.fb2_inv_group : plan.inv_group;
    const size_t chunk = plan.chunk_points, stride = n < chunk ? (n + 15) & ~(size_t)15 : chunk;  // columns of the scratch array
    const bool new_table = s->c != cw || memcmp(&s->base, &base, sizeof base) != 0;
    const size_t need_table = (size_t)plan.table_bytes, need_scratch = stride * FB2_SLOT_WORDS * 4;
    if ((new_table && s->table.cap < need_table) || s->scratch.cap < need_scratch) {
        if (s->used) HIPCHK(c, hipEventSynchronize(s->ev));  // an earlier call may still use what is freed
        int32_t rc;
        if (new_table && s->table.cap < need_table) {
            s->c = 0;
            if ((rc = ensure(c, s->table, need_table))) return rc;
        }
        if ((rc = ensure(c, s->scratch, need_scratch))) return rc;
    }
    if (new_table) {
        s->c = 0;
        s->base = base;  // (checked by fixed_base_in_group)
        s->have_base = true;
        uint32_t* table = (uint32_t*)s->table.p;
        k_fb2_window_bases<<<dim3(1), FB_GROUP, 0, st>>>(base, cw, W, table);
        for (uint32_t L = 1; L < cw; L++)
            k_fb2_table_level<<<grid1(fb_level_entries(W, L), FB_GROUP), FB_GROUP, 0, st>>>(table, cw, L, fb_level_entries(W, L));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(s->ev, st));  // (the table is in flight: a failure below must not leave it unguarded)
        s->used = true;
        s->last_stream = st;
        s->c = cw;
    }
    for (size_t at = 0; at < n; at += chunk) {  // one stream: a chunk's normalisation is behind its products and in front of the next chunk's
        const size_t cnt = n - at < chunk ? n - at : chunk;
        k_fb2_accumulate<<<grid1(cnt, FB2_BLOCK), FB2_BLOCK, 0, st>>>((const uint32_t*)s->table.p, cw, W, d_scalars + at * 8, (uint32_t)cnt, flags,
                                                                     (uint32_t*)s->scratch.p, (uint32_t)stride);
        k_fb2_normalise<<<grid1(fb2_chain_lanes(cnt, G), FB2_BLOCK), FB2_BLOCK, 0, st>>>((uint32_t*)s->scratch.p, (uint32_t)stride, (uint32_t)cnt, G, flags,
                                                                                         d_out_xy + at * FB2_REC_WORDS, d_out_inf + at);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(s->ev, st));
    s->used = true;
    s->last_stream = st;
    return MSM_OK;
}

// ---- shared ----

template <class G>
int32_t fixed_base_plan(uint32_t window_bits, void* out) {
    if (!out) return fail(nullptr, MSM_ERR_BAD_ARG, "NULL out pointer");
    typename FixedBaseSide<G>::Plan p;
    if (!FixedBaseSide<G>::plan(window_bits, p))
        return fail(nullptr, MSM_ERR_BAD_ARG, "window_bits = %u: 0 or %u..%u", window_bits, fbk::FB_C_MIN, fbk::FB_C_MAX);
    memcpy(out, &p, sizeof p);
    return MSM_OK;
}

// arguments both forms share; the base comes back as Montgomery words, on its curve
template <class G>
int32_t fixed_base_check(msm_ctx* c, const uint32_t* base_xy, uint32_t base_form, const void* scalars, size_t n, uint32_t window_bits, uint32_t flags,
                         const void* out_xy, const void* out_inf, typename FixedBaseSide<G>::Plan& plan, typename FixedBaseSide<G>::Base& base) {
    if (!base_xy || !scalars || !out_xy || !out_inf) return fail(c, MSM_ERR_BAD_ARG, "NULL base, scalar or output pointer");
    if (base_form != MSM_FORM_STD && base_form != MSM_FORM_MONT) return fail(c, MSM_ERR_BAD_ARG, "base_form = %u: MSM_FORM_STD or MSM_FORM_MONT", base_form);
    if (flags & ~(MSM_NTT_IN_MONT | MSM_FB_OUT_STD)) return fail(c, MSM_ERR_BAD_ARG, "flags = 0x%x: MSM_NTT_IN_MONT and / or MSM_FB_OUT_STD", flags);
    if (!FixedBaseSide<G>::plan(window_bits, plan))
        return fail(c, MSM_ERR_BAD_ARG, "window_bits = %u: 0 or %u..%u", window_bits, fbk::FB_C_MIN, fbk::FB_C_MAX);
    if (n == 0) return fail(c, MSM_ERR_EMPTY, "Empty input");
    return fixed_base_on_curve(c, base_xy, base_form, base);
}

// the context's state of the group, and the group check of the base
template <class G>
int32_t fixed_base_state(msm_ctx* c, const typename FixedBaseSide<G>::Base& base) {
    using State = typename FixedBaseSide<G>::State;
    State*& s = FixedBaseSide<G>::state(c);
    if (!s) {
        State* made = new (std::nothrow) State();
        if (!made) return fail(c, MSM_ERR_OOM, "out of host memory");
        hipError_t e = hipEventCreateWithFlags(&made->ev, hipEventDisableTiming);
        if (e != hipSuccess) {
            delete made;
            return fail(c, MSM_ERR_HIP, "hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
        }
        s = made;
    }
    return fixed_base_in_group(c, *s, base);
}

template <class G>
int32_t fixed_base_mul_device(msm_ctx* c, const uint32_t* base_xy, uint32_t base_form, const void* d_scalars, size_t n, uint32_t window_bits,
                              uint32_t flags, void* d_out_xy, void* d_out_inf, void* hip_stream) {
    using FB = FixedBaseSide<G>;
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    typename FB::Plan plan;
    typename FB::Base base;
    int32_t rc = fixed_base_check<G>(c, base_xy, base_form, d_scalars, n, window_bits, flags, d_out_xy, d_out_inf, plan, base);
    if (rc) return rc;
    if (((uintptr_t)d_scalars | (uintptr_t)d_out_xy | (uintptr_t)d_out_inf) & 15u) return fail(c, MSM_ERR_BAD_ARG, "the arrays must be 16-byte aligned");
    DeviceGuard g(c->device);
    Range r_(FB::RANGE_DEVICE);
    if ((rc = fixed_base_state<G>(c, base))) return rc;
    return fixed_base_enqueue(c, plan, base, (const uint32_t*)d_scalars, n, flags, (uint32_t*)d_out_xy, (uint8_t*)d_out_inf,
                              hip_stream ? (hipStream_t)hip_stream : c->stream);
}

template <class G>
int32_t fixed_base_mul_host(msm_ctx* c, const uint32_t* base_xy, uint32_t base_form, const uint32_t* scalars, size_t n, uint32_t window_bits,
                            uint32_t flags, uint32_t* out_xy, uint8_t* out_inf) {
    using FB = FixedBaseSide<G>;
    constexpr size_t WORDS = FB::WORDS, BYTES = WORDS * 4;
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    typename FB::Plan plan;
    typename FB::Base base;
    int32_t rc = fixed_base_check<G>(c, base_xy, base_form, scalars, n, window_bits, flags, out_xy, out_inf, plan, base);
    if (rc) return rc;
    DeviceGuard g(c->device);
    Range r_(FB::RANGE_HOST);
    if ((rc = fixed_base_state<G>(c, base))) return rc;
    typename FB::State* s = FB::state(c);
    HostPin pin_k, pin_xy;
    if (!c->no_host_pin) {
        pin_k.pin(scalars, n * 32);
        pin_xy.pin(out_xy, n * BYTES);
    }
    const size_t stage = n < FB::stage_max(plan) ? n : FB::stage_max(plan);
    if ((rc = ensure(c, s->io_k, stage * 32))) return rc;
    if ((rc = ensure(c, s->io_xy, stage * BYTES))) return rc;
    if ((rc = ensure(c, s->io_inf, stage))) return rc;
    for (size_t at = 0; at < n; at += stage) {  // one stream: a chunk's copies out are behind its kernels and in front of the next chunk's copy in
        const size_t cnt = n - at < stage ? n - at : stage;
        if ((rc = h2d(c, s->io_k.p, scalars + at * 8, cnt * 32, c->stream))) return rc;
        if ((rc = fixed_base_enqueue(c, plan, base, (const uint32_t*)s->io_k.p, cnt, flags, (uint32_t*)s->io_xy.p, (uint8_t*)s->io_inf.p, c->stream)))
            return rc;
        HIPCHK(c, hipMemcpyAsync(out_xy + at * WORDS, s->io_xy.p, cnt * BYTES, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(out_inf + at, s->io_inf.p, cnt, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MSM_OK;
}

}  // namespace

extern "C" {

int32_t msm_bn254_g1_fixed_base_plan(uint32_t window_bits, msm_fixed_base_plan_t* out) { return fixed_base_plan<HostG1>(window_bits, out); }
int32_t msm_bn254_g2_fixed_base_plan(uint32_t window_bits, msm_fixed_base_g2_plan_t* out) { return fixed_base_plan<HostG2>(window_bits, out); }

int32_t msm_bn254_g1_fixed_base_mul_device(msm_ctx* c, const uint32_t* base_xy, uint32_t base_form, const void* d_scalars, size_t n,
                                           uint32_t window_bits, uint32_t flags, void* d_out_xy, void* d_out_inf, void* hip_stream) {
    return fixed_base_mul_device<HostG1>(c, base_xy, base_form, d_scalars, n, window_bits, flags, d_out_xy, d_out_inf, hip_stream);
}
int32_t msm_bn254_g2_fixed_base_mul_device(msm_ctx* c, const uint32_t* base_xy, uint32_t base_form, const void* d_scalars, size_t n,
                                           uint32_t window_bits, uint32_t flags, void* d_out_xy, void* d_out_inf, void* hip_stream) {
    return fixed_base_mul_device<HostG2>(c, base_xy, base_form, d_scalars, n, window_bits, flags, d_out_xy, d_out_inf, hip_stream);
}

int32_t msm_bn254_g1_fixed_base_mul(msm_ctx* c, const uint32_t* base_xy, uint32_t base_form, const uint32_t* scalars, size_t n, uint32_t window_bits,
                                    uint32_t flags, uint32_t* out_xy, uint8_t* out_inf) {
    return fixed_base_mul_host<HostG1>(c, base_xy, base_form, scalars, n, window_bits, flags, out_xy, out_inf);
}
int32_t msm_bn254_g2_fixed_base_mul(msm_ctx* c, const uint32_t* base_xy, uint32_t base_form, const uint32_t* scalars, size_t n, uint32_t window_bits,
                                    uint32_t flags, uint32_t* out_xy, uint8_t* out_inf) {
    return fixed_base_mul_host<HostG2>(c, base_xy, base_form, scalars, n, window_bits, flags, out_xy, out_inf);
}

}  // extern "C"
