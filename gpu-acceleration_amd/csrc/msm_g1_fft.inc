// msm_g1_fft.inc -- the group transforms of both groups behind the C ABI: msm_bn254_g1_fft_plan (host only), msm_bn254_g1_fft_device,
// msm_bn254_g1_fft and the same three with _g2_.  Included by msm_hip.hip after msm_pointwise.inc; the routines are g1_fft_bn254.hpp /
// g2_fft_bn254.hpp, the kernels msm_kernels_g1_fft.hpp / msm_kernels_g2_fft.hpp.  The host side is one body per call, over GroupFftSide<G>: the
// record width, the kernels and the names of the ranges are all that differ between the groups.
//
// Per context (msm_ctx::group_fft, made on first use): one table of the n / 2 powers of w in standard form per log_n >= 2 that was asked for,
// built on the call's stream by the powers kernel of fr_vectors_bn254.hpp, with an event behind the build; a call on another stream waits for
// that event (two streams that first build a table order themselves; afterwards nothing is shared that is written).  One table serves both
// directions AND both groups: the twiddles are scalars (g1_fft_bn254.hpp).  The host-pointer forms add their staging arrays, shared as well.
// A call is: the bit-reversal sweep, log_n stage launches per 2^30 butterflies, and for the inverse one pass of k_pm_mul<true> resp.
// k_pm2_mul<true> with n^-1 (what msm_bn254_g1_scale_device / msm_bn254_g2_scale_device launch), which also gives the requested output form;
// log_n == 0 is that pass alone with the scalar 1.

static_assert(sizeof(msm_g1_fft_plan_t) == sizeof(gfk::GfPlan) && sizeof(gfk::GfPlan) == 16, "g1_fft_bn254.hpp mirrors the header's struct");
static_assert(sizeof(msm_g2_fft_plan_t) == sizeof(gfk::Gf2Plan) && sizeof(gfk::Gf2Plan) == 16, "g2_fft_bn254.hpp mirrors the header's struct");
static_assert(MSM_NTT_INVERSE == gfk::GF_F_INVERSE && MSM_FB_OUT_STD == gfk::GF_F_OUT_STD && MSM_PM_BASES_STD == gfk::GF_F_IN_STD,
              "g1_fft_bn254.hpp mirrors the header's constants");
static_assert(gfk::GF_MAX_LOG2 == nttk::NTT_MAX_LOG2, "the group transform has the scalar transform's domain");

struct GroupFftState {
    struct Table {
        uint32_t log_n;
        DevBuf buf;
        hipEvent_t built;       // behind the build
        hipStream_t built_on;
    };
    std::vector<Table> tw;
    DevBuf io_xy, io_inf;  // the staging arrays of the host-pointer call
};

namespace {

constexpr size_t GF_LAUNCH_MAX = (size_t)1 << 30;  // lanes per launch

// A group's side of the call: words per affine record (the element-wise call's), the kernels, the names of the ranges
template <class G>
struct GroupFftSide;
template <>
struct GroupFftSide<HostG1> {
    static constexpr size_t WORDS = PointwiseSide<HostG1>::WORDS;
    static constexpr const char* RANGE_DEVICE = "msm_bn254_g1_fft_device";
    static constexpr const char* RANGE_HOST = "msm_bn254_g1_fft";
    static constexpr auto KERNEL_BITREV = gfk::k_gf_bitrev;
    static constexpr auto KERNEL_FIRST = gfk::k_gf_stage<false>, KERNEL_LADDER = gfk::k_gf_stage<true>;  // the first stage (every twiddle 1) / the others
};
template <>
struct GroupFftSide<HostG2> {
    static constexpr size_t WORDS = PointwiseSide<HostG2>::WORDS;
    static constexpr const char* RANGE_DEVICE = "msm_bn254_g2_fft_device";
    static constexpr const char* RANGE_HOST = "msm_bn254_g2_fft";
    static constexpr auto KERNEL_BITREV = gfk::k_gf2_bitrev;
    static constexpr auto KERNEL_FIRST = gfk::k_gf2_stage<false>, KERNEL_LADDER = gfk::k_gf2_stage<true>;
};

void group_fft_release(msm_ctx* c) {
    GroupFftState* s = c->group_fft;
    if (!s) return;
    for (auto& t : s->tw) {
        release(t.buf);
        if (t.built) (void)hipEventDestroy(t.built);
    }
    release(s->io_xy);
    release(s->io_inf);
    delete s;
    c->group_fft = nullptr;
}

int32_t group_fft_check(msm_ctx* c, const void* xy, const void* out_inf, uint32_t log_n, size_t batch, uint32_t flags, uint32_t allowed) {
    if (!xy || !out_inf) return fail(c, MSM_ERR_BAD_ARG, "NULL point or flag pointer");
    if (log_n > gfk::GF_MAX_LOG2) return fail(c, MSM_ERR_BAD_ARG, "log_n = %u: r - 1 has 28 factors of two", log_n);
    if (flags & ~allowed)
        return fail(c, MSM_ERR_BAD_ARG, "flags = 0x%x: only 0x%x is taken here (MSM_NTT_INVERSE = 1, MSM_FB_OUT_STD = 8, MSM_PM_BASES_STD = 16)", flags, allowed);
    if (batch == 0) return fail(c, MSM_ERR_EMPTY, "Empty input");
    if (batch > (((size_t)1 << 36) >> log_n)) return fail(c, MSM_ERR_BAD_ARG, "batch x n = %zu x 2^%u exceeds 2^36 points", batch, log_n);
    return MSM_OK;
}

// the table of log_n >= 2, built on st if this is its first use; st waits for a build on another stream
int32_t group_fft_table(msm_ctx* c, uint32_t log_n, hipStream_t st, const uint32_t** out) {
    using namespace frvk;
    if (!c->group_fft) {
        c->group_fft = new (std::nothrow) GroupFftState();
        if (!c->group_fft) return fail(c, MSM_ERR_OOM, "out of host memory");
    }
    GroupFftState* s = c->group_fft;
    for (auto& t : s->tw)
        if (t.log_n == log_n) {
            if (t.built_on != st) HIPCHK(c, hipStreamWaitEvent(st, t.built, 0));
            *out = (const uint32_t*)t.buf.p;
            return MSM_OK;
        }
    GroupFftState::Table nt{log_n, {}, nullptr, st};
    const size_t entries = (size_t)gfk::gf_table_entries(log_n);
    int32_t rc = ensure(c, nt.buf, entries * 32);
    if (rc) return rc;
    hipError_t e = hipEventCreateWithFlags(&nt.built, hipEventDisableTiming);
    if (e != hipSuccess) {
        release(nt.buf);
        return fail(c, MSM_ERR_HIP, "hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
    }
    const FrvPowers a = frv_powers_args(nttk::ntt_root(log_n), fr_one(), 0, 0);  // standard form out
    k_frv_powers<<<grid1(frv_powers_lanes(entries), FRV_BLOCK), FRV_BLOCK, 0, st>>>(a, (uint32_t*)nt.buf.p, entries);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(nt.built, st);
    if (e != hipSuccess) {
        release(nt.buf);
        (void)hipEventDestroy(nt.built);
        return fail(c, MSM_ERR_HIP, "building the twiddle table failed: %s", hipGetErrorString(e));
    }
    s->tw.push_back(nt);
    *out = (const uint32_t*)nt.buf.p;
    return MSM_OK;
}

// the whole transform on st; the context's mutex is held, the arguments are checked
template <class G>
int32_t group_fft_enqueue(msm_ctx* c, uint32_t* d_xy, uint8_t* d_inf, uint32_t k, size_t batch, uint32_t flags, hipStream_t st) {
    using namespace gfk;
    using GF = GroupFftSide<G>;
    const bool inverse = flags & MSM_NTT_INVERSE;
    const size_t points = batch << k;
    if (k == 0) {  // the form and the flag only: one pass with the scalar 1
        const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
        const PmSplit uni = pm_split_host(one);
        return pointwise_enqueue<G>(c, d_xy, d_inf, nullptr, &uni, points, flags & (MSM_PM_BASES_STD | MSM_FB_OUT_STD), d_xy, d_inf, st);
    }
    const uint32_t* tw = nullptr;
    int32_t rc;
    if (k >= 2 && (rc = group_fft_table(c, k, st, &tw))) return rc;  // (the only step that can fail: nothing is written before it)
    for (size_t at = 0; at < points; at += GF_LAUNCH_MAX) {
        const size_t cnt = points - at < GF_LAUNCH_MAX ? points - at : GF_LAUNCH_MAX;
        GF::KERNEL_BITREV<<<grid1(cnt, FB_GROUP), FB_GROUP, 0, st>>>(d_xy, d_inf, k, (uint64_t)at, (uint32_t)cnt);
    }
    const size_t items = points >> 1;
    for (uint32_t s = 1; s <= k; s++) {
        GfStage stg{k, s, inverse ? GF_F_INVERSE : 0u};
        if (s == 1) stg.flags |= flags & MSM_PM_BASES_STD;
        if (s == k && !inverse) stg.flags |= flags & MSM_FB_OUT_STD;  // (the inverse's last pass is the scaling below)
        const auto kernel = s == 1 ? GF::KERNEL_FIRST : GF::KERNEL_LADDER;
        for (size_t at = 0; at < items; at += GF_LAUNCH_MAX) {
            const size_t cnt = items - at < GF_LAUNCH_MAX ? items - at : GF_LAUNCH_MAX;
            kernel<<<grid1(cnt, FB_GROUP), FB_GROUP, 0, st>>>(d_xy, d_inf, tw, stg, (uint64_t)at, (uint32_t)cnt);
        }
    }
    HIPCHK(c, hipGetLastError());
    if (!inverse) return MSM_OK;
    uint32_t n_std[8] = {1u << k, 0, 0, 0, 0, 0, 0, 0}, ninv_std[8];
    nttk::fr_to_std(ninv_std, nttk::fr_inv(nttk::fr_from_std(n_std)));
    const PmSplit uni = pm_split_host(ninv_std);
    return pointwise_enqueue<G>(c, d_xy, d_inf, nullptr, &uni, points, flags & MSM_FB_OUT_STD, d_xy, d_inf, st);
}

int32_t group_fft_plan(uint32_t log_n, void* out) {
    if (!out) return fail(nullptr, MSM_ERR_BAD_ARG, "NULL out pointer");
    if (log_n > gfk::GF_MAX_LOG2) return fail(nullptr, MSM_ERR_BAD_ARG, "log_n = %u: r - 1 has 28 factors of two", log_n);
    const gfk::GfPlan p = gfk::gf_plan(log_n);
    memcpy(out, &p, sizeof p);
    return MSM_OK;
}

template <class G>
int32_t group_fft_device(msm_ctx* c, void* d_xy, void* d_inf, uint32_t log_n, size_t batch, uint32_t flags, void* hip_stream) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int32_t rc = group_fft_check(c, d_xy, d_inf, log_n, batch, flags, MSM_NTT_INVERSE | MSM_FB_OUT_STD | MSM_PM_BASES_STD);
    if (rc) return rc;
    if (((uintptr_t)d_xy | (uintptr_t)d_inf) & 15u) return fail(c, MSM_ERR_BAD_ARG, "the arrays must be 16-byte aligned");
    DeviceGuard g(c->device);
    Range r_(GroupFftSide<G>::RANGE_DEVICE);
    return group_fft_enqueue<G>(c, (uint32_t*)d_xy, (uint8_t*)d_inf, log_n, batch, flags, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

template <class G>
int32_t group_fft_host(msm_ctx* c, const uint32_t* xy, uint32_t base_form, const uint8_t* inf, uint32_t log_n, size_t batch, uint32_t flags,
                       uint32_t* out_xy, uint8_t* out_inf) {
    constexpr size_t BYTES = GroupFftSide<G>::WORDS * 4;
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!out_xy) return fail(c, MSM_ERR_BAD_ARG, "NULL output pointer");
    if (base_form != MSM_FORM_STD && base_form != MSM_FORM_MONT) return fail(c, MSM_ERR_BAD_ARG, "base_form = %u: MSM_FORM_STD or MSM_FORM_MONT", base_form);
    int32_t rc = group_fft_check(c, xy, out_inf, log_n, batch, flags, MSM_NTT_INVERSE | MSM_FB_OUT_STD);
    if (rc) return rc;
    DeviceGuard g(c->device);
    Range r_(GroupFftSide<G>::RANGE_HOST);
    if (!c->group_fft) {
        c->group_fft = new (std::nothrow) GroupFftState();
        if (!c->group_fft) return fail(c, MSM_ERR_OOM, "out of host memory");
    }
    GroupFftState* s = c->group_fft;
    const size_t points = batch << log_n;
    if ((rc = ensure(c, s->io_xy, points * BYTES))) return rc;
    if ((rc = ensure(c, s->io_inf, points))) return rc;
    HostPin pin_i, pin_o;
    if (!c->no_host_pin) {
        pin_i.pin(xy, points * BYTES);
        if (out_xy != xy) pin_o.pin(out_xy, points * BYTES);
    }
    if ((rc = h2d(c, s->io_xy.p, xy, points * BYTES, c->stream))) return rc;
    if (inf) {
        if ((rc = h2d(c, s->io_inf.p, inf, points, c->stream))) return rc;
    } else {
        HIPCHK(c, hipMemsetAsync(s->io_inf.p, 0, points, c->stream));
    }
    const uint32_t kflags = flags | (base_form == MSM_FORM_STD ? MSM_PM_BASES_STD : 0u);
    if ((rc = group_fft_enqueue<G>(c, (uint32_t*)s->io_xy.p, (uint8_t*)s->io_inf.p, log_n, batch, kflags, c->stream))) return rc;
    HIPCHK(c, hipMemcpyAsync(out_xy, s->io_xy.p, points * BYTES, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_inf, s->io_inf.p, points, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MSM_OK;
}

}  // namespace

extern "C" {

int32_t msm_bn254_g1_fft_plan(uint32_t log_n, msm_g1_fft_plan_t* out) { return group_fft_plan(log_n, out); }
int32_t msm_bn254_g2_fft_plan(uint32_t log_n, msm_g2_fft_plan_t* out) { return group_fft_plan(log_n, out); }

int32_t msm_bn254_g1_fft_device(msm_ctx* c, void* d_xy, void* d_inf, uint32_t log_n, size_t batch, uint32_t flags, void* hip_stream) {
    return group_fft_device<HostG1>(c, d_xy, d_inf, log_n, batch, flags, hip_stream);
}
int32_t msm_bn254_g2_fft_device(msm_ctx* c, void* d_xy, void* d_inf, uint32_t log_n, size_t batch, uint32_t flags, void* hip_stream) {
    return group_fft_device<HostG2>(c, d_xy, d_inf, log_n, batch, flags, hip_stream);
}

int32_t msm_bn254_g1_fft(msm_ctx* c, const uint32_t* xy, uint32_t base_form, const uint8_t* inf, uint32_t log_n, size_t batch, uint32_t flags,
                         uint32_t* out_xy, uint8_t* out_inf) {
    return group_fft_host<HostG1>(c, xy, base_form, inf, log_n, batch, flags, out_xy, out_inf);
}
int32_t msm_bn254_g2_fft(msm_ctx* c, const uint32_t* xy, uint32_t base_form, const uint8_t* inf, uint32_t log_n, size_t batch, uint32_t flags,
                         uint32_t* out_xy, uint8_t* out_inf) {
    return group_fft_host<HostG2>(c, xy, base_form, inf, log_n, batch, flags, out_xy, out_inf);
}

}  // extern "C"
