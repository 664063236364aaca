// msm_r1cs.inc -- the R1CS rows behind the C ABI: msm_bn254_fr_r1cs_plan (host only), msm_bn254_fr_r1cs_upload, msm_bn254_fr_r1cs_info,
// msm_bn254_fr_r1cs_eval_device, msm_bn254_fr_r1cs_eval.  Included by msm_hip.hip after msm_ntt.inc; the plan, the per-item and fold routines and
// the kernels are r1cs_bn254.hpp.
//
// Per context (msm_ctx::r1cs, made by the first upload): the resident form of up to three matrices (items, group bases, entries, dictionary, fold
// rows), the scratch array of partial sums and the staging arrays of the host-pointer call.  The eval only ENQUEUES; the partial sums are shared
// by all streams a context is used with, so every eval leaves an event behind and an eval on ANOTHER stream waits for it first.

static_assert(sizeof(msm_r1cs_coef_t) == sizeof(r1csk::R1csCoef) && sizeof(msm_r1cs_info_t) == sizeof(r1csk::R1csInfo), "r1cs_bn254.hpp mirrors the header's structs");
static_assert(MSM_R1CS_COEF_MONT2 == r1csk::R1CS_COEF_MONT2 && MSM_R1CS_C_FROM_AB == r1csk::R1CS_F_C_FROM_AB, "r1cs_bn254.hpp mirrors the header's constants");

struct R1csState {
    DevBuf items, group_base, entries, dict, folds, partials, io_w, io_out;
    uint32_t n_items = 0, items01 = 0, n_folds = 0, folds01 = 0;
    uint32_t num_rows = 0, num_cols = 0, log_n = 0;
    bool has[3] = {false, false, false};
    bool resident = false;
    r1csk::R1csInfo info{};
    hipEvent_t ev = nullptr;  // behind the latest eval
    hipStream_t last_stream = nullptr;
    bool used = false;
};

namespace {

void r1cs_release(msm_ctx* c) {
    R1csState* s = c->r1cs;
    if (!s) return;
    for (DevBuf* b : {&s->items, &s->group_base, &s->entries, &s->dict, &s->folds, &s->partials, &s->io_w, &s->io_out}) release(*b);
    if (s->ev) (void)hipEventDestroy(s->ev);
    delete s;
    c->r1cs = nullptr;
}

int32_t r1cs_status(msm_ctx* c, int rc, const std::string& err) {
    return rc == 0 ? MSM_OK : fail(c, rc == -1 ? MSM_ERR_EMPTY : MSM_ERR_BAD_ARG, "%s", err.c_str());
}

// a || b || c on st; the context's mutex is held
int32_t r1cs_enqueue(msm_ctx* c, const uint32_t* d_wit, uint32_t* d_out, uint32_t flags, hipStream_t st) {
    using namespace r1csk;
    R1csState* s = c->r1cs;
    const size_t n = (size_t)1 << s->log_n;
    const bool from_ab = flags & MSM_R1CS_C_FROM_AB;
    if (s->used && s->last_stream != st) HIPCHK(c, hipStreamWaitEvent(st, s->ev, 0));
    // rows no item writes: a matrix without entries, and the rows from num_rows up to the domain's size
    for (uint32_t m = 0; m < (from_ab ? 2u : 3u); m++) {
        const size_t first = s->has[m] ? s->num_rows : 0;
        if (first < n) HIPCHK(c, hipMemsetAsync(d_out + (m * n + first) * 8, 0, (n - first) * 32, st));
    }
    const R1csView v{(const uint2*)s->items.p, (const uint32_t*)s->group_base.p, (const uint2*)s->entries.p, (const uint32_t*)s->dict.p, (const uint4*)s->folds.p};
    const fr post = r1cs_post(flags);
    const uint32_t n_items = from_ab ? s->items01 : s->n_items, n_folds = from_ab ? s->folds01 : s->n_folds;
    if (n_items) k_r1cs_items<<<grid1(n_items, 256), 256, 0, st>>>(v, n_items, d_wit, post, d_out, (uint32_t*)s->partials.p);
    if (n_folds) k_r1cs_fold<<<dim3(n_folds), R1CS_GROUP, 0, st>>>(v, (const uint32_t*)s->partials.p, post, d_out);
    if (from_ab) {
        // c = a * b in the form of the output words: the constants msm_bn254_fr_mul_sub_scale_device takes for (in, out) = (that form, that form)
        const uint32_t form = flags & MSM_NTT_OUT_MONT ? (MSM_NTT_IN_MONT | MSM_NTT_OUT_MONT) : 0u;
        k_fr_mul_sub_scale<<<grid1(n, 256), 256, 0, st>>>(d_out, d_out + n * 8, nullptr, ntt_factor_in(form), fr_canonical(fr_one()), d_out + 2 * n * 8, n);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(s->ev, st));
    s->used = true;
    s->last_stream = st;
    return MSM_OK;
}

int32_t r1cs_check_eval(msm_ctx* c, const void* wit, size_t n_witness, const void* out, uint32_t flags) {
    if (flags & ~(MSM_NTT_IN_MONT | MSM_NTT_OUT_MONT | MSM_R1CS_C_FROM_AB))
        return fail(c, MSM_ERR_BAD_ARG, "flags = 0x%x: MSM_NTT_IN_MONT, MSM_NTT_OUT_MONT and / or MSM_R1CS_C_FROM_AB", flags);
    if (!wit || !out) return fail(c, MSM_ERR_BAD_ARG, "NULL witness or output pointer");
    if (!c->r1cs || !c->r1cs->resident) return fail(c, MSM_ERR_STATE, "no constraint matrices uploaded (msm_bn254_fr_r1cs_upload)");
    if (n_witness != c->r1cs->num_cols) return fail(c, MSM_ERR_BAD_ARG, "n_witness = %zu, the matrices have %u columns", n_witness, c->r1cs->num_cols);
    return MSM_OK;
}

}  // namespace

extern "C" {

int32_t msm_bn254_fr_r1cs_plan(const msm_r1cs_coef_t* coefs, size_t n_coefs, uint32_t num_rows, uint32_t num_cols, uint32_t log_n,
                               msm_r1cs_info_t* out) {
    if (!out) return fail(nullptr, MSM_ERR_BAD_ARG, "NULL out pointer");
    r1csk::R1csHost h;
    std::string err;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = r1csk::r1cs_build((const r1csk::R1csCoef*)coefs, n_coefs, MSM_R1CS_COEF_STD, num_rows, num_cols, log_n, false, h, err);
    if (rc) return r1cs_status(nullptr, rc, err);
    h.info.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    memcpy(out, &h.info, sizeof h.info);
    return MSM_OK;
}

int32_t msm_bn254_fr_r1cs_upload(msm_ctx* c, const msm_r1cs_coef_t* coefs, size_t n_coefs, uint32_t coef_form, uint32_t num_rows,
                                 uint32_t num_cols, uint32_t log_n) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_r1cs_upload");
    const auto t0 = std::chrono::steady_clock::now();
    r1csk::R1csHost h;
    std::string err;
    int32_t rc = r1cs_status(c, r1csk::r1cs_build((const r1csk::R1csCoef*)coefs, n_coefs, coef_form, num_rows, num_cols, log_n, true, h, err), err);
    if (rc) return rc;  // (an earlier upload stays as it was)
    h.info.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (!c->r1cs) {
        R1csState* s = new (std::nothrow) R1csState();
        if (!s) return fail(c, MSM_ERR_OOM, "out of host memory");
        hipError_t e = hipEventCreateWithFlags(&s->ev, hipEventDisableTiming);
        if (e != hipSuccess) {
            delete s;
            return fail(c, MSM_ERR_HIP, "hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
        }
        c->r1cs = s;
    }
    R1csState* s = c->r1cs;
    if (s->used) HIPCHK(c, hipEventSynchronize(s->ev));  // an eval on any stream may still read what is replaced
    s->resident = false;
    struct Part {
        DevBuf* buf;
        const void* src;
        size_t bytes;
    } parts[] = {{&s->items, h.items.data(), h.items.size() * 8},          {&s->group_base, h.group_base.data(), h.group_base.size() * 4},
                 {&s->entries, h.entries.data(), h.entries.size() * 8},    {&s->dict, h.dict.data(), h.dict.size() * 4},
                 {&s->folds, h.folds.data(), h.folds.size() * 16},         {&s->partials, nullptr, (size_t)h.info.partial_sums * 32}};
    for (const Part& p : parts) {
        if (!p.bytes) continue;
        if ((rc = ensure(c, *p.buf, p.bytes))) return rc;
        if (p.src) HIPCHK(c, hipMemcpyAsync(p.buf->p, p.src, p.bytes, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s->n_items = (uint32_t)h.items.size(), s->items01 = h.items01, s->n_folds = (uint32_t)h.folds.size(), s->folds01 = h.folds01;
    s->num_rows = num_rows, s->num_cols = num_cols, s->log_n = log_n;
    for (int m = 0; m < 3; m++) s->has[m] = h.info.entries[m] != 0;
    h.info.upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    s->info = h.info;
    s->used = false;
    s->resident = true;
    return MSM_OK;
}

int32_t msm_bn254_fr_r1cs_info(msm_ctx* c, msm_r1cs_info_t* out) {
    if (!c) return MSM_ERR_BAD_ARG;
    if (!out) return fail(c, MSM_ERR_BAD_ARG, "NULL out pointer");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->r1cs || !c->r1cs->resident) return fail(c, MSM_ERR_STATE, "no constraint matrices uploaded (msm_bn254_fr_r1cs_upload)");
    memcpy(out, &c->r1cs->info, sizeof c->r1cs->info);
    return MSM_OK;
}

int32_t msm_bn254_fr_r1cs_eval_device(msm_ctx* c, const void* d_witness, size_t n_witness, void* d_out, uint32_t flags, void* hip_stream) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int32_t rc = r1cs_check_eval(c, d_witness, n_witness, d_out, flags);
    if (rc) return rc;
    if (((uintptr_t)d_witness | (uintptr_t)d_out) & 15u) return fail(c, MSM_ERR_BAD_ARG, "the arrays must be 16-byte aligned");
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_r1cs_eval_device");
    return r1cs_enqueue(c, (const uint32_t*)d_witness, (uint32_t*)d_out, flags, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int32_t msm_bn254_fr_r1cs_eval(msm_ctx* c, const uint32_t* witness, size_t n_witness, uint32_t* out, uint32_t flags) {
    if (!c) return MSM_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int32_t rc = r1cs_check_eval(c, witness, n_witness, out, flags);
    if (rc) return rc;
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_r1cs_eval");
    R1csState* s = c->r1cs;
    const size_t wb = n_witness * 32, ob = ((size_t)96) << s->log_n;
    HostPin pin_w, pin_o;
    if (!c->no_host_pin) {
        pin_w.pin(witness, wb);
        pin_o.pin(out, ob);
    }
    if ((rc = ensure(c, s->io_w, wb))) return rc;
    if ((rc = ensure(c, s->io_out, ob))) return rc;
    if ((rc = h2d(c, s->io_w.p, witness, wb, c->stream))) return rc;
    if ((rc = r1cs_enqueue(c, (const uint32_t*)s->io_w.p, (uint32_t*)s->io_out.p, flags, c->stream))) return rc;
    HIPCHK(c, hipMemcpyAsync(out, s->io_out.p, ob, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MSM_OK;
}

}  // extern "C"
