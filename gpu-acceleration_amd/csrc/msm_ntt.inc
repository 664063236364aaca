// msm_ntt.inc -- the BN254 scalar-field transforms behind the C ABI: msm_bn254_fr_root_of_unity, msm_bn254_fr_ntt_plan (host only),
// msm_bn254_fr_ntt_device, msm_bn254_fr_ntt, msm_bn254_fr_mul_sub_scale_device.  Included by msm_hip.hip after msm_g2_points.inc; the
// arithmetic is fr_bn254.hpp, the plan, the pass phases and the kernels are ntt_bn254.hpp.
//
// Per context (msm_ctx::ntt, made on first use): the butterfly table of either direction (2 x 512 entries), one two-level twiddle table per
// (size, direction) that needed more than one pass (2^ceil(k/2) + 2^floor(k/2) entries: 64 KiB at 2^20), the scratch array of multi-pass
// transforms, and one two-level table of coset powers per direction, rebuilt on the call's stream when the generator, the size or the form changes.  All of them are built on the
// device (k_ntt_pow_table).  The calls only ENQUEUE: the scratch array and the tables are shared by all streams a context is used with, so
// every call leaves an event behind and a call on ANOTHER stream waits for it first.

struct NttState {
    DevBuf wt[2];  // butterfly tables: forward, inverse
    struct Twiddle {
        uint32_t key;  // k << 1 | inverse
        DevBuf buf;    // lo entries, then hi entries
    };
    std::vector<Twiddle> tw;
    DevBuf scratch, io;  // io: the staging array of the host-pointer call
    struct Coset {       // one table per direction: the recipes alternate a forward and an inverse coset transform of one generator
        DevBuf buf;
        uint32_t key = ~0u;  // (k << 3 | flags) the table was built for, and its generator
        uint32_t g[8] = {};
    } coset[2];
    hipEvent_t ev = nullptr;    // behind the latest call
    hipStream_t last_stream = nullptr;
    bool used = false;
    uint32_t forced_tile = 0;   // hooks: msm_test_ntt_set_tile_log2
};

namespace {

void ntt_release(msm_ctx* c) {
    NttState* s = c->ntt;
    if (!s) return;
    release(s->wt[0]);
    release(s->wt[1]);
    for (auto& t : s->tw) release(t.buf);
    release(s->scratch);
    release(s->coset[0].buf);
    release(s->coset[1].buf);
    release(s->io);
    if (s->ev) (void)hipEventDestroy(s->ev);
    delete s;
    c->ntt = nullptr;
}

int32_t ntt_state(msm_ctx* c) {
    if (c->ntt) return MSM_OK;
    NttState* s = new (std::nothrow) NttState();
    if (!s) return fail(c, MSM_ERR_OOM, "out of host memory");
    hipError_t e = hipEventCreateWithFlags(&s->ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        delete s;
        return fail(c, MSM_ERR_HIP, "hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
    }
    c->ntt = s;
    return MSM_OK;
}

// count entries scale * base^e at d_out, on st
void ntt_pow_table(const nttk::fr& base, const nttk::fr& scale, uint32_t count, uint32_t* d_out, hipStream_t st) {
    nttk::k_ntt_pow_table<<<grid1(count, 256), 256, 0, st>>>(base, scale, count, d_out);
}
// two-level table of base over k-bit exponents: 2^h entries scale * base^e, then 2^(k-h) entries base^(e << h)
int32_t ntt_two_level(msm_ctx* c, DevBuf& buf, const nttk::fr& base, const nttk::fr& scale, uint32_t k, hipStream_t st) {
    const uint32_t h = nttk::ntt_split(k), nlo = 1u << h, nhi = 1u << (k - h);
    int32_t rc = ensure(c, buf, ((size_t)nlo + nhi) * 32);
    if (rc) return rc;
    nttk::fr bh = base;
    for (uint32_t i = 0; i < h; i++) bh = nttk::fr_mul(bh, bh);  // base < 2r (a root, a coset generator or the inverse of one): every square < 2r
    ntt_pow_table(base, scale, nlo, (uint32_t*)buf.p, st);
    ntt_pow_table(bh, nttk::fr_one(), nhi, (uint32_t*)buf.p + (size_t)nlo * 8, st);
    HIPCHK(c, hipGetLastError());
    return MSM_OK;
}

uint32_t ntt_tile_log2(const msm_ctx* c) { return c->ntt && c->ntt->forced_tile ? c->ntt->forced_tile : nttk::NTT_TILE_LOG2; }

int32_t ntt_check_args(msm_ctx* c, const void* data, uint32_t log_n, size_t batch, uint32_t flags) {
    if (!c) return MSM_ERR_BAD_ARG;
    if (log_n > nttk::NTT_MAX_LOG2) return fail(c, MSM_ERR_BAD_ARG, "log_n = %u: r - 1 has 28 factors of two", log_n);
    if (flags & ~(MSM_NTT_INVERSE | MSM_NTT_IN_MONT | MSM_NTT_OUT_MONT)) return fail(c, MSM_ERR_BAD_ARG, "unknown bits in flags = 0x%x", flags);
    if (!data) return fail(c, MSM_ERR_BAD_ARG, "NULL data pointer");
    if (batch == 0) return fail(c, MSM_ERR_EMPTY, "Empty input");
    if (batch > (((size_t)1 << 36) >> log_n)) return fail(c, MSM_ERR_BAD_ARG, "batch x n = %zu x 2^%u exceeds 2^36 elements", batch, log_n);
    return MSM_OK;
}

// the whole transform on st; the context's mutex is held
int32_t ntt_enqueue(msm_ctx* c, uint32_t* d_data, uint32_t k, size_t batch, uint32_t flags, const uint32_t* g_std, hipStream_t st) {
    using namespace nttk;
    int32_t rc;
    if ((uintptr_t)d_data & 15u) return fail(c, MSM_ERR_BAD_ARG, "the array must be 16-byte aligned");
    fr g{};
    if (g_std) {
        g = fr_from_std(g_std);
        if (fr_is_zero_exact(fr_canonical(g))) return fail(c, MSM_ERR_BAD_ARG, "the coset generator is 0 modulo r");
    }
    if ((rc = ntt_state(c))) return rc;
    NttState* s = c->ntt;
    const bool inverse = flags & MSM_NTT_INVERSE;
    const uint32_t T = ntt_tile_log2(c);
    NttPass ps[NTT_MAX_PASSES];
    const uint32_t P = ntt_make_passes(k, T, batch, flags, g_std != nullptr, ps);
    for (uint32_t p = 0; p < P; p++)
        if (ntt_groups(ps[p], T) > 0x7FFFFFFFull) return fail(c, MSM_ERR_BAD_ARG, "batch x n too large for this tile size");
    const size_t bytes = (batch << k) * 32;
    if (P > 1 && (rc = ensure(c, s->scratch, bytes))) return rc;
    if (s->used && s->last_stream != st) HIPCHK(c, hipStreamWaitEvent(st, s->ev, 0));
    NttTables tb{};
    if (k >= 2) {  // (a transform of one or two points has levels 0 only: no table)
        DevBuf& wt = s->wt[inverse ? 1 : 0];
        if (!wt.p) {
            if ((rc = ensure(c, wt, (size_t)32 << (NTT_WT_LOG2 - 1)))) return rc;
            fr w = ntt_root(NTT_WT_LOG2);
            if (inverse) w = fr_inv(w);
            ntt_pow_table(w, fr_one(), 1u << (NTT_WT_LOG2 - 1), (uint32_t*)wt.p, st);
        }
        tb.wt = (const uint32_t*)wt.p;
    }
    if (P > 1) {
        const uint32_t key = k << 1 | (inverse ? 1u : 0u);
        NttState::Twiddle* t = nullptr;
        for (auto& e : s->tw)
            if (e.key == key) t = &e;
        if (!t) {
            NttState::Twiddle nt{key, {}};
            fr w = ntt_root(k);
            if (inverse) w = fr_inv(w);
            if ((rc = ntt_two_level(c, nt.buf, w, fr_one(), k, st))) {
                release(nt.buf);
                return rc;
            }
            s->tw.push_back(nt);
            t = &s->tw.back();
        }
        tb.tw_lo = (const uint32_t*)t->buf.p;
        tb.tw_hi = tb.tw_lo + ((size_t)8 << ntt_split(k));
    }
    if (g_std) {
        const uint32_t key = k << 3 | flags;
        NttState::Coset& cs = s->coset[inverse ? 1 : 0];
        if (cs.key != key || memcmp(cs.g, g_std, 32) != 0) {
            cs.key = ~0u;
            // forward: the first load multiplies by rep(2^261 g^i) (or 2^5 for Montgomery words); inverse: the last store by raw(s g^-j)
            const fr base = inverse ? fr_inv(g) : g;
            if ((rc = ntt_two_level(c, cs.buf, base, inverse ? ntt_factor_out(k, flags) : ntt_factor_in(flags), k, st))) return rc;
            cs.key = key;
            memcpy(cs.g, g_std, 32);
        }
        tb.cs_lo = (const uint32_t*)cs.buf.p;
        tb.cs_hi = tb.cs_lo + ((size_t)8 << ntt_split(k));
    }
    uint32_t* scratch = (uint32_t*)s->scratch.p;
    for (uint32_t p = 0; p < P; p++) {
        const uint32_t* src = p == 0 ? d_data : scratch;
        uint32_t* dst = p + 1 == P ? d_data : scratch;
        const uint64_t groups = ntt_groups(ps[p], T);
        if (T == NTT_TILE_LOG2) k_ntt_pass<NTT_TILE_LOG2><<<dim3((unsigned)groups), 1u << (NTT_TILE_LOG2 - 1), 0, st>>>(ps[p], tb, src, dst);
        else k_ntt_pass<NTT_TILE_SMALL_LOG2><<<dim3((unsigned)groups), 1u << (NTT_TILE_SMALL_LOG2 - 1), 0, st>>>(ps[p], tb, src, dst);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(s->ev, st));
    s->used = true;
    s->last_stream = st;
    return MSM_OK;
}

}  // namespace

extern "C" {

int32_t msm_bn254_fr_root_of_unity(uint32_t log_n, uint32_t out_std[8]) {
    if (log_n > nttk::NTT_MAX_LOG2 || !out_std) return MSM_ERR_BAD_ARG;
    nttk::fr_to_std(out_std, nttk::ntt_root(log_n));
    return MSM_OK;
}

int32_t msm_bn254_fr_ntt_plan(uint32_t log_n, uint32_t* passes, uint32_t radix_log2[8]) {
    if (log_n > nttk::NTT_MAX_LOG2 || !passes || !radix_log2) return MSM_ERR_BAD_ARG;
    const nttk::NttPlan pl = nttk::ntt_make_plan(log_n, nttk::NTT_TILE_LOG2);
    *passes = pl.passes;
    for (uint32_t i = 0; i < 8; i++) radix_log2[i] = pl.radix[i];
    return MSM_OK;
}

int32_t msm_bn254_fr_ntt_device(msm_ctx* c, void* d_data, uint32_t log_n, size_t batch, uint32_t flags, const uint32_t* coset_gen_std,
                                void* hip_stream) {
    int32_t rc = ntt_check_args(c, d_data, log_n, batch, flags);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_ntt_device");
    return ntt_enqueue(c, (uint32_t*)d_data, log_n, batch, flags, coset_gen_std, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

int32_t msm_bn254_fr_ntt(msm_ctx* c, const uint32_t* in, uint32_t* out, uint32_t log_n, size_t batch, uint32_t flags,
                         const uint32_t* coset_gen_std) {
    int32_t rc = ntt_check_args(c, in, log_n, batch, flags);
    if (rc) return rc;
    if (!out) return fail(c, MSM_ERR_BAD_ARG, "NULL out pointer");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_ntt");
    const size_t bytes = (batch << log_n) * 32;
    HostPin pin_i, pin_o;
    if (!c->no_host_pin) {
        pin_i.pin(in, bytes);
        if (out != in) pin_o.pin(out, bytes);
    }
    if ((rc = ntt_state(c))) return rc;
    if ((rc = ensure(c, c->ntt->io, bytes))) return rc;
    if ((rc = h2d(c, c->ntt->io.p, in, bytes, c->stream))) return rc;
    if ((rc = ntt_enqueue(c, (uint32_t*)c->ntt->io.p, log_n, batch, flags, coset_gen_std, c->stream))) return rc;
    HIPCHK(c, hipMemcpyAsync(out, c->ntt->io.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MSM_OK;
}

int32_t msm_bn254_fr_mul_sub_scale_device(msm_ctx* c, const void* d_a, const void* d_b, const void* d_c, const uint32_t* k_std, void* d_out,
                                          size_t n, uint32_t flags, void* hip_stream) {
    using namespace nttk;
    if (!c) return MSM_ERR_BAD_ARG;
    if (flags & ~(MSM_NTT_IN_MONT | MSM_NTT_OUT_MONT)) return fail(c, MSM_ERR_BAD_ARG, "flags = 0x%x: MSM_NTT_IN_MONT and / or MSM_NTT_OUT_MONT", flags);
    if (!d_a || !d_b || !d_out) return fail(c, MSM_ERR_BAD_ARG, "NULL operand pointer");
    if (n == 0) return fail(c, MSM_ERR_EMPTY, "Empty input");
    if (((uintptr_t)d_a | (uintptr_t)d_b | (uintptr_t)d_c | (uintptr_t)d_out) & 15u) return fail(c, MSM_ERR_BAD_ARG, "the arrays must be 16-byte aligned");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    Range r_("msm_bn254_fr_mul_sub_scale_device");
    // a as raw limbs times pre, times b as raw limbs, is (a*b) in the form of the INPUT words (so that c subtracts as it is); post carries k and
    // the change of form: rep(k * 2^(256 * (out_mont - in_mont)))
    const bool im = flags & MSM_NTT_IN_MONT, om = flags & MSM_NTT_OUT_MONT;
    const fr pre = ntt_factor_in(flags);
    fr post = k_std ? fr_from_std(k_std) : fr_one();
    if (om && !im) post = fr_mul(post, ntt_consts().p256);  // post < 2r (fr_from_std) or < r, the constant < 2r: the product < 2r
    if (im && !om) post = fr_mul(post, ntt_consts().m256);
    post = fr_canonical(post);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    k_fr_mul_sub_scale<<<grid1(n, 256), 256, 0, st>>>((const uint32_t*)d_a, (const uint32_t*)d_b, (const uint32_t*)d_c, pre, post, (uint32_t*)d_out, n);
    HIPCHK(c, hipGetLastError());
    return MSM_OK;
}

}  // extern "C"
