// msm_g2_points.inc -- getting BN254 G2 bases in safely, behind the C ABI: msm_bn254_g2_compress (host only), msm_bn254_g2_decompress(_device),
// msm_bn254_g2_validate(_device), msm_bn254_g1_validate.  Included by msm_hip.hip after msm_g2.inc; kernels in msm_kernels_g2_points.hpp.
//
// Every GPU call is one kernel, one thread per point, and ONE word back: the kernels atomicMin (index << 2 | reason) into a word behind the staged
// input, so the host learns the lowest failing index and whether the decoding, the curve or the subgroup check failed from a 4-byte copy.
// All calls block until that verdict is on the host; a failed call leaves the context as it was (no MSM state is touched).

namespace {

constexpr uint32_t G2_CHECKS_ALL = MSM_G2_CHECK_CURVE | MSM_G2_CHECK_SUBGROUP;

// wait for the verdict word the kernel in front left at d_bad; what: "compressed G2 point" / "G2 point" / "G1 point"
int32_t points_verdict(msm_ctx* c, const uint32_t* d_bad, hipStream_t st, const char* what, int64_t* first_invalid) {
    uint32_t bad = msmk::G2P_NONE;
    HIPCHK(c, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    if (bad == msmk::G2P_NONE) return MSM_OK;
    const uint32_t idx = bad >> 2, why = bad & 3u;
    if (first_invalid) *first_invalid = (int64_t)idx;
    if (why == msmk::G2P_DECODE) return fail(c, MSM_ERR_INVALID_DATA, "%s %u does not decode (both flag bits set, or a component >= p)", what, idx);
    if (why == msmk::G2P_CURVE)
        return fail(c, MSM_ERR_INVALID_DATA, "%s %u is not on the curve (a coordinate >= p, or no y with y^2 = x^3 + b exists / is given)", what, idx);
    return fail(c, MSM_ERR_INVALID_DATA, "%s %u is on the twist but outside the subgroup of order r", what, idx);
}

// images (host) -> d_out (n x 32 Montgomery words) + d_inf (n bytes) on stream st; the images are staged in the context's workspace
int32_t g2_decompress_locked(msm_ctx* c, const uint8_t* compressed, size_t n, uint32_t checks, uint32_t* d_out, uint8_t* d_inf, hipStream_t st,
                             int64_t* first_invalid) {
    int32_t rc;
    if (first_invalid) *first_invalid = -1;
    if ((rc = ensure(c, c->bases, n * 64 + 16))) return rc;
    uint32_t* d_bad = (uint32_t*)((uint8_t*)c->bases.p + n * 64);  // the verdict word, kept behind the images
    const uint32_t none = msmk::G2P_NONE;
    HIPCHK(c, hipMemcpyAsync(c->bases.p, compressed, n * 64, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_bad, &none, 4, hipMemcpyHostToDevice, st));
    if (checks & MSM_G2_CHECK_SUBGROUP)
        msmk::k_g2_decompress<true><<<grid1(n, 256), 256, 0, st>>>((const uint32_t*)c->bases.p, (uint32_t)n, d_out, d_inf, d_bad);
    else
        msmk::k_g2_decompress<false><<<grid1(n, 256), 256, 0, st>>>((const uint32_t*)c->bases.p, (uint32_t)n, d_out, d_inf, d_bad);
    return points_verdict(c, d_bad, st, "compressed G2 point", first_invalid);
}

// words: bytes per point (128: G2, 64: G1); the verdict word sits at d_bad
int32_t validate_launch(msm_ctx* c, bool g2, const uint32_t* d_pts, const uint8_t* d_inf, size_t n, uint32_t form, uint32_t checks, uint32_t* d_bad,
                        hipStream_t st, int64_t* first_invalid) {
    const uint32_t none = msmk::G2P_NONE;
    HIPCHK(c, hipMemcpyAsync(d_bad, &none, 4, hipMemcpyHostToDevice, st));
    const uint32_t mont = form == MSM_FORM_MONT ? 1u : 0u;
    if (g2)
        msmk::k_g2_validate<<<grid1(n, 256), 256, 0, st>>>(d_pts, d_inf, (uint32_t)n, mont, (checks & MSM_G2_CHECK_SUBGROUP) ? 1u : 0u, d_bad);
    else
        msmk::k_g1_validate<<<grid1(n, 256), 256, 0, st>>>(d_pts, d_inf, (uint32_t)n, mont, d_bad);
    return points_verdict(c, d_bad, st, g2 ? "G2 point" : "G1 point", first_invalid);
}

// host words -> workspace, then validate_launch
int32_t validate_host(msm_ctx* c, bool g2, const uint32_t* pts, uint32_t form, const uint8_t* inf_mask, size_t n, uint32_t checks,
                      int64_t* first_invalid) {
    int32_t rc;
    const size_t rec = g2 ? 128 : 64;
    if (first_invalid) *first_invalid = -1;
    HostPin pin_b, pin_i;  // pageable caller memory pinned in place for the copies, as msm_bn254_g2 does
    if (!c->no_host_pin) {
        pin_b.pin(pts, n * rec);
        pin_i.pin(inf_mask, n);
    }
    hipStream_t st = c->stream;
    if ((rc = ensure(c, c->bases, n * rec + 16))) return rc;
    if (inf_mask && (rc = ensure(c, c->inf, n))) return rc;
    if ((rc = h2d(c, c->bases.p, pts, n * rec, st))) return rc;
    if (inf_mask && (rc = h2d(c, c->inf.p, inf_mask, n, st))) return rc;
    return validate_launch(c, g2, (const uint32_t*)c->bases.p, inf_mask ? (const uint8_t*)c->inf.p : nullptr, n, form, checks,
                           (uint32_t*)((uint8_t*)c->bases.p + n * rec), st, first_invalid);
}

int32_t check_checks(msm_ctx* c, uint32_t checks) {
    if (checks == 0 || (checks & ~G2_CHECKS_ALL)) return fail(c, MSM_ERR_BAD_ARG, "checks = 0x%x: MSM_G2_CHECK_CURVE and / or MSM_G2_CHECK_SUBGROUP", checks);
    return MSM_OK;
}

}  // namespace

extern "C" {

// host-side inverse of the decoding (ark-serialize 0.4): x.c0 | x.c1 standard form LE; byte 63 bit 7 = y > -y (c1 first, then c0), bit 6 = infinity
int32_t msm_bn254_g2_compress(const uint32_t* bases_xy, uint32_t base_form, const uint8_t* inf_mask, size_t n, uint8_t* out) {
    if (n == 0) return MSM_ERR_EMPTY;
    if (!bases_xy || !out || (base_form != MSM_FORM_STD && base_form != MSM_FORM_MONT)) return MSM_ERR_BAD_ARG;
    auto work = [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) hostg2::compress_point(bases_xy + i * 32, base_form == MSM_FORM_MONT, inf_mask && inf_mask[i], out + i * 64);
    };
    const size_t nt = n < 8192 ? 1 : std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
    if (nt == 1) {
        work(0, n);
    } else {
        std::vector<std::thread> th;
        for (size_t t = 0; t < nt; t++) th.emplace_back(work, n * t / nt, n * (t + 1) / nt);
        for (auto& t : th) t.join();
    }
    return MSM_OK;
}

int32_t msm_bn254_g2_decompress(msm_ctx* c, const uint8_t* compressed, size_t n, uint32_t checks, uint32_t* out_xy_mont, uint8_t* out_inf,
                                int64_t* first_invalid) {
    int32_t rc = check_common(c, compressed, out_xy_mont, n);
    if (rc) return rc;
    if (!out_inf) return fail(c, MSM_ERR_BAD_ARG, "NULL out_inf");
    if (checks & ~G2_CHECKS_ALL) return fail(c, MSM_ERR_BAD_ARG, "unknown bits in checks = 0x%x", checks);
    if (n > 0x3FFFFFFFull) return fail(c, MSM_ERR_BAD_ARG, "n = %zu exceeds 2^30-1 points per context call", n);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    Range r_("msm_bn254_g2_decompress");
    HostPin pin_c, pin_o, pin_i;
    if (!c->no_host_pin) {
        pin_c.pin(compressed, n * 64);
        pin_o.pin(out_xy_mont, n * 128);
        pin_i.pin(out_inf, n);
    }
    if ((rc = ensure(c, c->ibases, n * 128))) return rc;  // scratch of the call
    if ((rc = ensure(c, c->inf, n))) return rc;
    if ((rc = g2_decompress_locked(c, compressed, n, checks, (uint32_t*)c->ibases.p, (uint8_t*)c->inf.p, c->stream, first_invalid))) return rc;
    HIPCHK(c, hipMemcpyAsync(out_xy_mont, c->ibases.p, n * 128, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_inf, c->inf.p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MSM_OK;
}

int32_t msm_bn254_g2_decompress_device(msm_ctx* c, const uint8_t* compressed, size_t n, uint32_t checks, void* d_out_xy_mont, void* d_out_inf,
                                       void* hip_stream, int64_t* first_invalid) {
    int32_t rc = check_common(c, compressed, d_out_xy_mont, n);
    if (rc) return rc;
    if (!d_out_inf) return fail(c, MSM_ERR_BAD_ARG, "NULL d_out_inf");
    if (checks & ~G2_CHECKS_ALL) return fail(c, MSM_ERR_BAD_ARG, "unknown bits in checks = 0x%x", checks);
    if (n > 0x3FFFFFFFull) return fail(c, MSM_ERR_BAD_ARG, "n = %zu exceeds 2^30-1 points per context call", n);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    Range r_("msm_bn254_g2_decompress_device");
    HostPin pin_c;
    if (!c->no_host_pin) pin_c.pin(compressed, n * 64);
    return g2_decompress_locked(c, compressed, n, checks, (uint32_t*)d_out_xy_mont, (uint8_t*)d_out_inf,
                                hip_stream ? (hipStream_t)hip_stream : c->stream, first_invalid);
}

int32_t msm_bn254_g2_validate(msm_ctx* c, const uint32_t* bases_xy, uint32_t base_form, const uint8_t* inf_mask, size_t n, uint32_t checks,
                              int64_t* first_invalid) {
    int32_t rc = check_common(c, bases_xy, bases_xy, n);
    if (rc) return rc;
    if (base_form != MSM_FORM_STD && base_form != MSM_FORM_MONT) return fail(c, MSM_ERR_BAD_ARG, "unknown base_form %u", base_form);
    if ((rc = check_checks(c, checks))) return rc;
    if (n > 0x3FFFFFFFull) return fail(c, MSM_ERR_BAD_ARG, "n = %zu exceeds 2^30-1 points per context call", n);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    Range r_("msm_bn254_g2_validate");
    return validate_host(c, true, bases_xy, base_form, inf_mask, n, checks, first_invalid);
}

int32_t msm_bn254_g2_validate_device(msm_ctx* c, const void* d_bases_mont, const void* d_inf_mask, size_t n, uint32_t checks, void* hip_stream,
                                     int64_t* first_invalid) {
    int32_t rc = check_common(c, d_bases_mont, d_bases_mont, n);
    if (rc) return rc;
    if ((rc = check_checks(c, checks))) return rc;
    if (n > 0x3FFFFFFFull) return fail(c, MSM_ERR_BAD_ARG, "n = %zu exceeds 2^30-1 points per context call", n);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    Range r_("msm_bn254_g2_validate_device");
    if (first_invalid) *first_invalid = -1;
    if ((rc = ensure(c, c->bases, 16))) return rc;  // the verdict word
    return validate_launch(c, true, (const uint32_t*)d_bases_mont, (const uint8_t*)d_inf_mask, n, MSM_FORM_MONT, checks, (uint32_t*)c->bases.p,
                           hip_stream ? (hipStream_t)hip_stream : c->stream, first_invalid);
}

int32_t msm_bn254_g1_validate(msm_ctx* c, const uint32_t* bases_xy, uint32_t base_form, const uint8_t* inf_mask, size_t n, int64_t* first_invalid) {
    int32_t rc = check_common(c, bases_xy, bases_xy, n);
    if (rc) return rc;
    if (base_form != MSM_FORM_STD && base_form != MSM_FORM_MONT) return fail(c, MSM_ERR_BAD_ARG, "unknown base_form %u", base_form);
    if (n > 0x3FFFFFFFull) return fail(c, MSM_ERR_BAD_ARG, "n = %zu exceeds 2^30-1 points per context call", n);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    Range r_("msm_bn254_g1_validate");
    return validate_host(c, false, bases_xy, base_form, inf_mask, n, MSM_G2_CHECK_CURVE, first_invalid);
}

}  // extern "C"
