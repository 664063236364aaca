// msm_g2.inc -- the BN254 G2 MSM behind the C ABI (msm_bn254_g2, msm_bn254_g2_device, msm_bn254_g2_combine).  Included by msm_hip.hip after the
// G1 entry points: it shares their context, workspace and scalar pipeline.
//
// One call = the G1 pipeline with its point side replaced (msm_kernels_g2.hpp):
//   k_g2_convert (caller words -> internal records, phi2 records of a split plan)          [new]
//   enqueue_decompose + enqueue_sort (digits, GLV split, counting sort, piece plan)        [G1's, unchanged; the piece tally runs in its "into"
//                                                                                            form so that it writes no G1 identity into the buckets]
//   k_g2_clear_empty, k_g2_accumulate, k_g2_combine                                        [new]
//   k_g2_pair_level x levels, k_g2_reduce_bits -> (word, call number) pairs in pinned memory [new]
//   finish_sync<HostG2>: wait for the pairs, Horner chain over the bit sums, outputs        [G1's, templated]
// The flag words, the call numbers (done_seq) and flags_clean are the context's, shared with G1 calls: the G2 reduction copies the flag words
// out as pairs and zeroes them exactly as k_reduce_bits does.  No window table, no resident set, no streaming, no multi-device form (follow-ups).
// Decoding compressed bases and checking them (curve, subgroup) is msm_g2_points.inc: its outputs are what msm_bn254_g2_device takes.

namespace {

constexpr size_t XB2 = msmk::XW2 * 4;  // bytes per G2 XYZZ record

// K4/K5 for G2: plain row / column sums by pairwise levels, then the per-bit sums straight into the pinned G2 result buffer
int32_t enqueue_reduce_g2(msm_ctx* c, const PipeState& ps, hipStream_t st) {
    Range r_("msm:reduce_g2");
    const size_t tb = ps.tb;
    const uint32_t W = ps.rW, kb = ps.rkb, kb_lo = ps.kb_lo, kb_hi = ps.kb_hi, n_lo = ps.n_lo, n_hi = ps.n_hi;
    uint32_t *rbuf[2], *cbuf[2];
    reduce_bufs(c, tb, msmk::XW2, rbuf, cbuf);
    const uint32_t *rin = (const uint32_t*)c->buckets.p, *cin = rin;
    size_t rn = tb, cn = tb;
    const uint32_t levels = kb_hi > kb_lo ? kb_hi : kb_lo;
    for (uint32_t l = 0; l < levels; l++) {
        msmk::pair_job ja{nullptr, nullptr, 0, 1}, jb{nullptr, nullptr, 0, 1};
        if (l < kb_lo) {
            rn /= 2;
            ja = msmk::pair_job{rin, rbuf[l & 1], (uint32_t)rn, 1};
            rin = rbuf[l & 1];
        }
        if (l < kb_hi) {
            cn /= 2;
            jb = msmk::pair_job{cin, cbuf[l & 1], (uint32_t)cn, n_lo};
            cin = cbuf[l & 1];
        }
        msmk::k_g2_pair_level<<<grid1((size_t)ja.n_out + jb.n_out, 256), 256, 0, st>>>(ja, jb);
    }
    uint32_t *q_dev = nullptr, *f_dev = nullptr;
    HIPCHK(c, hipHostGetDevicePointer((void**)&q_dev, c->h_qsums2, 0));
    HIPCHK(c, hipHostGetDevicePointer((void**)&f_dev, c->h_flags, 0));
    if (++c->done_seq == 0) c->done_seq = 1;  // (0 is what fresh pairs hold)
    msmk::k_g2_reduce_bits<<<W * (kb + 1), 64, 0, st>>>(rin, cin, q_dev, n_hi, n_lo, kb_lo, kb, (uint32_t*)c->flags.p, f_dev, c->done_seq);
    if (c->stage_timing) HIPCHK(c, hipEventRecord(c->ev[EV_REDUCE], st));
    return MSM_OK;
}

// The whole G2 pipeline on device-resident inputs: d_raw = n x 32 caller words (form), d_inf nullable, d_scalars n x 8 standard form.
int32_t run_g2(msm_ctx* c, const uint32_t* d_raw, uint32_t form, const uint8_t* d_inf, const uint32_t* d_scalars, size_t n, hipStream_t st,
               uint32_t* out_jac, uint32_t* out_aff, uint8_t* out_inf) {
    int32_t rc;
    if (!c->h_qsums2) {  // first G2 call of the context
        hipError_t e = hipHostMalloc((void**)&c->h_qsums2, MAX_QSUM_POINTS * 384, hipHostMallocDefault);  // 48 (word, seq) pairs per bit sum
        if (e != hipSuccess) {
            c->h_qsums2 = nullptr;
            return fail(c, MSM_ERR_OOM, "hipHostMalloc of the G2 result buffer failed: %s", hipGetErrorString(e));
        }
        std::memset(c->h_qsums2, 0, MAX_QSUM_POINTS * 384);
        c->qsums2.assign(MAX_QSUM_POINTS * 48, 0);
    }
    PipeState ps;
    if ((rc = pipe_prepare(c, n, 0, 0, st, &ps, 0, 1, nullptr, XB2))) return rc;
    const bool glv = ps.pl.glv != 0;
    if ((rc = ensure(c, c->ibases, (glv ? 2 * n : n) * msmk::BW2 * 4))) return rc;
    uint32_t* ib = (uint32_t*)c->ibases.p;
    if (c->stage_timing) HIPCHK(c, hipEventRecord(c->ev[EV_H2D], st));
    msmk::k_g2_convert<<<grid1(4 * n, 256), 256, 0, st>>>(d_raw, ib, (uint32_t)n, form == MSM_FORM_MONT ? 1u : 0u, glv ? 1u : 0u);
    if ((rc = enqueue_decompose(c, ps, d_inf, d_scalars, 0, st, true))) return rc;
    if ((rc = enqueue_sort(c, ps, st, true))) return rc;  // ("into": the tally leaves the buckets alone -- k_g2_clear_empty writes the G2 identities)
    uint32_t* flags = (uint32_t*)c->flags.p;
    uint32_t* offsets = (uint32_t*)c->offsets.p;
    uint32_t *bk = (uint32_t*)c->buckets.p, *pt = (uint32_t*)c->partials.p;
    msmk::k_g2_clear_empty<<<grid1(ps.tb * 8, 256), 256, 0, st>>>(offsets, (uint32_t)ps.tb, bk);
    const bool timed = c->stage_timing || (c->ktime_every && (c->ktime_count++ % c->ktime_every) == 0);
    c->acc_last_timed = timed;
    const dim3 gp = grid1(ps.maxpieces, 256);
    const uint32_t* srt = (const uint32_t*)c->sorted.p;
    const uint4* pl = (const uint4*)c->plist.p;
    unsigned long long* clk = (unsigned long long*)c->clk.p;
    if (timed)
        hipExtLaunchKernelGGL(msmk::k_g2_accumulate, gp, dim3(256), 0, st, c->ev[EV_ACC0], c->ev[EV_ACC1], 0, (const uint32_t*)ib, srt, pl,
                              (const uint32_t*)(flags + msmk::FLAG_PIECES), bk, pt, clk);
    else
        hipLaunchKernelGGL(msmk::k_g2_accumulate, gp, dim3(256), 0, st, (const uint32_t*)ib, srt, pl, (const uint32_t*)(flags + msmk::FLAG_PIECES), bk, pt, clk);
    msmk::k_g2_combine<<<msmk::G2_LONG_BLOCKS + msmk::G2_MID_BLOCKS, msmk::G2_COMBINE_BLOCK, 0, st>>>(
        offsets, pt, bk, ps.pmax, split_arg(c, ps), (const uint32_t*)c->pbase.p, flags + msmk::FLAG_MID, flags + msmk::FLAG_MID2,
        (const uint32_t*)c->midlist.p, (uint32_t)ps.tb, flags + msmk::FLAG_LONG, (const uint32_t*)c->longlist.p, (uint32_t*)c->longdone.p,
        flags + msmk::FLAG_PAIRS);
    if (c->stage_timing) HIPCHK(c, hipEventRecord(c->ev[EV_COMBINE], st));
    if ((rc = enqueue_reduce_g2(c, ps, st))) return rc;
    rc = finish_sync<HostG2>(c, ps, n, st, out_jac, out_aff, out_inf);
    if (rc == ARK_RETRY_SLOW) return fail(c, MSM_ERR_HIP, "internal: unexpected error bit 16");  // (a G1 struct-array call's bit)
    if (rc) return rc;
    c->tm.convert_ms = stage_ms(c, EV_H2D, EV_CONVERT);
    return MSM_OK;
}

}  // namespace

extern "C" {

int32_t msm_bn254_g2(msm_ctx* c, const uint32_t* bases_xy, uint32_t base_form, const uint8_t* inf_mask, const uint32_t* scalars, size_t n,
                     uint32_t out_jac[48], uint32_t out_aff[32], uint8_t* out_inf) {
    int32_t rc = check_common(c, bases_xy, scalars, n);
    if (rc) return rc;
    if (base_form != MSM_FORM_STD && base_form != MSM_FORM_MONT) return fail(c, MSM_ERR_BAD_ARG, "unknown base_form %u", base_form);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    Range r_("msm_bn254_g2");
    const auto t0 = std::chrono::steady_clock::now();
    if (n > 0x3FFFFFFFull) return fail(c, MSM_ERR_BAD_ARG, "n = %zu exceeds 2^30-1 points per context call", n);
    HostPin pin_b, pin_s, pin_i;  // pageable caller memory pinned in place for the copies (run_host_input's rule)
    if (!c->no_host_pin) {
        pin_b.pin(bases_xy, n * 128);
        pin_s.pin(scalars, n * 32);
        pin_i.pin(inf_mask, n);
    }
    hipStream_t st = c->stream;
    if ((rc = ensure(c, c->bases, n * 128))) return rc;
    if ((rc = ensure(c, c->scalars, n * 32))) return rc;
    if (inf_mask && (rc = ensure(c, c->inf, n))) return rc;
    if ((rc = h2d(c, c->scalars.p, scalars, n * 32, st))) return rc;
    if (inf_mask && (rc = h2d(c, c->inf.p, inf_mask, n, st))) return rc;
    if ((rc = h2d(c, c->bases.p, bases_xy, n * 128, st))) return rc;
    rc = run_g2(c, (const uint32_t*)c->bases.p, base_form, inf_mask ? (const uint8_t*)c->inf.p : nullptr, (const uint32_t*)c->scalars.p, n, st,
                out_jac, out_aff, out_inf);
    if (rc) return rc;
    c->tm.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return MSM_OK;
}

int32_t msm_bn254_g2_device(msm_ctx* c, const void* d_bases_mont, const void* d_inf_mask, const void* d_scalars, size_t n, void* hip_stream,
                            uint32_t out_jac[48], uint32_t out_aff[32], uint8_t* out_inf) {
    int32_t rc = check_common(c, d_bases_mont, d_scalars, n);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    Range r_("msm_bn254_g2_device");
    const auto t0 = std::chrono::steady_clock::now();
    if (n > 0x3FFFFFFFull) return fail(c, MSM_ERR_BAD_ARG, "n = %zu exceeds 2^30-1 points per context call", n);
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    rc = run_g2(c, (const uint32_t*)d_bases_mont, MSM_FORM_MONT, (const uint8_t*)d_inf_mask, (const uint32_t*)d_scalars, n, st, out_jac, out_aff, out_inf);
    if (rc) return rc;
    c->tm.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return MSM_OK;
}

int32_t msm_bn254_g2_combine(const uint32_t* partials, size_t k, uint32_t flags, uint32_t out_jac[48], uint32_t out_aff[32], uint8_t* out_inf) {
    if (flags & ~(uint32_t)MSM_FLAG_DETERMINISTIC) return MSM_ERR_BAD_ARG;
    return combine_partials<HostG2>(partials, k, out_jac, out_aff, out_inf, (flags & MSM_FLAG_DETERMINISTIC) != 0);
}

}  // extern "C"
