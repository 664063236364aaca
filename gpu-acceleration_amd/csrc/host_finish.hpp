// host_finish.hpp -- the CPU end of an MSM, the same for both groups (G = HostG1, host_g1.hpp, or HostG2, host_g2.hpp): the Horner chain over
// the bit sums the GPU hands back, the fold of partial results (msm_bn254_g1_combine / _g2_combine, the multi-GPU fold) and the output words.
// Host code only (no HIP, no context): tools/host_asan_check.cpp and tools/host_g2_asan_check.cpp run it under ASan / UBSan.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/msm_hip.h"
#include "msm_host_pool.hpp"

// canonical = MSM_FLAG_DETERMINISTIC: the Jacobian result is handed out as its Z = 1 representative (x*R, y*R, R), the identity as (R, R, 0)
// -- the same words for the same group element, whatever order the buckets were filled in (the sort places entries inside a bucket with
// LDS atomics: the XYZZ sums, hence X : Y : Z, differ between identical calls; only the group element does not).  Costs the inversion the
// affine output pays anyway (~10 us of host time for G1), shared when both are asked for.  Without it the Jacobian words are r's own, the
// identity included (Z = 0).
template <class G>
void finish_outputs(const typename G::Jac& r, uint32_t* out_jac, uint32_t* out_aff, uint8_t* out_inf, bool canonical) {
    if (out_inf) *out_inf = G::is_identity(r) ? 1 : 0;
    if (canonical && out_jac) {
        if (G::is_identity(r)) {
            G::store_jac(out_jac, G::identity());
            if (out_aff) std::memset(out_aff, 0, G::AFF_WORDS * 4);
            return;
        }
        const typename G::Jac a = G::normalize(r);
        G::store_jac(out_jac, a);
        if (out_aff) {
            G::store_words(out_aff, G::from_mont(a.x));
            G::store_words(out_aff + G::AFF_WORDS / 2, G::from_mont(a.y));
        }
        return;
    }
    if (out_jac) G::store_jac(out_jac, r);
    if (out_aff) {  // the only inversion of the whole call: callers that want the reference's result type
                    // (Jacobian, metal_msm.rs:228-241) pass NULL and skip it
        typename G::F x, y;
        (void)G::to_affine_std(r, x, y);
        G::store_words(out_aff, x);
        G::store_words(out_aff + G::AFF_WORDS / 2, y);
    }
}

// the fold of k partial results (G::JAC_WORDS words each) in their given order, with the representative chosen by the caller's flags
template <class G>
int32_t combine_partials(const uint32_t* partials, size_t k, uint32_t* out_jac, uint32_t* out_aff, uint8_t* out_inf, bool canonical) {
    if (!partials) return MSM_ERR_BAD_ARG;
    if (k == 0) return MSM_ERR_EMPTY;
    typename G::Jac total = G::identity();
    for (size_t i = 0; i < k; i++) total = G::jadd(total, G::load_jac(partials + i * G::JAC_WORDS));  // fixed order
    finish_outputs<G>(total, out_jac, out_aff, out_inf, canonical);
    return MSM_OK;
}

// final_reduction (metal_msm.rs:204-261) on the CPU.  The device returns, for every (pseudo-)window q of every bucket array v, the bit
// sums Q_u (u < rkb: buckets whose index has bit u set) and the plain sum A, at qsums + ((v * 2^pw_bits + q) * (rkb + 1) + u) * G::JAC_WORDS
// (A at u = rkb).  With S_v = sum_b (b + 1) * B[v][b] and b = q * 2^rkb + b'
//     S_v = sum_q [ A_q + sum_u 2^u Q_q,u ]  +  2^rkb * sum_q q * A_q          (second term: arrays cut into pseudo-windows only)
// and the result is sum_v 2^(spacing * v) S_v (spacing = cbits * tf: tf windows share an array with a window table, tf = 1 without): ONE
// Horner chain over the bit positions p = spacing*v + u with the terms
//     u < rkb:  sum_q Q_q,u   (+ sum_q A_q at u == 0);      rkb <= u < kb:  sum over {q : bit u-rkb of q set} of A_q
// (one doubling and about one addition per position) instead of the reference's chain per window plus c doublings between windows
// (metal_msm.rs:249-258).  Index bits u >= top_bits of the top array (V - 1) hold point-index bits, not the digit (msmplan::glv_top_digit_bits):
// they carry no weight.  The chain is cut into a few segments of geometrically shrinking length (a segment starting at position lo pays lo
// extra doublings to shift its sum), one per host thread: 2 threads reach ~60 % of the serial time, 4 threads ~45 %, more add nothing
// because the shift of the top segment is serial.  TWO threads by default: every further worker lowers the median by a few microseconds and
// raises the MEAN through 2-8 ms outliers in ~1.3 % of the calls (busy hosts; a pool of 15: 2.5 %) -- tools/step_jitter.py.  With one
// shared bucket array (full window table) the chain is cbits - 1 positions long instead of 254.
template <class G>
typename G::Jac host_finish_chain(const uint32_t* qsums, uint32_t V, uint32_t kb, uint32_t rkb, uint32_t pw_bits, uint32_t spacing,
                                  uint32_t top_bits, HostPool* pool) {
    using Jac = typename G::Jac;
    const uint32_t PW = 1u << pw_bits;
    const uint32_t npos = spacing * (V - 1) + (kb > 0 ? kb : 1);  // positions 0 .. npos-1 carry terms
    auto qsum = [&](uint32_t v, uint32_t q, uint32_t u) { return G::load_jac(qsums + ((size_t)(v * PW + q) * (rkb + 1) + u) * G::JAC_WORDS); };
    auto segment = [&](uint32_t lo, uint32_t hi) {  // sum over p in [lo, hi) of 2^p * term(p)
        Jac acc = G::identity();
        for (uint32_t p = hi; p-- > lo;) {
            acc = G::jdbl(acc);
            const uint32_t v = p / spacing, u = p % spacing;
            if (v == V - 1 && u >= top_bits) {
                // index bits of a spread top window that hold point-index bits, not the digit: no weight
            } else if (u < rkb)
                for (uint32_t q = 0; q < PW; q++) acc = G::jadd(acc, qsum(v, q, u));
            else if (u < kb)
                for (uint32_t q = 0; q < PW; q++)
                    if ((q >> (u - rkb)) & 1u) acc = G::jadd(acc, qsum(v, q, rkb));
            if (u == 0)
                for (uint32_t q = 0; q < PW; q++) acc = G::jadd(acc, qsum(v, q, rkb));
        }
        for (uint32_t k = 0; k < lo; k++) acc = G::jdbl(acc);
        return acc;
    };
    const int nseg = pool ? std::min<int>(pool->size() + 1, 8) : 1;
    if (nseg == 1 || npos < 16) return segment(0, npos);
    // segment k has length proportional to 0.7^k (a doubling costs ~0.3 of a position's doubling + addition)
    uint32_t bound[9];
    double tot = 0, wgt = 1;
    for (int k = 0; k < nseg; k++, wgt *= 0.7) tot += wgt;
    double run = 0;
    wgt = 1;
    bound[0] = 0;
    for (int k = 0; k < nseg; k++, wgt *= 0.7) {
        run += wgt;
        bound[k + 1] = k + 1 == nseg ? npos : (uint32_t)(npos * (run / tot) + 0.5);
    }
    std::vector<Jac> part((size_t)nseg);
    pool->run(nseg, [&](int k) { part[(size_t)k] = segment(bound[k], bound[k + 1]); });  // job 0 (the longest) is taken first
    Jac total = part[0];
    for (int k = 1; k < nseg; k++) total = G::jadd(total, part[(size_t)k]);
    return total;
}
