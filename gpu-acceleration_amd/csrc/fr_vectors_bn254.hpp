// fr_vectors_bn254.hpp -- vectors over the BN254 scalar field made in HBM: the scalars of a setup (Groth16 queries, KZG powers) in the form the
// fixed-base calls read.  Powers scale * base^(first + i), element-wise inverses (Montgomery's trick), the Lagrange coefficients L_i(tau) of the
// transforms' domain, and the linear combination ka a + kb b + kc c.  The per-lane routines (__host__ __device__) and the kernels that run them.
// tools/fr_vectors_check.cpp runs the SAME routines on the CPU, lane by lane, under -DFP_BOUNDS_CHECK.
//
// Forms (fr_bn254.hpp: raw / rep).  The words of an array are read as raw limbs: raw(x) = rep(x * 2^-261), and raw(x * 2^256) = rep(x * 2^-5) for
// arkworks words.  Every routine works on what it loads and folds ALL changes of form into one constant the host prepares (FrvInverse::post, the
// start of a power walk, Lagrange's scale): no element pays a multiplication for a conversion.
//
// Chains.  The inverse and the Lagrange kernels run Montgomery's trick with ONE fr_inv per chain of G = inv_group elements, the layout of
// k_fb2_normalise: lane l of (global) wave w owns the elements (w * G + s) * 64 + l, s < G, so at every step of a chain a wavefront reads and
// writes 64 neighbouring elements (2 KiB).  The prefix products stay in registers (G is a template argument and the steps are unrolled by
// template recursion: nothing is indexed at run time, no scratch memory); the way down loads the element a second time instead of keeping it.  A workgroup of FRV_BLOCK = 256
// lanes covers block_points = 256 G consecutive elements.  Elements at or above n are neither read nor written.
//
// Bounds (values in units of r; 2^261 ~ 169 r).  A loaded word is any 256-bit pattern: < 5.3.  fr_mul(A, B) < A B / 169 + 1.
//   running product   run < 2:  run * u < 2 * 5.3 / 169 + 1 < 2;  run * d with a difference d < 5: the same
//   fr_inv(run)       < 2 (fr_bn254.hpp);  times post (canonical) < 2
//   on the way down   ni = inv * prefix < 2 * 2 / 169 + 1 < 2: fr_reduce_lt2r gives the canonical output;  inv * u < 2
//   a power walk      cur < 2, the stride's power < 2:  cur * step < 2
//   lincomb           three products word * rep(k) < 5.3 * 2 / 169 + 1 < 2 each, their sum < 6, times the canonical post < 6 / 169 + 1 < 2
//   host arguments    (frv_*_args, frv_pow_u64) every factor is a constant of ntt_consts(), an fr_from_std, an fr_inv / fr_pow_u32 result or a
//                     product of two such: < 2, so every product is < 2 * 2 / 169 + 1 < 2 and every fr_sub<3> has a subtrahend < 2
// No operand of an fr_mul here exceeds 5.3: fr_mul's precondition A * B < (2^261 - r) * 2^261 (fr_bn254.hpp) holds with room everywhere.
#pragma once
#include "ntt_bn254.hpp"

namespace frvk {

using namespace nttk;

constexpr uint32_t FRV_WAVE = 64;
constexpr uint32_t FRV_BLOCK = 256;       // lanes of a workgroup of every kernel here
constexpr uint32_t FRV_INV_GROUP = 8;     // elements of one chain = elements per field inversion: the fastest whose kernel needs no scratch memory (16 is faster and spills: DESIGN.md 9g)
constexpr uint32_t FRV_POW_STEPS = 16;    // elements one lane of the power walk makes: a wavefront covers 2^10 consecutive elements
constexpr uint32_t FRV_POW_WAVE_LOG2 = 10;
constexpr uint32_t FRV_MAX_LOG2 = 36;     // a call covers at most 2^36 elements (the transforms' limit)
static_assert(FRV_WAVE * FRV_POW_STEPS == 1u << FRV_POW_WAVE_LOG2, "a wavefront's share of the power walk is a power of two");

struct FrvPlan {  // == msm_fr_vector_plan_t
    uint32_t inv_group;            // elements that share one field inversion
    uint32_t block_points;         // elements one workgroup of the inverse / Lagrange kernels covers
    uint32_t powers_block_points;  // ... of the powers kernel
    uint32_t reserved;
};
inline FrvPlan frv_plan(uint32_t G = FRV_INV_GROUP) { return FrvPlan{G, FRV_BLOCK * G, FRV_BLOCK * FRV_POW_STEPS, 0}; }
inline bool frv_group_ok(uint32_t G) { return G == 4 || G == 8 || G == 16 || G == 32; }

NTT_HD fr frv_load(const uint32_t* p, size_t i) {  // any 256-bit pattern: normalised, < 5.3 r
    uint32_t w[8];
    ntt_load8(p + i * 8, w);
    return fr_unpack(w);
}
// a: normalised, < 2r -> its canonical words
NTT_HD void frv_store(uint32_t* p, size_t i, const fr& a) {
    uint32_t w[8];
    fr_pack(w, fr_reduce_lt2r(a));
    ntt_store8(p + i * 8, w);
}
NTT_HD void frv_store_zero(uint32_t* p, size_t i) {
    const uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    ntt_store8(p + i * 8, w);
}
NTT_HD bool frv_same(const fr& a, const fr& b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) d |= a.v[i] ^ b.v[i];
    return d == 0;
}

// ---- chains: lane t (over the whole grid) owns first + s * 64, s < G ----------------------------------------------------------------------
NTT_HD size_t frv_chain_first(size_t lane_global, uint32_t G) { return (lane_global / FRV_WAVE) * ((size_t)FRV_WAVE * G) + lane_global % FRV_WAVE; }
NTT_HD size_t frv_chain_lanes(size_t n, uint32_t G) { return (n + (size_t)FRV_WAVE * G - 1) / ((size_t)FRV_WAVE * G) * FRV_WAVE; }

// base^e from the powers pw[k] = base^(2^k): one multiplication per set bit; acc, pw[k] < 2r
NTT_HD fr frv_mul_pow(fr acc, const fr* pw, uint64_t e) {
    for (uint32_t k = 0; e; k++, e >>= 1)
        if (e & 1u) acc = fr_mul(acc, pw[k]);
    return acc;
}

// ---- batch inversion -----------------------------------------------------------------------------------------------------------------------
// The chain multiplies the words AS LOADED, v = rep(x * c) with c = 2^-261 (standard words) or 2^-5 (arkworks words); the inverse of the
// product times post = rep(c * f * 2^-261), f = 1 or 2^256 the output form, turns every rep(1 / (x c)) of the way down into raw(f / x).
struct FrvInverse {
    fr post;
};
inline FrvInverse frv_inverse_args(uint32_t flags) {
    const NttConsts& K = ntt_consts();
    const fr cin = flags & NTT_F_IN_MONT ? K.m5 : K.m261, cout = flags & NTT_F_OUT_MONT ? K.m5 : K.m261;  // (f * 2^-261 = 2^-5 for arkworks words)
    return FrvInverse{fr_canonical(fr_mul(cin, cout))};
}
// an element = 0 (mod r), spelled 0, r, .. 5r, enters the product as 1 and leaves as 0.  The steps of a chain are unrolled by template recursion
// (a loop of this size is not unrolled on request): every index into pre[] is a constant and the array lives in registers.
template <uint32_t G, uint32_t S>
FP_HD void frv_inverse_up(const uint32_t* in, size_t n, size_t first, fr (&pre)[G], fr& run, uint32_t& zeros) {
    if constexpr (S < G) {
        const size_t i = first + (size_t)S * FRV_WAVE;
        pre[S] = run;
        if (i < n) {
            const fr u = frv_load(in, i);
            if (fr_is_zero_exact(fr_canonical(u))) zeros |= 1u << S;
            else run = fr_mul(run, u);  // < 2 * 5.3 / 169 + 1
        }
        frv_inverse_up<G, S + 1>(in, n, first, pre, run, zeros);
    }
}
template <uint32_t G, uint32_t T>  // step S = G - 1 - T: the way down
FP_HD void frv_inverse_down(const uint32_t* in, uint32_t* out, size_t n, size_t first, const fr (&pre)[G], fr& inv, uint32_t zeros) {
    if constexpr (T < G) {
        constexpr uint32_t S = G - 1 - T;
        const size_t i = first + (size_t)S * FRV_WAVE;
        if (i < n) {
            if (zeros >> S & 1u) {
                frv_store_zero(out, i);
            } else {
                const fr u = frv_load(in, i);  // (out may be in: this lane alone touches element i, and reads it before it writes it)
                frv_store(out, i, fr_mul(inv, pre[S]));
                inv = fr_mul(inv, u);
            }
        }
        frv_inverse_down<G, T + 1>(in, out, n, first, pre, inv, zeros);
    }
}
template <uint32_t G>
NTT_HD void frv_inverse_chain(const FrvInverse& a, const uint32_t* in, uint32_t* out, size_t n, size_t first) {
    fr pre[G];
    fr run = fr_one();
    uint32_t zeros = 0;
    frv_inverse_up<G, 0>(in, n, first, pre, run, zeros);
    fr inv = fr_mul(fr_inv(run), a.post);  // run is a product of non-zero elements
    frv_inverse_down<G, 0>(in, out, n, first, pre, inv, zeros);
}

// ---- powers: out[i] = scale * base^(first + i) -----------------------------------------------------------------------------------------------
// Lane l of (global) wave w makes the elements w * 2^10 + s * 64 + l, s < 16: it starts from start * base^l * base^(w * 2^10) -- six
// multiplications for its own bits, one per set bit of w for the wavefront's -- and walks the stride base^64.  start = rep(scale * base^first * f *
// 2^-261) carries the scale, the first exponent and the output form.  base = 0 needs no special case: every power is 0 but the empty product.
struct FrvPowers {
    fr start;
    fr pw[FRV_MAX_LOG2];  // base^(2^k), < 2r
};
inline fr frv_out_factor(uint32_t flags) { return flags & NTT_F_OUT_MONT ? ntt_consts().m5 : ntt_consts().m261; }
inline fr frv_pow_u64(const fr& a, uint64_t e) {  // a^e, 0^0 = 1
    fr acc = fr_one(), b = a;
    for (; e; e >>= 1) {
        if (e & 1u) acc = fr_mul(acc, b);
        b = fr_mul(b, b);
    }
    return acc;
}
inline FrvPowers frv_powers_args(const fr& base, const fr& scale, uint64_t first, uint32_t flags) {
    FrvPowers a;
    a.start = fr_mul(fr_mul(scale, frv_pow_u64(base, first)), frv_out_factor(flags));
    a.pw[0] = base;
    for (uint32_t k = 1; k < FRV_MAX_LOG2; k++) a.pw[k] = fr_mul(a.pw[k - 1], a.pw[k - 1]);
    return a;
}
NTT_HD size_t frv_powers_lanes(size_t n) { return ((n + (1u << FRV_POW_WAVE_LOG2) - 1) >> FRV_POW_WAVE_LOG2) * FRV_WAVE; }
NTT_HD void frv_powers_lane(const FrvPowers& a, size_t lane_global, uint32_t* out, size_t n) {
    const size_t wave = lane_global / FRV_WAVE;
    const uint32_t l = (uint32_t)(lane_global % FRV_WAVE);
    size_t i = (wave << FRV_POW_WAVE_LOG2) + l;
    if (i >= n) return;
    fr cur = a.start;
#pragma unroll
    for (uint32_t k = 0; k < 6; k++)
        if (l >> k & 1u) cur = fr_mul(cur, a.pw[k]);
    cur = frv_mul_pow(cur, a.pw + FRV_POW_WAVE_LOG2, wave);  // (n <= 2^36: wave < 2^26)
    for (uint32_t s = 0; s < FRV_POW_STEPS && i < n; s++, i += FRV_WAVE) {
        frv_store(out, i, cur);
        cur = fr_mul(cur, a.pw[6]);
    }
}

// ---- Lagrange coefficients: out[i] = Z(tau) w^i / (n (tau - w^i)), Z(tau) = tau^n - 1 ----------------------------------------------------------
// One chain per lane as the inversion's, over the denominators d_s = tau - w^(first + 64 s): w walks up the chain with w^64 and back down with
// w^-64, so neither it nor d_s is kept.  scale = rep(Z(tau) / n * f * 2^-261) enters the inverted product once.  tau IN the domain (the host
// decides: tau^n = 1) has Z = 0 and one zero denominator: `unit` then makes the kernel compare instead of invert -- out[i] = 1 where w^i = tau.
struct FrvLagrange {
    fr tau;           // canonical rep
    fr scale;         // canonical rep; with unit: the words of 1 in the output form, as raw limbs
    fr step, unstep;  // w^64, w^-64
    fr pw[NTT_MAX_LOG2];  // w^(2^k)
    uint32_t unit;
};
inline FrvLagrange frv_lagrange_args(const fr& tau_in, uint32_t log_n, uint32_t flags) {
    FrvLagrange a{};
    a.tau = fr_canonical(tau_in);
    fr w = ntt_root(log_n);
    for (uint32_t k = 0; k < NTT_MAX_LOG2; k++) {  // (from k = log_n on the powers are 1: never selected, the indices are below n)
        a.pw[k] = w;
        w = fr_mul(w, w);
    }
    a.step = log_n > 6 ? a.pw[6] : fr_one();
    a.unstep = fr_inv(a.step);
    fr tn = a.tau;
    for (uint32_t k = 0; k < log_n; k++) tn = fr_mul(tn, tn);
    const fr z = fr_canonical(fr_sub<3>(tn, fr_one()));  // tau^n - 1
    a.unit = fr_is_zero_exact(z);
    if (a.unit) {
        a.scale = fr_reduce_lt2r(fr_mul(fr_one(), frv_out_factor(flags)));  // raw(f)
    } else {
        const fr n_inv = fr_pow_u32(ntt_consts().inv2, log_n);
        a.scale = fr_canonical(fr_mul(fr_mul(z, n_inv), frv_out_factor(flags)));
    }
    return a;
}
template <uint32_t G, uint32_t S>
FP_HD void frv_lagrange_up(const FrvLagrange& a, size_t n, size_t first, fr (&pre)[G], fr& run, fr& w) {
    if constexpr (S < G) {
        pre[S] = run;
        if (first + (size_t)S * FRV_WAVE < n) {
            run = fr_mul(run, fr_sub<3>(a.tau, w));  // tau < 1, w < 2: the difference < 4, never 0 (tau is not in the domain)
            w = fr_mul(w, a.step);
        }
        frv_lagrange_up<G, S + 1>(a, n, first, pre, run, w);
    }
}
template <uint32_t G, uint32_t T>
FP_HD void frv_lagrange_down(const FrvLagrange& a, uint32_t* out, size_t n, size_t first, const fr (&pre)[G], fr& inv, fr& w) {
    if constexpr (T < G) {
        constexpr uint32_t S = G - 1 - T;
        const size_t i = first + (size_t)S * FRV_WAVE;
        if (i < n) {
            w = fr_mul(w, a.unstep);
            const fr ni = fr_mul(inv, pre[S]);
            inv = fr_mul(inv, fr_sub<3>(a.tau, w));
            frv_store(out, i, fr_mul(ni, w));  // 2 * 2 / 169 + 1 < 2
        }
        frv_lagrange_down<G, T + 1>(a, out, n, first, pre, inv, w);
    }
}
template <uint32_t G>
NTT_HD void frv_lagrange_chain(const FrvLagrange& a, uint32_t* out, size_t n, size_t lane_global) {
    const size_t first = frv_chain_first(lane_global, G);
    if (first >= n) return;
    const uint32_t l = (uint32_t)(lane_global % FRV_WAVE);
    fr w = fr_one();
#pragma unroll
    for (uint32_t k = 0; k < 6; k++)
        if (l >> k & 1u) w = fr_mul(w, a.pw[k]);
    w = frv_mul_pow(w, a.pw + 6, (uint64_t)(lane_global / FRV_WAVE) * G);  // w^first: first = (wave * G) * 64 + l < n
    if (a.unit) {
        for (uint32_t s = 0; s < G; s++) {
            const size_t i = first + (size_t)s * FRV_WAVE;
            if (i >= n) break;
            if (frv_same(fr_reduce_lt2r(w), a.tau)) frv_store(out, i, a.scale);
            else frv_store_zero(out, i);
            w = fr_mul(w, a.step);
        }
        return;
    }
    fr pre[G];
    fr run = fr_one();
    frv_lagrange_up<G, 0>(a, n, first, pre, run, w);
    fr inv = fr_mul(fr_inv(run), a.scale);
    frv_lagrange_down<G, 0>(a, out, n, first, pre, inv, w);
}

// ---- linear combination: out = ka a + kb b + kc c ------------------------------------------------------------------------------------------
// word * rep(k) = the product in the form of the INPUT words; post = rep(2^(256 (out_mont - in_mont))), canonical, reduces the sum
struct FrvLincomb {
    fr ka, kb, kc;  // rep, < 2r
    fr post;
};
inline FrvLincomb frv_lincomb_args(const fr& ka, const fr& kb, const fr& kc, uint32_t flags) {
    const bool im = flags & NTT_F_IN_MONT, om = flags & NTT_F_OUT_MONT;
    return FrvLincomb{ka, kb, kc, fr_canonical(om == im ? fr_one() : (om ? ntt_consts().p256 : ntt_consts().m256))};
}
NTT_HD void frv_lincomb_one(const FrvLincomb& k, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, size_t i) {
    fr x = fr_mul(frv_load(a, i), k.ka);              // < 5.3 * 2 / 169 + 1 < 2
    if (b) x = fr_add(x, fr_mul(frv_load(b, i), k.kb));  // < 4
    if (c) x = fr_add(x, fr_mul(frv_load(c, i), k.kc));  // < 6
    frv_store(out, i, fr_mul(x, k.post));             // < 6 / 169 + 1 < 2
}

#if defined(__HIPCC__) && !defined(NTT_NO_KERNELS)
template <uint32_t G>
__global__ void __launch_bounds__(FRV_BLOCK) k_frv_batch_inverse(const FrvInverse a, const uint32_t* in, uint32_t* out, size_t n) {
    const size_t first = frv_chain_first((size_t)blockIdx.x * FRV_BLOCK + threadIdx.x, G);
    if (first < n) frv_inverse_chain<G>(a, in, out, n, first);
}
__global__ void __launch_bounds__(FRV_BLOCK) k_frv_powers(const FrvPowers a, uint32_t* out, size_t n) {
    frv_powers_lane(a, (size_t)blockIdx.x * FRV_BLOCK + threadIdx.x, out, n);
}
template <uint32_t G>
__global__ void __launch_bounds__(FRV_BLOCK) k_frv_lagrange(const FrvLagrange a, uint32_t* out, size_t n) {
    frv_lagrange_chain<G>(a, out, n, (size_t)blockIdx.x * FRV_BLOCK + threadIdx.x);
}
__global__ void __launch_bounds__(FRV_BLOCK) k_frv_lincomb(const FrvLincomb k, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * FRV_BLOCK + threadIdx.x;
    if (i < n) frv_lincomb_one(k, a, b, c, out, i);
}
#endif

}  // namespace frvk
