// ntt_bn254.hpp -- number-theoretic transform over the BN254 scalar field: the plan, the tile index routines and the three phases of a pass
// (load, butterfly level, store) as __host__ __device__ functions, and the kernels that run them.  tools/ntt_check.cpp runs the SAME phases on
// the CPU, tile group by tile group, under -DFP_BOUNDS_CHECK.
//
// A transform of n = 2^k elements is cut into P passes of t_0 + ... + t_(P-1) = k bits (ntt_make_plan).  Before pass p the array is indexed
//     [ j_0 .. j_(p-1) | i_p | rest ]       L = t_0 + .. + t_(p-1) bits of finished output digits (j_0 most significant), t = t_p, R = k - L - t
// and the pass runs, for every (prefix, rest), the 2^t-point transform over i_p inside LDS, multiplies by the twiddle w_M^(j_p * rest) of the
// remaining size M = 2^(k-L) and writes j_p where i_p was.  The LAST pass (R = 0) writes element (prefix, j) to j_0 + 2^t_0 j_1 + ... + 2^L j:
// natural order comes out of the addressing, there is no bit-reversal sweep.  A one-pass transform works in place; with P > 1 the first pass
// writes to a scratch array of the same size, the middle passes work there, and the last pass writes back: the array is read and written P times.
//
// Inside LDS a workgroup holds 2^T elements as 9 x 29-bit limbs (36 bytes; the odd word stride keeps consecutive elements on distinct banks):
// 2^(T-t) tiles of 2^t points side by side ("columns", consecutive `rest`, so their global accesses are contiguous).  Elements are placed at the
// bit-reversed row and t decimation-in-time levels leave the rows in natural order.  Bounds: a row starts < 2r; a level computes
// x = v * w (< V/169 r + r < 2r for V < 84r), u + x and u + 3r - x, so after s levels every value is < (2 + 3s) r <= 38r for t <= 12.
//
// What crosses global memory between two passes is the canonical internal form (rep, < r, 8 words).  The caller's words are converted in the
// first load and the last store, which also carry the coset powers and 1/n: one multiplication by a constant or by the product of two table
// entries (fr_bn254.hpp explains raw / rep).
#pragma once
#include "fr_bn254.hpp"

#include <string.h>

namespace nttk {

using namespace bn254;

constexpr uint32_t NTT_MAX_LOG2 = 28;       // two-adicity of r - 1
constexpr uint32_t NTT_MAX_PASSES = 8;
constexpr uint32_t NTT_TILE_LOG2 = 10;      // production tile: 2^10 x 36 B = 36 KiB of LDS, four workgroups per CU
constexpr uint32_t NTT_TILE_SMALL_LOG2 = 4; // hooks build only (msm_test_ntt_set_tile_log2): makes 2^12 a three-pass transform
constexpr uint32_t NTT_WT_LOG2 = 10;        // the butterfly table holds w_(2^10)^e, e < 2^9; smaller tiles read it at a stride

#define NTT_HD __host__ __device__ inline

struct NttPlan {
    uint32_t passes;
    uint32_t radix[NTT_MAX_PASSES];
};
// k <= T: one pass.  Otherwise ceil(k / T) passes of nearly equal width, the wider ones first (2^20, T = 10: 10 + 10; 2^21: 7 + 7 + 7).
NTT_HD NttPlan ntt_make_plan(uint32_t k, uint32_t T) {
    NttPlan p{};
    if (k <= T) {
        p.passes = 1;
        p.radix[0] = k;
        return p;
    }
    p.passes = (k + T - 1) / T;
    const uint32_t base = k / p.passes, extra = k % p.passes;
    for (uint32_t i = 0; i < p.passes; i++) p.radix[i] = base + (i < extra ? 1u : 0u);
    return p;
}

enum : uint32_t { NTT_IN_REP = 0, NTT_IN_FACTOR = 1, NTT_IN_COSET = 2 };       // how the load turns 8 words into an element
enum : uint32_t { NTT_OUT_TWIDDLE = 0, NTT_OUT_FACTOR = 1, NTT_OUT_COSET = 2 };  // what the store multiplies by

struct NttPass {
    uint32_t k, t, L, R;  // log2 n, this pass' width, bits finished before it, bits left after it
    uint32_t p;           // its number
    uint32_t radix[NTT_MAX_PASSES];
    uint32_t last;        // R == 0: output index is the digit-reversed prefix
    uint32_t in_mode, out_mode;
    uint32_t tw_h, cs_h;  // low-level bits of the twiddle table of size k / of the coset table
    uint64_t total_tiles; // batch << (k - t)
    fr factor_in, factor_out;
};
struct NttTables {
    const uint32_t* wt;     // w_(2^NTT_WT_LOG2)^e, e < 2^(NTT_WT_LOG2 - 1), of the direction; canonical rep, 8 words each
    const uint32_t* tw_lo;  // rho^e, e < 2^tw_h          (rho = w_k or its inverse)
    const uint32_t* tw_hi;  // rho^(e << tw_h), e < 2^(k - tw_h)
    const uint32_t* cs_lo;  // scale * g^e, e < 2^cs_h    (g, or 1/g with scale = the output factor)
    const uint32_t* cs_hi;  // g^(e << cs_h)
};

NTT_HD uint32_t ntt_bitrev(uint32_t i, uint32_t t) {
    if (t == 0) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(i) >> (32 - t);
#else
    uint32_t r = 0;
    for (uint32_t b = 0; b < t; b++) r |= ((i >> b) & 1u) << (t - 1 - b);
    return r;
#endif
}
// prefix = j_0 .. j_(p-1), j_0 most significant  ->  j_0 + 2^t_0 j_1 + ...
NTT_HD uint32_t ntt_digit_reverse(const NttPass& ps, uint32_t prefix) {
    uint32_t rev = 0, out_shift = 0, rem = ps.L;
    for (uint32_t i = 0; i < ps.p; i++) {
        rem -= ps.radix[i];
        rev |= ((prefix >> rem) & ((1u << ps.radix[i]) - 1u)) << out_shift;
        out_shift += ps.radix[i];
    }
    return rev;
}

NTT_HD void ntt_load8(const uint32_t* p, uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 a = ((const uint4*)p)[0], b = ((const uint4*)p)[1];
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
#else
    memcpy(w, p, 32);
#endif
}
NTT_HD void ntt_store8(uint32_t* p, const uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
    ((uint4*)p)[0] = make_uint4(w[0], w[1], w[2], w[3]);
    ((uint4*)p)[1] = make_uint4(w[4], w[5], w[6], w[7]);
#else
    memcpy(p, w, 32);
#endif
}
NTT_HD fr ntt_table(const uint32_t* tab, uint32_t e) {  // a canonical entry: normalised, < r
    uint32_t w[8];
    ntt_load8(tab + (size_t)e * 8, w);
    return fr_unpack(w);
}
// lo[e & mask] * hi[e >> h]: < r*r/2^261 + r < 2r
NTT_HD fr ntt_table2(const uint32_t* lo, const uint32_t* hi, uint32_t h, uint32_t e) {
    return fr_mul(ntt_table(lo, e & ((1u << h) - 1u)), ntt_table(hi, e >> h));
}
NTT_HD fr ntt_lds_get(const uint32_t* lds, uint32_t slot) {
    fr a;
#pragma unroll
    for (int i = 0; i < 9; i++) a.v[i] = lds[slot * 9 + i];
    return a;
}
NTT_HD void ntt_lds_put(uint32_t* lds, uint32_t slot, const fr& a) {
#pragma unroll
    for (int i = 0; i < 9; i++) lds[slot * 9 + i] = a.v[i];
}

// where tile q (over all arrays of the batch) sits: the array's first element and the tile's (prefix, rest)
struct NttTile {
    size_t base;
    uint32_t prefix, rest;
};
NTT_HD NttTile ntt_tile(const NttPass& ps, uint64_t q) {
    const uint32_t tl = ps.k - ps.t;
    const uint32_t qq = (uint32_t)(q & ((1ull << tl) - 1ull));
    return NttTile{(size_t)(q >> tl) << ps.k, qq >> ps.R, qq & ((1u << ps.R) - 1u)};
}

// ---- phase 1: slot x of the workgroup's 2^T (column = x mod 2^(T-t), row i = x >> (T-t)) from global memory to its bit-reversed row
template <uint32_t T>
NTT_HD void ntt_phase_load(const NttPass& ps, const NttTables& tb, const uint32_t* src, uint64_t group, uint32_t x, uint32_t* lds) {
    const uint32_t c = T - ps.t, col = x & ((1u << c) - 1u), i = x >> c;
    const uint32_t slot = (ntt_bitrev(i, ps.t) << c) | col;
    const uint64_t q = (group << c) | col;
    if (q >= ps.total_tiles) {  // the last group of a small call: columns without a tile stay zero
        ntt_lds_put(lds, slot, fr_zero());
        return;
    }
    const NttTile tl = ntt_tile(ps, q);
    const uint32_t idx = (tl.prefix << (ps.t + ps.R)) | (i << ps.R) | tl.rest;
    uint32_t w[8];
    ntt_load8(src + (tl.base + idx) * 8, w);
    fr a = fr_unpack(w);  // NTT_IN_REP: canonical rep, < r.  Otherwise any 256-bit pattern (< 5.3r) times a factor < 2r: < 2r
    if (ps.in_mode == NTT_IN_FACTOR) a = fr_mul(a, ps.factor_in);
    else if (ps.in_mode == NTT_IN_COSET) a = fr_mul(a, ntt_table2(tb.cs_lo, tb.cs_hi, ps.cs_h, idx));  // (first pass: idx is the natural index)
    ntt_lds_put(lds, slot, a);
}

// ---- phase 2: level s (rows a and a + 2^s), work item wi < 2^(T-1).  Values entering level s are < (2 + 3s) r: u + x < (2 + 3s) r + 2r and
// u + 3r - x < (2 + 3s) r + 3r.  s <= 9 here (twelve levels would end below 38r): rows stay far below 2^261 - r ~ 168.28 r, where fr_mul's precondition
// A * B < (2^261 - r) * 2^261 holds against any normalised factor (tests/test_gpu_22_fr_ops.py runs twelve levels on the device)
template <uint32_t T>
NTT_HD void ntt_phase_butterfly(const NttPass& ps, const NttTables& tb, uint32_t s, uint32_t wi, uint32_t* lds) {
    const uint32_t c = T - ps.t, col = wi & ((1u << c) - 1u), bf = wi >> c;
    const uint32_t half = 1u << s, e = bf & (half - 1u);
    const uint32_t a = ((bf >> s) << (s + 1)) | e;
    const uint32_t s0 = (a << c) | col, s1 = ((a + half) << c) | col;
    const fr u = ntt_lds_get(lds, s0);
    fr x = ntt_lds_get(lds, s1);
    if (s != 0) x = fr_mul(x, ntt_table(tb.wt, e << (NTT_WT_LOG2 - 1 - s)));  // w_(2^(s+1))^e; level 0 multiplies by 1 (x < 2r as loaded)
    ntt_lds_put(lds, s0, fr_add(u, x));
    ntt_lds_put(lds, s1, fr_sub<3>(u, x));  // x < 2r
}

// ---- phase 3: slot x (row j) times the pass' factor, canonical, to global memory
template <uint32_t T>
NTT_HD void ntt_phase_store(const NttPass& ps, const NttTables& tb, uint32_t* dst, uint64_t group, uint32_t x, const uint32_t* lds) {
    const uint32_t c = T - ps.t, col = x & ((1u << c) - 1u), j = x >> c;
    const uint64_t q = (group << c) | col;
    if (q >= ps.total_tiles) return;
    const NttTile tl = ntt_tile(ps, q);
    uint32_t idx;
    fr f;
    if (!ps.last) {
        idx = (tl.prefix << (ps.t + ps.R)) | (j << ps.R) | tl.rest;
        f = ntt_table2(tb.tw_lo, tb.tw_hi, ps.tw_h, (j * tl.rest) << ps.L);  // w_(2^(k-L))^(j * rest) = rho^((j * rest) << L), exponent < 2^k
    } else {
        idx = ntt_digit_reverse(ps, tl.prefix) | (j << ps.L);
        f = ps.out_mode == NTT_OUT_COSET ? ntt_table2(tb.cs_lo, tb.cs_hi, ps.cs_h, idx) : ps.factor_out;
    }
    // element < 38r, factor < 2r: product < 2r
    uint32_t w[8];
    fr_pack(w, fr_reduce_lt2r(fr_mul(ntt_lds_get(lds, x), f)));
    ntt_store8(dst + (tl.base + idx) * 8, w);
}

// table entry e: scale * base^e, canonical (base, scale: rep, < 2r)
NTT_HD void ntt_pow_entry(const fr& base, const fr& scale, uint32_t e, uint32_t* out) {
    uint32_t w[8];
    fr_pack(w, fr_canonical(fr_mul(scale, fr_pow_u32(base, e))));
    ntt_store8(out + (size_t)e * 8, w);
}

// out = (a * b - c) * k on 8-word elements: pre = the factor that lifts a (see msm_ntt.inc), post = k in the output form.  c: any 256-bit
// pattern (< 5.3r < 6r: pad 7r).  Product < 2r, difference < 9r, result < 2r.
NTT_HD void ntt_mul_sub_scale_one(const uint32_t* a, const uint32_t* b, const uint32_t* c, const fr& pre, const fr& post, uint32_t* out) {
    uint32_t w[8];
    ntt_load8(a, w);
    fr x = fr_mul(fr_unpack(w), pre);
    ntt_load8(b, w);
    x = fr_mul(x, fr_unpack(w));
    if (c) {
        ntt_load8(c, w);
        x = fr_sub<7>(x, fr_unpack(w));
    }
    fr_pack(w, fr_reduce_lt2r(fr_mul(x, post)));
    ntt_store8(out, w);
}

// ---- the host's share: constants and pass descriptors (used by msm_ntt.inc and tools/ntt_check.cpp alike) ----------------------------------
struct NttConsts {
    fr p261, p5, m261, m5, inv2, p256, m256;  // rep(2^261), rep(2^5), rep(2^-261), rep(2^-5), rep(1/2), rep(2^256), rep(2^-256)
    NttConsts() {
        const fr two = fr_add(fr_one(), fr_one());
        p261 = fr_pow_u32(two, 261);
        p5 = fr_pow_u32(two, 5);
        m261 = fr_inv(p261);
        m5 = fr_inv(p5);
        inv2 = fr_inv(two);
        p256 = fr_pow_u32(two, 256);
        m256 = fr_inv(p256);
    }
};
inline const NttConsts& ntt_consts() {
    static const NttConsts c;
    return c;
}
inline fr ntt_root(uint32_t k) {  // rep(w_k), w_k = w_28^(2^(28-k)); < 2r
    fr w = fr_const(FR29_ROOT28);
    for (uint32_t i = k; i < NTT_MAX_LOG2; i++) w = fr_mul(w, w);
    return w;
}
constexpr uint32_t NTT_F_INVERSE = 1u, NTT_F_IN_MONT = 2u, NTT_F_OUT_MONT = 4u;  // == MSM_NTT_* of include/msm_hip.h
// the caller's words as raw limbs times this give rep(x): rep(2^261) for plain integers, rep(2^5) for x * 2^256
inline fr ntt_factor_in(uint32_t flags) { return flags & NTT_F_IN_MONT ? ntt_consts().p5 : ntt_consts().p261; }
// rep(x) times this gives the output words as raw limbs: rep(s * 2^-261) resp. rep(s * 2^-5), s = 1/n for an inverse transform
inline fr ntt_factor_out(uint32_t k, uint32_t flags) {
    fr f = flags & NTT_F_OUT_MONT ? ntt_consts().m5 : ntt_consts().m261;
    if (flags & NTT_F_INVERSE) f = fr_mul(f, fr_pow_u32(ntt_consts().inv2, k));  // both fr_inv / fr_pow_u32 results, < 2r: the product < 2r
    return f;
}
inline uint32_t ntt_split(uint32_t k) { return (k + 1) / 2; }  // low-level bits of a two-level table over k-bit exponents
inline uint32_t ntt_make_passes(uint32_t k, uint32_t T, size_t batch, uint32_t flags, bool coset, NttPass out[NTT_MAX_PASSES]) {
    const NttPlan pl = ntt_make_plan(k, T);
    uint32_t L = 0;
    for (uint32_t p = 0; p < pl.passes; p++) {
        NttPass& ps = out[p];
        ps = NttPass{};
        ps.k = k, ps.t = pl.radix[p], ps.L = L, ps.R = k - L - ps.t, ps.p = p;
        for (uint32_t i = 0; i < NTT_MAX_PASSES; i++) ps.radix[i] = pl.radix[i];
        ps.last = p + 1 == pl.passes;
        ps.in_mode = p ? NTT_IN_REP : (coset && !(flags & NTT_F_INVERSE) ? NTT_IN_COSET : NTT_IN_FACTOR);
        ps.out_mode = !ps.last ? NTT_OUT_TWIDDLE : (coset && (flags & NTT_F_INVERSE) ? NTT_OUT_COSET : NTT_OUT_FACTOR);
        ps.tw_h = ntt_split(k), ps.cs_h = ntt_split(k);
        ps.total_tiles = (uint64_t)batch << (k - ps.t);
        ps.factor_in = ntt_factor_in(flags);
        ps.factor_out = ntt_factor_out(k, flags);
        L += ps.t;
    }
    return pl.passes;
}
inline uint64_t ntt_groups(const NttPass& ps, uint32_t T) {
    const uint32_t c = T - ps.t;
    return (ps.total_tiles + ((1ull << c) - 1ull)) >> c;
}

#if defined(__HIPCC__) && !defined(NTT_NO_KERNELS)  // (tools/ntt_check.cpp is a host-only build: no kernels, no device code object)
template <uint32_t T>
__global__ void __launch_bounds__(1u << (T - 1)) k_ntt_pass(const NttPass ps, const NttTables tb, const uint32_t* src, uint32_t* dst) {
    __shared__ uint32_t lds[9u << T];
    constexpr uint32_t H = 1u << (T - 1);
    const uint32_t tid = threadIdx.x;
    const uint64_t group = blockIdx.x;
    ntt_phase_load<T>(ps, tb, src, group, tid, lds);
    ntt_phase_load<T>(ps, tb, src, group, tid + H, lds);
    __syncthreads();
    for (uint32_t s = 0; s < ps.t; s++) {
        ntt_phase_butterfly<T>(ps, tb, s, tid, lds);
        __syncthreads();
    }
    ntt_phase_store<T>(ps, tb, dst, group, tid, lds);
    ntt_phase_store<T>(ps, tb, dst, group, tid + H, lds);
}
__global__ void __launch_bounds__(256) k_ntt_pow_table(const fr base, const fr scale, uint32_t count, uint32_t* out) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count) ntt_pow_entry(base, scale, e, out);
}
__global__ void __launch_bounds__(256) k_fr_mul_sub_scale(const uint32_t* a, const uint32_t* b, const uint32_t* c, const fr pre, const fr post,
                                                          uint32_t* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ntt_mul_sub_scale_one(a + i * 8, b + i * 8, c ? c + i * 8 : nullptr, pre, post, out + i * 8);
}
#endif

}  // namespace nttk
