// msm_kernels_g2_points.hpp -- gfx950 kernels that get BN254 G2 points IN safely: decoding of arkworks' compressed images (one Fq2 square root per
// point), the curve check and the subgroup check [r]P = O (the twist's cofactor 2p - r is not 1), and the curve check of G1 points.  The
// arithmetic -- root and sign, psi, the subgroup relation, with its value bounds -- is g2_points_bn254.hpp.
//
//   k_g2_decompress<SUB>  n x 64-byte images -> n x 32 arkworks Montgomery words (x.c0 x.c1 y.c0 y.c1) + n infinity bytes; SUB: + the subgroup test
//   k_g2_validate         n x 32 caller words (either form) [+ infinity mask]: range, curve, subgroup
//   k_g1_validate         n x 16 caller words (either form) [+ infinity mask]: range, curve (G1's cofactor is 1)
//   k_g2_test_sqrt        (hooks build) the root-and-sign routine on arbitrary Fq2 values
// One thread per point.  A failing point reports atomicMin(first_bad, index << 2 | reason): the host reads ONE word and knows the lowest failing
// index and why it failed (G2P_DECODE / G2P_CURVE / G2P_SUBGROUP; a point failing for two reasons reports the first it meets).
// The header needs nothing of the MSM kernels: tools/g2_points_resource_check.hip compiles it alone and tests/test_g2_points_cpu.py asserts from
// the compiler's resource remarks that no kernel here uses scratch memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "g2_points_bn254.hpp"

namespace msmk {
using namespace bn254;

// 8 packed words as two 16-byte accesses (p 16-byte aligned)
__device__ __forceinline__ void g2p_load8(uint32_t w[8], const uint32_t* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
}
__device__ __forceinline__ void g2p_store8(uint32_t* p, const uint32_t w[8]) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

constexpr uint32_t G2P_DECODE = 0, G2P_CURVE = 1, G2P_SUBGROUP = 2;  // reasons, in the low two bits of the word at first_bad
constexpr uint32_t G2P_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ void g2p_report(uint32_t* first_bad, uint32_t i, uint32_t reason) { atomicMin(first_bad, (i << 2) | reason); }

__device__ __forceinline__ void store_zero32(uint32_t* o) {
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; k++) g2p_store8(o + 8 * k, zero);
}

// n x 64-byte images (ark-serialize 0.4 G2Affine::serialize_compressed: x.c0, x.c1 little-endian standard form; byte 63 bit 7 = y is the larger of
// (y, -y), bit 6 = infinity) -> out: n x 32 arkworks Montgomery words, inf_out: n bytes.  Invalid or infinite: zero coordinates.
template <bool SUB>
__global__ void __launch_bounds__(256) k_g2_decompress(const uint32_t* __restrict__ rec, uint32_t n, uint32_t* __restrict__ out,
                                                       uint8_t* __restrict__ inf_out, uint32_t* __restrict__ first_bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w0[8], w1[8];
    g2p_load8(w0, rec + (size_t)i * 16);
    g2p_load8(w1, rec + (size_t)i * 16 + 8);
    const uint32_t f_neg = w1[7] >> 31, f_inf = (w1[7] >> 30) & 1u;
    w1[7] &= 0x3FFFFFFFu;
    uint32_t* o = out + (size_t)i * 32;
    if ((f_neg & f_inf) || !words_lt_p(w0) || !words_lt_p(w1)) {
        g2p_report(first_bad, i, G2P_DECODE);
        store_zero32(o);
        inf_out[i] = 0;
        return;
    }
    if (f_inf) {
        store_zero32(o);
        inf_out[i] = 1;
        return;
    }
    const fp2 x{fp_from_std(w0), fp_from_std(w1)};                   // < 1.01
    fp2 y;
    if (!g2_sqrt_signed(g2_rhs(x), f_neg != 0, y)) {
        g2p_report(first_bad, i, G2P_CURVE);
        store_zero32(o);
        inf_out[i] = 0;
        return;
    }
    uint32_t ow[8];
    fp_to_mont256(ow, x.c0), g2p_store8(o, ow);
    fp_to_mont256(ow, x.c1), g2p_store8(o + 8, ow);
    fp_to_mont256(ow, y.c0), g2p_store8(o + 16, ow);
    fp_to_mont256(ow, y.c1), g2p_store8(o + 24, ow);
    inf_out[i] = 0;
    if (SUB) {
        const affine2 p{fp2{fp_reduce_lt2p(x.c0), fp_reduce_lt2p(x.c1)}, y};
        if (!g2_in_subgroup(p)) g2p_report(first_bad, i, G2P_SUBGROUP);
    }
}

// n x 32 caller words (mont_form: arkworks Montgomery words, else standard form), inf nullable (non-zero: infinite, passes everything).
// Always: every component < p and y^2 == x^3 + b; subgroup != 0: [r]P == O as well.
__global__ void __launch_bounds__(256) k_g2_validate(const uint32_t* __restrict__ in, const uint8_t* __restrict__ inf, uint32_t n, uint32_t mont_form,
                                                     uint32_t subgroup, uint32_t* __restrict__ first_bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (inf && inf[i]) return;
    fp c[4];
    bool in_range = true;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t w[8];
        g2p_load8(w, in + (size_t)i * 32 + 8 * k);
        in_range = in_range && words_lt_p(w);
        c[k] = fp_reduce_lt2p(fp_mul(fp_unpack(w), mont_form ? fp_const(FP29_IN_MONT) : fp_const(FP29_IN_STD)));  // (words < 2^256 < 6p: < 1.04) canonical
    }
    const fp2 x{c[0], c[1]}, y{c[2], c[3]};
    const fp2 rhs = g2_rhs(x), y2 = fp2_sqr<3>(y);                   // y.c1 < 2p
    if (!in_range || !fp_equal(y2.c0, rhs.c0) || !fp_equal(y2.c1, rhs.c1)) {
        g2p_report(first_bad, i, G2P_CURVE);
        return;
    }
    if (subgroup && !g2_in_subgroup(affine2{x, y})) g2p_report(first_bad, i, G2P_SUBGROUP);
}

// n x 16 caller words of G1 points: both coordinates < p and y^2 == x^3 + 3 (the cofactor is 1: nothing else to check)
__global__ void __launch_bounds__(256) k_g1_validate(const uint32_t* __restrict__ in, const uint8_t* __restrict__ inf, uint32_t n, uint32_t mont_form,
                                                     uint32_t* __restrict__ first_bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (inf && inf[i]) return;
    uint32_t wx[8], wy[8];
    g2p_load8(wx, in + (size_t)i * 16);
    g2p_load8(wy, in + (size_t)i * 16 + 8);
    const fp cv = mont_form ? fp_const(FP29_IN_MONT) : fp_const(FP29_IN_STD);
    const fp x = fp_mul(fp_unpack(wx), cv), y = fp_mul(fp_unpack(wy), cv);   // < 1.04
    const fp three = fp_add(fp_dbl(fp_one()), fp_one());                       // < 3
    const fp rhs = fp_add(fp_mul(fp_sqr(x), x), three);                        // < 4.02
    if (!words_lt_p(wx) || !words_lt_p(wy) || !fp_equal(fp_sqr(y), rhs)) g2p_report(first_bad, i, G2P_CURVE);
}

#ifdef MSM_HIP_TEST_HOOKS
// the root-and-sign routine on arbitrary Fq2 values: a n x 16 standard-form words (canonical), want n bytes -> out n x 16 standard-form words, ok n bytes
__global__ void __launch_bounds__(256) k_g2_test_sqrt(const uint32_t* __restrict__ a, const uint8_t* __restrict__ want, uint32_t n,
                                                      uint32_t* __restrict__ out, uint8_t* __restrict__ ok) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w0[8], w1[8];
    g2p_load8(w0, a + (size_t)i * 16);
    g2p_load8(w1, a + (size_t)i * 16 + 8);
    const fp2 v{fp_from_std(w0), fp_from_std(w1)};                   // < 1.01
    fp2 y = fp2_zero();
    const bool good = g2_sqrt_signed(v, want[i] != 0, y);
    if (!good) y = fp2_zero();
    fp_to_std(w0, y.c0), g2p_store8(out + (size_t)i * 16, w0);
    fp_to_std(w1, y.c1), g2p_store8(out + (size_t)i * 16 + 8, w1);
    ok[i] = good ? 1 : 0;
}
#endif

}  // namespace msmk
