// HOST run of the scalar field Fr (gpu-acceleration_amd/csrc/fr_bn254.hpp is __host__ __device__) on RAW limb records with -DFP_BOUNDS_CHECK, which
// turns every limb-range assumption of the lazily reduced field (normalised operands, pad >= subtrahend limb, limb + carry < 2^32, value < 2^261, no
// 64-bit column overflow, fr_reduce_lt2r's input < 2r) into an abort.  It reads the launches tools/fr_ops_cases.py writes -- the operand classes
// tests/test_gpu_22_fr_ops.py hands the device through msm_test_fr_raw_op -- runs the one function per element exactly as msmk::k_test_fr_raw does
// and writes the limbs it got: that no assertion fires is the proof that those classes are legal, and tests/test_fr_ops_cpu.py compares every limb
// with the Python integer model.
//
//   hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --cuda-host-only tools/fr_bounds_check.cpp -o fr_bounds_check
//   fr_bounds_check in.bin out.bin
// in.bin: 32-bit little-endian words, launch after launch: op (MSM_OP_FR_RAW_* of include/msm_hip_testhooks.h), n, a (n x 9 words), b (n x 9 words,
// ignored where the operation reads none).  out.bin: n x 9 words per launch, in order.  The last line of stdout reports the counts.
#include <cstdio>
#include <vector>

#include "../gpu-acceleration_amd/csrc/fr_bn254.hpp"
#include "../include/msm_hip_testhooks.h"

using namespace bn254;

static fr load9(const uint32_t* p) {
    fr x;
    for (int k = 0; k < 9; k++) x.v[k] = p[k];
    return x;
}

// one element, as k_test_fr_raw<OP> computes it
static bool run_one(uint32_t op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    fr r = fr_zero();
    uint32_t w[8];
    bool words_out = false;
    switch (op) {
        case MSM_OP_FR_RAW_MUL: r = fr_mul(load9(a), load9(b)); break;
        case MSM_OP_FR_RAW_ADD: r = fr_add(load9(a), load9(b)); break;
        case MSM_OP_FR_RAW_SUB2: r = fr_sub<2>(load9(a), load9(b)); break;
        case MSM_OP_FR_RAW_SUB3: r = fr_sub<3>(load9(a), load9(b)); break;
        case MSM_OP_FR_RAW_SUB7: r = fr_sub<7>(load9(a), load9(b)); break;
        case MSM_OP_FR_RAW_SUB8: r = fr_sub<8>(load9(a), load9(b)); break;
        case MSM_OP_FR_RAW_NORMALIZE: r = fr_normalize(load9(a)); break;
        case MSM_OP_FR_RAW_REDUCE_LT2R: r = fr_reduce_lt2r(load9(a)); break;
        case MSM_OP_FR_RAW_CANONICAL: r = fr_canonical(load9(a)); break;
        case MSM_OP_FR_RAW_UNPACK: r = fr_unpack(a); break;
        case MSM_OP_FR_RAW_PACK: fr_pack(w, load9(a)), words_out = true; break;
        case MSM_OP_FR_RAW_FROM_STD: r = fr_from_std(a); break;
        case MSM_OP_FR_RAW_TO_STD: fr_to_std(w, load9(a)), words_out = true; break;
        case MSM_OP_FR_RAW_POW_U32: r = fr_pow_u32(load9(a), b[0]); break;
        case MSM_OP_FR_RAW_INV: r = fr_inv(load9(a)); break;
        default: return false;
    }
    for (int k = 0; k < 8; k++) out[k] = words_out ? w[k] : r.v[k];
    out[8] = words_out ? 0u : r.v[8];
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    std::vector<uint32_t> in;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t buf[4096];
    size_t got;
    while ((got = std::fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
    std::vector<uint32_t> out;
    unsigned long launches = 0, elements = 0;
    size_t pos = 0;
    while (pos < in.size()) {
        if (in.size() - pos < 2) return 2;
        const uint32_t op = in[pos];
        const size_t n = in[pos + 1];
        pos += 2;
        if (n == 0 || (in.size() - pos) / 18 < n) {
            std::fprintf(stderr, "launch %lu: truncated\n", launches);
            return 2;
        }
        const uint32_t *a = &in[pos], *b = &in[pos + n * 9];
        const size_t at = out.size();
        out.resize(at + n * 9);
        for (size_t i = 0; i < n; i++)
            if (!run_one(op, a + i * 9, b + i * 9, &out[at + i * 9])) {
                std::fprintf(stderr, "launch %lu: unknown op %u\n", launches, op);
                return 2;
            }
        pos += n * 18;
        launches++, elements += n;
    }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    std::printf("%lu launches, %lu elements, no bound violated\n", launches, elements);
    return 0;
}
