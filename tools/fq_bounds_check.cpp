// HOST run of the base field Fq and of Fq2 (gpu-acceleration_amd/csrc/fp_bn254.hpp and fp2_bn254.hpp are __host__ __device__) on RAW limb records
// with -DFP_BOUNDS_CHECK, which turns every limb-range assumption of the lazily reduced field (pad >= subtrahend limb, limb + carry < 2^32, value
// < 2^261, no 64-bit column overflow, a normalised result of fp_mul / fp_sqr / fp_mul_add, fp_reduce_lt2p's input < 2p, fp_pack's < 2^256) into an
// abort.  It reads the launches tools/fq_ops_cases.py writes -- the operand classes tests/test_gpu_24_fq_ops.py hands the device through
// msm_test_fq_raw_op / msm_test_fq2_raw_op -- runs every element through fqraw::fq_eval / fq2_eval, THE function the hooks' kernels call
// (csrc/msm_testhooks_fq_raw.hpp), and writes the limbs it got: that no assertion fires is the proof that those classes are legal, and
// tests/test_fq_ops_cpu.py compares every limb with the Python integer model.
//
//   hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --cuda-host-only tools/fq_bounds_check.cpp -o fq_bounds_check
//   fq_bounds_check in.bin out.bin
// in.bin: 32-bit little-endian words, launch after launch: field (1 = Fq, 2 = Fq2), op (kind | K << 8, MSM_OP_FQ_RAW_* / MSM_OP_FQ2_RAW_* of
// include/msm_hip_testhooks.h), n, then n elements of the operation's words.  out.bin: n x 9 (Fq) or n x 18 (Fq2) words per launch, in order.
// The last line of stdout reports the counts.
#include <cstdio>
#include <vector>

#include "../gpu-acceleration_amd/csrc/msm_testhooks_fq_raw.hpp"

// one launch; false: an operation that is not instantiated
static bool run_launch(uint32_t field, uint32_t op, const uint32_t* in, uint32_t* out, size_t n, size_t in_words) {
#define FQ_CASE(KIND, K)                                                                                      \
    case (KIND) | ((uint32_t)(K) << 8):                                                                       \
        for (size_t i = 0; i < n; i++) fqraw::fq_eval<KIND, K>(in + i * in_words, out + i * 9);               \
        return true;
#define FQ2_CASE(KIND, K)                                                                                     \
    case (KIND) | ((uint32_t)(K) << 8):                                                                       \
        for (size_t i = 0; i < n; i++) fqraw::fq2_eval<KIND, K>(in + i * in_words, out + i * 18);             \
        return true;
    if (field == 1) {
        switch (op) { MSM_FQ_RAW_OPS(FQ_CASE) }
    } else {
        switch (op) { MSM_FQ2_RAW_OPS(FQ2_CASE) }
    }
#undef FQ_CASE
#undef FQ2_CASE
    return false;
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
        if (in.size() - pos < 3) return 2;
        const uint32_t field = in[pos], op = in[pos + 1];
        const size_t n = in[pos + 2];
        pos += 3;
        const size_t in_words = field == 1 ? (size_t)fqraw::fq_arity(op & 0xFFu) * 9 : field == 2 ? (size_t)fqraw::fq2_words(op & 0xFFu) : 0;
        if (in_words == 0) {
            std::fprintf(stderr, "launch %lu: unknown field %u / op %u\n", launches, field, op);
            return 2;
        }
        if (n == 0 || (in.size() - pos) / in_words < n) {
            std::fprintf(stderr, "launch %lu: truncated\n", launches);
            return 2;
        }
        const size_t at = out.size(), out_words = field == 1 ? 9 : 18;
        out.resize(at + n * out_words);
        if (!run_launch(field, op, &in[pos], &out[at], n, in_words)) {
            std::fprintf(stderr, "launch %lu: op %u (kind %u, K %u) of field %u is not instantiated\n", launches, op, op & 0xFFu, op >> 8, field);
            return 2;
        }
        pos += n * in_words;
        launches++, elements += n;
    }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    std::printf("%lu launches, %lu elements, no bound violated\n", launches, elements);
    return 0;
}
