// CPU run of the R1CS rows (gpu-acceleration_amd/csrc/r1cs_bn254.hpp is __host__ __device__ where the kernels are concerned): the same upload plan,
// the same per-item and fold routines the kernels run, executed item by item on the host with -DFP_BOUNDS_CHECK, which turns every limb-range
// assumption of the lazily reduced sums into an abort.  tests/test_r1cs_cpu.py feeds it and compares every word with the independent Python
// yardstick (tools/bn254_fr_r1cs_py.py).  It is also the stand-alone program the upload's host code (sort, row cutting, dictionary, layout over
// caller data) runs in under -fsanitize=address,undefined (make -C gpu-acceleration_amd/csrc asan-r1cs).
//
//   hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --cuda-host-only tools/r1cs_check.cpp -o r1cs_check
// stdin, one query per line; files hold little-endian 32-bit words (coefficients: records of 11 words = msm_r1cs_coef_t):
//   E form num_rows num_cols log_n n_coefs flags coefs witness out   what msm_bn254_fr_r1cs_upload + _eval_device compute -> "E ok items folds partials distinct plus minus"
//   P form num_rows num_cols log_n n_coefs coefs                     the plan alone -> "P ok ..." (the fields of msm_r1cs_info_t) or "P error <code> <message>"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define NTT_NO_KERNELS
#include "../gpu-acceleration_amd/csrc/r1cs_bn254.hpp"

using namespace r1csk;

static bool read_file(const char* path, std::vector<uint32_t>& v, size_t words) {
    v.assign(words, 0);
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t got = std::fread(v.data(), 4, words, f);
    std::fclose(f);
    return got == words;
}
static bool write_file(const char* path, const std::vector<uint32_t>& v) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const size_t put = std::fwrite(v.data(), 4, v.size(), f);
    std::fclose(f);
    return put == v.size();
}

// what r1cs_enqueue (msm_r1cs.inc) queues, in its order
static void evaluate(const R1csHost& h, const std::vector<uint32_t>& wit, uint32_t flags, std::vector<uint32_t>& out) {
    const size_t n = (size_t)1 << h.log_n;
    const bool from_ab = flags & R1CS_F_C_FROM_AB;
    out.assign(3 * n * 8, 0xA5A5A5A5u);  // a row nothing writes shows up
    for (uint32_t m = 0; m < (from_ab ? 2u : 3u); m++) {
        const size_t first = h.info.entries[m] ? h.num_rows : 0;
        if (first < n) std::memset(out.data() + (m * n + first) * 8, 0, (n - first) * 32);
    }
    std::vector<uint32_t> partials((size_t)h.info.partial_sums * 8, 0xA5A5A5A5u);
    const R1csView v{h.items.data(), h.group_base.data(), h.entries.data(), h.dict.data(), h.folds.data()};
    const fr post = r1cs_post(flags);
    const uint32_t n_items = from_ab ? h.items01 : (uint32_t)h.items.size(), n_folds = from_ab ? h.folds01 : (uint32_t)h.folds.size();
    for (uint32_t i = 0; i < n_items; i++) r1cs_item(v, i, wit.data(), post, out.data(), partials.data());
    std::vector<uint32_t> sums(9 * R1CS_GROUP);
    for (uint32_t f = 0; f < n_folds; f++) {
        const uint4 fd = h.folds[f];
        for (uint32_t l = 0; l < R1CS_GROUP; l++) ntt_lds_put(sums.data(), l, r1cs_fold_lane(partials.data(), fd.y, fd.z, l));
        r1cs_fold_finish(sums.data(), post, out.data() + (size_t)fd.x * 8);
    }
    if (from_ab) {
        const uint32_t form = flags & NTT_F_OUT_MONT ? (NTT_F_IN_MONT | NTT_F_OUT_MONT) : 0u;
        for (size_t i = 0; i < n; i++)
            ntt_mul_sub_scale_one(&out[i * 8], &out[(n + i) * 8], nullptr, ntt_factor_in(form), fr_canonical(fr_one()), &out[(2 * n + i) * 8]);
    }
}

int main() {
    static char line[4096], f[10][600];
    unsigned long queries = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        const int nf = std::sscanf(line, "%599s %599s %599s %599s %599s %599s %599s %599s %599s %599s", f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7],
                                   f[8], f[9]);
        if (nf < 1) continue;
        queries++;
        if ((f[0][0] == 'E' && nf == 10) || (f[0][0] == 'P' && nf == 7)) {
            const bool eval = f[0][0] == 'E';
            const uint32_t form = (uint32_t)std::strtoul(f[1], nullptr, 10), rows = (uint32_t)std::strtoul(f[2], nullptr, 10),
                           cols = (uint32_t)std::strtoul(f[3], nullptr, 10), log_n = (uint32_t)std::strtoul(f[4], nullptr, 10);
            const size_t n_coefs = (size_t)std::strtoul(f[5], nullptr, 10);
            std::vector<uint32_t> cw, wit, out;
            if (!read_file(f[eval ? 7 : 6], cw, n_coefs * 11)) {
                std::printf("bad query: %s", line);
                return 2;
            }
            R1csHost h;
            std::string err;
            const int rc = r1cs_build((const R1csCoef*)cw.data(), n_coefs, form, rows, cols, log_n, eval, h, err);
            if (!eval) {
                if (rc) std::printf("P error %d %s\n", rc, err.c_str());
                else
                    std::printf("P ok %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)h.info.entries[0],
                                (unsigned long long)h.info.entries[1], (unsigned long long)h.info.entries[2], (unsigned long long)h.info.rows_with_entries[0],
                                (unsigned long long)h.info.rows_with_entries[1], (unsigned long long)h.info.rows_with_entries[2],
                                (unsigned long long)h.info.longest_row, (unsigned long long)h.info.plus_one, (unsigned long long)h.info.minus_one,
                                (unsigned long long)h.info.distinct_values, (unsigned long long)h.info.work_items, (unsigned long long)h.info.max_item_len,
                                (unsigned long long)h.info.fold_rows, (unsigned long long)h.info.partial_sums, (unsigned long long)h.info.device_bytes);
                continue;
            }
            const uint32_t flags = (uint32_t)std::strtoul(f[6], nullptr, 10);
            if (rc || log_n > 20 || !read_file(f[8], wit, (size_t)cols * 8)) {
                std::printf("bad query (%s): %s", err.c_str(), line);
                return 2;
            }
            evaluate(h, wit, flags, out);
            if (!write_file(f[9], out)) return 2;
            std::printf("E ok %zu %zu %llu %llu %llu %llu\n", h.items.size(), h.folds.size(), (unsigned long long)h.info.partial_sums,
                        (unsigned long long)h.info.distinct_values, (unsigned long long)h.info.plus_one, (unsigned long long)h.info.minus_one);
        } else {
            std::printf("bad query: %s", line);
            return 2;
        }
    }
    std::printf("%lu queries, no bound violated\n", queries);
    return 0;
}
