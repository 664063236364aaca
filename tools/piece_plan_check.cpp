// tools/piece_plan_check.cpp -- the piece rule of csrc/msm_planner.hpp (plain C++, host-callable) evaluated over a sweep, one result per line, for
// tests/test_g1_msm_cases_cpu.py to compare with the Python transcription of tools/msm_cases_common.py:
//   "P pairs mean total_buckets forced pmax psplit"   msmplan::make_piece_plan
//   "M pmax entries nonempty result"                  msmplan::effective_pmax
//   "S psplit shift entries result"                   msmplan::effective_psplit
// Build: c++ -O2 -std=c++17 tools/piece_plan_check.cpp -o piece_plan_check
#include <cstdio>
#include <cstdint>
#include <vector>

#include "../gpu-acceleration_amd/csrc/msm_planner.hpp"

int main() {
    // sizes around every threshold of the three functions: powers of two and their neighbours, squares and their neighbours (floor(2 sqrt(mean)))
    std::vector<uint64_t> vals = {0, 1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 24, 25, 26, 31, 32, 33, 35, 36, 37, 63, 64, 65, 99, 100, 101, 127, 128, 129, 130, 255, 256,
                                  257, 511, 512, 513, 1000, 1023, 1024, 1025, 1100, 2047, 2048, 4095, 4096, 4097, 65535, 65536, 65537};
    for (int b = 17; b <= 31; b++)
        for (int64_t d = -1; d <= 1; d++) vals.push_back(((uint64_t)1 << b) + d);
    vals.push_back(99000), vals.push_back(105600), vals.push_back(3 * 131072 + 5), vals.push_back(0xFFFFFFFFull);
    const uint32_t forced[] = {0, 1, 2, 3, 7, 26, 1024, 2000};
    const uint64_t tbs[] = {256, 8192, 131071, 131072, 1048576};
    const uint64_t means[] = {0, 1, 3, 4, 8, 12, 16, 25, 63, 64, 65, 100, 255, 256, 900, 1000, 1024, 5000};
    for (uint64_t pairs : vals)
        for (uint64_t mean : means)
            for (uint64_t tb : tbs)
                for (uint32_t f : forced) {
                    if (pairs == 0) continue;
                    const msmplan::piece_plan p = msmplan::make_piece_plan((size_t)pairs, (size_t)mean, (size_t)tb, f);
                    printf("P %llu %llu %llu %u %u %u\n", (unsigned long long)pairs, (unsigned long long)mean, (unsigned long long)tb, f, p.pmax, p.psplit);
                }
    const uint32_t pmaxes[] = {1, 8, 9, 16, 32, 72, 1024};
    for (uint32_t pmax : pmaxes)
        for (uint64_t entries : vals)
            for (uint64_t nonempty : vals) {
                if (entries > 0xFFFFFFFFull || nonempty > 0xFFFFFFFFull) continue;
                printf("M %u %llu %llu %u\n", pmax, (unsigned long long)entries, (unsigned long long)nonempty,
                       msmplan::effective_pmax(pmax, (uint32_t)entries, (uint32_t)nonempty));
            }
    // every mean from 0 to 70000 once (the exact floor(2 sqrt(mean)) through sqrtf and its correction loops)
    for (uint32_t mean = 0; mean <= 70000; mean++) printf("M %u %u %u %u\n", 8u, mean * 3u, 3u, msmplan::effective_pmax(8u, mean * 3u, 3u));
    const uint32_t psplits[] = {1, 7, 8, 16, 32, 64, 128, 1024};
    const uint32_t shifts[] = {0, 1, 10, 15, 16, 17, 18, 24};
    for (uint32_t ps : psplits)
        for (uint32_t sh : shifts)
            for (uint64_t entries : vals) {
                if (entries > 0xFFFFFFFFull) continue;
                printf("S %u %u %llu %u\n", ps, sh, (unsigned long long)entries, msmplan::effective_psplit(ps, sh, (uint32_t)entries));
            }
    return 0;
}
