// CPU run of the arithmetic behind msm_bn254_g2_decompress / _validate (gpu-acceleration_amd/csrc/g2_points_bn254.hpp is __host__ __device__):
// the kernels' own root-and-sign routine, curve equation and subgroup test, compiled for the host with -DFP_BOUNDS_CHECK, which turns every
// limb-range assumption of the lazily reduced field (pad >= subtrahend limb, no column overflow, value < 2^261) into an abort.
// tests/test_g2_points_cpu.py feeds it and compares every answer with the independent Python law.
//
//   hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --offload-arch=gfx950 tools/g2_points_check.cpp -o g2_points_check
// stdin, one query per line, numbers as 64 hex digits (standard form, < p):
//   S a0 a1 want        -> "S ok y0 y1"      square root of a0 + a1 u with the sign asked for (want = 1: the larger of (y, -y)); ok = 0: no square
//   P x0 x1 y0 y1       -> "P curve sub"     y^2 == x^3 + b ?   and, for points on the twist, [r]P == O ?  (sub = 0 when curve = 0)
#include <cstdio>
#include <cstring>

#include "../gpu-acceleration_amd/csrc/g2_points_bn254.hpp"

using namespace bn254;

static bool parse(const char* h, uint32_t w[8]) {
    if (std::strlen(h) != 64) return false;
    for (int i = 0; i < 8; i++) w[i] = 0;
    for (int i = 0; i < 64; i++) {
        const char ch = h[i];
        uint32_t d;
        if (ch >= '0' && ch <= '9') d = (uint32_t)(ch - '0');
        else if (ch >= 'a' && ch <= 'f') d = (uint32_t)(ch - 'a' + 10);
        else return false;
        const int bit = 4 * (63 - i);
        w[bit / 32] |= d << (bit % 32);
    }
    return words_lt_p(w);
}
static void print_fp(const fp& a) {
    uint32_t w[8];
    fp_to_std(w, a);
    for (int i = 7; i >= 0; i--) std::printf("%08x", w[i]);
}

int main() {
    char line[600], h[4][130];
    unsigned long queries = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        uint32_t w[4][8];
        int want = 0;
        if (line[0] == 'S' && std::sscanf(line + 1, "%129s %129s %d", h[0], h[1], &want) == 3 && parse(h[0], w[0]) && parse(h[1], w[1])) {
            fp2 y = fp2_zero();
            const bool ok = g2_sqrt_signed(fp2{fp_from_std(w[0]), fp_from_std(w[1])}, want != 0, y);
            if (!ok) y = fp2_zero();
            std::printf("S %d ", ok ? 1 : 0);
            print_fp(y.c0);
            std::printf(" ");
            print_fp(y.c1);
            std::printf("\n");
        } else if (line[0] == 'P' && std::sscanf(line + 1, "%129s %129s %129s %129s", h[0], h[1], h[2], h[3]) == 4 && parse(h[0], w[0]) &&
                   parse(h[1], w[1]) && parse(h[2], w[2]) && parse(h[3], w[3])) {
            fp c[4];
            for (int k = 0; k < 4; k++) c[k] = fp_reduce_lt2p(fp_from_std(w[k]));  // canonical, as the kernels hand them over
            const fp2 x{c[0], c[1]}, y{c[2], c[3]};
            const fp2 rhs = g2_rhs(x), y2 = fp2_sqr<3>(y);
            const bool curve = fp_equal(y2.c0, rhs.c0) && fp_equal(y2.c1, rhs.c1);
            const bool sub = curve && g2_in_subgroup(affine2{x, y});
            std::printf("P %d %d\n", curve ? 1 : 0, sub ? 1 : 0);
        } else {
            std::printf("bad query: %s", line);
            return 2;
        }
        queries++;
    }
    std::printf("%lu queries, no bound violated\n", queries);
    return 0;
}
