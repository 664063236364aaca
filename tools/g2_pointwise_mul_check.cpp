// CPU run of the G2 element-wise scalar multiplication (gpu-acceleration_amd/csrc/g2_pointwise_mul_bn254.hpp is __host__ __device__): the same
// scalar reduction, split, table over Fq2 and joint ladder the kernel runs, executed lane by lane and phase by phase on the host in
// k_pm2_mul's order, the two shared inversions of the norms through fb_batch_inverse_host, with -DFP_BOUNDS_CHECK, which turns every
// limb-range assumption of the lazily reduced field code into an abort.  tests/test_g2_pointwise_mul_cpu.py feeds it and compares every word
// with Python integers and the independent Python G2 law.  Also built under -fsanitize=address,undefined as this stand-alone program
// (make -C gpu-acceleration_amd/csrc asan-g2-pointwise).
//
//   hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --cuda-host-only tools/g2_pointwise_mul_check.cpp -o g2_pointwise_mul_check
// stdin (or the file named as the only argument), one query per line; numbers are hexadecimal integers of up to 256 bits, the WORDS as the call
// reads them; a point is four numbers x.c0 x.c1 y.c0 y.c1; flags: 2 = the scalars are Fr.0 words, 8 = standard-form output, 16 = standard-form
// bases:
//   S flags k          the halves of the scalar                                 -> "S neg1 |k1| neg2 |k2|"
//   T flags point k    the table of one point and one scalar                     -> "T P1 P2 S" (twelve numbers, standard form)
//   B inf point        queue a base (inf: 1 = flagged)
//   M k                queue a scalar
//   R flags            out[i] = k_i * Q_i over the queue, in groups of FB_GROUP as k_pm2_mul<false> does   -> one "P inf point" per point
//   U flags k          out[i] = k * Q_i over the queued bases (k in standard form, split by pm_split_host) as k_pm2_mul<true> does -> likewise
#include <cstdio>
#include <cstring>
#include <iostream>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../gpu-acceleration_amd/csrc/g2_pointwise_mul_bn254.hpp"

using namespace pmk;

static bool parse_hex(const std::string& s, uint32_t w[8]) {
    std::memset(w, 0, 32);
    if (s.empty() || s.size() > 64) return false;
    for (size_t i = 0; i < s.size(); i++) {
        const char ch = s[s.size() - 1 - i];
        uint32_t v;
        if (ch >= '0' && ch <= '9') v = (uint32_t)(ch - '0');
        else if (ch >= 'a' && ch <= 'f') v = (uint32_t)(ch - 'a' + 10);
        else if (ch >= 'A' && ch <= 'F') v = (uint32_t)(ch - 'A' + 10);
        else return false;
        w[i / 8] |= v << (4 * (i % 8));
    }
    return true;
}
static std::string hex(const uint32_t* w, int words = 8) {
    char buf[65];
    for (int i = 0; i < words; i++) std::snprintf(buf + 8 * i, 9, "%08x", w[words - 1 - i]);
    return buf;
}
static std::string std_hex(const fp& v) {
    uint32_t w[8];
    fp_to_std(w, v);
    return hex(w);
}
static std::string std_hex2(const fp2& x, const fp2& y) { return std_hex(x.c0) + " " + std_hex(x.c1) + " " + std_hex(y.c0) + " " + std_hex(y.c1); }

struct Base {
    alignas(16) uint32_t xy[32];
    bool inf;
};
struct Scalar {
    alignas(16) uint32_t k[8];
};
static bool parse_point(const std::vector<std::string>& f, size_t at, uint32_t xy[32]) {
    for (int c = 0; c < 4; c++)
        if (!parse_hex(f[at + c], xy + 8 * c)) return false;
    return true;
}

// one workgroup of k_pm2_mul<UNIFORM> after another
template <bool UNIFORM>
static void run(const std::vector<Base>& bases, const std::vector<Scalar>& ks, const PmSplit& uni, uint32_t flags) {
    std::vector<uint32_t> tree(FB_TREE_WORDS);
    std::vector<Pm2Lane> lane(FB_GROUP);
    std::vector<xyzz2> acc(FB_GROUP);
    fp den[FB_GROUP], inv[FB_GROUP];
    bool idle[FB_GROUP], skip[FB_GROUP];
    alignas(16) uint32_t xy[32];
    const size_t n = bases.size();
    for (size_t g = 0; g < n; g += FB_GROUP) {
        for (uint32_t l = 0; l < FB_GROUP; l++) {
            idle[l] = g + l >= n || bases[g + l].inf;
            den[l] = fp_one();
            bool x_zero = false;
            lane[l].s = uni;
            if (!idle[l]) den[l] = pm2_lane_begin<UNIFORM>(lane[l], bases[g + l].xy, UNIFORM ? nullptr : ks[g + l].k, flags, x_zero);
            skip[l] = idle[l] || x_zero;
        }
        fb_batch_inverse_host(tree.data(), den, skip, inv);
        for (uint32_t l = 0; l < FB_GROUP; l++) {
            acc[l] = idle[l] ? xyzz2_identity() : pm2_lane_finish(lane[l], inv[l]);
            skip[l] = pm2_is_identity(acc[l]);
            den[l] = skip[l] ? fp_one() : pm2_out_norm(acc[l]);
        }
        fb_batch_inverse_host(tree.data(), den, skip, inv);
        for (uint32_t l = 0; l < FB_GROUP && g + l < n; l++) {
            uint8_t inf;
            pm2_store_output(xy, &inf, acc[l], inv[l], skip[l], (flags & PM_F_OUT_STD) != 0);
            std::printf("P %u %s %s %s %s\n", (unsigned)inf, hex(xy).c_str(), hex(xy + 8).c_str(), hex(xy + 16).c_str(), hex(xy + 24).c_str());
        }
    }
}

int main(int argc, char** argv) {
    std::ifstream file;
    if (argc > 1) {
        file.open(argv[1]);
        if (!file) return 2;
    }
    std::istream& in = argc > 1 ? (std::istream&)file : std::cin;
    std::vector<Base> bases;
    std::vector<Scalar> scalars;
    std::string line;
    unsigned long queries = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string op;
        if (!(ls >> op)) continue;
        queries++;
        std::vector<std::string> f;
        for (std::string s; ls >> s;) f.push_back(s);
        uint32_t k[8];
        Base p;
        if (op == "S" && f.size() == 2 && parse_hex(f[1], k)) {
            pm_scalar_canonical(k, (std::stoul(f[0]) & PM_F_IN_MONT) != 0);
            const PmSplit s = pm_split(k);
            std::printf("S %u %s %u %s\n", s.neg1, hex(s.k1, 4).c_str(), s.neg2, hex(s.k2, 4).c_str());
        } else if (op == "T" && f.size() == 6 && parse_point(f, 1, p.xy) && parse_hex(f[5], k)) {
            const uint32_t flags = (uint32_t)std::stoul(f[0]);
            Scalar s;
            std::memcpy(s.k, k, 32);
            std::vector<uint32_t> tree(FB_TREE_WORDS);
            fp den[FB_GROUP], inv[FB_GROUP];
            bool skip[FB_GROUP];
            for (uint32_t l = 0; l < FB_GROUP; l++) den[l] = fp_one(), skip[l] = true;
            Pm2Lane t;
            den[0] = pm2_lane_begin<false>(t, p.xy, s.k, flags, skip[0]);
            fb_batch_inverse_host(tree.data(), den, skip, inv);
            pm2_table_finish(t, inv[0]);
            const affine2 p1 = pm2_select(t, 1), p2 = pm2_select(t, 2), ps = pm2_select(t, 3);
            std::printf("T %s %s %s\n", std_hex2(p1.x, p1.y).c_str(), std_hex2(p2.x, p2.y).c_str(), std_hex2(ps.x, ps.y).c_str());
        } else if (op == "B" && f.size() == 5 && parse_point(f, 1, p.xy)) {
            p.inf = f[0] != "0";
            bases.push_back(p);
        } else if (op == "M" && f.size() == 1 && parse_hex(f[0], k)) {
            Scalar s;
            std::memcpy(s.k, k, 32);
            scalars.push_back(s);
        } else if (op == "R" && f.size() == 1 && bases.size() == scalars.size()) {
            run<false>(bases, scalars, PmSplit{}, (uint32_t)std::stoul(f[0]));
            bases.clear(), scalars.clear();
        } else if (op == "U" && f.size() == 2 && parse_hex(f[1], k)) {
            run<true>(bases, scalars, pm_split_host(k), (uint32_t)std::stoul(f[0]));
            bases.clear(), scalars.clear();
        } else {
            std::printf("bad query: %s\n", line.c_str());
            return 2;
        }
    }
    std::printf("%lu queries, no bound violated\n", queries);
    return 0;
}
