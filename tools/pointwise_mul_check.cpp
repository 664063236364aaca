// CPU run of the G1 element-wise scalar multiplication (gpu-acceleration_amd/csrc/pointwise_mul_bn254.hpp is __host__ __device__): the same
// scalar reduction, split, three-entry table and joint ladder the kernel runs, executed lane by lane and phase by phase on the host in
// k_pm_mul's order, the two shared inversions through fb_batch_inverse_host, with -DFP_BOUNDS_CHECK, which turns every limb-range assumption of
// the lazily reduced field code into an abort.  tests/test_pointwise_mul_cpu.py feeds it and compares every word with Python integers and the
// oracle.  Also built under -fsanitize=address,undefined as this stand-alone program (make -C gpu-acceleration_amd/csrc asan-pointwise).
//
//   hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --cuda-host-only tools/pointwise_mul_check.cpp -o pointwise_mul_check
// stdin (or the file named as the only argument), one query per line; numbers are hexadecimal integers of up to 256 bits, the WORDS as the call
// reads them; flags: 2 = the scalars are Fr.0 words, 8 = standard-form output, 16 = standard-form bases:
//   S flags k        the halves of the scalar                                   -> "S neg1 |k1| neg2 |k2|"
//   T flags x y k    the table of one point and one scalar                       -> "T x1 y1 x2 y2 xs ys" (P1, P2, S in standard form)
//   B inf x y        queue a base (inf: 1 = flagged)
//   M k              queue a scalar
//   R flags          out[i] = k_i * P_i over the queue, in groups of FB_GROUP as k_pm_mul<false> does   -> one "P inf x y" per point
//   U flags k        out[i] = k * P_i over the queued bases (k in standard form, split by pm_split_host) as k_pm_mul<true> does -> likewise
#include <cstdio>
#include <cstring>
#include <iostream>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../gpu-acceleration_amd/csrc/pointwise_mul_bn254.hpp"

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

struct Base {
    alignas(16) uint32_t xy[16];
    bool inf;
};
struct Scalar {
    alignas(16) uint32_t k[8];
};

// one workgroup of k_pm_mul<UNIFORM> after another
template <bool UNIFORM>
static void run(const std::vector<Base>& bases, const std::vector<Scalar>& ks, const PmSplit& uni, uint32_t flags) {
    std::vector<uint32_t> tree(FB_TREE_WORDS);
    std::vector<PmLane> lane(FB_GROUP);
    std::vector<xyzz> acc(FB_GROUP);
    fp den[FB_GROUP], inv[FB_GROUP];
    bool idle[FB_GROUP], skip[FB_GROUP];
    alignas(16) uint32_t xy[16];
    const size_t n = bases.size();
    for (size_t g = 0; g < n; g += FB_GROUP) {
        for (uint32_t l = 0; l < FB_GROUP; l++) {
            idle[l] = g + l >= n || bases[g + l].inf;
            den[l] = fp_one();
            bool x_zero = false;
            lane[l].s = uni;
            if (!idle[l]) den[l] = pm_lane_begin<UNIFORM>(lane[l], bases[g + l].xy, UNIFORM ? nullptr : ks[g + l].k, flags, x_zero);
            skip[l] = idle[l] || x_zero;
        }
        fb_batch_inverse_host(tree.data(), den, skip, inv);
        for (uint32_t l = 0; l < FB_GROUP; l++) {
            acc[l] = idle[l] ? xyzz_identity() : pm_lane_finish(lane[l], inv[l]);
            den[l] = acc[l].zzz;
            skip[l] = pm_is_identity(acc[l]);
        }
        fb_batch_inverse_host(tree.data(), den, skip, inv);
        for (uint32_t l = 0; l < FB_GROUP && g + l < n; l++) {
            uint8_t inf;
            fb_store_output(xy, &inf, acc[l], inv[l], skip[l], (flags & PM_F_OUT_STD) != 0);
            std::printf("P %u %s %s\n", (unsigned)inf, hex(xy).c_str(), hex(xy + 8).c_str());
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
        uint32_t a[8], b[8], k[8];
        if (op == "S" && f.size() == 2 && parse_hex(f[1], k)) {
            pm_scalar_canonical(k, (std::stoul(f[0]) & PM_F_IN_MONT) != 0);
            const PmSplit s = pm_split(k);
            std::printf("S %u %s %u %s\n", s.neg1, hex(s.k1, 4).c_str(), s.neg2, hex(s.k2, 4).c_str());
        } else if (op == "T" && f.size() == 4 && parse_hex(f[1], a) && parse_hex(f[2], b) && parse_hex(f[3], k)) {
            const uint32_t flags = (uint32_t)std::stoul(f[0]);
            Base p;
            Scalar s;
            std::memcpy(p.xy, a, 32), std::memcpy(p.xy + 8, b, 32), std::memcpy(s.k, k, 32);
            std::vector<uint32_t> tree(FB_TREE_WORDS);
            fp den[FB_GROUP], inv[FB_GROUP];
            bool skip[FB_GROUP];
            for (uint32_t l = 0; l < FB_GROUP; l++) den[l] = fp_one(), skip[l] = true;
            PmLane t;
            den[0] = pm_lane_begin<false>(t, p.xy, s.k, flags, skip[0]);
            fb_batch_inverse_host(tree.data(), den, skip, inv);
            pm_table_finish(t, inv[0]);
            std::printf("T %s %s %s %s %s %s\n", std_hex(t.x).c_str(), std_hex(t.y1).c_str(), std_hex(t.bx).c_str(), std_hex(t.y2).c_str(),
                        std_hex(t.sx).c_str(), std_hex(t.sy).c_str());
        } else if (op == "B" && f.size() == 3 && parse_hex(f[1], a) && parse_hex(f[2], b)) {
            Base p;
            std::memcpy(p.xy, a, 32), std::memcpy(p.xy + 8, b, 32);
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
