// CPU run of the G1 fixed-base batch multiplication (gpu-acceleration_amd/csrc/fixed_base_bn254.hpp is __host__ __device__): the same digit recoding,
// the same window-table routines and the same product-tree batch inversion the kernels run, executed lane by lane and phase by phase on the host
// with -DFP_BOUNDS_CHECK, which turns every limb-range assumption of the lazily reduced field code into an abort.  tests/test_fixed_base_cpu.py
// feeds it and compares every word with the oracle.  Also built under -fsanitize=address,undefined as this stand-alone program
// (make -C gpu-acceleration_amd/csrc asan-fixed-base).
//
//   hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --cuda-host-only tools/fixed_base_check.cpp -o fixed_base_check
// stdin (or the file named as the only argument), one query per line; numbers are hexadecimal integers of up to 256 bits:
//   D c k            the signed digits of k                                    -> "D W d_0 .. d_{W-1}"
//   T c x y          build the window table of the base (x, y), standard form  -> "T W entries"      (what k_fb_window_bases + k_fb_table_level compute)
//   M k              queue a scalar
//   R flags          multiply the queued scalars by the table's base, in groups of FB_GROUP as k_fb_mul does; flags: 2 = the scalars are Fr.0 words,
//                    8 = standard-form output                                  -> one "P inf x y" per scalar
//   I z_0 .. z_m     batch inversion of one group, m < FB_GROUP, 0 = an identity's slot, standard form in and out -> "I f_0 v_0 f_1 v_1 .." (f = flag)
#include <cstdio>
#include <cstring>
#include <iostream>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../gpu-acceleration_amd/csrc/fixed_base_bn254.hpp"

using namespace fbk;

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
static std::string hex(const uint32_t w[8]) {
    char buf[65];
    for (int i = 0; i < 8; i++) std::snprintf(buf + 8 * i, 9, "%08x", w[7 - i]);
    return buf;
}

struct Table {
    uint32_t c = 0, W = 0;
    std::vector<uint32_t> rec;
};

// one group through the tree; live[l] false: the lane holds nothing (an identity)
static void group_inverse(std::vector<uint32_t>& tree, const std::vector<xyzz>& acc, std::vector<fp>& iz) {
    fp zzz[FB_GROUP];
    bool ident[FB_GROUP];
    for (uint32_t l = 0; l < FB_GROUP; l++) zzz[l] = acc[l].zzz, ident[l] = xyzz_is_identity(acc[l]);
    iz.resize(FB_GROUP);
    fb_batch_inverse_host(tree.data(), zzz, ident, iz.data());
}

static void build_table(Table& t, uint32_t c, const uint32_t x[8], const uint32_t y[8]) {
    FbPlan p;
    fb_plan(c, p);
    t.c = p.window_bits, t.W = p.num_windows;
    const size_t entries = (size_t)p.table_entries;
    t.rec.assign(entries * FB_REC_WORDS, 0xA5A5A5A5u);
    std::vector<uint32_t> tree(FB_TREE_WORDS);
    std::vector<xyzz> acc(FB_GROUP);
    std::vector<size_t> dst(FB_GROUP);
    std::vector<fp> iz;
    const affine base{fp_from_std(x), fp_from_std(y)};
    for (uint32_t j = 0; j < FB_GROUP; j++) acc[j] = j < t.W ? fb_window_base(base, t.c, j) : xyzz_identity();  // k_fb_window_bases
    group_inverse(tree, acc, iz);
    for (uint32_t j = 0; j < t.W; j++) fb_store_record(t.rec.data() + fb_table_index(j, 1, t.c) * FB_REC_WORDS, fb_to_affine(acc[j], iz[j]));
    for (uint32_t L = 1; L < t.c; L++) {  // k_fb_table_level, launch by launch
        const uint32_t n = fb_level_entries(t.W, L);
        for (uint32_t g = 0; g < n; g += FB_GROUP) {
            for (uint32_t l = 0; l < FB_GROUP; l++) acc[l] = g + l < n ? fb_table_step(t.rec.data(), t.c, L, g + l, dst[l]) : xyzz_identity();
            group_inverse(tree, acc, iz);
            for (uint32_t l = 0; l < FB_GROUP && g + l < n; l++) fb_store_record(t.rec.data() + dst[l] * FB_REC_WORDS, fb_to_affine(acc[l], iz[l]));
        }
    }
    for (uint32_t w : t.rec)
        if (w == 0xA5A5A5A5u) std::abort();  // (a record no level wrote; a coordinate word with this pattern is as good as impossible)
}

static void run(const Table& t, const std::vector<std::vector<uint32_t>>& ks, uint32_t flags) {  // k_fb_mul
    std::vector<uint32_t> tree(FB_TREE_WORDS);
    std::vector<xyzz> acc(FB_GROUP);
    std::vector<fp> iz;
    alignas(16) uint32_t xy[16];
    for (size_t g = 0; g < ks.size(); g += FB_GROUP) {
        for (uint32_t l = 0; l < FB_GROUP; l++) {
            acc[l] = xyzz_identity();
            if (g + l >= ks.size()) continue;
            uint32_t k[8];
            std::memcpy(k, ks[g + l].data(), 32);
            if (flags & FB_F_IN_MONT) fb_scalar_from_mont(k);
            acc[l] = fb_mul_point(t.rec.data(), t.c, t.W, k);
        }
        group_inverse(tree, acc, iz);
        for (uint32_t l = 0; l < FB_GROUP && g + l < ks.size(); l++) {
            uint8_t inf;
            fb_store_output(xy, &inf, acc[l], iz[l], xyzz_is_identity(acc[l]), (flags & FB_F_OUT_STD) != 0);
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
    Table table;
    std::vector<std::vector<uint32_t>> queued;
    std::string line;
    unsigned long queries = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string op;
        if (!(ls >> op)) continue;
        queries++;
        std::vector<std::string> f;
        for (std::string s; ls >> s;) f.push_back(s);
        uint32_t a[8], b[8];
        if (op == "D" && f.size() == 2 && parse_hex(f[1], a)) {
            FbPlan p;
            if (!fb_plan((uint32_t)std::stoul(f[0]), p)) return 2;
            uint32_t carry = 0;
            std::printf("D %u", p.num_windows);
            for (uint32_t j = 0; j < p.num_windows; j++) std::printf(" %d", (int)fb_next_digit(a, p.window_bits, carry));
            std::printf("\n");
            if (carry) return 3;
        } else if (op == "T" && f.size() == 3 && parse_hex(f[1], a) && parse_hex(f[2], b)) {
            build_table(table, (uint32_t)std::stoul(f[0]), a, b);
            std::printf("T %u %zu\n", table.W, ((size_t)table.W) << (table.c - 1));
        } else if (op == "M" && f.size() == 1 && parse_hex(f[0], a)) {
            queued.emplace_back(a, a + 8);
        } else if (op == "R" && f.size() == 1 && table.c) {
            run(table, queued, (uint32_t)std::stoul(f[0]));
            queued.clear();
        } else if (op == "I" && !f.empty() && f.size() <= FB_GROUP) {
            std::vector<uint32_t> tree(FB_TREE_WORDS);
            fp zzz[FB_GROUP], iz[FB_GROUP];
            bool ident[FB_GROUP];
            for (uint32_t l = 0; l < FB_GROUP; l++) {
                ident[l] = true, zzz[l] = fp_zero();
                if (l >= f.size()) continue;
                if (!parse_hex(f[l], a)) return 2;
                zzz[l] = fp_from_std(a);
                ident[l] = fp_is_zero_lt2p(zzz[l]);
            }
            fb_batch_inverse_host(tree.data(), zzz, ident, iz);
            std::printf("I");
            for (uint32_t l = 0; l < f.size(); l++) {
                fp_to_std(a, ident[l] ? fp_zero() : iz[l]);
                std::printf(" %u %s", ident[l] ? 1u : 0u, hex(a).c_str());
            }
            std::printf("\n");
        } else {
            std::printf("bad query: %s\n", line.c_str());
            return 2;
        }
    }
    std::printf("%lu queries, no bound violated\n", queries);
    return 0;
}
