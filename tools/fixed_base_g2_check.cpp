// CPU run of the G2 fixed-base batch multiplication (gpu-acceleration_amd/csrc/fixed_base_g2_bn254.hpp is __host__ __device__): the table step, the
// product, the norm, the chain inversion and the output conversion the kernels run, executed lane by lane and phase by phase on the host with
// -DFP_BOUNDS_CHECK, which turns every limb-range assumption of the lazily reduced field code into an abort.  tests/test_fixed_base_g2_cpu.py
// feeds it and compares every word with the Python model (tools/fixed_base_g2_cases.py).  Also built under -fsanitize=address,undefined as this
// stand-alone program (make -C gpu-acceleration_amd/csrc asan-fixed-base-g2).
//
//   hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --cuda-host-only tools/fixed_base_g2_check.cpp -o fixed_base_g2_check
// stdin (or the file named as the only argument), one query per line; numbers are hexadecimal integers of up to 256 bits, standard form:
//   T c x0 x1 y0 y1  build the window table of the base                        -> "T W entries"     (k_fb2_window_bases + k_fb2_table_level, group by group)
//   E j d            the record T_j[d] of the table                            -> "E x0 x1 y0 y1"
//   M k              queue a scalar
//   R flags          multiply the queued scalars by the table's base: k_fb2_accumulate into a scratch array, then k_fb2_normalise lane by lane;
//                    flags: 2 = the scalars are Fr.0 words, 8 = standard-form output   -> one "P inf x0 x1 y0 y1" per scalar
//   I G z0 z1 ..     the chains of k_fb2_normalise at inv_group G over the points (1, 1, 1, ZZZ_i = z_(2i) + z_(2i+1) u); 0 0 = an identity
//                    -> "I f_0 v0_0 v1_0 .." per point: the flag and 1 / ZZZ_i (the y the kernel writes; its x = y^2 is checked here)
#include <cstdio>
#include <cstring>
#include <iostream>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../gpu-acceleration_amd/csrc/fixed_base_g2_bn254.hpp"

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
static std::string hex4(const uint32_t* xy) { return hex(xy) + " " + hex(xy + 8) + " " + hex(xy + 16) + " " + hex(xy + 24); }

struct Table {
    uint32_t c = 0, W = 0;
    std::vector<uint32_t> rec;
};

// one group of FB_GROUP lanes through the G1 product tree over the norms, as the table kernels end
static void group_store(std::vector<uint32_t>& tree, const std::vector<xyzz2>& acc, const std::vector<size_t>& dst, uint32_t live, Table& t) {
    fp nrm[FB_GROUP], ni[FB_GROUP];
    bool ident[FB_GROUP];
    for (uint32_t l = 0; l < FB_GROUP; l++) {
        ident[l] = l >= live || xyzz2_is_identity(acc[l]);
        nrm[l] = ident[l] ? fp_one() : fb2_norm(acc[l].zzz);
    }
    fb_batch_inverse_host(tree.data(), nrm, ident, ni);
    for (uint32_t l = 0; l < live; l++)
        if (!ident[l]) fb2_store_record(t.rec.data() + dst[l] * FB2_REC_WORDS, fb2_to_affine(acc[l], fb2_inv_from_norm(acc[l].zzz, ni[l])));
}

static void build_table(Table& t, uint32_t c, const uint32_t std_xy[4][8]) {
    Fb2Plan p;
    fb2_plan(c, p);
    t.c = p.window_bits, t.W = p.num_windows;
    t.rec.assign((size_t)p.table_entries * FB2_REC_WORDS, 0xA5A5A5A5u);
    Fb2Base base;  // Montgomery words, what the host hands the kernel
    for (int k = 0; k < 4; k++) fp_to_mont256(base.w + 8 * k, fp_from_std(std_xy[k]));
    std::vector<uint32_t> tree(FB_TREE_WORDS);
    std::vector<xyzz2> acc(FB_GROUP);
    std::vector<size_t> dst(FB_GROUP);
    for (uint32_t j = 0; j < t.W; j++) acc[j] = fb2_window_base(fb2_base_affine(base.w), t.c, j), dst[j] = fb_table_index(j, 1, t.c);  // k_fb2_window_bases
    group_store(tree, acc, dst, t.W, t);
    for (uint32_t L = 1; L < t.c; L++) {  // k_fb2_table_level, launch by launch
        const uint32_t n = fb_level_entries(t.W, L);
        for (uint32_t g = 0; g < n; g += FB_GROUP) {
            const uint32_t live = n - g < FB_GROUP ? n - g : FB_GROUP;
            for (uint32_t l = 0; l < live; l++) acc[l] = fb2_table_step(t.rec.data(), t.c, L, g + l, dst[l]);
            group_store(tree, acc, dst, live, t);
        }
    }
    for (uint32_t w : t.rec)
        if (w == 0xA5A5A5A5u) std::abort();  // (a record no level wrote; a coordinate word with this pattern is as good as impossible)
}

// k_fb2_normalise over the n points of a scratch array, lane by lane
static void normalise(std::vector<uint32_t>& scratch, size_t stride, size_t n, uint32_t G, bool out_std, std::vector<uint4>& xy, std::vector<uint8_t>& inf) {
    xy.assign(n * FB2_REC_WORDS / 4, make_uint4(0x5A5A5A5Au, 0x5A5A5A5Au, 0x5A5A5A5Au, 0x5A5A5A5Au));  // (16-byte aligned: the routines store uint4)
    inf.assign(n, 0x5A);
    uint32_t* out = reinterpret_cast<uint32_t*>(xy.data());
    for (size_t t = 0; t < fb2_chain_lanes(n, G); t++) {
        const size_t first = fb2_chain_first(t, G);
        if (first >= n) continue;
        const fp inv = fp_inv(fb2_chain_up(scratch.data(), stride, first, G, n));
        fb2_chain_down(scratch.data(), stride, first, G, n, inv, out, inf.data(), out_std);
    }
    for (size_t i = 0; i < n; i++)
        if (inf[i] > 1) std::abort();  // a point no chain reached
}

static void run(const Table& t, const std::vector<std::vector<uint32_t>>& ks, uint32_t flags) {
    const size_t n = ks.size(), stride = (n + 15) & ~(size_t)15;
    std::vector<uint32_t> scratch(stride * FB2_SLOT_WORDS, 0xA5A5A5A5u);
    std::vector<uint4> xy;
    std::vector<uint8_t> inf;
    for (size_t i = 0; i < n; i++) {  // k_fb2_accumulate
        uint32_t k[8];
        std::memcpy(k, ks[i].data(), 32);
        if (flags & FB_F_IN_MONT) fb_scalar_from_mont(k);
        fb2_scratch_put(scratch.data(), stride, i, fb2_mul_point(t.rec.data(), t.c, t.W, k));
    }
    Fb2Plan p;
    fb2_plan(t.c, p);
    normalise(scratch, stride, n, p.inv_group, (flags & FB_F_OUT_STD) != 0, xy, inf);
    for (size_t i = 0; i < n; i++) std::printf("P %u %s\n", (unsigned)inf[i], hex4(reinterpret_cast<const uint32_t*>(xy.data()) + i * FB2_REC_WORDS).c_str());
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
        uint32_t a[8];
        if (op == "T" && f.size() == 5) {
            uint32_t b[4][8];
            for (int k = 0; k < 4; k++)
                if (!parse_hex(f[1 + k], b[k])) return 2;
            build_table(table, (uint32_t)std::stoul(f[0]), b);
            std::printf("T %u %zu\n", table.W, ((size_t)table.W) << (table.c - 1));
        } else if (op == "E" && f.size() == 2 && table.c) {
            const uint32_t j = (uint32_t)std::stoul(f[0]), d = (uint32_t)std::stoul(f[1]);
            if (j >= table.W || d < 1 || d > (1u << (table.c - 1))) return 2;
            const affine2 r = fb2_load_affine(table.rec.data() + fb_table_index(j, d, table.c) * FB2_REC_WORDS);
            alignas(16) uint32_t w[32];
            fp_to_std(w, r.x.c0), fp_to_std(w + 8, r.x.c1), fp_to_std(w + 16, r.y.c0), fp_to_std(w + 24, r.y.c1);
            std::printf("E %s\n", hex4(w).c_str());
        } else if (op == "M" && f.size() == 1 && parse_hex(f[0], a)) {
            queued.emplace_back(a, a + 8);
        } else if (op == "R" && f.size() == 1 && table.c && !queued.empty()) {
            run(table, queued, (uint32_t)std::stoul(f[0]));
            queued.clear();
        } else if (op == "I" && f.size() >= 3 && f.size() % 2 == 1) {
            const uint32_t G = (uint32_t)std::stoul(f[0]);
            const size_t n = (f.size() - 1) / 2, stride = (n + 15) & ~(size_t)15;
            if (G < 1 || G > 64) return 2;
            std::vector<uint32_t> scratch(stride * FB2_SLOT_WORDS, 0xA5A5A5A5u);
            std::vector<uint4> xy;
            std::vector<uint8_t> inf;
            for (size_t i = 0; i < n; i++) {
                uint32_t z0[8], z1[8];
                if (!parse_hex(f[1 + 2 * i], z0) || !parse_hex(f[2 + 2 * i], z1)) return 2;
                const fp2 zzz{fp_from_std(z0), fp_from_std(z1)};
                const bool ident = fp_is_zero_lt2p(zzz.c0) && fp_is_zero_lt2p(zzz.c1);
                fb2_scratch_put(scratch.data(), stride, i, ident ? xyzz2_identity() : xyzz2{fp2_one(), fp2_one(), fp2_one(), zzz});
            }
            normalise(scratch, stride, n, G, true, xy, inf);
            std::printf("I");
            for (size_t i = 0; i < n; i++) {
                const uint32_t* w = reinterpret_cast<const uint32_t*>(xy.data()) + i * FB2_REC_WORDS;
                if (!inf[i]) {  // x = t^2 with t = ZZ / ZZZ = y
                    const fp2 y{fp_from_std(w + 16), fp_from_std(w + 24)}, y2 = fp2_sqr<3>(y);
                    uint32_t c0[8], c1[8];
                    fp_to_std(c0, y2.c0), fp_to_std(c1, y2.c1);
                    if (std::memcmp(c0, w, 32) || std::memcmp(c1, w + 8, 32)) return 4;
                }
                std::printf(" %u %s %s", (unsigned)inf[i], hex(w + 16).c_str(), hex(w + 24).c_str());
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
