// CPU run of the G1 group transform (gpu-acceleration_amd/csrc/g1_fft_bn254.hpp is __host__ __device__): the same index arithmetic, bit-reversal
// sweep, ladder, pair of complete additions and shared inversion by products that k_gf_bitrev and k_gf_stage run, executed butterfly by
// butterfly and phase by phase on the host in the kernels' order, in groups of FB_GROUP through fb_batch_inverse_host, the twiddle table made
// by the powers kernel's own lane routine, the inverse's n^-1 by k_pm_mul<true>'s phases -- with -DFP_BOUNDS_CHECK, which turns every limb-range
// assumption of the lazily reduced field code into an abort.  tests/test_g1_fft_cpu.py feeds it and compares every word with the cases of
// tools/g1_fft_cases.py.  Also built under -fsanitize=address,undefined as this stand-alone program (make -C gpu-acceleration_amd/csrc asan-g1-fft).
//
//   hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --cuda-host-only tools/g1_fft_check.cpp -o g1_fft_check
// stdin (or the file named as the only argument), one query per line; numbers are hexadecimal integers of up to 256 bits, the WORDS as the call
// reads them; flags: 1 = inverse, 8 = standard-form output, 16 = standard-form input:
//   B inf x y            queue a point (inf: nonzero = flagged)
//   F flags log_n        the transform of the queue, batch = queue / 2^log_n arrays, as msm_bn254_g1_fft_device enqueues it -> one "P inf x y" per point
//   W flags w            ONE ladder-stage butterfly on the two queued points (A, B) with the twiddle w (standard form, any 256-bit pattern), the
//                        lane at the last place of its group; flags 8, 16 -> "P inf x y" of A + w B, then of A - w B
//   I item log_n s inv   gf_pair                                                                      -> "I a b out_sum out_diff tw"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#define NTT_NO_KERNELS  // a host-only build: no kernels, no device code object
#include "../gpu-acceleration_amd/csrc/g1_fft_bn254.hpp"
#include "../gpu-acceleration_amd/csrc/fr_vectors_bn254.hpp"

using namespace gfk;

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

struct Rec {
    alignas(16) uint32_t w[16];
};
struct Tw {
    alignas(16) uint32_t w[8];
};
struct Arrays {  // what the device call is given
    std::vector<Rec> xy;
    std::vector<uint8_t> inf;
};

// one launch of k_gf_stage<LADDER>: `count` butterflies from `first`, one workgroup after another
template <bool LADDER>
static void run_stage(Arrays& d, const uint32_t* tw, const GfStage& st, uint64_t first, uint32_t count) {
    std::vector<uint32_t> tree(FB_TREE_WORDS);
    std::vector<PmLane> lane(FB_GROUP);
    std::vector<xyzz> T(FB_GROUP), sum(FB_GROUP), diff(FB_GROUP);
    std::vector<GfPair> p(FB_GROUP);
    fp den[FB_GROUP], inv[FB_GROUP], zs[FB_GROUP], zd[FB_GROUP];
    bool live[FB_GROUP], idle[FB_GROUP], skip[FB_GROUP], a_inf[FB_GROUP], sum_id[FB_GROUP], diff_id[FB_GROUP];
    uint32_t* xy = d.xy[0].w;
    for (uint32_t g = 0; g < count; g += FB_GROUP) {
        for (uint32_t l = 0; l < FB_GROUP; l++) {
            live[l] = g + l < count;
            p[l] = GfPair{};
            a_inf[l] = true;
            bool b_inf = true;
            if (live[l]) {
                p[l] = gf_pair(first + g + l, st);
                FP_ASSERT(p[l].a < d.xy.size() && p[l].b < d.xy.size() && p[l].tw < gf_table_entries(st.log_n) + (LADDER ? 0 : 1), "an index leaves its array");
                a_inf[l] = d.inf[p[l].a] != 0;
                b_inf = d.inf[p[l].b] != 0;
            }
            idle[l] = !live[l] || b_inf;
            T[l] = xyzz_identity();
            den[l] = fp_one();
            bool x_zero = false;
            if (LADDER) {
                if (!idle[l]) den[l] = gf_lane_begin(lane[l], xy + p[l].b * 16, tw + p[l].tw * 8, st, x_zero);
                skip[l] = idle[l] || x_zero;
            } else if (!idle[l]) {
                T[l] = gf_lane_plain(xy + p[l].b * 16, st);
            }
        }
        if (LADDER) {
            fb_batch_inverse_host(tree.data(), den, skip, inv);
            for (uint32_t l = 0; l < FB_GROUP; l++)
                if (!idle[l]) T[l] = pm_lane_finish(lane[l], inv[l]);
        }
        for (uint32_t l = 0; l < FB_GROUP; l++) {
            sum[l] = diff[l] = xyzz_identity();
            if (live[l]) gf_butterfly(T[l], pm_load_point(xy + p[l].a * 16, (st.flags & GF_F_IN_STD) != 0), a_inf[l], sum[l], diff[l]);
            sum_id[l] = pm_is_identity(sum[l]);
            diff_id[l] = pm_is_identity(diff[l]);
            den[l] = gf_inv_enter(sum[l], sum_id[l], diff[l], diff_id[l], zs[l], zd[l]);
            skip[l] = false;
        }
        fb_batch_inverse_host(tree.data(), den, skip, inv);
        for (uint32_t l = 0; l < FB_GROUP; l++)
            if (live[l]) gf_lane_store(xy, d.inf.data(), p[l], sum[l], sum_id[l], diff[l], diff_id[l], inv[l], zs[l], zd[l], (st.flags & GF_F_OUT_STD) != 0);
    }
}

// k_pm_mul<true> over the arrays, in place (tools/pointwise_mul_check.cpp has the same loop)
static void run_scale(Arrays& d, const PmSplit& uni, uint32_t flags) {
    std::vector<uint32_t> tree(FB_TREE_WORDS);
    std::vector<PmLane> lane(FB_GROUP);
    std::vector<xyzz> acc(FB_GROUP);
    fp den[FB_GROUP], inv[FB_GROUP];
    bool idle[FB_GROUP], skip[FB_GROUP];
    const size_t n = d.xy.size();
    for (size_t g = 0; g < n; g += FB_GROUP) {
        for (uint32_t l = 0; l < FB_GROUP; l++) {
            idle[l] = g + l >= n || d.inf[g + l] != 0;
            den[l] = fp_one();
            bool x_zero = false;
            lane[l].s = uni;
            if (!idle[l]) den[l] = pm_lane_begin<true>(lane[l], d.xy[g + l].w, nullptr, flags, x_zero);
            skip[l] = idle[l] || x_zero;
        }
        fb_batch_inverse_host(tree.data(), den, skip, inv);
        for (uint32_t l = 0; l < FB_GROUP; l++) {
            acc[l] = idle[l] ? xyzz_identity() : pm_lane_finish(lane[l], inv[l]);
            den[l] = acc[l].zzz;
            skip[l] = pm_is_identity(acc[l]);
        }
        fb_batch_inverse_host(tree.data(), den, skip, inv);
        for (uint32_t l = 0; l < FB_GROUP && g + l < n; l++)
            fb_store_output(d.xy[g + l].w, &d.inf[g + l], acc[l], inv[l], skip[l], (flags & PM_F_OUT_STD) != 0);
    }
}

// g1_fft_enqueue of msm_g1_fft.inc
static void run_fft(Arrays& d, uint32_t k, uint32_t flags) {
    const bool inverse = flags & GF_F_INVERSE;
    const size_t points = d.xy.size();
    if (k == 0) {
        const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
        run_scale(d, pm_split_host(one), flags & (GF_F_IN_STD | GF_F_OUT_STD));
        return;
    }
    std::vector<Tw> tw((size_t)gf_table_entries(k) + 1);  // (+ 1: never empty)
    if (k >= 2) {
        const size_t entries = (size_t)gf_table_entries(k);
        const frvk::FrvPowers a = frvk::frv_powers_args(nttk::ntt_root(k), nttk::fr_one(), 0, 0);
        for (size_t t = 0; t < frvk::frv_powers_lanes(entries); t++) frvk::frv_powers_lane(a, t, tw[0].w, entries);
    }
    for (size_t i = 0; i < points; i++) gf_bitrev_one(d.xy[0].w, d.inf.data(), i, k);
    for (uint32_t s = 1; s <= k; s++) {
        GfStage st{k, s, inverse ? GF_F_INVERSE : 0u};
        if (s == 1) st.flags |= flags & GF_F_IN_STD;
        if (s == k && !inverse) st.flags |= flags & GF_F_OUT_STD;
        if (s == 1) run_stage<false>(d, tw[0].w, st, 0, (uint32_t)(points >> 1));
        else run_stage<true>(d, tw[0].w, st, 0, (uint32_t)(points >> 1));
    }
    if (!inverse) return;
    uint32_t n_std[8] = {1u << k, 0, 0, 0, 0, 0, 0, 0}, ninv_std[8];
    nttk::fr_to_std(ninv_std, nttk::fr_inv(nttk::fr_from_std(n_std)));
    run_scale(d, pm_split_host(ninv_std), flags & GF_F_OUT_STD);
}

static void print(const Arrays& d) {
    for (size_t i = 0; i < d.xy.size(); i++) std::printf("P %u %s %s\n", (unsigned)d.inf[i], hex(d.xy[i].w).c_str(), hex(d.xy[i].w + 8).c_str());
}

int main(int argc, char** argv) {
    std::ifstream file;
    if (argc > 1) {
        file.open(argv[1]);
        if (!file) return 2;
    }
    std::istream& in = argc > 1 ? (std::istream&)file : std::cin;
    Arrays d;
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
        if (op == "B" && f.size() == 3 && parse_hex(f[1], a) && parse_hex(f[2], b)) {
            Rec r;
            std::memcpy(r.w, a, 32), std::memcpy(r.w + 8, b, 32);
            d.xy.push_back(r);
            d.inf.push_back((uint8_t)std::stoul(f[0]));
        } else if (op == "F" && f.size() == 2 && std::stoul(f[1]) <= 16 && !d.xy.empty() && d.xy.size() % ((size_t)1 << std::stoul(f[1])) == 0) {
            run_fft(d, (uint32_t)std::stoul(f[1]), (uint32_t)std::stoul(f[0]));
            print(d);
            d.xy.clear(), d.inf.clear();
        } else if (op == "W" && f.size() == 2 && parse_hex(f[1], a) && d.xy.size() == 2) {
            // butterfly FB_GROUP - 1 of the second stage of a transform of 2^10 points whose other records are all flagged; the table holds w at
            // EVERY entry, so whichever one the butterfly reads is w
            const uint32_t k = 10, fl = (uint32_t)std::stoul(f[0]);
            Arrays big;
            big.xy.assign((size_t)1 << k, Rec{});
            big.inf.assign((size_t)1 << k, 1);
            const GfStage st{k, 2, fl & (GF_F_IN_STD | GF_F_OUT_STD)};
            const GfPair p = gf_pair(FB_GROUP - 1, st);
            big.xy[p.a] = d.xy[0], big.inf[p.a] = d.inf[0];
            big.xy[p.b] = d.xy[1], big.inf[p.b] = d.inf[1];
            std::vector<Tw> tw((size_t)gf_table_entries(k));
            for (auto& t : tw) std::memcpy(t.w, a, 32);
            run_stage<true>(big, tw[0].w, st, 0, (uint32_t)1 << (k - 1));
            for (const uint64_t at : {p.a, p.b}) std::printf("P %u %s %s\n", (unsigned)big.inf[at], hex(big.xy[at].w).c_str(), hex(big.xy[at].w + 8).c_str());
            for (size_t i = 0; i < big.xy.size(); i++)  // every other place: flagged in, so flagged and zero out
                if (i != p.a && i != p.b) {
                    uint32_t any = 0;
                    for (int w = 0; w < 16; w++) any |= big.xy[i].w[w];
                    if (big.inf[i] != 1 || any) {
                        std::printf("a flagged pair gave a point at %zu\n", i);
                        return 2;
                    }
                }
            d.xy.clear(), d.inf.clear();
        } else if (op == "I" && f.size() == 4) {
            const GfStage st{(uint32_t)std::stoul(f[1]), (uint32_t)std::stoul(f[2]), f[3] != "0" ? GF_F_INVERSE : 0u};
            const GfPair p = gf_pair(std::stoull(f[0]), st);
            std::printf("I %llu %llu %llu %llu %llu\n", (unsigned long long)p.a, (unsigned long long)p.b, (unsigned long long)p.out_sum,
                        (unsigned long long)p.out_diff, (unsigned long long)p.tw);
        } else {
            std::printf("bad query: %s\n", line.c_str());
            return 2;
        }
    }
    std::printf("%lu queries, no bound violated\n", queries);
    return 0;
}
