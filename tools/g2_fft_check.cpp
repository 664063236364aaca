// CPU run of the G2 group transform (gpu-acceleration_amd/csrc/g2_fft_bn254.hpp is __host__ __device__): the G1 transform's index arithmetic, the
// bit-reversal sweep of 128-byte records, the ladder of the G2 element-wise multiplication, the pair of complete additions to T and -T and the
// shared inversion by products of norms that k_gf2_bitrev and k_gf2_stage run, executed butterfly by butterfly and phase by phase on the host in
// the kernels' order, in groups of FB_GROUP through fb_batch_inverse_host, the twiddle table made by the powers kernel's own lane routine, the
// inverse's n^-1 by k_pm2_mul<true>'s phases -- with -DFP_BOUNDS_CHECK, which turns every limb-range assumption of the lazily reduced field code
// into an abort.  On top of those limb-wise checks every butterfly asserts the VALUE bounds g2_fft_bn254.hpp writes down: T.y < 7p, -T.y <= 8p,
// and X < 12p, Y < 8p, ZZ, ZZZ < 4.2p for T and both sums.  tests/test_g2_fft_cpu.py feeds it and compares every word with the cases of
// tools/g2_fft_cases.py.  Also built under -fsanitize=address,undefined as this stand-alone program (make -C gpu-acceleration_amd/csrc asan-g2-fft).
//
//   hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --cuda-host-only tools/g2_fft_check.cpp -o g2_fft_check
// stdin (or the file named as the only argument), one query per line, the protocol of tools/g1_fft_check.cpp; numbers are hexadecimal integers
// of up to 256 bits, the WORDS as the call reads them; a point is four numbers x.c0 x.c1 y.c0 y.c1; flags: 1 = inverse, 8 = standard-form
// output, 16 = standard-form input:
//   B inf point          queue a point (inf: nonzero = flagged)
//   F flags log_n        the transform of the queue, batch = queue / 2^log_n arrays, as msm_bn254_g2_fft_device enqueues it -> one "P inf point" per point
//   W flags w            ONE ladder-stage butterfly on the two queued points (A, B) with the twiddle w (standard form, any 256-bit pattern), the
//                        lane at the last place of its group; flags 8, 16 -> "P inf point" of A + w B, then of A - w B
//   I item log_n s inv   gf_pair                                                                      -> "I a b out_sum out_diff tw"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#define NTT_NO_KERNELS  // a host-only build: no kernels, no device code object
#include "../gpu-acceleration_amd/csrc/g2_fft_bn254.hpp"
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
    alignas(16) uint32_t w[32];
};
struct Tw {
    alignas(16) uint32_t w[8];
};
struct Arrays {  // what the device call is given
    std::vector<Rec> xy;
    std::vector<uint8_t> inf;
};

// ---- the value bounds of g2_fft_bn254.hpp: a normalised component against tenths * p / 10 ----
// v <= tenths * p / 10 (strict: <), both as 9 limbs of 29 bits; tenths * p / 10 is rounded DOWN, so the test is never too lenient
static bool below_tenths(const fp& v, uint32_t tenths, bool strict) {
    uint64_t t[9], c = 0;
    for (int i = 0; i < 9; i++) {  // tenths * p
        const uint64_t s = (uint64_t)tenths * FP29_P[i] + c;
        t[i] = i < 8 ? (s & FP_MASK) : s;
        c = i < 8 ? s >> FP_LIMB_BITS : 0;
    }
    uint64_t rem = 0;
    for (int i = 8; i >= 0; i--) {  // / 10
        const uint64_t cur = (rem << FP_LIMB_BITS) | t[i];
        t[i] = cur / 10;
        rem = cur % 10;
    }
    for (int i = 8; i >= 0; i--) {
        if (v.v[i] >= (1u << FP_LIMB_BITS)) return false;  // not normalised
        if ((uint64_t)v.v[i] != t[i]) return (uint64_t)v.v[i] < t[i];
    }
    return !strict;
}
static bool below2(const fp2& v, uint32_t tenths, bool strict = true) { return below_tenths(v.c0, tenths, strict) && below_tenths(v.c1, tenths, strict); }
static void assert_xyzz(const xyzz2& p, const char* what) {
    FP_ASSERT(below2(p.x, 120) && below2(p.y, 80, false) && below2(p.zz, 42) && below2(p.zzz, 42), what);
}
// what gf2_butterfly is promised and what it hands xyzz2_madd
static void assert_operands(const xyzz2& T) {
    assert_xyzz(T, "T leaves the XYZZ bounds");
    FP_ASSERT(below2(T.y, 70), "T.y >= 7p: fp2_neg<8> does not take it");
    FP_ASSERT(below2(gf2_neg(T).y, 80, false), "-T.y > 8p: outside what xyzz2_madd accepts for an accumulator");
}

// The phases as functions of their own, each compiled ONCE: the headers' routines are force-inlined, and a copy of the ladder, of the two additions and
// of the two output conversions in each of run_stage<true>, run_stage<false> and run_scale makes the sanitizer build of this file several times as long.
#define G2F_NOINLINE __attribute__((noinline))
static G2F_NOINLINE xyzz2 lane_finish(Pm2Lane& t, const fp& ni) { return pm2_lane_finish(t, ni); }
static G2F_NOINLINE void butterfly(const xyzz2& T, const uint32_t* a_rec, bool in_std, bool a_inf, xyzz2& sum, xyzz2& diff) {
    gf2_butterfly(T, pm2_load_point(a_rec, in_std), a_inf, sum, diff);
}
static G2F_NOINLINE void lane_store(uint32_t* xy, uint8_t* inf, const GfPair& p, const xyzz2& sum, bool sum_id, const xyzz2& diff, bool diff_id, const fp& inv,
                                    const fp& ns, const fp& nd, bool out_std) {
    gf2_lane_store(xy, inf, p, sum, sum_id, diff, diff_id, inv, ns, nd, out_std);
}
static G2F_NOINLINE void store_output(uint32_t* out_xy, uint8_t* out_inf, const xyzz2& p, const fp& ni, bool identity, bool out_std) {
    pm2_store_output(out_xy, out_inf, p, ni, identity, out_std);
}

// one launch of k_gf2_stage<LADDER>: `count` butterflies from `first`, one workgroup after another
template <bool LADDER>
static void run_stage(Arrays& d, const uint32_t* tw, const GfStage& st, uint64_t first, uint32_t count) {
    std::vector<uint32_t> tree(FB_TREE_WORDS);
    std::vector<Pm2Lane> lane(FB_GROUP);
    std::vector<xyzz2> T(FB_GROUP), sum(FB_GROUP), diff(FB_GROUP);
    std::vector<GfPair> p(FB_GROUP);
    fp den[FB_GROUP], inv[FB_GROUP], ns[FB_GROUP], nd[FB_GROUP];
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
            T[l] = xyzz2_identity();
            den[l] = fp_one();
            bool x_zero = false;
            if (LADDER) {
                if (!idle[l]) den[l] = gf2_lane_begin(lane[l], xy + p[l].b * FB2_REC_WORDS, tw + p[l].tw * 8, st, x_zero);
                skip[l] = idle[l] || x_zero;
            } else if (!idle[l]) {
                T[l] = gf2_lane_plain(xy + p[l].b * FB2_REC_WORDS, st);
            }
        }
        if (LADDER) {
            fb_batch_inverse_host(tree.data(), den, skip, inv);
            for (uint32_t l = 0; l < FB_GROUP; l++)
                if (!idle[l]) T[l] = lane_finish(lane[l], inv[l]);
        }
        for (uint32_t l = 0; l < FB_GROUP; l++) {
            sum[l] = diff[l] = xyzz2_identity();
            if (live[l]) {
                assert_operands(T[l]);
                butterfly(T[l], xy + p[l].a * FB2_REC_WORDS, (st.flags & GF_F_IN_STD) != 0, a_inf[l], sum[l], diff[l]);
                assert_xyzz(sum[l], "A + T leaves the XYZZ bounds");
                assert_xyzz(diff[l], "A - T leaves the XYZZ bounds");
            }
            sum_id[l] = pm2_is_identity(sum[l]);
            diff_id[l] = pm2_is_identity(diff[l]);
            den[l] = gf2_inv_enter(sum[l], sum_id[l], diff[l], diff_id[l], ns[l], nd[l]);
            FP_ASSERT(below_tenths(ns[l], 23, true) && below_tenths(nd[l], 23, true) && below_tenths(den[l], 22, true), "a norm or the leaf of the product tree exceeds its bound");
            skip[l] = false;
        }
        fb_batch_inverse_host(tree.data(), den, skip, inv);
        for (uint32_t l = 0; l < FB_GROUP; l++)
            if (live[l]) lane_store(xy, d.inf.data(), p[l], sum[l], sum_id[l], diff[l], diff_id[l], inv[l], ns[l], nd[l], (st.flags & GF_F_OUT_STD) != 0);
    }
}

// k_pm2_mul<true> over the arrays, in place (tools/g2_pointwise_mul_check.cpp has the same loop)
static void run_scale(Arrays& d, const PmSplit& uni, uint32_t flags) {
    std::vector<uint32_t> tree(FB_TREE_WORDS);
    std::vector<Pm2Lane> lane(FB_GROUP);
    std::vector<xyzz2> acc(FB_GROUP);
    fp den[FB_GROUP], inv[FB_GROUP];
    bool idle[FB_GROUP], skip[FB_GROUP];
    const size_t n = d.xy.size();
    for (size_t g = 0; g < n; g += FB_GROUP) {
        for (uint32_t l = 0; l < FB_GROUP; l++) {
            idle[l] = g + l >= n || d.inf[g + l] != 0;
            den[l] = fp_one();
            bool x_zero = false;
            lane[l].s = uni;
            if (!idle[l]) den[l] = pm2_lane_begin<true>(lane[l], d.xy[g + l].w, nullptr, flags, x_zero);
            skip[l] = idle[l] || x_zero;
        }
        fb_batch_inverse_host(tree.data(), den, skip, inv);
        for (uint32_t l = 0; l < FB_GROUP; l++) {
            acc[l] = idle[l] ? xyzz2_identity() : lane_finish(lane[l], inv[l]);
            skip[l] = pm2_is_identity(acc[l]);
            den[l] = skip[l] ? fp_one() : pm2_out_norm(acc[l]);
        }
        fb_batch_inverse_host(tree.data(), den, skip, inv);
        for (uint32_t l = 0; l < FB_GROUP && g + l < n; l++)
            store_output(d.xy[g + l].w, &d.inf[g + l], acc[l], inv[l], skip[l], (flags & PM_F_OUT_STD) != 0);
    }
}

// group_fft_enqueue<HostG2> of msm_g1_fft.inc
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
    for (size_t i = 0; i < points; i++) gf2_bitrev_one(d.xy[0].w, d.inf.data(), i, k);
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

static void print_one(const Arrays& d, size_t i) {
    const uint32_t* w = d.xy[i].w;
    std::printf("P %u %s %s %s %s\n", (unsigned)d.inf[i], hex(w).c_str(), hex(w + 8).c_str(), hex(w + 16).c_str(), hex(w + 24).c_str());
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
        uint32_t a[8];
        Rec r;
        if (op == "B" && f.size() == 5 && parse_hex(f[1], r.w) && parse_hex(f[2], r.w + 8) && parse_hex(f[3], r.w + 16) && parse_hex(f[4], r.w + 24)) {
            d.xy.push_back(r);
            d.inf.push_back((uint8_t)std::stoul(f[0]));
        } else if (op == "F" && f.size() == 2 && std::stoul(f[1]) <= 16 && !d.xy.empty() && d.xy.size() % ((size_t)1 << std::stoul(f[1])) == 0) {
            run_fft(d, (uint32_t)std::stoul(f[1]), (uint32_t)std::stoul(f[0]));
            for (size_t i = 0; i < d.xy.size(); i++) print_one(d, i);
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
            for (const uint64_t at : {p.a, p.b}) print_one(big, at);
            for (size_t i = 0; i < big.xy.size(); i++)  // every other place: flagged in, so flagged and zero out
                if (i != p.a && i != p.b) {
                    uint32_t any = 0;
                    for (int w = 0; w < 32; w++) any |= big.xy[i].w[w];
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
