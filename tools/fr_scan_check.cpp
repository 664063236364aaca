// CPU run of the scalar-field scans (gpu-acceleration_amd/csrc/fr_scan_bn254.hpp is __host__ __device__): the chains, the combine steps and the
// three launches the kernels run, executed on the host with the lanes of a workgroup emulated in a loop and -DFP_BOUNDS_CHECK, which turns every
// limb-range assumption of the lazily reduced field code -- and every bound the header's comments state -- into an abort.  The arrays are exactly
// n elements (the scratch array exactly `blocks` aggregates) long, so under -fsanitize=address a chain that reads or writes past n is caught.
// tests/test_fr_scan_cpu.py feeds it and compares every word with the Python yardstick (tools/bn254_fr_scan_py.py).  Also built under the
// sanitizers as this stand-alone program (make -C gpu-acceleration_amd/csrc asan-fr-scan).
//
//   hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --cuda-host-only tools/fr_scan_check.cpp -o fr_scan_check
// stdin (or the file named as the only argument), one query per line; G (1 or 8) and flags are decimal, field values hexadecimal integers of up
// to 256 bits; flags: 2 = the input words are Fr.0, 4 = the output words likewise, 32 = exclusive product:
//   E G flags z c_0 c_1 ..            launches 1 and 2 of the polynomial                                    -> "E p(z)"
//   D G flags inplace z c_0 c_1 ..    all three, in place or into a second array                            -> "D q_0 .. q_(n-1) p(z)"
//   R G flags inplace x_0 x_1 ..      the running product                                                   -> "R out_0 .. out_(n-1) total"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#define NTT_NO_KERNELS  // host-only build: the routines, not the kernels
#include "../gpu-acceleration_amd/csrc/fr_scan_bn254.hpp"

using namespace fsck;

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
static bool parse_array(const std::vector<std::string>& f, size_t at, size_t n, std::vector<uint32_t>& out) {
    out.resize(n * 8);
    for (size_t i = 0; i < n; i++)
        if (!parse_hex(f[at + i], out.data() + 8 * i)) return false;
    return true;
}
constexpr uint32_t FILL = 0x5A5A5A5Au;  // (no canonical element has this top word)
static void print(const char* op, const std::vector<uint32_t>& a, const uint32_t* last) {
    std::printf("%s", op);
    for (size_t i = 0; i <= a.size() / 8; i++) {
        const uint32_t* w = i < a.size() / 8 ? a.data() + 8 * i : last;
        if (w[7] == FILL) std::abort();  // an element no lane wrote
        char buf[65];
        for (int k = 0; k < 8; k++) std::snprintf(buf + 8 * k, 9, "%08x", w[7 - k]);
        std::printf(" %s", buf);
    }
    std::printf("\n");
}

// the 8 combine steps of fsc_wg_scan over the 256 values of a workgroup: step k reads what step k - 1 left
template <bool SUFFIX, class Step>
static void wg_scan(std::vector<fr>& v, Step step) {
    for (uint32_t k = 0; k < FSC_STEPS; k++) {
        const std::vector<fr> old = v;
        const uint32_t d = 1u << k;
        for (uint32_t t = 0; t < FSC_BLOCK; t++)
            if (SUFFIX ? t + d < FSC_BLOCK : t >= d) v[t] = step(old[t], old[SUFFIX ? t + d : t - d], k);
    }
}

template <uint32_t G>
static void poly(const FscPoly& a, const uint32_t* in, uint32_t* out, size_t n, uint32_t* result) {
    const size_t nb = fsc_blocks(n, G);
    std::vector<uint32_t> agg(nb * FSC_AGG_WORDS, FILL);
    std::vector<fr> v(FSC_BLOCK);
    auto step13 = [&](const fr& mine, const fr& other, uint32_t k) { return fsc_poly_combine(mine, other, a.pw[k]); };
    for (size_t b = 0; b < nb; b++) {  // k_fsc_poly_aggregate
        for (uint32_t t = 0; t < FSC_BLOCK; t++) v[t] = fsc_poly_chain<G>(a, in, n, (b * FSC_BLOCK + t) * G, fr_zero());
        wg_scan<true>(v, step13);
        fsc_store9(agg.data(), b, v[0]);
    }
    fr carry = fr_zero();  // k_fsc_poly_blocks
    for (size_t round = (nb + FSC_BLOCK - 1) / FSC_BLOCK; round-- > 0;) {
        for (uint32_t t = 0; t < FSC_BLOCK; t++) {
            const size_t b = round * FSC_BLOCK + t;
            v[t] = b < nb ? fsc_load9(agg.data(), b) : fr_zero();
        }
        v[FSC_BLOCK - 1] = fsc_poly_combine(v[FSC_BLOCK - 1], carry, a.pw[FSC_STEPS]);
        wg_scan<true>(v, [&](const fr& mine, const fr& other, uint32_t k) { return fsc_poly_combine(mine, other, a.pw[FSC_STEPS + k]); });
        for (uint32_t t = 0; t < FSC_BLOCK; t++) {
            const size_t b = round * FSC_BLOCK + t;
            if (b < nb) fsc_store9(agg.data(), b, t + 1 < FSC_BLOCK ? v[t + 1] : carry);
        }
        carry = v[0];
    }
    if (result) fsc_poly_result(a, result, carry);
    if (!out) return;
    for (size_t b = 0; b < nb; b++) {  // k_fsc_poly_apply: every lane reads its chain, then every lane writes
        const fr cin = fsc_load9(agg.data(), b);
        for (uint32_t t = 0; t < FSC_BLOCK; t++) v[t] = fsc_poly_chain<G>(a, in, n, (b * FSC_BLOCK + t) * G, t == FSC_BLOCK - 1 ? cin : fr_zero());
        wg_scan<true>(v, step13);
        for (uint32_t t = 0; t < FSC_BLOCK; t++) fsc_poly_apply<G>(a, in, out, n, (b * FSC_BLOCK + t) * G, t + 1 < FSC_BLOCK ? v[t + 1] : cin);
    }
}

template <uint32_t G>
static void product(const FscProduct& a, const uint32_t* in, uint32_t* out, size_t n, uint32_t* result) {
    const size_t nb = fsc_blocks(n, G);
    std::vector<uint32_t> agg(nb * FSC_AGG_WORDS, FILL);
    std::vector<fr> v(FSC_BLOCK);
    auto step = [&](const fr& mine, const fr& other, uint32_t) { return fsc_product_combine(mine, other); };
    for (size_t b = 0; b < nb; b++) {  // k_fsc_product_aggregate
        for (uint32_t t = 0; t < FSC_BLOCK; t++) v[t] = fsc_product_chain<G>(a, in, n, (b * FSC_BLOCK + t) * G, fr_one());
        wg_scan<false>(v, step);
        fsc_store9(agg.data(), b, v[FSC_BLOCK - 1]);
    }
    fr carry = fr_one();  // k_fsc_product_blocks
    for (size_t round = 0; round < (nb + FSC_BLOCK - 1) / FSC_BLOCK; round++) {
        for (uint32_t t = 0; t < FSC_BLOCK; t++) {
            const size_t b = round * FSC_BLOCK + t;
            v[t] = b < nb ? fsc_load9(agg.data(), b) : fr_one();
        }
        v[0] = fsc_product_combine(v[0], carry);
        wg_scan<false>(v, step);
        for (uint32_t t = 0; t < FSC_BLOCK; t++) {
            const size_t b = round * FSC_BLOCK + t;
            if (b < nb) fsc_store9(agg.data(), b, t ? v[t - 1] : carry);
        }
        carry = v[FSC_BLOCK - 1];
    }
    if (result) fsc_product_result(a, result, carry);
    for (size_t b = 0; b < nb; b++) {  // k_fsc_product_apply
        const fr cin = fsc_load9(agg.data(), b);
        for (uint32_t t = 0; t < FSC_BLOCK; t++) v[t] = fsc_product_chain<G>(a, in, n, (b * FSC_BLOCK + t) * G, t == 0 ? cin : fr_one());
        wg_scan<false>(v, step);
        for (uint32_t t = 0; t < FSC_BLOCK; t++) fsc_product_apply<G>(a, in, out, n, (b * FSC_BLOCK + t) * G, t ? v[t - 1] : cin);
    }
}

int main(int argc, char** argv) {
    std::ifstream file;
    if (argc > 1) {
        file.open(argv[1]);
        if (!file) return 2;
    }
    std::istream& in = argc > 1 ? (std::istream&)file : std::cin;
    std::string line;
    unsigned long queries = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string op;
        if (!(ls >> op)) continue;
        queries++;
        std::vector<std::string> f;
        for (std::string s; ls >> s;) f.push_back(s);
        if (f.size() < 4) return 2;
        const uint32_t G = (uint32_t)std::stoul(f[0]), flags = (uint32_t)std::stoul(f[1]);
        if (!fsc_chain_ok(G)) return 2;
        uint32_t last[8] = {FILL, FILL, FILL, FILL, FILL, FILL, FILL, FILL};
        if (op == "E" || (op == "D" && f.size() >= 5)) {
            const bool div = op == "D", inplace = div && f[2] == "1";
            const size_t at = div ? 4 : 3, n = f.size() - at;
            uint32_t z[8];
            std::vector<uint32_t> x, y(div ? n * 8 : 0, FILL);
            if (!parse_hex(f[at - 1], z) || !parse_array(f, at, n, x)) return 2;
            uint32_t* out = !div ? nullptr : inplace ? x.data() : y.data();
            const FscPoly a = fsc_poly_args(fr_from_std(z), G, flags);
            if (G == FSC_CHAIN) poly<FSC_CHAIN>(a, x.data(), out, n, last);
            else poly<FSC_CHAIN_SMALL>(a, x.data(), out, n, last);
            print(div ? "D" : "E", inplace ? x : y, last);
        } else if (op == "R") {
            const bool inplace = f[2] == "1";
            const size_t n = f.size() - 3;
            std::vector<uint32_t> x, y(n * 8, FILL);
            if (!parse_array(f, 3, n, x)) return 2;
            const FscProduct a = fsc_product_args(flags);
            if (G == FSC_CHAIN) product<FSC_CHAIN>(a, x.data(), inplace ? x.data() : y.data(), n, last);
            else product<FSC_CHAIN_SMALL>(a, x.data(), inplace ? x.data() : y.data(), n, last);
            print("R", inplace ? x : y, last);
        } else {
            std::printf("bad query: %s\n", line.substr(0, 100).c_str());
            return 2;
        }
    }
    std::printf("%lu queries, no bound violated\n", queries);
    return 0;
}
