// CPU run of the scalar-vector routines (gpu-acceleration_amd/csrc/fr_vectors_bn254.hpp is __host__ __device__): the power walk, the chain
// inversion, the Lagrange chain and the linear combination the kernels run, executed lane by lane on the host with -DFP_BOUNDS_CHECK, which turns
// every limb-range assumption of the lazily reduced field code into an abort.  The arrays are exactly n elements long, so under
// -fsanitize=address a chain that reads or writes past n is caught.  tests/test_fr_vectors_cpu.py feeds it and compares every word with the
// Python yardstick (tools/bn254_fr_vectors_py.py).  Also built under the sanitizers as this stand-alone program (make -C
// gpu-acceleration_amd/csrc asan-fr-vectors).
//
//   hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --cuda-host-only tools/fr_vectors_check.cpp -o fr_vectors_check
// stdin (or the file named as the only argument), one query per line; G, flags, counts are decimal, field values hexadecimal integers of up to
// 256 bits; flags: 2 = the input words are Fr.0, 4 = the output words likewise; "-" stands for a NULL coefficient:
//   I G flags inplace x_0 x_1 ..            k_frv_batch_inverse<G> (G = 4, 8, 16, 32) over the n words, in place or into a second array  -> "I y_0 y_1 .."
//   P flags first n base scale             k_frv_powers: scale * base^(first + i)                                    -> "P y_0 .."
//   L G flags log_n tau                    k_frv_lagrange<G> (4, 8)                                                      -> "L y_0 .."
//   C flags n alias present ka kb kc a.. [b..] [c..]  k_frv_lincomb on arrays of n words; present: 1 = b is given, 2 = c is given;
//                                          alias: 0 = an output array of its own, 1, 2, 3 = the output is a, b, c    -> "C y_0 .."
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#define NTT_NO_KERNELS  // host-only build: the routines, not the kernels
#include "../gpu-acceleration_amd/csrc/fr_vectors_bn254.hpp"

using namespace frvk;

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
static void print(const char* op, const std::vector<uint32_t>& a) {
    std::printf("%s", op);
    for (size_t i = 0; i < a.size() / 8; i++) {
        if (a[8 * i + 7] == FILL) std::abort();  // an element no lane wrote
        char buf[65];
        for (int k = 0; k < 8; k++) std::snprintf(buf + 8 * k, 9, "%08x", a[8 * i + 7 - k]);
        std::printf(" %s", buf);
    }
    std::printf("\n");
}

template <uint32_t G>
static void inverse(const FrvInverse& a, const uint32_t* in, uint32_t* out, size_t n) {
    for (size_t t = 0; t < frv_chain_lanes(n, G); t++) {  // the kernel's body, lane by lane
        const size_t first = frv_chain_first(t, G);
        if (first < n) frv_inverse_chain<G>(a, in, out, n, first);
    }
}
template <uint32_t G>
static void lagrange(const FrvLagrange& a, uint32_t* out, size_t n) {
    for (size_t t = 0; t < frv_chain_lanes(n, G); t++) frv_lagrange_chain<G>(a, out, n, t);
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
        if (op == "I" && f.size() >= 4) {
            const uint32_t G = (uint32_t)std::stoul(f[0]), flags = (uint32_t)std::stoul(f[1]);
            const bool inplace = f[2] == "1";
            const size_t n = f.size() - 3;
            std::vector<uint32_t> x, y(n * 8, FILL);
            if (!parse_array(f, 3, n, x)) return 2;
            uint32_t* out = inplace ? x.data() : y.data();
            const FrvInverse a = frv_inverse_args(flags);
            if (G == 4) inverse<4>(a, x.data(), out, n);
            else if (G == 8) inverse<8>(a, x.data(), out, n);
            else if (G == 16) inverse<16>(a, x.data(), out, n);
            else if (G == 32) inverse<32>(a, x.data(), out, n);
            else return 2;
            print("I", inplace ? x : y);
        } else if (op == "P" && f.size() == 5) {
            const uint32_t flags = (uint32_t)std::stoul(f[0]);
            const uint64_t first = std::stoull(f[1]);
            const size_t n = std::stoul(f[2]);
            uint32_t b[8], s[8];
            if (!n || !parse_hex(f[3], b) || (f[4] != "-" && !parse_hex(f[4], s))) return 2;
            const FrvPowers a = frv_powers_args(fr_from_std(b), f[4] == "-" ? fr_one() : fr_from_std(s), first, flags);
            std::vector<uint32_t> y(n * 8, FILL);
            for (size_t t = 0; t < frv_powers_lanes(n); t++) frv_powers_lane(a, t, y.data(), n);
            print("P", y);
        } else if (op == "L" && f.size() == 4) {
            const uint32_t G = (uint32_t)std::stoul(f[0]), flags = (uint32_t)std::stoul(f[1]), log_n = (uint32_t)std::stoul(f[2]);
            uint32_t t[8];
            if (log_n > 16 || !parse_hex(f[3], t)) return 2;
            const size_t n = (size_t)1 << log_n;
            const FrvLagrange a = frv_lagrange_args(fr_from_std(t), log_n, flags);
            std::vector<uint32_t> y(n * 8, FILL);
            if (G == 4) lagrange<4>(a, y.data(), n);  // (the library runs the default group only)
            else if (G == 8) lagrange<8>(a, y.data(), n);
            else return 2;
            print("L", y);
        } else if (op == "C" && f.size() >= 8) {
            const uint32_t flags = (uint32_t)std::stoul(f[0]), alias = (uint32_t)std::stoul(f[2]), present = (uint32_t)std::stoul(f[3]);
            const size_t n = std::stoul(f[1]);
            const bool has[3] = {true, (present & 1u) != 0, (present & 2u) != 0};
            const size_t arrays = 1 + has[1] + has[2];
            if (!n || present > 3 || f.size() != 7 + arrays * n || alias > 3 || (alias && !has[alias - 1])) return 2;
            fr k[3];
            for (int j = 0; j < 3; j++) {
                uint32_t w[8];
                if (f[4 + j] == "-") k[j] = fr_one();
                else if (parse_hex(f[4 + j], w)) k[j] = fr_from_std(w);
                else return 2;
            }
            std::vector<uint32_t> v[3], y(n * 8, FILL);
            size_t at = 7;
            for (int j = 0; j < 3; j++) {
                if (!has[j]) continue;
                if (!parse_array(f, at, n, v[j])) return 2;
                at += n;
            }
            uint32_t* out = alias ? v[alias - 1].data() : y.data();
            const FrvLincomb a = frv_lincomb_args(k[0], k[1], k[2], flags);
            for (size_t i = 0; i < n; i++) frv_lincomb_one(a, v[0].data(), has[1] ? v[1].data() : nullptr, has[2] ? v[2].data() : nullptr, out, i);
            print("C", alias ? v[alias - 1] : y);
        } else {
            std::printf("bad query: %s\n", line.substr(0, 100).c_str());
            return 2;
        }
    }
    std::printf("%lu queries, no bound violated\n", queries);
    return 0;
}
