// CPU run of the scalar-field transforms (gpu-acceleration_amd/csrc/fr_bn254.hpp and ntt_bn254.hpp are __host__ __device__): the same plan, the
// same tables, the same load / butterfly / store phases the kernels run, executed tile group by tile group on the host with -DFP_BOUNDS_CHECK,
// which turns every limb-range assumption of the lazily reduced field into an abort.  tests/test_ntt_cpu.py feeds it and compares every word
// with the independent Python yardstick (tools/bn254_fr_ntt_py.py).
//
//   hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --cuda-host-only tools/ntt_check.cpp -o ntt_check
// stdin, one query per line; field elements as 64 hex digits (ANY 256-bit pattern), arrays as files of 8 little-endian 32-bit words per element:
//   N log_n batch flags tile g|- in out   the transform msm_bn254_fr_ntt_device enqueues (flags: MSM_NTT_*; tile: log2 of the LDS tile; g: coset generator)
//   M n flags k|- a b c|- out             msm_bn254_fr_mul_sub_scale_device
//   O op a b                              -> "O result": mul, add, sub (a op b mod r), tomont (a * 2^256), frommont (a / 2^256); b ignored by the last two
//   P log_n tile                          -> "P passes r0 r1 ...": the plan
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define NTT_NO_KERNELS
#include "../gpu-acceleration_amd/csrc/ntt_bn254.hpp"

using namespace nttk;

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
    return true;
}
static void print_words(const uint32_t w[8]) {
    for (int i = 7; i >= 0; i--) std::printf("%08x", w[i]);
}
static bool read_file(const char* path, std::vector<uint32_t>& v, size_t words) {
    v.assign(words, 0);
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t got = std::fread(v.data(), 4, words, f);
    std::fclose(f);
    return got == words;
}
static bool write_file(const char* path, const std::vector<uint32_t>& v) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const size_t put = std::fwrite(v.data(), 4, v.size(), f);
    std::fclose(f);
    return put == v.size();
}

static std::vector<uint32_t> pow_table(const fr& base, const fr& scale, uint32_t count) {
    std::vector<uint32_t> t((size_t)count * 8);
    for (uint32_t e = 0; e < count; e++) ntt_pow_entry(base, scale, e, t.data());
    return t;
}
// lo entries then hi entries, as msm_ntt.inc lays a two-level table out
static std::vector<uint32_t> two_level(const fr& base, const fr& scale, uint32_t k) {
    const uint32_t h = ntt_split(k);
    fr bh = base;
    for (uint32_t i = 0; i < h; i++) bh = fr_mul(bh, bh);
    std::vector<uint32_t> t = pow_table(base, scale, 1u << h), hi = pow_table(bh, fr_one(), 1u << (k - h));
    t.insert(t.end(), hi.begin(), hi.end());
    return t;
}

template <uint32_t T>
static void run_pass(const NttPass& ps, const NttTables& tb, const uint32_t* src, uint32_t* dst) {
    std::vector<uint32_t> lds((size_t)9 << T);
    const uint64_t groups = ntt_groups(ps, T);
    for (uint64_t g = 0; g < groups; g++) {
        for (uint32_t x = 0; x < (1u << T); x++) ntt_phase_load<T>(ps, tb, src, g, x, lds.data());
        for (uint32_t s = 0; s < ps.t; s++)
            for (uint32_t wi = 0; wi < (1u << (T - 1)); wi++) ntt_phase_butterfly<T>(ps, tb, s, wi, lds.data());
        for (uint32_t x = 0; x < (1u << T); x++) ntt_phase_store<T>(ps, tb, dst, g, x, lds.data());
    }
}

static bool transform(std::vector<uint32_t>& data, uint32_t k, size_t batch, uint32_t flags, uint32_t T, const uint32_t* g_std) {
    const bool inverse = flags & NTT_F_INVERSE;
    NttPass ps[NTT_MAX_PASSES];
    const uint32_t P = ntt_make_passes(k, T, batch, flags, g_std != nullptr, ps);
    fr w10 = ntt_root(NTT_WT_LOG2), wk = ntt_root(k);
    if (inverse) w10 = fr_inv(w10), wk = fr_inv(wk);
    const std::vector<uint32_t> wt = pow_table(w10, fr_one(), 1u << (NTT_WT_LOG2 - 1)), tw = two_level(wk, fr_one(), k);
    std::vector<uint32_t> cs;
    if (g_std) {
        const fr g = fr_from_std(g_std);
        if (fr_is_zero_exact(fr_canonical(g))) return false;
        cs = two_level(inverse ? fr_inv(g) : g, inverse ? ntt_factor_out(k, flags) : ntt_factor_in(flags), k);
    }
    NttTables tb{wt.data(), tw.data(), tw.data() + ((size_t)8 << ntt_split(k)), cs.data(), cs.data() + ((size_t)8 << ntt_split(k))};
    std::vector<uint32_t> scratch(P > 1 ? data.size() : 0);
    for (uint32_t p = 0; p < P; p++) {
        const uint32_t* src = p == 0 ? data.data() : scratch.data();
        uint32_t* dst = p + 1 == P ? data.data() : scratch.data();
        if (T == NTT_TILE_LOG2) run_pass<NTT_TILE_LOG2>(ps[p], tb, src, dst);
        else run_pass<NTT_TILE_SMALL_LOG2>(ps[p], tb, src, dst);
    }
    return true;
}

int main() {
    static char line[2048], f[8][600];
    unsigned long queries = 0;
    while (std::fgets(line, sizeof line, stdin)) {
        const int nf = std::sscanf(line, "%599s %599s %599s %599s %599s %599s %599s %599s", f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7]);
        if (nf < 1) continue;
        queries++;
        if (f[0][0] == 'N' && nf == 8) {
            const uint32_t k = (uint32_t)std::atoi(f[1]), flags = (uint32_t)std::atoi(f[3]), T = (uint32_t)std::atoi(f[4]);
            const size_t batch = (size_t)std::atol(f[2]);
            uint32_t g[8];
            const bool coset = std::strcmp(f[5], "-") != 0;
            std::vector<uint32_t> data;
            if (k > 20 || (T != NTT_TILE_LOG2 && T != NTT_TILE_SMALL_LOG2) || (coset && !parse(f[5], g)) || !read_file(f[6], data, (batch << k) * 8) ||
                !transform(data, k, batch, flags, T, coset ? g : nullptr) || !write_file(f[7], data)) {
                std::printf("bad query: %s", line);
                return 2;
            }
            std::printf("N ok\n");
        } else if (f[0][0] == 'M' && nf == 8) {
            const size_t n = (size_t)std::atol(f[1]);
            const uint32_t flags = (uint32_t)std::atoi(f[2]);
            uint32_t kw[8];
            const bool has_k = std::strcmp(f[3], "-") != 0, has_c = std::strcmp(f[6], "-") != 0;
            std::vector<uint32_t> a, b, c, out(n * 8);
            if ((has_k && !parse(f[3], kw)) || !read_file(f[4], a, n * 8) || !read_file(f[5], b, n * 8) || (has_c && !read_file(f[6], c, n * 8))) {
                std::printf("bad query: %s", line);
                return 2;
            }
            // the constants as msm_bn254_fr_mul_sub_scale_device prepares them
            const bool im = flags & NTT_F_IN_MONT, om = flags & NTT_F_OUT_MONT;
            fr post = has_k ? fr_from_std(kw) : fr_one();
            if (om && !im) post = fr_mul(post, ntt_consts().p256);
            if (im && !om) post = fr_mul(post, ntt_consts().m256);
            post = fr_canonical(post);
            for (size_t i = 0; i < n; i++)
                ntt_mul_sub_scale_one(&a[i * 8], &b[i * 8], has_c ? &c[i * 8] : nullptr, ntt_factor_in(flags), post, &out[i * 8]);
            if (!write_file(f[7], out)) return 2;
            std::printf("M ok\n");
        } else if (f[0][0] == 'O' && nf == 4) {
            uint32_t a[8], b[8], w[8];
            if (!parse(f[2], a) || !parse(f[3], b)) {
                std::printf("bad query: %s", line);
                return 2;
            }
            const std::string op = f[1];
            const fr x = fr_from_std(a), y = fr_from_std(b);
            if (op == "mul") fr_to_std(w, fr_mul(x, y));
            else if (op == "add") fr_to_std(w, fr_add(x, y));
            else if (op == "sub") fr_to_std(w, fr_sub<3>(x, y));
            else if (op == "tomont") fr_pack(w, fr_reduce_lt2r(fr_mul(x, ntt_factor_out(0, NTT_F_OUT_MONT))));
            else if (op == "frommont") fr_to_std(w, fr_mul(fr_unpack(a), ntt_factor_in(NTT_F_IN_MONT)));
            else return 2;
            std::printf("O ");
            print_words(w);
            std::printf("\n");
        } else if (f[0][0] == 'P' && nf == 3) {
            const NttPlan pl = ntt_make_plan((uint32_t)std::atoi(f[1]), (uint32_t)std::atoi(f[2]));
            std::printf("P %u", pl.passes);
            for (uint32_t i = 0; i < pl.passes; i++) std::printf(" %u", pl.radix[i]);
            std::printf("\n");
        } else {
            std::printf("bad query: %s", line);
            return 2;
        }
    }
    std::printf("%lu queries, no bound violated\n", queries);
    return 0;
}
