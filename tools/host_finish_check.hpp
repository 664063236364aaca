// tools/host_finish_check.hpp -- checks of host_finish.hpp for one group (G = HostG1 / HostG2), shared by tools/host_asan_check.cpp and
// tools/host_g2_asan_check.cpp: the real Horner chain and the real fold of partials, with known answers built from one generator.
#pragma once
#include <cstdio>
#include <cstring>
#include <vector>

#include "../gpu-acceleration_amd/csrc/host_finish.hpp"

namespace finishcheck {

template <class G>
bool same_point(const typename G::Jac& a, const typename G::Jac& b) {
    if (G::is_identity(a) || G::is_identity(b)) return G::is_identity(a) && G::is_identity(b);
    const typename G::Jac na = G::normalize(a), nb = G::normalize(b);
    return std::memcmp(&na, &nb, sizeof na) == 0;
}
template <class G>
typename G::Jac smul(const typename G::Jac& p, uint64_t k) {  // double-and-add
    typename G::Jac acc = G::identity(), base = p;
    for (; k; k >>= 1) {
        if (k & 1) acc = G::jadd(acc, base);
        base = G::jdbl(base);
    }
    return acc;
}

// One shape of host_finish_chain's input: V bucket arrays spaced `spacing` bit positions apart, each reduced as 2^pw_bits (pseudo-)windows of
// rkb + 1 bit sums (kb = rkb + pw_bits index bits per array); only the low top_bits index bits of the top array carry weight.
struct Shape {
    const char* name;
    uint32_t V, kb, rkb, pw_bits, spacing, top_bits;
};

// Bit sums c * gen with small c (some zero: the identity), through the real chain with no pool and pools of 1 and 3 workers, against a
// direct sum of 2^e * gen * (coefficient of position e).  What each bit sum weighs, from the meaning of the buckets: bucket b = q * 2^rkb + b'
// of array v holds the digit 1 + (digit bits of b) at weight 2^(spacing * v), where digit bits are the index bits j < kb, in the top array
// only j < top_bits.  So Q[v][q][u] (buckets with bit u of b' set) weighs 2^(spacing*v + u) if u is a digit bit, and the plain sum A[v][q]
// weighs 2^(spacing*v) * (1 + sum of 2^(rkb + i) over the set bits i of q that are digit bits).
template <class G>
int check_chain(const typename G::Jac& gen, const char* group) {
    using Jac = typename G::Jac;
    const Shape shapes[] = {
        {"plain", 5, 7, 7, 0, 8, 7},
        {"pseudo-windows", 4, 7, 5, 2, 8, 7},
        {"top_bits < kb", 4, 7, 7, 0, 8, 3},
        {"pseudo-windows, top_bits < kb", 3, 7, 5, 2, 8, 6},
        {"window-table spacing (tf = 3, c = 4)", 3, 3, 3, 0, 12, 3},
    };
    std::vector<Jac> small(8);  // c * gen, c < 8
    for (uint64_t c = 0; c < small.size(); c++) small[c] = smul<G>(gen, c);
    int failures = 0;
    for (const Shape& s : shapes) {
        const uint32_t PW = 1u << s.pw_bits;
        const uint32_t npos = s.spacing * (s.V - 1) + s.kb;
        std::vector<uint32_t> qsums((size_t)s.V * PW * (s.rkb + 1) * G::JAC_WORDS);
        std::vector<uint64_t> coef(npos, 0);  // the expected result is sum_e coef[e] * 2^e * gen
        auto digit_bit = [&](uint32_t v, uint32_t j) { return j < s.kb && (v + 1 < s.V || j < s.top_bits); };
        for (uint32_t v = 0; v < s.V; v++)
            for (uint32_t q = 0; q < PW; q++)
                for (uint32_t u = 0; u <= s.rkb; u++) {
                    const uint64_t c = (v * 5 + q * 3 + u * 7 + 1) % 8;
                    G::store_jac(qsums.data() + ((size_t)(v * PW + q) * (s.rkb + 1) + u) * G::JAC_WORDS, small[c]);
                    const uint32_t e0 = s.spacing * v;
                    if (u < s.rkb) {
                        if (digit_bit(v, u)) coef[e0 + u] += c;
                        continue;
                    }
                    coef[e0] += c;  // A[v][q]
                    for (uint32_t i = 0; i < s.pw_bits; i++)
                        if (((q >> i) & 1u) && digit_bit(v, s.rkb + i)) coef[e0 + s.rkb + i] += c;
                }
        Jac want = G::identity(), pow2 = gen;  // pow2 = 2^e * gen
        for (uint32_t e = 0; e < npos; e++, pow2 = G::jdbl(pow2)) want = G::jadd(want, smul<G>(pow2, coef[e]));
        for (int workers : {0, 1, 3}) {
            HostPool* pool = workers ? new HostPool(workers) : nullptr;
            const Jac got = host_finish_chain<G>(qsums.data(), s.V, s.kb, s.rkb, s.pw_bits, s.spacing, s.top_bits, pool);
            delete pool;
            if (!same_point<G>(got, want)) {
                std::printf("FAIL: %s chain, shape \"%s\", %d pool workers\n", group, s.name, workers);
                failures++;
            }
        }
    }
    return failures;
}

// The fold of partials as msm_bn254_g*_combine runs it, and its outputs (G1's rule for both groups: without MSM_FLAG_DETERMINISTIC an
// identity is handed out as the Z = 0 representative the fold holds)
template <class G>
int check_combine(const typename G::Jac& gen, const char* group) {
    using Jac = typename G::Jac;
    int failures = 0;
    auto check = [&](bool ok, const char* what) {
        if (!ok) {
            std::printf("FAIL: %s combine: %s\n", group, what);
            failures++;
        }
    };
    uint32_t jac[G::JAC_WORDS], aff[G::AFF_WORDS], want_jac[G::JAC_WORDS], want_aff[G::AFF_WORDS];
    uint8_t inf = 7;
    check(combine_partials<G>(nullptr, 1, jac, aff, &inf, false) == MSM_ERR_BAD_ARG, "no partials");
    std::vector<uint32_t> parts(4 * G::JAC_WORDS);
    check(combine_partials<G>(parts.data(), 0, jac, aff, &inf, false) == MSM_ERR_EMPTY, "k = 0");
    // 5G + 0 + 7G + 3G (Z != 1 representatives from the double-and-add)
    const Jac terms[4] = {smul<G>(gen, 5), G::identity(), smul<G>(gen, 7), smul<G>(gen, 3)};
    for (int i = 0; i < 4; i++) G::store_jac(parts.data() + i * G::JAC_WORDS, terms[i]);
    const Jac p15 = smul<G>(gen, 15);
    typename G::F x, y;
    check(!G::to_affine_std(p15, x, y), "15G is not the identity");
    G::store_words(want_aff, x);
    G::store_words(want_aff + G::AFF_WORDS / 2, y);
    for (bool canonical : {false, true}) {
        check(combine_partials<G>(parts.data(), 4, jac, aff, &inf, canonical) == MSM_OK, "k = 4");
        check(same_point<G>(G::load_jac(jac), p15) && inf == 0, "k = 4: Jacobian result");
        check(std::memcmp(aff, want_aff, sizeof aff) == 0, "k = 4: affine result");
        if (canonical) {
            G::store_jac(want_jac, G::normalize(p15));
            check(std::memcmp(jac, want_jac, sizeof jac) == 0, "k = 4: the Z = 1 representative");
        }
        check(combine_partials<G>(parts.data(), 4, nullptr, aff, &inf, canonical) == MSM_OK && std::memcmp(aff, want_aff, sizeof aff) == 0,
              "k = 4: affine result alone");
    }
    // the identity as a Z = 0 partial whose X, Y are not those of G::identity()
    Jac odd = terms[2];
    odd.z = typename G::F{};
    G::store_jac(parts.data(), odd);
    std::memset(aff, 0xFF, sizeof aff);
    check(combine_partials<G>(parts.data(), 1, jac, aff, &inf, false) == MSM_OK && inf == 1, "identity");
    check(std::memcmp(jac, parts.data(), sizeof jac) == 0, "identity: its own words without the flag");
    std::memset(want_aff, 0, sizeof want_aff);
    check(std::memcmp(aff, want_aff, sizeof aff) == 0, "identity: affine (0, 0)");
    check(combine_partials<G>(parts.data(), 1, jac, aff, &inf, true) == MSM_OK && inf == 1, "identity, canonical");
    G::store_jac(want_jac, G::identity());
    check(std::memcmp(jac, want_jac, sizeof jac) == 0, "identity: G::identity() with the flag");
    return failures;
}

}  // namespace finishcheck
