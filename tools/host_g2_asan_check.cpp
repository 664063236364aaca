// HOST-only AddressSanitizer + UBSan check of host_g2.hpp (the G2 arithmetic that finishes and folds G2 MSMs) and of the G2 finish itself
// (host_finish.hpp): `make -C gpu-acceleration_amd/csrc asan-g2`, run by tests/test_host_g2_asan.py.  Fixed inputs, known answers derived
// inside the group (k * G by double-and-add):
//   * partial folds through combine_partials<HostG2>, as msm_bn254_g2_combine runs them (k = 1, 2, 5; the identity, P + (-P), P + P), on
//     Jacobian representatives with Z != 1, and its outputs (tools/host_finish_check.hpp);
//   * the Horner chain of the CPU finish, host_finish_chain<HostG2>, over bit sums of several shapes (tools/host_finish_check.hpp);
//   * affine conversion of the results onto the twist y^2 = x^3 + 3/(9+u).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_g2.hpp"
#include "../../tools/host_finish_check.hpp"

using hostg1::Fq;
using namespace hostg2;

static int failures = 0;
#define CHECK(c, what)                                              \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAIL: %s (line %d)\n", what, __LINE__);    \
            failures++;                                             \
        }                                                           \
    } while (0)

static Fq fq_hex(const char* h) {  // 64 hex digits, big-endian
    Fq r{{0, 0, 0, 0}};
    for (int i = 0; i < 64; i++) {
        const char ch = h[i];
        const uint64_t d = ch <= '9' ? (uint64_t)(ch - '0') : (uint64_t)(ch - 'a' + 10);
        const int bit = 4 * (63 - i);
        r.l[bit / 64] |= d << (bit % 64);
    }
    return hostg1::to_mont(r);
}
static bool same_point(const Jac& a, const Jac& b) { return finishcheck::same_point<HostG2>(a, b); }
static Jac smul(const Jac& p, uint64_t k) { return finishcheck::smul<HostG2>(p, k); }
static Jac rescale(const Jac& p, const Fq2& z) {  // the same point with Z multiplied by z
    const Fq2 z2 = sqr(z);
    return Jac{mul(p.x, z2), mul(p.y, mul(z2, z)), mul(p.z, z)};
}
static bool on_twist(const Jac& p) {
    Fq2 x, y;
    if (to_affine_std(p, x, y)) return true;
    // back to Montgomery form, then y^2 - x^3 == 3 / (9 + u)
    const Fq2 xm{hostg1::to_mont(x.c0), hostg1::to_mont(x.c1)}, ym{hostg1::to_mont(y.c0), hostg1::to_mont(y.c1)};
    const Fq three = hostg1::to_mont(Fq{{3, 0, 0, 0}}), nine = hostg1::to_mont(Fq{{9, 0, 0, 0}});
    const Fq2 b = mul(Fq2{three, Fq{{0, 0, 0, 0}}}, inv(Fq2{nine, hostg1::ONE}));
    const Fq2 lhs = sub(sqr(ym), mul(sqr(xm), xm));
    return std::memcmp(&lhs, &b, sizeof b) == 0;
}

int main() {
    const Jac G{{fq_hex("1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed"),
                 fq_hex("198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2")},
                {fq_hex("12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa"),
                 fq_hex("090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b")},
                one()};
    CHECK(on_twist(G), "generator on the twist");
    const Fq2 z1{hostg1::to_mont(Fq{{12345, 0, 0, 0}}), hostg1::to_mont(Fq{{678, 1, 0, 0}})};
    const Fq2 z2{hostg1::to_mont(Fq{{99, 0, 7, 0}}), hostg1::to_mont(Fq{{5, 0, 0, 3}})};
    // folds of partials through their 48-word images, by msm_bn254_g2_combine's code
    auto fold = [](const std::vector<Jac>& parts) {
        std::vector<uint32_t> w(parts.size() * 48);
        for (size_t i = 0; i < parts.size(); i++) store_jac(w.data() + 48 * i, parts[i]);
        uint32_t out[48];
        uint8_t inf = 2;
        CHECK(combine_partials<HostG2>(w.data(), parts.size(), out, nullptr, &inf, false) == MSM_OK, "combine_partials<HostG2>");
        const Jac t = load_jac(out);
        CHECK(inf == (is_identity(t) ? 1 : 0), "out_inf");
        return t;
    };
    const Jac p5 = smul(G, 5), p7 = smul(G, 7);
    CHECK(same_point(fold({rescale(p5, z1)}), p5), "k = 1");
    CHECK(same_point(fold({rescale(p5, z1), rescale(p7, z2)}), smul(G, 12)), "k = 2");
    CHECK(same_point(fold({p5, identity(), rescale(p7, z2), rescale(p5, z1), smul(G, 3)}), smul(G, 20)), "k = 5 with the identity");
    const Jac neg5{p5.x, sub(zero(), p5.y), p5.z};
    CHECK(is_identity(fold({rescale(p5, z2), neg5})), "P + (-P)");
    CHECK(same_point(fold({rescale(p7, z1), rescale(p7, z2)}), smul(G, 14)), "P + P through jadd");
    CHECK(same_point(jdbl(p7), smul(G, 14)), "jdbl");
    CHECK(on_twist(fold({rescale(p5, z1), rescale(p7, z2)})), "fold result on the twist");
    failures += finishcheck::check_chain<HostG2>(G, "G2") + finishcheck::check_combine<HostG2>(G, "G2");
    Fq2 x, y;
    CHECK(to_affine_std(identity(), x, y) && is_zero(x) && is_zero(y), "identity -> (0, 0)");
    // compress_point (msm_bn254_g2_compress): x bytes, the infinity bit, and the order of y -- c1 first, then c0; 0 is not larger
    {
        uint32_t w[32], ws[32];
        store_words(w, G.x), store_words(w + 16, G.y);
        store_words(ws, from_mont(G.x)), store_words(ws + 16, from_mont(G.y));
        uint8_t im[64], is_[64], in_[64], inf[64];
        compress_point(w, true, false, im);
        compress_point(ws, false, false, is_);
        CHECK(std::memcmp(im, is_, 64) == 0 && std::memcmp(im, ws, 63) == 0, "compress: both forms agree, x in standard form");
        CHECK((im[63] & 0x40) == 0, "compress: no infinity bit");
        store_words(w + 16, sub(zero(), G.y));
        compress_point(w, true, false, in_);
        CHECK(std::memcmp(im, in_, 63) == 0 && ((im[63] ^ in_[63]) == 0x80), "compress: y and -y differ in bit 7 alone");
        compress_point(w, true, true, inf);
        bool zeros = inf[63] == 0x40;
        for (int i = 0; i < 63; i++) zeros = zeros && inf[i] == 0;
        CHECK(zeros, "compress: infinity");
        auto larger = [&](uint64_t c0, uint64_t c1, bool neg0, bool neg1) {
            Fq a{{c0, 0, 0, 0}}, b{{c1, 0, 0, 0}};
            if (neg0) a = hostg1::sub(Fq{{0, 0, 0, 0}}, hostg1::to_mont(a)), a = hostg1::from_mont(a);
            if (neg1) b = hostg1::sub(Fq{{0, 0, 0, 0}}, hostg1::to_mont(b)), b = hostg1::from_mont(b);
            uint32_t v[32] = {};
            hostg1::store_words(v + 16, a), hostg1::store_words(v + 24, b);
            uint8_t o[64];
            compress_point(v, false, false, o);
            return (o[63] & 0x80) != 0;
        };
        CHECK(!larger(0, 0, false, false) && !larger(1, 0, false, false) && larger(1, 0, true, false), "compress: c1 = 0, c0 decides");
        CHECK(!larger(1, 1, true, false) && larger(1, 1, false, true) && !larger(0, 1, false, false) && larger(0, 1, false, true), "compress: c1 decides");
    }
    if (failures) return 1;
    std::printf("host_g2.hpp: folds, Horner chain, combine outputs, affine conversion, compressed images -- clean under ASan/UBSan\n");
    return 0;
}
