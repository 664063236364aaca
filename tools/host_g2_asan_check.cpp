// HOST-only AddressSanitizer + UBSan check of host_g2.hpp (the G2 arithmetic that finishes and folds G2 MSMs): `make -C gpu-acceleration_amd/csrc
// asan-g2`, run by tests/test_host_g2_asan.py.  Fixed inputs, known answers derived inside the group (k * G by double-and-add):
//   * partial folds as msm_bn254_g2_combine does them (k = 1, 2, 5; the identity, P + (-P), P + P), on Jacobian representatives with Z != 1;
//   * a Horner chain sum_u 2^u * (c_u G) -- the shape of the CPU finish over the bit sums -- against (sum_u 2^u c_u) * G;
//   * affine conversion of the results onto the twist y^2 = x^3 + 3/(9+u).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_g2.hpp"

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
static bool same_point(const Jac& a, const Jac& b) {
    if (is_identity(a) || is_identity(b)) return is_identity(a) && is_identity(b);
    const Jac na = normalize(a), nb = normalize(b);
    return std::memcmp(&na, &nb, sizeof na) == 0;
}
static Jac smul(const Jac& p, uint64_t k) {
    Jac acc = identity(), base = p;
    for (; k; k >>= 1) {
        if (k & 1) acc = jadd(acc, base);
        base = jdbl(base);
    }
    return acc;
}
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
    // folds of partials through their 48-word images, as msm_bn254_g2_combine reads them
    auto fold = [](const std::vector<Jac>& parts) {
        std::vector<uint32_t> w(parts.size() * 48);
        for (size_t i = 0; i < parts.size(); i++) store_jac(w.data() + 48 * i, parts[i]);
        Jac t = identity();
        for (size_t i = 0; i < parts.size(); i++) t = jadd(t, load_jac(w.data() + 48 * i));
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
    // Horner chain over 40 positions with small multiples as the terms
    Jac acc = identity();
    uint64_t want = 0;
    for (int u = 39; u >= 0; u--) {
        acc = jdbl(acc);
        const uint64_t c = (uint64_t)((u * 7 + 3) % 5);
        if (c) acc = jadd(acc, rescale(smul(G, c), u & 1 ? z1 : z2));
        want += c << u;
    }
    CHECK(same_point(acc, smul(G, want)), "Horner chain");
    CHECK(on_twist(acc), "chain result on the twist");
    Fq2 x, y;
    CHECK(to_affine_std(identity(), x, y) && is_zero(x) && is_zero(y), "identity -> (0, 0)");
    if (failures) return 1;
    std::printf("host_g2.hpp: folds, Horner chain, affine conversion -- clean under ASan/UBSan\n");
    return 0;
}
