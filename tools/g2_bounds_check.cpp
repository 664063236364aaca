// tools/g2_bounds_check.cpp -- host build of the DEVICE G2 group law (fp2_bn254.hpp / ec_g2_bn254.hpp are __host__ __device__) with every
// limb-range assumption of the lazily reduced 9 x 29-bit arithmetic asserted (-DFP_BOUNDS_CHECK): subtrahend limbs never exceed the K*p pad,
// normalisation never overflows a limb, no Montgomery column leaves 64 bits, values stay below 2^261.  The G2 counterpart of
// tools/fp_bounds_check.cpp; run by tests/test_g2_bounds.py.
//   A. fp2_mul<K> / fp2_sqr<K> / fp2_sub<K> / fp2_neg<K> / fp2_mul_fp for every K the G2 code instantiates, the pad-limited operand canonical and
//      as the largest representative below (K-1)p, components 0, 1, p-1 and 2p (a representative of 0), against the independent 4 x 64-bit
//      arithmetic of host_g2.hpp
//   B. xyzz2_madd / xyzz2_dbl / xyzz2_add on operands at the TOP of the documented ranges (X + 11p, Y + 7p, ZZ + 3p, ZZZ + 3p; affine y and
//      2p - y): same residues as on the reduced operands, outputs normalised and back inside X < 12p, Y < 8p, ZZ, ZZZ < 4.2p -- the closure
//      the header claims ("every function below re-establishes these")
//   C. the special cases on consistent records (ZZ = t^2, ZZZ = t^3), reduced and inflated: identity operands in both encodings, P + P with the
//      same and with a rescaled record, P + (-P), the doubling and the cancelling branch of the mixed addition, a negated y with a zero
//      component (exactly 2p) -- every result against the host's Jacobian law
//   D. long mixed chains of madd / add / dbl: the bounds under composition, the end of every chain against the host's law
// The group law is a set of rational identities in the coordinates: none of B, C, D needs its operands on the twist.
// Build+run:  hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --cuda-host-only tools/g2_bounds_check.cpp -o g2_bounds_check && ./g2_bounds_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../gpu-acceleration_amd/csrc/ec_g2_bn254.hpp"
#include "../gpu-acceleration_amd/csrc/host_g2.hpp"
using namespace bn254;
using hostg2::Fq2;

static std::mt19937_64 rng(0xB2540262);
static long checks = 0;

#define REQUIRE(cond, ...)                    \
    do {                                      \
        if (!(cond)) {                        \
            std::printf("FAILED: " __VA_ARGS__); \
            std::printf("\n");                \
            std::exit(1);                     \
        }                                     \
    } while (0)

// ---- operands ------------------------------------------------------------------------------------------------------------------------------
static fp rand_canonical() {  // uniform below p, as limbs
    const uint32_t P[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    uint32_t w[8];
    for (;;) {
        for (int i = 0; i < 8; i++) w[i] = (uint32_t)rng();
        w[7] &= 0x3FFFFFFFu;
        bool lt = false;
        for (int i = 7; i >= 0; i--)
            if (w[i] != P[i]) {
                lt = w[i] < P[i];
                break;
            }
        if (lt) return fp_unpack(w);
    }
}
static fp add_kp(fp a, int k) {  // a + k*p, limbs re-normalised: the same residue, a larger representative
    for (int j = 0; j < k; j++) {
        for (int i = 0; i < 9; i++) a.v[i] += FP29_P[i];
        a = fp_normalize(a);
    }
    return a;
}
static fp2 add_kp2(const fp2& a, int k) { return fp2{add_kp(a.c0, k), add_kp(a.c1, k)}; }
static fp small_int(uint32_t v) {
    fp r = fp_zero();
    r.v[0] = v;
    return r;
}
static fp p_minus_1() {
    fp r = fp_const(FP29_P);
    r.v[0] -= 1;
    return r;
}
// the component values that sit on an edge of the limb arithmetic, as INTEGERS in the limbs: 0, 1, p - 1, 2^261 mod p, then random ones.
// (2p, a representative of 0, is added by the callers where the pad allows it.)
constexpr int N_EDGE = 6;  // 4 named edge values + 2 random ones
static_assert(N_EDGE >= 4, "edge() names four edge values: every one of them must have a selector");
static fp edge(int sel) {
    switch (sel) {
        case 0: return fp_zero();
        case 1: return small_int(1);
        case 2: return p_minus_1();
        case 3: return fp_one();
        default: return rand_canonical();  // selectors 4 .. N_EDGE - 1: random values (a larger N_EDGE only adds random ones)
    }
}
static fp free_operand() {  // an operand no pad limits: an edge value or a random one, on a representative up to 13p above it
    static const int infl[4] = {0, 1, 7, 13};
    return add_kp(edge((int)(rng() % N_EDGE)), infl[rng() % 4]);
}
// A K*p pad has 2^29 - 1 of slack in every limb below the top one and none in the top limb (fp2_make_pads): a subtrahend passes it limb by limb up
// to within about 2^232 (3e-7 p) of K*p itself.  Only a value within that sliver of the top of its documented range can tell a pad that is one p
// too small, so the worst-case operands are residues just below p, which the inflation then lifts to 12p - d, 8p - d, 4p - d, 2p - d.
static fp near_p() {
    fp r = p_minus_1();
    r.v[0] -= (uint32_t)(rng() % (1u << 20));
    return r;
}
static bool all_near_p = false;  // (part B: every component of every operand at the top at once)
static fp rand_or_top() { return (all_near_p || rng() % 4 == 0) ? near_p() : rand_canonical(); }
static fp2 rand_fp2() { return fp2{rand_or_top(), rand_or_top()}; }
static fp2 rand_fp2_nonzero() {
    for (;;) {
        const fp2 a = rand_fp2();
        if (!fp2_is_zero_exact(a)) return a;
    }
}

// ---- the independent side: R = 2^256 Montgomery words on 4 x 64-bit limbs -----------------------------------------------------------------
static hostg1::Fq H(const fp& a) {
    uint32_t w[8];
    fp_to_mont256(w, a);
    return hostg1::load_words(w);
}
static Fq2 H(const fp2& a) { return Fq2{H(a.c0), H(a.c1)}; }
static bool same(const hostg1::Fq& a, const hostg1::Fq& b) { return a.l[0] == b.l[0] && a.l[1] == b.l[1] && a.l[2] == b.l[2] && a.l[3] == b.l[3]; }
static bool same(const Fq2& a, const Fq2& b) { return same(a.c0, b.c0) && same(a.c1, b.c1); }
static bool normalised(const fp& a) {
    for (int i = 0; i < 9; i++)
        if (a.v[i] > FP_MASK) return false;
    return true;
}
static bool normalised(const fp2& a) { return normalised(a.c0) && normalised(a.c1); }

// ---- exact comparison of a limb value with a rational multiple of p: den * a < num * p -----------------------------------------------------
struct U320 {
    uint64_t w[5];
};
static U320 scaled(const uint32_t v[9], uint32_t by) {  // by < 2^5, limbs < 2^32
    U320 r{};
    for (int i = 0; i < 9; i++) {
        const unsigned __int128 t = (unsigned __int128)((uint64_t)v[i] * by) << ((29 * i) % 64);
        int k = (29 * i) / 64;
        unsigned __int128 c = t;
        while (c != 0 && k < 5) {
            c += r.w[k];
            r.w[k] = (uint64_t)c;
            c >>= 64;
            k++;
        }
    }
    return r;
}
static bool below(const fp& a, uint32_t num, uint32_t den) {
    const U320 x = scaled(a.v, den), y = scaled(FP29_P, num);
    for (int k = 4; k >= 0; k--)
        if (x.w[k] != y.w[k]) return x.w[k] < y.w[k];
    return false;
}
static long double multiple_of_p(const fp& a) {
    long double v = 0, p = 0;
    for (int i = 8; i >= 0; i--) v = v * 536870912.0L + a.v[i], p = p * 536870912.0L + FP29_P[i];
    return v / p;
}

// ---- the header's own bounds, and the largest representative met per coordinate ------------------------------------------------------------
static long double seen_max[4] = {0, 0, 0, 0};  // X, Y, ZZ, ZZZ: over the outputs the functions COMPUTED
static void within_bounds(const xyzz2& r, const char* what, bool computed = true) {  // computed: r is a function's own output, not an operand handed back
    const fp2* c[4] = {&r.x, &r.y, &r.zz, &r.zzz};
    static const uint32_t num[4] = {12, 8, 21, 21}, den[4] = {1, 1, 5, 5};  // X < 12p, Y < 8p, ZZ < 4.2p, ZZZ < 4.2p
    static const char* name[4] = {"X", "Y", "ZZ", "ZZZ"};
    for (int k = 0; k < 4; k++) {
        REQUIRE(normalised(*c[k]), "%s: %s is not normalised", what, name[k]);
        for (const fp* f : {&c[k]->c0, &c[k]->c1}) {
            REQUIRE(below(*f, num[k], den[k]), "%s: %s = %.3Lf p leaves the documented bound %.1f p", what, name[k], multiple_of_p(*f),
                    (double)num[k] / den[k]);
            const long double m = multiple_of_p(*f);
            if (computed && m > seen_max[k]) seen_max[k] = m;
        }
    }
    checks++;
}
static bool same_residues(const xyzz2& a, const xyzz2& b) {
    return same(H(a.x), H(b.x)) && same(H(a.y), H(b.y)) && same(H(a.zz), H(b.zz)) && same(H(a.zzz), H(b.zzz)) &&
           xyzz2_is_identity(a) == xyzz2_is_identity(b);
}
static bool exact_identity_pattern(const xyzz2& r) {  // what xyzz2_identity() writes: (1, 1, 0, 0), limb for limb
    return fp_eq_exact(r.x.c0, FP29_ONE) && fp_is_zero_exact(r.x.c1) && fp_eq_exact(r.y.c0, FP29_ONE) && fp_is_zero_exact(r.y.c1) &&
           fp2_is_zero_exact(r.zz) && fp2_is_zero_exact(r.zzz);
}
static xyzz2 inflate(const xyzz2& a) {  // to the top of the documented ranges: X + 11p < 12p, Y + 7p < 8p, ZZ + 3p, ZZZ + 3p < 4p
    if (xyzz2_is_identity(a)) return a;
    return xyzz2{add_kp2(a.x, 11), add_kp2(a.y, 7), add_kp2(a.zz, 3), add_kp2(a.zzz, 3)};
}
static xyzz2 zero_record() { return xyzz2{fp2_zero(), fp2_zero(), fp2_zero(), fp2_zero()}; }  // the identity as k_g2_clear_empty writes it

// ---- the host's law on affine pairs --------------------------------------------------------------------------------------------------------
struct HA {
    Fq2 x, y;
    bool inf;
};
static HA haff(const xyzz2& p) {
    if (xyzz2_is_identity(p)) return HA{hostg2::zero(), hostg2::zero(), true};
    return HA{hostg2::mul(H(p.x), hostg2::inv(H(p.zz))), hostg2::mul(H(p.y), hostg2::inv(H(p.zzz))), false};
}
static HA haff(const affine2& q) { return HA{H(q.x), H(q.y), false}; }
static hostg2::Jac hjac(const HA& a) { return a.inf ? hostg2::identity() : hostg2::Jac{a.x, a.y, hostg2::one()}; }
static HA hfrom(const hostg2::Jac& j) {
    if (hostg2::is_identity(j)) return HA{hostg2::zero(), hostg2::zero(), true};
    const hostg2::Jac n = hostg2::normalize(j);
    return HA{n.x, n.y, false};
}
static HA hadd(const HA& a, const HA& b) { return hfrom(hostg2::jadd(hjac(a), hjac(b))); }
static HA hdbl(const HA& a) { return hfrom(hostg2::jdbl(hjac(a))); }
static bool same(const HA& a, const HA& b) { return a.inf == b.inf && (a.inf || (same(a.x, b.x) && same(a.y, b.y))); }
static bool consistent(const xyzz2& p) {  // ZZ^3 == ZZZ^2
    if (xyzz2_is_identity(p)) return true;
    const Fq2 zz = H(p.zz), zzz = H(p.zzz);
    return same(hostg2::mul(hostg2::sqr(zz), zz), hostg2::sqr(zzz));
}
// the record (x t^2, y t^3, t^2, t^3) of the affine pair q, canonical components
static fp2 canonical2(const fp2& a) { return fp2{fp_canonical(a.c0), fp_canonical(a.c1)}; }
static xyzz2 record_of(const affine2& q, const fp2& t) {
    const fp2 t2 = canonical2(fp2_sqr<3>(t)), t3 = canonical2(fp2_mul<3>(t2, t));
    return xyzz2{canonical2(fp2_mul<3>(q.x, t2)), canonical2(fp2_mul<3>(q.y, t3)), t2, t3};
}
static affine2 rand_affine() { return affine2{rand_fp2(), rand_fp2_nonzero()}; }
static affine2 negated(const affine2& q) { return affine2{q.x, fp2_neg<2>(q.y)}; }           // 2p - y, as k_g2_accumulate hands it over
static affine2 negated_canonical(const affine2& q) { return affine2{q.x, canonical2(fp2_neg<2>(q.y))}; }

// ============================================================================================================================================
// A. the Fq2 operations.  K values instantiated by the G2 code (ec_g2_bn254.hpp, msm_kernels_g2.hpp, g2_points_bn254.hpp, msm_kernels_g2_points.hpp,
//    fixed_base_g2_bn254.hpp) -- a new K in any of them belongs in the lists of part_a() below:
//      fp2_mul<K>  3 4 6 7 9 10 13 15 16 17
//      fp2_sqr<K>  3 5 6 12 13 15 16 17
//      fp2_sub<K>  3 5 6 7 8 9 12 13
//      fp2_neg<K>  2                      (and fp_neg_raw_k<6>, <9>, <13> of the conjugations, checked here as fp2_neg<6>, <9>, <13>)
// The pad-limited operand (b.c1 of a product, a.c1 of a square, b of a difference or a negation) must stay below (K-1)p: it is given canonical
// and on the largest representative below (K-1)p, i.e. + (K-2)p; 2p itself where 2p < (K-1)p.
template <int K>
static int limited_count() { return 2 * N_EDGE + (K >= 4 ? 1 : 0); }
template <int K>
static fp limited(int sel) {
    if (sel == 2 * N_EDGE) return add_kp(fp_zero(), 2);                  // 2p: what fp2_neg<2> makes of a zero component
    return add_kp(edge(sel % N_EDGE), sel < N_EDGE ? 0 : K - 2);       // canonical, or the top representative below (K-1)p
}
constexpr int REPS = 24;
template <int K>
static void check_mul() {
    for (int sel = 0; sel < limited_count<K>(); sel++)
        for (int rep = 0; rep < REPS; rep++) {
            const fp2 a{free_operand(), free_operand()}, b{rep & 1 ? limited<K>((int)(rng() % limited_count<K>())) : free_operand(), limited<K>(sel)};
            const fp2 r = fp2_mul<K>(a, b);
            REQUIRE(normalised(r), "fp2_mul<%d>: result not normalised", K);
            REQUIRE(same(H(r), hostg2::mul(H(a), H(b))), "fp2_mul<%d> differs from the host product (b.c1 = %.3Lf p)", K, multiple_of_p(b.c1));
            checks++;
        }
}
template <int K>
static void check_sqr() {
    for (int sel = 0; sel < limited_count<K>(); sel++)
        for (int rep = 0; rep < REPS; rep++) {
            const fp2 a{rep & 1 ? limited<K>((int)(rng() % limited_count<K>())) : free_operand(), limited<K>(sel)};
            const fp2 r = fp2_sqr<K>(a);
            REQUIRE(normalised(r), "fp2_sqr<%d>: result not normalised", K);
            REQUIRE(same(H(r), hostg2::sqr(H(a))), "fp2_sqr<%d> differs from the host square (a.c1 = %.3Lf p)", K, multiple_of_p(a.c1));
            checks++;
        }
}
template <int K>
static void check_sub() {
    for (int s0 = 0; s0 < limited_count<K>(); s0++)
        for (int s1 = 0; s1 < limited_count<K>(); s1++)
            for (int rep = 0; rep < 2; rep++) {
                const fp2 a{free_operand(), free_operand()}, b{limited<K>(s0), limited<K>(s1)};
                const fp2 r = fp2_sub<K>(a, b);
                REQUIRE(normalised(r), "fp2_sub<%d>: result not normalised", K);
                REQUIRE(same(H(r), hostg2::sub(H(a), H(b))), "fp2_sub<%d> differs from the host difference", K);
                checks++;
            }
}
template <int K>
static void check_neg() {
    for (int s0 = 0; s0 < limited_count<K>(); s0++)
        for (int s1 = 0; s1 < limited_count<K>(); s1++) {
            const fp2 b{limited<K>(s0), limited<K>(s1)};
            const fp2 r = fp2_neg<K>(b);
            REQUIRE(normalised(r), "fp2_neg<%d>: result not normalised", K);
            REQUIRE(same(H(r), hostg2::sub(hostg2::zero(), H(b))), "fp2_neg<%d> differs from the host negation", K);
            checks++;
        }
}
static void part_a() {
    check_mul<3>(), check_mul<4>(), check_mul<6>(), check_mul<7>(), check_mul<9>(), check_mul<10>(), check_mul<13>(), check_mul<15>(), check_mul<16>(),
        check_mul<17>();
    check_sqr<3>(), check_sqr<5>(), check_sqr<6>(), check_sqr<12>(), check_sqr<13>(), check_sqr<15>(), check_sqr<16>(), check_sqr<17>();
    check_sub<3>(), check_sub<5>(), check_sub<6>(), check_sub<7>(), check_sub<8>(), check_sub<9>(), check_sub<12>(), check_sub<13>();
    check_neg<2>(), check_neg<6>(), check_neg<9>(), check_neg<13>();
    {   // fp2_neg<2> of a canonical y with a zero component is EXACTLY 2p in that component
        const fp2 n = fp2_neg<2>(fp2{fp_zero(), rand_canonical()});
        const fp two_p = add_kp(fp_zero(), 2);
        for (int i = 0; i < 9; i++) REQUIRE(n.c0.v[i] == two_p.v[i], "fp2_neg<2>(0) is not 2p");
    }
    for (int rep = 0; rep < 40 * N_EDGE; rep++) {  // by an Fq element: a up to the X bound, s an edge value or a random one below 2p
        const fp2 a{free_operand(), free_operand()};
        const fp s = add_kp(edge(rep % N_EDGE), (rep / N_EDGE) & 1);
        const fp2 r = fp2_mul_fp(a, s);
        REQUIRE(normalised(r), "fp2_mul_fp: result not normalised");
        REQUIRE(same(H(r.c0), hostg1::mul(H(a.c0), H(s))) && same(H(r.c1), hostg1::mul(H(a.c1), H(s))), "fp2_mul_fp differs from the host products");
        checks++;
    }
}

// ============================================================================================================================================
// B. worst-case representatives on arbitrary field values
static void part_b(int iterations) {
    for (int it = 0; it < iterations; it++) {
        all_near_p = it % 8 == 0;
        // ZZ = 0 is the identity marker, never a value: ZZ, ZZZ are kept non-zero.  Every few iterations a component of the affine y is zero, so
        // that its negation is exactly 2p.
        const xyzz2 a{rand_fp2(), rand_fp2(), rand_fp2_nonzero(), rand_fp2_nonzero()}, b{rand_fp2(), rand_fp2(), rand_fp2_nonzero(), rand_fp2_nonzero()};
        const xyzz2 ai = inflate(a), bi = inflate(b);
        affine2 q = rand_affine();
        if (it % 7 == 0) q.y.c0 = fp_zero();
        if (it % 11 == 0) q.y.c1 = fp_zero();
        if (fp2_is_zero_exact(q.y)) q.y.c0 = small_int(1);
        for (const affine2& qq : {q, negated(q)}) {
            xyzz2 r1 = a, r2 = ai;
            xyzz2_madd(r1, qq);
            xyzz2_madd(r2, qq);
            within_bounds(r1, "madd (reduced)");
            within_bounds(r2, "madd (inflated)");
            REQUIRE(same_residues(r1, r2), "madd: inflated operands change the residues (it = %d)", it);
        }
        {
            const xyzz2 d1 = xyzz2_dbl(a), d2 = xyzz2_dbl(ai);
            within_bounds(d1, "dbl (reduced)");
            within_bounds(d2, "dbl (inflated)");
            REQUIRE(same_residues(d1, d2), "dbl: inflated operands change the residues (it = %d)", it);
        }
        {
            const xyzz2 s0 = xyzz2_add(a, b);
            within_bounds(s0, "add (reduced, reduced)");
            int mix = 0;
            for (const xyzz2& s : {xyzz2_add(ai, bi), xyzz2_add(a, bi), xyzz2_add(ai, b)}) {
                within_bounds(s, "add (inflated operands)");
                REQUIRE(same_residues(s0, s), "add: inflated operands change the residues (it = %d, mix %d)", it, mix);
                mix++;
            }
        }
    }
    all_near_p = false;
}

// ============================================================================================================================================
// C. special cases on consistent records, reduced and inflated, against the host's law
static void expect_point(const xyzz2& r, const HA& want, const char* what, bool computed = true) {
    within_bounds(r, what, computed);
    REQUIRE(consistent(r), "%s: ZZ^3 != ZZZ^2", what);
    REQUIRE(same(haff(r), want), "%s: not the host's point", what);
}
static void part_c(int iterations) {
    const xyzz2 ids[2] = {xyzz2_identity(), zero_record()};
    for (int it = 0; it < iterations; it++) {
        const affine2 p = rand_affine(), o = rand_affine();
        const fp2 t = rand_fp2_nonzero(), l = rand_fp2_nonzero();
        const HA hp = haff(p), ho = haff(o), h2p = hdbl(hp);
        REQUIRE(!h2p.inf, "2P is the identity");
        const xyzz2 rec = record_of(p, t), rec_l = record_of(p, canonical2(fp2_mul<3>(t, l)));      // the same point under another ZZ
        const xyzz2 neg_l = record_of(negated_canonical(p), canonical2(fp2_mul<3>(t, l)));          // -P under another ZZ
        const xyzz2 other = record_of(o, l);
        REQUIRE(same(haff(rec), hp) && same(haff(rec_l), hp) && consistent(rec_l), "record_of does not hold the point");
        for (int infl = 0; infl < 4; infl++) {  // bit 0: first operand inflated, bit 1: second
            const xyzz2 A = infl & 1 ? inflate(rec) : rec, A2 = infl & 2 ? inflate(rec) : rec;
            const xyzz2 B = infl & 2 ? inflate(rec_l) : rec_l, N = infl & 2 ? inflate(neg_l) : neg_l, O = infl & 2 ? inflate(other) : other;
            // an ordinary sum, for the record of the host check itself
            expect_point(xyzz2_add(A, O), hadd(hp, ho), "P + O");
            // the identity on either side and on both, in both encodings: the other operand comes back limb for limb
            for (const xyzz2& id : ids) {
                REQUIRE(same_residues(xyzz2_add(id, A), A) && same_residues(xyzz2_add(A, id), A), "identity + P is not P");
                expect_point(xyzz2_add(id, A), hp, "identity + P", false);
                expect_point(xyzz2_add(A, id), hp, "P + identity", false);
                for (const xyzz2& id2 : ids) REQUIRE(xyzz2_is_identity(xyzz2_add(id, id2)), "identity + identity is not the identity");
                REQUIRE(xyzz2_is_identity(xyzz2_dbl(id)), "2 * identity is not the identity");
                xyzz2 m = id;  // identity accumulator of the mixed addition: the affine point itself, ZZ = ZZZ = 1
                xyzz2_madd(m, infl & 2 ? negated(p) : p);
                expect_point(m, infl & 2 ? haff(negated(p)) : hp, "identity madd P");
            }
            // P + P: the same record, then another representative -- the doubling branch with DIFFERENT ZZ on the two sides
            expect_point(xyzz2_dbl(A), h2p, "dbl(P)");
            expect_point(xyzz2_add(A, A2), h2p, "P + P (same record)");
            expect_point(xyzz2_add(A, B), h2p, "P + P (rescaled record)");
            expect_point(xyzz2_add(B, A), h2p, "P + P (rescaled record, swapped)");
            // P + (-P): exactly the identity pattern
            for (const xyzz2& s : {xyzz2_add(A, N), xyzz2_add(N, A)}) {
                within_bounds(s, "P + (-P)");
                REQUIRE(exact_identity_pattern(s), "P + (-P) is not the exact identity pattern");
            }
            // the mixed addition: doubling branch, cancelling branch
            {
                xyzz2 m = A;
                xyzz2_madd(m, p);
                expect_point(m, h2p, "P madd P");
                xyzz2 c = A;
                xyzz2_madd(c, negated(p));
                within_bounds(c, "P madd (-P)");
                REQUIRE(exact_identity_pattern(c), "P madd (-P) is not the exact identity pattern");
                xyzz2 e = infl & 1 ? inflate(neg_l) : neg_l;  // -P + P with y given as it is
                xyzz2_madd(e, p);
                REQUIRE(exact_identity_pattern(e), "(-P) madd P is not the exact identity pattern");
            }
            // a negated y with a zero component: 2p - 0 = 2p exactly, the largest affine operand k_g2_accumulate can hand over
            for (int z = 0; z < 2; z++) {
                affine2 q = o;
                (z ? q.y.c1 : q.y.c0) = fp_zero();
                const affine2 qn = negated(q);
                REQUIRE(same(H(z ? qn.y.c1 : qn.y.c0), hostg1::Fq{{0, 0, 0, 0}}) && !fp_is_zero_exact(z ? qn.y.c1 : qn.y.c0), "2p - 0 is not 2p");
                xyzz2 m = A;
                xyzz2_madd(m, qn);
                expect_point(m, hadd(hp, haff(qn)), "P madd (x, 2p - y) with a zero component");
                xyzz2 d = record_of(negated_canonical(q), t);  // the same pair as accumulator: the doubling branch on a y with a component 2p
                if (infl & 1) d = inflate(d);
                xyzz2_madd(d, qn);
                expect_point(d, hdbl(haff(qn)), "doubling branch of madd, y with a component 2p");
            }
        }
    }
}

// ============================================================================================================================================
// D. long mixed chains: the bounds under composition (the records fed back are the functions' own outputs)
static void part_d(int chains, int steps) {
    for (int chain = 0; chain < chains; chain++) {
        const affine2 p0 = rand_affine();
        xyzz2 acc = chain & 1 ? inflate(record_of(p0, rand_fp2_nonzero())) : xyzz2{p0.x, p0.y, fp2_one(), fp2_one()};
        xyzz2 other = chain & 2 ? zero_record() : xyzz2_identity();
        HA hacc = haff(p0), hother{hostg2::zero(), hostg2::zero(), true};
        for (int s = 0; s < steps; s++) {
            affine2 q = rand_affine();
            if (s % 13 == 0) q.y.c0 = fp_zero();
            if (rng() & 1) q = negated(q);
            const HA hq = haff(q);
            xyzz2_madd(acc, q);
            hacc = hadd(hacc, hq);
            within_bounds(acc, "chain: madd");
            if (s % 5 == 0) {
                xyzz2_madd(other, q);
                within_bounds(other, "chain: madd (second accumulator)");
                other = xyzz2_add(other, acc);
                within_bounds(other, "chain: add");
                hother = hadd(hadd(hother, hq), hacc);
            }
            if (s % 7 == 0) {
                acc = xyzz2_dbl(acc);
                within_bounds(acc, "chain: dbl");
                hacc = hdbl(hacc);
            }
            if (s % 97 == 0) {  // the doubling branch of the full addition, on whatever representative the chain has reached
                acc = xyzz2_add(acc, acc);
                within_bounds(acc, "chain: add(acc, acc)");
                hacc = hdbl(hacc);
            }
            if (s % 61 == 60) {  // other + other through the addition, both operands the chain's own output
                other = xyzz2_add(other, other);
                within_bounds(other, "chain: add(other, other)");
                hother = hdbl(hother);
            }
        }
        REQUIRE(consistent(acc) && consistent(other), "chain %d: ZZ^3 != ZZZ^2", chain);
        REQUIRE(same(haff(acc), hacc), "chain %d: the accumulator is not the host's point", chain);
        REQUIRE(same(haff(other), hother), "chain %d: the second accumulator is not the host's point", chain);
        checks += 2;
    }
}

int main(int argc, char** argv) {
    const int scale = argc > 1 ? std::atoi(argv[1]) : 1;  // (a multiple of the default workload, for a longer soak by hand)
    part_a();
    part_b(100000 * scale);
    part_c(500 * scale);
    part_d(300 * scale, 300);
    std::printf("largest computed representative (multiples of p): X %.2Lf (< 12), Y %.2Lf (< 8), ZZ %.2Lf (< 4.2), ZZZ %.2Lf (< 4.2)\n", seen_max[0],
                seen_max[1], seen_max[2], seen_max[3]);
    std::printf("g2_bounds_check: %ld checks, no bound violated, residues identical to the 4x64 host arithmetic\n", checks);
    return 0;
}
