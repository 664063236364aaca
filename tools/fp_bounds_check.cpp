// tools/fp_bounds_check.cpp -- host build of the DEVICE field/group code (fp_bn254.hpp / ec_bn254.hpp are
// __host__ __device__) with every limb-range assumption of the lazily reduced 9 x 29-bit arithmetic asserted:
// subtrahend limbs never exceed the K*p pad, normalisation never overflows a limb, no Montgomery column leaves
// 64 bits, values stay below 2^261.  Drives long random chains of xyzz_madd / xyzz_add / xyzz_dbl (the value bounds
// do not depend on the operands being curve points) plus boundary operands, and cross-checks every field result
// against the independent 4 x 64-bit host arithmetic (host_g1.hpp).  Every group-law output of every part is asserted to be normalised and back
// inside the ranges ec_bn254.hpp documents (X < 7p, Y < 5p, ZZ, ZZZ < 2p: the closure the header claims), and parts 3 and 4 enter the doubling
// and the cancelling branch of xyzz_madd, xyzz_madd_m32 and xyzz_add with REAL equal and opposite curve points (multiples of the generator by the
// host's Jacobian law) under a second ZZ, reduced and at the top of the ranges: the operand classes tests/test_gpu_20_g1_ops.py hands the device
// through msm_test_g1_raw_op, proved legal here.  The largest representative each coordinate reached is printed on the final line.
// Build+run:  hipcc -O2 -std=c++17 -DFP_BOUNDS_CHECK -x hip --offload-arch=gfx950 tools/fp_bounds_check.cpp -o /tmp/fpchk && /tmp/fpchk
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include "../gpu-acceleration_amd/csrc/ec_bn254.hpp"
#include "../gpu-acceleration_amd/csrc/host_g1.hpp"
using namespace bn254;

static std::mt19937_64 rng(0xB254);
static void rand_words(uint32_t w[8], int mode) {
    const uint32_t P[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    if (mode == 1) { for (int i = 0; i < 8; i++) w[i] = P[i]; w[0] -= 1 + (uint32_t)(rng() % 3); return; }  // p-1..p-3
    if (mode == 2) { for (int i = 0; i < 8; i++) w[i] = 0; w[0] = (uint32_t)(rng() % 3); return; }           // 0..2
    for (;;) {
        for (int i = 0; i < 8; i++) w[i] = (uint32_t)rng();
        w[7] &= 0x3FFFFFFFu;
        bool lt = false;
        for (int i = 7; i >= 0; i--) if (w[i] != P[i]) { lt = w[i] < P[i]; break; }
        if (lt) return;
    }
}
static hostg1::Fq to_host_mont256(const fp& a) { uint32_t w[8]; fp_to_mont256(w, a); return hostg1::load_words(w); }
static bool same(const hostg1::Fq& a, const hostg1::Fq& b) { return a.l[0] == b.l[0] && a.l[1] == b.l[1] && a.l[2] == b.l[2] && a.l[3] == b.l[3]; }

static fp add_kp(fp a, int k) {  // a + k*p, limbs re-normalised: the same residue, a larger representative
    for (int j = 0; j < k; j++) {
        for (int i = 0; i < 9; i++) a.v[i] += FP29_P[i];
        a = fp_normalize(a);
    }
    return a;
}
static fp near_p() {  // p - 1 - d, d < 2^20: a residue whose inflation lands in the last sliver below the top of its range
    fp r = fp_const(FP29_P);
    r.v[0] -= 1 + (uint32_t)(rng() % (1u << 20));
    return r;
}
static bool same_residue(const fp& a, const fp& b) {
    uint32_t wa[8], wb[8];
    fp_to_mont256(wa, a);
    fp_to_mont256(wb, b);
    for (int i = 0; i < 8; i++) if (wa[i] != wb[i]) return false;
    return true;
}
static bool same_xyzz(const xyzz& a, const xyzz& b) {
    return same_residue(a.x, b.x) && same_residue(a.y, b.y) && same_residue(a.zz, b.zz) && same_residue(a.zzz, b.zzz);
}

// ---- the header's own bounds on every output, and the largest representative met per coordinate -------------------------------------------------
struct U320 {
    uint64_t w[5];
};
static U320 scaled(const uint32_t v[9], uint32_t by) {  // by < 2^5, limbs < 2^32
    U320 r{};
    for (int i = 0; i < 9; i++) {
        unsigned __int128 c = (unsigned __int128)((uint64_t)v[i] * by) << ((29 * i) % 64);
        for (int k = (29 * i) / 64; c != 0 && k < 5; k++) {
            c += r.w[k];
            r.w[k] = (uint64_t)c;
            c >>= 64;
        }
    }
    return r;
}
static bool below(const fp& a, uint32_t mult) {  // a < mult * p, exactly
    const U320 x = scaled(a.v, 1), y = scaled(FP29_P, mult);
    for (int k = 4; k >= 0; k--)
        if (x.w[k] != y.w[k]) return x.w[k] < y.w[k];
    return false;
}
static long double multiple_of_p(const fp& a) {
    long double v = 0, p = 0;
    for (int i = 8; i >= 0; i--) v = v * 536870912.0L + a.v[i], p = p * 536870912.0L + FP29_P[i];
    return v / p;
}
static long double seen_max[4] = {0, 0, 0, 0};  // X, Y, ZZ, ZZZ over the outputs the functions computed
static long bound_checks = 0;
static void within_bounds(const xyzz& r, const char* what) {
    const fp* c[4] = {&r.x, &r.y, &r.zz, &r.zzz};
    static const uint32_t bound[4] = {7, 5, 2, 2};
    static const char* name[4] = {"X", "Y", "ZZ", "ZZZ"};
    for (int k = 0; k < 4; k++) {
        for (int i = 0; i < 9; i++)
            if (c[k]->v[i] > FP_MASK) { printf("%s: limb %d of %s is not normalised\n", what, i, name[k]); exit(1); }
        if (!below(*c[k], bound[k])) { printf("%s: %s = %.4Lf p leaves the documented bound %u p\n", what, name[k], multiple_of_p(*c[k]), bound[k]); exit(1); }
        const long double m = multiple_of_p(*c[k]);
        if (m > seen_max[k]) seen_max[k] = m;
    }
    bound_checks++;
}
static xyzz inflate(const xyzz& a) {  // to the top of the documented ranges: X + 6p < 7p, Y + 4p < 5p, ZZ + p, ZZZ + p < 2p
    if (xyzz_is_identity(a)) return a;
    return xyzz{add_kp(a.x, 6), add_kp(a.y, 4), add_kp(a.zz, 1), add_kp(a.zzz, 1)};
}

// ---- real curve points: multiples of the generator by the host's Jacobian law, as device records under a chosen ZZ -----------------------------
struct HA {  // affine, R = 2^256 Montgomery, or the identity
    hostg1::Fq x, y;
    bool inf;
};
static HA hfrom(const hostg1::Jac& j) {
    if (hostg1::is_identity(j)) return HA{hostg1::Fq{{0, 0, 0, 0}}, hostg1::Fq{{0, 0, 0, 0}}, true};
    const hostg1::Jac n = hostg1::normalize(j);
    return HA{n.x, n.y, false};
}
static HA haff(const xyzz& p) {
    affine a;
    if (xyzz_to_affine(p, a)) return HA{hostg1::Fq{{0, 0, 0, 0}}, hostg1::Fq{{0, 0, 0, 0}}, true};
    return HA{to_host_mont256(a.x), to_host_mont256(a.y), false};
}
static bool same(const HA& a, const HA& b) { return a.inf == b.inf && (a.inf || (same(a.x, b.x) && same(a.y, b.y))); }
static bool consistent(const xyzz& p) {  // ZZ^3 == ZZZ^2
    if (xyzz_is_identity(p)) return true;
    const hostg1::Fq zz = to_host_mont256(p.zz), zzz = to_host_mont256(p.zzz);
    return same(hostg1::mul(hostg1::sqr(zz), zz), hostg1::sqr(zzz));
}
static fp fp_of_host(const hostg1::Fq& a) {  // canonical internal-domain limbs
    uint32_t w[8];
    hostg1::store_words(w, a);
    return fp_canonical(fp_from_mont256(w));
}
static xyzz record_of(const affine& q, const fp& t) {  // (x t^2, y t^3, t^2, t^3), canonical coordinates
    const fp t2 = fp_canonical(fp_sqr(t)), t3 = fp_canonical(fp_mul(t2, t));
    return xyzz{fp_canonical(fp_mul(q.x, t2)), fp_canonical(fp_mul(q.y, t3)), t2, t3};
}
static bool exact_identity_pattern(const xyzz& r) {  // what xyzz_identity() writes: (1, 1, 0, 0), limb for limb
    return fp_eq_exact(r.x, FP29_ONE) && fp_eq_exact(r.y, FP29_ONE) && fp_is_zero_exact(r.zz) && fp_is_zero_exact(r.zzz);
}
static void expect_point(const xyzz& r, const HA& want, const char* what, int it) {
    within_bounds(r, what);
    if (xyzz_is_identity(r) || !consistent(r) || !same(haff(r), want)) { printf("%s: not the host's point (it=%d)\n", what, it); exit(1); }
}
static void expect_identity(const xyzz& r, const char* what, int it) {
    within_bounds(r, what);
    if (!exact_identity_pattern(r)) { printf("%s: not the exact identity pattern (it=%d)\n", what, it); exit(1); }
}
static fp rand_nonzero_canonical() {
    for (;;) {
        uint32_t w[8];
        rand_words(w, 0);
        const fp t = fp_canonical(fp_from_mont256(w));
        if (!fp_is_zero_exact(t)) return t;
    }
}
// The doubling and the cancelling branch of every addition, entered with real equal and opposite points under ANOTHER ZZ (P == 0 mod p is then
// decided on values that are multiples of p without being equal limb for limb), every operand reduced and at the top of its range.
static long special_cases(int iterations) {
    long n = 0;
    const hostg1::Jac gen{hostg1::ONE, hostg1::dbl(hostg1::ONE), hostg1::ONE};  // (1, 2)
    hostg1::Jac walk = hostg1::jdbl(hostg1::jdbl(gen));
    const uint32_t PW[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    for (int it = 0; it < iterations; it++) {
        walk = hostg1::jadd(walk, it % 3 ? gen : hostg1::jdbl(walk));
        const HA hp = hfrom(walk), h2p = hfrom(hostg1::jdbl(walk));
        if (hp.inf || h2p.inf) { printf("special cases: the walk met the identity\n"); exit(1); }
        const affine p{fp_of_host(hp.x), fp_of_host(hp.y)};
        const affine pn{p.x, fp_canonical(fp_neg<2>(p.y))};  // -P, canonical
        const fp t = rand_nonzero_canonical(), l = rand_nonzero_canonical(), tl = fp_canonical(fp_mul(t, l));
        const xyzz rec = record_of(p, t), rec_l = record_of(p, tl), neg_l = record_of(pn, tl);
        if (!same(haff(rec), hp) || !same(haff(rec_l), hp) || !consistent(rec_l)) { printf("record_of does not hold the point\n"); exit(1); }
        // arkworks words of P and of -P, canonical and + p (still 256 bits)
        uint32_t wp[2][2][8], wn[2][2][8];  // [canonical / + p][x / y]
        hostg1::store_words(wp[0][0], hp.x), hostg1::store_words(wp[0][1], hp.y);
        hostg1::store_words(wn[0][0], hp.x), hostg1::store_words(wn[0][1], hostg1::sub(hostg1::Fq{{0, 0, 0, 0}}, hp.y));
        for (int c = 0; c < 2; c++) {
            uint64_t cp = 0, cn = 0;
            for (int k = 0; k < 8; k++) {
                cp += (uint64_t)wp[0][c][k] + PW[k], wp[1][c][k] = (uint32_t)cp, cp >>= 32;
                cn += (uint64_t)wn[0][c][k] + PW[k], wn[1][c][k] = (uint32_t)cn, cn >>= 32;
            }
            if (cp || cn) { printf("words + p leave 256 bits\n"); exit(1); }
        }
        for (int infl = 0; infl < 4; infl++) {  // bit 0: first operand inflated, bit 1: second
            const xyzz A = infl & 1 ? inflate(rec) : rec, A2 = infl & 2 ? inflate(rec) : rec;
            const xyzz B = infl & 2 ? inflate(rec_l) : rec_l, N = infl & 2 ? inflate(neg_l) : neg_l;
            // xyzz_add and xyzz_dbl
            expect_point(xyzz_dbl(A), h2p, "dbl(P)", it);
            expect_point(xyzz_add(A, A2), h2p, "P + P (same ZZ)", it);
            expect_point(xyzz_add(A, B), h2p, "P + P (another ZZ)", it);
            expect_point(xyzz_add(B, A), h2p, "P + P (another ZZ, swapped)", it);
            expect_identity(xyzz_add(A, N), "P + (-P)", it);
            expect_identity(xyzz_add(N, A), "(-P) + P", it);
            // xyzz_madd: every spelling of the affine y (canonical, y + p, the normalised 2p - y, the raw 2p - y), on both accumulators
            for (const xyzz& acc : {A, B}) {
                const affine same_pt[4] = {p, affine{p.x, add_kp(p.y, 1)}, affine{p.x, fp_neg<2>(pn.y)}, affine{p.x, fp_neg_raw<2>(pn.y)}};
                const affine opposite[4] = {pn, affine{p.x, add_kp(pn.y, 1)}, affine{p.x, fp_neg<2>(p.y)}, affine{p.x, fp_neg_raw<2>(p.y)}};
                for (int s = 0; s < 4; s++) {
                    xyzz m = acc, c = acc;
                    xyzz_madd(m, same_pt[s]);
                    expect_point(m, h2p, "P madd P", it);
                    xyzz_madd(c, opposite[s]);
                    expect_identity(c, "P madd (-P)", it);
                    if (s < 3) {  // the fully normalised form takes the same branches
                        xyzz mp = acc, cp = acc;
                        xyzz_madd_plain(mp, same_pt[s]);
                        xyzz_madd_plain(cp, opposite[s]);
                        if (!same_xyzz(m, mp) || !exact_identity_pattern(cp)) { printf("madd: lazy and plain differ on a special case (it=%d)\n", it); exit(1); }
                    }
                }
                // xyzz_madd_m32: the words of P / -P, canonical and + p, both signs
                for (int c = 0; c < 2; c++) {
                    const fp px = fp_unpack_shl5(wp[c][0]), py = fp_unpack_shl5(wp[c][1]), ny = fp_unpack_shl5(wn[c][1]);
                    xyzz m1 = acc, m2 = acc, c1 = acc, c2 = acc;
                    xyzz_madd_m32(m1, px, py, false);
                    expect_point(m1, h2p, "P madd_m32 P", it);
                    xyzz_madd_m32(m2, px, ny, true);
                    expect_point(m2, h2p, "P madd_m32 -(-P)", it);
                    xyzz_madd_m32(c1, px, py, true);
                    expect_identity(c1, "P madd_m32 -P", it);
                    xyzz_madd_m32(c2, px, ny, false);
                    expect_identity(c2, "P madd_m32 (-P)", it);
                }
            }
            n += 6 + 2 * (8 + 8);
        }
    }
    return n;
}

int main() {
    long checks = 0;
    // 1. field ops against the 4x64 host arithmetic, in the R = 2^256 Montgomery domain both sides
    for (int it = 0; it < 200000; it++) {
        uint32_t wa[8], wb[8];
        rand_words(wa, it % 11 == 0 ? 1 : it % 13 == 0 ? 2 : 0);
        rand_words(wb, it % 7 == 0 ? 1 : it % 17 == 0 ? 2 : 0);
        fp a = fp_from_mont256(wa), b = fp_from_mont256(wb);
        hostg1::Fq ha = hostg1::load_words(wa), hb = hostg1::load_words(wb);
        if (!same(to_host_mont256(fp_mul(a, b)), hostg1::mul(ha, hb))) { printf("mul mismatch\n"); return 1; }
        if (!same(to_host_mont256(fp_sqr(a)), hostg1::sqr(ha))) { printf("sqr mismatch\n"); return 1; }
        if (!same(to_host_mont256(fp_add(a, b)), hostg1::add(ha, hb))) { printf("add mismatch\n"); return 1; }
        if (!same(to_host_mont256(fp_sub<3>(a, b)), hostg1::sub(ha, hb))) { printf("sub mismatch\n"); return 1; }
        if (!same(to_host_mont256(fp_mul_add(a, b, b, fp_neg<3>(a))), hostg1::sub(hostg1::mul(ha, hb), hostg1::mul(hb, ha)))) { printf("mul_add mismatch\n"); return 1; }
        checks += 5;
        if (it % 100 == 0) {  // the windowed Fermat inversion (fp_inv) against the host's bit-by-bit one; 0 -> 0
            if (!same(to_host_mont256(fp_inv(a)), hostg1::inv(ha))) { printf("inv mismatch\n"); return 1; }
            checks++;
        }
    }
    {
        uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const fp zero = fp_from_mont256(z);
        if (!same(to_host_mont256(fp_inv(zero)), hostg1::load_words(z))) { printf("inv(0) != 0\n"); return 1; }
    }
    // 2. long chains of group operations on arbitrary field values (bounds are what is being checked)
    for (int chain = 0; chain < 2000; chain++) {
        uint32_t wx[8], wy[8];
        rand_words(wx, chain % 5 == 0 ? 1 : 0);
        rand_words(wy, chain % 7 == 0 ? 1 : chain % 11 == 0 ? 2 : 0);
        affine q{fp_from_mont256(wx), fp_from_mont256(wy)};
        xyzz acc = xyzz_from_affine(q), other = xyzz_identity();
        for (int s = 0; s < 600; s++) {
            rand_words(wx, s % 31 == 0 ? 1 : s % 37 == 0 ? 2 : 0);
            rand_words(wy, s % 29 == 0 ? 1 : 0);
            affine p2{fp_from_mont256(wx), fp_from_mont256(wy)};
            const bool ng = rng() & 1;
            affine p2n = p2, p2r = p2;
            if (ng) p2n.y = fp_neg<2>(p2.y), p2r.y = fp_neg_raw<2>(p2.y);
            p2 = p2n;
            {   // the lazily normalised mixed addition (raw negated y) against the fully normalised one
                xyzz a1 = acc, a2 = acc;
                xyzz_madd(a1, p2r);
                xyzz_madd_plain(a2, p2n);
                if (!same_xyzz(a1, a2) || xyzz_is_identity(a1) != xyzz_is_identity(a2)) { printf("madd: lazy and plain differ (chain %d step %d)\n", chain, s); return 1; }
                within_bounds(a2, "chain: madd_plain");
            }
            xyzz_madd(acc, p2r);
            within_bounds(acc, "chain: madd");
            if (s % 5 == 0) {
                xyzz_madd(other, p2);
                within_bounds(other, "chain: madd (second accumulator)");
                other = xyzz_add(other, acc);
                within_bounds(other, "chain: add");
            }
            if (s % 7 == 0) acc = xyzz_dbl(acc), within_bounds(acc, "chain: dbl");
            if (s % 97 == 0) acc = xyzz_add(acc, acc), within_bounds(acc, "chain: add(acc, acc)");  // takes the doubling branch
            if (s % 101 == 0) { jacobian j = xyzz_to_jacobian(other); uint32_t w[8]; fp_to_mont256(w, j.x); fp_to_mont256(w, j.z); }
            checks += 3;
        }
    }
    // 3. worst-case representatives: the same operations on operands pushed to the top of their documented ranges
    //    (X + 6p < 7p, Y + 4p < 5p, ZZ + p, ZZZ + p < 2p; affine y given as 2p - y) must pass every assertion and
    //    produce the same residues as on the reduced operands
    for (int it = 0; it < 100000; it++) {
        uint32_t w[6][8];
        for (int j = 0; j < 6; j++) rand_words(w[j], (it + j) % 19 == 0 ? 1 : (it + j) % 23 == 0 ? 2 : 0);
        // the identity is the EXACT limb pattern ZZ = 0 (only ever produced by xyzz_identity()), so residues 0 are
        // kept out of ZZ/ZZZ here; they are exercised in part 2
        if ((w[2][0] | w[2][1] | w[2][7]) == 0) w[2][0] = 5;
        if ((w[1][0] | w[1][1] | w[1][7]) == 0) w[1][0] = 5;
        xyzz a{fp_from_mont256(w[0]), fp_from_mont256(w[1]), fp_from_mont256(w[2]), fp_from_mont256(w[3])};
        affine q{fp_from_mont256(w[4]), fp_from_mont256(w[5])};
        xyzz b{fp_from_mont256(w[4]), fp_from_mont256(w[5]), fp_from_mont256(w[1]), fp_from_mont256(w[0])};
        // A K*p pad has no slack in its top limb only: a subtrahend within about 2^232 of the top of its range is the one that can tell a pad that
        // is one p too small.  Every eighth iteration the subtracted coordinates are p - 1 - d (d < 2^20), inflated to 7p - 1 - d, 5p - 1 - d, 2p - 1 - d
        if (it % 8 == 0) a.x = near_p(), a.y = near_p(), q.x = near_p(), q.y = near_p(), b.x = near_p(), b.y = near_p();
        xyzz ai{add_kp(a.x, 6), add_kp(a.y, 4), add_kp(a.zz, 1), add_kp(a.zzz, 1)};
        affine qi{q.x, add_kp(q.y, 1)};
        xyzz r1 = a, r2 = ai;
        if (it & 1) {  // negated y: normalised on the reduced operands, RAW (no carry ripple) on the inflated ones
            xyzz_madd(r1, affine{q.x, fp_neg<2>(q.y)});
            xyzz_madd(r2, affine{q.x, fp_neg_raw<2>(q.y)});
        } else {
            xyzz_madd(r1, q);
            xyzz_madd(r2, qi);
        }
        if (!same_xyzz(r1, r2)) { printf("madd: inflated operands change the residues (it=%d)\n", it); return 1; }
        within_bounds(r1, "madd (reduced)"), within_bounds(r2, "madd (inflated)");
        if (!same_xyzz(xyzz_dbl(a), xyzz_dbl(ai))) { printf("dbl: inflated operands change the residues\n"); return 1; }
        within_bounds(xyzz_dbl(a), "dbl (reduced)"), within_bounds(xyzz_dbl(ai), "dbl (inflated)");
        xyzz bi{add_kp(b.x, 6), add_kp(b.y, 4), add_kp(b.zz, 1), add_kp(b.zzz, 1)};
        if (!same_xyzz(xyzz_add(a, b), xyzz_add(ai, bi))) { printf("add: inflated operands change the residues\n"); return 1; }
        if (!same_xyzz(xyzz_add(a, bi), xyzz_add(ai, b))) { printf("add (mixed): inflated operands change the residues\n"); return 1; }
        for (const xyzz& sum : {xyzz_add(a, b), xyzz_add(ai, bi), xyzz_add(a, bi), xyzz_add(ai, b)}) within_bounds(sum, "add (reduced / inflated operands)");
        checks += 4;
    }
    // 3b / 4b. the doubling and the cancelling branch of xyzz_madd, xyzz_madd_m32 and xyzz_add on real equal and opposite points under a second
    //    ZZ, reduced and inflated, every result against the host's Jacobian law
    checks += special_cases(1500);
    // 4. round 5: the mixed addition on the caller's R = 2^256 Montgomery words as they are (fp_unpack_shl5 + xyzz_madd_m32) against the
    //    normalised one on converted operands -- canonical words, ANY 256-bit words (all ones: the largest multiplier, 2^261 - 32), reduced and
    //    inflated accumulators, both signs, the identity start and the doubling / cancelling branches
    for (int it = 0; it < 200000; it++) {
        uint32_t w[6][8];
        for (int j = 0; j < 6; j++) rand_words(w[j], (it + j) % 19 == 0 ? 1 : (it + j) % 23 == 0 ? 2 : 0);
        if ((w[2][0] | w[2][1] | w[2][7]) == 0) w[2][0] = 5;
        if (it % 3 == 1) for (int j = 4; j < 6; j++) for (int k = 0; k < 8; k++) w[j][k] = (uint32_t)rng();  // not canonical: any 256 bits
        if (it % 1000 == 7) for (int j = 4; j < 6; j++) for (int k = 0; k < 8; k++) w[j][k] = 0xFFFFFFFFu;
        xyzz a{fp_from_mont256(w[0]), fp_from_mont256(w[1]), fp_from_mont256(w[2]), fp_from_mont256(w[3])};
        if (it % 50 == 0) a = xyzz_identity();
        const xyzz ai = xyzz_is_identity(a) ? a : xyzz{add_kp(a.x, 6), add_kp(a.y, 4), add_kp(a.zz, 1), add_kp(a.zzz, 1)};
        const bool ng = (it >> 1) & 1;
        const fp qx = fp_unpack_shl5(w[4]), qy = fp_unpack_shl5(w[5]);
        for (int i = 0; i < 8; i++)
            if (qx.v[i] > FP_MASK || qy.v[i] > FP_MASK) { printf("unpack_shl5: limb not normalised\n"); return 1; }
        affine q{fp_from_mont256(w[4]), fp_from_mont256(w[5])};  // (fp_mul takes any 256-bit words: the value mod p)
        q.x = fp_reduce_lt2p(q.x), q.y = fp_reduce_lt2p(q.y);
        if (!same_residue(qx, q.x) || !same_residue(qy, q.y)) { printf("unpack_shl5: 32 * W is not the internal-domain value\n"); return 1; }
        if (ng) q.y = fp_neg<2>(q.y);
        xyzz r0 = a, r1 = a, r2 = ai;
        xyzz_madd_plain(r0, q);
        xyzz_madd_m32(r1, qx, qy, ng);
        xyzz_madd_m32(r2, qx, qy, ng);
        if (!same_xyzz(r0, r1) || !same_xyzz(r0, r2) || xyzz_is_identity(r0) != xyzz_is_identity(r1) || xyzz_is_identity(r0) != xyzz_is_identity(r2)) {
            printf("madd_m32 differs from the plain mixed addition (it=%d)\n", it);
            return 1;
        }
        within_bounds(r0, "madd_plain"), within_bounds(r1, "madd_m32 (reduced)"), within_bounds(r2, "madd_m32 (inflated)");
        // same point again (doubling branch), then its inverse (cancels to the identity)
        xyzz d0 = r0, d1 = r1;
        xyzz_madd_plain(d0, q);
        xyzz_madd_m32(d1, qx, qy, ng);
        within_bounds(d1, "madd_m32 (second addition)");
        if (xyzz_is_identity(a)) {  // a was the identity: r = q, so this was q + q
            if (!same_xyzz(d0, d1)) { printf("madd_m32: doubling branch differs (it=%d)\n", it); return 1; }
            xyzz c1 = r1;
            xyzz_madd_m32(c1, qx, qy, !ng);
            within_bounds(c1, "madd_m32 (q - q)");
            const bool y_zero = fp_is_zero_lt2p(fp_mul(qy, fp_one()));  // (y = 0 is its own inverse -- not a curve point, but a boundary operand here)
            if (!y_zero && !xyzz_is_identity(c1)) { printf("madd_m32: q + (-q) is not the identity (it=%d)\n", it); return 1; }
        }
        // a long chain keeps the bounds
        if (it % 100 == 0) {
            xyzz c0 = r0, c1 = r1;
            for (int s = 0; s < 200; s++) {
                uint32_t u[2][8];
                for (int j = 0; j < 2; j++) for (int k = 0; k < 8; k++) u[j][k] = (s % 3) ? (uint32_t)rng() : 0xFFFFFFFFu - (uint32_t)(rng() % 4);
                affine t{fp_reduce_lt2p(fp_from_mont256(u[0])), fp_reduce_lt2p(fp_from_mont256(u[1]))};
                const bool g2 = rng() & 1;
                if (g2) t.y = fp_neg<2>(t.y);
                xyzz_madd_plain(c0, t);
                xyzz_madd_m32(c1, fp_unpack_shl5(u[0]), fp_unpack_shl5(u[1]), g2);
                within_bounds(c1, "madd_m32 (chain)");
            }
            if (!same_xyzz(c0, c1)) { printf("madd_m32: chain differs (it=%d)\n", it); return 1; }
        }
        checks += 4;
    }
    printf("fp_bounds_check: %ld checked operations, no bound violated, field results identical to the 4x64 host arithmetic; %ld outputs inside the "
           "documented ranges, largest computed representative (multiples of p): X %.2Lf (< 7), Y %.2Lf (< 5), ZZ %.2Lf (< 2), ZZZ %.2Lf (< 2)\n",
           checks, bound_checks, seen_max[0], seen_max[1], seen_max[2], seen_max[3]);
    return 0;
}
