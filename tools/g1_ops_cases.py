"""Operands and checks for the BN254 G1 group law on RAW limb records (msm_test_g1_raw_op): shared by tests/test_gpu_20_g1_ops.py (the device) and
tests/test_g1_ops_cpu.py (the checks themselves).  Pure Python over tools/bn254_py.py; imports no library.

A record is what store_xyzz writes: X, Y, ZZ, ZZZ, 9 limbs of 29 bits each, internal domain (v * 2^261 mod p) plus a multiple of p of the caller's
choice.  csrc/ec_bn254.hpp promises X < 7p, Y < 5p, ZZ < 2p, ZZZ < 2p for every record and x < p, y < 2p for an affine operand: LOW is the bottom of
those ranges, TOP the top, and check_output() asserts everything the header promises of an output."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn254_py as bn  # noqa: E402

P, R_ORDER, G = bn.P, bn.R_ORDER, bn.G
R261 = 1 << 261
R261_INV = pow(R261, -1, P)
R256 = 1 << 256
R256_INV = pow(R256, -1, P)
MASK = (1 << 29) - 1
LOW = (0, 0, 0, 0)
TOP = (6, 4, 1, 1)         # multiples of p added to X, Y, ZZ, ZZZ: X + 6p < 7p, Y + 4p < 5p, ZZ + p, ZZZ + p < 2p
BOUNDS = (7, 5, 2, 2)      # X < 7p, Y < 5p, ZZ < 2p, ZZZ < 2p
NAMES = ("X", "Y", "ZZ", "ZZZ")
A0, D0 = 0x1234567890ABCDEF1234567890ABCDEF, 0xFEDCBA987654321  # point i = (A0 + i * D0) * G
SPELLINGS = ("canonical", "plus_p", "negated")


# ---- limbs -------------------------------------------------------------------------------------------------------------------------------------
def limbs(v):
    assert 0 <= v < R261
    return [(v >> (29 * i)) & MASK for i in range(9)]


def enc(v, k=0):
    """9 x 29-bit limbs of v * 2^261 mod p + k * p"""
    return limbs(v * R261 % P + k * P)


def value(ws):
    return sum(int(w) << (29 * i) for i, w in enumerate(ws))


def residue(ws):
    """the field element a limb vector holds"""
    return value(ws) * R261_INV % P


# ---- records -----------------------------------------------------------------------------------------------------------------------------------
def record(pt, t, infl=LOW):
    """the XYZZ record (x t^2, y t^3, t^2, t^3) of an affine pair, each coordinate on the representative + infl[.] * p"""
    assert t % P != 0
    t2 = t * t % P
    t3 = t2 * t % P
    return enc(pt[0] * t2 % P, infl[0]) + enc(pt[1] * t3 % P, infl[1]) + enc(t2, infl[2]) + enc(t3, infl[3])


def affine_record(pt, spelling="canonical"):
    """18 limbs x, y.  x canonical; y canonical, as y + p (the same point, the top of y < 2p), or as the normalised 2p - y that a negation gives:
    the point -pt, and exactly 2p for y = 0"""
    y = enc(pt[1])
    if spelling == "plus_p":
        y = enc(pt[1], 1)
    elif spelling == "negated":
        y = limbs(2 * P - value(y))
    else:
        assert spelling == "canonical", spelling
    return enc(pt[0]) + y


def affine_of(rec18):
    """the affine pair an 18-limb affine record holds"""
    return (residue(rec18[:9]), residue(rec18[9:18]))


def words8(v):
    assert 0 <= v < R256
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def words_m256(pt, noncanonical=False):
    """16 words x, y as arkworks holds them (v * 2^256 mod p); noncanonical: + p, which still fits 256 bits (2p < 2^256)"""
    k = P if noncanonical else 0
    return words8(pt[0] * R256 % P + k) + words8(pt[1] * R256 % P + k)


ALL_ONES_WORDS = [0xFFFFFFFF] * 16


def pair_of_words(ws16):
    """the affine pair ANY 16 words stand for: W * 2^-256 mod p per coordinate.  Not on the curve in general and need not be: the chord and the
    tangent are rational functions of the coordinates, which bn254_py.add evaluates on any pair"""
    v = lambda ws: sum(int(w) << (32 * i) for i, w in enumerate(ws))
    return (v(ws16[:8]) * R256_INV % P, v(ws16[8:16]) * R256_INV % P)


def near_top_record(t, rnd):
    """(record, affine pair) with X and Y in the last 2^-33 p below their bounds: X = 7p - 1 - d, Y = 5p - 1 - d' (d, d' < 2^20), ZZ = t^2 + p,
    ZZZ = t^3 + p: the largest subtrahends the header allows (X and Y are the coordinates that are ever subtracted).  A difference a + K*p - b
    comes out wrong on the device exactly when that integer is negative (the top limb wraps modulo 2^32 and the carry puts it right otherwise), so
    against a pad that is too small a TOP record fails for the residues above a, these for every a; on the host they are the operands that meet
    the limb-wise assertion of a K*p pad (no slack in its top limb) at its edge.  The pair is whatever the record then holds (off the curve; see
    pair_of_words)"""
    assert t % P != 0
    t2 = t * t % P
    t3 = t2 * t % P
    X, Y = 7 * P - 1 - rnd.randrange(1 << 20), 5 * P - 1 - rnd.randrange(1 << 20)
    pair = (X * R261_INV * pow(t2, -1, P) % P, Y * R261_INV * pow(t3, -1, P) % P)
    return limbs(X) + limbs(Y) + enc(t2, 1) + enc(t3, 1), pair


def near_top_affine(rnd, canonical_y=False):
    """(18 limbs, affine pair) with x in the last 2^-33 p below p and y below 2p: the top of an affine operand's range.  canonical_y: y below p,
    the top of what a RAW negation may be applied to (fp_neg_raw<2> takes a canonical y)"""
    x, y = P - 1 - rnd.randrange(1 << 20), (P if canonical_y else 2 * P) - 1 - rnd.randrange(1 << 20)
    return limbs(x) + limbs(y), (x * R261_INV % P, y * R261_INV % P)


ID_ONE = enc(1) + enc(1) + [0] * 18  # what xyzz_identity() writes
ID_ZERO = [0] * 36                   # a cleared bucket


# ---- the checks --------------------------------------------------------------------------------------------------------------------------------
def coords(rec):
    rec = [int(w) for w in rec]
    assert len(rec) == 36
    return [rec[9 * k:9 * k + 9] for k in range(4)]


def is_identity(rec):
    return not any(int(w) for w in rec[18:27])


def to_affine(rec):
    """record -> affine pair (X / ZZ, Y / ZZZ), None for the identity"""
    if is_identity(rec):
        return None
    x, y, zz, zzz = (residue(c) for c in coords(rec))
    return (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P)


def check_output(rec, want, what=""):
    """everything csrc/ec_bn254.hpp promises of an output record, and the point itself (want: an affine pair, None = the identity)"""
    cs = coords(rec)
    for k, c in enumerate(cs):
        assert max(c) <= MASK, (what, NAMES[k], "limb not normalised")
        assert value(c) < BOUNDS[k] * P, (what, NAMES[k], value(c) / P)
    if want is None:
        assert is_identity(rec), (what, "ZZ of an identity result is not zero limb for limb")
        return
    assert not is_identity(rec), (what, "identity")
    zz, zzz = residue(cs[2]), residue(cs[3])
    assert zz != 0 and zzz != 0, (what, "ZZ or ZZZ is a multiple of p")
    assert pow(zz, 3, P) == zzz * zzz % P, (what, "ZZ^3 != ZZZ^2")
    assert to_affine(rec) == want, (what, "not the expected point")


def check_all(out, wants, what=""):
    assert len(out) == len(wants), what
    for i, (rec, want) in enumerate(zip(out, wants)):
        check_output(rec, want, (what, i))


# ---- points ------------------------------------------------------------------------------------------------------------------------------------
def chain_points(n, a0=A0, d0=D0):
    """[(a0 + i * d0) * G for i < n] by repeated addition: two scalar multiplications, then one affine addition per point"""
    pt, step = bn.mul(a0, G), bn.mul(d0, G)
    out = []
    for _ in range(n):
        out.append(pt)
        pt = bn.add(pt, step)
    return out
