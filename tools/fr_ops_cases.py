"""Operands, the integer model and the checks for the BN254 scalar field Fr on RAW limb records (msm_test_fr_raw_op): shared by
tests/test_gpu_22_fr_ops.py (the device), tools/fr_bounds_check.cpp (the host compile of csrc/fr_bn254.hpp with every assertion live) and
tests/test_fr_ops_cpu.py (which runs the latter and tests the checks themselves).  Pure Python integers; imports no library.

A record is nine words: 9 limbs of 29 bits, value = sum limb_i * 2^(29 i).  raw(x) spells x, rep(x) = raw(x * 2^261 mod r) is the internal form.
Every function of fr_bn254.hpp returns ONE determined integer (model()): the Montgomery integer (A*B + m*r) >> 261 with m = -A*B/r mod 2^261 for
a product, a + b, a + K*r - b, a or a - r, bit moves, and the chains of those.  check_output() asserts, for one element, that the limbs are the
model's limb for limb, that every limb is at most 2^29 - 1, that the value is inside the bound the header documents for the operation, and that it
is congruent modulo r to the PLAIN result (x * y * 2^-261 mod r ...), which is computed without the Montgomery model and so cross-checks it.
Integer work: no tolerance anywhere.

legal() is the value discipline of fr_bn254.hpp as an assertion; every operand class below passes through it when it is built.  The limb patterns
come from FR29_R and FR29_PAD as csrc/fr29_constants.inc spells them (parsed here, checked against the integers), not from copies."""
import math
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
CONSTANTS = os.path.join(HERE, "..", "gpu-acceleration_amd", "csrc", "fr29_constants.inc")

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
B = 29
MASK = (1 << B) - 1
R261 = 1 << 261
R261_INV = pow(R261, -1, R)
R256 = 1 << 256
MUL_LIMIT = (R261 - R) * R261  # fr_mul needs A * B < (2^261 - r) * 2^261
POW_LIMIT = 84                 # fr_pow_u32 / fr_inv: base < 84 r

OPS = ("MUL", "ADD", "SUB2", "SUB3", "SUB7", "SUB8", "NORMALIZE", "REDUCE_LT2R", "CANONICAL", "UNPACK", "PACK", "FROM_STD", "TO_STD", "POW_U32", "INV")
(MUL, ADD, SUB2, SUB3, SUB7, SUB8, NORMALIZE, REDUCE_LT2R, CANONICAL, UNPACK, PACK, FROM_STD, TO_STD, POW_U32, INV) = range(15)
SUB_K = {SUB2: 2, SUB3: 3, SUB7: 7, SUB8: 8}
NEEDS_B = (MUL, ADD, SUB2, SUB3, SUB7, SUB8, POW_U32)
WORDS_IN = (UNPACK, FROM_STD)   # a is 8 words of 32 bits, word 8 ignored
WORDS_OUT = (PACK, TO_STD)      # out is 8 words of 32 bits, word 8 written as 0


# ---- the constant tables, as the header's include spells them ----------------------------------------------------------------------------------
def _parse_constants():
    text = open(CONSTANTS).read()
    one = lambda name: [int(x, 16) for x in re.search(r"\b%s\[\d+\] = \{([^}]*)\}" % name, text).group(1).replace("u", "").split(",")]
    pad_body = re.search(r"FR29_PAD\[FR29_MAX_PAD \+ 1\]\[9\] = \{(.*?)\n\};", text, re.S).group(1)
    pad = [[int(x, 16) for x in row.replace("u", "").split(",")] for row in re.findall(r"\{([^}]*)\}", pad_body)]
    inv = int(re.search(r"FR29_INV = (0x[0-9a-f]+)u", text).group(1), 16)
    return one("FR29_R"), pad, one("FR29_ONE"), one("FR29_IN_STD"), inv, one("FR_EXP_RM2")


FR29_R, FR29_PAD, FR29_ONE, FR29_IN_STD, FR29_INV, FR_EXP_RM2 = _parse_constants()


def value(ws):
    """the integer nine limbs (normalised or not) spell"""
    return sum(int(w) << (B * i) for i, w in enumerate(ws))


def limbs(v):
    assert 0 <= v < R261, "not a normalised value"
    return [(v >> (B * i)) & MASK for i in range(9)]


def words8(v):
    """8 words of 32 bits and an ignored ninth"""
    assert 0 <= v < R256
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0]


def value32(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws[:8]))


def rep(x):
    return limbs(x * R261 % R)


def check_tables():
    """what the issue verified by hand, as assertions: r, rep(1), 2^522, -1/r, r - 2; every pad row spells K*r with limbs 0..7 >= 2^29 - 1 and a
    top limb that covers any normalised value below (K-1)*r"""
    assert value(FR29_R) == R and max(FR29_R) <= MASK
    assert value(FR29_ONE) == R261 % R and value(FR29_IN_STD) == (1 << 522) % R and max(FR29_ONE + FR29_IN_STD) <= MASK
    assert (FR29_INV * R + 1) % (1 << B) == 0
    assert value32(FR_EXP_RM2) == R - 2 and len(FR29_PAD) == 9
    for k in range(2, 9):
        row = FR29_PAD[k]
        assert value(row) == k * R and min(row[:8]) >= MASK and max(row) < (1 << 31), k
        assert row[8] >= ((k - 1) * R - 1) >> (8 * B), k


check_tables()


# ---- legality: the value discipline of fr_bn254.hpp ------------------------------------------------------------------------------------------
def _normalised(ws):
    return len(ws) == 9 and all(0 <= int(w) <= MASK for w in ws)


def _normalize_legal(ws):
    c = 0
    for i in range(8):
        t = int(ws[i]) + c
        assert t < (1 << 32), "fr_normalize: limb + carry overflows 32 bits"
        c = t >> B
    assert int(ws[8]) + c < (1 << B), "fr_normalize: value >= 2^261"


def legal(op, a, b=None):
    """raises AssertionError unless (a, b) is inside what fr_bn254.hpp allows `op` to be called on"""
    a = [int(w) for w in a]
    b = [int(w) for w in b] if b is not None else None
    assert len(a) == 9 and (op not in NEEDS_B or (b is not None and len(b) == 9)), OPS[op]
    if op in WORDS_IN:
        assert all(0 <= w <= 0xFFFFFFFF for w in a)
        return
    if op == NORMALIZE:
        assert all(0 <= w <= 0xFFFFFFFF for w in a)
        _normalize_legal(a)
        return
    assert _normalised(a), (OPS[op], "a not normalised")
    A = value(a)
    if op == MUL:
        assert _normalised(b) and A * value(b) < MUL_LIMIT, "fr_mul: A * B >= (2^261 - r) * 2^261"
    elif op == ADD:
        assert _normalised(b) and A + value(b) < R261, "fr_add: sum >= 2^261"
    elif op in SUB_K:
        k = SUB_K[op]
        assert _normalised(b) and value(b) < (k - 1) * R, "fr_sub: b >= (K-1) r"
        assert all(x <= p for x, p in zip(b, FR29_PAD[k])), "fr_sub: a subtrahend limb exceeds the pad"
        assert A + k * R - value(b) < R261, "fr_sub: a + K r - b >= 2^261"
    elif op == REDUCE_LT2R:
        assert A < 2 * R, "fr_reduce_lt2r: a >= 2r"
    elif op == PACK:
        assert A < R256, "fr_pack: a >= 2^256"
    elif op in (POW_U32, INV):
        assert A < POW_LIMIT * R, "fr_pow_u32 / fr_inv: a >= 84 r"
        assert op == INV or 0 <= b[0] <= 0xFFFFFFFF
    else:
        assert op in (CANONICAL, TO_STD), op


def is_legal(op, a, b=None):
    try:
        legal(op, a, b)
        return True
    except AssertionError:
        return False


# ---- the model: the one integer each function returns ----------------------------------------------------------------------------------------
_R_NEG_INV = (-pow(R, -1, R261)) % R261


def mont(A, Bv):
    """fr_mul as an integer: (A*B + m*r) >> 261 with m = -A*B / r mod 2^261 (the nine m[k] of the product scan are the limbs of this m)"""
    assert A * Bv < MUL_LIMIT, "fr_mul: A * B >= (2^261 - r) * 2^261"
    t = A * Bv
    m = t * _R_NEG_INV % R261
    q, rem = divmod(t + m * R, R261)
    assert rem == 0 and q < R261
    return q


def mont_m(A, Bv):
    return A * Bv * _R_NEG_INV % R261


def _lt2r(v):
    assert v < 2 * R
    return v - R if v >= R else v


def _pow(A, e):
    acc, b = value(FR29_ONE), A
    while e:
        if e & 1:
            acc = mont(acc, b)
        b = mont(b, b)
        e >>= 1
    return acc


def _inv(A):
    acc, b, e = value(FR29_ONE), A, R - 2
    for i in range(254):
        if (e >> i) & 1:
            acc = mont(acc, b)
        b = mont(b, b)
    return acc


def model(op, a, b=None):
    """the nine words `op` stores for the LEGAL operands (a, b)"""
    legal(op, a, b)
    a = [int(w) for w in a]
    if op == UNPACK:
        return limbs(value32(a))
    if op == FROM_STD:
        return limbs(mont(value32(a), value(FR29_IN_STD)))
    A = value(a)
    Bv = value(b) if op in NEEDS_B and op != POW_U32 else None
    if op == MUL:
        return limbs(mont(A, Bv))
    if op == ADD:
        return limbs(A + Bv)
    if op in SUB_K:
        return limbs(A + SUB_K[op] * R - Bv)
    if op == NORMALIZE:
        return limbs(A)
    if op == REDUCE_LT2R:
        return limbs(_lt2r(A))
    if op == CANONICAL:
        return limbs(_lt2r(mont(A, value(FR29_ONE))))
    if op == PACK:
        return words8(A)
    if op == TO_STD:
        return words8(_lt2r(mont(A, 1)))
    if op == POW_U32:
        return limbs(_pow(A, int(b[0])))
    assert op == INV
    return limbs(_inv(A))


# ---- the plain-arithmetic result and the documented bound: computed WITHOUT the Montgomery model ---------------------------------------------
def plain_residue(op, a, b=None):
    """what the result must be congruent to modulo r, from the operands' values alone"""
    a = [int(w) for w in a]
    A = value32(a) if op in WORDS_IN else value(a)
    Bv = value(b) if op in NEEDS_B and op != POW_U32 else None
    if op == MUL:
        return A * Bv * R261_INV % R
    if op == ADD:
        return (A + Bv) % R
    if op in SUB_K:
        return (A - Bv) % R
    if op in (NORMALIZE, REDUCE_LT2R, CANONICAL, UNPACK, PACK):
        return A % R
    if op == FROM_STD:
        return A * R261 % R
    if op == TO_STD:
        return A * R261_INV % R
    x = A * R261_INV % R  # a = rep(x) + a multiple of r
    if op == POW_U32:
        return pow(x, int(b[0]), R) * R261 % R
    return pow(x, R - 2, R) * R261 % R


def check_bound(op, a, b, v):
    """the value the header documents for an output of `op` (v: the integer the output spells)"""
    a = [int(w) for w in a]
    if op == MUL:
        assert (v << 261) < value(a) * value(b) + (R << 261), "fr_mul: value >= A*B/2^261 + r"
    elif op in (ADD, NORMALIZE) or op in SUB_K:
        assert v < R261
    elif op in (REDUCE_LT2R, CANONICAL, TO_STD):
        assert v < R, OPS[op] + ": not canonical"
    elif op in (UNPACK, PACK):
        assert v < R256
    else:
        assert op in (FROM_STD, POW_U32, INV) and v < 2 * R, OPS[op] + ": value >= 2r"


def check_output(op, a, b, out, what=""):
    """one element: limbs == the model's, every limb <= 2^29 - 1, the value inside the documented bound and congruent to the plain result"""
    out = [int(w) for w in out]
    assert len(out) == 9, what
    want = model(op, a, b)
    assert out == want, (what, OPS[op], "not the model's limbs", out, want)
    if op in WORDS_OUT:
        assert out[8] == 0 and all(0 <= w <= 0xFFFFFFFF for w in out), (what, OPS[op])
        v = value32(out)
    else:
        assert max(out) <= MASK and min(out) >= 0, (what, OPS[op], "limb not normalised")
        v = value(out)
    check_bound(op, a, b, v)
    res = plain_residue(op, a, b)
    assert v % R == res, (what, OPS[op], "not congruent to the plain result")
    if op in (REDUCE_LT2R, CANONICAL, TO_STD):
        assert v == res, (what, OPS[op])
    elif op in (ADD, NORMALIZE, UNPACK, PACK) or op in SUB_K:  # no reduction happens: the integer itself is determined by plain arithmetic
        A = value32(a) if op in WORDS_IN else value(a)
        assert v == (A if op not in NEEDS_B else A + value(b) if op == ADD else A + SUB_K[op] * R - value(b)), (what, OPS[op])
    elif op == INV and not any(int(w) for w in a):
        assert not any(out), (what, "fr_inv(0) != 0")


def check_all(op, a, b, out, what=""):
    """every element of a launch (a, b, out: n x 9; b None where the operation reads none)"""
    assert len(out) == len(a) and (b is None or len(b) == len(a)), what
    for i in range(len(a)):
        check_output(op, a[i], b[i] if b is not None else None, out[i], (what, i))


# ---- operand classes ---------------------------------------------------------------------------------------------------------------------------
def common_values(rnd, n_random=8):
    """the classes every operation sees (as far as they are legal for it): 0, 1, r - 1, rep(0), rep(1), rep(r - 1), random canonical values, random
    normalised values below 84 r"""
    vals = [0, 1, R - 1, 0, R261 % R, (R - 1) * R261 % R]
    vals += [rnd.randrange(R) for _ in range(n_random)]
    vals += [rnd.randrange(POW_LIMIT * R) for _ in range(n_random)]
    return vals


def _a_limit(op):
    """the exclusive bound on a random operand a of `op` (b likewise where it is a record)"""
    return {REDUCE_LT2R: 2 * R, PACK: R256, UNPACK: R256, FROM_STD: R256, CANONICAL: R261, TO_STD: R261}.get(op, POW_LIMIT * R)


def _b_limit(op):
    return (SUB_K[op] - 1) * R if op in SUB_K else POW_LIMIT * R


POW_EXPONENTS = (0, 1, 2, 3, 1 << 31, (1 << 32) - 1)


def random_launch(op, n, rnd):
    """(a, b) of n elements: the common classes first (those legal for `op`), then random values below the operation's own limit; b None where
    the operation reads none.  Un-normalised limbs for NORMALIZE, 256-bit patterns for UNPACK / FROM_STD"""
    la, lb = _a_limit(op), _b_limit(op)
    pool = [v for v in common_values(rnd) if v < la]
    a_vals = [pool[i] if i < len(pool) and n > 1 else rnd.randrange(la) for i in range(n)]
    rnd.shuffle(a_vals)
    if op in WORDS_IN:
        a = [words8(v)[:8] + [rnd.getrandbits(32)] for v in a_vals]  # word 8 is ignored: anything
    elif op == NORMALIZE:
        a = [fatten(limbs(v), rnd) for v in a_vals]
    else:
        a = [limbs(v) for v in a_vals]
    b = None
    if op == POW_U32:
        b = [[rnd.choice(POW_EXPONENTS) if i % 2 else rnd.getrandbits(rnd.randrange(1, 33))] + [rnd.getrandbits(32) for _ in range(8)] for i in range(n)]
    elif op in NEEDS_B:
        poolb = [v for v in common_values(rnd) if v < lb]
        b_vals = [rnd.choice(poolb) if i % 3 == 0 else rnd.randrange(lb) for i in range(n)]
        b = [limbs(v) for v in b_vals]
    for i in range(n):
        legal(op, a[i], b[i] if b is not None else None)
    return a, b


def fatten(ls, rnd):
    """the same integer on un-normalised limbs: limb i + 1 lends t to limb i (t * 2^29 more there), as far as limb + carry stays below 2^32"""
    ls = list(ls)
    for i in range(8):
        t = min(ls[i + 1], rnd.randrange(8))
        if ls[i] + (t << B) + 8 < (1 << 32):
            ls[i] += t << B
            ls[i + 1] -= t
    return ls


def _pairs(op, pairs):
    a, b = [list(p[0]) for p in pairs], [list(p[1]) for p in pairs]
    for x, y in zip(a, b):
        legal(op, x, y)
    return a, b


def _single(op, rows):
    rows = [list(r) for r in rows]
    for x in rows:
        legal(op, x)
    return rows, None


def one_limb(i, v=MASK):
    ls = [0] * 9
    ls[i] = v
    return ls


def edge_classes(rnd):
    """{name: (op, a, b)}: every edge class, one launch each, every element proved legal as it is built"""
    out = {}
    top = R261 - 1
    # ---- MUL
    sq = math.isqrt(MUL_LIMIT)
    assert sq * sq < MUL_LIMIT <= (sq + 1) * (sq + 1)
    out["mul top of the domain"] = (MUL,) + _pairs(MUL, [(limbs(top), limbs(2 * R - 1)), (limbs(top), limbs(R - 1)), (limbs(top), limbs(1 << 260)),
                                                          (limbs(2 * R - 1), limbs(top)), (limbs(168 * R), limbs(168 * R)), (limbs(sq), limbs(sq)),
                                                          (limbs(top), limbs(R261 - R)), (limbs(top), limbs(0)), (limbs(top), limbs(1))])
    pairs = []
    for i in range(9):
        for j in range(9):
            x, y = one_limb(i), one_limb(j)
            if value(x) * value(y) >= MUL_LIMIT:  # only (8, 8): (2^261 - 2^232)^2 is outside the domain.  a keeps its limb of ones; b's top limb is
                y = one_limb(j, (MUL_LIMIT - 1) // value(x) >> (8 * B))  # the largest that is legal against it
                assert (i, j) == (8, 8) and y[8] < MASK and value(x) * (value(y) + (1 << (8 * B))) >= MUL_LIMIT
            pairs.append((x, y))
    out["mul one limb of ones against one limb of ones"] = (MUL,) + _pairs(MUL, pairs)
    pairs = []
    for _ in range(16):  # A * B = r modulo 2^261: m = -A*B/r = -1 = all limbs 2^29 - 1
        A = rnd.randrange(POW_LIMIT * R) | 1
        Bv = R * pow(A, -1, R261) % R261
        assert mont_m(A, Bv) == top
        pairs.append((limbs(A), limbs(Bv)))
    pairs.append((limbs(1), limbs(R)))
    pairs.append((limbs(R), limbs(1)))
    out["mul with m all ones"] = (MUL,) + _pairs(MUL, pairs)
    # ---- ADD
    pairs = [(limbs(v), limbs(top - v)) for v in [0, top, 1, R, (1 << 232) - 1, 1 << 260] + [rnd.randrange(R261) for _ in range(10)]]
    pairs += [(limbs((1 << 232) - 1), limbs(1)), (limbs(1), limbs((1 << 232) - 1)), (limbs(0), limbs(0)),
              (limbs(top - 1), limbs(1)), (limbs((1 << 232) - 1), limbs(top - ((1 << 232) - 1)))]
    out["add to the top and through every carry"] = (ADD,) + _pairs(ADD, pairs)
    # ---- SUB<K>
    for op, k in SUB_K.items():
        bmax = (k - 1) * R - 1
        ones8 = [MASK] * 8 + [(bmax >> (8 * B)) - 1]  # limbs 0..7 all ones under the largest top limb that keeps it below (K-1) r
        assert value(ones8) <= bmax and value(ones8) + (1 << (8 * B)) > bmax
        bs = [bmax, 0, value(ones8), R - 1, 1] + [rnd.randrange(bmax + 1) for _ in range(6)]
        pairs = []
        for bv in bs:
            amax = top - k * R + bv          # a + K r - b = 2^261 - 1
            for av in (0, bv, amax, 1, R - 1, rnd.randrange(amax + 1)):
                if av <= amax:
                    pairs.append((limbs(av), limbs(bv)))
            pairs.append((limbs(amax), limbs(bv)))
        out["sub<%d> at both ends of a and b" % k] = (op,) + _pairs(op, pairs)
    # ---- NORMALIZE
    rows = [[0] * 9]
    fat = [(1 << 32) - 1] + [(1 << 32) - 1 - 7] * 7  # limb + carry < 2^32 with the largest carry (7) a 32-bit limb can hand on
    carry = 0
    for w in fat:
        carry = (w + carry) >> B
    rows.append(fat + [MASK - carry])                 # the top limb lands exactly on 2^29 - 1
    rows.append(fat + [0])
    rows.append([MASK] * 9)
    rows.append([MASK + 1] + [MASK] * 7 + [MASK - 1])  # one carry rippling through all eight low limbs into the top one
    for _ in range(8):
        ws = [rnd.getrandbits(32) & ~7 for _ in range(8)]
        carry = 0
        for w in ws:
            carry = (w + carry) >> B
        rows.append(ws + [rnd.randrange(MASK - carry + 1)])
    out["normalize fat limbs"] = (NORMALIZE,) + _single(NORMALIZE, rows)
    # ---- REDUCE_LT2R
    borrow_all = [FR29_R[0] - 1] + FR29_R[1:]          # limb 0 one less, limbs 1..8 equal: r - 1, the subtraction borrows through every limb
    equal_all = list(FR29_R)                           # every limb equal: r itself
    assert value(borrow_all) == R - 1 and value(equal_all) == R
    vals = [0, 1, R - 1, R, R + 1, 2 * R - 1, R + (1 << 232), R - (1 << 232), (1 << 232) - 1]
    rows = [limbs(v) for v in vals] + [borrow_all, equal_all]
    for i in range(9):  # r with one limb one less / one more: the borrow starts, and stops, at every limb
        rows.append(limbs(R - (1 << (B * i))))
        rows.append(limbs(R + (1 << (B * i))))
    out["reduce_lt2r around r"] = (REDUCE_LT2R,) + _single(REDUCE_LT2R, rows)
    # ---- CANONICAL and TO_STD
    vals = [top, 0, 1, top - 1, R261 - R, 169 * R, 169 * R - 1, 169 * R + 1]
    for k in range(1, 169):
        vals += [k * R - 1, k * R, k * R + 1]
    vals += [rnd.randrange(R261) for _ in range(24)]
    for op in (CANONICAL, TO_STD):
        out[OPS[op].lower() + " of any normalised value"] = (op,) + _single(op, [limbs(v) for v in vals])
    # ---- UNPACK, PACK, FROM_STD
    patterns = [R256 - 1, 0, R, R - 1, R + 1, 2 * R, 5 * R, R256 - 2, 0xFFFFFFFF, 0xFFFFFFFF << 224] + [rnd.getrandbits(256) for _ in range(8)]
    bits = [1 << i for i in range(256)]
    for op in (UNPACK, FROM_STD):
        out[OPS[op].lower() + " of edge patterns"] = (op,) + _single(op, [words8(v)[:8] + [0xFFFFFFFF] for v in patterns])
        out[OPS[op].lower() + " of every single bit"] = (op,) + _single(op, [words8(v) for v in bits])
    out["pack of edge patterns"] = (PACK,) + _single(PACK, [limbs(v) for v in patterns])
    out["pack of every single bit"] = (PACK,) + _single(PACK, [limbs(v) for v in bits])
    # ---- POW_U32
    bases = [0, R261 % R, (R - 1) * R261 % R, POW_LIMIT * R - 1, 83 * R, R, 1] + [rnd.randrange(POW_LIMIT * R) for _ in range(3)]
    pairs = [(limbs(v), [e] + [0] * 8) for v in bases for e in POW_EXPONENTS]
    out["pow_u32 edge exponents"] = (POW_U32,) + _pairs(POW_U32, pairs)
    # ---- INV
    vals = [0, R261 % R, (R - 1) * R261 % R, 1, R - 1, POW_LIMIT * R - 1, R261 % R + 83 * R] + [rnd.randrange(R) for _ in range(6)]
    vals += [rnd.randrange(POW_LIMIT * R) for _ in range(6)]
    out["inv"] = (INV,) + _single(INV, [limbs(v) for v in vals])
    return out


def roundtrip_patterns(rnd):
    """the 256-bit patterns of the PACK(UNPACK(w)) == w and TO_STD(FROM_STD(w)) == w mod r checks, as n x 9 words"""
    vals = [R256 - 1, 0, R, R - 1, R + 1] + [1 << i for i in range(256)] + [rnd.getrandbits(256) for _ in range(8)]
    return [words8(v) for v in vals]


# ---- the butterfly chain of ntt_bn254.hpp composed from the operations -----------------------------------------------------------------------
CHAIN_LEVELS = 12


def chain_start(rnd, n):
    """(u, v, twiddles[level]): rows just below 2r; a twiddle is a table entry (< r) or, every third element, a product of two (< 2r)"""
    near = lambda: limbs(2 * R - 1 - rnd.randrange(1 << 20))
    u, v = [near() for _ in range(n)], [near() for _ in range(n)]
    u[0], v[0] = limbs(2 * R - 1), limbs(2 * R - 1)
    tw = [[limbs(rnd.randrange(R, 2 * R) if i % 3 == 2 else rnd.randrange(R)) for i in range(n)] for _ in range(CHAIN_LEVELS)]
    for row in tw:
        row[0] = limbs(2 * R - 1)
    return u, v, tw


def chain_level(run, s, u, v, w, what="chain"):
    """one level: x = MUL(v, w), u' = ADD(u, x), v' = SUB3(u, x) through run(op, a, b) -> out.  Rows entering level s are below (2 + 3s) r, as
    ntt_bn254.hpp claims; every output is checked against the model and the next level's bound"""
    lim_in, lim_out = (2 + 3 * s) * R, (2 + 3 * (s + 1)) * R
    assert all(value(r) < lim_in for r in u) and all(value(r) < lim_in for r in v), (what, s, "row at or above (2 + 3s) r on the way in")
    x = run(MUL, v, w)
    check_all(MUL, v, w, x, (what, s, "mul"))
    assert all(value(r) < 2 * R for r in x), (what, s, "x >= 2r")
    un = run(ADD, u, x)
    check_all(ADD, u, x, un, (what, s, "add"))
    vn = run(SUB3, u, x)
    check_all(SUB3, u, x, vn, (what, s, "sub<3>"))
    assert all(value(r) < lim_out for r in un) and all(value(r) < lim_out for r in vn), (what, s, "row at or above (2 + 3(s+1)) r")
    return un, vn


# ---- the records file tools/fr_bounds_check.cpp reads ----------------------------------------------------------------------------------------
def launch_words(op, a, b):
    """one launch as 32-bit words: op, n, then a (n x 9) and b (n x 9, zeros where the operation reads none)"""
    n = len(a)
    flat = [op, n]
    for row in a:
        flat += [int(w) for w in row]
    for i in range(n):
        flat += [int(w) for w in b[i]] if b is not None else [0] * 9
    return flat


ILLEGAL_MUL = (MUL, [limbs(R261 - 1)], [limbs(R261 - 1)])  # the header's old contract allowed it; the top limb of the result leaves 29 bits
assert not is_legal(MUL, ILLEGAL_MUL[1][0], ILLEGAL_MUL[2][0])
