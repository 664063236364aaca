"""Operands, the integer model and the checks for the BN254 base field Fq and its extension Fq2 on RAW limb records (msm_test_fq_raw_op,
msm_test_fq2_raw_op): shared by tests/test_gpu_24_fq_ops.py (the device), tools/fq_bounds_check.cpp (the host compile of csrc/fp_bn254.hpp and
csrc/fp2_bn254.hpp with every assertion live) and tests/test_fq_ops_cpu.py (which runs the latter and tests the checks themselves).  Pure Python
integers; imports no library and nothing from the project.

A record is nine words: 9 limbs of 29 bits, value = sum limb_i * 2^(29 i); an Fq2 record is two of them (c0, c1).  An operation is
(field, kind, K): field 1 = Fq, 2 = Fq2, kind a name of FQ_KINDS / FQ2_KINDS, K the pad multiple (0 where the function has none); op_word() is
the hook's kind | K << 8.  An element is the flat list of the words of its ARITY records.

evaluate() runs one element through the functions of the two headers AS WRITTEN -- limb-wise sums against the pad rows, the carry ripple, the
product scan column by column -- on Python integers, with the value discipline of the headers as assertions (normalised limbs, subtrahend limb <=
pad limb, limb + carry < 2^32, value < 2^261 after every addition, A*B (+ C*D) < (2^261 - p) * 2^261 for every product, every 64-bit column of a
product below 2^64, fp_reduce_lt2p / fp_inv input < 2p, fp_pack input < 2^256): legal() is "evaluate() raises nothing", model() its result.  Every
product is also computed in closed form, (A*B + C*D + m*p) >> 261 with m = -(A*B + C*D)/p mod 2^261, and the two must agree.
check_output() asserts, for one element, that the limbs are the model's limb for limb, that every limb is at most 2^29 - 1, that the value is
inside the bound the header documents, and that it is congruent modulo p to the PLAIN result (plain(): x * y * 2^-261 mod p ...), computed from the
operands' values alone, without the Montgomery model and without the pad tables.  Integer work: no tolerance anywhere.

The pad rows and constants come from csrc/fp29_constants.inc as the include spells them (parsed here, checked against the integers); FP2_PAD is
rebuilt by the rule of fp2_make_pads."""
import math
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "gpu-acceleration_amd", "csrc")

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
B = 29
MASK = (1 << B) - 1
R261 = 1 << 261
R261_INV = pow(R261, -1, P)
R256 = 1 << 256
TOP = R261 - 1
MUL_LIMIT = (R261 - P) * R261  # a normalised result of fp_mul / fp_sqr / fp_mul_add needs A*B (+ C*D) < (2^261 - p) * 2^261
FP2_MAX_PAD = 18

FQ_KINDS = ("MUL", "SQR", "MUL_ADD", "ADD", "DBL", "SUB", "NEG", "SUB_B_2C", "NORMALIZE", "REDUCE_LT2P", "CANONICAL", "INV", "IS_ZERO_LT2P", "UNPACK",
            "UNPACK_SHL5", "FROM_MONT256", "FROM_STD", "PACK", "TO_MONT256", "TO_STD", "MUL_NEG_RAW2", "NORMALIZE_NEG_RAW2", "SUB6_NEG_RAW4", "Y3")
FQ_ARITY = {"MUL": 2, "ADD": 2, "SUB": 2, "MUL_NEG_RAW2": 2, "SUB6_NEG_RAW4": 2, "SUB_B_2C": 3, "MUL_ADD": 4, "Y3": 5}
FQ_K = {"SUB": (2, 3, 4, 5, 6, 7, 8), "NEG": (2, 3, 4, 6), "Y3": (3, 6)}
FQ2_KINDS = ("MUL", "SQR", "SUB", "NEG", "ADD", "DBL", "MUL_FP", "IS_ZERO_LT2P", "IS_ZERO_ANY", "NEG_RAW6_MUL_ONE", "NEG_RAW6_MUL_FP", "CONJ")
FQ2_WORDS = {"MUL": 36, "SUB": 36, "ADD": 36, "MUL_FP": 27, "NEG_RAW6_MUL_FP": 27}
FQ2_K = {"MUL": (3, 4, 6, 7, 9, 10, 13, 15, 16, 17), "SQR": (3, 5, 6, 12, 13, 15, 16, 17), "SUB": (2, 3, 4, 5, 6, 7, 8, 9, 12, 13), "NEG": (2, 8),
         "CONJ": (9, 13)}
WORDS_IN = ("UNPACK", "UNPACK_SHL5", "FROM_MONT256", "FROM_STD")  # Fq: 8 words of 32 bits in, word 8 ignored
WORDS_OUT = ("PACK", "TO_MONT256", "TO_STD")                     # Fq: 8 words of 32 bits out, word 8 written as 0
FLAG_OUT = ("IS_ZERO_LT2P", "IS_ZERO_ANY")                       # 0 or 1 in word 0, the other words 0

ALL_OPS = tuple((1, kind, k) for kind in FQ_KINDS for k in FQ_K.get(kind, (0,))) + tuple((2, kind, k) for kind in FQ2_KINDS for k in FQ2_K.get(kind, (0,)))


def op_word(op):
    field, kind, k = op
    return (FQ_KINDS if field == 1 else FQ2_KINDS).index(kind) | k << 8


def op_name(op):
    return "%s_%s%s" % ("fq" if op[0] == 1 else "fq2", op[1], "<%d>" % op[2] if op[2] else "")


def in_words(op):
    return 9 * FQ_ARITY.get(op[1], 1) if op[0] == 1 else FQ2_WORDS.get(op[1], 18)


def out_words(op):
    return 9 * op[0]


# ---- the constant tables, as the header's include spells them ----------------------------------------------------------------------------------
def _parse_constants():
    text = open(os.path.join(CSRC, "fp29_constants.inc")).read()
    hexes = lambda body: [int(x, 16) for x in body.replace("u", "").split(",")]
    c = {name: hexes(re.search(r"\b%s\[9\] = \{([^}]*)\}" % name, text).group(1))
         for name in ("FP29_P", "FP29_ONE", "FP29_IN_MONT", "FP29_IN_STD", "FP29_OUT_MONT", "FP29_2P", "FP29_PAD5_FAT3")}
    pad_body = re.search(r"FP29_PAD\[FP29_MAX_PAD \+ 1\]\[9\] = \{(.*?)\n\};", text, re.S).group(1)
    c["FP29_PAD"] = [hexes(row) for row in re.findall(r"\{([^}]*)\}", pad_body)]
    c["FP29_INV"] = int(re.search(r"FP29_INV = (0x[0-9a-f]+)u", text).group(1), 16)
    c["FP29_MAX_PAD"] = int(re.search(r"FP29_MAX_PAD = (\d+);", text).group(1))
    return c


C = _parse_constants()
FP29_P, FP29_PAD, FP29_ONE, FP29_PAD5_FAT3 = C["FP29_P"], C["FP29_PAD"], C["FP29_ONE"], C["FP29_PAD5_FAT3"]


def make_fp2_pads(drop_minus_one=False):
    """FP2_PAD by the rule of fp2_make_pads (fp2_bn254.hpp): K*p on normalised limbs, then 2^29 lent downwards limb by limb"""
    t = [[0] * 9 for _ in range(FP2_MAX_PAD + 1)]
    for k in range(2, FP2_MAX_PAD + 1):
        c, n = 0, [0] * 9
        for i in range(8):
            s = k * FP29_P[i] + c
            n[i], c = s & MASK, s >> B
        n[8] = k * FP29_P[8] + c
        t[k] = [n[0] + (1 << B)] + [n[i] + (1 << B) - 1 for i in range(1, 8)] + [n[8] - (0 if drop_minus_one else 1)]
    return t


FP2_PAD = make_fp2_pads()


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
    return limbs(x * R261 % P)


def check_pad_row(row, k, fat=1):
    """a pad row spells k*p with limbs 0..7 >= fat * (2^29 - 1), 32-bit limbs, and a top limb that covers any normalised value below (k - 1) p"""
    assert value(row) == k * P and min(row[:8]) >= fat * MASK and max(row) < (1 << 32) and row[8] >= ((k - 1) * P - 1) >> (8 * B), k


def check_tables():
    assert value(FP29_P) == P and max(FP29_P) <= MASK and (C["FP29_INV"] * P + 1) % (1 << B) == 0
    assert value(FP29_ONE) == R261 % P and value(C["FP29_IN_MONT"]) == (1 << 266) % P and value(C["FP29_IN_STD"]) == (1 << 522) % P
    assert value(C["FP29_OUT_MONT"]) == R256 % P and C["FP29_2P"] == limbs(2 * P)
    assert max(FP29_ONE + C["FP29_IN_MONT"] + C["FP29_IN_STD"] + C["FP29_OUT_MONT"]) <= MASK
    assert len(FP29_PAD) == C["FP29_MAX_PAD"] + 1 == 13 and not any(FP29_PAD[0] + FP29_PAD[1])
    for k in range(2, 13):
        check_pad_row(FP29_PAD[k], k)
    check_pad_row(FP29_PAD5_FAT3, 5, fat=3)
    for k in range(2, FP2_MAX_PAD + 1):
        check_pad_row(FP2_PAD[k], k)
        assert k > 12 or FP2_PAD[k] == FP29_PAD[k]  # the two tables agree where both exist


check_tables()


# ---- the functions of the two headers on limb lists, every assumption asserted ---------------------------------------------------------------
_P_NEG_INV = (-pow(P, -1, R261)) % R261
COLUMN = {"max": 0, "where": ""}  # the largest 64-bit column any product scan met


def normalised(ws):
    return len(ws) == 9 and all(0 <= int(w) <= MASK for w in ws)


def need_normalised(*operands):
    for ws in operands:
        assert normalised(ws), "operand not normalised"


def h_normalize(ws):
    c = 0
    for i in range(8):
        t = ws[i] + c
        assert 0 <= t < (1 << 32), "fp_normalize: limb + carry overflows 32 bits"
        c = t >> B
    assert ws[8] + c < (1 << B), "fp_normalize: value >= 2^261"
    return limbs(value(ws))


def h_add(a, b):
    need_normalised(a, b)
    return h_normalize([x + y for x, y in zip(a, b)])


def h_dbl(a):
    need_normalised(a)
    return h_normalize([x << 1 for x in a])


def h_neg_raw(pad, k, b):
    """K*p - b limb-wise (fp_neg_raw / fp_neg_raw_k): b normalised, below (K-1) p, no limb above the pad's"""
    need_normalised(b)
    assert value(b) < (k - 1) * P, "pad: b >= (K-1) p"
    assert all(x <= q for x, q in zip(b, pad[k])), "pad: a subtrahend limb exceeds the pad"
    return [q - x for x, q in zip(b, pad[k])]


def h_sub_raw(pad, k, a, b):
    need_normalised(a)
    return [x + y for x, y in zip(a, h_neg_raw(pad, k, b))]


def h_sub_b_2c(a, b, c):
    need_normalised(a, b, c)
    assert value(b) + 2 * value(c) < 4 * P, "fp_sub_b_2c: b + 2c >= 4p"
    assert all(y + 2 * z <= q for y, z, q in zip(b, c, FP29_PAD5_FAT3)), "fp_sub_b_2c: b + 2c exceeds the pad limb"
    return h_normalize([x + (q - y - 2 * z) for x, y, z, q in zip(a, b, c, FP29_PAD5_FAT3)])


def closed_mont(t):
    """(t + m*p) >> 261 with m = -t/p mod 2^261, t = A*B (+ C*D)"""
    assert t < MUL_LIMIT, "product: A*B (+ C*D) >= (2^261 - p) * 2^261"
    q, rem = divmod(t + t * _P_NEG_INV % R261 * P, R261)
    assert rem == 0 and q < R261
    return q


def mont_m(t):
    return t * _P_NEG_INV % R261


def h_mul(pairs, scan=True, where=""):
    """fp_mul / fp_sqr (one pair) and fp_mul_add (two): the product scan of fp_bn254.hpp column by column, one 64-bit accumulator.  A factor may be
    RAW (limbs up to 2^29 + 2^30) as far as every column stays below 2^64; scan=False (normalised factors only: a column is then at most
    27 * (2^29 - 1)^2 + carry < 2^63) returns the closed form alone"""
    t = sum(value(a) * value(b) for a, b in pairs)
    want = closed_mont(t)
    if not scan:
        for a, b in pairs:
            need_normalised(a, b)
        return limbs(want)
    for a, b in pairs:
        assert len(a) == 9 and len(b) == 9 and all(0 <= w < (1 << 32) for w in list(a) + list(b))
    acc, m, r, biggest = 0, [0] * 9, [0] * 9, 0
    for k in range(17):
        lo, hi = max(0, k - 8), min(k, 8)
        for a, b in pairs:
            acc += sum(a[i] * b[k - i] for i in range(lo, hi + 1))
        acc += sum(m[i] * FP29_P[k - i] for i in range(lo, min(k, 9)))  # m[0 .. k-1] below column 9, m[k-8 .. 8] from there on
        if k < 9:
            m[k] = ((acc & 0xFFFFFFFF) * C["FP29_INV"]) & MASK
            acc += m[k] * FP29_P[0]
            assert acc & MASK == 0
        else:
            r[k - 9] = acc & MASK
        biggest = max(biggest, acc)  # every partial sum of the column is at most its total
        assert acc < (1 << 64), "product: a column accumulator overflows 64 bits"
        acc >>= B
    assert acc < (1 << B), "product: result not normalised"
    r[8] = acc
    if biggest > COLUMN["max"]:
        COLUMN["max"], COLUMN["where"] = biggest, where
    assert r == limbs(want) and value(m) == mont_m(t), "the product scan and the closed form disagree"
    return r


def h_reduce_lt2p(a):
    need_normalised(a)
    v = value(a)
    assert v < 2 * P, "fp_reduce_lt2p: a >= 2p"
    return limbs(v - P if v >= P else v)


def h_is_zero_lt2p(a):
    need_normalised(a)
    assert value(a) < 2 * P, "fp_is_zero_lt2p: a >= 2p"
    return list(a) == [0] * 9 or list(a) == FP29_P


def h_inv(a):
    """fp_inv as written: a^1 .. a^7, then fixed 3-bit windows over p - 2, most significant first"""
    need_normalised(a)
    assert value(a) < 2 * P, "fp_inv: a >= 2p"
    mul = lambda x, y: h_mul([(x, y)], scan=False)
    tab = [a, mul(a, a)]
    tab.append(mul(tab[1], a))
    tab.append(mul(tab[1], tab[1]))
    tab.append(mul(tab[3], a))
    tab.append(mul(tab[2], tab[2]))
    tab.append(mul(tab[5], a))
    acc, started, e = list(FP29_ONE), False, P - 2
    for k in range(84, -1, -1):
        d = (e >> (3 * k)) & 7
        if started:
            for _ in range(3):
                acc = mul(acc, acc)
        if d:
            acc = mul(acc, tab[d - 1]) if started else tab[d - 1]
            started = True
    return acc


def h_unpack(w, shift=0):
    """limb i = bits [29 i - shift, 29 i - shift + 29) of the 256-bit word"""
    v = value32(w) << shift
    return [(v >> (B * i)) & MASK for i in range(9)]


def h_pack(a):
    need_normalised(a)
    assert value(a) < R256, "fp_pack: a >= 2^256"
    return words8(value(a))


_RAW_ONE = [1] + [0] * 8


def _records(elem, n=9):
    return [list(elem[i:i + n]) for i in range(0, len(elem), n)]


def evaluate(op, elem):
    """the words `op` stores for the element; AssertionError where the headers do not allow the call"""
    field, kind, k = op
    elem = [int(w) for w in elem]
    assert op in ALL_OPS and len(elem) == in_words(op), (op_name(op), "unknown operation or wrong element size")
    assert all(0 <= w <= 0xFFFFFFFF for w in elem)
    where = op_name(op)
    if field == 1:
        r = _records(elem)
        a = r[0]
        if kind in WORDS_IN:
            if kind == "UNPACK":
                return h_unpack(a)
            if kind == "UNPACK_SHL5":
                return h_unpack(a, 5)
            return h_mul([(h_unpack(a), C["FP29_IN_MONT"] if kind == "FROM_MONT256" else C["FP29_IN_STD"])], where=where)
        if kind == "NORMALIZE":
            return h_normalize(a)
        need_normalised(*r)
        if kind == "MUL":
            return h_mul([(a, r[1])], where=where)
        if kind == "SQR":
            return h_mul([(a, a)], where=where)
        if kind == "MUL_ADD":
            return h_mul([(a, r[1]), (r[2], r[3])], where=where)
        if kind == "ADD":
            return h_add(a, r[1])
        if kind == "DBL":
            return h_dbl(a)
        if kind == "SUB":
            return h_normalize(h_sub_raw(FP29_PAD, k, a, r[1]))
        if kind == "NEG":
            return h_normalize(h_neg_raw(FP29_PAD, k, a))
        if kind == "SUB_B_2C":
            return h_sub_b_2c(a, r[1], r[2])
        if kind == "REDUCE_LT2P":
            return h_reduce_lt2p(a)
        if kind == "CANONICAL":
            return h_reduce_lt2p(h_mul([(a, FP29_ONE)], where=where))
        if kind == "INV":
            return h_inv(a)
        if kind == "IS_ZERO_LT2P":
            return [int(h_is_zero_lt2p(a))] + [0] * 8
        if kind == "PACK":
            return h_pack(a)
        if kind == "TO_MONT256":
            return h_pack(h_reduce_lt2p(h_mul([(a, C["FP29_OUT_MONT"])], where=where)))
        if kind == "TO_STD":
            return h_pack(h_reduce_lt2p(h_mul([(a, _RAW_ONE)], where=where)))
        if kind == "MUL_NEG_RAW2":
            return h_mul([(h_neg_raw(FP29_PAD, 2, a), r[1])], where=where)
        if kind == "NORMALIZE_NEG_RAW2":
            return h_normalize(h_neg_raw(FP29_PAD, 2, a))
        if kind == "SUB6_NEG_RAW4":
            raw = h_neg_raw(FP29_PAD, 4, a)
            return h_normalize([x + y for x, y in zip(raw, h_neg_raw(FP29_PAD, 6, r[1]))])
        assert kind == "Y3"
        return h_mul([(a, h_sub_raw(FP29_PAD, 8, r[1], r[2])), (h_neg_raw(FP29_PAD, k, r[3]), r[4])], where=where)
    r = _records(elem)
    need_normalised(*r)
    a0, a1 = r[0], r[1]
    if kind == "MUL":
        b0, b1 = r[2], r[3]
        return h_mul([(a0, b0), (a1, h_neg_raw(FP2_PAD, k, b1))], where=where) + h_mul([(a0, b1), (a1, b0)], where=where)
    if kind == "SQR":
        return h_mul([(h_add(a0, a1), h_sub_raw(FP2_PAD, k, a0, a1))], where=where) + h_mul([(h_dbl(a0), a1)], where=where)
    if kind == "SUB":
        return h_normalize(h_sub_raw(FP2_PAD, k, a0, r[2])) + h_normalize(h_sub_raw(FP2_PAD, k, a1, r[3]))
    if kind == "NEG":
        return h_normalize(h_neg_raw(FP2_PAD, k, a0)) + h_normalize(h_neg_raw(FP2_PAD, k, a1))
    if kind == "ADD":
        return h_add(a0, r[2]) + h_add(a1, r[3])
    if kind == "DBL":
        return h_dbl(a0) + h_dbl(a1)
    if kind == "MUL_FP":
        return h_mul([(a0, r[2])], where=where) + h_mul([(a1, r[2])], where=where)
    if kind == "IS_ZERO_LT2P":
        z0, z1 = h_is_zero_lt2p(a0), h_is_zero_lt2p(a1)
        return [int(z0 and z1)] + [0] * 17
    if kind == "IS_ZERO_ANY":
        z0 = h_is_zero_lt2p(h_mul([(a0, FP29_ONE)], where=where))
        z1 = h_is_zero_lt2p(h_mul([(a1, FP29_ONE)], where=where))
        return [int(z0 and z1)] + [0] * 17
    if kind in ("NEG_RAW6_MUL_ONE", "NEG_RAW6_MUL_FP"):
        s = FP29_ONE if kind == "NEG_RAW6_MUL_ONE" else r[2]
        return h_mul([(h_neg_raw(FP2_PAD, 6, a0), s)], where=where) + h_mul([(h_neg_raw(FP2_PAD, 6, a1), s)], where=where)
    assert kind == "CONJ"
    return list(a0) + h_normalize(h_neg_raw(FP2_PAD, k, a1))


_MODEL_CACHE = {}


def model(op, elem):
    key = (op, tuple(int(w) for w in elem))
    if key not in _MODEL_CACHE:
        if len(_MODEL_CACHE) > 200000:
            _MODEL_CACHE.clear()
        _MODEL_CACHE[key] = evaluate(op, elem)
    return list(_MODEL_CACHE[key])


def legal(op, elem):
    """raises AssertionError unless the element is inside what the two headers allow `op` to be called on"""
    model(op, elem)


def is_legal(op, elem):
    try:
        legal(op, elem)
        return True
    except AssertionError:
        return False


# ---- the plain-arithmetic result and the documented bound: from the operands' VALUES alone, no Montgomery model, no pad table --------------------
def plain(op, elem):
    """per output record a dict: res (what the value must be congruent to modulo p), and one of exact (the integer itself, where no reduction
    happens), prod (t: the value is below t / 2^261 + p), below (an exclusive bound), flag (0 / 1), words (8 x 32-bit words out)"""
    field, kind, k = op
    elem = [int(w) for w in elem]
    r = _records(elem)
    v = [value32(x) if (field == 1 and kind in WORDS_IN) else value(x) for x in r]
    prod = lambda t: {"res": t * R261_INV % P, "prod": t}
    exact = lambda x: {"res": x % P, "exact": x}
    if field == 1:
        a = v[0]
        if kind == "MUL":
            return [prod(a * v[1])]
        if kind == "SQR":
            return [prod(a * a)]
        if kind == "MUL_ADD":
            return [prod(a * v[1] + v[2] * v[3])]
        if kind == "ADD":
            return [exact(a + v[1])]
        if kind == "DBL":
            return [exact(2 * a)]
        if kind == "SUB":
            return [exact(a + k * P - v[1])]
        if kind == "NEG":
            return [exact(k * P - a)]
        if kind == "SUB_B_2C":
            return [exact(a + 5 * P - v[1] - 2 * v[2])]
        if kind in ("NORMALIZE", "UNPACK"):
            return [exact(a)]
        if kind == "UNPACK_SHL5":
            return [exact(32 * a)]
        if kind == "PACK":
            return [dict(exact(a), words=True)]
        if kind in ("REDUCE_LT2P", "CANONICAL"):
            return [exact(a % P)]
        if kind == "TO_MONT256":
            return [dict(exact(a * pow(32, -1, P) % P), words=True)]
        if kind == "TO_STD":
            return [dict(exact(a * R261_INV % P), words=True)]
        if kind == "FROM_MONT256":
            return [{"res": 32 * a % P, "below": 2 * P}]
        if kind == "FROM_STD":
            return [{"res": a * R261 % P, "below": 2 * P}]
        if kind == "INV":
            x = a * R261_INV % P
            return [{"res": pow(x, P - 2, P) * R261 % P, "below": 2 * P}]
        if kind == "IS_ZERO_LT2P":
            return [{"flag": int(a % P == 0)}]
        if kind == "MUL_NEG_RAW2":
            return [prod((2 * P - a) * v[1])]
        if kind == "NORMALIZE_NEG_RAW2":
            return [exact(2 * P - a)]
        if kind == "SUB6_NEG_RAW4":
            return [exact(10 * P - a - v[1])]
        assert kind == "Y3"
        return [prod(a * (v[1] + 8 * P - v[2]) + (k * P - v[3]) * v[4])]
    a0, a1 = v[0], v[1]
    if kind == "MUL":
        b0, b1 = v[2], v[3]
        out = [prod(a0 * b0 + a1 * (k * P - b1)), prod(a0 * b1 + a1 * b0)]
        assert out[0]["res"] == (a0 * b0 - a1 * b1) * R261_INV % P
        return out
    if kind == "SQR":
        out = [prod((a0 + a1) * (a0 + k * P - a1)), prod(2 * a0 * a1)]
        assert out[0]["res"] == (a0 * a0 - a1 * a1) * R261_INV % P
        return out
    if kind == "SUB":
        return [exact(a0 + k * P - v[2]), exact(a1 + k * P - v[3])]
    if kind == "NEG":
        return [exact(k * P - a0), exact(k * P - a1)]
    if kind == "ADD":
        return [exact(a0 + v[2]), exact(a1 + v[3])]
    if kind == "DBL":
        return [exact(2 * a0), exact(2 * a1)]
    if kind == "MUL_FP":
        return [prod(a0 * v[2]), prod(a1 * v[2])]
    if kind in FLAG_OUT:
        return [{"flag": int(a0 % P == 0 and a1 % P == 0)}, exact(0)]
    if kind in ("NEG_RAW6_MUL_ONE", "NEG_RAW6_MUL_FP"):
        s = R261 % P if kind == "NEG_RAW6_MUL_ONE" else v[2]
        return [prod((6 * P - a0) * s), prod((6 * P - a1) * s)]
    assert kind == "CONJ"
    return [exact(a0), exact(k * P - a1)]


def check_output(op, elem, out, what=""):
    """one element: limbs == the model's, every limb <= 2^29 - 1, the value inside the documented bound and congruent to the plain result"""
    out = [int(w) for w in out]
    assert len(out) == out_words(op), (what, op_name(op), "wrong size")
    want = model(op, elem)  # raises for an illegal operand, whatever the output
    assert out == want, (what, op_name(op), "not the model's limbs", out, want)
    for rec, pl in zip(_records(out), plain(op, elem)):
        if "flag" in pl:
            assert rec == [pl["flag"]] + [0] * 8, (what, op_name(op), "flag")
            continue
        if pl.get("words"):
            assert rec[8] == 0 and all(0 <= w <= 0xFFFFFFFF for w in rec), (what, op_name(op), "word 8 must be 0")
            v = value32(rec)
            assert v < R256
        else:
            assert 0 <= min(rec) and max(rec) <= MASK, (what, op_name(op), "limb not normalised")
            v = value(rec)
        assert v % P == pl["res"], (what, op_name(op), "not congruent to the plain result")
        if "exact" in pl:
            assert v == pl["exact"], (what, op_name(op), "not the integer plain arithmetic gives")
        elif "prod" in pl:
            assert (v << 261) < pl["prod"] + (P << 261), (what, op_name(op), "value >= t / 2^261 + p")
        else:
            assert v < pl["below"], (what, op_name(op), "value outside the documented bound")
    if op == (1, "INV", 0) and value(elem) % P == 0:
        assert value(out) % P == 0, (what, "fp_inv(0) != 0")


def check_all(op, rows, out, what=""):
    """every element of a launch (rows: n x in_words, out: n x out_words)"""
    assert len(out) == len(rows), what
    for i in range(len(rows)):
        check_output(op, rows[i], out[i], (what, i))


# ---- operand classes ---------------------------------------------------------------------------------------------------------------------------
SQ = math.isqrt(MUL_LIMIT - 1)              # the largest legal square: SQ^2 < MUL_LIMIT <= (SQ + 1)^2, just below 168.78 p
SQ2 = math.isqrt((MUL_LIMIT - 1) // 2)      # four equal operands of fp_mul_add: 2 * SQ2^2 < MUL_LIMIT, just below 119.3 p
assert SQ * SQ < MUL_LIMIT <= (SQ + 1) ** 2 and 2 * SQ2 * SQ2 < MUL_LIMIT <= 2 * (SQ2 + 1) ** 2
assert 16879 * P // 100 > SQ > 16878 * P // 100 and 1194 * P // 10 > SQ2 > 1193 * P // 10


def pick(rnd, lim, i):
    """the mix of a random class: reduced, inflated by multiples of p up to the operation's limit `lim` (exclusive), the top of the range"""
    if i % 3 == 0:
        return rnd.randrange(min(P, lim))
    if i % 3 == 1:
        return rnd.randrange(lim)
    return lim - 1 - rnd.randrange(min(lim, 1 << 20))


def fatten(ls, rnd):
    """the same integer on un-normalised limbs: limb i + 1 lends t to limb i (t * 2^29 more there), as far as limb + carry stays below 2^32"""
    ls = list(ls)
    for i in range(8):
        t = min(ls[i + 1], rnd.randrange(8))
        if ls[i] + (t << B) + 8 < (1 << 32):
            ls[i] += t << B
            ls[i + 1] -= t
    return ls


def random_element(op, rnd, i):
    """one legal element of `op`, class i % 3 of the mix"""
    field, kind, k = op
    L = lambda lim: limbs(pick(rnd, lim, i))
    L2 = lambda lim: limbs(pick(rnd, lim, i + 1))  # the "fat" mix: the second operand from the next class
    big = 100 * P
    if field == 1:
        if kind in WORDS_IN:
            return words8(rnd.getrandbits(256) if i % 3 else rnd.randrange(P))[:8] + [rnd.getrandbits(32)]
        if kind == "MUL":
            return L(SQ + 1) + L2(SQ + 1)
        if kind == "SQR":
            return L(SQ + 1)
        if kind == "MUL_ADD":
            return L(SQ2 + 1) + L2(SQ2 + 1) + L2(SQ2 + 1) + L(SQ2 + 1)
        if kind == "ADD":
            a = pick(rnd, R261, i)
            return limbs(a) + limbs(pick(rnd, R261 - a, i + 1))
        if kind == "DBL":
            return L(1 << 260)
        if kind == "SUB":
            b = pick(rnd, (k - 1) * P, i)
            return limbs(pick(rnd, R261 - k * P + b, i + 1)) + limbs(b)
        if kind == "NEG":
            return L((k - 1) * P)
        if kind == "SUB_B_2C":
            c = pick(rnd, 2 * P, i)
            b = pick(rnd, 4 * P - 2 * c, i + 1)
            return limbs(pick(rnd, R261 - 5 * P + b + 2 * c, i + 2)) + limbs(b) + limbs(c)
        if kind == "NORMALIZE":
            return fatten(L(R261), rnd)
        if kind in ("REDUCE_LT2P", "INV", "IS_ZERO_LT2P"):
            return L(2 * P) if i % 7 else limbs((0, P)[i // 7 % 2])
        if kind in ("CANONICAL", "TO_MONT256", "TO_STD"):
            return L(R261)
        if kind == "PACK":
            return L(R256)
        if kind == "MUL_NEG_RAW2":
            return L(P) + L2(R261)
        if kind == "NORMALIZE_NEG_RAW2":
            return L(P)
        if kind == "SUB6_NEG_RAW4":
            return L(3 * P) + L2(5 * P)
        assert kind == "Y3"
        return L(big) + L2(big) + L(7 * P) + L2((k - 1) * P) + L(big)
    if kind == "MUL":
        return L(big) + L2(big) + L2(big) + L((k - 1) * P)
    if kind == "SQR":
        return L(80 * P) + L2((k - 1) * P)
    if kind == "SUB":
        b0, b1 = pick(rnd, (k - 1) * P, i), pick(rnd, (k - 1) * P, i + 1)
        return limbs(pick(rnd, R261 - k * P + b0, i + 1)) + limbs(pick(rnd, R261 - k * P + b1, i)) + limbs(b0) + limbs(b1)
    if kind in ("NEG", "CONJ"):
        return (L(R261) if kind == "CONJ" else L((k - 1) * P)) + L2((k - 1) * P)
    if kind == "ADD":
        a0, a1 = pick(rnd, R261, i), pick(rnd, R261, i + 1)
        return limbs(a0) + limbs(a1) + limbs(pick(rnd, R261 - a0, i + 1)) + limbs(pick(rnd, R261 - a1, i))
    if kind == "DBL":
        return L(1 << 260) + L2(1 << 260)
    if kind == "MUL_FP":
        return L(SQ + 1) + L2(SQ + 1) + L2(SQ + 1)
    if kind == "IS_ZERO_LT2P":
        return [L(2 * P), limbs(0), limbs(P)][i % 4 % 3] + [limbs(P), limbs(0), L2(2 * P)][i % 5 % 3]
    if kind == "IS_ZERO_ANY":
        zero = lambda: limbs(P * rnd.randrange(169))
        return (L(R261) if i % 4 == 0 else zero()) + (L2(R261) if i % 5 == 0 else zero())
    assert kind in ("NEG_RAW6_MUL_ONE", "NEG_RAW6_MUL_FP")
    return L(5 * P) + L2(5 * P) + (L2(R261) if kind == "NEG_RAW6_MUL_FP" else [])


def random_launch(op, n, rnd):
    rows = [random_element(op, rnd, i) for i in range(n)]
    for row in rows:
        legal(op, row)
    return rows


def _launch(op, rows):
    rows = [[int(w) for w in row] for row in rows]
    for row in rows:
        legal(op, row)
    assert 0 < len(rows) <= 600
    return op, rows


def _cat(*vals):
    """values -> the limbs of each, one after the other"""
    out = []
    for v in vals:
        out += limbs(v) if isinstance(v, int) else list(v)
    return out


ONES8 = [MASK] * 8  # limbs 0..7 all 2^29 - 1: with a top limb of 0, the fullest middle columns of a product


def ones8_below(bound):
    """limbs 0..7 all ones under the largest top limb that keeps the value below `bound`"""
    top = ((bound - 1) >> (8 * B)) - 1
    assert top >= 0
    v = ONES8 + [top]
    assert value(v) < bound <= value(v) + (2 << (8 * B))
    return v


def around_p():
    """0, 1, p - 1, p, p + 1, 2p - 1; p with one bit flipped in each of the nine limbs in turn (the lowest and the highest bit of the limb); values
    whose comparison against p is decided only in limb 0 (p +- 1, p - 1 borrows through all nine limbs) or only in limb 8 (p +- 2^232)"""
    vals = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P - 2, P + (1 << 232), P - (1 << 232), (1 << 232) - 1, 1 << 232]
    for i in range(9):
        for bit in (0, 28) if i < 8 else (0, 21):
            v = P ^ (1 << (B * i + bit))
            assert v < 2 * P
            vals.append(v)
        vals += [P - (1 << (B * i)), P + (1 << (B * i))]
    return vals


WORD_PATTERNS = [R256 - 1, 0, P, P - 1, P + 1, 2 * P, 5 * P, R256 - 2, 0xFFFFFFFF, 0xFFFFFFFF << 224]


def edge_classes(rnd):
    """{name: (op, rows)}: every edge class, one launch each, every element proved legal as it is built"""
    out = {}
    fq = lambda kind, k=0: (1, kind, k)
    fq2 = lambda kind, k=0: (2, kind, k)
    one, zero = value(FP29_ONE), 0
    # ---- products: m all ones (A*B (+ C*D) = p modulo 2^261, so m = -1)
    rows, rows_ma = [], []
    for _ in range(16):
        A = rnd.randrange(84 * P) | 1
        Bv = P * pow(A, -1, R261) % R261
        assert mont_m(A * Bv) == TOP
        rows.append(_cat(A, Bv))
        Cv, Dv = rnd.randrange(84 * P) | 1, rnd.randrange(84 * P)
        A2 = (P - Cv * Dv) * pow(Cv | 1, -1, R261) % R261  # A2 * Cv + Cv * Dv = p modulo 2^261, and A2 < 2^261 with Cv, Dv < 84p is legal
        assert mont_m(A2 * Cv + Cv * Dv) == TOP
        rows_ma.append(_cat(A2, Cv, Cv, Dv))
    rows += [_cat(1, P), _cat(P, 1)]
    out["mul with m all ones"] = _launch(fq("MUL"), rows)
    out["mul_add with m all ones"] = _launch(fq("MUL_ADD"), rows_ma)
    # ---- products: the fullest middle columns; the raw factor at its largest legal limbs
    full = ONES8 + [0]
    out["mul fullest middle columns"] = _launch(fq("MUL"), [full + full, full + ONES8 + [1], _cat(TOP, 2 * P - 1), _cat(TOP, 1 << 260)])
    out["sqr fullest middle columns and the largest square"] = _launch(fq("SQR"), [full, limbs(SQ), limbs(SQ - 1), ones8_below(SQ + 1), limbs(168 * P),
                                                                                    limbs(0), limbs(1), limbs(P), limbs(one)])
    out["mul_add fullest middle columns"] = _launch(fq("MUL_ADD"), [full * 4, ones8_below(SQ2 + 1) * 4])
    zero9 = [0] * 9
    rows = []
    for k in FQ_K["Y3"]:
        # q_i = 2^29 - 1 and x3_i = 0: fp_sub_raw<8> has its largest limbs (pad + 2^29 - 1); y = 0: fp_neg_raw<K> is the pad row itself
        rows.append((k, full + full + zero9 + zero9 + full))
        rows.append((k, ones8_below(100 * P) + ones8_below(100 * P) + zero9 + zero9 + ones8_below(100 * P)))
    for k in FQ_K["Y3"]:
        out["y3<%d> raw factors at their largest limbs" % k] = _launch(fq("Y3", k), [row for kk, row in rows if kk == k])
    out["mul_neg_raw2 raw factor at its largest limbs"] = _launch(fq("MUL_NEG_RAW2"), [zero9 + full, zero9 + limbs(TOP), _cat(P - 1, TOP), _cat(0, 0),
                                                                                        _cat(1, one), zero9 + ones8_below(R261)])
    # ---- products: the top of the domain; factors of 0, 1, p, rep(1)
    out["mul top of the domain"] = _launch(fq("MUL"), [_cat(SQ, SQ), _cat(TOP, (MUL_LIMIT - 1) // TOP), _cat((MUL_LIMIT - 1) // TOP, TOP), _cat(168 * P, 168 * P),
                                                       _cat(TOP, R261 - P - 1), _cat(TOP, P), _cat(TOP, 2 * P - 1)])
    special = [zero, 1, P, one, P - 1, 2 * P - 1]
    others = special + [SQ, rnd.randrange(P), rnd.randrange(SQ)]
    out["mul by 0, 1, p and rep(1)"] = _launch(fq("MUL"), [_cat(s, o) for s in special for o in others] + [_cat(o, s) for s in special for o in others])
    out["mul_add just below its limit"] = _launch(fq("MUL_ADD"), [_cat(SQ2, SQ2, SQ2, SQ2), _cat(168 * P, 168 * P, 0, 0), _cat(0, 0, 168 * P, 168 * P),
                                                                  _cat(SQ, SQ, 0, TOP), _cat(TOP, 0, SQ, SQ), _cat(SQ, SQ, 1, 1)[:27] + limbs(0),
                                                                  _cat(119 * P, 119 * P, 119 * P, 119 * P), _cat(TOP, (MUL_LIMIT - 1) // TOP, 0, 0)]
                                               + [_cat(s, o, o, s) for s in special for o in special])
    # ---- sums and differences
    rows = [_cat(v, TOP - v) for v in [0, TOP, 1, P, (1 << 232) - 1, 1 << 260] + [rnd.randrange(R261) for _ in range(10)]]
    rows += [_cat((1 << 232) - 1, 1), _cat(1, (1 << 232) - 1), _cat(0, 0), _cat(TOP - 1, 1), ONES8 + [5] + limbs(1), ONES8 + [MASK - 1] + limbs(1)]
    out["add to the top and through every carry"] = _launch(fq("ADD"), rows)
    out["dbl to the top and through every carry"] = _launch(fq("DBL"), [limbs(v) for v in (0, 1, (1 << 260) - 1, 1 << 259, P, 84 * P)]
                                                            + [[1 << 28] * 8 + [5], [MASK] * 8 + [(1 << 28) - 1], ones8_below(1 << 260)])
    for k in FQ_K["SUB"]:
        out["sub<%d> at both ends of a and b" % k] = _launch(fq("SUB", k), _sub_rows(rnd, k))
    for k in FQ2_K["SUB"]:
        rows = _sub_rows(rnd, k)
        out["fq2 sub<%d> at both ends of a and b" % k] = _launch(fq2("SUB", k), [x[:9] + y[:9] + x[9:] + y[9:] for x, y in zip(rows, rows[1:] + rows[:1])])
    for k in FQ_K["NEG"]:
        out["neg<%d> up to (K-1)p" % k] = _launch(fq("NEG", k), _neg_rows(rnd, k))
    for k in FQ2_K["NEG"]:
        rows = _neg_rows(rnd, k)
        out["fq2 neg<%d> up to (K-1)p" % k] = _launch(fq2("NEG", k), [x + y for x, y in zip(rows, rows[1:] + rows[:1])])
    for k in FQ2_K["CONJ"]:
        rows = _neg_rows(rnd, k)
        out["fq2 conj<%d> up to (K-1)p" % k] = _launch(fq2("CONJ", k), [limbs(rnd.choice((0, TOP, P, rnd.randrange(R261)))) + y for y in rows])
    out["normalize_neg_raw2"] = _launch(fq("NORMALIZE_NEG_RAW2"), [limbs(v) for v in (0, 1, P - 1, (1 << 232) - 1, 1 << 232, rnd.randrange(P))]
                                        + [ones8_below(P)])
    rows = []
    for a in (0, 1, 3 * P - 1, rnd.randrange(3 * P), value(ones8_below(3 * P))):
        for b in (0, 1, 5 * P - 1, rnd.randrange(5 * P), value(ones8_below(5 * P))):
            rows.append(_cat(a, b))
    out["sub6_neg_raw4 at both ends"] = _launch(fq("SUB6_NEG_RAW4"), rows)
    # b + 2c one below 4p; b_i = c_i = 2^29 - 1 in limbs 0..7: b_i + 2 c_i = 3 * (2^29 - 1), the most a normalised pair can put against the pad limb
    rows = []
    b8 = ones8_below(4 * P // 3)
    assert value(b8) * 3 < 4 * P
    for b, c in [(4 * P - 1, 0), (1, 2 * P - 1), (0, 0), (value(b8), value(b8)), (P, P), (2 * P - 1, P - 1), (rnd.randrange(2 * P), rnd.randrange(P))]:
        assert b + 2 * c < 4 * P
        amax = TOP - 5 * P + b + 2 * c
        for a in (0, amax, rnd.randrange(amax), (1 << 232) - 1):
            rows.append(_cat(a, b, c))
    out["sub_b_2c at both ends"] = _launch(fq("SUB_B_2C"), rows)
    # ---- NORMALIZE
    fat = [(1 << 32) - 1] + [(1 << 32) - 1 - 7] * 7  # limb + carry < 2^32 with the largest carry (7) a 32-bit limb can hand on
    carry = 0
    for w in fat:
        carry = (w + carry) >> B
    rows = [[0] * 9, fat + [MASK - carry], fat + [0], [MASK] * 9, [MASK + 1] + [MASK] * 7 + [MASK - 1]]
    for _ in range(8):
        ws = [rnd.getrandbits(32) & ~7 for _ in range(8)]
        carry = 0
        for w in ws:
            carry = (w + carry) >> B
        rows.append(ws + [rnd.randrange(MASK - carry + 1)])
    out["normalize fat limbs"] = _launch(fq("NORMALIZE"), rows)
    # ---- REDUCE_LT2P, CANONICAL, IS_ZERO_LT2P around p
    vals = around_p()
    for kind in ("REDUCE_LT2P", "IS_ZERO_LT2P", "CANONICAL"):
        out[kind.lower() + " around p"] = _launch(fq(kind), [limbs(v) for v in vals])
    vals = [TOP, 0, 1, TOP - 1, R261 - P, 169 * P, 169 * P - 1, 169 * P + 1]
    for k in range(1, 169, 7):
        vals += [k * P - 1, k * P, k * P + 1]
    vals += [rnd.randrange(R261) for _ in range(16)]
    for kind in ("CANONICAL", "TO_MONT256", "TO_STD"):
        out[kind.lower() + " of any normalised value"] = _launch(fq(kind), [limbs(v) for v in vals])
    rows = [_cat(a, b) for a in (0, P, 1, 2 * P - 1, rnd.randrange(2 * P)) for b in (0, P, P + 1, P - 1, 1)]
    out["fq2 is_zero_lt2p around 0 and p"] = _launch(fq2("IS_ZERO_LT2P"), rows)
    rows = [_cat(a, b) for a in (0, P, 168 * P, 169 * P, 169 * P + 1, TOP, 1) for b in (0, P, 169 * P, 84 * P, 84 * P - 1, TOP)]
    out["fq2 is_zero_any of multiples of p"] = _launch(fq2("IS_ZERO_ANY"), rows)
    # ---- word conversions
    patterns = WORD_PATTERNS + [rnd.getrandbits(256) for _ in range(8)] + [rnd.randrange(P) for _ in range(8)]
    bits = [1 << i for i in range(256)]
    for kind in WORDS_IN:
        out[kind.lower() + " of edge patterns"] = _launch(fq(kind), [words8(v)[:8] + [0xFFFFFFFF] for v in patterns])
        out[kind.lower() + " of every single bit"] = _launch(fq(kind), [words8(v) for v in bits])
    out["pack of edge patterns"] = _launch(fq("PACK"), [limbs(v) for v in patterns])
    out["pack of every single bit"] = _launch(fq("PACK"), [limbs(v) for v in bits])
    # ---- INV
    vals = [0, P, 1, P - 1, P + 1, 2 * P - 1, one, one + P] + [rnd.randrange(2 * P) for _ in range(8)]
    out["inv"] = _launch(fq("INV"), [limbs(v) for v in vals])
    # ---- Fq2: every K at the top of its range, components of 0 and of p, the zero real part, the bounds ec_g2_bn254.hpp writes at its calls
    for k in FQ2_K["MUL"]:
        b1 = (k - 1) * P - 1
        rows = [_cat(a0, a1, b0, b1) for a0, a1, b0 in [(k * P, k * P, k * P), (0, P, P), (P, 0, 0), (TOP // 2, 0, 1), (100 * P, 100 * P, 100 * P),
                                                         (0, 0, 0), (P, P, P), (rnd.randrange(k * P), rnd.randrange(k * P), rnd.randrange(k * P))]]
        rows.append(_cat(k * P, k * P, k * P) + ones8_below((k - 1) * P))
        rows.append(_cat(one, 0, 0, one) if k > 2 else _cat(0, 0, 0, 0))
        out["fq2 mul<%d> with b1 one below (K-1)p" % k] = _launch(fq2("MUL", k), rows)
    for k in FQ2_K["SQR"]:
        a1 = (k - 1) * P - 1
        rows = [_cat(a0, a1) for a0 in (0, P, a1, k * P, 2 * (k - 1) * P - 1, 80 * P, rnd.randrange(k * P))]
        rows += [_cat(0, 0), _cat(P, P), _cat(P, 0), _cat(0, P), _cat(k * P) + ones8_below((k - 1) * P)]
        for v in (1, P - 1, rnd.randrange(P)):
            rows += [_cat(v, v), _cat(P - v, v), _cat(v, P - v)]  # a0 = a1 and a0 = -a1: the real part is zero
        out["fq2 sqr<%d> with a1 one below (K-1)p" % k] = _launch(fq2("SQR", k), rows)
    for name, op, bounds in G2_CALL_BOUNDS:
        rows = []
        for j in range(8):
            top = j == 0
            rows.append(_cat(*[(int(bd * P) - 1) if top else rnd.randrange(int(bd * P)) for bd in bounds]))
        out["fq2 " + name] = _launch(op, rows)
    out["fq2 mul_fp top of the domain"] = _launch(fq2("MUL_FP"), [_cat(SQ, SQ, SQ), _cat(TOP, 0, P), _cat(0, TOP, 2 * P - 1), _cat(P, one, one), _cat(0, 0, 0)])
    out["fq2 neg_raw6_mul_one"] = _launch(fq2("NEG_RAW6_MUL_ONE"), [_cat(a, b) for a in (0, 5 * P - 1, P, value(ones8_below(5 * P))) for b in (0, 5 * P - 1, 1)])
    out["fq2 neg_raw6_mul_fp"] = _launch(fq2("NEG_RAW6_MUL_FP"), [_cat(a, b, s) for a in (0, 5 * P - 1, value(ones8_below(5 * P))) for b in (0, 5 * P - 1)
                                                               for s in (0, TOP, value(full), one)])
    rows = [_cat(v, TOP - v, TOP - v, v) for v in [0, TOP, 1, P, (1 << 232) - 1, rnd.randrange(R261)]]
    out["fq2 add to the top"] = _launch(fq2("ADD"), rows)
    out["fq2 dbl to the top"] = _launch(fq2("DBL"), [_cat((1 << 260) - 1, 0), _cat(0, (1 << 260) - 1), _cat(P, 84 * P), ones8_below(1 << 260) + limbs(1)])
    return out


# the operand bounds ec_g2_bn254.hpp writes next to its calls (multiples of p; fp2_mul: a, a, b, b -- fp2_sqr: a, a), from its comments:
# X < 12, Y < 8, ZZ, ZZZ < 4.2;  u = 2Y < 16;  v < 7.3;  m < 13.8;  s - x3 < 15.1;  P = u2 - X < 14.1;  pp < 6;  r < 10.2;  qv - x3 < 13.9
G2_CALL_BOUNDS = (
    ("sqr<17>(u), u = 2Y < 16", (2, "SQR", 17), (16, 16)),
    ("mul<17>(v, u), v < 7.3, u < 16", (2, "MUL", 17), (7.3, 7.3, 16, 16)),
    ("mul<13>(v, X), X < 12", (2, "MUL", 13), (7.3, 7.3, 12, 12)),
    ("sqr<13>(X)", (2, "SQR", 13), (12, 12)),
    ("sqr<15>(m), m < 13.8", (2, "SQR", 15), (13.8, 13.8)),
    ("mul<17>(m, s - x3), s - x3 < 15.1", (2, "MUL", 17), (13.8, 13.8, 15.1, 15.1)),
    ("mul<9>(w, Y), w < 2.5, Y < 8", (2, "MUL", 9), (2.5, 2.5, 8, 8)),
    ("mul<6>(v, ZZ), ZZ < 4.2", (2, "MUL", 6), (7.3, 7.3, 4.2, 4.2)),
    ("sqr<16>(P), P < 14.1", (2, "SQR", 16), (14.1, 14.1)),
    ("mul<7>(ZZ, pp), pp < 6", (2, "MUL", 7), (4.2, 4.2, 6, 6)),
    ("mul<16>(pp, P)", (2, "MUL", 16), (6, 6, 14.1, 14.1)),
    ("sqr<12>(r), r < 10.2", (2, "SQR", 12), (10.2, 10.2)),
    ("mul<15>(r, qv - x3), qv - x3 < 13.9", (2, "MUL", 15), (10.2, 10.2, 13.9, 13.9)),
    ("mul<4>(ZZZ, ppp), ppp < 2.1", (2, "MUL", 4), (4.2, 4.2, 2.1, 2.1)),
    # (the comment there said qv - x3 < 9.1, above the 9p fp2_mul<10> allows: x3 = r^2 + 5p - (ppp + 2 qv) >= 1.8p, so qv + 8p - x3 < 7.3p)
    ("mul<10>(r, qv - x3), r < 4.5, qv - x3 < 7.3", (2, "MUL", 10), (4.5, 4.5, 7.3, 7.3)),
    ("mul<3>(ppp, s1), s1 < 1.5", (2, "MUL", 3), (1.1, 1.1, 1.5, 1.5)),
)


def _sub_rows(rnd, k):
    """(a, b) of fp_sub<K> / a component of fp2_sub<K>: b one below (K-1)p, b with every limb 0..7 at 2^29 - 1 (the pad limb less what the pad has
    above it), a at 0 and where a + K p - b = 2^261 - 1; a borrow-free and a carry-rippling a"""
    bmax = (k - 1) * P - 1
    ones = value(ones8_below((k - 1) * P))
    rows = []
    for bv in [bmax, 0, ones, P - 1, 1] + [rnd.randrange(bmax + 1) for _ in range(3)]:
        amax = TOP - k * P + bv
        for av in (0, bv, amax, 1, (1 << 232) - 1, rnd.randrange(amax + 1)):
            if av <= amax:
                rows.append(_cat(av, bv))
    return rows


def _neg_rows(rnd, k):
    bmax = (k - 1) * P - 1
    return [limbs(v) for v in (bmax, 0, 1, P, P - 1, (1 << 232) - 1, rnd.randrange(bmax + 1)) if v <= bmax] + [ones8_below((k - 1) * P)]


def roundtrip_patterns(rnd):
    """the 256-bit patterns of the PACK(UNPACK(w)) == w, TO_STD(FROM_STD(w)) == w mod p and TO_MONT256(FROM_MONT256(w)) == w mod p checks"""
    vals = WORD_PATTERNS + [1 << i for i in range(256)] + [rnd.getrandbits(256) for _ in range(8)] + [rnd.randrange(P) for _ in range(8)]
    return [words8(v) for v in vals]


def crosscheck_values(rnd):
    return [0, 1, P - 1, P - 2] + [rnd.randrange(P) for _ in range(61)]


def crosscheck_launches(run, vals):
    """msm_test_fp_op's ops 2, 3, 4 on canonical words, composed from the raw operations through run(op, rows) -> out:
    ({2: to_mont256(mul(from_mont256 a, from_mont256 b)), 3: to_mont256(from_std a), 4: to_std(from_mont256 a)}, a, b); b is a reversed"""
    a, b = [words8(v) for v in vals], [words8(v) for v in reversed(vals)]
    fm_a, fm_b = run((1, "FROM_MONT256", 0), a), run((1, "FROM_MONT256", 0), b)
    prod = run((1, "MUL", 0), [list(x) + list(y) for x, y in zip(fm_a, fm_b)])
    out = {2: run((1, "TO_MONT256", 0), prod), 3: run((1, "TO_MONT256", 0), run((1, "FROM_STD", 0), a)), 4: run((1, "TO_STD", 0), fm_a)}
    assert [value32(x) for x in out[2]] == [x * y * pow(R256, -1, P) % P for x, y in zip(vals, reversed(vals))]
    assert [value32(x) for x in out[3]] == [x * R256 % P for x in vals] and [value32(x) for x in out[4]] == [x * pow(R256, -1, P) % P for x in vals]
    return out, a, b


# ---- a chain of the Y3 of xyzz_madd composed from the operations, fed back from its own outputs ----------------------------------------------
CHAIN_ROUNDS = 16
OP_SUB8, OP_NEG6, OP_MUL_ADD, OP_SUB5 = (1, "SUB", 8), (1, "NEG", 6), (1, "MUL_ADD", 0), (1, "SUB", 5)


def chain_start(rnd, n):
    """(x, y): x just below 7p (the X of an accumulator), y just below 4p"""
    x = [limbs(7 * P - 1 - rnd.randrange(1 << 20)) for _ in range(n)]
    y = [limbs(4 * P - 1 - rnd.randrange(1 << 20)) for _ in range(n)]
    x[0], y[0] = limbs(7 * P - 1), limbs(4 * P - 1)
    return x, y


def chain_round(run, s, x, y, what="chain"):
    """one round through run(op, rows) -> out, the shape of the Y3 of xyzz_madd: d = SUB<8>(y, x), e = NEG<6>(y), t = MUL_ADD(x, d, e, x),
    x' = SUB<5>(t, y), y' = t.  Bounds: x < 7p (the subtrahend of the 8p pad) and y < 4p (of the 5p and 6p pads) on the way in; d < 12p, e <= 6p,
    t < (7 * 12 + 6 * 7) p^2 / 2^261 + p < 1.75p, x' = t + 5p - y < 6.75p: the bounds close, and from the second round on (y < 1.75p) x' > 3.25p
    stays outside the reduced range"""
    assert all(value(r) < 7 * P for r in x) and all(value(r) < 4 * P for r in y), (what, s, "bound on the way in")
    d = run(OP_SUB8, [list(b) + list(a) for a, b in zip(x, y)])
    e = run(OP_NEG6, [list(b) for b in y])
    assert all(value(r) < 12 * P for r in d) and all(value(r) <= 6 * P for r in e), (what, s)
    t = run(OP_MUL_ADD, [list(a) + list(dd) + list(ee) + list(a) for a, dd, ee in zip(x, d, e)])
    assert all(4 * value(r) < 7 * P for r in t), (what, s, "t >= 1.75p")
    xn = run(OP_SUB5, [list(tt) + list(b) for tt, b in zip(t, y)])
    assert all(value(r) < 7 * P for r in xn) and (s == 0 or all(value(r) > 3 * P for r in xn)), (what, s, "x' outside (3p, 7p)")
    return xn, t


def checked(run):
    """run(op, rows) -> out with every element of every launch through check_output"""
    def go(op, rows):
        out = run(op, rows)
        check_all(op, rows, out, ("chain", op_name(op)))
        return [list(int(w) for w in r) for r in out]
    return go


# ---- the records file tools/fq_bounds_check.cpp reads ----------------------------------------------------------------------------------------
def launch_words(op, rows):
    """one launch as 32-bit words: field, op word, n, then the n elements"""
    flat = [op[0], op_word(op), len(rows)]
    for row in rows:
        assert len(row) == in_words(op)
        flat += [int(w) for w in row]
    return flat


# four operands of 128p: inside the header's former "normalised and < 128p", outside A*B + C*D < (2^261 - p) * 2^261: the top limb leaves 29 bits
ILLEGAL_MUL_ADD = ((1, "MUL_ADD", 0), [_cat(128 * P - 1, 128 * P - 1, 128 * P - 1, 128 * P - 1)])
assert not is_legal(*[ILLEGAL_MUL_ADD[0], ILLEGAL_MUL_ADD[1][0]])
