#!/usr/bin/env python3
"""Pure-Python yardstick of the R1CS rows (msm_bn254_fr_r1cs_*): a = A w, b = B w, c = C w (or c = a o b) over Python ints mod r, and a seeded
generator of synthetic circuits.  Independent of the C++: nothing here is shared with fr_bn254.hpp / r1cs_bn254.hpp.

A coefficient list is a list of (matrix, row, col, value) with value the 256-bit pattern as handed to the library (an int < 2^256, read modulo r
in the form the upload names)."""
import random

import numpy as np

from bn254_fr_ntt_py import IN_MONT, MONT, MONT_INV, OUT_MONT, R, from_words, to_words

COEF_STD, COEF_MONT, COEF_MONT2 = 0, 1, 2  # MSM_R1CS_COEF_*
C_FROM_AB = 8                              # MSM_R1CS_C_FROM_AB
COEF_DTYPE = np.dtype([("matrix", "<u4"), ("row", "<u4"), ("col", "<u4"), ("value", "<u4", (8,))])  # msm_r1cs_coef_t


def coef_value(pattern, form):
    """the coefficient a 256-bit pattern stands for"""
    return pattern * pow(MONT_INV, form, R) % R


def coef_pattern(c, form):
    """the canonical pattern of coefficient c in a form"""
    return c % R * pow(MONT, form, R) % R


def evaluate(coefs, form, witness, log_n, from_ab=False):
    """integers in, integers out: the lists a, b, c of 2^log_n values each"""
    n = 1 << log_n
    abc = [[0] * n for _ in range(3)]
    for m, row, col, v in coefs:
        abc[m][row] = (abc[m][row] + coef_value(v, form) * witness[col]) % R
    if from_ab:
        abc[2] = [x * y % R for x, y in zip(abc[0], abc[1])]
    return abc


def eval_words(coefs, form, witness_words, log_n, flags=0):
    """what msm_bn254_fr_r1cs_eval(_device) leaves: the (3 * 2^log_n) x 8 words [a | b | c]; any witness pattern is read modulo r"""
    w = from_words(witness_words)
    if flags & IN_MONT:
        w = [v * MONT_INV % R for v in w]
    a, b, c = evaluate(coefs, form, w, log_n, bool(flags & C_FROM_AB))
    out = a + b + c
    if flags & OUT_MONT:
        out = [v * MONT % R for v in out]
    return to_words(out)


def pack(coefs):
    """the list as an array of msm_r1cs_coef_t records"""
    out = np.zeros(len(coefs), COEF_DTYPE)
    for i, (m, row, col, v) in enumerate(coefs):
        out[i] = (m, row, col, [(v >> (32 * j)) & 0xFFFFFFFF for j in range(8)])
    return out


def synthetic(seed, rows, cols, mean_len=(3, 2, 1), pm1_share=0.9, long_rows=0, long_len=0, form=COEF_STD, distinct=64, shuffle=True):
    """a seeded circuit: per matrix m (mean_len[m] == 0: no entries) every row draws 1 .. 2 * mean_len[m] - 1 entries at random columns (mean
    mean_len[m]); a share pm1_share of the coefficients is +1 or -1 (evenly), the others come from `distinct` random values; the first
    `long_rows` rows of matrix 0 (spread over the rows) get long_len entries instead.  The list is shuffled: entries come in any order."""
    rnd = random.Random(seed)
    others = [rnd.randrange(2, R - 1) for _ in range(distinct)]
    long_at = {(i * rows) // max(long_rows, 1) for i in range(long_rows)}
    out = []
    for m, mean in enumerate(mean_len):
        if not mean:
            continue
        for row in range(rows):
            cnt = long_len if (m == 0 and row in long_at) else rnd.randint(1, 2 * mean - 1)
            for _ in range(cnt):
                u = rnd.random()
                c = (1 if u < pm1_share / 2 else R - 1) if u < pm1_share else others[rnd.randrange(distinct)]
                out.append((m, row, rnd.randrange(cols), coef_pattern(c, form)))
    if shuffle:
        rnd.shuffle(out)
    return out


def synthetic_array(seed, rows, cols, mean_len=(3, 2, 0), pm1_share=0.9, long_rows=0, long_len=0, distinct=64):
    """the same kind of circuit straight into a record array (numpy; for sizes the list form is too slow for), standard-form values, unshuffled"""
    g = np.random.default_rng(seed)
    rnd = random.Random(seed)
    others = np.array([[(v >> (32 * j)) & 0xFFFFFFFF for j in range(8)] for v in (rnd.randrange(2, R - 1) for _ in range(distinct))], np.uint32)
    one = np.array([1, 0, 0, 0, 0, 0, 0, 0], np.uint32)
    minus = np.array([((R - 1) >> (32 * j)) & 0xFFFFFFFF for j in range(8)], np.uint32)
    parts = []
    for m, mean in enumerate(mean_len):
        if not mean:
            continue
        cnt = g.integers(1, 2 * mean, size=rows)
        if m == 0 and long_rows:
            cnt[(np.arange(long_rows) * rows) // long_rows] = long_len
        rec = np.zeros(int(cnt.sum()), COEF_DTYPE)
        rec["matrix"] = m
        rec["row"] = np.repeat(np.arange(rows, dtype=np.uint32), cnt)
        rec["col"] = g.integers(0, cols, size=rec.shape[0], dtype=np.uint32)
        u = g.random(rec.shape[0])
        val = others[g.integers(0, distinct, size=rec.shape[0])]
        val[u < pm1_share] = minus
        val[u < pm1_share / 2] = one
        rec["value"] = val
        parts.append(rec)
    return np.concatenate(parts)


def edge_circuit(form=COEF_STD, with_c=True, item_len=24, rows=300, cols=211, seed=0x52314353):
    """the circuit of the word-for-word tests (rows x cols, for a domain of 2^9): in matrix 0 rows of 0, 1, L, L + 1 and 3L + 1 entries (L = the
    library's item length) and one of 64L + 5 (more than 64 work items); elsewhere 0 to 4 entries per row; coefficients 0, 1, r - 1, 2, r - 2,
    random ones and patterns >= r; repeated (matrix, row, col) entries; matrix 2 with entries or without; shuffled"""
    rnd = random.Random(seed)
    special = [0, 1, R - 1, 2, R - 2]

    def pattern():
        u = rnd.random()
        c = special[rnd.randrange(5)] if u < 0.6 else rnd.randrange(R)
        p = coef_pattern(c, form)
        if rnd.random() < 0.25:  # the same coefficient as a pattern >= r (5 r < 2^256)
            p += R * rnd.randint(1, 4)
        return p

    fixed = {0: 0, 1: 1, 2: item_len, 3: item_len + 1, 4: 3 * item_len + 1, 5: 64 * item_len + 5}
    out = []
    for m in range(3 if with_c else 2):
        for row in range(rows):
            cnt = fixed[row] if (m == 0 and row in fixed) else rnd.randint(0, 4)
            for _ in range(cnt):
                out.append((m, row, rnd.randrange(cols), pattern()))
    for _ in range(40):  # repeated (matrix, row, col): they add up
        m, row, col, _v = out[rnd.randrange(len(out))]
        if m == 0 and row in fixed:  # (the rows of fixed length keep it)
            continue
        out.append((m, row, col, pattern()))
    out += [(0, 7, 3, coef_pattern(5, form)), (0, 7, 3, coef_pattern(R - 5, form))]  # ... here to zero (row 0 stays the row without entries)
    rnd.shuffle(out)
    return out


def edge_witness(n, seed=0x5731):
    """n elements of 8 words: mostly canonical, some patterns >= r (read modulo r), the all-ones word among them"""
    rnd = random.Random(seed)
    vals = [rnd.randrange(R) for _ in range(n)]
    for i in range(0, n, 7):
        vals[i] = rnd.randrange(R, 1 << 256)
    vals[rnd.randrange(n)] = (1 << 256) - 1
    return to_words(vals)


def overflow_circuit(item_len=24):
    """three rows of 4L + 1 entries each, all +1, all -1 (as r - 1) and all r - 2, over 4L + 1 columns: with every witness word 2^256 - 1 these
    are the largest lazy sums the kernels can meet"""
    n = 4 * item_len + 1
    return [(0, row, col, c) for row, c in enumerate((1, R - 1, R - 2)) for col in range(n)], n


if __name__ == "__main__":
    rnd = random.Random(1)
    cs = synthetic(5, 40, 30, long_rows=2, long_len=100)
    w = [rnd.randrange(R) for _ in range(30)]
    a, b, c = evaluate(cs, COEF_STD, w, 6)
    dense = [[[0] * 30 for _ in range(64)] for _ in range(3)]
    for m, row, col, v in cs:
        dense[m][row][col] = (dense[m][row][col] + v) % R
    for m, got in enumerate((a, b, c)):
        assert got == [sum(x * y for x, y in zip(dense[m][i], w)) % R for i in range(64)]
    print("ok")
