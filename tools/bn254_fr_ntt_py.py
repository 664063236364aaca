#!/usr/bin/env python3
"""Pure-Python yardstick of the BN254 scalar-field transforms (msm_bn254_fr_ntt*): an iterative radix-2 transform over Python ints and the
O(n^2) definition it is checked against.  Independent of the C++: nothing here is shared with fr_bn254.hpp / ntt_bn254.hpp.

    forward:  A[j] = sum_i a[i] (g w^j)^i        w = root(log2 n), g = 1 without a coset
    inverse:  the exact inverse of that (1/n included, times g^-i afterwards)
"""
import numpy as np

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
ROOT28 = pow(5, (R - 1) >> 28, R)
MONT = 1 << 256  # arkworks' Fr.0 holds x * 2^256 mod r
INVERSE, IN_MONT, OUT_MONT = 1, 2, 4  # MSM_NTT_*


def root(log_n):
    assert 0 <= log_n <= 28
    return pow(ROOT28, 1 << (28 - log_n), R)


def ntt_definition(a, g=1, inverse=False):
    """O(n^2), straight from the definition"""
    n = len(a)
    k = n.bit_length() - 1
    assert 1 << k == n
    w = root(k)
    if not inverse:
        return [sum(a[i] * pow(g * pow(w, j, R) % R, i, R) for i in range(n)) % R for j in range(n)]
    wi, ni, gi = pow(w, R - 2, R), pow(n, R - 2, R), pow(g, R - 2, R)
    return [sum(a[j] * pow(wi, i * j, R) for j in range(n)) * ni * pow(gi, i, R) % R for i in range(n)]


def _radix2(a, w):
    """in natural order, out natural order (bit-reversal first, then decimation in time)"""
    n = len(a)
    k = n.bit_length() - 1
    a = [a[int(format(i, "0%db" % k)[::-1], 2)] if k else a[i] for i in range(n)]
    half = 1
    while half < n:
        ws = pow(w, n // (2 * half), R)
        tw = [1] * half
        for e in range(1, half):
            tw[e] = tw[e - 1] * ws % R
        for s in range(0, n, 2 * half):
            for e in range(half):
                u, x = a[s + e], a[s + e + half] * tw[e] % R
                a[s + e], a[s + e + half] = (u + x) % R, (u - x) % R
        half *= 2
    return a


def ntt(a, g=1, inverse=False):
    a = [x % R for x in a]
    n = len(a)
    k = n.bit_length() - 1
    assert 1 << k == n
    w = root(k)
    if not inverse:
        if g != 1:
            p = 1
            for i in range(n):
                a[i] = a[i] * p % R
                p = p * g % R
        return _radix2(a, w)
    a = _radix2(a, pow(w, R - 2, R))
    ni, gi = pow(n, R - 2, R), pow(g, R - 2, R)
    p = ni
    for i in range(n):
        a[i] = a[i] * p % R
        p = p * gi % R
    return a


# ---- the calls' view: arrays of 8 little-endian 32-bit words ------------------------------------------------------------------------------
def to_words(vals):
    out = np.zeros((len(vals), 8), np.uint32)
    for i, v in enumerate(vals):
        for j in range(8):
            out[i, j] = (v >> (32 * j)) & 0xFFFFFFFF
    return out


def from_words(words):
    w = np.asarray(words, dtype=np.uint32).reshape(-1, 8)
    return [sum(int(x) << (32 * j) for j, x in enumerate(row.tolist())) for row in w]


MONT_INV = pow(MONT, R - 2, R)


def ntt_words(words, log_n, batch=1, flags=0, g=None):
    """what msm_bn254_fr_ntt(_device) leaves: any input pattern is read modulo r, outputs are canonical"""
    vals = from_words(words)
    n = 1 << log_n
    assert len(vals) == n * batch
    if flags & IN_MONT:
        vals = [v * MONT_INV % R for v in vals]
    out = []
    for b in range(batch):
        out += ntt(vals[b * n:(b + 1) * n], 1 if g is None else g, bool(flags & INVERSE))
    if flags & OUT_MONT:
        out = [v * MONT % R for v in out]
    return to_words(out)


def mul_sub_scale_words(a, b, c=None, k=None, flags=0):
    """msm_bn254_fr_mul_sub_scale_device"""
    a, b = from_words(a), from_words(b)
    c = from_words(c) if c is not None else [0] * len(a)
    if flags & IN_MONT:
        a, b, c = ([v * MONT_INV % R for v in x] for x in (a, b, c))
    out = [(x * y - z) * (1 if k is None else k) % R for x, y, z in zip(a, b, c)]
    if flags & OUT_MONT:
        out = [v * MONT % R for v in out]
    return to_words(out)


if __name__ == "__main__":
    import random
    rng = random.Random(1)
    for k in range(0, 6):
        a = [rng.randrange(R) for _ in range(1 << k)]
        for g in (1, 5, root(k + 1)):
            assert ntt(a, g) == ntt_definition(a, g)
            assert ntt(a, g, True) == ntt_definition(a, g, True)
            assert ntt(ntt(a, g), g, True) == a
    print("ok")
