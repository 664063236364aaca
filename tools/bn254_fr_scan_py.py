"""Pure-Python yardstick of the scalar-field scans (msm_bn254_fr_poly_eval_device, _poly_div_linear(_device), _running_product_device):
Python integers modulo r and nothing of the library.  tests/test_fr_scan_cpu.py checks it against the definitions (the O(n^2) sums,
q (X - z) + rem = p, a plain loop) and then the CPU run of the kernels' routines against it; tests/test_gpu_25_fr_scan.py checks the GPU against
it, word for word.

Words: an element is 8 little-endian 32-bit words; `mont` names arkworks' Fr.0 form (x * 2^256 mod r).  Inputs are ANY 256-bit patterns, read
modulo r; outputs are canonical."""
import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT_R = (1 << 256) % R
MONT_R_INV = pow(MONT_R, -1, R)


def poly_eval(c, z):
    """sum_i c[i] z^i"""
    acc = 0
    for x in reversed(c):
        acc = (acc * z + x) % R
    return acc


def poly_div_linear(c, z):
    """(q, rem): p(X) = q(X) (X - z) + rem, q as long as c with q[n - 1] = 0.  Horner from the top coefficient down; nothing is inverted."""
    n, z = len(c), z % R
    q, acc = [0] * n, 0
    for j in range(n - 1, -1, -1):
        q[j] = acc
        acc = (acc * z + c[j]) % R
    return q, acc


def running_product(x, exclusive=False):
    """(out, total): out[i] = x[0] .. x[i], or x[0] .. x[i - 1] with out[0] = 1 when exclusive; total = the product of all"""
    out, run = [], 1
    for v in x:
        if exclusive:
            out.append(run)
        run = run * v % R
        if not exclusive:
            out.append(run)
    return out, run


def mul_linear(s, z):
    """the coefficients of (X - z) s(X): one more than s has"""
    z = z % R
    out = [0] * (len(s) + 1)
    for i, v in enumerate(s):
        out[i + 1] = (out[i + 1] + v) % R
        out[i] = (out[i] - z * v) % R
    return out


def to_words(values):
    """integers < 2^256, as they are (NOT reduced), -> n x 8 uint32"""
    raw = b"".join(v.to_bytes(32, "little") for v in values)  # (raises for a value outside 0 .. 2^256 - 1)
    return np.frombuffer(raw, dtype="<u4").astype(np.uint32).reshape(len(values), 8)


def from_words(words):
    raw = np.ascontiguousarray(np.asarray(words).reshape(-1, 8), dtype="<u4").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def read(patterns, mont=False):
    """what a call reads from these 256-bit patterns: the field elements"""
    return [p % R * MONT_R_INV % R if mont else p % R for p in patterns]


def encode(values, mont=False):
    """canonical integers whose words a call reads as these field elements"""
    return [v % R * MONT_R % R if mont else v % R for v in values]


def write(values, mont=False):
    """the canonical words a call writes for these field elements"""
    return to_words(encode(values, mont))


def patterns(seed, n):
    """n seeded 256-bit patterns (most of them >= r)"""
    rng = np.random.default_rng(seed)
    return from_words(rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32))


# the classes of tests/test_fr_scan_cpu.py and tests/test_gpu_25_fr_scan.py
def points(seed):
    """z: 0, 1, r - 1, two spellings above r, a random pattern"""
    return [0, 1, R - 1, R + 5, (1 << 256) - 1, patterns(seed, 1)[0]]


def coefficient_sets(seed, n, z, mont=False):
    """name -> n patterns: all zero, all r - 1, all 2^256 - 1, random patterns, (X - z) s for a random s (read in the given form), X^(n - 1)"""
    s = [v % R for v in patterns(seed + 1, n - 1)]
    return {
        "zero": [0] * n,
        "r-1": [R - 1] * n,
        "ones": [(1 << 256) - 1] * n,
        "random": patterns(seed, n),
        "multiple": encode(mul_linear(s, z), mont) if n > 1 else [0],
        "monomial": encode([0] * (n - 1) + [1], mont),
    }


def product_sets(seed, n, zero_at=()):
    """name -> n patterns: all ones, random patterns (none of them 0 mod r), and the random set with a zero (spelled 0, r, 2r, 5r in turn) at each
    place of zero_at below n"""
    rnd = [x if x % R else 1 for x in patterns(seed, n)]
    sets = {"one": [1] * n, "random": rnd}
    for t, at in enumerate(zero_at):
        if 0 <= at < n:
            xs = list(rnd)
            xs[at] = (0, R, 2 * R, 5 * R)[t % 4]
            sets["zero@%d" % at] = xs
    return sets
