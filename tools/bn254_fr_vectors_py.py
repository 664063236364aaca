"""Pure-Python yardstick of the scalar-vector calls (msm_bn254_fr_powers_device, _batch_inverse(_device), _lagrange_device, _lincomb_device):
Python integers modulo r and nothing of the library.  tests/test_fr_vectors_cpu.py checks it against the definitions (x * x^-1 = 1, sum_i L_i(tau)
p(w^i) = p(tau)) and then the CPU run of the kernels' routines against it; tests/test_gpu_13_fr_vectors.py checks the GPU against it, word for word.

Words: an element is 8 little-endian 32-bit words; `mont` names arkworks' Fr.0 form (x * 2^256 mod r).  Inputs are ANY 256-bit patterns, read
modulo r; outputs are canonical."""
import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT_R = (1 << 256) % R
MONT_R_INV = pow(MONT_R, -1, R)
ROOT28 = 19103219067921713944291392827692070036145651957329286315305642004821462161904  # 5^((r-1)/2^28): arkworks' TWO_ADIC_ROOT_OF_UNITY


def root_of_unity(log_n):
    assert 0 <= log_n <= 28
    return pow(ROOT28, 1 << (28 - log_n), R)


def inverse(x):
    """x^-1 modulo r; 0 for x = 0 (mod r), as arkworks' batch_inversion leaves it"""
    return pow(x % R, R - 2, R)


def batch_inverse(xs):
    return [inverse(x) for x in xs]


def powers(base, n, scale=1, first=0):
    """scale * base^(first + i), i < n; 0^0 = 1"""
    cur, out = scale % R * pow(base % R, first, R) % R, []
    for _ in range(n):
        out.append(cur)
        cur = cur * base % R
    if base % R == 0 and first == 0 and n:
        out[0] = scale % R
    return out


def lagrange(tau, log_n):
    """L_i(tau) = Z(tau) w^i / (n (tau - w^i)) over the domain of 2^log_n points; the unit vector when tau is one of them"""
    n, w, tau = 1 << log_n, root_of_unity(log_n), tau % R
    dom = powers(w, n)
    if pow(tau, n, R) == 1:
        return [1 if x == tau else 0 for x in dom]
    zn = (pow(tau, n, R) - 1) * inverse(n) % R
    return [zn * x % R * inverse(tau - x) % R for x in dom]


def lincomb(a, ka=1, b=None, kb=1, c=None, kc=1):
    out = [x * ka % R for x in a]
    if b is not None:
        out = [(o + y * kb) % R for o, y in zip(out, b)]
    if c is not None:
        out = [(o + y * kc) % R for o, y in zip(out, c)]
    return out


def to_words(values):
    """integers < 2^256, as they are (NOT reduced), -> n x 8 uint32"""
    out = np.zeros((len(values), 8), np.uint32)
    for i, v in enumerate(values):
        assert 0 <= v < 1 << 256
        out[i] = [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]
    return out


def from_words(words):
    return [sum(int(w) << (32 * k) for k, w in enumerate(row)) for row in np.asarray(words).reshape(-1, 8).tolist()]


def read(patterns, mont=False):
    """what a call reads from these 256-bit patterns: the field elements"""
    return [p % R * MONT_R_INV % R if mont else p % R for p in patterns]


def write(values, mont=False):
    """the canonical words a call writes for these field elements"""
    return to_words([v % R * MONT_R % R if mont else v % R for v in values])


def patterns(seed, n):
    """n seeded 256-bit patterns (most of them >= r)"""
    rng = np.random.default_rng(seed)
    return from_words(rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32))
