#!/usr/bin/env python3
"""Independent pure-Python-integer BN254 G2 group law (test infrastructure only; the product never imports it).

G2 is the order-r subgroup of the sextic twist E'(Fq2): y^2 = x^3 + 3/(9+u), Fq2 = Fq[u]/(u^2+1).  Points are affine pairs of Fq2 elements
((x0, x1), (y0, y1)) with None for the point at infinity; the law is the textbook chord / tangent over Fq2 with one inversion per operation.
Shares nothing with gpu-acceleration_amd/ (no constants, no formulas): the generator below is the standard one (EIP-197), the endomorphism
check uses the G1 GLV constants recomputed from scratch.
"""
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R256 = 1 << 256

G2_GEN = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
           11559732032986387107991004021392285783925812861821192530917403151452391805634),
          (8495653923123431417604973247489272438418190587263600148770280649306958101930,
           4082367875863433681332203403145435568316851327593401208105741076214120093531))


def f2(a0, a1=0):
    return (a0 % P, a1 % P)


def add2(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def sub2(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def neg2(a):
    return ((-a[0]) % P, (-a[1]) % P)


def mul2(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def inv2(a):
    t = pow((a[0] * a[0] + a[1] * a[1]) % P, P - 2, P)
    return (a[0] * t % P, (-a[1]) * t % P)


def smul2(a, s):
    return (a[0] * s % P, a[1] * s % P)


B_TWIST = mul2((3, 0), inv2((9, 1)))  # 3 / (9 + u)


def on_curve(pt):
    if pt is None:
        return True
    x, y = pt
    return sub2(mul2(y, y), add2(mul2(mul2(x, x), x), B_TWIST)) == (0, 0)


def neg(pt):
    return None if pt is None else (pt[0], neg2(pt[1]))


def add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if add2(y1, y2) == (0, 0):
            return None
        lam = mul2(smul2(mul2(x1, x1), 3), inv2(smul2(y1, 2)))
    else:
        lam = mul2(sub2(y2, y1), inv2(sub2(x2, x1)))
    x3 = sub2(sub2(mul2(lam, lam), x1), x2)
    return (x3, sub2(mul2(lam, sub2(x1, x3)), y1))


def mul(pt, k):
    k %= R
    acc, base = None, pt
    while k:
        if k & 1:
            acc = add(acc, base)
        base = add(base, base)
        k >>= 1
    return acc


def mul_raw(pt, k):
    """k * pt WITHOUT reducing k mod r (order checks)"""
    acc, base = None, pt
    while k:
        if k & 1:
            acc = add(acc, base)
        base = add(base, base)
        k >>= 1
    return acc


def msm(points, scalars):
    acc = None
    for p_, s in zip(points, scalars):
        acc = add(acc, mul(p_, s))
    return acc


# ---- word images (little-endian u32; the C ABI's x.c0, x.c1, y.c0, y.c1 order) -------------------------------------------------
def int_words(v, n=8):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def words_int(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def point_words(pt, mont=False):
    if pt is None:
        return [0] * 32
    f = (lambda v: v * R256 % P) if mont else (lambda v: v)
    (x0, x1), (y0, y1) = pt
    return int_words(f(x0)) + int_words(f(x1)) + int_words(f(y0)) + int_words(f(y1))


def affine_words_std(pt):
    return point_words(pt, False)


def from_mont_words(ws):
    ri = pow(R256, -1, P)
    return [words_int(ws[8 * k:8 * k + 8]) * ri % P for k in range(len(ws) // 8)]


def jacobian_mont_to_affine(ws):
    """48 Jacobian Montgomery words (X.c0 X.c1 Y.c0 Y.c1 Z.c0 Z.c1) -> affine point or None"""
    v = from_mont_words(ws)
    X, Y, Z = (v[0], v[1]), (v[2], v[3]), (v[4], v[5])
    if Z == (0, 0):
        return None
    zi = inv2(Z)
    zi2 = mul2(zi, zi)
    return (mul2(X, zi2), mul2(Y, mul2(zi2, zi)))


def jacobian_mont_words(pt, z=(1, 0)):
    """Jacobian Montgomery words of pt with the given Z (None: the identity (1, 1, 0))"""
    if pt is None:
        return [w for v in (1, 0, 1, 0, 0, 0) for w in int_words(v * R256 % P)]
    z2 = mul2(z, z)
    X, Y = mul2(pt[0], z2), mul2(pt[1], mul2(z2, z))
    return [w for v in (X[0], X[1], Y[0], Y[1], z[0] % P, z[1] % P) for w in int_words(v * R256 % P)]


def batch_add(ps, qs):
    """[p + q] for affine pairs with p.x != q.x, one Fq inversion for the whole list"""
    dx = [sub2(q[0], p[0]) for p, q in zip(ps, qs)]
    norms = [(a * a + b * b) % P for a, b in dx]
    pref, acc = [], 1
    for v in norms:
        pref.append(acc)
        acc = acc * v % P
    inv = pow(acc, P - 2, P)
    out = [None] * len(ps)
    for i in range(len(ps) - 1, -1, -1):
        ni = inv * pref[i] % P
        inv = inv * norms[i] % P
        a, b = dx[i]
        dinv = (a * ni % P, (-b) * ni % P)
        p, q = ps[i], qs[i]
        lam = mul2(sub2(q[1], p[1]), dinv)
        x3 = sub2(sub2(mul2(lam, lam), p[0]), q[0])
        out[i] = (x3, sub2(mul2(lam, sub2(p[0], x3)), p[1]))
    return out


def chain_points(a, d, m, block=512):
    """[(a + i d) * G2 for i < m]: one block of chained additions, then whole blocks by batched additions of (block * d) * G2"""
    dp = mul(G2_GEN, d)
    t = [mul(G2_GEN, a)]
    for _ in range(block - 1):
        t.append(add(t[-1], dp))
    step = mul(G2_GEN, block * d)
    pts, row = list(t), list(t)
    while len(pts) < m:
        row = batch_add(row, [step] * block)
        pts.extend(row)
    return pts[:m]


# ---- Fq2 powers and square roots, the Frobenius endomorphism, the subgroup test, compressed images ----------------------------------
def pow2(a, e):
    r, b = (1, 0), a
    while e:
        if e & 1:
            r = mul2(r, b)
        b = mul2(b, b)
        e >>= 1
    return r


def sqrt2(a):
    """a square root of a in Fq2 (p = 3 mod 4, the two-exponentiation "complex" method), or None when a is not a square"""
    a1 = pow2(a, (P - 3) // 4)
    alpha = mul2(mul2(a1, a1), a)
    x0 = mul2(a1, a)
    if alpha == (P - 1, 0):
        x = mul2((0, 1), x0)
    else:
        x = mul2(pow2(add2((1, 0), alpha), (P - 1) // 2), x0)
    return x if mul2(x, x) == a else None


def is_larger2(y):
    """y > -y in the order of ark-ff 0.4's quadratic extensions: c1 first, then c0, each as a standard-form integer (0 is not larger)"""
    n = neg2(y)
    return (y[1], y[0]) > (n[1], n[0])


XI = (9, 1)
PSI_X = pow2(XI, (P - 1) // 3)
PSI_Y = pow2(XI, (P - 1) // 2)
COFACTOR = 2 * P - R  # of the twist: #E'(Fq2) = r * (2p - r)


def conj2(a):
    return (a[0], (-a[1]) % P)


def psi(pt):
    """the untwist-Frobenius-twist endomorphism: (conj(x) * xi^((p-1)/3), conj(y) * xi^((p-1)/2)); acts on G2 as multiplication by p"""
    if pt is None:
        return None
    return (mul2(conj2(pt[0]), PSI_X), mul2(conj2(pt[1]), PSI_Y))


def in_subgroup(pt):
    """the DEFINING test [r]P = O (pt on the twist)"""
    return mul_raw(pt, R) is None


def compress(pt):
    """64-byte image of ark-serialize 0.4 G2Affine::serialize_compressed: x.c0, x.c1 (32 bytes each, little-endian, standard form);
    byte 63 bit 7 = y is the larger of (y, -y), bit 6 = infinity"""
    if pt is None:
        return bytes(63) + bytes([0x40])
    b = bytearray(pt[0][0].to_bytes(32, "little") + pt[0][1].to_bytes(32, "little"))
    if is_larger2(pt[1]):
        b[63] |= 0x80
    return bytes(b)


def decompress(img):
    """image -> (point or None for infinity); raises ValueError("decode" / "curve") for an invalid image.  No subgroup test."""
    assert len(img) == 64
    larger, inf = img[63] >> 7, (img[63] >> 6) & 1
    if larger and inf:
        raise ValueError("decode")
    x0 = int.from_bytes(img[:32], "little")
    x1 = int.from_bytes(img[32:63] + bytes([img[63] & 0x3F]), "little")
    if x0 >= P or x1 >= P:
        raise ValueError("decode")
    if inf:
        return None
    x = (x0, x1)
    y = sqrt2(add2(mul2(mul2(x, x), x), B_TWIST))
    if y is None:
        raise ValueError("curve")
    if bool(larger) != is_larger2(y):
        y = neg2(y)
    return (x, y)


def glv_lambda_beta():
    """(lambda, beta): the nontrivial cube roots of unity mod r and mod p with lambda * (x, y) = (beta * x, y) on G1 (recomputed, not imported
    from the product; the G1 side is tools/bn254_py.py)"""
    import bn254_py as g1

    def cube_roots(m):
        for w in range(2, 100):
            c = pow(w, (m - 1) // 3, m)
            if c != 1:
                return c, c * c % m
    for l_ in cube_roots(R):
        q = g1.mul(l_, (1, 2))
        for b_ in cube_roots(P):
            if q == (b_, 2):
                return l_, b_
    raise AssertionError("no matching (lambda, beta) pair")
