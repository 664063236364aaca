#!/usr/bin/env python3
"""Emit tests/golden/g2_compressed_points.json: compressed BN254 G2 images (ark-serialize 0.4 G2Affine::serialize_compressed) with what they must
decode to, and invalid images with the reason each must be refused for.  Data only; seeded; everything comes from the independent Python law
(tools/bn254_g2_py.py), nothing from the product.

valid:   the generator, k * G2 for a few k (r - 1 among them: both signs of y), the points of tests/golden/zkey_g2_points.json (its infinite ones too)
invalid: both flag bits set, c0 >= p, c1 >= p (a value between p and 2^254: the top two bits are flags), an x with x^3 + b not a square  -> "decode" / "curve"
         a random twist point, points of order 10069 and 5864401, a G2 point plus a point of order 10069                            -> "subgroup"
The small-order points are T = [r (2p - r) / f] Q for a random twist point Q: f = 10069, 5864401 divide the cofactor 2p - r.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bn254_g2_py as g2  # noqa: E402

P, R, G = g2.P, g2.R, g2.G2_GEN
GOLDEN = os.path.join(HERE, "..", "tests", "golden")
SEED = 0xB2546202
rnd = random.Random(SEED)


def mont_hex(pt):
    return b"".join(int(w).to_bytes(4, "little") for w in g2.point_words(pt, mont=True)).hex()


def rand_twist_point():
    while True:
        x = (rnd.randrange(P), rnd.randrange(P))
        y = g2.sqrt2(g2.add2(g2.mul2(g2.mul2(x, x), x), g2.B_TWIST))
        if y is not None:
            return (x, y if rnd.random() < 0.5 else g2.neg2(y))


def point_of_order(f):
    assert g2.COFACTOR % f == 0
    while True:
        t = g2.mul_raw(rand_twist_point(), R * (g2.COFACTOR // f))
        if t is not None:
            assert g2.mul_raw(t, f) is None
            return t


valid, invalid = [], []


def add_valid(name, pt):
    assert pt is None or (g2.on_curve(pt) and g2.in_subgroup(pt))
    img = g2.compress(pt)
    assert g2.decompress(img) == pt
    valid.append({"name": name, "image_hex": img.hex(), "infinity": pt is None, "larger_y": bool(img[63] >> 7), "mont_le_hex": mont_hex(pt)})


def add_invalid(name, img, reason, pt=None):
    """pt: what the image decodes to when only the subgroup check refuses it"""
    assert len(img) == 64
    if reason == "subgroup":
        assert g2.decompress(img) == pt and g2.on_curve(pt) and not g2.in_subgroup(pt)
    else:
        try:
            g2.decompress(img)
            raise AssertionError(name)
        except ValueError as e:
            assert str(e) == reason, (name, str(e))
    invalid.append({"name": name, "image_hex": img.hex(), "reason": reason, "mont_le_hex": mont_hex(pt) if pt is not None else None})


add_valid("generator", G)
for k in (2, 3, 0x1234567, 0xFEDCBA9876543210FEDCBA9876543210, R - 2, R - 1):
    add_valid("k_%x" % k, g2.mul(G, k))
for _ in range(4):
    add_valid("random_multiple", g2.mul(G, rnd.randrange(1, R)))
with open(os.path.join(GOLDEN, "zkey_g2_points.json")) as f:
    zk = json.load(f)["points"]
ri = pow(g2.R256, -1, P)
for i, p_ in enumerate(zk):
    if p_["infinity"]:
        add_valid("zkey_%s_%d_infinity" % (p_["section"], i), None)
    else:
        raw = bytes.fromhex(p_["mont_le_hex"])
        c = [int.from_bytes(raw[32 * j:32 * j + 32], "little") * ri % P for j in range(4)]
        add_valid("zkey_%s_%d" % (p_["section"], i), ((c[0], c[1]), (c[2], c[3])))
assert {v["larger_y"] for v in valid if not v["infinity"]} == {True, False}

good = bytearray(g2.compress(g2.mul(G, 77)))
both = bytearray(good)
both[63] |= 0xC0
add_invalid("both_flags", bytes(both), "decode")
add_invalid("both_flags_zero_x", bytes(63) + bytes([0xC0]), "decode")
add_invalid("c0_ge_p", (P + 5).to_bytes(32, "little") + bytes(good[32:]), "decode")
add_invalid("c0_eq_p", P.to_bytes(32, "little") + bytes(good[32:]), "decode")
c1 = P + 7
assert P <= c1 < 1 << 254
add_invalid("c1_ge_p", bytes(good[:32]) + c1.to_bytes(32, "little"), "decode")
add_invalid("c1_ge_p_flagged_larger", bytes(good[:32]) + (c1 | 1 << 255).to_bytes(32, "little"), "decode")
while True:
    x = (rnd.randrange(P), rnd.randrange(P))
    if g2.sqrt2(g2.add2(g2.mul2(g2.mul2(x, x), x), g2.B_TWIST)) is None:
        break
add_invalid("non_residue_x", x[0].to_bytes(32, "little") + x[1].to_bytes(32, "little"), "curve")
q = rand_twist_point()
add_invalid("random_twist_point", g2.compress(q), "subgroup", q)
t1, t2 = point_of_order(10069), point_of_order(5864401)
add_invalid("order_10069", g2.compress(t1), "subgroup", t1)
add_invalid("order_5864401", g2.compress(t2), "subgroup", t2)
s = g2.add(g2.mul(G, rnd.randrange(1, R)), t1)
add_invalid("g2_plus_order_10069", g2.compress(s), "subgroup", s)

out = {"seed": "0x%x" % SEED,
       "format": "image: 64 bytes x.c0 | x.c1 little-endian standard form, byte 63 bit 7 = y larger than -y (c1 first, then c0), bit 6 = infinity; "
                 "mont_le_hex: x.c0 x.c1 y.c0 y.c1 as R = 2^256 Montgomery words, little-endian (all zero for infinity)",
       "valid": valid, "invalid": invalid}
with open(os.path.join(GOLDEN, "g2_compressed_points.json"), "w") as f:
    json.dump(out, f, indent=1)
print("%d valid, %d invalid images" % (len(valid), len(invalid)))
