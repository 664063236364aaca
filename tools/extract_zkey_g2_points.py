#!/usr/bin/env python3
"""Extract the BN254 G2 points of the reference's Groth16 proving key into tests/golden/zkey_g2_points.json.

Source (present only in the build container; this script never runs on the GPU box):
  /root/reference/example-app/test-vectors/circom/multiplier2_final.zkey
Section 2 (Groth16 header) holds beta2, gamma2 and delta2; section 7 the B2 query (one G2 point per witness variable).  A G2 point is
4 x 32 bytes of little-endian R = 2^256 Montgomery words in the order x.c0, x.c1, y.c0, y.c1 -- what include/msm_hip.h calls MSM_FORM_MONT
for msm_bn254_g2 -- and all-zero bytes are the point at infinity.  The fixture keeps the bytes as they are (hex); this script CHECKS with
Python integers (tools/bn254_g2_py.py) that every finite point lies on y^2 = x^3 + 3/(9+u) and has order r.  Data only.
"""
import json
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn254_g2_py as g2  # noqa: E402

SRC = "/root/reference/example-app/test-vectors/circom/multiplier2_final.zkey"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "zkey_g2_points.json")


def decode(b):
    """128 bytes -> affine point (standard form) or None"""
    if not any(b):
        return None
    w = [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(4)]
    assert all(v < g2.P for v in w), "word not canonical"
    ri = pow(g2.R256, -1, g2.P)
    x0, x1, y0, y1 = (v * ri % g2.P for v in w)
    return ((x0, x1), (y0, y1))


def main():
    raw = open(SRC, "rb").read()
    assert raw[:4] == b"zkey"
    _, nsec = struct.unpack_from("<II", raw, 4)
    pos, sections = 12, {}
    for _ in range(nsec):
        typ, size = struct.unpack_from("<IQ", raw, pos)
        sections[typ] = raw[pos + 12:pos + 12 + size]
        pos += 12 + size
    h = sections[2]
    n8q = struct.unpack_from("<I", h, 0)[0]
    assert n8q == 32 and int.from_bytes(h[4:36], "little") == g2.P
    o = 4 + n8q
    n8r = struct.unpack_from("<I", h, o)[0]
    o += 4 + n8r + 12  # r, then n_vars, n_public, domain size
    g1b, g2b = 64, 128
    hdr = {"beta2": o + 2 * g1b, "gamma2": o + 2 * g1b + g2b, "delta2": o + 3 * g1b + 2 * g2b}  # alpha1 beta1 beta2 gamma2 delta1 delta2
    assert len(h) == o + 3 * g1b + 3 * g2b
    points = []

    def take(b, section, index):
        assert len(b) == g2b
        pt = decode(b)
        if pt is not None:
            assert g2.on_curve(pt), (section, index, "not on the twist")
            assert g2.mul_raw(pt, g2.R) is None, (section, index, "not of order r")
        points.append({"section": section, "index": index, "infinity": pt is None, "mont_le_hex": b.hex()})

    for name, off in hdr.items():
        take(h[off:off + g2b], name, 0)
    b2 = sections[7]
    assert len(b2) % g2b == 0
    for i in range(len(b2) // g2b):
        take(b2[i * g2b:(i + 1) * g2b], "B2", i)
    with open(OUT, "w") as f:
        json.dump({"source": "multiplier2_final.zkey (reference example-app test vector)", "encoding": "x.c0 x.c1 y.c0 y.c1, 32-byte little-endian "
                   "R = 2^256 Montgomery words each; all zero = infinity", "points": points}, f, indent=1)
    print(f"{len(points)} points ({sum(p['infinity'] for p in points)} at infinity) -> {OUT}")


if __name__ == "__main__":
    main()
