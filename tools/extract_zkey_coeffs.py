#!/usr/bin/env python3
"""Extract the constraint-matrix coefficients the reference holds as DATA into tests/golden/zkey_r1cs_coeffs.json.

Source (present only in the build container; this script never runs on the GPU box):
  /root/reference/example-app/test-vectors/circom/multiplier2_final.zkey   (snarkjs Groth16 proving key, see tools/extract_zkey_points.py)
Section 4 of the container holds a count and then one record per non-zero coefficient of the A and B matrices: matrix u32, constraint u32,
signal u32, 32 little-endian bytes = coefficient * 2^512 mod r -- the layout of msm_r1cs_coef_t with MSM_R1CS_COEF_MONT2 (include/msm_hip.h).  The
fixture keeps the header fields and the records as they are (the value as hex of its 32 bytes), and this script CHECKS, with Python integers, that
the header's r is the BN254 scalar-field modulus and what every value stands for.  Data only: no text of the reference travels.
"""
import json
import os
import struct

SRC = "/root/reference/example-app/test-vectors/circom/multiplier2_final.zkey"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "zkey_r1cs_coeffs.json")
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def main():
    raw = open(SRC, "rb").read()
    assert raw[:4] == b"zkey"
    _version, nsec = struct.unpack_from("<II", raw, 4)
    pos, sections = 12, {}
    for _ in range(nsec):
        typ, size = struct.unpack_from("<IQ", raw, pos)
        sections[typ] = raw[pos + 12:pos + 12 + size]
        pos += 12 + size
    assert pos == len(raw) and struct.unpack_from("<I", sections[1], 0)[0] == 1, "not a Groth16 key"
    h = sections[2]
    n8q = struct.unpack_from("<I", h, 0)[0]
    o = 4 + n8q
    n8r = struct.unpack_from("<I", h, o)[0]
    r = int.from_bytes(h[o + 4:o + 4 + n8r], "little")
    o += 4 + n8r
    n_vars, n_public, domain = struct.unpack_from("<III", h, o)
    assert n8r == 32 and r == R, "header modulus is not the BN254 scalar field"
    sec = sections[4]
    n = struct.unpack_from("<I", sec, 0)[0]
    assert len(sec) == 4 + 44 * n
    inv = pow(1 << 512, -1, R)
    coefs = []
    for i in range(n):
        m, row, col = struct.unpack_from("<III", sec, 4 + 44 * i)
        v = sec[4 + 44 * i + 12:4 + 44 * i + 44]
        c = int.from_bytes(v, "little") * inv % R
        assert m < 2 and row < domain and col < n_vars and c in (1, R - 1)
        coefs.append({"matrix": m, "row": row, "col": col, "value_le_hex": v.hex(), "coefficient": 1 if c == 1 else -1})
    out = {
        "_source": "example-app/test-vectors/circom/multiplier2_final.zkey of the reference: Groth16 header fields and section 4 (coefficients)",
        "_format": "value_le_hex = the 32 bytes as stored: little-endian, coefficient * 2^512 mod r (MSM_R1CS_COEF_MONT2); coefficient = what it stands for",
        "r_hex": hex(r), "n_vars": n_vars, "n_public": n_public, "domain_size": domain, "coefs": coefs,
    }
    json.dump(out, open(OUT, "w"), indent=1)
    print(f"{n} coefficients, {n_vars} variables, domain {domain} -> {os.path.normpath(OUT)}")


if __name__ == "__main__":
    main()
