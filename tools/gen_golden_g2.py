#!/usr/bin/env python3
"""Generate the G2 MSM golden vectors tests/golden/msm_g2_*.npz and their index tests/golden/g2_index.json (tests/golden/index.json, the G1
set, is not touched).  Expected values come from tools/bn254_g2_py.py (pure Python integers, independent of the product).

Bases are P_i = k_i * G2 for seeded k_i, so that the expected sum is (sum s_i k_i mod r) * G2: one scalar multiplication per vector.  Each file
holds bases (n x 32 standard-form words), bases_mont (the same in R = 2^256 Montgomery words), inf (n bytes), scalars (n x 8 words, standard
form), expected (32 affine standard-form words, zero for the identity) and expected_inf.
"""
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn254_g2_py as g2  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
R = g2.R


def build(name, logs, scalars, inf=None):
    n = len(logs)
    inf = inf or [0] * n
    pts = [None if inf[i] else g2.mul(g2.G2_GEN, logs[i]) for i in range(n)]
    total = sum(s * k for s, k, f in zip(scalars, logs, inf) if not f) % R
    exp = g2.mul(g2.G2_GEN, total)
    np.savez(os.path.join(OUT, f"msm_g2_{name}.npz"),
             bases=np.array([g2.point_words(p_) for p_ in pts], np.uint32).reshape(n, 32),
             bases_mont=np.array([g2.point_words(p_, True) for p_ in pts], np.uint32).reshape(n, 32),
             inf=np.array(inf, np.uint8),
             scalars=np.array([g2.int_words(s) for s in scalars], np.uint32).reshape(n, 8),
             expected=np.array(g2.affine_words_std(exp), np.uint32), expected_inf=np.uint8(exp is None))
    return {"name": name, "file": f"msm_g2_{name}.npz", "n": n, "expected_inf": exp is None}


def main():
    rnd = random.Random(0xB2542002)
    entries = []
    for n in (1, 2, 3, 17, 256, 1024):
        entries.append(build(f"rand_n{n}", [rnd.randrange(1, R) for _ in range(n)], [rnd.randrange(R) for _ in range(n)]))
    k = [rnd.randrange(1, R) for _ in range(16)]
    entries.append(build("edge_inf_bases", k, [rnd.randrange(R) for _ in k], [1 if i % 3 == 0 else 0 for i in range(16)]))
    entries.append(build("edge_zero_scalars", k, [0 if i % 2 else rnd.randrange(R) for i in range(16)]))
    entries.append(build("edge_all_zero_scalars", k[:8], [0] * 8))
    entries.append(build("edge_p_minus_p", [k[0], R - k[0], k[1], R - k[1]], [5, 5, 7, 7]))  # sums to the identity
    entries.append(build("edge_same_base_same_scalar", [k[2]] * 12, [k[3]] * 12))
    entries.append(build("edge_scalar_r_minus_1", k[:6], [R - 1] * 6))
    carry = [(1 << b) - 1 for b in (16, 32, 64, 127, 128, 200, 253)] + [(1 << 253) + (1 << 200), 1 << 126, (1 << 127) + 1]
    entries.append(build("edge_carry_patterns", k[:len(carry)], carry))
    with open(os.path.join(OUT, "g2_index.json"), "w") as f:
        json.dump({"generator": "tools/gen_golden_g2.py", "vectors": entries}, f, indent=1)
    print(f"{len(entries)} vectors -> {OUT}")


if __name__ == "__main__":
    main()
