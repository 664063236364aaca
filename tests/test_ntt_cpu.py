"""The BN254 scalar-field transforms without a GPU: the new C-ABI symbols, the host-only calls (root of unity, plan), the pure-Python yardstick
against the O(n^2) definition, and a CPU run of the kernels' own plan, tables and tile phases (tools/ntt_check.cpp, -DFP_BOUNDS_CHECK) against
the yardstick, word for word."""
import ctypes as C
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from mopro_msm_hip import testhooks as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_fr_ntt_py as ny  # noqa: E402

R = ny.R
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"  # what csrc/Makefile builds the product with
NEW_SYMBOLS = ["msm_bn254_fr_root_of_unity", "msm_bn254_fr_ntt_plan", "msm_bn254_fr_ntt_device", "msm_bn254_fr_ntt",
               "msm_bn254_fr_mul_sub_scale_device"]
ROOT28 = 19103219067921713944291392827692070036145651957329286315305642004821462161904
SMALL_TILE = 4


def test_symbols_are_exported_bound_and_listed():
    lib = mh.load_library()
    hdr = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in mh.ABI_SYMBOLS and re.search(r"\b%s\s*\(" % s, hdr), s
        assert getattr(lib, s).argtypes is not None and getattr(lib, s).restype is C.c_int32, s
    assert re.search(r"#define\s+MSM_HIP_ABI_VERSION\s+7u?\b", hdr) and lib.msm_abi_version() == 7
    assert (mh.NTT_INVERSE, mh.NTT_IN_MONT, mh.NTT_OUT_MONT) == (1, 2, 4)
    for name, val in (("MSM_NTT_INVERSE", 1), ("MSM_NTT_IN_MONT", 2), ("MSM_NTT_OUT_MONT", 4)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, val), hdr), name
    assert "msm_test_ntt_set_tile_log2" in th.HOOK_SYMBOLS and hasattr(th.load_hooks_library(), "msm_test_ntt_set_tile_log2")
    assert not hasattr(lib, "msm_test_ntt_set_tile_log2")
    rust = open(os.path.join(ROOT, "rust", "mopro-msm-hip", "src", "lib.rs")).read()
    hdr_code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NEW_SYMBOLS:  # declared by the shim with as many parameters as the header gives them
        m = re.search(r"\bfn %s\s*\((.*?)\)\s*->\s*i32;" % s, rust, re.S)
        assert m, s
        n_c = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % s, hdr_code, re.S).group(1).split(","))
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_c, s


def test_root_of_unity():
    assert mh.fr_root_of_unity(28) == ROOT28 == ny.root(28)
    with open(os.path.join(ROOT, "tests", "golden", "srs_kzg_points.json")) as f:
        sets = {s["k"]: int(s["omega_hex"], 16) for s in json.load(f)["sets"]}
    assert mh.fr_root_of_unity(3) == sets[3] and mh.fr_root_of_unity(4) == sets[4]
    assert mh.fr_root_of_unity(0) == 1
    with pytest.raises(mh.MsmError) as e:
        mh.fr_root_of_unity(29)
    assert e.value.code == mh.ERR_BAD_ARG
    for k in range(1, 29):
        w = mh.fr_root_of_unity(k)
        assert w == ny.root(k) and pow(w, 1 << (k - 1), R) == R - 1, k


def test_plan():
    for k in range(0, 29):
        radix = mh.ntt_plan(k)
        assert len(radix) >= 1 and sum(radix) == k, (k, radix)
        assert all(0 < t <= 10 for t in radix) or k == 0, (k, radix)
    assert len(mh.ntt_plan(20)) <= 2
    assert mh.ntt_plan(10) == [10] and mh.ntt_plan(11) == [6, 5] and mh.ntt_plan(20) == [10, 10] and mh.ntt_plan(21) == [7, 7, 7]
    with pytest.raises(mh.MsmError) as e:
        mh.ntt_plan(29)
    assert e.value.code == mh.ERR_BAD_ARG


def test_yardstick_is_the_definition():
    rnd = random.Random(11)
    for k in range(0, 7):
        a = [rnd.randrange(R) for _ in range(1 << k)]
        for g in (1, 5, ny.root(k + 1)):
            f = ny.ntt(a, g)
            assert f == ny.ntt_definition(a, g), (k, g)
            assert ny.ntt(a, g, True) == ny.ntt_definition(a, g, True), (k, g)
            assert ny.ntt(f, g, True) == a
    # the identity the Groth16 recipes rest on: A*B - C vanishes on the domain, so it is h * (x^n - 1)
    n = 16
    a, b = [rnd.randrange(R) for _ in range(n)], [rnd.randrange(R) for _ in range(n)]
    c = [x * y % R for x, y in zip(a, b)]
    pa, pb, pc = (ny.ntt(v, 1, True) for v in (a, b, c))
    ea, eb, ec = (ny.ntt(v, 5) for v in (pa, pb, pc))
    zinv = pow(pow(5, n, R) - 1, R - 2, R)
    h = ny.ntt([(x * y - z) * zinv % R for x, y, z in zip(ea, eb, ec)], 5, True)
    assert h[n - 1] == 0
    prod = [0] * (2 * n)
    for i, x in enumerate(pa):
        for j, y in enumerate(pb):
            prod[i + j] = (prod[i + j] + x * y) % R
    for i, z in enumerate(pc):
        prod[i] = (prod[i] - z) % R
    hz = [0] * (2 * n)  # h * (x^n - 1)
    for i, x in enumerate(h):
        hz[i + n] = (hz[i + n] + x) % R
        hz[i] = (hz[i] - x) % R
    assert prod == hz


@pytest.fixture(scope="module")
def ntt_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("ntt_check")
    exe = d / "ntt_check"
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-DFP_BOUNDS_CHECK", "-x", "hip", "--cuda-host-only",  # host code only: no device pass
                    os.path.join(ROOT, "tools", "ntt_check.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=900)

    def run(queries):
        r = subprocess.run([str(exe)], input="\n".join(queries) + "\n", capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = r.stdout.strip().split("\n")
        assert lines[-1] == "%d queries, no bound violated" % len(queries)
        return lines[:-1]

    return d, run


def h64(v):
    return "%064x" % v


def random_words(rnd, n):
    """n elements of 8 words: mostly canonical, some patterns >= r (read modulo r), the all-ones word among them"""
    vals = [rnd.randrange(R) for _ in range(n)]
    for i in range(0, n, 7):
        vals[i] = rnd.randrange(R, 1 << 256)
    vals[rnd.randrange(n)] = (1 << 256) - 1
    return ny.to_words(vals)


def test_cpu_run_of_the_kernel_phases_matches_the_yardstick(ntt_check):
    d, run = ntt_check
    rnd = random.Random(0x4E5454)
    cases = []
    for k in range(0, 13):
        cases.append((k, 1, 0, 10, None))
    for k in (4, 5, 8, 9, 12):
        cases.append((k, 1, 0, SMALL_TILE, None))
    for k, tile in ((6, 10), (11, 10), (9, SMALL_TILE)):  # one pass, two passes, three passes
        for flags in range(8):
            for g in (None, 5, ny.root(k + 1)):
                cases.append((k, 3 if flags in (0, 7) else 1, flags, tile, g))
    cases.append((12, 3, mh.NTT_INVERSE | mh.NTT_IN_MONT, SMALL_TILE, 5))
    queries, expect = [], []
    for i, (k, batch, flags, tile, g) in enumerate(cases):
        words = random_words(rnd, batch << k)
        fin, fout = d / ("in%d.bin" % i), d / ("out%d.bin" % i)
        words.tofile(fin)
        queries.append("N %d %d %d %d %s %s %s" % (k, batch, flags, tile, h64(g) if g is not None else "-", fin, fout))
        expect.append((fout, ny.ntt_words(words, k, batch, flags, g)))
    assert run(queries) == ["N ok"] * len(queries)
    for (fout, want), case in zip(expect, cases):
        got = np.fromfile(fout, np.uint32).reshape(-1, 8)
        assert got.shape == want.shape and (got == want).all(), case


def test_cpu_run_of_mul_sub_scale(ntt_check):
    d, run = ntt_check
    rnd = random.Random(77)
    queries, expect = [], []
    i = 0
    for n in (1, 255):
        for flags in (0, mh.NTT_IN_MONT, mh.NTT_OUT_MONT, mh.NTT_IN_MONT | mh.NTT_OUT_MONT):
            for has_c, k in ((True, rnd.randrange(1, R)), (False, None), (True, None)):
                a, b, c = (random_words(rnd, n) for _ in range(3))
                fa, fb, fc, fo = (d / ("m%d_%s.bin" % (i, x)) for x in "abco")
                a.tofile(fa), b.tofile(fb), c.tofile(fc)
                queries.append("M %d %d %s %s %s %s %s" % (n, flags, h64(k) if k is not None else "-", fa, fb, fc if has_c else "-", fo))
                expect.append((fo, ny.mul_sub_scale_words(a, b, c if has_c else None, k, flags)))
                i += 1
    assert run(queries) == ["M ok"] * len(queries)
    for fo, want in expect:
        assert (np.fromfile(fo, np.uint32).reshape(-1, 8) == want).all()


def test_fr_operation_known_answers(ntt_check):
    _, run = ntt_check
    rnd = random.Random(3)
    special = [0, 1, R - 1, (1 << 256) % R, (1 << 256) - 1, R, R + 1]
    vals = special + [rnd.randrange(1 << 256) for _ in range(8)]
    law = {"mul": lambda a, b: a * b % R, "add": lambda a, b: (a + b) % R, "sub": lambda a, b: (a - b) % R,
           "tomont": lambda a, b: (a << 256) % R, "frommont": lambda a, b: a * ny.MONT_INV % R}
    queries, expect = [], []
    for op, f in law.items():
        for a in vals:
            for b in (special if op in ("mul", "add", "sub") else [0]):
                queries.append("O %s %s %s" % (op, h64(a), h64(b)))
                expect.append("O " + h64(f(a, b)))
    assert run(queries) == expect
    assert run(["P 20 10", "P 12 4", "P 9 4", "P 5 4", "P 0 10"]) == ["P 2 10 10", "P 3 4 4 4", "P 3 3 3 3", "P 2 3 2", "P 1 0"]
