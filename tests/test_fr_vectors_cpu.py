"""The scalar vectors of a setup without a GPU: the new C-ABI symbols and the host-only plan, the Python yardstick (tools/bn254_fr_vectors_py.py)
against the definitions it stands for, and a CPU run of the kernels' own per-lane routines -- power walk, chain inversion, Lagrange chain, linear
combination (tools/fr_vectors_check.cpp, -DFP_BOUNDS_CHECK) -- against that yardstick, word for word; once more as a stand-alone program under
AddressSanitizer / UBSan, where the arrays are exactly n elements long."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_fr_vectors_py as frv  # noqa: E402

R = frv.R
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"  # what csrc/Makefile builds the product with
NEW_SYMBOLS = ["msm_bn254_fr_vector_plan", "msm_bn254_fr_powers_device", "msm_bn254_fr_batch_inverse_device", "msm_bn254_fr_batch_inverse",
               "msm_bn254_fr_lagrange_device", "msm_bn254_fr_lincomb_device"]
IM, OM = mh.NTT_IN_MONT, mh.NTT_OUT_MONT
FLAG_SETS = (0, IM, OM, IM | OM)


def test_symbols_are_exported_bound_and_listed():
    lib = mh.load_library()
    hdr = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in mh.ABI_SYMBOLS and re.search(r"\b%s\s*\(" % s, hdr), s
        assert getattr(lib, s).argtypes is not None and getattr(lib, s).restype is C.c_int32, s
    assert re.search(r"#define\s+MSM_HIP_ABI_VERSION\s+7u?\b", hdr) and lib.msm_abi_version() == 7
    rust = open(os.path.join(ROOT, "rust", "mopro-msm-hip", "src", "lib.rs")).read()
    hdr_code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NEW_SYMBOLS:  # declared by the shim with as many parameters as the header gives them
        m = re.search(r"\bfn %s\s*\((.*?)\)\s*->\s*i32;" % s, rust, re.S)
        assert m, s
        n_c = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % s, hdr_code, re.S).group(1).split(","))
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_c == len(getattr(lib, s).argtypes), s
    for name in ("fr_powers_device", "fr_batch_inverse_device", "fr_batch_inverse", "fr_lagrange_device", "fr_lincomb_device", "fr_vector_plan"):
        assert callable(getattr(mh.MsmContext, name)), name


def test_plan():
    p = mh.fr_vector_plan()
    assert p["inv_group"] >= 2 and p["block_points"] == 256 * p["inv_group"] and p["powers_block_points"] > 0
    assert C.sizeof(mh.FrVectorPlan) == 16
    assert mh.load_library().msm_bn254_fr_vector_plan(None) == mh.ERR_BAD_ARG
    assert mh.fr_vector_plan() == p  # (the failed call left nothing behind)


def test_sizeof_the_plan_in_c(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include "msm_hip.h"\n_Static_assert(sizeof(msm_fr_vector_plan_t) == 16, "16 bytes");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")],
                   check=True, capture_output=True)


def test_transpose_r1cs_coefs():
    coefs = [(0, 1, 5, 7), (2, 3, 0, R - 1), (1, 0, 2, 1 << 255)]
    t = mh.transpose_r1cs_coefs(coefs)
    a = mh.r1cs_coefs(coefs)
    assert t.dtype == mh.R1CS_COEF_DTYPE and list(t["row"]) == [5, 0, 2] and list(t["col"]) == [1, 3, 0]
    assert (t["matrix"] == a["matrix"]).all() and (t["value"] == a["value"]).all()
    assert list(a["row"]) == [1, 3, 0]  # (the argument is left alone)
    assert (mh.transpose_r1cs_coefs(t) == a).all()


# ---- the yardstick against the definitions --------------------------------------------------------------------------------------------------
def test_the_yardstick_inverse():
    for x in frv.patterns(21, 40) + [1, R - 1, R + 1, (1 << 256) - 1]:
        assert frv.inverse(x) * x % R == 1
    assert [frv.inverse(z) for z in (0, R, 2 * R, 5 * R)] == [0, 0, 0, 0]
    assert frv.batch_inverse([3, 0, 5]) == [frv.inverse(3), 0, frv.inverse(5)]


def test_the_yardstick_powers_and_lincomb():
    assert frv.powers(3, 5) == [1, 3, 9, 27, 81] and frv.powers(3, 3, scale=2, first=2) == [18, 54, 162]
    assert frv.powers(0, 3) == [1, 0, 0] and frv.powers(0, 3, scale=7) == [7, 0, 0] and frv.powers(0, 2, first=1) == [0, 0]
    assert frv.powers(R - 1, 4, first=(1 << 40) + 3) == [R - 1, 1, R - 1, 1]
    assert frv.lincomb([1, 2], 3) == [3, 6] and frv.lincomb([1, 2], 3, [1, 1], R - 1) == [2, 5]
    assert frv.lincomb([1, 2], 1, None, 1, [5, 5], 2) == [11, 12]


@pytest.mark.parametrize("log_n", range(7))
def test_the_yardstick_lagrange(log_n):
    rng = random.Random(0x1A64 + log_n)
    n, w = 1 << log_n, frv.root_of_unity(log_n)
    assert pow(w, n, R) == 1 and (n == 1 or pow(w, n // 2, R) == R - 1)
    assert w == mh.fr_root_of_unity(log_n)  # the root the transforms use
    dom = [pow(w, i, R) for i in range(n)]
    for tau in (rng.randrange(R), rng.randrange(R), 0):
        L = frv.lagrange(tau, log_n)
        assert sum(L) % R == 1
        p = [rng.randrange(R) for _ in range(n)]  # a polynomial of degree < n by its coefficients
        ev = lambda x: sum(c * pow(x, j, R) for j, c in enumerate(p)) % R
        assert sum(l * ev(x) for l, x in zip(L, dom)) % R == ev(tau)
    for k in sorted({0, 1 % n, n // 2, n - 1}):
        assert frv.lagrange(dom[k], log_n) == [int(i == k) for i in range(n)]


# ---- the kernels' routines on the CPU against the yardstick -------------------------------------------------------------------------------------
def build_check(d, sanitize):
    exe = d / ("fr_vectors_check_asan" if sanitize else "fr_vectors_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([HIPCC, *flags, "-std=c++17", "-DFP_BOUNDS_CHECK", "-x", "hip", "--cuda-host-only",  # host code only: no device pass
                    os.path.join(ROOT, "tools", "fr_vectors_check.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=900)

    def run(queries):
        (d / "queries.txt").write_text("\n".join(queries) + "\n")
        r = subprocess.run([str(exe), str(d / "queries.txt")], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = r.stdout.strip().split("\n")
        assert lines[-1] == "%d queries, no bound violated" % len(queries)
        return [[int(v, 16) for v in ln.split()[1:]] for ln in lines[:-1]]

    return run


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("fr_vectors_check"), False)


@pytest.fixture(scope="module")
def check_asan(tmp_path_factory):
    """the same program as a stand-alone host binary under AddressSanitizer and UBSan"""
    return build_check(tmp_path_factory.mktemp("fr_vectors_check_asan"), True)


def hexes(vs):
    return " ".join("%x" % v for v in vs)


def want_words(values, flags):
    return frv.from_words(frv.write(values, bool(flags & OM)))


def ask(run, queries_and_wants):
    got = run([q for q, _ in queries_and_wants])
    assert len(got) == len(queries_and_wants)
    for (q, want), g in zip(queries_and_wants, got):
        assert g == want, q[:60]


def inverse_cases():
    p = mh.fr_vector_plan()
    G, B = p["inv_group"], p["block_points"]
    pool = [x if x % R else 1 for x in frv.patterns(31, B + 1)]
    cases = []

    def add(xs, flags=0, inplace=0, g=G):
        cases.append(("I %d %d %d %s" % (g, flags, inplace, hexes(xs)), want_words(frv.batch_inverse(frv.read(xs, bool(flags & IM))), flags)))

    for n in sorted({1, 2, 63, 64, 65, 64 * G - 1, 64 * G, 64 * G + 1, B - 1, B + 1}):
        add(pool[:n], inplace=n & 1)
    n = 64 * G + 70
    chain = [3 + 64 * s for s in range(G)]  # the chain of lane 3
    for at in [[chain[0]], [chain[-1]], chain, list(range(n))] + [[i] for i in chain[1:-1]]:
        xs = list(pool[:n])
        for t, i in enumerate(at):
            xs[i] = (0, R, 2 * R, 5 * R)[t % 4]
        add(xs)
    special = [0, R, 2 * R, 5 * R, (1 << 256) - 1, R - 1, 1, R + 1] + pool[:62]
    for flags in FLAG_SETS:
        for inplace in (0, 1):
            add(special, flags, inplace)
    for g in (4, 8, 16, 32):  # every chain length the sweep runs
        add(special + pool[:64 * g - 5], IM, 0, g)
    return cases


def powers_cases():
    B = mh.fr_vector_plan()["powers_block_points"]
    scale, tau = frv.patterns(32, 2)
    cases = []
    for flags in (0, OM):
        for first in (0, 1, (1 << 40) + 3):
            for base in (0, 1, R - 1, tau):
                for s in (None, scale):
                    n = 67 if base != tau else 1024 + 65
                    cases.append(("P %d %d %d %x %s" % (flags, first, n, base, "-" if s is None else "%x" % s),
                                  want_words(frv.powers(base, n, 1 if s is None else s, first), flags)))
    for n in (1, 63, 64, 65, 1023, 1024, 1025, B - 1, B + 1):
        cases.append(("P 0 5 %d %x %x" % (n, tau, scale), want_words(frv.powers(tau, n, scale, 5), 0)))
    return cases


def lagrange_cases():
    p = mh.fr_vector_plan()
    G = p["inv_group"]
    big = p["block_points"].bit_length()  # the first power of two above block_points
    assert 1 << big > p["block_points"] >= 1 << (big - 1)
    tau = frv.patterns(33, 1)[0]
    cases = []
    for log_n in (0, 1, 2, 7, big):
        w = frv.root_of_unity(log_n)
        inside = [1, w, pow(w, (1 << log_n) - 1, R), pow(w, (1 << log_n) // 2 + 1, R) + R]  # (the last one spelled above r)
        for flags in (0, OM):
            for t in [tau, 0] + inside[:4 if flags == 0 else 2]:
                cases.append(("L %d %d %d %x" % (G, flags, log_n, t), want_words(frv.lagrange(t, log_n), flags)))
    cases.append(("L %d 0 9 %x" % (12 - G, tau), want_words(frv.lagrange(tau, 9), 0)))  # the other chain length the check program has
    return cases


def lincomb_cases():
    n = 70
    a, b, c = (frv.patterns(34 + j, n) for j in range(3))
    a[:6] = [0, R, (1 << 256) - 1, R - 1, 5 * R, 1]
    b[:3] = c[:3] = [(1 << 256) - 1] * 3  # the largest words in all three terms at once
    ka, kb, kc = frv.patterns(37, 2) + [(1 << 256) - 1]
    cases = []
    for flags in FLAG_SETS:
        m = bool(flags & IM)
        ra, rb, rc = frv.read(a, m), frv.read(b, m), frv.read(c, m)
        for present in range(4):
            for ks in ((ka, kb, kc), (None, None, None), (ka, None, kc)):
                if flags and ks[0] is None:
                    continue
                k1 = [1 if k is None else k for k in ks]
                want = frv.lincomb(ra, k1[0], rb if present & 1 else None, k1[1], rc if present & 2 else None, k1[2])
                arrays = a + (b if present & 1 else []) + (c if present & 2 else [])
                for alias in (0, 1, 2, 3):
                    if alias >= 2 and not present >> (alias - 2) & 1:
                        continue
                    if alias and (flags not in (0, IM | OM) or ks[0] is None):
                        continue
                    cases.append(("C %d %d %d %d %s %s" % (flags, n, alias, present, " ".join("-" if k is None else "%x" % k for k in ks), hexes(arrays)),
                                  want_words(want, flags)))
    return cases


@pytest.fixture(scope="module")
def cases():
    return {"inverse": inverse_cases(), "powers": powers_cases(), "lagrange": lagrange_cases(), "lincomb": lincomb_cases()}


@pytest.mark.parametrize("what", ["inverse", "powers", "lagrange", "lincomb"])
def test_the_routines_match_the_yardstick(check, cases, what):
    ask(check, cases[what])


def test_the_same_cases_under_the_sanitizers(check_asan, cases):
    for what in ("inverse", "powers", "lagrange", "lincomb"):
        ask(check_asan, cases[what])


def test_zero_is_written_as_zero_and_neighbours_are_exact(check):
    G = mh.fr_vector_plan()["inv_group"]
    xs = [x if x % R else 1 for x in frv.patterns(38, 64 * G)]
    xs[64 * (G - 1) + 5] = 2 * R
    (got,) = check(["I %d 0 0 %s" % (G, hexes(xs))])
    assert got[64 * (G - 1) + 5] == 0 and all(g * x % R == 1 for i, (g, x) in enumerate(zip(got, xs)) if i != 64 * (G - 1) + 5)
    assert all(g < R for g in got)
