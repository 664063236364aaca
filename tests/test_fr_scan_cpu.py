"""The scalar-field scans without a GPU: the new C-ABI symbols and the host-only plan, the Python yardstick (tools/bn254_fr_scan_py.py) against the
definitions it stands for, and a CPU run of the kernels' own routines -- the chains, the combine steps over the lanes of a workgroup and over the
workgroups, the three launches (tools/fr_scan_check.cpp, -DFP_BOUNDS_CHECK) -- against that yardstick, word for word, for both chain lengths the
kernels are instantiated for; once more as a stand-alone program under AddressSanitizer / UBSan, where the arrays are exactly n elements long."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import pytest

import mopro_msm_hip as mh
from mopro_msm_hip import testhooks as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_fr_scan_py as fs  # noqa: E402

R = fs.R
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"  # what csrc/Makefile builds the product with
NEW_SYMBOLS = ["msm_bn254_fr_scan_plan", "msm_bn254_fr_poly_eval_device", "msm_bn254_fr_poly_div_linear_device", "msm_bn254_fr_poly_div_linear",
               "msm_bn254_fr_running_product_device"]
HOOK = "msm_test_fr_scan_set_chain"
IM, OM, EX = mh.NTT_IN_MONT, mh.NTT_OUT_MONT, 32
FLAG_SETS = (0, IM, OM, IM | OM)


# ---- the interface ----------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_bound_and_listed():
    lib = mh.load_library()
    hdr = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in mh.ABI_SYMBOLS and re.search(r"\b%s\s*\(" % s, hdr), s
        assert getattr(lib, s).argtypes is not None and getattr(lib, s).restype is C.c_int32, s
    assert re.search(r"#define\s+MSM_HIP_ABI_VERSION\s+7u?\b", hdr) and lib.msm_abi_version() == 7
    assert mh.FR_SCAN_EXCLUSIVE == EX and re.search(r"#define\s+MSM_FR_SCAN_EXCLUSIVE\s+32u\b", hdr)
    assert EX & (mh.NTT_INVERSE | IM | OM | mh.FB_OUT_STD | mh.PM_BASES_STD) == 0  # a bit none of the flags this family honours uses
    rust = open(os.path.join(ROOT, "rust", "mopro-msm-hip", "src", "lib.rs")).read()
    hdr_code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NEW_SYMBOLS:  # declared by the shim with as many parameters as the header gives them
        m = re.search(r"\bfn %s\s*\((.*?)\)\s*->\s*i32;" % s, rust, re.S)
        assert m, s
        n_c = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % s, hdr_code, re.S).group(1).split(","))
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_c == len(getattr(lib, s).argtypes), s
    for name in ("fr_poly_eval_device", "fr_poly_div_linear_device", "fr_poly_div_linear", "fr_running_product_device", "fr_scan_plan"):
        assert callable(getattr(mh.MsmContext, name)), name


def test_the_setter_is_a_hook_only():
    hooks_hdr = open(os.path.join(ROOT, "include", "msm_hip_testhooks.h")).read()
    assert HOOK in th.HOOK_SYMBOLS and hasattr(th.load_hooks_library(), HOOK) and re.search(r"\b%s\s*\(" % HOOK, hooks_hdr)
    assert not hasattr(mh.load_library(), HOOK)
    assert HOOK not in open(os.path.join(ROOT, "include", "msm_hip.h")).read()


def test_plan():
    lib = mh.load_library()
    p = mh.fr_scan_plan(1)
    G, B = p["chain"], p["block_points"]
    assert G >= 1 and B == 256 * G and p["eval_launches"] == 2 and p["div_launches"] == 3
    assert p["blocks"] == 1 and p["scratch_bytes"] == 36
    for n in (B, B + 1, 256 * B, 256 * B + 1, 1 << 20, 1 << 28, 1 << 36):
        q = mh.fr_scan_plan(n)
        assert q["blocks"] == -(-n // B) and q["scratch_bytes"] == 36 * q["blocks"] and (q["chain"], q["block_points"]) == (G, B)
    assert C.sizeof(mh.FrScanPlan) == 32
    out = mh.FrScanPlan()
    assert lib.msm_bn254_fr_scan_plan(5, None) == mh.ERR_BAD_ARG
    assert lib.msm_bn254_fr_scan_plan(0, C.byref(out)) == mh.ERR_EMPTY
    assert lib.msm_bn254_fr_scan_plan((1 << 36) + 1, C.byref(out)) == mh.ERR_BAD_ARG
    assert mh.fr_scan_plan(1) == p  # (the failed calls left nothing behind)


def test_sizeof_the_plan_in_c(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include "msm_hip.h"\n_Static_assert(sizeof(msm_fr_scan_plan_t) == 32, "32 bytes");\n'
                   '_Static_assert(MSM_FR_SCAN_EXCLUSIVE == 32u, "the flag");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")],
                   check=True, capture_output=True)


# ---- the yardstick against the definitions --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 7, 40])
def test_the_yardstick_division(n):
    rng = random.Random(0x5CA0 + n)
    for z in fs.points(n) + [rng.randrange(R)]:
        zr = z % R
        for c in ([rng.randrange(R) for _ in range(n)], [R - 1] * n, [0] * (n - 1) + [1]):
            q, rem = fs.poly_div_linear(c, z)
            assert len(q) == n and q[n - 1] == 0
            for j in range(n):  # the O(n^2) sums
                assert q[j] == sum(c[i] * pow(zr, i - j - 1, R) for i in range(j + 1, n)) % R
            assert rem == sum(c[i] * pow(zr, i, R) for i in range(n)) % R == fs.poly_eval(c, zr)
            back = fs.mul_linear(q[:n - 1], z)  # q (X - z) + rem == p, coefficient by coefficient
            back[0] = (back[0] + rem) % R
            assert back == c
    s = [rng.randrange(R) for _ in range(n)]
    q, rem = fs.poly_div_linear(fs.mul_linear(s, 12345), 12345)
    assert rem == 0 and q == s + [0]
    assert fs.poly_div_linear([5, 6, 7], 0) == ([6, 7, 0], 5)  # z = 0: the shift


def test_the_yardstick_running_product():
    rng = random.Random(0x5CA1)
    for n in (1, 2, 9, 40):
        x = [rng.randrange(R) for _ in range(n)]
        inc, total = fs.running_product(x)
        exc, total2 = fs.running_product(x, True)
        run, want = 1, []
        for v in x:
            run = run * v % R
            want.append(run)
        assert inc == want and exc == [1] + want[:-1] and total == total2 == want[-1]
    assert fs.running_product([3, 0, 5]) == ([3, 0, 0], 0) and fs.running_product([3, 0, 5], True) == ([1, 3, 0], 0)
    assert fs.read([fs.MONT_R * 7 % R], True) == [7] and fs.encode([7], True) == [fs.MONT_R * 7 % R]


# ---- the kernels' routines on the CPU against the yardstick -------------------------------------------------------------------------------------
def build_check(d, sanitize):
    exe = d / ("fr_scan_check_asan" if sanitize else "fr_scan_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([HIPCC, *flags, "-std=c++17", "-DFP_BOUNDS_CHECK", "-x", "hip", "--cuda-host-only",  # host code only: no device pass
                    os.path.join(ROOT, "tools", "fr_scan_check.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=900)

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
    return build_check(tmp_path_factory.mktemp("fr_scan_check"), False)


@pytest.fixture(scope="module")
def check_asan(tmp_path_factory):
    """the same program as a stand-alone host binary under AddressSanitizer and UBSan"""
    return build_check(tmp_path_factory.mktemp("fr_scan_check_asan"), True)


def hexes(vs):
    return " ".join("%x" % v for v in vs)


def sizes(G):
    B = 256 * G
    return sorted({n for n in (1, 2, G - 1, G, G + 1, 64 * G - 1, 64 * G, 64 * G + 1, B - 1, B, B + 1, 2 * B + 1, 3 * B - 1) if n >= 1})


def zero_places(G):
    """the first, middle and last place of a chain, of a wavefront's range and of a block, all in the SECOND block of an array of 2 B + 1"""
    B = 256 * G
    chain, wave = B + 5 * G, B + 64 * G
    return sorted({chain, chain + G // 2, chain + G - 1, wave, wave + 32 * G, wave + 64 * G - 1, B, B + B // 2, 2 * B - 1})


def poly_cases(G):
    """every size with every coefficient set, the point moving through its six classes so that every set meets every point; the flag matrix
    and both placements at the sizes around a block; the two-round sizes of the short chain"""
    cases = []

    def add(c, z, flags=0, inplace=0):
        q, rem = fs.poly_div_linear(fs.read(c, bool(flags & IM)), z)
        cases.append(("D %d %d %d %x %s" % (G, flags, inplace, z, hexes(c)), fs.encode(q + [rem], bool(flags & OM))))
        cases.append(("E %d %d %x %s" % (G, flags, z, hexes(c)), fs.encode([rem], bool(flags & OM))))

    B = 256 * G
    for si, n in enumerate(sizes(G)):
        zs = fs.points(0x600 + n)
        for ci, name in enumerate(("zero", "r-1", "ones", "random", "multiple", "monomial")):
            z = zs[(si + ci) % 6]
            add(fs.coefficient_sets(0x700 + n, n, z)[name], z, inplace=(si + ci) & 1)
    for n in (G + 1, B + 1, 2 * B + 1):
        for flags in FLAG_SETS:
            for zi in (1, 4, 5):
                z = fs.points(0x800 + n)[zi]
                for name in ("random", "multiple"):
                    add(fs.coefficient_sets(0x900 + n, n, z, bool(flags & IM))[name], z, flags, inplace=flags >> 2 & 1)
    if G == 1:
        for n in (256 * 256 + 3, 2 * 256 * 256 - 1):
            z = fs.points(0xA00 + n)[5]
            add(fs.coefficient_sets(0xB00 + n, n, z)["random"], z, inplace=n & 1)
    return cases


def product_cases(G):
    cases = []

    def add(x, flags=0, inplace=0):
        out, total = fs.running_product(fs.read(x, bool(flags & IM)), bool(flags & EX))
        cases.append(("R %d %d %d %s" % (G, flags, inplace, hexes(x)), fs.encode(out + [total], bool(flags & OM))))

    B = 256 * G
    for si, n in enumerate(sizes(G)):
        sets = fs.product_sets(0xC00 + n, n, (0, n // 2, n - 1))
        for ci, name in enumerate(sorted(sets)):
            for ex in (0, EX):
                add(sets[name], ex, inplace=(si + ci) & 1)
    n = 2 * B + 1
    sets = fs.product_sets(0xD00, n, zero_places(G))
    for name in sorted(sets):
        if name.startswith("zero@"):
            add(sets[name], 0)
            add(sets[name], EX | IM | OM, inplace=1)
    for n in (G + 1, B + 1):
        x = fs.product_sets(0xE00 + n, n)["random"]
        x[:5] = [(1 << 256) - 1, R - 1, R + 1, 2 * R + 3, 1]
        for flags in FLAG_SETS:
            for ex in (0, EX):
                add(x, flags | ex, inplace=flags >> 1 & 1)
    if G == 1:
        for n in (256 * 256 + 3, 2 * 256 * 256 - 1):
            add(fs.product_sets(0xF00 + n, n)["random"], EX if n & 2 else 0, inplace=n & 1)
    return cases


@pytest.fixture(scope="module")
def cases():
    return {(what, G): (poly_cases if what == "poly" else product_cases)(G) for what in ("poly", "product") for G in (8, 1)}


def ask(run, queries_and_wants):
    got = run([q for q, _ in queries_and_wants])
    assert len(got) == len(queries_and_wants)
    for (q, want), g in zip(queries_and_wants, got):
        assert g == want, q[:60]


def test_the_plan_has_the_chain_the_cases_use():
    assert mh.fr_scan_plan(1)["chain"] == 8


@pytest.mark.parametrize("G", [8, 1])
@pytest.mark.parametrize("what", ["poly", "product"])
def test_the_routines_match_the_yardstick(check, cases, what, G):
    ask(check, cases[(what, G)])


@pytest.mark.parametrize("G", [8, 1])
def test_the_same_cases_under_the_sanitizers(check_asan, cases, G):
    for what in ("poly", "product"):
        ask(check_asan, cases[(what, G)])


def test_a_zero_zeroes_what_follows_and_nothing_before(check):
    G, B = 8, 2048
    n = 2 * B + 1
    places = zero_places(G)
    sets = fs.product_sets(0xD00, n, places)
    ref, *gots = check(["R %d 0 0 %s" % (G, hexes(sets[name])) for name in ["random"] + ["zero@%d" % at for at in places]])
    for at, got in zip(places, gots):
        assert got[:at] == ref[:at] and all(g == 0 for g in got[at:]) and got[at - 1] != 0, at
