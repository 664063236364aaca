"""The G2 element-wise multiplication without a GPU: the new C-ABI symbols, the host-only plan, and a CPU run of the kernel's own per-lane
routines -- scalar reduction, GLV split, the three-entry table over Fq2, the joint ladder, the two shared inversions of the norms
(tools/g2_pointwise_mul_check.cpp, -DFP_BOUNDS_CHECK) -- against Python integers and the independent Python G2 law, word for word; once more
as a stand-alone program under AddressSanitizer / UBSan."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import mopro_msm_hip as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import g2_pointwise_mul_cases as pm2  # noqa: E402

P, R = pm2.P, pm2.R
g2 = pm2.g2
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"  # what csrc/Makefile builds the product with
NEW_SYMBOLS = ["msm_bn254_g2_pointwise_mul_plan", "msm_bn254_g2_pointwise_mul_device", "msm_bn254_g2_scale_device", "msm_bn254_g2_pointwise_mul"]
G = 256  # the inversion group the plan must report
ALL_FLAGS = [a | b | c for a in (0, 2) for b in (0, 8) for c in (0, 16)]  # NTT_IN_MONT, FB_OUT_STD, PM_BASES_STD


def test_symbols_are_exported_bound_listed_and_the_plan_holds(tmp_path):
    lib = mh.load_library()
    hdr = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in mh.ABI_SYMBOLS and re.search(r"\b%s\s*\(" % s, hdr), s
        assert getattr(lib, s).argtypes is not None and getattr(lib, s).restype is C.c_int32, s
    assert re.search(r"#define\s+MSM_HIP_ABI_VERSION\s+7u?\b", hdr) and lib.msm_abi_version() == 7 == mh.ABI_VERSION
    rust = open(os.path.join(ROOT, "rust", "mopro-msm-hip", "src", "lib.rs")).read()
    hdr_code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NEW_SYMBOLS:  # declared by the shim with as many parameters as the header gives them, and as the G1 sibling has
        m = re.search(r"\bfn %s\s*\((.*?)\)\s*->\s*i32;" % s, rust, re.S)
        assert m, s
        n_c = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % s, hdr_code, re.S).group(1).split(","))
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_c, s
        assert n_c == len(re.search(r"\b%s\s*\((.*?)\)\s*;" % s.replace("_g2_", "_g1_"), hdr_code, re.S).group(1).split(",")), s
        assert len(getattr(lib, s).argtypes) == n_c, s
    # the plan's struct: 16 bytes here and for a C compiler
    assert C.sizeof(mh.G2PointwisePlan) == 16
    src = tmp_path / "size.c"
    src.write_text('#include "msm_hip.h"\n_Static_assert(sizeof(msm_pointwise_g2_plan_t) == 16, "16 bytes");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")],
                   check=True, capture_output=True)
    p = mh.g2_pointwise_mul_plan()
    assert p == mh.MsmContext.g2_pointwise_mul_plan() and set(p) == {"inv_group", "ladder_bits", "table_points"}
    assert p["inv_group"] == G and p["ladder_bits"] == 126 == pm2.HALF_BITS and p["table_points"] == 3
    assert lib.msm_bn254_g2_pointwise_mul_plan(None) == mh.ERR_BAD_ARG


def test_the_endomorphism_constant_against_the_python_law_and_the_g2_msm():
    """beta^2 of the kernel's header is beta^2 of the split's constants and the constant the G2 MSM converts its bases with, and
    (beta^2 x, y) = lambda * (x, y) by the independent law"""
    csrc = os.path.join(ROOT, "gpu-acceleration_amd", "csrc")
    consts = []
    for name, sym in (("g2_pointwise_mul_bn254.hpp", "PM2_BETA2_STD"), ("msm_kernels_g2.hpp", "BETA2_STD")):
        m = re.search(r"constexpr uint32_t %s\[8\] = \{(.*?)\};" % sym, open(os.path.join(csrc, name)).read())
        consts.append(sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(m.group(1).split(","))))
    assert consts[0] == consts[1] == pm2.BETA2 == (-pm2.BETA - 1) % P
    assert pm2.LAMBDA not in (1, R - 1) and pm2.LAMBDA * pm2.LAMBDA % R == (-pm2.LAMBDA - 1) % R
    for pt in (pm2.GEN, g2.mul(pm2.GEN, 0xC0FFEE)):
        assert pm2.phi2(pt) == g2.mul(pt, pm2.LAMBDA)


def build_check(d, sanitize):
    exe = d / ("g2_pointwise_mul_check_asan" if sanitize else "g2_pointwise_mul_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([HIPCC, *flags, "-std=c++17", "-DFP_BOUNDS_CHECK", "-x", "hip", "--cuda-host-only",  # host code only: no device pass
                    os.path.join(ROOT, "tools", "g2_pointwise_mul_check.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=900)

    def run(queries, expect_lines, from_file=False):
        text = "\n".join(queries) + "\n"
        if from_file:
            (d / "queries.txt").write_text(text)
            r = subprocess.run([str(exe), str(d / "queries.txt")], capture_output=True, text=True, timeout=900)
        else:
            r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = r.stdout.strip().split("\n")
        assert lines[-1] == "%d queries, no bound violated" % len(queries) and len(lines) == expect_lines + 1
        return lines[:-1]

    return run


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("g2_pointwise_mul_check"), False)


@pytest.fixture(scope="module")
def check_asan(tmp_path_factory):
    """the same program as a stand-alone host binary under AddressSanitizer and UBSan"""
    return build_check(tmp_path_factory.mktemp("g2_pointwise_mul_check_asan"), True)


def as_read(k, flags):
    """the words the call is given for the integer k under flags: with IN_MONT k is reduced first and sent as k * 2^256 mod r"""
    return k % R * pm2.MONT_R % R if flags & mh.NTT_IN_MONT else k


def pt_hex(rec):
    return "%x %x %x %x" % pm2.point_ints(rec)


def flat(pt):
    return (pt[0][0], pt[0][1], pt[1][0], pt[1][1])


def splits_and_tables_hold(run, ks):
    """the halves (sign, magnitude) and P1, P2, S against Python integers"""
    lines = run(["S %d %x" % (f, as_read(k, f)) for f in (0, mh.NTT_IN_MONT) for k in ks], 2 * len(ks))
    for i, ln in enumerate(lines):
        k = ks[i % len(ks)]
        f = ln.split()
        k1, k2 = pm2.split(k % R)
        assert f[0] == "S" and (int(f[1]), int(f[2], 16), int(f[3]), int(f[4], 16)) == (int(k1 < 0), abs(k1), int(k2 < 0), abs(k2)), hex(k)
        assert abs(k1) < 1 << 126 and abs(k2) < 1 << 126
    pts = pm2.base_points(pm2.logs(0x7AB1E, len(ks)))
    arr = {form: pm2.point_array(pts, form) for form in (pm2.FORM_STD, pm2.FORM_MONT)}
    q = []
    for i, k in enumerate(ks):
        flags = (0, 2, 16, 18)[i % 4]
        q.append("T %d %s %x" % (flags, pt_hex(arr[pm2.FORM_STD if flags & mh.PM_BASES_STD else pm2.FORM_MONT][i]), as_read(k, flags)))
    for i, ln in enumerate(run(q, len(ks))):
        p1, p2, s = pm2.table(pts[i], ks[i])
        assert [int(v, 16) for v in ln.split()[1:]] == [*flat(p1), *flat(p2), *flat(s)], hex(ks[i])


def products_hold(run, ks, bs, inf, flag_sets, from_file=False):
    q, want = [], []
    arr = {form: pm2.bases(bs, form) for form in (pm2.FORM_STD, pm2.FORM_MONT)}
    for flags in flag_sets:
        b = arr[pm2.FORM_STD if flags & mh.PM_BASES_STD else pm2.FORM_MONT]
        for i, k in enumerate(ks):
            q += ["B %d %s" % (inf[i], pt_hex(b[i])), "M %x" % as_read(k, flags)]
        q.append("R %d" % flags)
    exp = {std: pm2.expected(ks, bs, inf, std) for std in (False, True)}
    want = [exp[bool(flags & mh.FB_OUT_STD)] for flags in flag_sets]
    lines = run(q, len(flag_sets) * len(ks), from_file)
    for s, (xy, winf) in enumerate(want):
        for i, k in enumerate(ks):
            f = lines[s * len(ks) + i].split()
            assert (int(f[1]),) + tuple(int(v, 16) for v in f[2:]) == (int(winf[i]),) + pm2.point_ints(xy[i]), (flag_sets[s], i, hex(k))


def one_scalar_holds(run, k_list, bs, inf, flags):
    b = pm2.bases(bs, pm2.FORM_STD if flags & mh.PM_BASES_STD else pm2.FORM_MONT)
    q = []
    for k in k_list:
        q += ["B %d %s" % (inf[i], pt_hex(b[i])) for i in range(len(bs))] + ["U %d %x" % (flags, k)]
    lines = run(q, len(k_list) * len(bs))
    for s, k in enumerate(k_list):
        xy, winf = pm2.expected([k] * len(bs), bs, inf, bool(flags & mh.FB_OUT_STD))
        for i in range(len(bs)):
            f = lines[s * len(bs) + i].split()
            assert (int(f[1]),) + tuple(int(v, 16) for v in f[2:]) == (int(winf[i]),) + pm2.point_ints(xy[i]), (hex(k), i)


def cases(n_patterns):
    """every edge scalar and n_patterns seeded ones on seeded bases; flagged bases among live ones at places 0, 255, 256 and last"""
    ks = pm2.edge_scalars() + pm2.patterns(0xE1E, n_patterns)
    bs = pm2.logs(0xBA5E5, len(ks))
    inf = [0] * len(ks)
    for i in (0, G - 1, G, len(ks) - 1):
        inf[i] = 1
    return ks, bs, inf


def test_split_and_table_against_python_integers(check):
    splits_and_tables_hold(check, pm2.edge_scalars() + pm2.patterns(3, 40))


def test_products_match_the_python_law_under_every_flag(check):
    ks, bs, inf = cases(300)
    assert 2 * G > len(ks) > G + 1 and sum(inf) == 4  # two groups, the second one partly filled
    for k in (0, 1, 2, 3, R - 1, R, R + 1, 2 * R, 5 * R, pm2.LAMBDA, 1 << 255):
        assert k in ks
    assert any(max(abs(h) for h in pm2.split(k % R)) >= 1 << 125 for k in ks)  # a half of the full 126 bits
    products_hold(check, ks, bs, inf, ALL_FLAGS)


def test_one_scalar_for_all_points(check):
    bs = pm2.logs(0x5CA1E, G + 3)
    inf = [1 if i in (0, G - 1, G) else 0 for i in range(G + 3)]
    one_scalar_holds(check, [0, 1, R - 1, pm2.LAMBDA, R, pm2.patterns(9, 1)[0] | 1 << 255], bs, inf, 0)
    one_scalar_holds(check, [pm2.LAMBDA + 1, (1 + pm2.LAMBDA) * 3 % R], bs[:5], [0, 1, 0, 0, 0], mh.FB_OUT_STD | mh.PM_BASES_STD)


def test_the_same_cases_under_the_sanitizers(check_asan):
    splits_and_tables_hold(check_asan, pm2.edge_scalars() + pm2.patterns(3, 4))
    ks, bs, inf = cases(G + 2 - len(pm2.edge_scalars()))  # the edge scalars and enough patterns for a second group
    assert len(ks) == G + 2
    products_hold(check_asan, ks, bs, inf, (0, 2 | 8 | 16), from_file=True)
    one_scalar_holds(check_asan, [0, R - 1, pm2.patterns(9, 1)[0]], bs[:7], [0, 0, 1, 0, 0, 0, 0], mh.FB_OUT_STD)
