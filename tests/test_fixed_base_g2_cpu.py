"""The G2 fixed-base multiplication without a GPU: the new C-ABI symbols, the host-only plan, the Python model of the expected values against
g2.mul, and a CPU run of the kernels' own routines -- table step, product, norm, chain inversion, output conversion
(tools/fixed_base_g2_check.cpp, -DFP_BOUNDS_CHECK) -- against that model, word for word; once more as a stand-alone program under
AddressSanitizer / UBSan."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import mopro_msm_hip as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fixed_base_g2_cases as fb2  # noqa: E402

g2 = fb2.g2
P, R = fb2.P, fb2.R
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"  # what csrc/Makefile builds the product with
NEW_SYMBOLS = ["msm_bn254_g2_fixed_base_plan", "msm_bn254_g2_fixed_base_mul_device", "msm_bn254_g2_fixed_base_mul"]
IM, OS = mh.NTT_IN_MONT, mh.FB_OUT_STD
OTHER = None


def other_base():
    global OTHER
    if OTHER is None:
        OTHER = g2.mul(g2.G2_GEN, 0xC0FFEE)
    return OTHER


def test_symbols_are_exported_bound_and_listed():
    lib = mh.load_library()
    hdr = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in mh.ABI_SYMBOLS and re.search(r"\b%s\s*\(" % s, hdr), s
        assert getattr(lib, s).argtypes is not None and getattr(lib, s).restype is C.c_int32, s
    assert re.search(r"#define\s+MSM_HIP_ABI_VERSION\s+7u?\b", hdr) and lib.msm_abi_version() == 7
    assert C.sizeof(mh.FixedBaseG2Plan) == 40
    rust = open(os.path.join(ROOT, "rust", "mopro-msm-hip", "src", "lib.rs")).read()
    hdr_code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NEW_SYMBOLS:  # declared by the shim with as many parameters as the header gives them
        m = re.search(r"\bfn %s\s*\((.*?)\)\s*->\s*i32;" % s, rust, re.S)
        assert m, s
        n_c = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % s, hdr_code, re.S).group(1).split(","))
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_c, s


def test_sizeof_the_plan_in_c(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include "msm_hip.h"\n_Static_assert(sizeof(msm_fixed_base_g2_plan_t) == 40, "40 bytes");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")],
                   check=True, capture_output=True)


def test_plan():
    for c in range(4, 17):
        p = mh.fixed_base_g2_plan(c)
        W = -(-257 // c)
        assert p["window_bits"] == c and p["num_windows"] == W and W * c >= 257 > (W - 1) * c
        assert p["table_entries"] == W << (c - 1) and p["table_bytes"] == 128 * p["table_entries"]
        assert p["inv_group"] >= 2
        assert p["chunk_points"] > 0 and p["chunk_points"] % p["inv_group"] == 0
        assert p["scratch_bytes"] > 0
    d = mh.fixed_base_g2_plan(0)
    assert 4 <= d["window_bits"] <= 16 and d == mh.fixed_base_g2_plan(d["window_bits"]) == mh.fixed_base_g2_plan()
    for c in (3, 17, 1 << 31):
        with pytest.raises(mh.MsmError) as e:
            mh.fixed_base_g2_plan(c)
        assert e.value.code == mh.ERR_BAD_ARG and "window_bits" in str(e.value)
    assert mh.load_library().msm_bn254_g2_fixed_base_plan(8, None) == mh.ERR_BAD_ARG


def test_the_model_agrees_with_the_python_law():
    ks = [0, 1, 2, R - 1, R, R + 1, 2 * R, 5 * R, (1 << 256) - 1, 1 << 255, 255, 256, (1 << 248) - 1] + fb2.patterns(5, 24)
    assert len(ks) >= 32
    got = fb2.points(ks)
    for k, pt in zip(ks, got):
        assert pt == g2.mul(g2.G2_GEN, k), hex(k)
    assert [pt is None for pt in got[:8]] == [True, False, False, False, True, False, True, True]
    b = other_base()
    assert b != g2.G2_GEN and g2.on_curve(b)
    ks_b = [0, 1, R - 1, R + 1, 5 * R, (1 << 256) - 1] + fb2.patterns(6, 6)
    for k, pt in zip(ks_b, fb2.points(ks_b, b)):
        assert pt == g2.mul(b, k), hex(k)
    xy, inf = fb2.expected([0, 1], out_std=True)
    assert list(inf) == [1, 0] and not xy[0].any() and list(xy[1]) == g2.point_words(g2.G2_GEN)
    q = fb2.off_subgroup_point()
    assert g2.on_curve(q) and not g2.in_subgroup(q)


def build_check(d, sanitize):
    exe = d / ("fixed_base_g2_check_asan" if sanitize else "fixed_base_g2_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([HIPCC, *flags, "-std=c++17", "-DFP_BOUNDS_CHECK", "-x", "hip", "--cuda-host-only",  # host code only: no device pass
                    os.path.join(ROOT, "tools", "fixed_base_g2_check.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=900)

    def run(queries, from_file=False):
        text = "\n".join(queries) + "\n"
        if from_file:
            (d / "queries.txt").write_text(text)
            r = subprocess.run([str(exe), str(d / "queries.txt")], capture_output=True, text=True, timeout=900)
        else:
            r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = r.stdout.strip().split("\n")
        assert lines[-1] == "%d queries, no bound violated" % len(queries)
        return lines[:-1]

    return run


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("fixed_base_g2_check"), False)


@pytest.fixture(scope="module")
def check_asan(tmp_path_factory):
    """the same program as a stand-alone host binary under AddressSanitizer and UBSan"""
    return build_check(tmp_path_factory.mktemp("fixed_base_g2_check_asan"), True)


def coords(pt):
    return (pt[0][0], pt[0][1], pt[1][0], pt[1][1])


def t_query(c, base):
    return "T %d %x %x %x %x" % ((c,) + coords(base))


def table_levels_hold(run, widths, base):
    """every record of every level: T_j[d] = d * 2^(c j) * base"""
    for c in widths:
        W, half = -(-257 // c), 1 << (c - 1)
        windows = sorted({0, 1, W // 2, W - 1})
        ask = [(j, d) for j in windows for d in range(1, half + 1)]
        lines = run([t_query(c, base)] + ["E %d %d" % jd for jd in ask])
        assert lines[0] == "T %d %d" % (W, W * half)
        want = fb2.points([d << (c * j) for j, d in ask], base)
        for jd, ln, pt in zip(ask, lines[1:], want):
            f = ln.split()
            assert f[0] == "E" and tuple(int(v, 16) for v in f[1:]) == coords(pt), (c, jd)


def products_hold(run, c, base, ks, flag_sets, from_file=False):
    """ks as the call reads them: integers; with IN_MONT the words are k * 2^256 mod r of a k that is reduced first"""
    queries, want = [t_query(c, base)], []
    for flags in flag_sets:
        queries += ["M %x" % (k % R * fb2.MONT_R % R if flags & IM else k) for k in ks] + ["R %d" % flags]
        want.append(fb2.expected(ks, base, bool(flags & OS)))
    lines = run(queries, from_file)
    assert lines[0] == "T %d %d" % (-(-257 // c), -(-257 // c) << (c - 1)) and len(lines) == 1 + len(flag_sets) * len(ks)
    for s, (xy, inf) in enumerate(want):
        for i, k in enumerate(ks):
            f = lines[1 + s * len(ks) + i].split()
            got = (int(f[1]),) + tuple(int(v, 16) for v in f[2:6])
            assert got == (int(inf[i]),) + tuple(g2.words_int(xy[i, 8 * q:8 * q + 8]) for q in range(4)), (c, flag_sets[s], hex(k))


def inversions_hold(run):
    """chains with identities at the first, last, every second and all places; a chain of length 1 at the tail of the array; two waves"""
    G = mh.fixed_base_g2_plan()["inv_group"]
    n = 64 * G + 1  # the last point is a chain of length 1 of the second wave's first lane
    z = [(v % P or 1, w % P) for v, w in zip(fb2.patterns(11, n), fb2.patterns(12, n))]
    chain0 = [s * 64 for s in range(G)]  # the points of lane 0's chain
    O = (0, 0)
    cases = [(G, z)]
    for at in ([chain0[0]], [chain0[-1]], chain0[::2], chain0, list(range(n)), [n - 1], list(range(0, n, 2))):
        zs = list(z)
        for i in at:
            zs[i] = O
        cases.append((G, zs))
    cases += [(2, z[:129]), (2, z[:128] + [O]), (8, z[:8 * 64 - 1]), (32, z[:70]), (1, z[:3]), (G, z[:1]), (G, [O])]
    lines = run(["I %d " % g + " ".join("%x %x" % v for v in zs) for g, zs in cases])
    for (g, zs), ln in zip(cases, lines):
        f = ln.split()[1:]
        assert len(f) == 3 * len(zs)
        for i, v in enumerate(zs):
            want = (1, 0, 0) if v == O else (0,) + g2.inv2(v)
            assert (int(f[3 * i]), int(f[3 * i + 1], 16), int(f[3 * i + 2], 16)) == want, (g, len(zs), i)


def test_table_levels_match_the_model(check):
    table_levels_hold(check, (4, 5), g2.G2_GEN)
    table_levels_hold(check, (8,), other_base())


def test_products_match_the_model(check):
    for c, base in ((4, g2.G2_GEN), (8, other_base()), (13, g2.G2_GEN), (16, g2.G2_GEN)):
        ks = fb2.edge_scalars(c) + fb2.patterns(c, 8)
        products_hold(check, c, base, ks, (0, OS, IM))


def test_chain_inversion_with_identities_everywhere(check):
    inversions_hold(check)


def test_the_same_cases_under_the_sanitizers(check_asan):
    table_levels_hold(check_asan, (4, 5), g2.G2_GEN)
    table_levels_hold(check_asan, (8,), other_base())
    for c, base in ((4, g2.G2_GEN), (8, other_base()), (13, g2.G2_GEN), (16, g2.G2_GEN)):
        ks = fb2.edge_scalars(c) + fb2.patterns(c, 8)
        products_hold(check_asan, c, base, ks, (0, OS, IM), from_file=(c == 4))
    inversions_hold(check_asan)
