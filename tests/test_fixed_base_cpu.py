"""The G1 fixed-base multiplication without a GPU: the new C-ABI symbols, the host-only plan, and a CPU run of the kernels' own routines -- digit
recoding, window table, product-tree batch inversion (tools/fixed_base_check.cpp, -DFP_BOUNDS_CHECK) -- against the oracle, word for word; once
more as a stand-alone program under AddressSanitizer / UBSan."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import mopro_msm_hip as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fixed_base_cases as fb  # noqa: E402

P, R = fb.P, fb.R
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"  # what csrc/Makefile builds the product with
NEW_SYMBOLS = ["msm_bn254_g1_fixed_base_plan", "msm_bn254_g1_fixed_base_mul_device", "msm_bn254_g1_fixed_base_mul"]
IM, OS = mh.NTT_IN_MONT, mh.FB_OUT_STD


def test_symbols_are_exported_bound_and_listed():
    lib = mh.load_library()
    hdr = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in mh.ABI_SYMBOLS and re.search(r"\b%s\s*\(" % s, hdr), s
        assert getattr(lib, s).argtypes is not None and getattr(lib, s).restype is C.c_int32, s
    assert re.search(r"#define\s+MSM_HIP_ABI_VERSION\s+7u?\b", hdr) and lib.msm_abi_version() == 7
    assert mh.FB_OUT_STD == 8 and re.search(r"#define\s+MSM_FB_OUT_STD\s+8u\b", hdr)
    assert C.sizeof(mh.FixedBasePlan) == 32
    rust = open(os.path.join(ROOT, "rust", "mopro-msm-hip", "src", "lib.rs")).read()
    hdr_code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NEW_SYMBOLS:  # declared by the shim with as many parameters as the header gives them
        m = re.search(r"\bfn %s\s*\((.*?)\)\s*->\s*i32;" % s, rust, re.S)
        assert m, s
        n_c = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % s, hdr_code, re.S).group(1).split(","))
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_c, s


def test_sizeof_the_plan_in_c(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include "msm_hip.h"\n_Static_assert(sizeof(msm_fixed_base_plan_t) == 32, "32 bytes");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")],
                   check=True, capture_output=True)


def test_plan():
    for c in range(4, 17):
        p = mh.fixed_base_plan(c)
        W = -(-257 // c)
        assert p["window_bits"] == c and p["num_windows"] == W and W * c >= 257 > (W - 1) * c
        assert p["table_entries"] == W << (c - 1) and p["table_bytes"] == 64 * p["table_entries"]
        assert p["inv_group"] >= 2 and p["inv_group"] & (p["inv_group"] - 1) == 0
    d = mh.fixed_base_plan(0)
    assert 4 <= d["window_bits"] <= 16 and d == mh.fixed_base_plan(d["window_bits"]) == mh.fixed_base_plan()
    for c in (3, 17, 1, 1 << 31):
        with pytest.raises(mh.MsmError) as e:
            mh.fixed_base_plan(c)
        assert e.value.code == mh.ERR_BAD_ARG and "window_bits" in str(e.value)
    assert mh.load_library().msm_bn254_g1_fixed_base_plan(8, None) == mh.ERR_BAD_ARG


def build_check(d, sanitize):
    exe = d / ("fixed_base_check_asan" if sanitize else "fixed_base_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([HIPCC, *flags, "-std=c++17", "-DFP_BOUNDS_CHECK", "-x", "hip", "--cuda-host-only",  # host code only: no device pass
                    os.path.join(ROOT, "tools", "fixed_base_check.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=900)

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
    return build_check(tmp_path_factory.mktemp("fixed_base_check"), False)


@pytest.fixture(scope="module")
def check_asan(tmp_path_factory):
    """the same program as a stand-alone host binary under AddressSanitizer and UBSan"""
    return build_check(tmp_path_factory.mktemp("fixed_base_check_asan"), True)


def digits_hold(run, widths, extra):
    for c in widths:
        ks = fb.edge_scalars(c) + extra
        lines = run(["D %d %x" % (c, k) for k in ks])
        W, H = -(-257 // c), 1 << (c - 1)
        for k, ln in zip(ks, lines):
            f = ln.split()
            d = [int(x) for x in f[2:]]
            assert f[0] == "D" and int(f[1]) == W == len(d), (c, hex(k))
            assert sum(dj << (c * j) for j, dj in enumerate(d)) == k and max(abs(x) for x in d) <= H, (c, hex(k), d)
        every = [int(x) for x in lines[-1 - len(extra)].split()[2:]]  # the last edge scalar: +2^(c-1) in every window that lies in 256 bits
        assert every[:256 // c] == [H] * (256 // c) and not any(every[256 // c:]), c


def products_hold(run, c, base, ks, flag_sets, from_file=False):
    """ks as the call reads them: integers; with IN_MONT the words are k * 2^256 mod r of a k that is reduced first"""
    queries, want = ["T %d %x %x" % (c, base[0], base[1])], []
    for flags in flag_sets:
        queries += ["M %x" % (k % R * fb.MONT_R % R if flags & IM else k) for k in ks] + ["R %d" % flags]
        want.append(fb.expected(ks, base, bool(flags & OS)))
    lines = run(queries, from_file)
    assert lines[0] == "T %d %d" % (-(-257 // c), -(-257 // c) << (c - 1)) and len(lines) == 1 + len(flag_sets) * len(ks)
    for s, (xy, inf) in enumerate(want):
        for i, k in enumerate(ks):
            f = lines[1 + s * len(ks) + i].split()
            got = (int(f[1]), int(f[2], 16), int(f[3], 16))
            assert got == (int(inf[i]), fb.orc.words_to_int(xy[i, :8]), fb.orc.words_to_int(xy[i, 8:])), (c, flag_sets[s], hex(k))


def inversions_hold(run, n_random):
    G = mh.fixed_base_plan()["inv_group"]
    z = [v % P or 1 for v in fb.patterns(11, G)]
    lists = [[0] + z[1:], z[:-1] + [0], [0] * G, [0 if i % 2 else v for i, v in enumerate(z)], z, z[:1], [0], [0, 0, 5, 0], z[:G // 2 + 1]]
    lists += [[0 if i == j else v for i, v in enumerate(z[:9])] for j in range(9)]  # the zero at every position of a short list
    lists += [[v if i == j else 0 for i, v in enumerate(z[:9])] for j in range(9)]  # and everything but one position zero
    lists = lists[:n_random] if n_random else lists
    lines = run(["I " + " ".join("%x" % v for v in zs) for zs in lists])
    for zs, ln in zip(lists, lines):
        f = ln.split()[1:]
        assert len(f) == 2 * len(zs)
        for i, v in enumerate(zs):
            assert (int(f[2 * i]), int(f[2 * i + 1], 16)) == ((0, pow(v, -1, P)) if v else (1, 0)), (len(zs), i)


def test_digits_of_every_edge_scalar(check):
    digits_hold(check, (4, 8, 13, 16), fb.patterns(3, 40))


def test_products_match_the_oracle(check):
    other = fb.point(0xC0FFEE)
    for c, base in ((4, fb.GEN), (8, other)):
        ks = fb.edge_scalars(c) + fb.patterns(c, 8 if base == other else 300)  # more than one inversion group for the generator
        products_hold(check, c, base, ks, (0, OS, IM, IM | OS))


def test_batch_inversion_with_zeros_everywhere(check):
    inversions_hold(check, 0)


def test_the_same_cases_under_the_sanitizers(check_asan):
    digits_hold(check_asan, (4, 8, 13, 16), fb.patterns(3, 4))
    products_hold(check_asan, 4, fb.GEN, fb.edge_scalars(4) + fb.patterns(4, 130), (0, IM | OS), from_file=True)
    products_hold(check_asan, 8, fb.point(0xC0FFEE), fb.edge_scalars(8), (OS,))
    inversions_hold(check_asan, 0)
