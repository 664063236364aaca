"""The G2 group transform without a GPU: the new C-ABI symbols, the host-only plan, the yardstick (the cases of tools/g2_fft_cases.py) held against
the definition out[i] = sum_j w^(+-ij) * Q_j computed on the POINTS with the independent Python G2 law, and a CPU run of the kernels' own
per-butterfly routines -- the G1 transform's index arithmetic, bit reversal of 128-byte records, the ladder over Fq2, the two complete additions
to T and -T, the shared inversion by products of norms (tools/g2_fft_check.cpp, -DFP_BOUNDS_CHECK and the value bounds of g2_fft_bn254.hpp) --
against those cases, word for word; once more as a stand-alone program under AddressSanitizer / UBSan."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import g2_fft_cases as gc  # noqa: E402

P, R = gc.P, gc.R
g2 = gc.g2
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"  # what csrc/Makefile builds the product with
NEW_SYMBOLS = ["msm_bn254_g2_fft_plan", "msm_bn254_g2_fft_device", "msm_bn254_g2_fft"]
G = 256  # the inversion group the plan must report


def test_symbols_are_exported_bound_listed_and_the_plan_holds(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    for lib in (mh.load_library(), C.CDLL(os.path.join(ROOT, "gpu-acceleration_amd", "libmsm_hip_hooks.so"))):
        for s in NEW_SYMBOLS:
            assert hasattr(lib, s), s
    lib = mh.load_library()
    for s in NEW_SYMBOLS:
        assert s in mh.ABI_SYMBOLS and re.search(r"\b%s\s*\(" % s, hdr), s
        assert getattr(lib, s).argtypes is not None and getattr(lib, s).restype is C.c_int32, s
    assert re.search(r"#define\s+MSM_HIP_ABI_VERSION\s+7u?\b", hdr) and lib.msm_abi_version() == 7
    assert (mh.NTT_INVERSE, mh.FB_OUT_STD, mh.PM_BASES_STD) == (gc.INVERSE, gc.OUT_STD, gc.IN_STD) == (1, 8, 16)
    rust = open(os.path.join(ROOT, "rust", "mopro-msm-hip", "src", "lib.rs")).read()
    hdr_code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NEW_SYMBOLS:  # declared by the shim with as many parameters as the header gives them
        m = re.search(r"\bfn %s\s*\((.*?)\)\s*->\s*i32;" % s, rust, re.S)
        assert m, s
        n_c = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % s, hdr_code, re.S).group(1).split(","))
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_c, s
    # the plan's struct: 16 bytes here and for a C compiler
    assert C.sizeof(mh.G2FftPlan) == 16
    src = tmp_path / "size.c"
    src.write_text('#include "msm_hip.h"\n_Static_assert(sizeof(msm_g2_fft_plan_t) == 16, "16 bytes");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")],
                   check=True, capture_output=True)
    for name in ("g2_fft", "g2_fft_device", "g2_fft_plan"):
        assert callable(getattr(mh.MsmContext, name)), name
    for k in (0, 1, 2, 3, 9, 12, 20, 28):
        p = mh.g2_fft_plan(k)
        assert p == mh.MsmContext.g2_fft_plan(k) and set(p) == {"stages", "ladder_stages", "inv_group", "table_bytes"}
        assert p["stages"] == k and p["ladder_stages"] == max(k - 1, 0) and p["inv_group"] == G
        assert p["table_bytes"] == (32 << (k - 1) if k >= 2 else 0)  # n / 2 twiddles; no table where no stage runs a ladder
        assert p["table_bytes"] == mh.g1_fft_plan(k)["table_bytes"]  # one table serves both groups
    assert lib.msm_bn254_g2_fft_plan(3, None) == mh.ERR_BAD_ARG
    assert lib.msm_bn254_g2_fft_plan(29, C.byref(mh.G2FftPlan())) == mh.ERR_BAD_ARG
    with pytest.raises(mh.MsmError) as e:
        mh.g2_fft_plan(29)
    assert e.value.code == mh.ERR_BAD_ARG


# ---- the yardstick against the definition ---------------------------------------------------------------------------------------------------
def test_the_cases_hold_the_definition_on_points():
    """log_n = 3, both directions: out[i] = sum_j w^(+-ij) * Q_j (with n^-1 on the way back) by g2.mul / g2.add on the points themselves,
    never on their logarithms, with an identity among the inputs; the input records are those points' words"""
    k = 3
    n = 1 << k
    a = gc.logs(0x62D3F, n, zero_every=5)
    assert [j for j, v in enumerate(a) if v == 0] == [1, 6]
    pts = [None if v == 0 else g2.mul(gc.GEN, v) for v in a]
    xy, inf = gc.inputs(a)
    assert list(inf) == [1 if pt is None else 0 for pt in pts] and (xy[inf != 0] == gc.GARBAGE).all()
    for j, pt in enumerate(pts):
        if pt is not None:
            assert list(xy[j]) == list(g2.point_words(pt, True)), j
    w = gc.root(k)
    assert pow(w, n, R) == 1 and pow(w, n // 2, R) == R - 1
    for flags in (0, gc.INVERSE):
        ww, scale = (pow(w, -1, R), pow(n, -1, R)) if flags else (w, 1)
        out = []
        for i in range(n):
            acc = None
            for j, pt in enumerate(pts):
                if pt is not None:
                    acc = g2.add(acc, g2.mul(pt, scale * pow(ww, i * j, R) % R))
            out.append(acc)
        want_xy, want_inf = gc.expected(a, k, flags)
        assert list(want_inf) == [1 if o is None else 0 for o in out], flags
        for i, o in enumerate(out):
            assert list(want_xy[i]) == (list(g2.point_words(o, True)) if o is not None else [0] * 32), (flags, i)


# ---- the kernels' routines on the CPU ------------------------------------------------------------------------------------------------------
def build_check(d, sanitize):
    exe = d / ("g2_fft_check_asan" if sanitize else "g2_fft_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([HIPCC, *flags, "-std=c++17", "-DFP_BOUNDS_CHECK", "-x", "hip", "--cuda-host-only",  # host code only: no device pass
                    os.path.join(ROOT, "tools", "g2_fft_check.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=900)

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
    return build_check(tmp_path_factory.mktemp("g2_fft_check"), False)


@pytest.fixture(scope="module")
def check_asan(tmp_path_factory):
    """the same program as a stand-alone host binary under AddressSanitizer and UBSan"""
    return build_check(tmp_path_factory.mktemp("g2_fft_check_asan"), True)


def queue(xy, inf):
    return ["B %d %x %x %x %x" % ((inf[i],) + gc.point_ints(xy[i])) for i in range(len(inf))]


def parse(lines):
    return [(int(f[1]),) + tuple(int(v, 16) for v in f[2:6]) for f in (ln.split() for ln in lines)]


def as_tuples(want):
    xy, inf = want
    return [(int(inf[i]),) + gc.point_ints(xy[i]) for i in range(len(inf))]


def transforms_hold(run, jobs, from_file=False):
    """jobs: (logarithms, log_n, flags, batch, name); every output word against the cases"""
    q, want = [], []
    for a, k, flags, batch, _ in jobs:
        q += queue(*gc.inputs(a, flags)) + ["F %d %d" % (flags, k)]
        want += as_tuples(gc.expected(a, k, flags, batch))
    got = parse(run(q, len(want), from_file))
    at = 0
    for a, k, flags, batch, name in jobs:
        for i in range(len(a)):
            assert got[at + i] == want[at + i], (name, k, flags, i)
        at += len(a)


def stage_shape_jobs(flag_sets):
    """every stage shape of log_n = 0 .. 4 with identities among the inputs, and a batch of three"""
    jobs = []
    for k in range(5):
        for flags in flag_sets:
            jobs.append((gc.logs(0xF0 + k, 1 << k, zero_every=3 if k >= 2 else 0), k, flags, 1, "seeded"))
    jobs.append((gc.logs(0xBA7C, 3 << 3, zero_every=5), 3, gc.INVERSE, 3, "batch"))
    return jobs


def identity_jobs(log_ns, flag_sets):
    return [(a, k, flags, 1, name) for k in log_ns for name, a in gc.identity_cases(k).items() for flags in flag_sets]


def test_pairs_use_the_g1_index_arithmetic(check):
    """the program answers gf_pair of g1_fft_bn254.hpp (not a copy): a spot check of both directions at log_n = 4, every stage"""
    k = 4
    n = 1 << k
    q, want = [], []
    for s in range(1, k + 1):
        half = 1 << (s - 1)
        for inv in (0, 1):
            for item in range(n):  # two arrays
                arr, b = divmod(item, n // 2)
                g, j = divmod(b, half)
                a_at = arr * n + g * 2 * half + j
                t = j * (n >> s)
                swap = inv and t
                q.append("I %d %d %d %d" % (item, k, s, inv))
                want.append((a_at, a_at + half) + ((a_at + half, a_at) if swap else (a_at, a_at + half)) + ((n // 2 - t) if swap else t,))
    got = [tuple(int(v) for v in ln.split()[1:]) for ln in check(q, len(q))]
    assert got == want


def test_every_stage_shape_under_every_flag(check):
    transforms_hold(check, stage_shape_jobs(gc.FLAG_MATRIX))


def test_identities_doublings_and_cancellations(check):
    transforms_hold(check, identity_jobs((1, 2, 3, 4), (0, gc.INVERSE)))
    # flagged places carry garbage words in every job above (gc.GARBAGE); a flag byte other than 1 flags as well
    a = gc.logs(0xF1A6, 8, zero_every=2)
    xy, inf = gc.inputs(a)
    assert (xy[inf != 0] == gc.GARBAGE).all() and inf.any()
    q = queue(xy, inf * 0x80) + ["F 0 3"]
    assert parse(check(q, 8)) == as_tuples(gc.expected(a, 3))


def butterflies_hold(run, out_std):
    a, b = gc.logs(0xB077, 2)
    flags = gc.IN_STD | (gc.OUT_STD if out_std else 0)
    q, want = [], []
    for w in gc.edge_twiddles():
        for la, lb in ((a, b), (a, a), (b, R - b), (0, b), (a, 0), (0, 0), (w * b % R, b), (-w * b % R, b)):  # the last two: A = T and A = -T
            q += queue(*gc.points([la, lb], gc.FORM_STD)) + ["W %d %x" % (flags, w)]
            s, d = gc.butterfly_expected(la, lb, w % R, out_std)
            want += as_tuples((np.stack([s[0], d[0]]), np.array([s[1], d[1]])))
    assert parse(run(q, len(want))) == want


def test_edge_twiddles_in_one_butterfly(check):
    tw = gc.edge_twiddles()
    assert tw[:4] == [1, R - 1, gc.root(2), R - gc.root(2)] and pow(tw[4], 3, R) == 1 and tw[6] == 0
    butterflies_hold(check, False)
    butterflies_hold(check, True)


def test_the_same_cases_under_the_sanitizers(check_asan):
    transforms_hold(check_asan, stage_shape_jobs((0, gc.INVERSE | gc.IN_STD | gc.OUT_STD)) + identity_jobs((1, 4), (gc.INVERSE,)), from_file=True)
    butterflies_hold(check_asan, False)
