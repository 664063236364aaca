"""The R1CS rows without a GPU: the new C-ABI symbols, the host-only plan and its errors, the pure-Python yardstick against the definition, and a
CPU run of the upload plan and the kernels' own per-item and fold routines (tools/r1cs_check.cpp, -DFP_BOUNDS_CHECK) against the yardstick, word
for word -- once more under AddressSanitizer / UBSan for the host code that sorts and cuts caller data."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_fr_ntt_py as ny  # noqa: E402
import bn254_fr_r1cs_py as ry  # noqa: E402

R = ny.R
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"  # what csrc/Makefile builds the product with
NEW_SYMBOLS = ["msm_bn254_fr_r1cs_plan", "msm_bn254_fr_r1cs_upload", "msm_bn254_fr_r1cs_info", "msm_bn254_fr_r1cs_eval_device",
               "msm_bn254_fr_r1cs_eval"]
L = 24  # the item length: 24 * 7 r = 168 r < 2^261 (r1cs_bn254.hpp)
IM, OM, AB = mh.NTT_IN_MONT, mh.NTT_OUT_MONT, mh.R1CS_C_FROM_AB


def load_zkey_coeffs():
    """the reference key's coefficient records: (matrix, row, col, pattern) in MSM_R1CS_COEF_MONT2 form, and the header fields"""
    with open(os.path.join(ROOT, "tests", "golden", "zkey_r1cs_coeffs.json")) as f:
        d = json.load(f)
    return [(c["matrix"], c["row"], c["col"], int.from_bytes(bytes.fromhex(c["value_le_hex"]), "little")) for c in d["coefs"]], d


def test_symbols_are_exported_bound_and_listed():
    lib = mh.load_library()
    hdr = open(os.path.join(ROOT, "include", "msm_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in mh.ABI_SYMBOLS and re.search(r"\b%s\s*\(" % s, hdr), s
        assert getattr(lib, s).argtypes is not None and getattr(lib, s).restype is C.c_int32, s
    assert re.search(r"#define\s+MSM_HIP_ABI_VERSION\s+7u?\b", hdr) and lib.msm_abi_version() == 7
    assert (mh.R1CS_COEF_STD, mh.R1CS_COEF_MONT, mh.R1CS_COEF_MONT2, mh.R1CS_C_FROM_AB) == (0, 1, 2, 8)
    assert (ry.COEF_STD, ry.COEF_MONT, ry.COEF_MONT2, ry.C_FROM_AB) == (0, 1, 2, 8)
    for name, val in (("MSM_R1CS_COEF_STD", 0), ("MSM_R1CS_COEF_MONT", 1), ("MSM_R1CS_COEF_MONT2", 2), ("MSM_R1CS_C_FROM_AB", 8)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, val), hdr), name
    assert mh.R1CS_COEF_DTYPE.itemsize == 44 == ry.COEF_DTYPE.itemsize
    assert re.search(r"typedef struct \{ uint32_t matrix, row, col; uint32_t value\[8\]; \} msm_r1cs_coef_t;", hdr)
    assert C.sizeof(mh.R1csInfo) == 17 * 8
    rust = open(os.path.join(ROOT, "rust", "mopro-msm-hip", "src", "lib.rs")).read()
    hdr_code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NEW_SYMBOLS:  # declared by the shim with as many parameters as the header gives them
        m = re.search(r"\bfn %s\s*\((.*?)\)\s*->\s*i32;" % s, rust, re.S)
        assert m, s
        n_c = len(re.search(r"\b%s\s*\((.*?)\)\s*;" % s, hdr_code, re.S).group(1).split(","))
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_c, s


def test_sizeof_the_record_in_c(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include "msm_hip.h"\n_Static_assert(sizeof(msm_r1cs_coef_t) == 44, "44 bytes");\n'
                   '_Static_assert(sizeof(msm_r1cs_info_t) == 136, "17 x 8 bytes");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")],
                   check=True, capture_output=True)


def test_plan_on_small_lists():
    coefs = [(0, 0, 0, 1), (0, 0, 1, R - 1), (0, 0, 2, R + 1), (0, 0, 2, 2), (0, 2, 1, 7), (1, 1, 3, 2), (1, 1, 0, 0), (1, 3, 3, R + 2),
             (2, 4, 4, 2 * R - 1)]
    p = mh.r1cs_plan(coefs, 5, 5, 3)
    assert p["entries"] == [5, 3, 1] and p["rows_with_entries"] == [2, 2, 1]
    assert p["plus_one"] == 2 and p["minus_one"] == 2      # 1 and r + 1; r - 1 and 2r - 1
    assert p["distinct_values"] == 3                        # 2 (three times, once as r + 2), 7, 0
    assert p["longest_row"] == 4 and p["max_item_len"] == 4
    assert p["work_items"] == 15 and p["fold_rows"] == 0 and p["partial_sums"] == 0  # every row of a matrix with entries is an item
    assert p["device_bytes"] > 0 and p["upload_ms"] == 0
    # rows cut into items of L entries; the entries of matrix 1 alone
    long = [(1, 2, i % 7, 1) for i in range(3 * L + 1)] + [(1, 0, 0, 5)] * L
    p = mh.r1cs_plan(long, 3, 7, 2)
    assert p["entries"] == [0, 4 * L + 1, 0] and p["longest_row"] == 3 * L + 1 and p["max_item_len"] == L
    assert p["work_items"] == 1 + 1 + 4 and p["fold_rows"] == 1 and p["partial_sums"] == 4 and p["distinct_values"] == 1
    assert p["plus_one"] == 3 * L + 1 and p["minus_one"] == 0
    # the records' bytes as they would come out of a file
    assert mh.r1cs_plan(ry.pack(coefs).tobytes(), 5, 5, 3)["entries"] == [5, 3, 1]


def test_plan_reports_every_error_of_the_upload():
    ok = [(0, 0, 0, 1), (1, 1, 1, 1), (2, 2, 2, 1)]
    cases = [([], 3, 3, 2, mh.ERR_EMPTY, "Empty"),
             (ok + [(3, 0, 0, 1)], 3, 3, 2, mh.ERR_BAD_ARG, "entry 3: matrix"),
             (ok[:1] + [(0, 3, 0, 1)] + ok[1:], 3, 3, 2, mh.ERR_BAD_ARG, "entry 1: row"),
             (ok[:2] + [(0, 0, 3, 1)], 3, 3, 2, mh.ERR_BAD_ARG, "entry 2: col"),
             (ok, 5, 3, 2, mh.ERR_BAD_ARG, "num_rows"),
             (ok, 3, 3, 29, mh.ERR_BAD_ARG, "log_n")]
    for coefs, rows, cols, log_n, code, text in cases:
        with pytest.raises(mh.MsmError) as e:
            mh.r1cs_plan(coefs, rows, cols, log_n)
        assert e.value.code == code and text in str(e.value), (text, str(e.value))
    assert mh.r1cs_plan(ok, 3, 3, 2)["entries"] == [1, 1, 1]  # ... and the next call is fine


def test_yardstick_is_the_definition():
    coefs, d = load_zkey_coeffs()
    assert (d["n_vars"], d["n_public"], d["domain_size"], len(coefs)) == (4, 2, 4, 5) and int(d["r_hex"], 16) == R
    assert all(ry.coef_value(v, ry.COEF_MONT2) in (1, R - 1) for _, _, _, v in coefs)
    a, b, c = ry.evaluate(coefs, ry.COEF_MONT2, [1, 33, 3, 11], 2)
    assert a == [R - 3, 1, 33, 3] and b == [11, 0, 0, 0] and c == [0, 0, 0, 0]
    assert ry.evaluate(coefs, ry.COEF_MONT2, [1, 33, 3, 11], 2, True)[2] == [(R - 3) * 11 % R, 0, 0, 0]
    w = ry.eval_words(coefs, ry.COEF_MONT2, ny.to_words([1, 33, 3, 11]), 2)
    assert ny.from_words(w) == [R - 3, 1, 33, 3, 11, 0, 0, 0, 0, 0, 0, 0]
    rnd = random.Random(21)
    for form in (ry.COEF_STD, ry.COEF_MONT, ry.COEF_MONT2):  # a dense matrix against a plain double loop
        rows, cols = 13, 16
        dense = [[[rnd.randrange(R) for _ in range(cols)] for _ in range(rows)] for _ in range(3)]
        wit = [rnd.randrange(R) for _ in range(cols)]
        coefs = [(m, i, j, ry.coef_pattern(dense[m][i][j], form)) for m in range(3) for i in range(rows) for j in range(cols)]
        rnd.shuffle(coefs)
        got = ry.evaluate(coefs, form, wit, 4)
        for m in range(3):
            want = [0] * 16
            for i in range(rows):
                for j in range(cols):
                    want[i] = (want[i] + dense[m][i][j] * wit[j]) % R
            assert got[m] == want, (form, m)
        words = ry.eval_words(coefs, form, ny.to_words([v * ny.MONT % R for v in wit]), 4, IM | OM | AB)
        assert ny.from_words(words)[32:] == [x * y * ny.MONT % R for x, y in zip(got[0], got[1])]


def build_check(d, sanitize):
    exe = d / ("r1cs_check_asan" if sanitize else "r1cs_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    subprocess.run([HIPCC, *flags, "-std=c++17", "-DFP_BOUNDS_CHECK", "-x", "hip", "--cuda-host-only",  # host code only: no device pass
                    os.path.join(ROOT, "tools", "r1cs_check.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=900)

    def run(queries):
        r = subprocess.run([str(exe)], input="\n".join(queries) + "\n", capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = r.stdout.strip().split("\n")
        assert lines[-1] == "%d queries, no bound violated" % len(queries)
        return lines[:-1]

    return run


@pytest.fixture(scope="module")
def r1cs_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("r1cs_check")
    return d, build_check(d, False)


@pytest.fixture(scope="module")
def r1cs_check_asan(tmp_path_factory):
    """the same program as a stand-alone host binary under AddressSanitizer and UBSan"""
    d = tmp_path_factory.mktemp("r1cs_check_asan")
    return d, build_check(d, True)


def run_cases(d, run, cases):
    """cases: (coefs, form, rows, cols, log_n, flags, witness words); every output word against the yardstick"""
    queries, expect = [], []
    for i, (coefs, form, rows, cols, log_n, flags, wit) in enumerate(cases):
        fc, fw, fo = d / ("c%d.bin" % i), d / ("w%d.bin" % i), d / ("o%d.bin" % i)
        ry.pack(coefs).tofile(fc)
        wit.tofile(fw)
        queries.append("E %d %d %d %d %d %d %s %s %s" % (form, rows, cols, log_n, len(coefs), flags, fc, fw, fo))
        expect.append((fo, ry.eval_words(coefs, form, wit, log_n, flags)))
    lines = run(queries)
    assert all(ln.startswith("E ok ") for ln in lines) and len(lines) == len(queries)
    for (fo, want), case, ln in zip(expect, cases, lines):
        got = np.fromfile(fo, np.uint32).reshape(-1, 8)
        assert got.shape == want.shape and (got == want).all(), (case[1:6], ln)
    return [[int(x) for x in ln.split()[2:]] for ln in lines]


def edge_cases(forms, flag_sets, with_cs):
    rows, cols = 300, 211
    wit = ry.edge_witness(cols)
    return [(ry.edge_circuit(form, with_c, L, rows, cols), form, rows, cols, 9, flags, wit)
            for form in forms for with_c in with_cs for flags in flag_sets]


def test_cpu_run_of_the_kernel_routines_matches_the_yardstick(r1cs_check):
    d, run = r1cs_check
    cases = edge_cases((0, 1, 2), [f | ab for f in (0, IM, OM, IM | OM) for ab in (0, AB)], (True, False))
    stats = run_cases(d, run, cases)
    p = mh.r1cs_plan(cases[0][0], 300, 211, 9)
    assert p["max_item_len"] == L and p["longest_row"] >= 64 * L + 5 and p["fold_rows"] >= 3 and p["partial_sums"] >= 65 + 4 + 2
    items, folds, partials = stats[0][:3]
    assert (items, folds, partials) == (p["work_items"], p["fold_rows"], p["partial_sums"])
    assert all(s[3] > 5 and s[4] > 0 and s[5] > 0 for s in stats)  # general values, +1 and -1 entries in every form


def test_the_overflow_rows(r1cs_check):
    d, run = r1cs_check
    coefs, cols = ry.overflow_circuit(L)
    ones = ny.to_words([(1 << 256) - 1] * cols)
    cases = [(coefs, 0, 3, cols, 2, flags, ones) for flags in (0, IM, OM, IM | OM, AB)]
    shuffled = list(coefs)
    random.Random(5).shuffle(shuffled)
    cases.append((shuffled, 0, 3, cols, 2, 0, ones))
    cases.append(([(m, r_, c, ry.coef_pattern(v, 2)) for m, r_, c, v in coefs], 2, 3, cols, 2, IM, ones))
    stats = run_cases(d, run, cases)
    assert stats[0][:3] == [15, 3, 15] and stats[0][3:] == [1, cols, cols]
    s = ((1 << 256) - 1) * cols
    assert ny.from_words(ry.eval_words(coefs, 0, ones, 2))[:4] == [s % R, -s % R, -2 * s % R, 0]


def test_host_code_under_the_sanitizers(r1cs_check_asan):
    d, run = r1cs_check_asan
    coefs, cols = ry.overflow_circuit(L)
    cases = edge_cases((0, 2), (0, IM | OM | AB), (True, False))
    cases.append((coefs, 1, 3, cols, 2, OM, ny.to_words([(1 << 256) - 1] * cols)))
    zk, hdr = load_zkey_coeffs()
    cases.append((zk, 2, 4, 4, 2, 0, ny.to_words([1, 33, 3, 11])))
    run_cases(d, run, cases)
    # the plan alone, and the paths that reject caller data
    fc = d / "bad.bin"
    ry.pack([(0, 0, 0, 1), (1, 9, 0, 1), (3, 0, 0, 1)]).tofile(fc)
    lines = run(["P 0 10 1 4 3 %s" % fc, "P 0 9 1 4 3 %s" % fc, "P 0 10 1 4 2 %s" % fc, "P 0 10 1 2 2 %s" % fc])
    assert lines[0].startswith("P error -2 entry 2: matrix") and lines[1].startswith("P error -2 entry 1: row")
    assert lines[2].startswith("P ok 1 1 0 1 1 0 1 2 0 0 20 1 0 0 ") and lines[3].startswith("P error -2 num_rows")
