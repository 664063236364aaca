"""The R1CS rows on the GPU (-m gpu): msm_bn254_fr_r1cs_upload / _eval(_device) against the pure-Python yardstick (tools/bn254_fr_r1cs_py.py), and
witness -> [a | b | c] -> H scalars -> MSM end to end on one stream with nothing crossing PCIe in between.  Inputs come from fixed seeds; every
comparison is word-exact."""
import json
import os
import sys

import numpy as np
import pytest

import mopro_msm_hip as mh
from conftest import load_zkey_points
from oracle import bn254_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn254_fr_ntt_py as ny  # noqa: E402
import bn254_fr_r1cs_py as ry  # noqa: E402

pytestmark = pytest.mark.gpu
R = ny.R
INV, IM, OM, AB = mh.NTT_INVERSE, mh.NTT_IN_MONT, mh.NTT_OUT_MONT, mh.R1CS_C_FROM_AB
L = 24
FILL = 0x5A5A5A5A  # d_out before every call: a row the kernels skip shows up


@pytest.fixture(scope="module")
def ctx():
    c = mh.MsmContext()
    yield c
    c.close()


def load_zkey_coeffs():
    """the reference key's coefficient records: (matrix, row, col, pattern) in MSM_R1CS_COEF_MONT2 form"""
    with open(os.path.join(ROOT, "tests", "golden", "zkey_r1cs_coeffs.json")) as f:
        d = json.load(f)
    return [(c["matrix"], c["row"], c["col"], int.from_bytes(bytes.fromhex(c["value_le_hex"]), "little")) for c in d["coefs"]]


ZK_WITNESS = [1, 33, 3, 11]


def dev(words):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32).copy()).to("cuda:0")


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32).reshape(-1, 8)


def filled(log_n):
    return dev(np.full((3 << log_n, 8), FILL, np.uint32))


def device_eval(c, wit, log_n, flags=0, stream=None):
    dw, do = dev(wit), filled(log_n)
    c.r1cs_eval_device(dw.data_ptr(), wit.shape[0], do.data_ptr(), flags, stream)
    return host(do)


@pytest.fixture(scope="module")
def edge():
    """the circuit of the CPU tests (300 x 211, log_n = 9) with a matrix 2, its witness, and the yardstick's words per flag set, computed once"""
    coefs, wit = ry.edge_circuit(ry.COEF_STD, True, L), ry.edge_witness(211)
    want = {f: ry.eval_words(coefs, ry.COEF_STD, wit, 9, f) for f in range(16) if not f & INV}
    return coefs, wit, want


def upload_edge(c, edge):
    return c.r1cs_upload(edge[0], 300, 211, 9)


# 1
def test_reference_key(ctx):
    coefs = load_zkey_coeffs()
    info = ctx.r1cs_upload(coefs, 4, 4, 2, mh.R1CS_COEF_MONT2)
    assert info["entries"] == [4, 1, 0] and info["plus_one"] == 4 and info["minus_one"] == 1 and info["distinct_values"] == 0
    wit = ny.to_words(ZK_WITNESS)
    want = ry.eval_words(coefs, ry.COEF_MONT2, wit, 2)
    assert ny.from_words(want)[:8] == [R - 3, 1, 33, 3, 11, 0, 0, 0]
    assert (ctx.r1cs_eval(wit, 2) == want).all()
    assert (device_eval(ctx, wit, 2) == want).all()
    assert (device_eval(ctx, wit, 2, AB) == ry.eval_words(coefs, ry.COEF_MONT2, wit, 2, AB)).all()


# 2
def test_edge_circuit_all_flags(ctx, edge):
    coefs, wit, want = edge
    info = upload_edge(ctx, edge)
    assert info["max_item_len"] == L and info["fold_rows"] >= 3 and info["partial_sums"] >= 71 and info["upload_ms"] >= info["build_ms"] > 0
    for flags, w in want.items():
        got = device_eval(ctx, wit, 9, flags)
        assert (got == w).all(), flags
        for m in range(3):
            assert not got[m * 512 + 300:(m + 1) * 512].any(), (flags, m)  # rows from num_rows up
        assert not got[0].any()                                            # matrix 0, row 0: no entries
    assert (ctx.r1cs_eval(wit, 9, OM) == want[OM]).all()
    for form in (ry.COEF_MONT, ry.COEF_MONT2):  # the other coefficient forms, and a matrix 2 without entries
        cf = ry.edge_circuit(form, False, L)
        ctx.r1cs_upload(cf, 300, 211, 9, form)
        for flags in (0, IM | OM, IM | AB):
            got = device_eval(ctx, wit, 9, flags)
            assert (got == ry.eval_words(cf, form, wit, 9, flags)).all(), (form, flags)
            assert flags & AB or not got[1024:].any()


# 3
def test_overflow_rows(ctx):
    coefs, cols = ry.overflow_circuit(L)
    ones = ny.to_words([(1 << 256) - 1] * cols)
    ctx.r1cs_upload(coefs, 3, cols, 2)
    for flags in (0, IM, OM, IM | OM, AB):
        assert (device_eval(ctx, ones, 2, flags) == ry.eval_words(coefs, 0, ones, 2, flags)).all(), flags


# 4
def test_synthetic_circuit_with_long_rows(ctx):
    rows, cols = 1 << 12, 3000
    coefs = ry.synthetic(0xA104, rows, cols, (3, 2, 1), 0.9, 4, 5000)
    assert 30000 < len(coefs) < 50000
    wit = ry.edge_witness(cols, 0xA105)
    info = ctx.r1cs_upload(ry.pack(coefs), rows, cols, 13)
    assert info["longest_row"] == 5000 and info["fold_rows"] == 4 and info["partial_sums"] == 4 * 209
    assert info["plus_one"] + info["minus_one"] > 0.85 * len(coefs) and 0 < info["distinct_values"] <= 64
    for flags in (0, IM | OM | AB):
        assert (device_eval(ctx, wit, 13, flags) == ry.eval_words(coefs, 0, wit, 13, flags)).all(), flags


# 5
def test_second_upload_replaces_the_first(ctx, edge):
    coefs, cols = ry.overflow_circuit(L)
    ctx.r1cs_upload(coefs, 3, cols, 2)
    upload_edge(ctx, edge)
    assert (device_eval(ctx, edge[1], 9) == edge[2][0]).all()
    zk = load_zkey_coeffs()
    ctx.r1cs_upload(zk, 4, 4, 2, mh.R1CS_COEF_MONT2)
    wit = ny.to_words(ZK_WITNESS)
    assert (device_eval(ctx, wit, 2) == ry.eval_words(zk, ry.COEF_MONT2, wit, 2)).all()
    with pytest.raises(mh.MsmError) as e:  # a rejected upload leaves the resident one alone
        ctx.r1cs_upload(zk + [(0, 4, 0, 1)], 4, 4, 2, mh.R1CS_COEF_MONT2)
    assert e.value.code == mh.ERR_BAD_ARG and "entry 5: row" in str(e.value)
    assert (device_eval(ctx, wit, 2) == ry.eval_words(zk, ry.COEF_MONT2, wit, 2)).all()


# 6 - 9
def test_errors_leave_the_context_usable(edge):
    coefs, wit, want = edge
    with mh.MsmContext() as c:
        dw, do = dev(wit), filled(9)
        with pytest.raises(mh.MsmError) as e:  # 6
            c.r1cs_eval_device(dw.data_ptr(), 211, do.data_ptr())
        assert e.value.code == mh.ERR_STATE
        with pytest.raises(mh.MsmError) as e:
            c.r1cs_info()
        assert e.value.code == mh.ERR_STATE
        upload_edge(c, edge)

        def good():  # 9
            assert (device_eval(c, wit, 9) == want[0]).all()

        good()
        for call, code in ((lambda: c.r1cs_eval_device(dw.data_ptr(), 210, do.data_ptr()), mh.ERR_BAD_ARG),              # 7
                           (lambda: c.r1cs_eval_device(dw.data_ptr() + 8, 211, do.data_ptr()), mh.ERR_BAD_ARG),          # 8
                           (lambda: c.r1cs_eval_device(dw.data_ptr(), 211, do.data_ptr() + 4), mh.ERR_BAD_ARG),
                           (lambda: c.r1cs_eval_device(dw.data_ptr(), 211, do.data_ptr(), INV), mh.ERR_BAD_ARG),
                           (lambda: c.r1cs_eval_device(dw.data_ptr(), 211, do.data_ptr(), 16), mh.ERR_BAD_ARG),
                           (lambda: c.r1cs_eval_device(None, 211, do.data_ptr()), mh.ERR_BAD_ARG),
                           (lambda: c.r1cs_eval_device(dw.data_ptr(), 211, None), mh.ERR_BAD_ARG),
                           (lambda: c.r1cs_upload([], 300, 211, 9), mh.ERR_EMPTY),
                           (lambda: c.r1cs_upload(coefs, 300, 211, 8), mh.ERR_BAD_ARG),
                           (lambda: c.r1cs_upload(coefs, 300, 211, 29), mh.ERR_BAD_ARG),
                           (lambda: c.r1cs_upload(coefs, 300, 211, 9, 3), mh.ERR_BAD_ARG),
                           (lambda: c.r1cs_upload(coefs, 300, 210, 9), mh.ERR_BAD_ARG),
                           (lambda: c.r1cs_upload(coefs + [(3, 0, 0, 1)], 300, 211, 9), mh.ERR_BAD_ARG)):
            with pytest.raises(mh.MsmError) as e:
                call()
            assert e.value.code == code
            good()
        assert (host(do) == FILL).all()  # no failed call touched the array


# 10
def test_two_streams_back_to_back(ctx):
    import torch
    rows, cols = 600, 400
    coefs = ry.synthetic(0xA110, rows, cols, (3, 2, 1), 0.9, 3, 2000)
    ctx.r1cs_upload(ry.pack(coefs), rows, cols, 10)
    w1, w2 = ry.edge_witness(cols, 1), ry.edge_witness(cols, 2)
    d1, d2, o1, o2 = dev(w1), dev(w2), filled(10), filled(10)
    s1, s2 = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    ctx.r1cs_eval_device(d1.data_ptr(), cols, o1.data_ptr(), 0, s1.cuda_stream)
    ctx.r1cs_eval_device(d2.data_ptr(), cols, o2.data_ptr(), OM, s2.cuda_stream)
    s1.synchronize(), s2.synchronize()
    assert (host(o1) == ry.eval_words(coefs, 0, w1, 10, 0)).all()
    assert (host(o2) == ry.eval_words(coefs, 0, w2, 10, OM)).all()


# 11
def snarkjs_h_on_stream(c, d_wit, n_wit, k, st):
    """witness in HBM -> [a | b | c] -> the snarkjs H recipe of INTEGRATION.md 4f, all enqueued on one stream; the H scalars end in a's place"""
    n = 1 << k
    d = filled(k)
    import torch
    torch.cuda.synchronize()
    p, s = d.data_ptr(), st.cuda_stream
    c.r1cs_eval_device(d_wit.data_ptr(), n_wit, p, AB, s)
    c.ntt_device(p, k, 3, INV | OM, None, s)
    c.ntt_device(p, k, 3, IM | OM, ny.root(k + 1), s)
    c.fr_mul_sub_scale_device(p, p + 32 * n, p + 64 * n, p, n, None, IM, s)
    return d


def yardstick_h(coefs, form, wit_ints, k):
    a, b, c = ry.evaluate(coefs, form, wit_ints, k, True)
    g = ny.root(k + 1)
    ea, eb, ec = (ny.ntt(ny.ntt(v, 1, True), g) for v in (a, b, c))
    return [(x * y - z) % R for x, y, z in zip(ea, eb, ec)]


def test_witness_to_h_scalars_end_to_end(ctx, edge):
    import torch
    st = torch.cuda.Stream(device="cuda:0")
    # the reference key: log_n = 2, and the H scalars go on into the MSM over the key's four H points
    zk = load_zkey_coeffs()
    ctx.r1cs_upload(zk, 4, 4, 2, mh.R1CS_COEF_MONT2)
    bases, inf, _, _, d = load_zkey_points()
    sel = [i for i, p in enumerate(d["points"]) if p["section"] == "H"]
    assert len(sel) == 4
    hb, hi = np.ascontiguousarray(bases[sel]), np.ascontiguousarray(inf[sel])
    ctx.upload_bases(hb, mh.FORM_MONT, hi)
    dh = snarkjs_h_on_stream(ctx, dev(ny.to_words(ZK_WITNESS)), 4, 2, st)
    r = ctx.msm_resident_device(dh.data_ptr(), 4, st.cuda_stream)  # h never left HBM
    st.synchronize()
    want = yardstick_h(zk, ry.COEF_MONT2, ZK_WITNESS, 2)
    assert any(want) and (host(dh)[:4] == ny.to_words(want)).all()
    exp, einf, _ = orc.msm_pippenger(hb, ny.to_words(want), orc.FORM_MONT, hi)
    assert bool(r.is_infinity) == bool(einf) and (r.affine_std == exp).all()
    # the circuit of test 2 at log_n = 9
    coefs, wit, _ = edge
    upload_edge(ctx, edge)
    dh = snarkjs_h_on_stream(ctx, dev(wit), 211, 9, st)
    st.synchronize()
    want = yardstick_h(coefs, ry.COEF_STD, [v % R for v in ny.from_words(wit)], 9)
    assert (host(dh)[:512] == ny.to_words(want)).all()
