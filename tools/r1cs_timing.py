#!/usr/bin/env python3
"""The R1CS rows on one GPU, one process: msm_bn254_fr_r1cs_upload and msm_bn254_fr_r1cs_eval_device on synthetic circuits of 2^16 .. 2^22 rows
(as many columns; mean row length 3 in A and 2 in B, 90 % of the coefficients +1 or -1, sixteen rows of 2^16 entries; c = a o b), timed with
events on the stream the calls are enqueued on, median of --steps runs after --warmup.  Per size, on ONE line:
  the upload (whole call / its host part), the eval's median and minimum ms, the algorithmic floor at 8 TB/s (the entry bytes, 32 per gathered
  witness word, 96 per output row) and the fraction of it reached, the same circuit with every +1 / -1 replaced by 2 / r - 2 (every entry through
  the dictionary and a multiplication: what the special case saves), a forward transform of the same log_n, the copy of 96 * 2^log_n bytes from
  pinned memory (the step the eval removes), and msm_bn254_g1_device at the same n with the accumulate kernel's clock (a slow box is recognisable).
A few rows of every result, the long ones among them, are checked against Python integers.

  python tools/r1cs_timing.py [--steps 20] [--warmup 3] [--sizes 16,18,20,22] [--no-msm]

The synthetic shape stands in for a real circuit.  Run one size per process under a time limit of its own when the GPU is shared (tools/README.md)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gpu-acceleration_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mopro_msm_hip as mh  # noqa: E402
import bn254_fr_r1cs_py as ry  # noqa: E402

PEAK_BYTES_PER_S = 8e12
M = 1 << 16
R = ry.R
LONG_ROWS, LONG_LEN = 16, 1 << 16


def event_ms(torch, stream, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def to_int(words):
    return sum(int(x) << (32 * j) for j, x in enumerate(words.tolist()))


def spot_check(rec, wit, out, n, rows_to_check):
    """rows of a and b against Python integers"""
    for m in (0, 1):
        sel = rec[rec["matrix"] == m]
        for row in rows_to_check:
            e = sel[sel["row"] == row]
            want = sum(to_int(v) * to_int(wit[c]) for v, c in zip(e["value"], e["col"])) % R
            if to_int(out[m * n + row]) != want:
                raise SystemExit("WRONG RESULT: matrix %d row %d" % (m, row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="16,18,20,22")
    ap.add_argument("--no-msm", action="store_true")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    results = []
    with mh.MsmContext(device=0) as ctx:
        for lg in [int(x) for x in a.sizes.split(",") if x]:
            n = 1 << lg
            rec = ry.synthetic_array(0x7100 + lg, n, n, (3, 2, 0), 0.9, LONG_ROWS, LONG_LEN)
            rng = np.random.default_rng(lg)
            w = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
            w[:, 7] &= 0x1FFFFFFF
            dw = torch.from_numpy(w.view(np.int32)).to(dev)
            do = torch.zeros((3 * n, 8), dtype=torch.int32, device=dev)
            info = ctx.r1cs_upload(rec, n, n, lg)
            torch.cuda.synchronize()
            run = lambda: ctx.r1cs_eval_device(dw.data_ptr(), n, do.data_ptr(), mh.R1CS_C_FROM_AB, s)  # noqa: E731
            ms = event_ms(torch, st, run, a.steps, a.warmup)
            out = do.cpu().numpy().view(np.uint32)
            long_at = [(i * n) // LONG_ROWS for i in (0, LONG_ROWS - 1)]
            spot_check(rec, w, out, n, long_at + [1, n // 3, n - 1])
            entries = int(rec.shape[0])
            floor_ms = (info["device_bytes"] - info["partial_sums"] * 32 + 32 * entries + 96 * n) / PEAK_BYTES_PER_S * 1e3
            res = {"log2_rows": lg, "entries": entries, "upload_ms": info["upload_ms"], "build_ms": info["build_ms"], "device_bytes": info["device_bytes"],
                   "work_items": info["work_items"], "partial_sums": info["partial_sums"], "distinct_values": info["distinct_values"],
                   "eval_ms_median": statistics.median(ms), "eval_ms_min": min(ms), "floor_ms_at_8TBps": floor_ms,
                   "fraction_of_floor": floor_ms / statistics.median(ms)}
            # the same circuit with no +1 / -1 entry: 1 -> 2, r - 1 -> r - 2
            gen = rec.copy()
            v = gen["value"]
            is_one = (v[:, 0] == 1) & (v[:, 1:] == 0).all(axis=1)
            is_minus = (v == np.array([((R - 1) >> (32 * j)) & 0xFFFFFFFF for j in range(8)], np.uint32)).all(axis=1)
            v[is_one, 0] = 2
            v[is_minus, 0] -= 1
            gen["value"] = v
            ginfo = ctx.r1cs_upload(gen, n, n, lg)
            assert ginfo["plus_one"] == 0 and ginfo["minus_one"] == 0, ginfo
            res["eval_all_general_ms_median"] = statistics.median(event_ms(torch, st, run, a.steps, a.warmup))
            del gen, v
            # a forward transform of the same size, and the copy the eval removes
            res["ntt_ms_median"] = statistics.median(event_ms(torch, st, lambda: ctx.ntt_device(do.data_ptr(), lg, 1, 0, None, s), a.steps, a.warmup))
            pinned = torch.zeros((3 * n, 8), dtype=torch.int32).pin_memory()
            with torch.cuda.stream(st):
                res["h2d_copy_ms_median"] = statistics.median(event_ms(torch, st, lambda: do.copy_(pinned, non_blocking=True), a.steps, a.warmup))
            del pinned
            line = (f"2^{lg} rows, {entries} entries: upload {res['upload_ms']:.1f} ms (host build {res['build_ms']:.1f}), {info['device_bytes'] / 1e6:.1f} MB resident, "
                    f"{info['work_items']} items, {info['partial_sums']} partial sums, {info['distinct_values']} distinct values; "
                    f"eval {res['eval_ms_median']:.4f} ms (min {res['eval_ms_min']:.4f}), floor {floor_ms:.4f} ms = {100 * res['fraction_of_floor']:.1f} % of 8 TB/s; "
                    f"all entries general {res['eval_all_general_ms_median']:.4f} ms; forward NTT {res['ntt_ms_median']:.4f} ms; "
                    f"copy of {96 * n / 1e6:.1f} MB from pinned memory {res['h2d_copy_ms_median']:.4f} ms")
            if not a.no_msm:
                from oracle import bn254_oracle as orc
                b1 = orc.gen_bases_from_logs(orc.gen_scalars(0xB2540101, M, nonzero=True), orc.FORM_MONT).astype(np.uint32).reshape(M, 16)
                db = torch.from_numpy(np.ascontiguousarray(np.tile(b1, (n // M + 1, 1))[:n]).view(np.int32)).to(dev)
                for _ in range(a.warmup):
                    ctx.msm_device(db.data_ptr(), dw.data_ptr(), n)
                ctx.reset_kernel_stats()
                ctx.set_kernel_timing(1)
                mm = []
                for _ in range(a.steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ctx.msm_device(db.data_ptr(), dw.data_ptr(), n)
                    mm.append((time.perf_counter() - t0) * 1e3)
                ctx.set_kernel_timing(0)
                ck = ctx.clock_stats()
                res.update({"g1_msm_ms_median": statistics.median(mm), "sclk_ghz": ck["sclk_ghz"]})
                line += f"; G1 MSM {res['g1_msm_ms_median']:.3f} ms at sclk {ck['sclk_ghz']:.3f} GHz"
                del db
            results.append(res)
            print(line, flush=True)
            del dw, do, rec
    print(json.dumps({"r1cs_timing": results, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
