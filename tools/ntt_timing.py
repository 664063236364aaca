#!/usr/bin/env python3
"""The scalar-field transforms on one GPU, one process: msm_bn254_fr_ntt_device at 2^16 .. 2^24 elements (in HBM, forward, standard form),
timed with events on the stream the calls are enqueued on, median of --steps runs after --warmup.  Per size, on ONE line: the median and
minimum ms, the passes of the plan, the algorithmic floor (passes x 2 x 32 n batch bytes at 8 TB/s) and the fraction of it reached,
msm_bn254_g1_device at the same n in the same process (median ms) with the accumulate kernel's clock (msm_get_clock_stats: a slow box is
recognisable), and the ratio NTT / MSM.  --recipe LOG_N adds the arkworks H recipe of INTEGRATION.md 4f (seven transforms and the pointwise
step on one stream) at that size.

  python tools/ntt_timing.py [--steps 20] [--warmup 3] [--sizes 16,18,20,22,24] [--batch 1] [--recipe 20] [--no-msm]

Run one size per process under a time limit of its own when the GPU is shared (tools/README.md)."""
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
import mopro_msm_hip as mh  # noqa: E402

PEAK_BYTES_PER_S = 8e12
M = 1 << 16
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="16,18,20,22,24")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--recipe", type=int, default=0)
    ap.add_argument("--no-msm", action="store_true")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    rows = []
    with mh.MsmContext(device=0) as ctx:
        for lg in [int(x) for x in a.sizes.split(",") if x]:
            n = 1 << lg
            rng = np.random.default_rng(lg)
            w = rng.integers(0, 1 << 32, size=(a.batch * n, 8), dtype=np.uint64).astype(np.uint32)
            w[:, 7] &= 0x1FFFFFFF
            d = torch.from_numpy(w.view(np.int32)).to(dev)
            torch.cuda.synchronize()
            ms = event_ms(torch, st, lambda: ctx.ntt_device(d.data_ptr(), lg, a.batch, 0, None, s), a.steps, a.warmup)
            passes = len(mh.ntt_plan(lg))
            floor_ms = passes * 2 * 32 * n * a.batch / PEAK_BYTES_PER_S * 1e3
            res = {"log2_n": lg, "batch": a.batch, "ntt_ms_median": statistics.median(ms), "ntt_ms_min": min(ms), "passes": passes,
                   "floor_ms_at_8TBps": floor_ms, "fraction_of_floor": floor_ms / statistics.median(ms)}
            line = (f"2^{lg} x {a.batch}: NTT {res['ntt_ms_median']:.4f} ms (min {res['ntt_ms_min']:.4f}), {passes} passes, floor {floor_ms:.4f} ms "
                    f"= {100 * res['fraction_of_floor']:.1f} % of 8 TB/s")
            if not a.no_msm:
                from oracle import bn254_oracle as orc
                b1 = orc.gen_bases_from_logs(orc.gen_scalars(0xB2540101, M, nonzero=True), orc.FORM_MONT).astype(np.uint32).reshape(M, 16)
                db = torch.from_numpy(np.ascontiguousarray(np.tile(b1, (n // M + 1, 1))[:n]).view(np.int32)).to(dev)
                ds = d[:n]
                for _ in range(a.warmup):
                    ctx.msm_device(db.data_ptr(), ds.data_ptr(), n)
                ctx.reset_kernel_stats()
                ctx.set_kernel_timing(1)
                mm = []
                for _ in range(a.steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ctx.msm_device(db.data_ptr(), ds.data_ptr(), n)
                    mm.append((time.perf_counter() - t0) * 1e3)
                ctx.set_kernel_timing(0)
                ck = ctx.clock_stats()
                res.update({"g1_msm_ms_median": statistics.median(mm), "sclk_ghz": ck["sclk_ghz"],
                            "ntt_over_msm": res["ntt_ms_median"] / statistics.median(mm)})
                line += f"; G1 MSM {res['g1_msm_ms_median']:.3f} ms at sclk {ck['sclk_ghz']:.3f} GHz, NTT / MSM = {res['ntt_over_msm']:.3f}"
                del db
            rows.append(res)
            print(line, flush=True)
            del d
        if a.recipe:
            lg = a.recipe
            n = 1 << lg
            rng = np.random.default_rng(77)
            w = rng.integers(0, 1 << 32, size=(3 * n, 8), dtype=np.uint64).astype(np.uint32)
            w[:, 7] &= 0x1FFFFFFF
            d = torch.from_numpy(w.view(np.int32)).to(dev)
            torch.cuda.synchronize()
            p = d.data_ptr()
            zinv = pow(pow(5, n, R) - 1, R - 2, R)
            I, IM, OM = mh.NTT_INVERSE, mh.NTT_IN_MONT, mh.NTT_OUT_MONT

            def recipe():
                ctx.ntt_device(p, lg, 3, I | OM, None, s)
                ctx.ntt_device(p, lg, 3, IM | OM, 5, s)
                ctx.fr_mul_sub_scale_device(p, p + 32 * n, p + 64 * n, p, n, zinv, IM | OM, s)
                ctx.ntt_device(p, lg, 1, I | IM, 5, s)

            ms = event_ms(torch, st, recipe, a.steps, a.warmup)
            rows.append({"recipe_log2_n": lg, "ms_median": statistics.median(ms), "ms_min": min(ms)})
            print(f"arkworks H recipe at 2^{lg} (7 transforms + pointwise, one stream): {statistics.median(ms):.4f} ms (min {min(ms):.4f})", flush=True)
    print(json.dumps({"ntt_timing": rows, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
