#!/usr/bin/env python3
"""Decoding and validating G2 points on one GPU, one process, after warm-up: per size (2^16, 2^18, 2^20) the median wall clock of
  msm_bn254_g2_decompress_device   checks 0 and MSM_G2_CHECK_SUBGROUP   (includes 64 B per point over PCIe)
  msm_bn254_g2_validate_device     MSM_G2_CHECK_SUBGROUP                (points already in HBM)
  msm_bn254_g1_decompress          the yardstick: G1's square root on the same sizes, same run (32 B per point up, 64 B + 1 B back)
and the accumulate kernel's clock from a neighbouring G1 MSM (msm_get_clock_stats), so that a slow box can be told from slow code.
Kernel times come from a second run of the same script under `rocprofv3 --kernel-trace --stats -- python tools/g2_points_timing.py --steps 5`.

  python tools/g2_points_timing.py [--steps K] [--warmup W] [--sizes 16,18,20]
"""
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
import bn254_g2_py as g2  # noqa: E402
import mopro_msm_hip as mh  # noqa: E402
from oracle import bn254_oracle as orc  # noqa: E402

M = 1 << 14  # distinct points, tiled (no kernel here depends on the points being distinct)


def median_ms(call, steps, warmup, sync):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(steps):
        sync()
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="16,18,20")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    pts = g2.chain_points(0x5EED, 0x1F2E3D, M)
    b2 = np.array([g2.point_words(p_, mont=True) for p_ in pts], np.uint32)
    b1 = orc.gen_bases_from_logs(orc.gen_scalars(0xB2540101, M, nonzero=True), orc.FORM_MONT).astype(np.uint32).reshape(M, 16)
    rows = []
    with mh.MsmContext(device=0) as ctx:
        for lg in [int(x) for x in a.sizes.split(",")]:
            n = 1 << lg
            t2 = np.ascontiguousarray(np.tile(b2, (n // M + 1, 1))[:n])
            t1 = np.ascontiguousarray(np.tile(b1, (n // M + 1, 1))[:n])
            img2 = torch.from_numpy(np.frombuffer(mh.compress_points_g2(t2, mh.FORM_MONT), np.uint8).copy()).pin_memory().numpy()
            img1 = torch.from_numpy(np.frombuffer(mh.compress_points(t1, mh.FORM_MONT), np.uint8).copy()).pin_memory().numpy()
            d_xy = torch.empty(n * 32, dtype=torch.int32, device=dev)
            d_inf = torch.empty(n, dtype=torch.uint8, device=dev)
            res = {"log2_n": lg}
            sync = torch.cuda.synchronize
            res["g2_decompress_device"] = median_ms(lambda: ctx.decompress_g2_device(img2, d_xy.data_ptr(), d_inf.data_ptr(), 0), a.steps, a.warmup, sync)
            res["g2_decompress_device_subgroup"] = median_ms(
                lambda: ctx.decompress_g2_device(img2, d_xy.data_ptr(), d_inf.data_ptr(), mh.G2_CHECK_SUBGROUP), a.steps, a.warmup, sync)
            assert (d_xy.cpu().numpy().view(np.uint32).reshape(n, 32) == t2).all()
            res["g2_validate_device_subgroup"] = median_ms(lambda: ctx.validate_g2_device(d_xy.data_ptr(), n, checks=mh.G2_CHECK_SUBGROUP), a.steps, a.warmup, sync)
            res["g2_validate_device_curve"] = median_ms(lambda: ctx.validate_g2_device(d_xy.data_ptr(), n, checks=mh.G2_CHECK_CURVE), a.steps, a.warmup, sync)
            res["g1_decompress"] = median_ms(lambda: ctx.decompress(img1), a.steps, a.warmup, sync)
            # the neighbouring G1 call: the accumulate kernel's clock on this box, now
            rng = np.random.default_rng(lg)
            s = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
            s[:, 7] &= 0x1FFFFFFF
            ds, db = torch.from_numpy(s.view(np.int32)).to(dev), torch.from_numpy(t1.view(np.int32)).to(dev)
            ctx.reset_kernel_stats()
            for _ in range(5):
                ctx.msm_device(db.data_ptr(), ds.data_ptr(), n)
            res["g1_msm_clock"] = ctx.clock_stats()
            rows.append(res)
            f = lambda k: "%.3f (min %.3f)" % res[k]
            print(f"2^{lg}: G2 decompress_device {f('g2_decompress_device')} ms, + subgroup {f('g2_decompress_device_subgroup')} ms, "
                  f"validate_device subgroup {f('g2_validate_device_subgroup')} ms, curve {f('g2_validate_device_curve')} ms; "
                  f"G1 decompress {f('g1_decompress')} ms; G1 MSM clock {res['g1_msm_clock']}", flush=True)
            del d_xy, d_inf, ds, db
    print(json.dumps({"g2_points_timing": rows, "median_of": a.steps, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
