#!/usr/bin/env python3
"""G2 against G1 on one GPU, one process: device-pointer calls (msm_bn254_g2_device / msm_bn254_g1_device) at 2^16 .. 2^22 points, uniform
random scalars, after warm-up.  Prints per size the median ms of each, the ratio, the additions per call (msm_timings_t.num_adds) and the
accumulation kernel's shader cycles per mixed addition and clock (msm_get_clock_stats over the timed calls).

  python tools/g2_timing.py [--steps K] [--warmup W] [--sizes 16,18,20,22]

Bases: G2 points (a + (i mod 2^16) d) * G2 (tools/bn254_g2_py.py), G1 points from the oracle's generator (2^16 distinct, tiled)."""
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

M = 1 << 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="16,18,20,22")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    pts = g2.chain_points(0x5EED, 0x1F2E3D, M)
    b2 = np.array([[w for c in (p_[0][0], p_[0][1], p_[1][0], p_[1][1]) for w in g2.int_words(c * g2.R256 % g2.P)] for p_ in pts], np.uint32)
    b1 = orc.gen_bases_from_logs(orc.gen_scalars(0xB2540101, M, nonzero=True), orc.FORM_MONT).astype(np.uint32).reshape(M, 16)
    rows = []
    with mh.MsmContext(device=0) as ctx:
        for lg in [int(x) for x in a.sizes.split(",")]:
            n = 1 << lg
            rng = np.random.default_rng(lg)
            s = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
            s[:, 7] &= 0x1FFFFFFF
            ds = torch.from_numpy(s.view(np.int32)).to(dev)
            res = {"log2_n": lg}
            for name, base in (("g1", b1), ("g2", b2)):
                db = torch.from_numpy(np.ascontiguousarray(np.tile(base, (n // M + 1, 1))[:n]).view(np.int32)).to(dev)
                call = (lambda: ctx.msm_g2_device(db.data_ptr(), ds.data_ptr(), n)) if name == "g2" else (lambda: ctx.msm_device(db.data_ptr(), ds.data_ptr(), n))
                for _ in range(a.warmup):
                    call()
                ctx.reset_kernel_stats()
                ctx.set_kernel_timing(1)
                ms = []
                for _ in range(a.steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()
                    ms.append((time.perf_counter() - t0) * 1e3)
                ctx.set_kernel_timing(0)
                ck = ctx.clock_stats()
                acc_ms, _ = ctx.accumulate_kernel_stats()
                tm = ctx.timings()
                res[name] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "num_adds": int(tm["num_adds"]), "accumulate_ms": acc_ms, "clock": ck}
                del db
            res["ratio_g2_over_g1"] = res["g2"]["ms_median"] / res["g1"]["ms_median"]
            rows.append(res)
            print(f"2^{lg}: G1 {res['g1']['ms_median']:.3f} ms  G2 {res['g2']['ms_median']:.3f} ms  ratio {res['ratio_g2_over_g1']:.2f}  "
                  f"adds G1 {res['g1']['num_adds']} G2 {res['g2']['num_adds']}  accumulate G1 {res['g1']['accumulate_ms']:.3f} G2 {res['g2']['accumulate_ms']:.3f} ms  "
                  f"clock G1 {res['g1']['clock']} G2 {res['g2']['clock']}", flush=True)
    print(json.dumps({"g2_timing": rows, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
