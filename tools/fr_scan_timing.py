#!/usr/bin/env python3
"""The scalar-field scans on one GPU, the whole sweep in one process (run it under a time limit when the GPU is shared, tools/README.md):

  per size 2^16, 2^18, 2^20, 2^22 (--log2 16,18,20,22): msm_bn254_fr_poly_eval_device, _poly_div_linear_device (out of place and in place) and
      _running_product_device (inclusive and exclusive), median and minimum of --steps calls after --warmup, by events on the call's stream;
      beside them, in the same process, what they are measured against: a one-term msm_bn254_fr_lincomb_device (the same one read and one
      write), one forward transform of the size, the hipMemcpy of n x 32 bytes from and to pinned host memory that a call replaces (a caller
      without it copies the coefficients out and the quotient back), and msm_bn254_g1_device at the same n, the MSM a quotient feeds.

  python tools/fr_scan_timing.py [--steps 20] [--warmup 3] [--out profiles/fr_scan_timing_mi355x.txt]

The first and last elements of every result, the remainder and the total are checked against the Python yardstick.  Every result line is printed
and, with --out, appended."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gpu-acceleration_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mopro_msm_hip as mh  # noqa: E402
import bn254_fr_scan_py as fs  # noqa: E402
import fixed_base_cases as fb  # noqa: E402
from fixed_base_timing import event_ms, med_min  # noqa: E402

R = fs.R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", default="16,18,20,22")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(device=dev)
    s = st.cuda_stream
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def must(what, got, want):
        if got != want:
            raise SystemExit("WRONG RESULT at %s" % (what,))

    def words(t, lo, hi):
        torch.cuda.synchronize()
        return fs.from_words(t[lo:hi].cpu().numpy().view(np.uint32))

    z = fs.patterns(0x5CA7, 1)[0]
    sizes = [int(v) for v in a.log2.split(",") if v]
    nmax = 1 << max(sizes)
    rng = np.random.default_rng(0x5CA8)
    h_x = rng.integers(0, 1 << 32, size=(nmax, 8), dtype=np.uint64).astype(np.uint32)
    d_x = torch.from_numpy(h_x.view(np.int32)).to(dev)
    d_out = torch.zeros((nmax, 8), dtype=torch.int32, device=dev)
    d_io = torch.zeros((nmax, 8), dtype=torch.int32, device=dev)
    d_one = torch.zeros((1, 8), dtype=torch.int32, device=dev)
    h_pin = torch.from_numpy(h_x.view(np.int32)).pin_memory()
    h_back = torch.zeros((nmax, 8), dtype=torch.int32).pin_memory()
    torch.cuda.synchronize()

    with mh.MsmContext(device=0) as ctx:
        for lg in sizes:
            n = 1 << lg
            plan = mh.fr_scan_plan(n)
            say(f"2^{lg}: plan {plan}")
            x = fs.from_words(h_x[:n])
            q, rem = fs.poly_div_linear(fs.read(x), z)
            inc, total = fs.running_product(fs.read(x))
            ends = lambda v: v[:3] + v[n - 3:n]
            got_ends = lambda t: words(t, 0, 3) + words(t, n - 3, n)
            ev = {}
            ev["poly_eval"] = event_ms(torch, st, lambda: ctx.fr_poly_eval_device(d_x.data_ptr(), n, z, d_one.data_ptr(), stream=s), a.steps, a.warmup)
            must(("eval", lg), words(d_one, 0, 1), [rem])
            ev["poly_div_linear"] = event_ms(torch, st, lambda: ctx.fr_poly_div_linear_device(d_x.data_ptr(), n, z, d_out.data_ptr(), d_one.data_ptr(), stream=s),
                                             a.steps, a.warmup)
            must(("div", lg), got_ends(d_out) + words(d_one, 0, 1), ends(q) + [rem])
            # in place: the array changes from call to call, the time does not depend on the values
            d_io[:n].copy_(d_x[:n])
            torch.cuda.synchronize()
            ev["poly_div_linear in place"] = event_ms(torch, st, lambda: ctx.fr_poly_div_linear_device(d_io.data_ptr(), n, z, d_io.data_ptr(), stream=s),
                                                      a.steps, a.warmup)
            ev["running_product"] = event_ms(torch, st, lambda: ctx.fr_running_product_device(d_x.data_ptr(), d_out.data_ptr(), n, d_one.data_ptr(), stream=s),
                                             a.steps, a.warmup)
            must(("product", lg), got_ends(d_out) + words(d_one, 0, 1), ends(inc) + [total])
            ev["running_product exclusive"] = event_ms(torch, st, lambda: ctx.fr_running_product_device(d_x.data_ptr(), d_out.data_ptr(), n, None,
                                                                                                        mh.FR_SCAN_EXCLUSIVE, stream=s), a.steps, a.warmup)
            must(("exclusive", lg), got_ends(d_out), ends([1] + inc[:-1]))
            # what they are measured against
            ev["lincomb, one term"] = event_ms(torch, st, lambda: ctx.fr_lincomb_device(d_x.data_ptr(), d_out.data_ptr(), n, z, stream=s), a.steps, a.warmup)
            ev["ntt forward"] = event_ms(torch, st, lambda: ctx.ntt_device(d_out.data_ptr(), lg, stream=s), a.steps, a.warmup)
            with torch.cuda.stream(st):
                ev["hipMemcpy H2D"] = event_ms(torch, st, lambda: d_out[:n].copy_(h_pin[:n], non_blocking=True), a.steps, a.warmup)
                ev["hipMemcpy D2H"] = event_ms(torch, st, lambda: h_back[:n].copy_(d_out[:n], non_blocking=True), a.steps, a.warmup)
            d_xy = torch.zeros((n, 16), dtype=torch.int32, device=dev)
            d_inf = torch.zeros(n, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ctx.fixed_base_mul_device(fb.base_words(fb.GEN), d_x.data_ptr(), n, d_xy.data_ptr(), d_inf.data_ptr(), stream=s)
            st.synchronize()
            ctx.fr_poly_div_linear_device(d_x.data_ptr(), n, z, d_out.data_ptr(), stream=s)
            ev["G1 MSM (msm_bn254_g1_device)"] = event_ms(torch, st, lambda: ctx.msm_device(d_xy.data_ptr(), d_out.data_ptr(), n, d_inf.data_ptr(), stream=s),
                                                          max(3, a.steps // 4), 1)
            del d_xy, d_inf
            med = {k: statistics.median(v) for k, v in ev.items()}
            copies = med["hipMemcpy H2D"] + med["hipMemcpy D2H"]
            for name, ms in ev.items():
                extra = ""
                if name.startswith(("poly_", "running_")):
                    extra = "; %.2f x the one-term lincomb, %.2f x the forward transform; the two copies it replaces take %.2f x as long" % (
                        med[name] / med["lincomb, one term"], med[name] / med["ntt forward"], copies / med[name])
                say(f"2^{lg}: {name} {med_min(ms)} by events{extra}")
    say("device: %s" % torch.cuda.get_device_name(0))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
