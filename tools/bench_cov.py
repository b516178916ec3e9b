#!/usr/bin/env python3
"""Covariance / correlation matrix timing on device-resident data: Context.cov (corrla_cov_dev_*, the symmetric MFMA kernel)
against the route the library offered before it -- a centred (and, for the correlation, scaled) copy of x made with torch,
then Context.matmul(xc, xc, trans=True).  One process, interleaved rounds: each round times the new call and then the old
route once, each ended by a device synchronise; median of the rounds with min - max beside it, after warm-up.

Appends one JSON line per shape and mode to --out (default profiles/cov_corr.jsonl).  Also recorded, from shapes alone: the
flops the kernel actually does, n (n + BT) m multiply-adds (every tile pair on and above the diagonal, whole tiles), those
flops over the WHOLE call's time as a fraction of the exact-MFMA peak (whole_call_flops_over_exact_mfma_peak: moments,
product, finish and the Python call -- a lower bound of the kernel's own share, not that share), and the bytes the
product reads from x.
  --shapes small    tiny shapes, to rehearse the tool"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import corrla_rs_amd as cr  # noqa: E402

BT = 128
# exact MFMA peak of an MI355X: 256 CUs x 4 SIMDs x 64 FLOP / clk (v_mfma_f32_16x16x4_f32) at 2.4 GHz = 157.3 TF; the f64
# 16x16x4 form at half of it (78.6 TF, the public FP64 matrix figure)
PEAK_TFLOPS = {"float32": 157.3, "float64": 78.6}
SHAPES = {"full": ((1000000, 256, torch.float32), (100000, 1024, torch.float64), (16384, 4096, torch.float32),
                   (16384, 16384, torch.float32)),
          "small": ((20000, 256, torch.float32), (5000, 300, torch.float64))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cov_corr.jsonl"))
    ap.add_argument("--shapes", default="full", choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.rounds < 11 and args.shapes == "full":
        ap.error("at least 11 rounds")
    ctx = cr.Context(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for (m, n, dt) in SHAPES[args.shapes]:
        name = str(dt).split(".")[-1]
        esz = 4 if dt == torch.float32 else 8
        free, _ = torch.cuda.mem_get_info()
        need = m * n * esz * 2 + 3 * n * n * esz + (n // BT + 1) ** 2 // 2 * BT * BT * esz
        if need > 0.8 * free:
            print(json.dumps({"tool": "bench_cov", "m": m, "n": n, "dtype": name, "skipped": "needs %.1f GiB, %.1f free" % (need / 2 ** 30, free / 2 ** 30)}))
            continue
        x = torch.empty((m, n), dtype=dt, device="cuda")
        ctx.fill_normal(x, seed=11)
        x *= torch.linspace(3.0, 0.2, n, device="cuda", dtype=dt)
        x += torch.linspace(-2.0, 2.0, n, device="cuda", dtype=dt)
        for corr in (False, True):
            def new():
                return ctx.cov(x, correlation=corr)[0]

            def old():
                xc = x - x.mean(dim=0, keepdim=True)
                if corr:
                    xc = xc / x.std(dim=0, keepdim=True)
                return ctx.matmul(xc, xc, trans=True, beta=1.0 / (m - 1))

            for _ in range(args.warmup):
                new(), old()
            torch.cuda.synchronize()
            t_new, t_old = [], []
            for _ in range(args.rounds):
                for fn, ts in ((new, t_new), (old, t_old)):
                    t0 = time.perf_counter()
                    res = fn()
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    del res
            # same result, to the rounding of two different summation orders
            a, b = new(), old()
            scale = float(b.abs().max())
            diff = float((a - b).abs().max()) / scale
            del a, b

            def stats(ts):
                ts = sorted(ts)
                return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}
            nb = (n + BT - 1) // BT
            flops = 2.0 * (nb * (nb + 1) // 2) * BT * BT * m      # n (n + BT) m multiply-adds for n a multiple of BT
            sn, so = stats(t_new), stats(t_old)
            row = {"tool": "bench_cov", "m": m, "n": n, "dtype": name, "mode": "correlation" if corr else "covariance", "compute_units": cus,
                   "rounds": args.rounds, "warmup": args.warmup, "route": ctx.last_cov_route(), "cov": sn, "torch_copy_then_matmul": so,
                   "ratio_new_over_old": round(sn["median_ms"] / so["median_ms"], 4),
                   "spread_ms": round((sn["max_ms"] - sn["min_ms"]) + (so["max_ms"] - so["min_ms"]), 3),
                   "max_rel_diff_new_vs_old": diff,
                   "kernel_flops": flops, "whole_call_flops_over_exact_mfma_peak": round(flops / (sn["median_ms"] * 1e-3) / (PEAK_TFLOPS[name] * 1e12), 4),
                   "x_bytes_read_by_product": float(nb * m * n * esz),   # every column tile is staged once per pair it is in: nb times
                   "x_bytes_read_by_moments": float(m * n * esz)}
            print(json.dumps(row), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")
        del x
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
