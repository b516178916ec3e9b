#!/usr/bin/env python3
"""Quadratic response surfaces on device-resident samples: Context.polyfit_gram (corrla_polyfit_gram_dev_*: the columns of
the Vandermonde matrix formed in registers and fed to the f64 MFMAs, never stored) and Context.poly_eval (xt^T C xt, with
the analytic gradient) against the route a user had on the device before them:
  fit   V = [x, x_a x_b (a <= b), 1] built with torch on the device, then V.T @ V and V.T @ y in float64
  eval  V @ c
both chunked over the samples where the m x p temporary would not fit a chunk; the chunk count is in the row.  The old
route works on x as it is; the new call is timed with its default normalisation (which adds the column pass) and without.
One process, interleaved rounds: each round times the new calls and then the old route once, each ended by a device
synchronise; median of the rounds with min - max beside it, after warm-up.

Appends one JSON line per shape and operation to --out (default profiles/polyfit.jsonl): the timings, their ratio, the
achieved f64 TFLOP/s of the fit counted as m (p + r)^2 flops (one multiply-add per sample and entry on or above the
diagonal, the work a symmetric product needs; the old route's full product is counted as twice that) beside the f64 MFMA
ceiling DESIGN states, and the largest relative difference of the two results (a plausibility figure:
tests/test_gpu_polyfit.py holds the bounds).
  --shapes small    tiny shapes, to rehearse the tool"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import corrla_rs_amd as cr  # noqa: E402

F64 = torch.float64
F64_MFMA_PEAK_TFLOPS = 78.6   # DESIGN: the dense f64 matrix ceiling of the MI355X
# (m, k, r)
SHAPES = {"full": ((10 ** 6, 16, 1), (10 ** 6, 64, 1), (10 ** 5, 128, 1)),
          "small": ((5000, 4, 1), (3000, 16, 2), (2000, 40, 1))}
CHUNK_BYTES = 2 << 30   # of one m-chunk of the old route's Vandermonde matrix


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}


def vandermonde(x, ia, ib):
    return torch.cat([x, x[:, ia] * x[:, ib], torch.ones((x.shape[0], 1), dtype=x.dtype, device=x.device)], dim=1)


def timed(fns, rounds, warmup):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for fn, t in zip(fns, ts):
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
            del res
    return [stats(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "polyfit.jsonl"))
    ap.add_argument("--shapes", default="full", choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.rounds < 11 and args.shapes == "full":
        ap.error("at least 11 rounds")
    assert torch.cuda.is_available(), "bench_polyfit needs a GPU"
    ctx = cr.Context(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for (m, k, r) in SHAPES[args.shapes]:
        gen = torch.Generator("cuda").manual_seed(5)
        x = torch.rand((m, k), dtype=F64, device="cuda", generator=gen)
        y = torch.randn((m, r), dtype=F64, device="cuda", generator=gen)
        ia, ib = torch.triu_indices(k, k, device="cuda")
        p = k + k * (k + 1) // 2 + 1
        c = torch.randn((p, r), dtype=F64, device="cuda", generator=gen)
        rows = max(1, min(m, CHUNK_BYTES // (p * 8)))
        n_chunks = (m + rows - 1) // rows

        def fit_new():
            return ctx.polyfit_gram(x, y)

        def fit_new_raw():
            return ctx.polyfit_gram(x, y, normalize=False)

        def fit_old():
            vtv = torch.zeros((p, p), dtype=F64, device="cuda")
            vty = torch.zeros((p, r), dtype=F64, device="cuda")
            for i0 in range(0, m, rows):
                v = vandermonde(x[i0:i0 + rows], ia, ib)
                vtv += v.T @ v
                vty += v.T @ y[i0:i0 + rows]
                del v
            return vtv, vty

        def eval_new():
            return ctx.poly_eval(x, c)

        def eval_new_jac():
            return ctx.poly_eval(x, c, jac=True)

        def eval_old():
            out = torch.empty((m, r), dtype=F64, device="cuda")
            for i0 in range(0, m, rows):
                out[i0:i0 + rows] = vandermonde(x[i0:i0 + rows], ia, ib) @ c
            return out

        common = {"tool": "bench_polyfit", "m": m, "k": k, "r": r, "p": p, "degree": 2, "dtype": "float64", "compute_units": cus,
                  "rounds": args.rounds, "warmup": args.warmup, "old_chunks": n_chunks, "old_chunk_rows": rows}
        s_new, s_raw, s_old = timed((fit_new, fit_new_raw, fit_old), args.rounds, args.warmup)
        g = fit_new_raw()[0]
        vtv, vty = fit_old()
        diff = max(float((g[:p, :p] - vtv).abs().max() / vtv.abs().max()), float((g[:p, p:] - vty).abs().max() / vty.abs().max()))
        del g, vtv, vty
        flops = float(m) * (p + r) ** 2
        row = dict(common, op="polyfit_gram", new=s_new, new_no_normalize=s_raw, old=s_old,
                   old_route="torch: V on the device, V.T @ V and V.T @ y in float64",
                   ratio_new_over_old=round(s_new["median_ms"] / s_old["median_ms"], 4),
                   ratio_no_normalize_over_old=round(s_raw["median_ms"] / s_old["median_ms"], 4),
                   spread_over_old_median=round(((s_new["max_ms"] - s_new["min_ms"]) + (s_old["max_ms"] - s_old["min_ms"])) / s_old["median_ms"], 4),
                   f64_tflops_new=round(flops / (s_new["median_ms"] * 1e-3) / 1e12, 2),
                   f64_tflops_old_full_product=round(2.0 * flops / (s_old["median_ms"] * 1e-3) / 1e12, 2),
                   f64_mfma_ceiling_tflops=F64_MFMA_PEAK_TFLOPS, max_rel_diff_new_vs_old=diff)
        print(json.dumps(row), flush=True)
        rows_out = [row]
        e_new, e_jac, e_old = timed((eval_new, eval_new_jac, eval_old), args.rounds, args.warmup)
        a, b = eval_new(), eval_old()
        diff = float((a - b).abs().max() / b.abs().max())
        del a, b
        row = dict(common, op="poly_eval", new=e_new, new_with_jac=e_jac, old=e_old, old_route="torch: V on the device, V @ c",
                   ratio_new_over_old=round(e_new["median_ms"] / e_old["median_ms"], 4),
                   ratio_with_jac_over_old=round(e_jac["median_ms"] / e_old["median_ms"], 4),
                   spread_over_old_median=round(((e_new["max_ms"] - e_new["min_ms"]) + (e_old["max_ms"] - e_old["min_ms"])) / e_old["median_ms"], 4),
                   f64_tflops_new=round(2.0 * m * r * (k + 1) ** 2 / (e_new["median_ms"] * 1e-3) / 1e12, 3),
                   f64_mfma_ceiling_tflops=F64_MFMA_PEAK_TFLOPS, max_rel_diff_new_vs_old=diff)
        print(json.dumps(row), flush=True)
        rows_out.append(row)
        with open(args.out, "a") as f:
            for row in rows_out:
                f.write(json.dumps(row) + "\n")
        del x, y, c
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
