#!/usr/bin/env python3
"""The dense LU solve and the RBF fit on it: wall times on the device against the routes a user had before.

  fit    RbfInterp.fit at n_s supports (dim 3, cubic kernel, linear tail, 8 right-hand sides), the supports on the device:
           lu     solver="lu": one Context.rbf_fit, the system never leaves the device
           pinv   solver="pinv": today's route -- K from the device, the block system and its SVD pseudo-inverse on the host
           numpy  numpy.linalg.solve of the same system on the host (the system from Context.rbf_system, its download
                  included), with the host's threads as the environment sets them
         The host routes grow as n^3 on the CPU: above --host-max supports they are not run and the row says so.
  solve  Context.solve against torch.linalg.solve on the same device and the same Gaussian system -- a comparison line only,
         nothing in the library calls it.

One process; every timing is a host clock around work that ends in a device synchronise, after warm-up; median of the rounds
with min - max beside it.  Appends one JSON line per row to --out (default profiles/lu_solve.jsonl).
  --only-lu N     nothing but `rounds` fits with solver="lu" at n_s = N (the run a kernel trace or a counter run wraps)
  --shapes small  tiny shapes, to rehearse the tool"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import corrla_rs_amd as cr  # noqa: E402

FIT_SHAPES = {"full": (2048, 8192, 16384), "small": (300, 700)}
SOLVE_SHAPES = {"full": ((2048, 8), (8192, 8), (16384, 8)), "small": ((200, 3), (700, 8))}
DIM, KERNEL, EPS, DEGREE, N_RHS = 3, 3, 0.0, 1, 8


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3), "rounds": len(ts)}


def timed(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        del res
    return stats(ts)


def points(n_s):
    gen = torch.Generator("cuda").manual_seed(n_s)
    x = torch.rand((n_s, DIM), dtype=torch.float64, device="cuda", generator=gen) * 2.0 - 1.0
    y = torch.randn((n_s, N_RHS), dtype=torch.float64, device="cuda", generator=gen)
    return x, y


def fit_with(ctx, solver, x, y):
    def run():
        m = cr.RbfInterp(KERNEL, EPS, DIM, DEGREE, ctx=ctx, solver=solver)
        m.fit(x, y)
        return m.coeffs
    return run


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(root, "profiles", "lu_solve.jsonl"))
    ap.add_argument("--shapes", default="full", choices=sorted(FIT_SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-max", type=int, default=8192, help="largest n_s at which the host routes are run (once each)")
    ap.add_argument("--only-lu", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_solve needs a GPU"
    ctx = cr.Context(0)
    threads = os.environ.get("OMP_NUM_THREADS")

    def emit(row):
        row.update(tool="bench_solve", omp_num_threads=threads)
        print(json.dumps(row), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")

    if args.only_lu:
        x, y = points(args.only_lu)
        s = timed(fit_with(ctx, "lu", x, y), args.rounds, args.warmup)
        print(json.dumps({"op": "rbf_fit_only", "n_s": args.only_lu, "lu": s, "info": ctx.last_solve_info}), flush=True)
        ctx.close()
        return

    for n_s in FIT_SHAPES[args.shapes]:
        x, y = points(n_s)
        n = n_s + DIM + 1
        row = {"op": "rbf_fit", "n_s": n_s, "n": n, "dim": DIM, "kernel": KERNEL, "poly_degree": DEGREE, "n_rhs": N_RHS}
        row["lu"] = timed(fit_with(ctx, "lu", x, y), args.rounds, args.warmup)
        row["lu_info"] = dict(ctx.last_solve_info, route=ctx.last_solve_route)
        row["lu_gflops"] = round((2.0 / 3.0) * n ** 3 / (row["lu"]["median_ms"] * 1e-3) / 1e9, 1)
        c_lu = fit_with(ctx, "lu", x, y)()
        if n_s <= args.host_max:
            row["pinv"] = timed(fit_with(ctx, "pinv", x, y), 1, 0)

            def host_solve():
                m = ctx.rbf_system(x, KERNEL, EPS, poly_degree=DEGREE).cpu().numpy()
                b = np.vstack([y.cpu().numpy(), np.zeros((n - n_s, N_RHS))])
                return np.linalg.solve(m, b)
            row["numpy_solve"] = timed(host_solve, 1, 0)
            c_np = host_solve()
            row["max_rel_diff_lu_vs_numpy"] = float(np.abs(c_lu.cpu().numpy() - c_np).max() / np.abs(c_np).max())
            row["ratio_lu_over_pinv"] = round(row["lu"]["median_ms"] / row["pinv"]["median_ms"], 5)
            row["ratio_lu_over_numpy"] = round(row["lu"]["median_ms"] / row["numpy_solve"]["median_ms"], 5)
        else:
            row["pinv"] = row["numpy_solve"] = "not measured: host routes are run up to --host-max supports"
        emit(row)
        del x, y, c_lu
        torch.cuda.empty_cache()

    for n, n_rhs in SOLVE_SHAPES[args.shapes]:
        gen = torch.Generator("cuda").manual_seed(n)
        a = torch.randn((n, n), dtype=torch.float64, device="cuda", generator=gen)
        b = torch.randn((n, n_rhs), dtype=torch.float64, device="cuda", generator=gen)
        row = {"op": "solve", "n": n, "n_rhs": n_rhs, "matrix": "gaussian"}
        row["context_solve"] = timed(lambda: ctx.solve(a, b), args.rounds, args.warmup)
        row["route"] = ctx.last_solve_route
        row["torch_linalg_solve"] = timed(lambda: torch.linalg.solve(a, b), args.rounds, args.warmup)
        xa, xb = ctx.solve(a, b), torch.linalg.solve(a, b)
        row["max_rel_diff"] = float((xa - xb).abs().max() / xb.abs().max())
        row["ratio_context_over_torch"] = round(row["context_solve"]["median_ms"] / row["torch_linalg_solve"]["median_ms"], 4)
        row["context_gflops"] = round((2.0 / 3.0) * n ** 3 / (row["context_solve"]["median_ms"] * 1e-3) / 1e9, 1)
        emit(row)
        del a, b, xa, xb
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
