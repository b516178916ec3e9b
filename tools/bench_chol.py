#!/usr/bin/env python3
"""The dense Cholesky solve and the covariance factor on it: wall times on the device against the routes a user had before.

  solve   at n = 2048, 8192 and 16384 with 8 right-hand sides, one symmetric positive definite matrix (a Gram matrix plus
          the identity) on the device:
            chol    Context.solve(a, b, assume="pos")
            lu      Context.solve(a, b): the LU route on the same matrix
            torch   torch.linalg.cholesky followed by torch.cholesky_solve
  factor  at d = 2048 and 8192, the covariance on the device:
            device  mvn_factor(cov, device=True)
            host    mvn_factor(cov): the download, numpy's Cholesky and nothing else (the host's threads as the
                    environment sets them)

One process; every timing is a host clock around work that ends in a device synchronise, after warm-up; median of the rounds
with min - max beside it.  Appends one JSON line per row to --out (default profiles/chol_solve.jsonl).
  --only-chol N   nothing but `rounds` solves with assume="pos" at n = N (the run a kernel trace wraps)
  --shapes small  tiny shapes, to rehearse the tool"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import corrla_rs_amd as cr  # noqa: E402

SOLVE_SHAPES = {"full": (2048, 8192, 16384), "small": (200, 700)}
FACTOR_SHAPES = {"full": (2048, 8192), "small": (200, 700)}
N_RHS = 8


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


def spd(n):
    """G G^T / n + I with G Gaussian: condition about 5"""
    gen = torch.Generator("cuda").manual_seed(n)
    g = torch.randn((n, n), dtype=torch.float64, device="cuda", generator=gen)
    a = g @ g.T / n
    a = 0.5 * (a + a.T) + torch.eye(n, dtype=torch.float64, device="cuda")
    b = torch.randn((n, N_RHS), dtype=torch.float64, device="cuda", generator=gen)
    del g
    return a, b


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(root, "profiles", "chol_solve.jsonl"))
    ap.add_argument("--shapes", default="full", choices=sorted(SOLVE_SHAPES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only-chol", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_chol needs a GPU"
    ctx = cr.Context(0)
    threads = os.environ.get("OMP_NUM_THREADS")

    def emit(row):
        row.update(tool="bench_chol", omp_num_threads=threads)
        print(json.dumps(row), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")

    if args.only_chol:
        a, b = spd(args.only_chol)
        s = timed(lambda: ctx.solve(a, b, assume="pos"), args.rounds, args.warmup)
        print(json.dumps({"op": "chol_solve_only", "n": args.only_chol, "chol": s, "info": ctx.last_chol_info}), flush=True)
        ctx.close()
        return

    for n in SOLVE_SHAPES[args.shapes]:
        a, b = spd(n)
        row = {"op": "spd_solve", "n": n, "n_rhs": N_RHS, "matrix": "gram + identity"}
        row["chol"] = timed(lambda: ctx.solve(a, b, assume="pos"), args.rounds, args.warmup)
        row["chol_info"] = dict(ctx.last_chol_info, route=ctx.last_chol_route)
        row["lu"] = timed(lambda: ctx.solve(a, b), args.rounds, args.warmup)
        row["torch_cholesky_solve"] = timed(lambda: torch.cholesky_solve(b, torch.linalg.cholesky(a)), args.rounds, args.warmup)
        xc, xl, xt = ctx.solve(a, b, assume="pos"), ctx.solve(a, b), torch.cholesky_solve(b, torch.linalg.cholesky(a))
        row["max_rel_diff_chol_vs_lu"] = float((xc - xl).abs().max() / xl.abs().max())
        row["max_rel_diff_chol_vs_torch"] = float((xc - xt).abs().max() / xt.abs().max())
        ctx.solve(a, b, assume="pos")
        ld = 2.0 * float(torch.log(torch.diagonal(torch.linalg.cholesky(a))).sum())
        row["logdet_rel_diff_vs_torch"] = abs(ctx.last_chol_info["logdet"] - ld) / abs(ld)
        row["ratio_chol_over_lu"] = round(row["chol"]["median_ms"] / row["lu"]["median_ms"], 4)
        row["ratio_chol_over_torch"] = round(row["chol"]["median_ms"] / row["torch_cholesky_solve"]["median_ms"], 4)
        row["chol_gflops"] = round(n ** 3 / 3.0 / (row["chol"]["median_ms"] * 1e-3) / 1e9, 1)
        emit(row)
        del a, b, xc, xl, xt
        torch.cuda.empty_cache()

    for d in FACTOR_SHAPES[args.shapes]:
        cov, _ = spd(d)
        row = {"op": "mvn_factor", "d": d, "matrix": "gram + identity"}
        row["device"] = timed(lambda: cr.mvn_factor(cov, device=True, ctx=ctx)[0], args.rounds, args.warmup)
        row["host"] = timed(lambda: cr.mvn_factor(cov)[0], min(args.rounds, 3), 0)
        fd, fh = cr.mvn_factor(cov, device=True, ctx=ctx)[0], cr.mvn_factor(cov)[0]
        row["max_rel_diff"] = float((fd.cpu() - torch.as_tensor(fh)).abs().max() / abs(fh).max())
        row["ratio_device_over_host"] = round(row["device"]["median_ms"] / row["host"]["median_ms"], 5)
        emit(row)
        del cov, fd, fh
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
