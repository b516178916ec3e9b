#!/usr/bin/env python3
"""Multivariate normal rows and sandwich variances on the device: Context.mvn_sample (corrla_mvn_sample_dev_*: the normals of
a row tile generated into LDS and multiplied there) and Context.sandwich_diag (corrla_sandwich_diag_dev_*) against the routes
a user had before them.

  sample    n rows of N(mu, F F^T), F (d, r), against
              (a) unfused: this package's own Context.fill_normal into an (n, r) tensor, column-major as the back-projection
                  kernel reads it, then Context.pca_inverse_transform -- the SAME stream, so the largest difference of the two
                  results is in the row (a plausibility figure; tests/test_gpu_mvn.py holds the bounds);
              (b) torch: torch.randn(n, r) @ F.T + mu -- another stream, for time only.
  sandwich  v_i = j_i^T C j_i against torch's ((J @ C) * J).sum(1), which writes and reads an (m, d) temporary.

One process, interleaved rounds: each round times every arm once, each call ended by a device synchronise (the library runs on
its own stream, so the calls are bracketed by host clocks around synchronising calls, as in the other tools; a call is
milliseconds long); median of the rounds with min - max beside it, after warm-up (which also ramps the clocks).  Appends one
JSON line per row to --out (default profiles/mvn.jsonl) with the timings, the ratios new / old, the output bytes per second
and the normals per second of the new call.
  --shapes small    tiny shapes, to rehearse the tool
  --shapes boundary full-rank widths between the measured shapes, where the fused route stops paying
  --only sample,sandwich    rows to run (a counter run of its own takes one kind, --rounds 1 --warmup 0 --no-old)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import corrla_rs_amd as cr  # noqa: E402

F32, F64 = torch.float32, torch.float64
# (n, d, r, dtype, lower)
SAMPLE = {"full": tuple((10 ** 6, d, d, dt, False) for d in (16, 64, 256) for dt in (F32, F64))
          + tuple((10 ** 6, 256, 32, dt, False) for dt in (F32, F64)) + tuple((10 ** 6, 256, 256, dt, True) for dt in (F32, F64)),
          # full rank around the widths where the fused route stops paying (the fused / staged boundary)
          "boundary": tuple((10 ** 6, r, r, F32, False) for r in (128, 192, 288)) + tuple((10 ** 6, r, r, F64, False) for r in (96, 128, 144)),
          "small": ((5000, 16, 16, F32, False), (5000, 70, 9, F64, False), (3000, 160, 160, F64, True))}
# (m, d, dtype)
SANDWICH = {"full": tuple((m, d, dt) for (m, d) in ((10 ** 6, 64), (10 ** 5, 512)) for dt in (F32, F64)),
            "boundary": (), "small": ((5000, 64, F32), (3000, 200, F64))}


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3), "rounds": len(ts)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mvn.jsonl"))
    ap.add_argument("--shapes", default="full", choices=sorted(SAMPLE))
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="sample,sandwich")
    ap.add_argument("--no-old", action="store_true", help="time the new calls alone (a counter run)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mvn needs a GPU"
    ctx = cr.Context(0)
    only = args.only.split(",")
    rows = []
    for (n, d, r, dt, lower) in (SAMPLE[args.shapes] if "sample" in only else ()):
        name = str(dt).split(".")[-1]
        esz = 4 if dt == F32 else 8
        gen = torch.Generator("cuda").manual_seed(5)
        f = torch.randn((d, r), dtype=F64, device="cuda", generator=gen) / np.sqrt(r)
        if lower:
            f = torch.tril(f)
        f = f.to(dt)
        mu = torch.randn(d, dtype=F64, device="cuda", generator=gen).to(dt)
        out = torch.empty((n, d), dtype=dt, device="cuda")
        zt = torch.empty((r, n), dtype=dt, device="cuda").t()   # (n, r) column-major: what pca_inverse_transform reads in place
        comps = f.t().contiguous()                              # (r, d): x = z @ comps + mu

        def new():
            return ctx.mvn_sample(n, f, mu, seed=7, lower=lower, out=out)

        def unfused():
            ctx.fill_normal(zt, 7, row0=0, global_cols=r)
            return ctx.pca_inverse_transform(zt, mu, comps)

        def torch_route():
            return torch.randn((n, r), dtype=dt, device="cuda") @ f.t() + mu

        arms = [("new", new)] + ([] if args.no_old else [("unfused", unfused), ("torch", torch_route)])
        ts = {k: [] for k, _ in arms}
        diff = None
        for it in range(args.warmup + args.rounds):
            res = {}
            for k, fn in arms:
                t, res[k] = timed(fn)
                if it >= args.warmup:
                    ts[k].append(t)
            if diff is None and "unfused" in res:
                diff = float((res["new"] - res["unfused"]).abs().max())
            del res
        new()
        row = {"op": "mvn_sample", "n": n, "d": d, "r": r, "dtype": name, "lower": lower, "route": ctx.last_mvn_route(),
               "new": stats(ts["new"])}
        med = row["new"]["median_ms"]
        row["out_GBps"] = round(n * d * esz / med / 1e6, 1)
        row["normals_per_s"] = float(f"{n * r / med * 1e3:.4g}")
        if not args.no_old:
            row["unfused"], row["torch"] = stats(ts["unfused"]), stats(ts["torch"])
            row["new_over_unfused"] = round(med / row["unfused"]["median_ms"], 3)
            row["new_over_torch"] = round(med / row["torch"]["median_ms"], 3)
            row["max_abs_diff_vs_unfused"] = diff
        rows.append(row)
        print(json.dumps(row), flush=True)
        del out, zt
    for (m, d, dt) in (SANDWICH[args.shapes] if "sandwich" in only else ()):
        name = str(dt).split(".")[-1]
        gen = torch.Generator("cuda").manual_seed(6)
        j = torch.randn((m, d), dtype=F64, device="cuda", generator=gen).to(dt)
        a = torch.randn((d, d), dtype=F64, device="cuda", generator=gen)
        c = (a @ a.t() / d).to(dt)
        arms = [("new", lambda: ctx.sandwich_diag(j, c))] + ([] if args.no_old else [("torch", lambda: ((j @ c) * j).sum(1))])
        ts = {k: [] for k, _ in arms}
        diff = None
        for it in range(args.warmup + args.rounds):
            res = {}
            for k, fn in arms:
                t, res[k] = timed(fn)
                if it >= args.warmup:
                    ts[k].append(t)
            if diff is None and "torch" in res:
                diff = float(((res["new"] - res["torch"]).abs() / res["torch"].abs().clamp_min(1e-30)).max())
        row = {"op": "sandwich_diag", "m": m, "d": d, "dtype": name, "new": stats(ts["new"])}
        med = row["new"]["median_ms"]
        row["TFLOPs"] = round(2.0 * m * d * d / med / 1e9, 2)
        if not args.no_old:
            row["torch"] = stats(ts["torch"])
            row["new_over_torch"] = round(med / row["torch"]["median_ms"], 3)
            row["max_rel_diff_vs_torch"] = diff
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
