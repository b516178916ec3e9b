#!/usr/bin/env python3
"""Fitted PCA model on device-resident data: Context.pca_transform / pca_inverse_transform (corrla_pca_transform_dev_*,
corrla_pca_inverse_dev_*, the back-projection MFMA kernel) against what the library offered before them, each built from
torch elementwise passes and Context.matmul:
  transform   (x - mu) / sigma as a torch copy, then Context.matmul(copy, V^T)
  inverse     Context.matmul(scores, V), then torch * sigma + mu
  residuals   transform as above, that reconstruction, then a torch row norm of the standardised difference
(where Context.matmul refuses a product -- the reconstruction has n columns on its skinny side -- torch.matmul stands in and
the row says so: "old_product").  One process, interleaved rounds: each round times the new call and then the old route
once, each ended by a device synchronise; median of the rounds with min - max beside it, after warm-up.

The model is not a fit (the timing does not depend on it): mu and sigma are the column moments, V is k orthonormal rows.
Appends one JSON line per shape and operation to --out (default profiles/pca_transform.jsonl).  Also recorded: the bytes of
one m x n pass over the new call's time (inverse: the one write; residuals: the one read, over the time the residuals add to
the transform), as achieved TB/s.
  --shapes small    tiny shapes, to rehearse the tool
  --center fused    the new transform with that centring instead of the library's default;  --ops transform,residuals"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import corrla_rs_amd as cr  # noqa: E402

SHAPES = {"full": ((1000000, 512, 64, torch.float32), (16384, 16384, 32, torch.float32), (65536, 4096, 256, torch.float64)),
          "small": ((20000, 256, 16, torch.float32), (5000, 300, 40, torch.float64))}


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pca_transform.jsonl"))
    ap.add_argument("--shapes", default="full", choices=sorted(SHAPES))
    ap.add_argument("--center", default=None, choices=("fused", "copy"), help="centring of the new transform (default: the library's)")
    ap.add_argument("--ops", default="transform,inverse,residuals", help="comma-separated subset of the three operations")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.rounds < 11 and args.shapes == "full":
        ap.error("at least 11 rounds")
    ctx = cr.Context(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for (m, n, k, dt) in SHAPES[args.shapes]:
        name = str(dt).split(".")[-1]
        esz = 4 if dt == torch.float32 else 8
        free, _ = torch.cuda.mem_get_info()
        need = 6 * m * n * esz
        if need > 0.8 * free:
            print(json.dumps({"tool": "bench_pca_transform", "m": m, "n": n, "k": k, "dtype": name,
                              "skipped": "needs %.1f GiB, %.1f free" % (need / 2 ** 30, free / 2 ** 30)}))
            continue
        x = torch.empty((m, n), dtype=dt, device="cuda")
        ctx.fill_normal(x, seed=11)
        x *= torch.linspace(3.0, 0.2, n, device="cuda", dtype=dt)
        x += torch.linspace(-2.0, 2.0, n, device="cuda", dtype=dt)
        mu, sd = x.mean(dim=0, keepdim=True), x.std(dim=0, keepdim=True)
        v = torch.linalg.qr(torch.randn((n, k), dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(3)))[0]
        v = v.t().contiguous().to(dt)                                  # (k, n)
        vt = v.t().contiguous()                                        # (n, k)
        scores = ctx.pca_transform(x, mu, v, sd, center=args.center)

        product = {"name": "Context.matmul"}

        def old_product(a, b):
            """a @ b by the library's product hook, or by torch where the hook refuses the shape"""
            if product["name"] == "Context.matmul":
                try:
                    return ctx.matmul(a, b)
                except Exception as e:  # noqa: BLE001 -- whatever the hook raises for a shape outside its domain
                    product["name"] = "torch.matmul (Context.matmul: %s)" % str(e)[:80]
            return a @ b

        def new_transform():
            return ctx.pca_transform(x, mu, v, sd, center=args.center)

        def old_transform():
            return ctx.matmul((x - mu) / sd, vt)

        def new_inverse():
            return ctx.pca_inverse_transform(scores, mu, v, sd)

        def old_inverse():
            return old_product(scores.contiguous(), v) * sd + mu

        def new_resid():
            return ctx.pca_transform(x, mu, v, sd, residuals=True, center=args.center)

        def old_resid():
            t = old_transform()
            xh = old_product(t.contiguous(), v) * sd + mu
            return t, ((x - xh) / sd).square().sum(dim=1)

        medians = {}
        for op, new, old in (("transform", new_transform, old_transform), ("inverse", new_inverse, old_inverse),
                             ("residuals", new_resid, old_resid)):
            if op not in args.ops.split(","):
                continue
            product["name"] = "Context.matmul"
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
            a, b = new(), old()
            a, b = (a[-1], b[-1]) if isinstance(a, tuple) else (a, b)
            diff = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)
            del a, b
            sn, so = stats(t_new), stats(t_old)
            medians[op] = sn["median_ms"]
            row = {"tool": "bench_pca_transform", "op": op, "m": m, "n": n, "k": k, "dtype": name, "compute_units": cus,
                   "rounds": args.rounds, "warmup": args.warmup, "center_arg": args.center, "centring": ctx.last_pca_apply_centring() if op != "inverse" else None,
                   "route": ctx.last_pca_apply_route(), "new": sn, "old": so, "old_product": product["name"] if op != "transform" else "Context.matmul",
                   "ratio_new_over_old": round(sn["median_ms"] / so["median_ms"], 4),
                   "spread_ms": round((sn["max_ms"] - sn["min_ms"]) + (so["max_ms"] - so["min_ms"]), 3),
                   "spread_over_old_median": round(((sn["max_ms"] - sn["min_ms"]) + (so["max_ms"] - so["min_ms"])) / so["median_ms"], 4),
                   "max_rel_diff_new_vs_old": diff, "mn_pass_bytes": float(m * n * esz)}
            if op == "inverse":
                row["mn_pass_tb_per_s"] = round(m * n * esz / (sn["median_ms"] * 1e-3) / 1e12, 3)
            if op == "residuals" and "transform" in medians:
                added = sn["median_ms"] - medians["transform"]
                row["added_to_transform_ms"] = round(added, 3)
                row["mn_pass_tb_per_s"] = round(m * n * esz / (max(added, 1e-6) * 1e-3) / 1e12, 3)
            print(json.dumps(row), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")
        del x, scores
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
