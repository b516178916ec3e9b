#!/usr/bin/env python3
"""RBF interpolation on device-resident points: Context.rbf_apply (corrla_rbf_apply_dev_*: the kernel matrix formed in
registers and fed to the exact MFMAs, never stored) against the route a user had on the device before it:
  torch.cdist(xq, xs), the elementwise phi, then Context.matmul(Phi, W)
chunked over the queries where the n_q x n_s temporary (and cdist's own workspace) would not fit; the chunk count is in the
row.  One process, interleaved rounds: each round times the new call and then the old route once, each ended by a device
synchronise; median of the rounds with min - max beside it, after warm-up.

Appends one JSON line per shape to --out (default profiles/rbf_interp.jsonl): the two timings, their ratio, the (query,
support) pairs per second of the new call and the largest relative difference of the two results (cdist forms distances
its own way, so this is a plausibility figure, not a bound -- tests/test_gpu_rbf.py holds the bounds).
  --shapes small    tiny shapes, to rehearse the tool"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import corrla_rs_amd as cr  # noqa: E402

F32, F64 = torch.float32, torch.float64
# (n_q, n_s, dim, n_rhs, dtype, kernel, eps)
SHAPES = {"full": tuple((10 ** 6, 4096, 3, n_rhs, dt, kernel, eps) for dt in (F64, F32) for n_rhs in (1, 32) for kernel, eps in ((1, 0.0), (4, 0.5)))
          + ((10 ** 5, 16384, 16, 32, F64, 1, 0.0), (10 ** 5, 16384, 16, 32, F64, 4, 0.2),
             (10 ** 5, 16384, 16, 32, F32, 1, 0.0), (10 ** 5, 16384, 16, 32, F32, 4, 0.2)),
          "small": ((3000, 500, 3, 1, F64, 1, 0.0), (3000, 500, 3, 32, F32, 4, 0.5), (2000, 700, 16, 32, F64, 4, 0.2))}
CHUNK_BYTES = 2 << 30   # of one n_q-chunk of the old route's kernel matrix


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}


def phi(kernel, r, eps):
    if kernel == 1:
        return r
    if kernel == 2:
        return torch.sqrt(1.0 + (eps * r) ** 2)
    if kernel == 3:
        return r * r * r
    return torch.exp(-((eps * r) ** 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rbf_interp.jsonl"))
    ap.add_argument("--shapes", default="full", choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.rounds < 11 and args.shapes == "full":
        ap.error("at least 11 rounds")
    assert torch.cuda.is_available(), "bench_rbf needs a GPU"
    ctx = cr.Context(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for (n_q, n_s, dim, n_rhs, dt, kernel, eps) in SHAPES[args.shapes]:
        name = str(dt).split(".")[-1]
        esz = 4 if dt == F32 else 8
        gen = torch.Generator("cuda").manual_seed(5)
        xq = torch.rand((n_q, dim), dtype=dt, device="cuda", generator=gen)
        xs = torch.rand((n_s, dim), dtype=dt, device="cuda", generator=gen)
        w = torch.randn((n_s, n_rhs), dtype=dt, device="cuda", generator=gen)
        rows = max(1, min(n_q, CHUNK_BYTES // (n_s * esz)))
        n_chunks = (n_q + rows - 1) // rows

        def new():
            return ctx.rbf_apply(xq, xs, w, kernel, eps)

        def old():
            out = torch.empty((n_q, n_rhs), dtype=dt, device="cuda")
            for i0 in range(0, n_q, rows):
                k = phi(kernel, torch.cdist(xq[i0:i0 + rows], xs), eps)
                out[i0:i0 + rows] = ctx.matmul(k, w)
                del k
            return out

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
        diff = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)
        del a, b
        sn, so = stats(t_new), stats(t_old)
        row = {"tool": "bench_rbf", "op": "rbf_apply", "n_q": n_q, "n_s": n_s, "dim": dim, "n_rhs": n_rhs, "dtype": name, "kernel": kernel,
               "eps": eps, "compute_units": cus, "rounds": args.rounds, "warmup": args.warmup, "new": sn, "old": so,
               "old_route": "torch.cdist + elementwise phi + Context.matmul", "old_chunks": n_chunks, "old_chunk_rows": rows,
               "ratio_new_over_old": round(sn["median_ms"] / so["median_ms"], 4),
               "spread_over_old_median": round(((sn["max_ms"] - sn["min_ms"]) + (so["max_ms"] - so["min_ms"])) / so["median_ms"], 4),
               "pairs_per_s": round(n_q * n_s / (sn["median_ms"] * 1e-3), 1), "max_rel_diff_new_vs_old": diff}
        print(json.dumps(row), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        del xq, xs, w
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
