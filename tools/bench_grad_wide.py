#!/usr/bin/env python3
"""Timing of the gradient stage's wide kernels (grad_wide_kernels.hpp) on device-resident data, two shapes no limited
kernel serves:
  * 1e5 points x 256 features, order 1, 300 neighbours, every point a query;
  * 2e4 points x 64 features, order 2, 2200 neighbours, 256 queries.
Prints one JSON line per shape: the scan and fit times of corrla_timings (knn_ms, fit_ms; second of two calls), the
achieved f64 rate of the scan (3 flops per pair and dimension) and the oracle's time per query on a small sample.
usage: bench_grad_wide.py [out.jsonl]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import corrla_rs_amd as cr  # noqa: E402
from oracle import active_ss_oracle as aso  # noqa: E402  (reported baseline only)

SHAPES = [  # (n_pts, k, order, n_nbrs, n_queries, oracle sample)
    (100000, 256, 1, 300, 100000, 8),
    (20000, 64, 2, 2200, 256, 2),
]
ctx = cr.Context(0)
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
for n, k, order, n_nbrs, nq, n_oracle in SHAPES:
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((n, k), dtype=torch.float64, device="cuda", generator=g)
    w = torch.linspace(1.0, 0.05, k, dtype=torch.float64, device="cuda")
    y = torch.sin(x @ w * 0.2) + 0.05 * ((x * w) ** 2).sum(dim=1)
    xq = x[:nq]
    times = []
    for _ in range(2):   # the first call loads the code object and sizes the workspaces
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gm, nreg = ctx.grad_mat(x, y, order, n_nbrs, xq)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t = ctx.timings()
    xs, ys = x.cpu().numpy(), y.cpu().numpy()
    est = aso.PolyGradientEstimator(xs, ys, order, n_nbrs)
    est.exact_quad_gradient = True
    t0 = time.perf_counter()
    go = aso.create_grad_mat(est, xs[:n_oracle])
    t_cpu = (time.perf_counter() - t0) / n_oracle
    dev = float(np.max(np.abs(gm[:, :n_oracle].cpu().numpy() - go)) / np.abs(go).max())
    rec = {"shape": "%d x %d, order %d, %d neighbours, %d queries" % (n, k, order, n_nbrs, nq),
           "knn_ms": round(t["knn_ms"], 2), "fit_ms": round(t["fit_ms"], 2), "wall_s": round(times[-1], 3),
           "scan_tflops": round(3.0 * n * nq * k / (t["knn_ms"] * 1e-3) / 1e12, 2),
           "n_regularised": nreg, "oracle_s_per_query": round(t_cpu, 4), "oracle_queries": n_oracle,
           "max_rel_dev_vs_oracle": dev}
    print(json.dumps(rec), flush=True)
    if out:
        out.write(json.dumps(rec) + "\n")
        out.flush()
