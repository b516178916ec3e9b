#!/usr/bin/env python3
"""Gaussian kernel density estimates on device-resident samples: Context.kde_eval / kde_nll (corrla_kde_*_dev_*: fused
pairwise sums, the n x n_s matrix never stored) and a whole KdeRv.est_bandwidth against the route a user has in torch on
the same device: chunked broadcasting x[:, None] - s[None, :], then exp / special.erfc / logsumexp and the reduction, the
chunk of points sized to a fixed workspace (the chunk count is in the row).  The comparator is torch, not the code under test.

One process, interleaved rounds: each round times the new call and then the torch route once, each ended by a device
synchronise; median of the rounds with min - max beside it, after warm-up (which also ramps the clocks).  Appends one JSON
line per row to --out (default profiles/kde.jsonl): the two timings, their ratio, the (point, support) pairs -- times
bandwidths for the likelihood -- per second of the new call and the largest difference of the two results (a plausibility
figure, not a bound -- tests/test_gpu_kde.py holds the bounds).  The torch arm of the est_bandwidth row runs the same search
over torch likelihoods; it takes --est-old-rounds rounds (default 3: it is some twenty times slower), as its row says.
  --shapes small    tiny shapes, to rehearse the tool"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import corrla_rs_amd as cr  # noqa: E402
from corrla_rs_amd.callers import KdeRv  # noqa: E402

F32, F64 = torch.float32, torch.float64
# (op, n_points, n_supports, n_h, dtype)
SHAPES = {"full": tuple((op, 10 ** 6, 10 ** 5, 1, dt) for op in ("pdf", "cdf", "logpdf") for dt in (F32, F64))
          + tuple(("nll", 10 ** 5, 10 ** 5, n_h, dt) for n_h in (1, 64) for dt in (F32, F64))
          + (("est_bandwidth", 60000, 140000, 64, F32), ("est_bandwidth", 60000, 140000, 64, F64)),
          "small": (("pdf", 3000, 2500, 1, F32), ("cdf", 3000, 2500, 1, F64), ("logpdf", 3000, 2500, 1, F64), ("nll", 2000, 2500, 5, F32),
                    ("est_bandwidth", 600, 1400, 64, F64))}
CHUNK_BYTES = 1 << 30   # of one chunk of points x all supports in the torch route


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3), "rounds": len(ts)}


def torch_eval(x, s, h, what, rows):
    out = torch.empty_like(x)
    n_s = s.shape[0]
    for i0 in range(0, x.shape[0], rows):
        d = x[i0:i0 + rows, None] - s[None, :]
        if what == "cdf":
            out[i0:i0 + rows] = torch.special.erfc(d * (-1.0 / (h * math.sqrt(2.0)))).sum(dim=1) * (0.5 / n_s)
        elif what == "pdf":
            out[i0:i0 + rows] = torch.exp(d * d * (-0.5 / (h * h))).sum(dim=1) * (1.0 / (n_s * h * math.sqrt(2.0 * math.pi)))
        else:
            out[i0:i0 + rows] = torch.logsumexp(d * d * (-0.5 / (h * h)), dim=1) - math.log(n_s * h * math.sqrt(2.0 * math.pi))
        del d
    return out


def torch_nll(x, s, hb, rows):
    """-> (nll, dnll) float64 tensors: d^2 once per chunk, logsumexp and the softmax-weighted mean of 2 t per bandwidth"""
    n_s = s.shape[0]
    nll = torch.zeros(len(hb), dtype=F64, device=x.device)
    dnll = torch.zeros(len(hb), dtype=F64, device=x.device)
    for i0 in range(0, x.shape[0], rows):
        d = x[i0:i0 + rows, None] - s[None, :]
        d2 = d * d
        del d
        for b, h in enumerate(hb):
            t = d2 * (0.5 / (h * h))
            lse = torch.logsumexp(-t, dim=1)
            r = 2.0 * (torch.exp(-t - lse[:, None]) * t).sum(dim=1)
            nll[b] -= (lse.double() - math.log(n_s * h * math.sqrt(2.0 * math.pi))).sum()
            dnll[b] -= ((r.double() - 1.0) / h).sum()
            del t
        del d2
    return nll, dnll


class TorchKdeRv(KdeRv):
    """the same search over the torch route's likelihoods"""

    def nll_dnll(self, samples, bandwidths):
        hb = [float(v) for v in np.atleast_1d(bandwidths)]
        a, b = torch_nll(samples, self.supports, hb, self.rows)
        return a.cpu().numpy(), b.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kde.jsonl"))
    ap.add_argument("--shapes", default="full", choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--est-old-rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated ops to run")
    args = ap.parse_args()
    if args.rounds < 10 and args.shapes == "full":
        ap.error("at least 10 rounds")
    assert torch.cuda.is_available(), "bench_kde needs a GPU"
    ctx = cr.Context(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for (op, n_q, n_s, n_h, dt) in SHAPES[args.shapes]:
        if args.only and op not in args.only.split(","):
            continue
        name = str(dt).split(".")[-1]
        esz = 4 if dt == F32 else 8
        gen = torch.Generator("cuda").manual_seed(5)
        s = (5.25 + 10.0 * torch.randn(n_s, dtype=F64, device="cuda", generator=gen)).to(dt)
        x = (5.25 + 10.0 * torch.randn(n_q, dtype=F64, device="cuda", generator=gen)).to(dt)
        h0 = 1.06 * 10.0 * n_s ** -0.2          # the normal-reference bandwidth of the supports
        hb = [h0 * 2.0 ** ((b - n_h // 2) / 8.0) for b in range(n_h)]
        rows = max(1, min(n_q, CHUNK_BYTES // (n_s * esz)))
        old_rounds = args.rounds
        if op == "nll":
            new, old = (lambda: ctx.kde_nll(x, s, hb)), (lambda: torch_nll(x, s, hb, rows))
            work = n_q * n_s * n_h
        elif op == "est_bandwidth":
            def new():
                return torch.tensor(KdeRv(1.0, s, device=True, ctx=ctx).est_bandwidth(x))

            def old():
                rv = TorchKdeRv(1.0, s)
                rv.rows = rows
                return torch.tensor(rv.est_bandwidth(x))
            old_rounds = min(args.rounds, args.est_old_rounds)
            work = None
        else:
            new, old = (lambda: ctx.kde_eval(x, s, h0, op)), (lambda: torch_eval(x, s, h0, op, rows))
            work = n_q * n_s
        for _ in range(args.warmup):
            new()
        old()
        torch.cuda.synchronize()
        t_new, t_old = [], []
        for r in range(args.rounds):
            for fn, ts in ((new, t_new), (old, t_old)):
                if fn is old and r >= old_rounds:
                    continue
                t0 = time.perf_counter()
                res = fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                del res
        a, b = new(), old()
        if op == "nll":
            diff = max(float(((a[i] - b[i]).abs() / b[i].abs()).max()) for i in range(2))
        elif op in ("logpdf",):
            diff = float((a - b).abs().max())
        else:
            diff = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)
        sn, so = stats(t_new), stats(t_old)
        row = {"tool": "bench_kde", "op": op, "n_points": n_q, "n_supports": n_s, "n_h": n_h, "dtype": name, "compute_units": cus,
               "warmup": args.warmup, "new": sn, "old": so, "route": ctx.last_kde_route(),
               "old_route": "torch: chunked x[:, None] - s[None, :], exp / special.erfc / logsumexp, sum", "old_chunk_rows": rows,
               "old_chunks": (n_q + rows - 1) // rows, "ratio_new_over_old": round(sn["median_ms"] / so["median_ms"], 4),
               "spread_over_old_median": round(((sn["max_ms"] - sn["min_ms"]) + (so["max_ms"] - so["min_ms"])) / so["median_ms"], 4),
               "max_diff_new_vs_old": diff}
        if work is not None:
            row["pairs_per_s"] = round(work / (sn["median_ms"] * 1e-3), 1)
        else:
            rv = KdeRv(1.0, s, device=True, ctx=ctx)
            row["bandwidth"], row["nll_calls"] = rv.est_bandwidth(x), rv.n_nll_calls
        print(json.dumps(row), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        del x, s, a, b
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
