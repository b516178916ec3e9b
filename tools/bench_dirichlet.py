#!/usr/bin/env python3
"""Constrained Dirichlet sampling on the device: Context.dirichlet_sample (corrla_dirichlet_sample_dev_f64: draws generated,
tested against the box and counted where they are made, one bit per draw stored, the accepted ones generated again) against the
route a user has in torch on the same device: torch.distributions.Dirichlet(alpha).sample((chunk,)) in float64, the box mask
and nonzero, chunk after chunk until n_samples rows are found -- the same stop rule, the comparator is torch.

Rows appended to --out (default profiles/dirichlet.jsonl), one JSON line each:
  test_rate   draws per second of the TEST / SCAN / EMIT launches when nothing is ever accepted (a box no draw reaches), so
              that a call runs every draw it was given: d = 3 with alpha = 1 and 0.6, d = 17 with alpha = 1.  The time is the
              whole call's (its read-backs included); `readbacks` says how many it made.
  example     the whole call of examples/benchmark_dirichlet_sampler.py: the uranium box, 3000 samples, alpha = 1, 500 shots of
              10^6 allowed -- about 1.7 * 10^8 draws -- against the torch route; n_drawn, the read-backs, and the share of the
              call's time beyond n_drawn / (the measured rate of the test_rate row of the same d and alpha): what the batching
              and the draws behind the last needed shot cost.
  error       the measured device error of Context.dirichlet_draws against the numpy restatement (tests/dirichlet_reference.py)
              in units of u = 2^-53 and as a share of the bound tests/test_gpu_dirichlet.py derives.
One process, interleaved rounds after warm-up (which also ramps the clocks): each round times the new call and then the torch
route once, each ended by a device synchronise; medians with min - max.  The torch arm of the example takes --old-rounds rounds.
  --shapes small    tiny shapes, to rehearse the tool"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import corrla_rs_amd as cr  # noqa: E402

URANIUM = np.array(((0.0, 0.0026), (0.1955, 0.1995), (0.80, 0.825)))


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3), "rounds": len(ts)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def unreachable_box(d):
    """feasible (the upper bounds sum above 1) but no draw gets there: the first component within 2^-40 of 1"""
    b = np.zeros((d, 2))
    b[:, 1] = 1.0
    b[0, 0] = 1.0 - 2.0 ** -40
    return b


def torch_sample(bounds, alphas, n_samples, max_zshots, chunk):
    """the stop rule of constr_dirichlet_sample on torch: -> (samples, n_found, n_drawn)"""
    dist = torch.distributions.Dirichlet(alphas)
    lo, hi = bounds[:, 0], bounds[:, 1]
    out = torch.zeros((n_samples, alphas.shape[0]), dtype=torch.float64, device=alphas.device)
    found = shots = 0
    while shots < max_zshots and found < n_samples:
        x = dist.sample((chunk,))
        rows = torch.nonzero(((x >= lo) & (x <= hi)).all(dim=1)).reshape(-1)[: n_samples - found]    # synchronises: the count decides
        out[found: found + rows.shape[0]] = x[rows]
        found += int(rows.shape[0])
        shots += 1
    return out, found, shots * chunk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dirichlet.jsonl"))
    ap.add_argument("--shapes", choices=("full", "small"), default="full")
    ap.add_argument("--only", default="test_rate,example,error")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--old-rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    only = a.only.split(",")
    ctx = cr.Context(0)
    dev = torch.device("cuda:0")
    small = a.shapes == "small"
    rows, rates = [], {}

    if "test_rate" in only:
        shots, chunk = (4, 1 << 16) if small else (2048, 1 << 20)     # 2.1 * 10^9 draws: 32 full launches
        for d, alpha in ((3, 1.0), (3, 0.6), (17, 1.0)):
            box, al = unreachable_box(d), np.full(d, alpha)
            call = lambda: ctx.dirichlet_sample(box, 1000, al, seed=1, max_zshots=shots, chunk_size=chunk, device=True)
            for _ in range(a.warmup):
                call()
            ts = []
            for _ in range(a.rounds):
                t, (_, found, drawn) = timed(call)
                assert found == 0 and drawn == shots * chunk
                ts.append(t)
            s = stats(ts)
            rates[(d, alpha)] = drawn / (s["median_ms"] * 1e-3)
            rows.append({"op": "test_rate", "d": d, "alpha": alpha, "draws": drawn, **s, "draws_per_s": rates[(d, alpha)],
                         "readbacks": ctx.last_dirichlet_readbacks(), "route": ctx.last_dirichlet_route()})
            print(json.dumps(rows[-1]), flush=True)

    if "example" in only:
        n_samples, shots, chunk = (30, 500, 100_000) if small else (3000, 500, 1_000_000)
        al_t, b_t = torch.ones(3, dtype=torch.float64, device=dev), torch.from_numpy(URANIUM).to(dev)
        new = lambda seed: ctx.dirichlet_sample(URANIUM, n_samples, None, seed=seed, max_zshots=shots, chunk_size=chunk, device=True)
        old = lambda: torch_sample(b_t, al_t, n_samples, shots, chunk)
        for w in range(a.warmup):
            new(100 + w)
        old()
        t_new, t_old, drawn_new, drawn_old, rb = [], [], [], [], []
        for r in range(a.rounds):
            t, (x, found, drawn) = timed(lambda: new(r))       # a seed per round: the draws needed vary by a few per cent
            assert found == n_samples
            t_new.append(t), drawn_new.append(drawn), rb.append(ctx.last_dirichlet_readbacks())
            if r < a.old_rounds:
                t, (y, found, drawn) = timed(old)
                assert found == n_samples
                t_old.append(t), drawn_old.append(drawn)
        xs = x.cpu().numpy()
        assert np.all((URANIUM[:, 0] <= xs) & (xs <= URANIUM[:, 1])) and np.max(np.abs(xs.sum(axis=1) - 1.0)) < 1e-12
        s_new, s_old = stats(t_new), stats(t_old)
        row = {"op": "example", "box": "uranium", "n_samples": n_samples, "alpha": 1.0, "chunk_size": chunk, "new": s_new, "torch": s_old,
               "ratio_new_over_torch": round(s_new["median_ms"] / s_old["median_ms"], 5), "n_drawn_median": int(np.median(drawn_new)),
               "n_drawn_torch_median": int(np.median(drawn_old)), "readbacks": sorted(set(rb)),
               "draws_per_s_whole_call": np.median(drawn_new) / (s_new["median_ms"] * 1e-3)}
        if (3, 1.0) in rates:
            needed_ms = float(np.median(drawn_new)) / rates[(3, 1.0)] * 1e3
            row["ms_of_n_drawn_at_test_rate"] = round(needed_ms, 3)
            row["share_of_time_beyond_the_needed_draws"] = round(1.0 - needed_ms / s_new["median_ms"], 4)
        rows.append(row)
        print(json.dumps(row), flush=True)

    if "error" in only:
        from tests import dirichlet_reference as R
        for alphas in ((1.0,) * 3, (0.6,) * 3, (0.3, 1.0, 2.5, 7.0, 0.6), (1.0,) * 17, (0.6,) * 40):
            n = 1024 if small else 8192
            want, margin, rel = R.draws(0, n, alphas, 1.0, 20241008, full=True)
            got = ctx.dirichlet_draws(n, alphas, seed=20241008)
            err = np.abs(got - want)
            rows.append({"op": "error", "d": len(alphas), "alpha": sorted(set(alphas)), "draws": n, "min_margin": float(margin.min()) if np.isfinite(margin.min()) else None,
                         "max_rel_err_u": float(np.max(err / want) / R.U), "max_share_of_derived_bound": float(np.max(err / (rel * R.U * want))),
                         "test_bound_factor": 4.0, "rows_differing_outright": int(np.sum(np.any(err > 1e-6 * want, axis=1)))})
            print(json.dumps(rows[-1]), flush=True)

    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
