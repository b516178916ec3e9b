#!/usr/bin/env python3
"""Randomised sweep of the active-subspace gradient stage (corrla_grad_mat_f64) against the oracle: dimensions,
cloud sizes, neighbour counts, both orders, the three k-NN kernels (CORRLA_KNN = 1 / 2 / 3), both order-1 fit kernels
(CORRLA_FIT), and now and then an order-2 design too large for LDS (k up to 30: normal equations in global memory).
--wide draws the wide kernels' ground instead: k up to 256 and n_nbrs up to 2048 (order 1), order 2 up to k = 48, and
the switches that force the wide scan and fit (CORRLA_KNN=4, CORRLA_FIT=2) next to the others.
Every case is multiplied by a power-of-two scale, one for the cloud or one per feature (2^-40 .. 2^40), and checked in
feature units against the scale-free reference of tests/grad_reference.py (exact least squares; the oracle's pseudo-inverse
adds 1e-14 to the singular values and is only accurate for O(1) features).
usage: fuzz_grad.py [n_cases] [seed] [--wide]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import corrla_rs_amd as cr  # noqa: E402
from tests import grad_reference as gr  # noqa: E402


def run(n_cases=60, seed=0, ctx=None, verbose=True, wide=False):
    rng = np.random.default_rng(seed)
    rng_scale = np.random.default_rng([seed, 1])   # a stream of its own: the shapes of a seed stay what they were
    ctx = ctx or cr.Context(0)
    bad = 0
    worst = 0.0
    for case in range(n_cases):
        order = int(rng.integers(1, 3))
        if wide:
            k, n_nbrs, n, nq = _wide_draw(rng, order)
        else:
            big2 = order == 2 and rng.random() < 0.15
            k = int(rng.integers(1, 65)) if order == 1 else (int(rng.integers(15, 31)) if big2 else int(rng.integers(1, 11)))
            need = k + 1 if order == 1 else k * (k + 3) // 2
            n_nbrs = int(rng.integers(need + 1, min(512 if big2 else 160, need + 40) + 1))
            n = int(rng.integers(n_nbrs + 5, 3000))
        x = rng.standard_normal((n, k)) * rng.uniform(0.1, 10.0) + rng.uniform(-3, 3)
        w = rng.standard_normal(k)
        y = np.sin(x @ w * 0.1) + 0.05 * (x ** 2).sum(axis=1) + rng.uniform(-5, 5)
        if not wide:
            nq = int(rng.integers(1, 8 if big2 else 60))
        xq = x[rng.choice(n, size=nq, replace=False)] if rng.random() < 0.5 else rng.standard_normal((nq, k))
        # units: one power of two for the whole cloud, or one per feature
        d = np.exp2(rng_scale.integers(-40, 41, size=k if rng_scale.random() < 0.5 else 1).astype(np.float64)) * np.ones(k)
        x, xq = x * d, xq * d
        if wide:
            os.environ["CORRLA_KNN"] = str(int(rng.integers(0, 5)))   # 4 = the wide scan on any call
            os.environ["CORRLA_FIT"] = str(int(rng.integers(0, 3)))   # 2 = the wide fit on any call
        else:
            os.environ["CORRLA_KNN"] = str(int(rng.integers(1, 4)))   # 3 = the bf16-filter scan (n_nbrs <= 128, else round 2's)
            os.environ["CORRLA_FIT"] = str(int(rng.integers(0, 2)))   # 1 = the general fit kernel for order 1 too
        try:
            g, nreg = ctx.grad_mat(x, y, order, n_nbrs, xq)
        except Exception as e:  # noqa: BLE001
            if verbose:
                print("EXCEPTION", case, order, k, n, n_nbrs, repr(e)[:160])
            bad += 1
            continue
        go, _ = gr.gradients(x, y, xq, order, n_nbrs)
        dev = gr.feature_unit_error(g, go, d)
        # ill-conditioned local designs amplify the rounding differences of the two solvers (normal equations here)
        tol = 1e-7 if order == 1 else 1e-3
        worst = max(worst, dev)
        if nreg == 0 and not (dev <= tol):
            if verbose:
                print("VIOLATION", case, "order", order, "k", k, "n", n, "nbrs", n_nbrs, "nq", nq, "log2 scales %d..%d" %
                      (np.log2(d.min()), np.log2(d.max())), "dev %.2e" % dev)
            bad += 1
    os.environ.pop("CORRLA_KNN", None)
    os.environ.pop("CORRLA_FIT", None)
    return bad, worst


def _wide_draw(rng, order):
    """(k, n_nbrs, n_pts, n_queries) for --wide: order 1 up to k = 256 and 2048 neighbours, order 2 up to k = 48"""
    if order == 1:
        k = int(rng.integers(1, 257))
        n_nbrs = int(rng.integers(k + 2, max(k + 3, min(2048, k + 2 + int(rng.integers(1, 1800))))))
    else:
        k = int(rng.integers(1, 49))
        need = k * (k + 3) // 2
        n_nbrs = int(rng.integers(need + 1, min(2048, need + 200) + 1))
    n = int(rng.integers(n_nbrs + 5, max(3000, n_nbrs + 1000)))
    big = (k + 1 if order == 1 else k + k * (k + 1) // 2 + 1) > 300   # the oracle's pinv is the slow part
    nq = int(rng.integers(1, 4 if big else 40))
    return k, n_nbrs, n, nq


if __name__ == "__main__":
    wide = "--wide" in sys.argv
    args = [a for a in sys.argv[1:] if a != "--wide"]
    n_cases = int(args[0]) if args else 60
    bad, worst = run(n_cases, int(args[1]) if len(args) > 1 else 0, wide=wide)
    print("cases", n_cases, "violations", bad, "worst deviation %.2e" % worst)
    sys.exit(1 if bad else 0)
