"""Writes kde_known.npz: the inputs of every shape tests/test_gpu_kde.py uses (GPU_CALLS of tests/test_kde_plan.py) and
pdf, cdf, logpdf, nll and dnll of the Gaussian kernel density estimate on them, evaluated with mpmath at 50 digits and
rounded once to float64.  Needs mpmath (a development machine); the tests read only the .npz.

    python tests/golden/kde/make_kde_golden.py [--jobs N]

One data set per (n_q, n_s): the n_h axis reuses the base case's points and takes the first n_h of its 64 bandwidths.
  supports  s_j ~ N(5.25, 10^2), rounded to float32 (so the same values serve the f32 and the f64 runs)
  points    x_i = s_r + h_0 U(-3.5, 3.5) for a random support r, rounded to float32; where n_q > 1 the LAST point is the far
            point max_j s_j + 60 h_0
  h         h_0 = 0.5 is the bandwidth of pdf, cdf and logpdf and the smallest of the likelihood's; the others are log-spaced
            up to 16 h_0, in a fixed scattered order so that every prefix spans the range
Conditions the tests' bounds rely on, asserted here: every point but the far one lies within 4 h_0 of its nearest support
(t* <= 8 at every bandwidth), the far point lies 60 h_0 beyond the largest support.
Plain sums, no stabilisation: mpmath's exponent range does not underflow.  Terms below 10^-56 of the largest term of their
sum are skipped (50 digits)."""
import argparse
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from test_kde_plan import BASE, GPU_CALLS, HG, HL, MAX_H, QT, SC  # noqa: E402

SEED = 20241008
H0 = 0.5
CUT = 130.0       # e^-130 < 10^-56


def bandwidths():
    h = H0 * 16.0 ** (np.arange(MAX_H) / (MAX_H - 1.0))
    order = (np.arange(MAX_H) * 37) % MAX_H      # 37 is odd: a permutation; index 0 stays first
    return h[order]


def case_data(n_q, n_s):
    rng = np.random.default_rng([SEED, n_q, n_s])
    s = rng.normal(5.25, 10.0, n_s).astype(np.float32)
    x = (s[rng.integers(0, n_s, n_q)].astype(np.float64) + H0 * rng.uniform(-3.5, 3.5, n_q)).astype(np.float32)
    if n_q > 1:
        x[-1] = np.float32(float(s.max()) + 60.0 * H0)
    d2 = (x.astype(np.float64)[:, None] - s.astype(np.float64)[None, :]) ** 2
    near = np.sqrt(d2.min(axis=1))
    body = near[:-1] if n_q > 1 else near
    assert body.max() <= 4.0 * H0, "a point lies more than 4 bandwidths from its nearest support"
    if n_q > 1:
        assert abs(float(x[-1]) - float(s.max()) - 60.0 * H0) < 1e-4 and near[-1] >= 59.99 * H0
    return x, s


def point(args):
    """one point against every support: (pdf, cdf, logpdf at hs[0], logpdf and R at every h)"""
    import mpmath
    mpmath.mp.dps = 50
    mpf = mpmath.mpf
    xi, s, hs = args
    n_s = len(s)
    d = [mpf(float(xi)) - mpf(float(v)) for v in s]
    d2 = [v * v for v in d]
    d2min = min(d2)
    sqrt2pi = mpmath.sqrt(2 * mpmath.pi)
    logpdf, rr = [], []
    for h in hs:
        h = mpf(float(h))
        c = 1 / (2 * h * h)
        tmin = d2min * c
        sk = mpf(0)
        st = mpf(0)
        for v in d2:
            t = v * c
            if t - tmin > CUT:
                continue
            kk = mpmath.exp(-t)
            sk += kk
            st += 2 * t * kk
        logpdf.append(mpmath.log(sk) - mpmath.log(n_s * h * sqrt2pi))
        rr.append(st / sk)
    h0 = mpf(float(hs[0]))
    pdf = mpmath.exp(logpdf[0])
    r = 1 / (h0 * mpmath.sqrt(2))
    acc = mpf(0)
    for v in d:
        z = -v * r
        acc += 0 if z > 12 else (2 if z < -12 else mpmath.erfc(z))   # erfc(12) < 10^-64, the sum is >= erfc(4 / sqrt 2)
    cdf = acc / (2 * n_s)
    return float(pdf), float(cdf), float(logpdf[0]), logpdf, rr


def case(pool, n_q, n_s, n_h):
    import mpmath
    mpmath.mp.dps = 50
    x, s = case_data(n_q, n_s)
    hs = bandwidths()[:n_h]
    rows = pool.map(point, [(xi, s, hs) for xi in x], chunksize=4)
    out = {"x": x, "s": s, "h": hs,
           "pdf": np.array([r[0] for r in rows]), "cdf": np.array([r[1] for r in rows]), "logpdf": np.array([r[2] for r in rows])}
    nll, dnll = [], []
    for b, h in enumerate(hs):
        nll.append(float(-mpmath.fsum(r[3][b] for r in rows)))
        dnll.append(float(-mpmath.fsum((r[4][b] - 1) / mpmath.mpf(float(h)) for r in rows)))
    out["nll"], out["dnll"] = np.array(nll), np.array(dnll)
    # the far point's log-density is finite where the plain float64 density is zero
    if n_q > 1:
        assert out["pdf"][-1] == 0.0 and np.isfinite(out["logpdf"][-1]) and out["logpdf"][-1] < -1700.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=os.cpu_count() or 1)
    ap.add_argument("--out", default=os.path.join(HERE, "kde_known.npz"))
    a = ap.parse_args()
    shapes = {}
    for n_q, n_s, n_h in GPU_CALLS:           # the most bandwidths asked of each data set
        shapes[(n_q, n_s)] = max(shapes.get((n_q, n_s), 0), n_h)
    assert shapes[BASE[:2]] == MAX_H
    arrays = {"consts": np.array([QT, SC, HG, HL, MAX_H]), "h0": np.array(H0)}
    with multiprocessing.Pool(a.jobs) as pool:
        for (n_q, n_s), n_h in shapes.items():
            print("case", n_q, n_s, n_h, flush=True)
            for key, v in case(pool, n_q, n_s, n_h).items():
                arrays[f"{n_q}_{n_s}_{key}"] = v
    np.savez_compressed(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
