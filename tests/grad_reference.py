"""A scale-free reference of the gradient stage (corrla_grad_mat_*) for the tests -- plain numpy f64, no GPU.

The oracle (oracle/active_ss_oracle.py) restates the reference library, whose pseudo-inverse adds 1e-14 to every singular
value: accurate for O(1) features, not for features of 1e-9 or for features that differ in scale.  Here the fit is the exact
least-squares solution at any scale: every column of the design is divided by its 2-norm before numpy's lstsq and the
coefficients are un-scaled afterwards.  Neighbours are the oracle's: squared distances on the coordinates as passed, ordered
by (distance, index).

The clouds of tests/test_grad_reference.py (CPU: the conditions the GPU tests rest on) and tests/test_gpu_grad_scales.py
live here too, seeded, so that both files see the same points and queries.  Every y is iid N(0, 1), independent of x: any
change of a neighbour set then changes the gradient at leading order (with y = f(x) two tied points are often duplicates
with the same y, and swapping them changes nothing)."""
import functools

import numpy as np


# ---- the reference ---------------------------------------------------------------------------------------------------
def neighbours(x, x0, n_nbrs=None):
    """indices ordered by (squared distance, index) and the squared distances -- nearest_indices of the oracle"""
    d2 = np.sum((x - x0.reshape(1, -1)) ** 2, axis=1)
    order = np.lexsort((np.arange(d2.size), d2))
    return (order if n_nbrs is None else order[:n_nbrs]), d2


def design(dx, order):
    """[dx, 1] or [dx, dx_a dx_b (a <= b, a-major), 1]: the constant column is the last one"""
    cols = [dx]
    if order == 2:
        k = dx.shape[1]
        cols.append(np.stack([dx[:, a] * dx[:, b] for a in range(k) for b in range(a, k)], axis=1))
    cols.append(np.ones((dx.shape[0], 1)))
    return np.hstack(cols)


def fit_gradient(x_nbr, y_nbr, x0, order):
    """the k linear coefficients of the least-squares polynomial in x - x0: its gradient at x0"""
    d = design(x_nbr - x0.reshape(1, -1), order)
    norms = np.linalg.norm(d, axis=0)
    norms[norms == 0.0] = 1.0
    beta = np.linalg.lstsq(d / norms, y_nbr, rcond=None)[0] / norms
    return beta[: x_nbr.shape[1]]


def gradients(x, y, xq, order, n_nbrs, swap=False):
    """k x n_q reference gradients.  swap: the n-th neighbour is replaced by the (n + 1)-th (what a wrong tie rule does).
    Also returns the n-th and (n + 1)-th squared distances of every query."""
    x, y, xq = np.asarray(x, np.float64), np.asarray(y, np.float64).ravel(), np.asarray(xq, np.float64)
    g = np.zeros((x.shape[1], xq.shape[0]))
    cut = np.zeros((xq.shape[0], 2))
    for i, x0 in enumerate(xq):
        idx, d2 = neighbours(x, x0)
        cut[i] = d2[idx[n_nbrs - 1]], d2[idx[min(n_nbrs, idx.size - 1)]]
        take = idx[:n_nbrs].copy()
        if swap:
            take[-1] = idx[n_nbrs]
        g[:, i] = fit_gradient(x[take], y[take], x0, order)
    return g, cut


def feature_unit_error(g, ref, d=None):
    """max_j |g_j - ref_j| D_j / max_j |ref_j| D_j over a k x n_q matrix: an error in an O(1) feature does not hide behind
    the large slope of a small-scale feature"""
    d = np.ones(ref.shape[0]) if d is None else np.asarray(d, np.float64)
    return float(np.max(np.abs(g - ref) * d[:, None]) / np.max(np.abs(ref) * d[:, None]))


# ---- the pivot rule of the limited fits before they equilibrated (documentation of the finding) ------------------------
def raw_pivot_rule_accepts(dsg):
    """Cholesky of the raw normal equations of a design with every pivot tested against 1e-13 max diag, as grad_fit_kernel
    and grad_fit_lin_kernel did: False where they called the design numerically singular"""
    m = dsg.T @ dsg
    dmax = float(np.max(np.diag(m)))
    p = m.shape[0]
    low = np.zeros_like(m)
    for j in range(p):
        sjj = m[j, j] - low[j, :j] @ low[j, :j]
        if not sjj > 1e-13 * dmax:
            return False
        low[j, j] = np.sqrt(sjj)
        low[j + 1:, j] = (m[j + 1:, j] - low[j + 1:, :j] @ low[j, :j]) / low[j, j]
    return True


# ---- clouds ------------------------------------------------------------------------------------------------------------
UNIFORM_SCAN_EXPONENTS = (-83, -66, -62, -20, 0, 20, 62, 83)   # -66 / -62: squares in and just above the f32 denormals
UNIFORM_FIT_EXPONENTS = (-40, -20, -10, 0, 10, 27, 40)
N_QUERIES = 64


def ladder(k):
    """per-feature scales 2^round(-30 + 60 j / (k - 1)): micrometres beside pascals"""
    return np.exp2(np.round(-30.0 + 60.0 * np.arange(k) / (k - 1)))


@functools.lru_cache(maxsize=None)
def gaussian_cloud(k, n_pts=3000):
    """(x, y, xq): an O(1) Gaussian cloud; the tests multiply it by powers of two only, so neighbour sets do not depend on the
    scale and reference(scaled) = reference(unscaled) / scale exactly"""
    rng = np.random.default_rng(7000 + k)
    x = rng.standard_normal((n_pts, k))
    y = rng.standard_normal(n_pts)
    return x, y, x[:N_QUERIES].copy()


@functools.lru_cache(maxsize=None)
def ladder_cloud(k, n_pts=3000):
    """(x, y, xq, D): a Gaussian cloud with feature j multiplied by D_j; neighbours are those of the scaled cloud"""
    rng = np.random.default_rng(7100 + k)
    d = ladder(k)
    x = rng.standard_normal((n_pts, k)) * d
    y = rng.standard_normal(n_pts)
    return x, y, x[:N_QUERIES].copy(), d


@functools.lru_cache(maxsize=None)
def lattice_cloud():
    """(x, y, xq): the shuffled integer lattice {0..20}^3 -- 9261 points, exact integer distances, every shell a tie"""
    rng = np.random.default_rng(7200)
    ax = np.arange(21.0)
    x = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    x = x[rng.permutation(x.shape[0])]
    y = rng.standard_normal(x.shape[0])
    return x, y, x[:128].copy()


INTEGER_CLOUDS = {16: 40, 40: 60, 64: 80}   # features -> neighbours
LATTICE_NBRS = (12, 30, 70)


@functools.lru_cache(maxsize=None)
def integer_cloud(k):
    """(x, y, xq): 9000 points with coordinates in {-2..2}: squared distances are small integers, ties everywhere"""
    rng = np.random.default_rng(7300 + k)
    x = rng.integers(-2, 3, (9000, k)).astype(np.float64)
    y = rng.standard_normal(9000)
    return x, y, x[:N_QUERIES].copy()


PAIRED_CLOUDS = {16: (2000, 41), 24: (4100, 81)}   # features -> (distinct points, neighbours): an odd count splits a pair
OUTLIER_EXPONENTS = (80, 120)   # 2^80: an O(1) point keeps normal f32 products beside it; 2^120: it no longer does


@functools.lru_cache(maxsize=None)
def paired_cloud(k):
    """(x, y, xq): every point twice (copy i + n of point i), y drawn independently of x.  With an odd number of neighbours
    the cut separates the two copies of one point for every query: the lower index must be kept"""
    n = PAIRED_CLOUDS[k][0]
    rng = np.random.default_rng(7400 + k)
    x = rng.standard_normal((n, k))
    x = np.vstack([x, x])
    y = rng.standard_normal(2 * n)
    return x, y, x[:N_QUERIES].copy()


def with_outliers(x, y, kind, e):
    """the cloud with one point (kind "one") or a +- pair ("pair") of coordinates 2^e appended: every index, neighbour set and
    gradient of the O(1) queries stays what it was"""
    far = np.full((1, x.shape[1]), 2.0 ** e)
    extra = far if kind == "one" else np.vstack([far, -far])
    return np.vstack([x, extra]), np.concatenate([y, np.zeros(extra.shape[0])])


@functools.lru_cache(maxsize=None)
def reference(cloud, k, order, n_nbrs, n_q=None, swap=False):
    """reference gradients of a named cloud, computed once and shared (read-only): (g, cut, D or None)"""
    if cloud == "gauss":
        x, y, xq = gaussian_cloud(k)
        d = None
    elif cloud == "ladder":
        x, y, xq, d = ladder_cloud(k)
    elif cloud == "lattice":
        x, y, xq = lattice_cloud()
        d = None
    elif cloud == "paired":
        x, y, xq = paired_cloud(k)
        d = None
    elif cloud == "ladder-all":          # the queries of the end-to-end case: the first 400 points
        x, y, _, d = ladder_cloud(k)
        xq = x
    else:
        x, y, xq = integer_cloud(k)
        d = None
    g, cut = gradients(x, y, xq[:n_q], order, n_nbrs, swap=swap)
    g.setflags(write=False)
    cut.setflags(write=False)
    return g, cut, d


# ---- the calls of tests/test_gpu_grad_scales.py: (features, neighbours, order, CORRLA_KNN, CORRLA_FIT) -> what they reach,
#      in the notation of ROUTES in tests/test_grad_plan.py (scan, waves, slices, steps | fit, tiles); 3000 points ----------
SCANS = {
    "valu": ((6, 12, 1, 1, 0), ("valu", 0, 0, 0)),
    "mfma4x4": ((16, 150, 1, 2, 0), ("mfma", 4, 4, 0)),
    "mfma2x16": ((64, 130, 1, 2, 0), ("mfma", 2, 16, 0)),
    "knn2s1": ((5, 12, 1, 3, 0), ("knn2", 0, 0, 1)),
    "knn2s2": ((40, 50, 1, 3, 0), ("knn2", 0, 0, 2)),
    "wide": ((5, 30, 1, 4, 0), ("wide", 0, 0, 0)),
}
# the units ladder at k = 5, 40 and 64 on every scan that takes that k
LADDER_SCANS = {
    "valu-k5": ((5, 12, 1, 1, 0), ("valu", 0, 0, 0)),
    "valu-k40": ((40, 60, 1, 1, 0), ("valu", 0, 0, 0)),
    "valu-k64": ((64, 80, 1, 1, 0), ("valu", 0, 0, 0)),
    "mfma4x4-k5": ((5, 150, 1, 2, 0), ("mfma", 4, 4, 0)),
    "mfma4x16-k40": ((40, 60, 1, 2, 0), ("mfma", 4, 16, 0)),
    "mfma2x16-k64": ((64, 130, 1, 2, 0), ("mfma", 2, 16, 0)),
    "knn2s1-k5": ((5, 12, 1, 3, 0), ("knn2", 0, 0, 1)),
    "knn2s2-k40": ((40, 50, 1, 3, 0), ("knn2", 0, 0, 2)),
    "knn2s2-k64": ((64, 80, 1, 3, 0), ("knn2", 0, 0, 2)),
    "wide-k5": ((5, 30, 1, 4, 0), ("wide", 0, 0, 0)),
    "wide-k40": ((40, 60, 1, 4, 0), ("wide", 0, 0, 0)),
    "wide-k64": ((64, 80, 1, 4, 0), ("wide", 0, 0, 0)),
}
FITS = {   # all behind the VALU scan, so that a scan fault cannot mask a fit fault
    "lin1": ((6, 12, 1, 1, 0), ("lin", 1)),
    "lin3": ((40, 60, 1, 1, 0), ("lin", 3)),
    "lin5": ((64, 80, 1, 1, 0), ("lin", 5)),
    "lds-o1": ((5, 12, 1, 1, 1), ("lds", 0)),
    "lds-o2": ((3, 14, 2, 1, 0), ("lds", 0)),
    "global-o2": ((20, 300, 2, 1, 0), ("global", 0)),
    "wide-o2": ((5, 30, 2, 1, 2), ("wide", 0)),
}
OUTLIER_SCANS = ("mfma4x4", "mfma2x16", "knn2s1", "knn2s2")   # rows of SCANS: the scans whose filters work on f32 images
FIT_SVD_LADDER = (40, 60, 400, 8)   # features, neighbours, queries, components of the end-to-end case
TIE_SCANS = {"valu": 1, "mfma": 2, "knn2": 3, "wide": 4}   # CORRLA_KNN


def tolerance(order):
    """the project's own (test_every_route_matches_the_oracle)"""
    return 1e-9 if order == 1 else 1e-8
