"""What the tests of the symmetric eigensolver (corrla_eigh_*, Context.eigh) share: the seeded matrix families, the bound
helpers, and a numpy restatement of the device algorithm (corrla_rs_amd/csrc/eigh_kernels.hpp) with the same schedule, the
same thresholds and the same threshold-Jacobi inner solver.  tools/record_eigh_cases.py runs the restatement once on every
case of GPU_CALLS (tests/test_eigh_plan.py) and stores the sweeps and the three error ratios in tests/golden/eigh_cases.json;
the GPU test takes its working bounds from that file.

Units: u = 2^-53.  residual |A V - V diag(w)|_F / (n u |A|_F), orthogonality |V^T V - I|_F / (n u), eigenvalues
max |w - w_LAPACK| / (n u |A|_F).  A ratio whose numerator and denominator are both zero is 0."""
import json
import os

import numpy as np

U = 2.0 ** -53
B = 32
PAIR = 64
SMALL_N = 64
MAX_SWEEPS = 40
INNER_SWEEPS = 1
# the fixed caps: conditions, so that a working bound cannot hide a failure
CAP_RESIDUAL, CAP_ORTH, CAP_EIG = 64.0, 32.0, 4.0
FAMILIES = ("gauss", "gram", "cluster", "graded", "rbf", "pm", "diag", "zero")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eigh_cases.json")


def _seed(name, n):
    return 1000 * FAMILIES.index(name) + n


def _orthogonal(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def family(name, n):
    """The matrix of family `name` and order n: symmetric, float64, seeded by (name, n)."""
    rng = np.random.default_rng(_seed(name, n))
    if name == "gauss":
        g = rng.standard_normal((n, n))
        a = 0.5 * (g + g.T)
    elif name == "gram":                       # rank n / 3
        x = rng.standard_normal((n, max(1, n // 3)))
        a = x @ x.T
    elif name == "cluster":                    # the spectrum {-2, 1, 1 + 1e-9, 3}
        d = np.array([-2.0, 1.0, 1.0 + 1e-9, 3.0])[np.arange(n) % 4]
        q = _orthogonal(rng, n)
        a = (q * d) @ q.T
    elif name == "graded":                     # +-10^(0 .. -18)
        e = -18.0 * np.arange(n) / max(1, n - 1)
        d = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * 10.0 ** e
        q = _orthogonal(rng, n)
        a = (q * d) @ q.T
    elif name == "rbf":                        # the cubic-kernel saddle system [[K, P], [P^T, 0]], P = [x, 1] in the plane
        n_s = n - 3 if n >= 5 else n
        x = rng.uniform(-1.0, 1.0, (n_s, 2))
        k = np.linalg.norm(x[:, None, :] - x[None, :, :], axis=2) ** 3
        a = np.zeros((n, n))
        a[:n_s, :n_s] = k
        if n_s < n:
            p = np.hstack([x, np.ones((n_s, 1))])
            a[:n_s, n_s:] = p
            a[n_s:, :n_s] = p.T
    elif name == "pm":                         # [[0, P], [P^T, 0]]: exact +- pairs
        h = n // 2
        p = rng.standard_normal((h, n - h))
        a = np.zeros((n, n))
        a[:h, h:] = p
        a[h:, :h] = p.T
    elif name == "diag":
        a = np.diag(rng.standard_normal(n))
    elif name == "zero":
        a = np.zeros((n, n))
    else:
        raise KeyError(name)
    return np.ascontiguousarray(0.5 * (a + a.T))


def tournament(nb, r):
    """The pairs (i < j) of round r over nb blocks: eigh_pair of eigh_plan.hpp."""
    m = nb + (nb & 1)
    out = []
    for p in range(nb // 2):
        q = p + (nb & 1)
        a, b = (r, m - 1) if q == 0 else ((r + q) % (m - 1), (r - q) % (m - 1))
        out.append((min(a, b), max(a, b)))
    return out


_STEPS = [np.array(tournament(PAIR, r)) for r in range(PAIR - 1)]


def measure(g, active):
    d = np.diag(g)[active]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.abs(g[np.ix_(active, active)]) / np.sqrt(np.outer(d, d))
    q = np.where(np.outer(d, d) > 0.0, q, 0.0)
    np.fill_diagonal(q, 0.0)
    return float(q.max()) if q.size else 0.0


def jacobi_threshold(g, r, active, thr, max_sweeps):
    """eigh_jacobi_lds: cyclic threshold Jacobi on the 64 x 64 g in the order of the tournament, 32 disjoint rotations per
    step, the smaller angle, an exact zero at the rotated entry; r accumulates the rotations.  -> the sweeps that rotated."""
    act = np.zeros(PAIR, bool)
    act[active] = True
    rotated = 0
    for _ in range(max_sweeps):
        any_rot = False
        for pq in _STEPS:
            p, q = pq[:, 0], pq[:, 1]
            gpp, gqq, gpq = g[p, p], g[q, q], g[p, q]
            rot = act[p] & act[q] & (np.abs(gpq) > thr * np.sqrt(np.abs(gpp * gqq)))
            if not rot.any():
                continue
            p, q, gpp, gqq, gpq = p[rot], q[rot], gpp[rot], gqq[rot], gpq[rot]
            with np.errstate(over="ignore"):
                zeta = (gqq - gpp) / (2.0 * gpq)
                t = np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = c * t
            ok = s != 0.0
            if not ok.any():
                continue
            p, q, c, s = p[ok], q[ok], c[ok], s[ok]
            any_rot = True
            for m in (g, r):
                x, y = m[:, p].copy(), m[:, q].copy()
                m[:, p] = c * x - s * y
                m[:, q] = s * x + c * y
            x, y = g[p, :].copy(), g[q, :].copy()
            g[p, :] = c[:, None] * x - s[:, None] * y
            g[q, :] = s[:, None] * x + c[:, None] * y
            g[p, q] = 0.0
            g[q, p] = 0.0
        if not any_rot:
            break
        rotated += 1
    return rotated


def shift_of(a):
    fro = float(np.sqrt(np.sum(a * a)))
    inf = float(np.abs(a).sum(axis=1).max())
    return 1.5 * (fro if 0.0 < fro < inf else inf)


def _finish(a, cols):
    """eigh_colnorm / unit / rayleigh / rank / scatter: unit columns with the component of largest magnitude positive (the
    first of equal magnitudes), the Rayleigh quotients u^T a u as eigenvalues, ascending, ties in column order.  The device
    keeps the sums of squares and the quotients in two doubles; numpy's pairwise sums play that part here."""
    top = np.argmax(np.abs(cols), axis=0)
    sgn = np.where(cols[top, np.arange(cols.shape[1])] < 0.0, -1.0, 1.0)
    u = cols / (sgn * np.sqrt(np.sum(cols * cols, axis=0)))
    lam = np.sum(u * (a @ u), axis=0) / np.sum(u * u, axis=0)   # over the rounded u's own length: the normalisation's rounding cancels
    order = np.argsort(lam, kind="stable")
    return lam[order], u[:, order]


def restatement(a):
    """The device algorithm in numpy -> (w, v, sweeps).  Only the lower triangle of a is read."""
    n = a.shape[0]
    a = np.tril(a) + np.tril(a, -1).T
    sigma = shift_of(a)
    if sigma == 0.0:
        return np.zeros(n), np.eye(n), 0
    tol = 2.0 * np.sqrt(n) * U
    # SMALL is BLOCKED with one pair that holds every column: block 0 the first 32, block 1 the rest
    nb = 2 if n <= SMALL_N else -(-n // B)
    w_ = np.zeros((n, nb * B))
    w_[:, :n] = np.linalg.cholesky(a + sigma * np.eye(n))
    rounds = nb + (nb & 1) - 1
    sweeps = 0
    while True:
        worst = 0.0
        for rd in range(rounds):
            for i, j in tournament(nb, rd):
                cols = np.r_[i * B:(i + 1) * B, j * B:(j + 1) * B]
                active = np.nonzero(cols < n)[0]
                x = w_[:, cols]
                g = x.T @ x
                m = measure(g, active)
                worst = max(worst, m)
                if not m > tol:
                    continue
                r = np.eye(PAIR)
                jacobi_threshold(g, r, active, 0.5 * tol, INNER_SWEEPS)
                w_[:, cols] = x @ r
        if worst <= tol:
            break
        sweeps += 1
        if sweeps > MAX_SWEEPS:
            raise RuntimeError("the restatement did not converge within the sweep cap")
    w, v = _finish(a, w_[:, :n])
    return w, v, sweeps


def _ratio(num, den):
    return 0.0 if num == 0.0 else (float("inf") if den == 0.0 else num / den)


def ratios(a, w, v, w_lapack=None):
    """-> {"residual", "orth", "eig"} of (w, v) on the symmetric a, in the units of the module docstring."""
    n = a.shape[0]
    na = float(np.linalg.norm(a))
    if w_lapack is None:
        w_lapack = np.linalg.eigh(a)[0]   # not eigvalsh: it takes another LAPACK path, and the two differ by a few ulps
    return {"residual": _ratio(float(np.linalg.norm(a @ v - v * w)), n * U * na),
            "orth": float(np.linalg.norm(v.T @ v - np.eye(n))) / (n * U),
            "eig": _ratio(float(np.max(np.abs(w - w_lapack))), n * U * na)}


CAPS = {"residual": CAP_RESIDUAL, "orth": CAP_ORTH, "eig": CAP_EIG}


def working_bound(recorded, key):
    """4 x the restatement's recorded value of the case, never above the cap"""
    return min(4.0 * recorded, CAPS[key])


def within_restatement_limits(got):
    """What the restatement itself has to meet before its values may serve as working bounds: a quarter of every cap."""
    return all(got[key] <= 0.25 * CAPS[key] for key in CAPS)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def case_id(name, n):
    return f"{name}-{n}"


def sign_convention_holds(v):
    top = np.argmax(np.abs(v), axis=0)
    return bool(np.all(v[top, np.arange(v.shape[1])] > 0.0))
