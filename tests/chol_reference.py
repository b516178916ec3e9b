"""numpy restatements for tests/test_gpu_chol.py and tests/test_gpu_chol_callers.py: symmetric positive definite matrices, a
matrix whose elimination is exact and fails at a chosen column, an unblocked Cholesky, and the derived bounds.  Host code
only.  gamma, the error-free product and the right-hand sides are tests/lu_reference.py's."""
import functools

import numpy as np

from tests.lu_reference import U, exact_matmul, gamma, rhs  # noqa: F401

KINDS = ("gram", "lehmer", "kms", "scaled")


# ---- matrices ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spd(kind, n):
    """read-only symmetric positive definite (n, n) float64"""
    rng = np.random.default_rng(6007 * n + len(kind))
    i, j = np.indices((n, n))
    if kind in ("gram", "scaled"):
        g = rng.standard_normal((n, n + 8))
        a = np.tril(g @ g.T / (n + 8))
        a = a + np.tril(a, -1).T  # symmetrised from the lower triangle
        if kind == "scaled":  # condition ~1e25; Cholesky is invariant under a two-sided scaling by powers of two
            d = np.exp2(rng.integers(-20, 21, size=n).astype(np.float64))
            a = a * np.outer(d, d)
    elif kind == "lehmer":  # min(i, j) / max(i, j), condition ~n^2
        a = (np.minimum(i, j) + 1.0) / (np.maximum(i, j) + 1.0)
    elif kind == "kms":  # Kac-Murdock-Szego
        a = 0.5 ** np.abs(i - j)
    else:
        raise ValueError(kind)
    a.setflags(write=False)
    return a


def not_spd_at(n, col, pivot, seed=11):
    """(a, lt): elimination exact in any summation order.  a = lt lt^T with lt = L0 diag(s), L0 unit lower with its other
    entries 0, +-1/2 or +-1/4 and s_j in {1/2, 1, 2} -- every partial sum is a small dyadic number -- and then
    pivot - s_col^2 added to a[col, col]: every earlier column of the factor is exactly lt's, and the pivot of column `col` is
    exactly `pivot` (0 or -1)."""
    rng = np.random.default_rng(seed + 31 * n + col)
    l0 = np.tril(rng.choice([0.0, 0.0, 0.5, -0.5, 0.25, -0.25], size=(n, n)), -1) + np.eye(n)
    s = rng.choice([0.5, 1.0, 2.0], size=n)
    lt = l0 * s[None, :]
    a = lt @ lt.T
    a[col, col] += pivot - s[col] ** 2
    return a, lt


# ---- the factorisation as the library states it -----------------------------------------------------------------------------------
def cholesky(a):
    """Unblocked right-looking Cholesky over the lower triangle of a copy of `a` -> (l with zeros above, info): info is the
    1-based column of the first pivot that is <= 0 or not finite (the elimination goes on), or 0."""
    w = np.tril(np.array(a, dtype=np.float64))
    n = w.shape[0]
    info = 0
    with np.errstate(all="ignore"):
        for j in range(n):
            piv = w[j, j]
            if not (piv > 0.0 and np.isfinite(piv)) and info == 0:
                info = j + 1
            d = np.sqrt(piv)
            w[j, j] = d
            w[j + 1:, j] /= d
            w[j + 1:, j + 1:] -= np.tril(np.outer(w[j + 1:, j], w[j + 1:, j]))
    return w, info


# ---- the derived checks -------------------------------------------------------------------------------------------------------------
def check_factorisation(a, l, k=None):
    """diag(L) > 0; |A - L L^T| <= gamma_k |L||L^T| componentwise with k = n + 1 (Higham, Thm 10.3), the product formed without
    rounding.  `a` is the symmetric matrix, `l` lower triangular with zeros above.  -> the largest ratio"""
    n = a.shape[0]
    assert np.all(np.diag(l) > 0.0), "a diagonal entry of L is not positive"
    assert not np.triu(l, 1).any()
    resid = np.abs(a.astype(np.longdouble) - exact_matmul(l, l.T)).astype(np.float64)
    bound = gamma(n + 1 if k is None else k) * (np.abs(l) @ np.abs(l).T)
    ratio = float(np.max(resid / np.where(bound > 0, bound, np.inf)))
    print(f"factorisation n={n}: max |A - L L^T| / bound = {ratio:.3f}")
    assert np.all(resid <= bound), f"|A - L L^T| exceeds gamma |L||L^T| by a factor {np.max(resid / np.where(bound > 0, bound, 1))}"
    return ratio


def check_logdet(diag, logdet):
    """|logdet - 2 sum log l_jj| <= (gamma_n + 4u) sum |2 log l_jj|: the reference sum in longdouble over the returned diagonal,
    gamma_n for a summation in any fixed order, 4u for two ulp of the device log (HIP documents 1 ulp for the f64 log)."""
    n = diag.shape[0]
    terms = 2.0 * np.log(diag.astype(np.longdouble))
    ref, scale = float(np.sum(terms)), float(np.sum(np.abs(terms)))
    err, bound = abs(logdet - ref), (gamma(n) + 4.0 * U) * scale
    print(f"logdet n={n}: {logdet!r} against {ref!r}, error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (logdet, ref, err, bound)


def check_solve(a, b, x, l):
    """|A x - b| <= gamma_(3n+1) |L||L^T||x| + gamma_(n+1) (|A||x| + |b|) componentwise (Thm 10.4; the second term is the f64
    residual of this very line)"""
    n = a.shape[0]
    resid = np.abs(a @ x - b)
    bound = gamma(3 * n + 1) * (np.abs(l) @ (np.abs(l).T @ np.abs(x))) + gamma(n + 1) * (np.abs(a) @ np.abs(x) + np.abs(b))
    ratio = float(np.max(resid / np.where(bound > 0, bound, np.inf)))
    print(f"solve n={n}: max |A x - b| / bound = {ratio:.3f}")
    assert np.all(resid <= bound), f"|Ax - b| exceeds its bound by a factor {np.max(resid / np.where(bound > 0, bound, 1))}"
    return ratio
