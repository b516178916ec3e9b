"""numpy restatements for tests/test_gpu_lu.py and tests/test_gpu_rbf_fit.py: the matrices, partial pivoting with the
library's tie rule, an error-free matrix product for the factorisation residual, and the derived bounds.  Host code only."""
import functools

import numpy as np

U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- matrices ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrix(kind, n):
    """read-only (n, n) float64"""
    rng = np.random.default_rng(7919 * n + len(kind))
    if kind == "gauss":
        a = rng.standard_normal((n, n))
    elif kind == "shift":  # a cyclic shift plus noise: the pivot of column j sits in row (j + 1) mod n, every column interchanges
        a = np.roll(np.eye(n), 1, axis=0) + 1.0e-3 * rng.standard_normal((n, n))
    elif kind == "wilkinson":  # growth 2^(n - 1) under partial pivoting, no interchange (every column ties, lowest row wins)
        a = np.eye(n) - np.tril(np.ones((n, n)), -1)
        a[:, -1] = 1.0
    else:
        raise ValueError(kind)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def rhs(n, n_rhs):
    b = np.random.default_rng(104729 * n + n_rhs).standard_normal((n, n_rhs))
    b.setflags(write=False)
    return b


def singular_at(n, col, seed=5):
    """Elimination exact in any order: A = Pi L0 U0 with L0 unit lower, its other entries 0, +-1/2 or +-1/4, and U0 upper with
    small integers and a nonzero diagonal -- but column `col` of U0 a copy of column col - 1 above the diagonal and zero from it
    on.  The candidates of column j are L0[:, j] u_jj: the row of the unit entry wins alone, the multipliers (l u) / u are
    exactly L0's, every intermediate value is a small dyadic number -- so the candidates of column `col` are all exactly zero
    while every earlier pivot is not.  The rows are shuffled: the pivots interchange.  col >= 1."""
    rng = np.random.default_rng(seed + 31 * n + col)
    l0 = np.tril(rng.choice([0.0, 0.0, 0.5, -0.5, 0.25, -0.25], size=(n, n)), -1) + np.eye(n)
    u0 = np.triu(rng.integers(-2, 3, size=(n, n)).astype(np.float64), 1) + np.diag(rng.choice([-3.0, -2.0, 2.0, 3.0], size=n))
    u0[:, col] = u0[:, col - 1]
    u0[col:, col] = 0.0
    return (l0 @ u0)[rng.permutation(n)]


# ---- partial pivoting as the library states it ----------------------------------------------------------------------------------
def getrf(a, follow=None, tol=None):
    """Unblocked LU of a copy of `a`: the pivot of column j is the entry of largest magnitude on or below the diagonal, ties
    to the lowest row.  -> (lu, ipiv, margin, info): margin[j] = |winner| - |runner-up| (inf with one candidate), info the
    1-based column of an exactly zero or non-finite pivot (the factorisation stops there) or 0.
    follow, tol: where margin[j] <= tol[j], take follow[j] instead when it is one of the near-tied rows -- a tie within
    rounding may go either way, and the later columns are only comparable along the same path."""
    lu = np.array(a, dtype=np.float64)
    n = lu.shape[0]
    ipiv = np.arange(n)
    margin = np.full(n, np.inf)
    for j in range(n):
        col = np.abs(lu[j:, j])
        p = j + int(np.argmax(col))  # argmax: the first of equal maxima
        if n - j > 1:
            rest = np.delete(col, p - j)
            margin[j] = col[p - j] - rest.max()
        if follow is not None and tol is not None and margin[j] <= tol[j]:
            f = int(follow[j])
            if j <= f < n and col[p - j] - col[f - j] <= tol[j]:
                p = f
        ipiv[j] = p
        if p != j:
            lu[[j, p]] = lu[[p, j]]
        piv = lu[j, j]
        if not (abs(piv) > 0.0 and np.isfinite(piv)):
            return lu, ipiv, margin, j + 1
        lu[j + 1:, j] /= piv
        lu[j + 1:, j + 1:] -= np.outer(lu[j + 1:, j], lu[j, j + 1:])
    return lu, ipiv, margin, 0


def split_lu(lu):
    return np.tril(lu, -1) + np.eye(lu.shape[0]), np.triu(lu)


def permute(a, ipiv):
    """P a: the interchanges applied in order"""
    pa = np.array(a)
    for j, p in enumerate(ipiv):
        if p != j:
            pa[[j, p]] = pa[[p, j]]
    return pa


# ---- an error-free product (the residual P A - L U must not carry the test's own rounding) --------------------------------------
def _slices(m, axis, beta):
    """m as a sum of matrices whose rows (axis=1) or columns (axis=0) are integers of at most beta + 1 bits times one power of
    two each: the extraction (r + sigma) - sigma with sigma = 0.75 * 2^(e + 53 - beta) rounds r to a multiple of 2^(e - beta)."""
    out, r = [], np.array(m, dtype=np.float64)
    for _ in range(64):
        mx = np.max(np.abs(r), axis=axis, keepdims=True)
        if not mx.any():
            break
        e = np.ceil(np.log2(np.where(mx > 0, mx, 1.0)))
        sigma = np.where(mx > 0, 0.75 * np.exp2(e + 53 - beta), 0.0)
        s = (r + sigma) - sigma
        out.append(s)
        r = r - s
    assert not r.any(), "the slices did not exhaust the operand"
    return out


def exact_matmul(a, b):
    """a @ b with every partial product exact in float64 (integers below 2^53 under any summation order), summed in extended
    precision: the error is that of a handful of longdouble additions, 2^-11 u relative to the largest term."""
    n = a.shape[1]
    beta = int((53 - np.ceil(np.log2(max(n, 2)))) // 2)
    total = np.zeros((a.shape[0], b.shape[1]), dtype=np.longdouble)
    for sa in _slices(a, 1, beta):
        for sb in _slices(b, 0, beta):
            total += (sa @ sb).astype(np.longdouble)
    return total


# ---- the derived checks ---------------------------------------------------------------------------------------------------------
def check_factorisation(a, lu, ipiv):
    """|l_ij| <= 1 exactly; |P A - L U| <= gamma_N |L| |U| componentwise (Higham, Thm 9.3).  -> the largest ratio"""
    n = a.shape[0]
    lo, up = split_lu(lu)
    assert np.all(np.abs(np.tril(lu, -1)) <= 1.0), "a multiplier exceeds 1"
    resid = np.abs(permute(a, ipiv).astype(np.longdouble) - exact_matmul(lo, up)).astype(np.float64)
    bound = gamma(n) * (np.abs(lo) @ np.abs(up))
    assert np.all(resid <= bound), f"|PA - LU| exceeds gamma_N |L||U| by a factor {np.max(resid / np.where(bound > 0, bound, 1))}"
    return float(np.max(resid / np.where(bound > 0, bound, np.inf)))


def check_solve(a, b, x, lu):
    """|A x - b| <= gamma_3N |L||U||x| + gamma_(N+1) (|A||x| + |b|) componentwise (Thm 9.4; the second term is the f64
    residual of this very line)"""
    n = a.shape[0]
    lo, up = split_lu(lu)
    resid = np.abs(a @ x - b)
    bound = gamma(3 * n) * (np.abs(lo) @ (np.abs(up) @ np.abs(x))) + gamma(n + 1) * (np.abs(a) @ np.abs(x) + np.abs(b))
    assert np.all(resid <= bound), f"|Ax - b| exceeds its bound by a factor {np.max(resid / np.where(bound > 0, bound, 1))}"


def check_pivots(a, ipiv, max_excluded=0.01):
    """ipiv against the restatement wherever its winning margin exceeds gamma_N (|L||U|)_jj; the share of columns left out
    by that rule is at most max_excluded."""
    n = a.shape[0]
    ref_lu, ref, margin, info = getrf(a)
    assert info == 0
    lo, up = split_lu(ref_lu)
    tol = gamma(n) * np.einsum("jk,kj->j", np.abs(lo), np.abs(up))
    if not np.all(margin > tol):  # along the device's path through the ties within rounding
        _, ref, margin, info = getrf(a, follow=ipiv, tol=tol)
        assert info == 0
    decided = margin > tol
    assert np.array_equal(np.asarray(ipiv)[decided], ref[decided]), "the pivot sequence differs where the margin decides"
    assert np.mean(~decided) <= max_excluded, f"{np.sum(~decided)} of {n} columns are ties within rounding"
