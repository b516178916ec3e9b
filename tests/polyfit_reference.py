"""numpy restatement of the polynomial fits of the reference (src/lib_math_utils/stats_corr.rs:112-249 and mat_pinv,
src/lib_math_utils/mat_utils.rs:37-53), formula for formula: the Vandermonde matrix is stored and the pseudo-inverse divides
by s + 1e-14.  What the device path is compared against; not part of the product."""
import numpy as np


def mat_col_interactions(x, include_self_interactions=True):
    """stats_corr.rs:112-142: x_a * x_b, a outer, b from a (with the squares) or a + 1"""
    k = x.shape[1]
    cols = [x[:, a] * x[:, b] for a in range(k) for b in range(a, k) if include_self_interactions or a != b]
    return np.stack(cols, axis=1) if cols else np.zeros((x.shape[0], 0))


def build_vandermonde(x, include_self_interactions=True):
    """stats_corr.rs:201-209: [x, interactions, 1]"""
    return np.hstack([x, mat_col_interactions(x, include_self_interactions), np.ones((x.shape[0], 1))])


def build_full_vandermonde(x, degree):
    """stats_corr.rs:183-198"""
    if degree < 2:
        return np.hstack([x, np.ones((x.shape[0], 1))])
    return build_vandermonde(x, True)


def mat_pinv(v):
    """mat_utils.rs:37-53: V diag(1 / (s + 1e-14)) U^T"""
    u, s, vt = np.linalg.svd(v, full_matrices=False)
    return (vt.T * (1.0 / (s + 1.0e-14))) @ u.T


def linear_fit(x, y):
    """stats_corr.rs:146-160"""
    return mat_pinv(build_full_vandermonde(x, 1)) @ y


def jac_from_lin(x, y):
    """stats_corr.rs:164-169"""
    return linear_fit(x, y)[:x.shape[1]].T.copy()


def quad_fit(x, y):
    """stats_corr.rs:213-219"""
    return mat_pinv(build_vandermonde(x, True)) @ y


def quad_eval(x, coeffs):
    """stats_corr.rs:222-226"""
    return build_vandermonde(x, True) @ coeffs


def jac_from_quad(x0, coeffs):
    """stats_corr.rs:230-249: forward differences with eps = 1e-10, of the first coefficient column"""
    eps = 1.0e-10
    y0 = quad_eval(x0, coeffs)
    out = np.zeros(x0.shape)
    for k in range(x0.shape[1]):
        xp = x0.copy()
        xp[:, k] = xp[:, k] + eps
        out[:, k] = ((quad_eval(xp, coeffs) - y0) * (1.0 / eps))[:, 0]
    return out


def poly_sym(c, k, degree):
    """One coefficient column c (p,) as the symmetric C (k + 1, k + 1) with V(x) c = xt^T C xt, xt = [x, 1]; written with
    loops, independently of the product's vectorised form."""
    cm = np.zeros((k + 1, k + 1), dtype=c.dtype)
    for a in range(k):
        cm[a, k] = cm[k, a] = c[a] / 2
    cm[k, k] = c[-1]
    if degree >= 2:
        idx = k
        for a in range(k):
            for b in range(a, k):
                if a == b:
                    cm[a, a] = c[idx]
                else:
                    cm[a, b] = cm[b, a] = c[idx] / 2
                idx += 1
    return cm
