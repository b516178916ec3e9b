"""l x l cores by design, handed to the core SVD through the public rsvd entry (TEST INFRASTRUCTURE).

For an upper-triangular R the call  rsvd([R; 0], k = l, q = 0, p = 0, omega = I_l)  sketches Y = A itself, the thin-Q leaves
B = Q^T A with B B^T = R R^T up to rounding, and the core the Jacobi kernels see is the triangular factor of that Gram:
the transposed Cholesky factor of R R^T (driver.hpp: the core is formed transposed).  With k = l nothing is truncated, so S
against numpy's f64 svd(R), U diag(S) V^T = A and the orthonormality of U and of the square V^T do not depend on how a
degenerate cluster is split.

Families (each a function of l; `case` adds the element type):
  equicorr(rho)     R R^T = (1 - rho) I + rho 1 1^T: one large and an (l - 1)-fold equal singular value
  kahan(cond)       diag(s^i) (I - c triu(1, 1)), theta by bisection so that cond(R) is the requested value: graded and
                    triangular, the smallest diagonal entry far above the smallest singular value
  scaled_perm_diag  P^T diag(d) P, d log-spaced 1 .. 1e-3, P a seeded permutation: diagonal, unsorted -- no rotation at all
  two_level         triangular QR factor of diag(1 .. 1, 1e-2 .. 1e-2) Q0, Q0 a seeded orthogonal matrix: two clusters of l / 2
  scale(family, e)  family * 2^e: the power-of-two prescale of the Jacobi kernels and the ldexp on output
  identity(e)       2^e I, e = -/+ the scale exponent and 24: a Gram that is exactly 4^e I -- after the thin-Q's power-of-four
                    prescale it IS the identity, which the first-order series branch of chol_inv_kernel must not take for
                    the Gram it was given (2^24: just outside the window in which a Gram is left unscaled)

tests/test_core_cases_host.py proves on the CPU that the oracle and the emulated driver meet every bound `check` applies."""
import functools

import numpy as np

from tests.helpers import orth_err

# element type -> (cond of the Kahan core, exponent of the scaled cores)
KAHAN_COND = {np.float32: 300.0, np.float64: 1e5}
SCALE_EXP = {np.float32: 60, np.float64: 400}
# the W-only window of the multi-workgroup block Jacobi (jacobi_mc_kernels.hpp: kJmcFastCond, kJmcVerifyCond)
FAST_COND, VERIFY_COND = 16.0, 64.0
EQUICORR_RHO = 0.99        # chosen W-only from the diagonal, refused by the computed sigma (l >= 96)
EQUICORR_RHO_KEPT = 0.5    # chosen and kept


def equicorr_gram(l, rho):
    return (1.0 - rho) * np.eye(l) + rho * np.ones((l, l))


def equicorr(l, rho):
    """Upper triangular with R R^T = equicorr_gram: the reverse Cholesky J chol(J G J) J."""
    g = equicorr_gram(l, rho)
    return np.linalg.cholesky(g[::-1, ::-1])[::-1, ::-1].copy()


def _kahan(l, theta):
    s, c = np.sin(theta), np.cos(theta)
    return (s ** np.arange(l))[:, None] * (np.eye(l) - c * np.triu(np.ones((l, l)), 1))


@functools.lru_cache(maxsize=None)
def _kahan_theta(l, cond):
    lo, hi = 1e-6, np.pi / 2
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if np.linalg.cond(_kahan(l, mid)) > cond:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def kahan(l, cond):
    """cond(R(theta)) falls from infinity to 1 as theta goes from 0 to pi / 2: bisection on theta."""
    return np.ones((1, 1)) if l == 1 else _kahan(l, _kahan_theta(l, cond))


def perm_diag_values(l, seed=0):
    d = np.logspace(0.0, -3.0, l) if l > 1 else np.ones(1)
    return d[np.random.default_rng(seed + l).permutation(l)]


def scaled_perm_diag(l, seed=0):
    """diag(d) P with its rows re-sorted, P^T diag(d) P: the diagonal matrix of the permuted d."""
    return np.diag(perm_diag_values(l, seed))


def two_level_values(l):
    hi = (l + 1) // 2
    return np.concatenate([np.ones(hi), np.full(l - hi, 1e-2)])


def two_level(l, seed=0):
    q0, _ = np.linalg.qr(np.random.default_rng(seed + 7 * l).standard_normal((l, l)))
    return np.triu(np.linalg.qr(two_level_values(l)[:, None] * q0)[1])


def scale(r, e):
    return np.ldexp(r, e)


def model_core_diagonal_ratio(r):
    """max / min |diagonal| of the core the kernels see: the Cholesky factor of R R^T (what jmc_init_kernel tests against
    kJmcFastCond).  Scaled by max |R| first, so that the Gram of a 2^400 core does not overflow here."""
    rs = r / np.max(np.abs(r))
    d = np.abs(np.diag(np.linalg.cholesky(rs @ rs.T)))
    return float(d.max() / d.min())


IDENTITY_MID_EXP = 24      # Gram 2^48: outside 2^-40 .. 2^40, the core itself inside the block Jacobi's 2^-30 .. 2^30
FAMILIES = ("equicorr_kept", "scaled_perm_diag", "two_level", "two_level_down", "two_level_up", "identity_down", "identity_mid",
            "identity_up", "kahan", "equicorr")


def build(name, l, dtype):
    """The f64 design of family `name` at width l (dtype selects the Kahan condition and the scale exponent)."""
    dtype = np.dtype(dtype).type
    if name == "equicorr":
        return equicorr(l, EQUICORR_RHO)
    if name == "equicorr_kept":
        return equicorr(l, EQUICORR_RHO_KEPT)
    if name == "kahan":
        return kahan(l, KAHAN_COND[dtype])
    if name == "scaled_perm_diag":
        return scaled_perm_diag(l)
    if name == "two_level":
        return two_level(l)
    if name == "two_level_down":
        return scale(two_level(l), -SCALE_EXP[dtype])
    if name == "two_level_up":
        return scale(two_level(l), SCALE_EXP[dtype])
    if name == "identity_down":
        return scale(np.eye(l), -SCALE_EXP[dtype])
    if name == "identity_mid":
        return scale(np.eye(l), IDENTITY_MID_EXP)
    if name == "identity_up":
        return scale(np.eye(l), SCALE_EXP[dtype])
    raise KeyError(name)


def families_for(l):
    """l = 1 has no pair to rotate, no cluster and no grading: the diagonal families only."""
    return ("scaled_perm_diag", "identity_down", "identity_mid", "identity_up") if l == 1 else FAMILIES


class Case:
    """The rsvd arguments of one designed core and its f64 reference.  Computed once per (name, l, dtype), read-only."""

    def __init__(self, name, l, dtype):
        dtype = np.dtype(dtype).type
        self.name, self.l, self.dtype = name, l, dtype
        self.m = max(3 * l, 200)
        r = build(name, l, dtype).astype(dtype)
        self.a = np.zeros((self.m, l), dtype=dtype)
        self.a[:l] = r
        self.omega = np.eye(l, dtype=dtype)
        self.r = r.astype(np.float64)                       # the core as the call receives it
        self.s_ref = np.linalg.svd(self.r, compute_uv=False)
        for v in (self.a, self.omega, self.r, self.s_ref):
            v.setflags(write=False)

    @property
    def args(self):
        """(a, k, q, p) of rsvd; pass omega=case.omega"""
        return self.a, self.l, 0, 0


@functools.lru_cache(maxsize=None)
def _case(name, l, dtype_name):
    return Case(name, l, np.dtype(dtype_name))


def case(name, l, dtype):
    return _case(name, int(l), np.dtype(dtype).name)


def figures(c, u, s, vt):
    """-> (max |S - svd(R)| / sigma_1, orth_err(U), orth_err(V), ||U S V^T - A||_F / ||A||_F), all in f64."""
    u, vt = np.asarray(u, np.float64), np.asarray(vt, np.float64)
    s = np.asarray(s, np.float64).ravel()
    a = c.a.astype(np.float64)
    # (norms relative to sigma_1: 2^800 and 2^-800 squared leave f64)
    rec = (u * (s / c.s_ref[0])) @ vt - a / c.s_ref[0]
    return (float(np.max(np.abs(s - c.s_ref)) / c.s_ref[0]), orth_err(u), orth_err(vt.T),
            float(np.linalg.norm(rec) / np.linalg.norm(a / c.s_ref[0])))


def bounds(c):
    """The project's tight class (tests/test_gpu_sparse.py: _parity_sparse; tests/test_gpu_core_svd_routes.py):
    (S, orthonormality of either factor, reconstruction)."""
    f64 = c.dtype == np.float64
    return (1e-10 if f64 else 3e-5), 200 * np.finfo(c.dtype).eps * np.sqrt(c.m), (1e-8 if f64 else 1e-3)


def check(c, u, s, vt, what=""):
    """Every assertion of a designed-core case on the factors (u, s, vt) of case c."""
    u, s, vt = np.asarray(u), np.asarray(s), np.asarray(vt)
    assert u.shape == (c.m, c.l) and s.size == c.l and vt.shape == (c.l, c.l), (u.shape, s.shape, vt.shape)
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(s)) and np.all(np.isfinite(vt)), what
    sv = s.ravel()
    assert np.all(sv >= 0) and np.all(np.diff(sv) <= 0), what
    ds, ou, ov, rec = figures(c, u, s, vt)
    bs, bo, br = bounds(c)
    print("%s %s l=%d %s: dS %.2e (<= %.0e)  orth U %.2e V %.2e (<= %.2e)  rec %.2e (<= %.0e)"
          % (what, c.name, c.l, np.dtype(c.dtype).name, ds, bs, ou, ov, bo, rec, br))
    assert ds <= bs, (what, "S", ds)
    assert ou <= bo and ov <= bo, (what, "orthonormality", ou, ov)
    assert rec <= br, (what, "reconstruction", rec)
