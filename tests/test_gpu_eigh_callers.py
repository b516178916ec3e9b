"""The callers of the device eigensolver on the GPU: quad_fit(solve="device") / polyfit_solve(device=True),
mvn_factor(device=True, eig="device") and RbfInterp(solver="eigh") (corrla_rs_amd/callers.py over Context.eigh /
Context.eigh_solve).  Run with -m gpu on an MI355X.

No tolerance is tuned.  With u = 2^-53, the device decomposition of a matrix A of order n satisfies the fixed caps of
tests/eigh_reference.py -- residual 64 n u |A|_F, orthogonality 32 n u -- so
  fits         the coefficients of the equilibrated normal equations move by at most kappa(A) 64 p u relatively, and the
               predictions V c by kappa(V) = kappa(A)^(1/2) times that relative to |y|: kappa(A)^(3/2) 64 p u, kappa over the
               directions the cut keeps;
  covariance   C - F F^T = (C V - V L) V^T + C (I - V V^T) + the dropped directions: (64 + 32 + 2) d u |C|_F in the Frobenius
               norm.  The existing caller test's componentwise bound gamma_k |F||F^T| belongs to the Cholesky factor; for a
               normwise stable decomposition its form is this norm bound;
  RBF          the predictions K_q c move by at most |K_q| |c| kappa(M) 64 N u, kappa with the regularised rule.
The defaults are pinned bitwise against the host formulas restated here."""
import numpy as np
import pytest

from tests import eigh_reference as R

pytestmark = pytest.mark.gpu
U = R.U


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx():
    import corrla_rs_amd as cr
    c = cr.Context(0)
    yield c
    c.close()


def host_polyfit_solve(g, p):
    """steps 1 to 3 of polyfit_solve as they stood before the device route, restated: the fixture of the default's bits"""
    a, b = g[:p, :p], g[:p, p:]
    d = np.sqrt(np.diag(a))
    d = np.where(d > 0.0, d, 1.0)
    w, q = np.linalg.eigh(a / np.outer(d, d))
    keep = w > p * 2.0 ** -52 * w[-1]
    qk = q[:, keep]
    return (qk @ ((qk.T @ (b / d[:, None])) / w[keep][:, None])) / d[:, None], w[keep]


def _fit_case(which):
    if which == "well_posed":       # k = 6, m = 400
        rng = np.random.default_rng(17)
        x = rng.uniform(-1.0, 1.0, (400, 6))
        y = (1.0 + x @ rng.standard_normal(6) + np.einsum("ij,jk,ik->i", x, rng.standard_normal((6, 6)), x)
             + 1e-3 * rng.standard_normal(400))[:, None]
        return x, y
    # the points of the reference's test_quad_fit: six points, six columns, V of rank 5
    x = np.array([[0.00, 0.00], [0.50, 0.00], [1.00, 0.00], [0.25, 0.25], [0.50, 0.50], [1.00, 1.00]])
    y = np.array([[0.00], [0.25], [0.50], [0.30], [0.50], [1.00]])
    return x, y


@pytest.mark.parametrize("which", ["well_posed", "rank_deficient"])
def test_quad_fit_with_the_device_solve(torch, ctx, which):
    from corrla_rs_amd import callers
    x, y = _fit_case(which)
    k = x.shape[1]
    p = k + k * (k + 1) // 2 + 1
    host = callers.quad_fit(x, y, ctx=ctx)
    dev = callers.quad_fit(x, y, ctx=ctx, solve="device")
    assert isinstance(dev, np.ndarray) and dev.shape == host.shape == (p, 1)
    assert ctx.last_eigh_route == "small" and ctx.last_eigh_info["info"] == 0
    g, _, _ = ctx.polyfit_gram(x, y, 2, normalize=True)
    _, kept = host_polyfit_solve(np.asarray(g), p)
    assert ctx.last_eigh_info["dropped"] == p - kept.size and (kept.size < p) == (which == "rank_deficient")
    kappa = kept.max() / kept.min()
    bound = kappa ** 1.5 * 64 * p * U
    ph, pd = callers.quad_eval(x, host, ctx=ctx), callers.quad_eval(x, dev, ctx=ctx)
    err = np.linalg.norm(pd - ph) / np.linalg.norm(y)
    print(f"{which}: kappa {kappa:.3e}, predictions differ by {err:.3e} |y|, bound {bound:.3e}")
    assert err <= bound
    # CUDA tensors in -> a tensor out, the same coefficients; the Gram matrix stays on the device
    dt = callers.quad_fit(torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda"), ctx=ctx, solve="device")
    assert dt.is_cuda and np.linalg.norm(callers.quad_eval(x, dt.cpu().numpy(), ctx=ctx) - ph) / np.linalg.norm(y) <= bound
    lin_h, lin_d = callers.linear_fit(x, y, ctx=ctx), callers.linear_fit(x, y, ctx=ctx, solve="device")
    assert lin_d.shape == lin_h.shape == (k + 1, 1) and np.allclose(lin_d, lin_h, rtol=0, atol=bound * np.abs(lin_h).max())
    with pytest.raises(ValueError, match="solve"):
        callers.quad_fit(x, y, ctx=ctx, solve="gpu")


def test_fit_defaults_keep_their_bits(ctx):
    from corrla_rs_amd import callers
    x, y = _fit_case("well_posed")
    g, means, scales = ctx.polyfit_gram(x, y, 2, normalize=False)
    p = 28
    want, _ = host_polyfit_solve(np.asarray(g, dtype=np.float64), p)
    for got in (callers.polyfit_solve(g, 6, 2), callers.polyfit_solve(g, 6, 2, device=False), callers.polyfit_solve(g, 6, 2, device=False, ctx=ctx)):
        assert np.array_equal(got, want)
    a = callers.quad_fit(x, y, ctx=ctx)
    assert np.array_equal(a, callers.quad_fit(x, y, ctx=ctx, solve="host")) and np.array_equal(a, callers.quad_fit(x, y, ctx=ctx))
    g, means, scales = ctx.polyfit_gram(x, y, 2, normalize=True)
    assert np.array_equal(a, callers.polyfit_solve(g, 6, 2, means, scales))


def host_factor(cov):
    """mvn_factor as it stood before the device routes, restated: the fixture of the default's bits"""
    c = np.asarray(cov, dtype=np.float64)
    d = c.shape[0]
    c = 0.5 * (c + c.T)
    sd = np.sqrt(np.diag(c).clip(min=0.0))
    sd = np.where(sd > 0.0, sd, 1.0)
    try:
        return sd[:, None] * np.linalg.cholesky(c / np.outer(sd, sd)), True
    except np.linalg.LinAlgError:
        pass
    w, v = np.linalg.eigh(c)
    keep = w > d * 2.0 ** -52 * max(float(w[-1]), 0.0)
    return v[:, keep] * np.sqrt(w[keep])[None, :], False


def _singular_cov(d=70, m=20):
    """The Gram matrix of m samples in d features whose first two features coincide, [2, 0, ..., 0]: the equilibrated matrix
    starts with [[1, 1], [1, 1]] exactly, so the pivot of column 2 is exactly zero on the host and on the device alike."""
    x = np.random.default_rng(23).standard_normal((m, d))
    x[:, 0] = x[:, 1] = 0.0
    x[0, 0] = x[0, 1] = 2.0
    cov = x.T @ x
    return np.tril(cov) + np.tril(cov, -1).T


def test_singular_covariance_factored_on_the_device(torch, ctx):
    from corrla_rs_amd import callers
    cov = _singular_cov()
    d = cov.shape[0]
    want, want_lower = callers.mvn_factor(cov)
    w0, l0 = host_factor(cov)
    assert want_lower is False and l0 is False and np.array_equal(want, w0)          # the default's bits
    bound = (64 + 32 + 2) * d * U * np.linalg.norm(cov)
    for given in (cov, torch.tensor(cov, device="cuda")):
        f, lower = callers.mvn_factor(given, device=True, ctx=ctx, eig="device")
        assert ctx.last_chol_info["info"] == 2 and ctx.last_eigh_route == "blocked" and ctx.last_eigh_info["info"] == 0
        assert lower is False and f.is_cuda and f.dtype == torch.float64
        assert tuple(f.shape) == want.shape                                            # r equals the host's
        fn = f.cpu().numpy()
        err = np.linalg.norm(cov - fn @ fn.T)
        comp = np.max(np.abs(cov - fn @ fn.T) / (np.abs(fn) @ np.abs(fn).T))
        print(f"|C - F F^T|_F {err:.3e}, bound {bound:.3e}; componentwise against |F||F^T|: {comp / U:.1f} u")
        assert err <= bound
    # eig="host" is the route as it was: the host's bits
    f, lower = callers.mvn_factor(cov, device=True, ctx=ctx)
    assert lower is False and np.array_equal(f.cpu().numpy(), want)
    # an indefinite matrix is a ValueError on the device route too, on both eigensolver routes
    bad = np.eye(70)
    bad[3, 3] = -1.0
    for m in (np.diag([1.0, -1.0, 2.0]), bad):
        with pytest.raises(ValueError, match="positive semi-definite"):
            callers.mvn_factor(m, device=True, ctx=ctx, eig="device")
    with pytest.raises(ValueError, match="eig"):
        callers.mvn_factor(cov, eig="device")
    # the samples of the device factor
    got = callers.sample_mv_normal(cov, 9, seed=3, ctx=ctx, factor="device", eig="device")
    assert isinstance(got, np.ndarray) and got.shape == (9, d) and np.all(np.isfinite(got))
    assert np.array_equal(callers.sample_mv_normal(cov, 9, seed=3, ctx=ctx), callers.sample_mv_normal(cov, 9, seed=3, ctx=ctx, factor="host"))


def _pinv_reg(m):
    u, sv, vt = np.linalg.svd(m, full_matrices=False)
    return (vt.T * (1.0 / (sv + 1.0e-14))) @ u.T


def test_rbf_interp_with_the_eigh_solver(torch, ctx):
    from corrla_rs_amd import callers
    rng = np.random.default_rng(31)
    n_s, dim = 150, 3
    x = rng.uniform(-1.0, 1.0, (n_s, dim))
    y = np.stack([np.sin(x.sum(axis=1)), x[:, 0] * x[:, 1]], axis=1)
    xq = rng.uniform(-1.0, 1.0, (40, dim))
    ref = callers.RbfInterp(3, 0.0, dim, 1, ctx=ctx)
    ref.fit(x, y)
    # the default route keeps its bits: the numpy formula restated
    r = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
    pb = np.hstack([x, np.ones((n_s, 1))])
    kp = np.vstack([np.hstack([r * r * r, pb]), np.hstack([pb.T, np.zeros((4, 4))])])
    assert np.array_equal(ref.coeffs, _pinv_reg(kp) @ np.vstack([y, np.zeros((4, 2))]))
    got = callers.RbfInterp(3, 0.0, dim, 1, ctx=ctx, solver="eigh")
    got.fit(x, y)
    assert ctx.last_eigh_route == "blocked" and ctx.last_eigh_info["info"] == 0 and ctx.last_eigh_info["dropped"] == 0
    assert isinstance(got.coeffs, np.ndarray) and got.coeffs.shape == ref.coeffs.shape == (n_s + 4, 2)
    sv = np.linalg.svd(kp, compute_uv=False)
    kappa = sv.max() / (sv.min() + 1e-14)
    upper = np.linalg.norm(ref._upper(xq), 2)
    bound = upper * np.linalg.norm(ref.coeffs) * kappa * 64 * (n_s + 4) * U
    pr, pg = ref.predict(xq), got.predict(xq)
    err = np.linalg.norm(pg - pr)
    print(f"kappa {kappa:.3e}: predictions differ by {err:.3e}, bound {bound:.3e}, |predictions| {np.linalg.norm(pr):.3e}")
    assert err <= bound
    # supports on the device: the model stays there
    gt = callers.RbfInterp(3, 0.0, dim, 1, ctx=ctx, solver="eigh")
    gt.fit(torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda"))
    assert gt.coeffs.is_cuda and np.linalg.norm(gt.predict(xq) - pr) <= bound
    # Coincident supports: the system is exactly singular (two identical rows).  "lu" raises where the two rows stay bitwise
    # equal through the elimination -- the one-workgroup route, 40 supports here; on the blocked route (150 supports) the two
    # rows pass through different kernels, the pivot comes out as rounding noise instead of zero and the solve completes on
    # it, with ``last_solve_info["min_pivot"]`` as the witness LU's docstring names.  "eigh" answers either way.
    for m_s in (40, n_s):
        x2, y2 = np.vstack([x[:m_s], x[:1]]), np.vstack([y[:m_s], y[:1]])
        lu = callers.RbfInterp(3, 0.0, dim, 1, ctx=ctx, solver="lu")
        try:
            lu.fit(x2, y2)
            raised = False
        except RuntimeError:
            raised = True
        info = ctx.last_solve_info
        print(f"coincident supports, {m_s} + 1: lu raised {raised}, route {ctx.last_solve_route}, min_pivot {info['min_pivot']:.3e}, max_u {info['max_u']:.3e}")
        assert raised or info["min_pivot"] <= 64 * (m_s + 5) * U * info["max_u"]
        if m_s == 40:
            assert raised and ctx.last_solve_route == "small"
        sing = callers.RbfInterp(3, 0.0, dim, 1, ctx=ctx, solver="eigh")
        sing.fit(x2, y2)
        ps = sing.predict(xq)
        assert np.all(np.isfinite(ps)) and np.all(np.isfinite(sing.coeffs))
        if m_s == n_s:   # the duplicated support carries the same values: the interpolant is the regular fit's
            print(f"coincident supports: predictions differ from the regular fit's by {np.linalg.norm(ps - pr):.3e}, bound {bound:.3e}")
    with pytest.raises(ValueError, match="solver"):
        callers.RbfInterp(3, 0.0, dim, 1, solver="qr")
