"""GPU tests of the gradient stage's wide kernels (grad_wide_kernels.hpp; run with -m gpu on an MI355X): calls beyond the
limited kernels' k <= 64 / n_nbrs <= 512 / 160 KiB of LDS against the oracle, and the wide scan and fit forced
(CORRLA_KNN=4, CORRLA_FIT=2) on calls the limited kernels serve, against those kernels."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import corrla_rs_amd as cr
    return cr.Context(0)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.abs(b).max())


def _cloud(rng, n, k, offset=0.5):
    return rng.standard_normal((n, k)) + offset


# ---- 1. beyond today's limits, against the oracle -------------------------------------------------------------------
@pytest.mark.parametrize("k,n_nbrs,n_pts,nq", [(96, 120, 6000, 64), (64, 1024, 20000, 32), (300, 400, 5000, 24),
                                               (1024, 1100, 3000, 8)])
def test_order1_beyond_the_limits_matches_the_oracle(ctx, k, n_nbrs, n_pts, nq):
    from oracle import active_ss_oracle as aso
    rng = np.random.default_rng(k + n_nbrs)
    x = _cloud(rng, n_pts, k)
    b = rng.standard_normal(k)
    y = np.sin(x @ b / np.sqrt(k)) + 0.1 * (x[:, 0] ** 2)
    xq = x[rng.choice(n_pts, nq, replace=False)]
    g, nreg = ctx.grad_mat(x, y, 1, n_nbrs, xq)
    assert g.shape == (k, nq) and nreg == 0
    go = aso.create_grad_mat(aso.PolyGradientEstimator(x, y, 1, n_nbrs), xq)
    assert _rel(g, go) <= 1e-9
    if k == 1024:   # an affine function: exact slopes at every query
        g2, _ = ctx.grad_mat(x, x @ b + 2.0, 1, n_nbrs, xq)
        assert np.max(np.abs(g2 - b[:, None])) <= 1e-9 * np.abs(b).max()


@pytest.mark.parametrize("k,n_nbrs,n_pts,nq,n_oracle", [(32, 1200, 4000, 6, 6), (40, 1800, 5000, 4, 4), (64, 2400, 6000, 3, 2)])
def test_order2_beyond_the_limits(ctx, k, n_nbrs, n_pts, nq, n_oracle):
    from oracle import active_ss_oracle as aso
    rng = np.random.default_rng(k)
    x = _cloud(rng, n_pts, k)
    qm = rng.standard_normal((k, k)) * 0.1
    qm = qm + qm.T
    b = rng.standard_normal(k)
    y = 0.5 * np.einsum("ni,ij,nj->n", x, qm, x) + x @ b + 3.0 + 1e-3 * np.sin(x @ b)
    g, nreg = ctx.grad_mat(x, y, 2, n_nbrs, x[:nq])
    assert g.shape == (k, nq) and nreg == 0
    est = aso.PolyGradientEstimator(x, y, 2, n_nbrs)
    est.exact_quad_gradient = True
    go = aso.create_grad_mat(est, x[:n_oracle])
    assert _rel(g[:, :n_oracle], go) <= 1e-7
    # an exact quadratic with an offset is recovered
    y2 = 0.5 * np.einsum("ni,ij,nj->n", x, qm, x) + x @ b + 3.0
    g2, _ = ctx.grad_mat(x, y2, 2, n_nbrs, x[:nq])
    assert np.max(np.abs(g2 - (x[:nq] @ qm + b).T)) <= 1e-6 * np.abs(g2).max()


# ---- 2. the wide scan against the VALU scan on calls both serve ------------------------------------------------------
def _clouds(rng, n, k):
    gauss = rng.standard_normal((n, k))
    dup = rng.standard_normal((n, k))
    dup[n // 3: n // 3 + n // 4] = dup[: n // 4]               # exact duplicates: tied distances
    clus = (rng.standard_normal((n, k)) * 0.05 + rng.integers(0, 4, (n, 1)) * 1.0)
    off = rng.standard_normal((n, k)) * 0.01 + 1000.0
    bad = rng.standard_normal((n, k))
    bad[7, 2], bad[100, 0], bad[n - 3, k - 1] = np.nan, np.inf, -np.inf
    return {"gauss": gauss, "dup": dup, "clustered": clus, "offset": off, "nonfinite": bad}


@pytest.mark.parametrize("k,n_nbrs", [(5, 12), (5, 60), (24, 60), (24, 128), (64, 128), (64, 480)])
def test_wide_scan_matches_the_valu_scan(ctx, monkeypatch, k, n_nbrs):
    rng = np.random.default_rng(10 * k + n_nbrs)
    n = 3000
    for name, x in _clouds(rng, n, k).items():
        fin = np.all(np.isfinite(x), axis=1)
        y = np.where(fin, np.cos(np.nan_to_num(x) @ np.linspace(0.1, 1.0, k)), 0.0)
        xq = x[fin][:: max(1, n // 101)][:101]              # 101 queries: not a multiple of the 64-query tile
        monkeypatch.setenv("CORRLA_KNN", "1")
        g1, r1 = ctx.grad_mat(x, y, 1, n_nbrs, xq)
        monkeypatch.setenv("CORRLA_KNN", "4")
        g4, r4 = ctx.grad_mat(x, y, 1, n_nbrs, xq)
        assert r1 == r4, name
        assert np.max(np.abs(g4 - g1)) <= 1e-12 * np.abs(g1).max(), name


# ---- 3. the wide fit against the limited fits -------------------------------------------------------------------------
@pytest.mark.parametrize("order,k,n_nbrs,tol", [(1, 64, 90, 1e-10), (1, 6, 12, 1e-10), (2, 9, 80, 1e-9), (2, 20, 260, 1e-9)])
def test_wide_fit_matches_the_limited_fits(ctx, monkeypatch, order, k, n_nbrs, tol):
    rng = np.random.default_rng(order * 100 + k)
    x = _cloud(rng, 4000, k)
    y = np.exp(0.3 * np.sin(x @ np.linspace(-1, 1, k))) + 0.05 * np.sum(x ** 2, axis=1)
    xq = x[:77]
    g0, r0 = ctx.grad_mat(x, y, order, n_nbrs, xq)
    monkeypatch.setenv("CORRLA_FIT", "2")
    g2, r2 = ctx.grad_mat(x, y, order, n_nbrs, xq)
    assert r0 == r2 == 0
    assert _rel(g2, g0) <= tol


@pytest.mark.parametrize("order,k,n_nbrs", [(1, 8, 30), (2, 5, 40)])
def test_wide_fit_reports_rank_deficient_designs_like_the_limited_fits(ctx, monkeypatch, order, k, n_nbrs):
    rng = np.random.default_rng(5)
    x = _cloud(rng, 600, k)
    x[:, 3] = 1.25                                           # a constant feature
    x[300:400] = x[:100]                                     # duplicated neighbours
    y = np.sin(x.sum(axis=1))
    g0, r0 = ctx.grad_mat(x, y, order, n_nbrs, x[:40])
    monkeypatch.setenv("CORRLA_FIT", "2")
    g2, r2 = ctx.grad_mat(x, y, order, n_nbrs, x[:40])
    assert r0 == r2 == 40
    assert np.all(np.isfinite(g2))


# ---- 4. coordinate scale ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-25, 1e25])
def test_wide_path_at_extreme_coordinate_scales(ctx, scale):
    from oracle import active_ss_oracle as aso
    rng = np.random.default_rng(80)
    k, n_nbrs = 80, 100
    x = _cloud(rng, 3000, k)
    y = np.sin(x @ np.linspace(0.2, 1.0, k) / 8.0)
    xs = x * scale
    g, nreg = ctx.grad_mat(xs, y, 1, n_nbrs, xs[:16])
    assert nreg == 0
    go = aso.create_grad_mat(aso.PolyGradientEstimator(x, y, 1, n_nbrs), x[:16]) / scale   # the rescaled problem
    assert _rel(g, go) <= 1e-9


# ---- 5. edge shapes ---------------------------------------------------------------------------------------------------
def test_edge_shapes(ctx):
    import torch
    from oracle import active_ss_oracle as aso
    rng = np.random.default_rng(65)
    # k = 65: one past the limited kernels
    x = _cloud(rng, 2000, 65)
    y = np.sin(x @ np.linspace(0.1, 1, 65) / 4)
    g, _ = ctx.grad_mat(x, y, 1, 90, x[:10])
    assert _rel(g, aso.create_grad_mat(aso.PolyGradientEstimator(x, y, 1, 90), x[:10])) <= 1e-9
    # n_nbrs == n_pts: every point is a neighbour of every query (and queries that are not support points)
    x = _cloud(rng, 700, 70)
    y = np.cos(x @ np.linspace(-1, 1, 70) / 5)
    xq = _cloud(rng, 5, 70) * 0.7
    g, _ = ctx.grad_mat(x, y, 1, 700, xq)
    assert _rel(g, aso.create_grad_mat(aso.PolyGradientEstimator(x, y, 1, 700), xq)) <= 1e-9
    # a device-resident torch cloud at k = 128
    x = _cloud(rng, 4000, 128)
    y = np.sin(x @ np.linspace(0.1, 1, 128) / 8)
    xt, yt = torch.tensor(x, device="cuda:0"), torch.tensor(y, device="cuda:0")
    g, _ = ctx.grad_mat(xt, yt, 1, 200, xt[:40])
    assert g.is_cuda and tuple(g.shape) == (128, 40)
    t = ctx.timings()
    assert t["knn_ms"] > 0 and t["fit_ms"] > 0
    go = aso.create_grad_mat(aso.PolyGradientEstimator(x, y, 1, 200), x[:4])
    assert _rel(g.cpu().numpy()[:, :4], go) <= 1e-9


# ---- 6. the public surface end to end ---------------------------------------------------------------------------------
def test_active_ss_at_100_features(ctx):
    from corrla_rs import active_ss
    from oracle import active_ss_oracle as aso
    rng = np.random.default_rng(100)
    x = rng.standard_normal((8000, 100))
    y = 0.5 * (x[:, :5] ** 2) @ np.array([5.0, 4.0, 3.0, 2.0, 1.0]) + 0.01 * np.sin(x[:, 5:] @ np.linspace(0, 1, 95))
    comps, svals, sensi = active_ss(x, y, 1, 150, 5)
    est = aso.PolyGradientEstimator(x, y, 1, 150)
    vo, so = aso.fit(est, x)
    sensi_o = aso.var_diag_evd_sensi(vo, so)   # over all k eigenpairs, as the fitted object computes it
    assert np.max(np.abs(np.diag(svals)[:5] - np.diag(so)[:5])) <= 1e-8 * so[0, 0]
    # the 5-dimensional subspace (well separated from the sixth eigenvalue): projector difference
    p, po = comps @ comps.T, vo[:, :5] @ vo[:, :5].T
    assert np.max(np.abs(p - po)) <= 1e-6
    assert np.max(np.abs(sensi - sensi_o)) <= 1e-8 * np.abs(sensi_o).max()


def test_fit_svd_at_128_features(ctx):
    from corrla_rs_amd.callers import ActiveSsRsvd, PolyGradientEstimator
    from oracle import active_ss_oracle as aso
    rng = np.random.default_rng(128)
    k, n = 128, 3000
    x = rng.standard_normal((n, k))
    y = np.sin(x @ np.linspace(0.5, -0.5, k) / 6.0) + 0.05 * x[:, 0] * x[:, 1]
    omega = rng.standard_normal((k, 8 + 10))
    fit = ActiveSsRsvd(PolyGradientEstimator(x, y, 1, 160, ctx=ctx), 8, ctx=ctx).fit_svd(x, omega=omega)
    uo, so = aso.fit_svd(aso.PolyGradientEstimator(x, y, 1, 160), x, 8, omega=omega)
    s, so = np.diag(fit.singular_vals()), np.diag(so)
    assert np.max(np.abs(s - so)) <= 1e-8 * so[0]
