"""GPU test of the gradient stage's dispatch (grad_stage.hpp; run with -m gpu on an MI355X): one call per instantiation the
launchers can select -- the VALU scan, the six f32-MFMA scans, the two bf16-filter scans, the wide scan, the five order-1
fits, the general fit with its normal equations in LDS and in global memory, the wide fit -- at the smallest shapes that
reach them, each against the oracle.  tests/test_grad_plan.py pins on the CPU that every row reaches what it names."""
import numpy as np
import pytest

from tests.test_grad_plan import ROUTES, route_points

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import corrla_rs_amd as cr
    return cr.Context(0)


def _route_id(row):
    (k, n, order, knn, fit), exp = row
    scan = exp[0] + ("%dx%d" % exp[1:3] if exp[0] == "mfma" else "s%d" % exp[3] if exp[0] == "knn2" else "")
    return "%s-%s%s-k%d-n%d-o%d" % (scan, exp[4], exp[5] or "", k, n, order)


@pytest.mark.parametrize("row", ROUTES, ids=_route_id)
def test_every_route_matches_the_oracle(ctx, monkeypatch, row):
    """The tolerances of test_grad_mat_matches_the_oracle: 1e-9 of the largest gradient entry for order 1, 1e-8 against
    the exactly differentiated fitted quadratic for order 2; no query regularised."""
    from oracle import active_ss_oracle as aso
    (k, n_nbrs, order, knn, fit), _ = row
    rng = np.random.default_rng(1000 * k + n_nbrs)
    x = rng.standard_normal((route_points(k, order), k)) + 1.5
    y = np.sin(x @ rng.standard_normal(k) * 0.3) + 0.1 * (x ** 2).sum(axis=1) - 4.0
    if knn:
        monkeypatch.setenv("CORRLA_KNN", str(knn))
    if fit:
        monkeypatch.setenv("CORRLA_FIT", str(fit))
    g, nreg = ctx.grad_mat(x, y, order, n_nbrs, x[:64])
    est = aso.PolyGradientEstimator(x, y, order, n_nbrs)
    est.exact_quad_gradient = order == 2
    go = aso.create_grad_mat(est, x[:64])
    err, scale = float(np.max(np.abs(g - go))), float(np.abs(go).max())
    print("route %s: nreg %d, error %.3e of scale %.3e" % (_route_id(row), nreg, err, scale))
    assert g.shape == (k, 64) and nreg == 0
    assert err <= (1e-9 if order == 1 else 1e-8) * scale
