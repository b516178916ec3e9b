"""GPU tests of the gradient stage across feature scales and exact ties (run with -m gpu on an MI355X), against the
scale-free reference of tests/grad_reference.py.  corrla_grad_mat_* accepts any f64 coordinates whose squares are finite,
normal numbers, and features may differ in scale; it promises the exact nearest neighbours with equal distances ordered by
index, and the least-squares gradients.  Every other GPU test of the limited scans and fits draws O(1) coordinates and ties
between points that share their y.

Errors are in feature units (grad_reference.feature_unit_error), tolerances the project's own: 1e-9 for order 1, 1e-8 for
order 2.  Every y is iid N(0, 1): a wrong neighbour moves a gradient by >= 1e-4 (tests/test_grad_reference.py asserts it
for every query used here).  Every parametrisation holds scale 1 as its control.  Routes are forced with CORRLA_KNN and
CORRLA_FIT; tests/test_grad_reference.py pins that every row reaches what it names."""
import time

import numpy as np
import pytest

from tests import grad_reference as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import corrla_rs_amd as cr
    return cr.Context(0)


def _force(monkeypatch, knn, fit):
    for name, v in (("CORRLA_KNN", knn), ("CORRLA_FIT", fit)):
        if v:
            monkeypatch.setenv(name, str(v))
        else:
            monkeypatch.delenv(name, raising=False)


def _clear(cut):
    """queries whose n-th and (n + 1)-th distances differ by more than rounding (all of them are expected to)"""
    keep = (cut[:, 1] - cut[:, 0]) > 1e-12 * cut[:, 1]
    assert keep.mean() >= 0.95
    return keep


def _check(tag, g, nreg, ref, order, d=None, keep=None):
    keep = slice(None) if keep is None else keep
    assert g.shape == ref.shape and np.all(np.isfinite(g)), tag
    err = gr.feature_unit_error(g[:, keep], ref[:, keep], d)
    print("%s: n_regularised %d, feature-unit error %.3e" % (tag, nreg, err))
    assert nreg == 0, tag
    assert err <= gr.tolerance(order), (tag, err)


def _uniform(ctx, monkeypatch, row, e, tag):
    (k, n_nbrs, order, knn, fit), _ = row
    n_q = 32 if k == 20 else gr.N_QUERIES
    x, y, xq = gr.gaussian_cloud(k)
    ref, cut, _ = gr.reference("gauss", k, order, n_nbrs, n_q)
    s = 2.0 ** e
    _force(monkeypatch, knn, fit)
    g, nreg = ctx.grad_mat(x * s, y, order, n_nbrs, xq[:n_q] * s)
    _check("%s at 2^%d" % (tag, e), g, nreg, ref / s, order, keep=_clear(cut))      # the rescaled problem, exactly


def _ladder(ctx, monkeypatch, row, tag):
    (k, n_nbrs, order, knn, fit), _ = row
    n_q = 32 if k == 20 else gr.N_QUERIES
    x, y, xq, d = gr.ladder_cloud(k)
    ref, cut, _ = gr.reference("ladder", k, order, n_nbrs, n_q)
    _force(monkeypatch, knn, fit)
    g, nreg = ctx.grad_mat(x, y, order, n_nbrs, xq[:n_q])
    _check("%s on the units ladder" % tag, g, nreg, ref, order, d, _clear(cut))


# ---- 1. every scan over uniform scales ---------------------------------------------------------------------------------
@pytest.mark.parametrize("e", gr.UNIFORM_SCAN_EXPONENTS)
@pytest.mark.parametrize("scan", sorted(gr.SCANS))
def test_scans_find_the_exact_neighbours_at_every_uniform_scale(ctx, monkeypatch, scan, e):
    """2^-83 .. 2^83: below 2^-63 the squares leave f32's normal range, above 2^63 they leave f32 altogether; the filters
    of the two MFMA scans work on f32 images of the coordinates."""
    _uniform(ctx, monkeypatch, gr.SCANS[scan], e, "scan " + scan)


# ---- 2. every scan over features of different units --------------------------------------------------------------------
@pytest.mark.parametrize("scan", sorted(gr.LADDER_SCANS))
def test_scans_find_the_exact_neighbours_on_the_units_ladder(ctx, monkeypatch, scan):
    _ladder(ctx, monkeypatch, gr.LADDER_SCANS[scan], "scan " + scan)


# ---- 2b. a cloud with far outliers: the filters' images are scaled by the cloud's largest point ---------------------------
@pytest.mark.parametrize("e", gr.OUTLIER_EXPONENTS)
@pytest.mark.parametrize("kind", ["one", "pair"])
@pytest.mark.parametrize("scan", gr.OUTLIER_SCANS)
def test_mfma_scans_keep_the_neighbours_of_o1_points_beside_far_outliers(ctx, monkeypatch, scan, kind, e):
    """an O(1) cloud plus one point, or a +- pair (which leaves the mean where it was), of coordinates 2^80 / 2^120.  One
    scale serves the whole cloud: beside 2^80 the O(1) points' f32 products are still normal numbers, beside 2^120 they are
    not and the points have to reach the exact re-check.  The outliers come last, so the reference is that of the cloud
    without them."""
    (k, n_nbrs, order, knn, fit), _ = gr.SCANS[scan]
    x, y, xq = gr.gaussian_cloud(k)
    ref, cut, _ = gr.reference("gauss", k, order, n_nbrs, gr.N_QUERIES)
    xo, yo = gr.with_outliers(x, y, kind, e)
    _force(monkeypatch, knn, fit)
    g, nreg = ctx.grad_mat(xo, yo, order, n_nbrs, xq)
    _check("scan %s, %s outlier(s) at 2^%d" % (scan, kind, e), g, nreg, ref, order, keep=_clear(cut))


# ---- 3. exact ties: equal distances -> lower index ----------------------------------------------------------------------
@pytest.mark.parametrize("n_nbrs", gr.LATTICE_NBRS)
@pytest.mark.parametrize("scan", sorted(gr.TIE_SCANS))
def test_ties_on_the_integer_lattice_go_to_the_lower_index(ctx, monkeypatch, scan, n_nbrs):
    """{0..20}^3 shuffled: distances are exact integers and the cut falls inside a tied shell for nearly every query; a scan
    that breaks ties any other way is off by >= 7e-3"""
    x, y, xq = gr.lattice_cloud()
    ref, _, _ = gr.reference("lattice", 3, 1, n_nbrs, 128)
    _force(monkeypatch, gr.TIE_SCANS[scan], 0)
    g, nreg = ctx.grad_mat(x, y, 1, n_nbrs, xq)
    _check("lattice, scan %s, %d neighbours" % (scan, n_nbrs), g, nreg, ref, 1)


@pytest.mark.parametrize("k", sorted(gr.INTEGER_CLOUDS))
@pytest.mark.parametrize("scan", sorted(gr.TIE_SCANS))
def test_ties_in_integer_clouds_go_to_the_lower_index(ctx, monkeypatch, scan, k):
    """coordinates in {-2..2}: at k = 40 and 64 the bf16 scan runs two MFMA steps and the f32-MFMA scan its 16 slices"""
    n_nbrs = gr.INTEGER_CLOUDS[k]
    x, y, xq = gr.integer_cloud(k)
    ref, _, _ = gr.reference("integer", k, 1, n_nbrs, gr.N_QUERIES)
    _force(monkeypatch, gr.TIE_SCANS[scan], 0)
    g, nreg = ctx.grad_mat(x, y, 1, n_nbrs, xq)
    _check("integer cloud k = %d, scan %s" % (k, scan), g, nreg, ref, 1)


@pytest.mark.parametrize("k", sorted(gr.PAIRED_CLOUDS))
@pytest.mark.parametrize("scan", sorted(gr.TIE_SCANS))
def test_ties_between_the_two_copies_of_a_point_go_to_the_lower_index(ctx, monkeypatch, scan, k):
    """every point twice, an odd number of neighbours: every query's cut separates the two copies of one point"""
    n_nbrs = gr.PAIRED_CLOUDS[k][1]
    x, y, xq = gr.paired_cloud(k)
    ref, _, _ = gr.reference("paired", k, 1, n_nbrs, gr.N_QUERIES)
    _force(monkeypatch, gr.TIE_SCANS[scan], 0)
    g, nreg = ctx.grad_mat(x, y, 1, n_nbrs, xq)
    _check("paired cloud k = %d, scan %s" % (k, scan), g, nreg, ref, 1)


# ---- 4. every fit over scales, behind the VALU scan -------------------------------------------------------------------------
@pytest.mark.parametrize("e", gr.UNIFORM_FIT_EXPONENTS)
@pytest.mark.parametrize("fit", sorted(gr.FITS))
def test_fits_solve_full_rank_designs_at_every_uniform_scale(ctx, monkeypatch, fit, e):
    """a feature's spread among the neighbours enters the normal equations squared (to the fourth power for the quadratic
    columns) beside the constant column's n_nbrs: the pivot test has to be relative to each column's own scale"""
    _uniform(ctx, monkeypatch, gr.FITS[fit], e, "fit " + fit)


@pytest.mark.parametrize("fit", sorted(gr.FITS))
def test_fits_solve_full_rank_designs_on_the_units_ladder(ctx, monkeypatch, fit):
    _ladder(ctx, monkeypatch, gr.FITS[fit], "fit " + fit)


@pytest.mark.parametrize("fit_mode", [0, 2])
@pytest.mark.parametrize("order,k,n_nbrs", [(1, 8, 30), (2, 5, 40)])
def test_rank_deficient_designs_are_still_reported_at_other_scales(ctx, monkeypatch, order, k, n_nbrs, fit_mode):
    """the cloud of test_wide_fit_reports_rank_deficient_designs_like_the_limited_fits (a constant feature, duplicated rows):
    the count of regularised queries at 2^-20 and 2^27 is the one at scale 1, and the gradients stay finite"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((600, k)) + 0.5
    x[:, 3] = 1.25
    x[300:400] = x[:100]
    y = rng.standard_normal(600)
    _force(monkeypatch, 1, fit_mode)
    counts = {}
    for e in (0, -20, 27):
        s = 2.0 ** e
        g, counts[e] = ctx.grad_mat(x * s, y, order, n_nbrs, x[:40] * s)
        assert np.all(np.isfinite(g)), e
    print("rank-deficient designs, order %d, CORRLA_FIT=%d: regularised" % (order, fit_mode), counts)
    assert counts[0] == 40 and counts[-20] == counts[0] and counts[27] == counts[0]


# ---- 5. no silent degeneration: the filter still filters ---------------------------------------------------------------
def test_the_bf16_filter_still_filters_at_extreme_scales(ctx, monkeypatch):
    """the shape of test_non_finite_support_points_never_become_neighbours_and_do_not_slow_the_scan and its bound: a scan that
    passed every pair to the exact re-check at 2^83 or 2^-83 would be right, and ~100 times slower"""
    rng = np.random.default_rng(31)
    n, k, n_nbrs, nq = 60_000, 16, 40, 512
    x = rng.standard_normal((n, k))
    y = rng.standard_normal(n)
    xq = x[rng.permutation(n)[:nq]]
    monkeypatch.setenv("CORRLA_KNN", "3")
    monkeypatch.delenv("CORRLA_FIT", raising=False)
    ctx.grad_mat(x, y, 1, n_nbrs, xq[:8])                     # warm-up (code object, workspaces)
    took, grads = {}, {}
    for e in (0, 83, -83):
        s = 2.0 ** e
        xs, xqs = x * s, xq * s
        t0 = time.perf_counter()
        grads[e], nreg = ctx.grad_mat(xs, y, 1, n_nbrs, xqs)
        took[e] = time.perf_counter() - t0
        assert nreg == 0, e
    print("bf16-filter scan, 60000 x 16, 512 queries: %s s" % {e: round(t, 4) for e, t in took.items()})
    for e in (83, -83):
        assert np.max(np.abs(grads[e] * 2.0 ** e - grads[0])) <= 1e-9 * np.abs(grads[0]).max(), e
        assert took[e] < 5.0 * took[0] + 0.5, took


# ---- 6. end to end -------------------------------------------------------------------------------------------------------
def test_fit_svd_on_a_units_ladder(ctx, monkeypatch):
    """The Python surface on a cloud whose features span 2^-30 .. 2^30, defaults throughout.  PolyGradientEstimator.grad_mat:
    all 400 gradients in feature units, so that an error in an O(1) or a large feature shows.  ActiveSsRsvd.fit_svd: the
    singular values are the roots of the eigenvalues of G G^T / n of the reference gradients, at the tolerance of
    test_fit_svd_at_128_features -- relative to the largest, which the small-scale features' slopes dominate."""
    from corrla_rs_amd.callers import ActiveSsRsvd, PolyGradientEstimator
    monkeypatch.delenv("CORRLA_KNN", raising=False)
    monkeypatch.delenv("CORRLA_FIT", raising=False)
    k, n_nbrs, n, r = gr.FIT_SVD_LADDER
    x, y, _, d = gr.ladder_cloud(k)
    xs = x[:n]
    ref, _, _ = gr.reference("ladder-all", k, 1, n_nbrs, n)
    est = PolyGradientEstimator(x, y, 1, n_nbrs, ctx=ctx)
    _check("grad_mat on the units ladder, %d queries" % n, est.grad_mat(xs), est.n_regularised, ref, 1, d)
    fit = ActiveSsRsvd(est, r, ctx=ctx).fit_svd(xs, seed=4)
    w = np.sort(np.linalg.eigvalsh(ref @ ref.T / n))[::-1]
    s = np.diag(fit.singular_vals())
    print("fit_svd on the ladder: s^2", s ** 2, "eigenvalues", w[:r])
    assert np.max(np.abs(s - np.sqrt(w[:r]))) <= 1e-8 * np.sqrt(w[0])
