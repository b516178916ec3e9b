"""CPU tests of tests/grad_reference.py alone: the conditions tests/test_gpu_grad_scales.py rests on, asserted on the very
clouds and queries it uses.  Nothing here calls the library."""
import numpy as np
import pytest

from tests import grad_reference as gr
from tests.test_grad_plan import old_routing


def _oracle(x, y, xq, order, n_nbrs):
    from oracle import active_ss_oracle as aso
    est = aso.PolyGradientEstimator(x, y, order, n_nbrs)
    est.exact_quad_gradient = order == 2
    return aso.create_grad_mat(est, xq)


# ---- the helper is the oracle at unit scale ---------------------------------------------------------------------------
@pytest.mark.parametrize("order,n_nbrs", [(1, 12), (1, 30), (2, 30), (2, 70)])
def test_reference_equals_the_oracle_on_the_lattice(order, n_nbrs):
    x, y, xq = gr.lattice_cloud()
    g, _ = gr.gradients(x, y, xq[:24], order, n_nbrs)
    err = gr.feature_unit_error(g, _oracle(x, y, xq[:24], order, n_nbrs))
    print("lattice order %d, %d neighbours: %.2e" % (order, n_nbrs, err))
    assert err <= 1e-10


@pytest.mark.parametrize("k,order,n_nbrs", [(6, 1, 12), (40, 1, 60), (3, 2, 14)])
def test_reference_equals_the_oracle_on_a_gaussian_cloud(k, order, n_nbrs):
    x, y, xq = gr.gaussian_cloud(k)
    g, _ = gr.gradients(x, y, xq[:16], order, n_nbrs)
    assert gr.feature_unit_error(g, _oracle(x, y, xq[:16], order, n_nbrs)) <= 1e-10


def test_reference_is_exact_under_power_of_two_scaling():
    x, y, xq = gr.gaussian_cloud(6)
    g, _ = gr.gradients(x, y, xq[:8], 1, 12)
    for e in (-83, 62):
        s = 2.0 ** e
        gs, _ = gr.gradients(x * s, y, xq[:8] * s, 1, 12)
        assert np.array_equal(gs, g / s)


# ---- tie clouds: the cut falls inside a tied shell, and a wrong tie rule shows ---------------------------------------
def _tie_conditions(cloud, k, n_nbrs, n_q):
    g, cut, _ = gr.reference(cloud, k, 1, n_nbrs, n_q)
    gs, _, _ = gr.reference(cloud, k, 1, n_nbrs, n_q, swap=True)
    moved = np.max(np.abs(gs - g), axis=0) / np.max(np.abs(g), axis=0)   # per query
    tied = int(np.sum(cut[:, 0] == cut[:, 1]))
    print("%s k = %d, %d neighbours: %d of %d queries cut a tied shell; a swapped neighbour moves the gradient by >= %.1e"
          % (cloud, k, n_nbrs, tied, n_q, moved.min()))
    assert tied >= 0.8 * n_q
    assert moved.min() >= 1e-4


@pytest.mark.parametrize("n_nbrs", gr.LATTICE_NBRS)
def test_lattice_queries_cut_tied_shells_and_see_a_swapped_neighbour(n_nbrs):
    _tie_conditions("lattice", 3, n_nbrs, 128)


@pytest.mark.parametrize("k", sorted(gr.INTEGER_CLOUDS))
def test_integer_cloud_queries_cut_tied_shells_and_see_a_swapped_neighbour(k):
    _tie_conditions("integer", k, gr.INTEGER_CLOUDS[k], gr.N_QUERIES)


@pytest.mark.parametrize("k", sorted(gr.PAIRED_CLOUDS))
def test_paired_cloud_queries_cut_a_pair_and_see_a_swapped_neighbour(k):
    n_nbrs = gr.PAIRED_CLOUDS[k][1]
    g, cut, _ = gr.reference("paired", k, 1, n_nbrs, gr.N_QUERIES)
    gs, _, _ = gr.reference("paired", k, 1, n_nbrs, gr.N_QUERIES, swap=True)
    moved = np.max(np.abs(gs - g), axis=0) / np.max(np.abs(g), axis=0)
    print("paired cloud k = %d, %d neighbours: a swapped copy moves the gradient by >= %.1e" % (k, n_nbrs, moved.min()))
    assert np.all(cut[:, 0] == cut[:, 1])
    assert moved.min() >= 1e-4


def test_outliers_leave_the_reference_of_the_o1_queries_alone():
    x, y, xq = gr.gaussian_cloud(5)
    g, _, _ = gr.reference("gauss", 5, 1, 12, 16)
    for kind in ("one", "pair"):
        for e in gr.OUTLIER_EXPONENTS:
            xo, yo = gr.with_outliers(x, y, kind, e)
            assert np.array_equal(gr.gradients(xo, yo, xq[:16], 1, 12)[0], g)


def test_fit_svd_ladder_queries_have_a_clear_cut_and_see_a_swapped_neighbour():
    k, n_nbrs, n_q, _ = gr.FIT_SVD_LADDER
    g, cut, d = gr.reference("ladder-all", k, 1, n_nbrs, n_q)
    gs, _, _ = gr.reference("ladder-all", k, 1, n_nbrs, n_q, swap=True)
    assert np.all((cut[:, 1] - cut[:, 0]) > 1e-12 * cut[:, 1])
    moved = np.max(np.abs(gs - g) * d[:, None], axis=0) / np.max(np.abs(g) * d[:, None], axis=0)
    assert moved.min() >= 1e-4


# ---- Gaussian and ladder clouds: no near-ties at the cut (a scan may then order by rounding), a swap shows -----------------
def _rows():
    rows = {("gauss", c[0], c[2], c[1]) for c, _ in list(gr.SCANS.values()) + list(gr.FITS.values())}
    rows |= {("ladder", c[0], c[2], c[1]) for c, _ in list(gr.LADDER_SCANS.values()) + list(gr.FITS.values())}
    return sorted(rows)


@pytest.mark.parametrize("cloud,k,order,n_nbrs", _rows())
def test_gaussian_and_ladder_queries_have_a_clear_cut_and_see_a_swapped_neighbour(cloud, k, order, n_nbrs):
    n_q = 32 if k == 20 else gr.N_QUERIES
    g, cut, d = gr.reference(cloud, k, order, n_nbrs, n_q)
    gap = (cut[:, 1] - cut[:, 0]) / cut[:, 1]
    assert np.mean(gap <= 1e-12) <= 0.05            # (the GPU tests drop such queries; none is expected)
    gs, _, _ = gr.reference(cloud, k, order, n_nbrs, n_q, swap=True)
    dd = np.ones(k) if d is None else d
    moved = np.max(np.abs(gs - g) * dd[:, None], axis=0) / np.max(np.abs(g) * dd[:, None], axis=0)
    print("%s k = %d order %d, %d neighbours: smallest gap %.1e, a swapped neighbour moves the gradient by >= %.1e"
          % (cloud, k, order, n_nbrs, gap.min(), moved.min()))
    assert moved.min() >= 1e-4


# ---- every row of the GPU file reaches what it names ------------------------------------------------------------------
def test_rows_reach_the_kernels_they_name():
    for table in (gr.SCANS, gr.LADDER_SCANS, gr.FITS):
        for name, ((k, n, order, knn, fit), exp) in table.items():
            if knn == 4 or fit == 2:     # the wide kernels are forced by the knob itself
                continue
            scan, fitr = old_routing(3000, k, gr.N_QUERIES, order, n, knn, fit)
            got = scan[:4] if len(exp) == 4 else fitr[:2]
            assert got == exp, (name, scan, fitr)
    tie_rows = [(9000, k, n) for k, n in gr.INTEGER_CLOUDS.items()] + [(9261, 3, n) for n in gr.LATTICE_NBRS]
    tie_rows += [(2 * n, k, nn) for k, (n, nn) in gr.PAIRED_CLOUDS.items()]
    for n_pts, k, n in tie_rows:
        for knn in (1, 2, 3):
            assert old_routing(n_pts, k, 64, 1, n, knn, 0)[0][0] == {1: "valu", 2: "mfma", 3: "knn2"}[knn]
    # the integer clouds at k = 40 and 64 take the two-step bf16 scan and the 16-slice f32-MFMA scan
    assert old_routing(9000, 64, 64, 1, 80, 3, 0)[0][3] == 2 and old_routing(9000, 40, 64, 1, 60, 2, 0)[0][2] == 16


# ---- finding 1, as it was: the raw pivot rule rejects full-rank designs -------------------------------------------------
def test_the_raw_pivot_rule_rejected_full_rank_designs():
    """grad_fit_kernel and grad_fit_lin_kernel tested every Cholesky pivot of the RAW normal equations of [x - x0, 1]
    against 1e-13 max diag, and the constant column's diagonal is n_nbrs.  k = 6, 40 neighbours of spread 0.1."""
    rng = np.random.default_rng(6)
    dx = 0.1 * rng.standard_normal((40, 6))
    assert np.linalg.matrix_rank(gr.design(dx, 1)) == 7
    for e in (-4, 0, 4):
        assert gr.raw_pivot_rule_accepts(gr.design(dx * 10.0 ** e, 1))
    for scale in (1e-6, 1e-9, 1e8, 1e12):                                     # uniform scales
        assert not gr.raw_pivot_rule_accepts(gr.design(dx * scale, 1))
    mixed = dx.copy()
    mixed[:, 2] *= 1e-6                                                       # one small feature beside O(1) ones
    assert not gr.raw_pivot_rule_accepts(gr.design(mixed, 1))
    # order 2: the columns carry the fourth power of the spread
    dx2 = 0.1 * rng.standard_normal((40, 3))
    assert gr.raw_pivot_rule_accepts(gr.design(dx2, 2))
    assert not gr.raw_pivot_rule_accepts(gr.design(dx2 * 1e-3, 2))            # spread 1e-4
    # equilibrated (unit column norms), the same rule accepts every one of them
    for dsg in (gr.design(dx * 1e-9, 1), gr.design(dx * 1e12, 1), gr.design(mixed, 1), gr.design(dx2 * 1e-3, 2)):
        assert gr.raw_pivot_rule_accepts(dsg / np.linalg.norm(dsg, axis=0))
