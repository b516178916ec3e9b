"""The RBF fit that never leaves the device: Context.rbf_system / rbf_fit (corrla_rbffit_system_*, corrla_rbffit_*,
csrc/lu_stage.hpp) and RbfInterp(solver="lu") over them.  Run with -m gpu on an MI355X.

Cases: (kernel, eps, poly_degree) in {(1, 0, 1), (2, 2.0, 1), (3, 0, 2), (4, 6.0, 1), (4, 6.0, None)} at (n_s, dim) = (97, 2)
and (700, 3), the supports uniform on [-1, 1]^dim, three right-hand sides; (1100, 3) for the cubic kernel only.  The system's
condition number runs from 4e2 to 3e10.  On the CPU, with the restatement of tests/lu_reference.py alone, at most 1 % of the
columns of these systems are pivot ties within rounding (7 of 704 for the Gaussian with its linear tail, none for most).

Bitwise: the K block against Context.rbf_matrix(x, x), P and P^T against _poly_block (one rounding per product), the corner
zero, rbf_fit against solve(rbf_system(x), [y; 0]), predict of an "lu" model against rbf_apply with its coefficients, and the
default RbfInterp against the unchanged numpy formula of the pseudo-inverse route.
Derived: the coefficients satisfy the solve bound of tests/test_gpu_lu.py against the system, and
  ||c_lu - c_pinv||_inf / ||c_pinv||_inf <= 2 kappa_inf(M) (eta_lu + eta_pinv)
with kappa_inf from numpy.linalg.cond and each eta the normwise backward error ||M c - b||_inf / (||M||_inf ||c||_inf +
||b||_inf), computed by the same code for both, column by column."""
import functools

import numpy as np
import pytest

from tests import lu_reference as R
from tests.test_gpu_lu import solve_dev

pytestmark = pytest.mark.gpu

KERNELS = ((1, 0.0, 1), (2, 2.0, 1), (3, 0.0, 2), (4, 6.0, 1), (4, 6.0, None))
SHAPES = ((97, 2), (700, 3))
CASES = [(k, s) for s in SHAPES for k in KERNELS] + [((3, 0.0, 2), (1100, 3))]
N_RHS = 3


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


@functools.lru_cache(maxsize=None)
def _data(n_s, dim):
    rng = np.random.default_rng(n_s + dim)
    x = rng.uniform(-1.0, 1.0, (n_s, dim))
    y = np.stack([np.sin(2.0 * x.sum(axis=1)), (x ** 2).sum(axis=1), rng.standard_normal(n_s)], axis=1)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _n_poly(dim, degree):
    return 0 if degree is None else (dim + 1 if degree < 2 else dim + dim * (dim + 1) // 2 + 1)


def _eta(m, c, b):
    """normwise backward error of every column"""
    norm_m = np.abs(m).sum(axis=1).max()
    return np.abs(m @ c - b).max(axis=0) / (norm_m * np.abs(c).max(axis=0) + np.abs(b).max(axis=0))


@pytest.mark.parametrize("kern,shape", CASES)
def test_system_blocks_fit_bits_and_bounds(torch, ctx, kern, shape):
    from corrla_rs_amd.callers import _poly_block
    (kernel, eps, degree), (n_s, dim) = kern, shape
    x, y = _data(n_s, dim)
    n = n_s + _n_poly(dim, degree)
    m = ctx.rbf_system(x, kernel, eps, poly_degree=degree)
    assert isinstance(m, np.ndarray) and m.shape == (n, n)
    assert np.array_equal(m[:n_s, :n_s], ctx.rbf_matrix(x, x, kernel, eps))
    if degree is not None:
        p = _poly_block(x, degree)
        assert np.array_equal(m[:n_s, n_s:], p) and np.array_equal(m[n_s:, :n_s], p.T)
        assert not m[n_s:, n_s:].any() and not np.signbit(m[n_s:, n_s:]).any()
    assert np.array_equal(m, m.T)
    b = np.vstack([y, np.zeros((n - n_s, N_RHS))])
    c = ctx.rbf_fit(x, y, kernel, eps, poly_degree=degree)
    assert isinstance(c, np.ndarray) and c.shape == (n, N_RHS)
    assert ctx.last_solve_route == ("small" if n <= 128 else "blocked") and ctx.last_solve_info["info"] == 0
    assert np.array_equal(c, ctx.solve(m, b))
    # the tensor path: tensors in, tensors out, the same bits
    xt, yt = torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")
    mt, ct = ctx.rbf_system(xt, kernel, eps, poly_degree=degree), ctx.rbf_fit(xt, yt, kernel, eps, poly_degree=degree)
    assert mt.is_cuda and ct.is_cuda and np.array_equal(mt.cpu().numpy(), m) and np.array_equal(ct.cpu().numpy(), c)
    # the solve bound against that system, with the factors the device entry leaves
    rc, lu, x_dev, ipiv = solve_dev(torch, ctx, m, b)
    assert rc == 0 and np.array_equal(x_dev, c)
    R.check_factorisation(m, lu, ipiv)
    R.check_pivots(m, ipiv)
    R.check_solve(m, b, c, lu)


@pytest.mark.parametrize("kern,shape", [c for c in CASES if c[0][2] is not None])
def test_lu_against_pinv_and_predict(torch, ctx, kern, shape):
    """(RbfInterp always carries a tail: the case without one is Context.rbf_fit's alone)"""
    from corrla_rs_amd import RbfInterp
    (kernel, eps, degree), (n_s, dim) = kern, shape
    x, y = _data(n_s, dim)
    lu_model = RbfInterp(kernel, eps, dim, degree, device=True, ctx=ctx, solver="lu")
    lu_model.fit(x, y)
    pinv_model = RbfInterp(kernel, eps, dim, degree, device=True, ctx=ctx)
    pinv_model.fit(x, y)
    assert pinv_model.solver == "pinv"
    c_lu, c_pinv = lu_model.coeffs, pinv_model.coeffs
    assert np.array_equal(c_lu, ctx.rbf_fit(x, y, kernel, eps, poly_degree=degree))
    m = ctx.rbf_system(x, kernel, eps, poly_degree=degree)
    b = np.vstack([y, np.zeros((m.shape[0] - n_s, N_RHS))])
    kappa = np.linalg.cond(m, np.inf)
    diff = np.abs(c_lu - c_pinv).max(axis=0) / np.abs(c_pinv).max(axis=0)
    bound = 2.0 * kappa * (_eta(m, c_lu, b) + _eta(m, c_pinv, b))
    assert np.all(diff <= bound), (diff, bound, kappa)
    xq = np.random.default_rng(11).uniform(-1.0, 1.0, (70, dim))
    assert np.array_equal(lu_model.predict(xq), ctx.rbf_apply(xq, x, c_lu, kernel, eps, poly_degree=degree))


def test_lu_model_on_tensors_stays_on_the_device(torch, ctx):
    from corrla_rs_amd import RbfInterp
    x, y = _data(97, 2)
    xt = torch.tensor(x, device="cuda")
    model = RbfInterp(3, 0.0, 2, 2, ctx=ctx, solver="lu")
    model.fit(xt, y)  # y is a host array: it alone crosses to the device
    assert model.coeffs.is_cuda and model.x_known.is_cuda and model.coeffs.dtype == torch.float64
    assert np.array_equal(model.coeffs.cpu().numpy(), ctx.rbf_fit(x, y, 3, 0.0, poly_degree=2))
    out = model.predict(torch.tensor(x[:9], device="cuda"))
    assert out.is_cuda and out.shape == (9, N_RHS)
    # the interpolant reproduces its data to the conditioning of the system
    assert np.allclose(model.predict(xt).cpu().numpy(), y, atol=1e-6)


def test_singular_system_raises_with_the_column(ctx):
    from corrla_rs_amd import RbfInterp
    x = np.array(_data(97, 2)[0][:20])
    x[13] = x[4]  # coincident supports: two identical rows, eliminated identically on the small route
    model = RbfInterp(1, 0.0, 2, 1, ctx=ctx, solver="lu")
    with pytest.raises(RuntimeError, match="column"):
        model.fit(x, np.ones((20, 1)))
    assert 1 <= ctx.last_solve_info["info"] <= 23 and ctx.last_solve_info["min_pivot"] == 0.0
    with pytest.raises(ValueError, match="solver"):
        RbfInterp(1, 0.0, 2, 1, solver="qr")


def test_default_interp_keeps_the_bits_of_the_pseudo_inverse_route(ctx):
    """the unchanged numpy formula, restated: [[K, P], [P^T, 0]], every singular value inverted as 1 / (s + 1e-14)"""
    from corrla_rs_amd import RbfInterp
    from corrla_rs_amd.callers import _poly_block
    x, y = (np.array(v[:40]) for v in _data(97, 2))
    p = _poly_block(x, 1)
    zero, rhs = np.zeros((p.shape[1], p.shape[1])), np.vstack([y, np.zeros((p.shape[1], y.shape[1]))])

    def pinv_reg(kp):
        u, sv, vt = np.linalg.svd(kp, full_matrices=False)
        return (vt.T * (1.0 / (sv + 1.0e-14))) @ u.T

    host = RbfInterp(3, 0.0, 2, 1)
    host.fit(x, y)
    r = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
    upper = np.hstack([r * r * r, p])
    assert np.array_equal(host.coeffs, pinv_reg(np.vstack([upper, np.hstack([p.T, zero])])) @ rhs)
    dev = RbfInterp(3, 0.0, 2, 1, device=True, ctx=ctx)
    dev.fit(x, y)
    k = ctx.rbf_matrix(x, x, 3, 0.0)
    assert np.array_equal(dev.coeffs, pinv_reg(np.vstack([np.hstack([k, p]), np.hstack([p.T, zero])])) @ rhs)


def test_value_errors_and_their_einval_twins(ctx):
    x, y = (np.array(v[:10]) for v in _data(97, 2))
    m, c = np.empty((13, 13)), np.empty((13, 3))
    h, lib = ctx._h, ctx._lib

    def rejected(rc, text):
        assert rc == 1 and text in lib.corrla_last_error().decode(), lib.corrla_last_error()

    px, py, pm, pc = x.ctypes.data, y.ctypes.data, m.ctypes.data, c.ctypes.data
    rejected(lib.corrla_rbffit_system_f64(h, None, 10, 2, 2, 1, 0.0, 1, pm, 13), "xs is NULL")
    rejected(lib.corrla_rbffit_system_f64(h, px, 10, 2, 2, 1, 0.0, 1, None, 13), "m is NULL")
    rejected(lib.corrla_rbffit_system_f64(h, px, 0, 2, 2, 1, 0.0, 1, pm, 13), "n_s must be >= 1")
    rejected(lib.corrla_rbffit_system_f64(h, px, 10, 2, 0, 1, 0.0, 1, pm, 13), "dim must be in [1, 128]")
    rejected(lib.corrla_rbffit_system_f64(h, px, 10, 2, 2, 5, 0.0, 1, pm, 13), "kernel must be in [1, 4]")
    rejected(lib.corrla_rbffit_system_f64(h, px, 10, 2, 2, 1, float("nan"), 1, pm, 13), "eps must be finite")
    rejected(lib.corrla_rbffit_system_f64(h, px, 10, 1, 2, 1, 0.0, 1, pm, 13), "ldxs < dim")
    rejected(lib.corrla_rbffit_system_f64(h, px, 10, 2, 2, 1, 0.0, 1, pm, 12), "ldm < n_s + n_poly")
    rejected(lib.corrla_rbffit_system_f64(h, px, 10, 2, 2, 1, 0.0, 1, px, 13), "m overlaps xs")
    rejected(lib.corrla_rbffit_f64(h, px, 10, 2, 2, None, 3, 3, 1, 0.0, 1, pc, 3), "y is NULL")
    rejected(lib.corrla_rbffit_f64(h, px, 10, 2, 2, py, 3, 3, 1, 0.0, 1, None, 3), "coeffs is NULL")
    rejected(lib.corrla_rbffit_f64(h, px, 10, 2, 2, py, 0, 3, 1, 0.0, 1, pc, 3), "n_rhs must be in")
    rejected(lib.corrla_rbffit_f64(h, px, 10, 2, 2, py, 3, 2, 1, 0.0, 1, pc, 3), "ldy < n_rhs")
    rejected(lib.corrla_rbffit_f64(h, px, 10, 2, 2, py, 3, 3, 1, 0.0, 1, pc, 2), "ldw < n_rhs")
    rejected(lib.corrla_rbffit_f64(h, px, 10, 2, 2, py, 3, 3, 1, 0.0, 1, py, 3), "coeffs overlaps y")
    for bad in (lambda: ctx.rbf_fit(x, y[:9], 1), lambda: ctx.rbf_fit(np.empty((0, 2)), np.empty((0, 1)), 1),
                lambda: ctx.rbf_system(x, 1, poly_degree=1.5), lambda: ctx.rbf_fit(x, np.empty((10, 0)), 1),
                lambda: ctx.rbf_system(np.zeros((3, 129)), 1)):
        with pytest.raises(ValueError):
            bad()
