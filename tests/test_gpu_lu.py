"""The dense LU solve on the GPU: corrla_lu_solve_f64 / corrla_lu_solve_dev_f64 and Context.solve over them
(csrc/lu_kernels.hpp).  Run with -m gpu on an MI355X.  tests/test_lu_plan.py pins on the CPU what plan each call of this file
gets (GPU_CALLS there): the small route at n = 1, 2, 5, 100 and kLuSmallN, the blocked route at kLuSmallN + 1, around a panel
boundary with three panels and at 704; n_rhs 1, 3 and 65; padded strides with sentinels in the gaps.

No tolerance is tuned (tests/lu_reference.py).  With u = 2^-53 and gamma_k = k u / (1 - k u), after the device entry, which
leaves L, U and ipiv:
  pivoting       |l_ij| <= 1 exactly; ipiv equals the pivot sequence of the numpy restatement wherever that restatement's
                 winning margin exceeds gamma_N (|L||U|)_jj, and at most 1 % of the columns are left out by that rule
  factorisation  |P A - L U| <= gamma_N |L||U| componentwise (Higham, Thm 9.3), the product formed without rounding
  solve          |A x - b| <= gamma_3N |L||U||x| + gamma_(N+1) (|A||x| + |b|) componentwise (Thm 9.4 plus the f64 residual)
Matrices: Gaussian; a cyclic shift plus 1e-3 Gaussian (every column interchanges, pivots cross panel boundaries);
Wilkinson's growth matrix at n = 40 (max |u| = 2^39 exactly, no interchange); RBF systems (tests/test_gpu_rbf_fit.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import lu_reference as R
from tests.test_lu_plan import GPU_CALLS, NB, SMALL_N

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e300
ENUMERIC, EINVAL = 5, 1


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


def _padded(torch, m, pad):
    """m in a device array with `pad` more columns, the gaps filled with the sentinel -> (whole array, view of m)"""
    whole = torch.full((m.shape[0], m.shape[1] + pad), SENTINEL, dtype=torch.float64, device="cuda")
    whole[:, :m.shape[1]] = torch.from_numpy(np.array(m))
    return whole, whole[:, :m.shape[1]]


def solve_dev(torch, ctx, a, b, pad_a=0, pad_b=0):
    """the raw device entry -> (status, lu, x, ipiv) as numpy; asserts the gaps untouched"""
    n, n_rhs = b.shape
    wa, va = _padded(torch, a, pad_a)
    wb, vb = _padded(torch, b, pad_b)
    ipiv = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = ctx._lib.corrla_lu_solve_dev_f64(ctx._h, wa.data_ptr(), n, n + pad_a, wb.data_ptr(), n_rhs, n_rhs + pad_b, ipiv.data_ptr())
    torch.cuda.synchronize()
    assert bool((wa[:, n:] == SENTINEL).all()) and bool((wb[:, n_rhs:] == SENTINEL).all()), "a padding column was written"
    return rc, va.cpu().numpy(), vb.cpu().numpy(), ipiv.cpu().numpy()


def last_solve(ctx):
    route, info, minp, maxu = C.c_int(0), C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
    assert ctx._lib.corrla_ctx_last_solve(ctx._h, C.byref(route), C.byref(info), C.byref(minp), C.byref(maxu)) == 0
    return route.value, info.value, minp.value, maxu.value


@functools.lru_cache(maxsize=None)
def _case(kind, n, n_rhs):
    return R.matrix(kind, n), R.rhs(n, n_rhs)


@pytest.mark.parametrize("n,n_rhs,pad_a,pad_b,kind", GPU_CALLS)
def test_factorisation_and_solve_bounds(torch, ctx, n, n_rhs, pad_a, pad_b, kind):
    a, b = _case(kind, n, n_rhs)
    rc, lu, x, ipiv = solve_dev(torch, ctx, a, b, pad_a, pad_b)
    assert rc == 0
    route, info, minp, maxu = last_solve(ctx)
    assert route == (1 if n <= SMALL_N else 2) and info == 0
    assert np.all(ipiv >= np.arange(n)) and np.all(ipiv < n)
    ratio = R.check_factorisation(a, lu, ipiv)
    if kind == "wilkinson":  # exact elimination: every column ties, the lowest row wins, the last column doubles n - 1 times
        assert np.array_equal(ipiv, np.arange(n)) and ratio == 0.0
        assert maxu == 2.0 ** (n - 1)
    else:
        R.check_pivots(a, ipiv)
    R.check_solve(a, b, x, lu)
    assert maxu == np.abs(np.triu(lu)).max() and minp == np.abs(np.diag(lu)).min()


@pytest.mark.parametrize("n,n_rhs", [(100, 3), (3 * NB + 1, 65)])
def test_host_entry_is_bitwise_the_device_entry_and_repeats(torch, ctx, n, n_rhs):
    a, b = _case("gauss", n, n_rhs)
    rc, _, x_dev, _ = solve_dev(torch, ctx, a, b)
    assert rc == 0
    x_host = ctx.solve(a, b)
    assert isinstance(x_host, np.ndarray) and np.array_equal(x_host, x_dev)
    x_t = ctx.solve(torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda"))
    assert x_t.is_cuda and np.array_equal(x_t.cpu().numpy(), x_dev)
    assert np.array_equal(ctx.solve(a, b), x_host)  # two identical calls, identical bits
    assert ctx.last_solve_route == ("small" if n <= SMALL_N else "blocked") and ctx.last_solve_info["info"] == 0
    # a vector right-hand side, and the host entry with padded rows: x's gaps keep the sentinel
    assert np.array_equal(ctx.solve(a, b[:, 0]), x_host[:, 0])
    wa = np.full((n, n + 3), SENTINEL)
    wa[:, :n] = a
    wx = np.full((n, n_rhs + 2), SENTINEL)
    rc = ctx._lib.corrla_lu_solve_f64(ctx._h, wa.ctypes.data, n, n + 3, b.ctypes.data, n_rhs, n_rhs, wx.ctypes.data, n_rhs + 2)
    assert rc == 0 and np.array_equal(wx[:, :n_rhs], x_host) and np.all(wx[:, n_rhs:] == SENTINEL) and np.array_equal(wa[:, :n], a)


def test_overwrite_leaves_lu_and_x_in_place(torch, ctx):
    a, b = _case("gauss", 3 * NB, 3)
    ta, tb = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")
    x = ctx.solve(ta, tb, overwrite=True)
    assert x.data_ptr() == tb.data_ptr()
    _, lu, x_ref, _ = solve_dev(torch, ctx, a, b)
    assert np.array_equal(ta.cpu().numpy(), lu) and np.array_equal(tb.cpu().numpy(), x_ref)
    with pytest.raises(ValueError, match="overwrite"):
        ctx.solve(a, b, overwrite=True)


# one in each route, and one in a panel other than the first; each runs to completion and reports its column
@pytest.mark.parametrize("n,col", [(100, 37), (3 * NB + 1, 5), (3 * NB + 1, 2 * NB + 2)])
def test_zero_pivot_reports_its_column(torch, ctx, n, col):
    from corrla_rs_amd._lib import CorrlaError
    a = R.singular_at(n, col)
    _, ref_ipiv, _, ref_info = R.getrf(a)
    assert ref_info == col + 1
    b = R.rhs(n, 3)
    rc, _, _, ipiv = solve_dev(torch, ctx, a, b)
    assert rc == ENUMERIC
    route, info, minp, _ = last_solve(ctx)
    assert info == col + 1 and minp == 0.0 and route == (1 if n <= SMALL_N else 2)
    assert np.array_equal(ipiv[:col], ref_ipiv[:col]) and np.all(ipiv >= np.arange(n)) and np.all(ipiv < n)
    with pytest.raises(CorrlaError, match=f"column {col + 1} ") as e:
        ctx.solve(a, b)
    assert e.value.code == ENUMERIC and isinstance(e.value, RuntimeError)
    assert ctx.last_solve_info["info"] == col + 1
    # the context is usable afterwards
    good, gb = _case("gauss", n, 3)
    R.check_solve(good, gb, ctx.solve(good, gb), solve_dev(torch, ctx, good, gb)[1])


@pytest.mark.parametrize("n,where", [(5, (3, 1)), (100, (0, 99)), (3 * NB + 1, (150, 70)), (3 * NB + 1, (2, 190))])
def test_nan_entry_is_enumeric(torch, ctx, n, where):
    a = np.array(R.matrix("gauss", n))
    a[where] = np.nan
    rc, _, _, ipiv = solve_dev(torch, ctx, a, R.rhs(n, 1))
    assert rc == ENUMERIC and 1 <= last_solve(ctx)[1] <= n
    assert np.all(ipiv >= 0) and np.all(ipiv < n)
    a[where] = np.inf
    assert solve_dev(torch, ctx, a, R.rhs(n, 1))[0] == ENUMERIC


def test_value_errors_and_their_einval_twins(torch, ctx):
    a, b = (np.array(v) for v in _case("gauss", 5, 3))
    x = np.empty((5, 3))
    f = ctx._lib.corrla_lu_solve_f64
    h, pa, pb, px = ctx._h, a.ctypes.data, b.ctypes.data, x.ctypes.data

    def rejected(rc, text):
        assert rc == EINVAL and text in ctx._lib.corrla_last_error().decode(), ctx._lib.corrla_last_error()

    rejected(f(h, None, 5, 5, pb, 3, 3, px, 3), "a is NULL")
    rejected(f(h, pa, 5, 5, None, 3, 3, px, 3), "b is NULL")
    rejected(f(h, pa, 5, 5, pb, 3, 3, None, 3), "x is NULL")
    rejected(f(h, pa, 0, 5, pb, 3, 3, px, 3), "n must be >= 1")
    rejected(f(h, pa, (1 << 17) + 1, 1 << 18, pb, 3, 3, px, 3), "n must be <= 131072")
    rejected(f(h, pa, 5, 5, pb, 0, 3, px, 3), "n_rhs must be >= 1")
    rejected(f(h, pa, 5, 4, pb, 3, 3, px, 3), "lda < n")
    rejected(f(h, pa, 5, 5, pb, 3, 2, px, 3), "ldb < n_rhs")
    rejected(f(h, pa, 5, 5, pb, 3, 3, px, 2), "ldx < n_rhs")
    rejected(f(h, pa, 5, 5, pb, 3, 3, pb, 3), "x overlaps b")
    rejected(f(h, pa, 5, 5, pb, 3, 3, pa, 3), "x overlaps a")
    ta, tb = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")
    ip = torch.zeros(5, dtype=torch.int64, device="cuda")
    g = ctx._lib.corrla_lu_solve_dev_f64
    rejected(g(h, ta.data_ptr(), 5, 5, ta.data_ptr(), 3, 5, None), "overlaps")
    rejected(g(h, ta.data_ptr(), 5, 5, tb.data_ptr(), 3, 3, ta.data_ptr()), "overlaps")
    rejected(g(h, ta.data_ptr(), 5, 4, tb.data_ptr(), 3, 3, ip.data_ptr()), "lda < n")
    assert np.array_equal(ta.cpu().numpy(), a)  # a rejected call touches nothing
    for bad_a, bad_b in ((a[:, :4], b), (a, b[:4]), (np.empty((0, 0)), np.empty((0, 1))), (a, np.empty((5, 0)))):
        with pytest.raises(ValueError):
            ctx.solve(bad_a, bad_b)
    with pytest.raises(ValueError):
        ctx.solve(a, b, overwrite=1)
    assert ctx.solve(a.astype(np.float32), b).dtype == np.float64
