"""The dense Cholesky factor and SPD solve on the GPU: corrla_chol_factor_[dev_]f64, corrla_chol_solve_[dev_]f64 and
Context.cholesky / Context.solve(assume="pos") over them (csrc/chol_kernels.hpp).  Run with -m gpu on an MI355X.
tests/test_chol_plan.py pins on the CPU what plan each call of this file gets (GPU_CALLS there): the small route at n = 1, 2, 5,
100 and kCholSmallN, the blocked route at kCholSmallN + 1, around a panel boundary with three panels and at 704; n_rhs 1, 3 and
65; padded strides with sentinels in the gaps; every kind of matrix on both routes.

No tolerance is tuned (tests/chol_reference.py).  With u = 2^-53 and gamma_k = k u / (1 - k u):
  factorisation  diag(L) > 0; |A - L L^T| <= gamma_(n+1) |L||L^T| componentwise (Higham, Thm 10.3), the product formed without
                 rounding; min_diag and max_diag bitwise numpy's over the returned diagonal
  logdet         |logdet - 2 sum log l_jj| <= (gamma_n + 4u) sum |2 log l_jj|, the reference sum in longdouble over the returned
                 diagonal: gamma_n covers the summation in any fixed order, 4u two ulp for the device log (the HIP math API
                 documents 1 ulp for the double-precision log)
  solve          |A x - b| <= gamma_(3n+1) |L||L^T||x| + gamma_(n+1) (|A||x| + |b|) componentwise (Thm 10.4 plus the f64 residual)
The strict upper triangle of A holds a sentinel in every device call and comes back untouched: it is neither read nor written.
Matrices: a Gram matrix, Lehmer's, Kac-Murdock-Szego's, the Gram matrix badly scaled by powers of two (condition ~1e25), and
matrices whose elimination is exact and fails at a chosen column."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import chol_reference as R
from tests.test_chol_plan import GPU_CALLS, NB, SMALL_N

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


def _padded(torch, m, pad, lower_only=False):
    """m in a device array with `pad` more columns, the gaps -- and with lower_only the strict upper triangle -- filled with
    the sentinel -> (whole array, view of m)"""
    src = np.array(m)
    if lower_only:
        src[np.triu_indices(src.shape[0], 1)] = SENTINEL
    whole = torch.full((m.shape[0], m.shape[1] + pad), SENTINEL, dtype=torch.float64, device="cuda")
    whole[:, :m.shape[1]] = torch.from_numpy(src)
    return whole, whole[:, :m.shape[1]]


def _lower_and_untouched(wa, n):
    """the view's lower triangle as numpy with zeros above; asserts the sentinel above the diagonal and in the padding"""
    got = wa.cpu().numpy()
    assert np.all(got[:, n:] == SENTINEL), "a padding column of a was written"
    assert np.all(got[:, :n][np.triu_indices(n, 1)] == SENTINEL), "the strict upper triangle of a was written"
    return np.tril(got[:, :n])


def factor_dev(torch, ctx, a, pad_a=0):
    """the raw in-place factor entry on the lower triangle of a -> (status, L as numpy with zeros above)"""
    n = a.shape[0]
    wa, _ = _padded(torch, a, pad_a, lower_only=True)
    torch.cuda.synchronize()
    rc = ctx._lib.corrla_chol_factor_dev_f64(ctx._h, wa.data_ptr(), n, n + pad_a)
    torch.cuda.synchronize()
    return rc, _lower_and_untouched(wa, n)


def solve_dev(torch, ctx, a, b, pad_a=0, pad_b=0):
    """the raw in-place solve entry -> (status, L, x) as numpy"""
    n, n_rhs = b.shape
    wa, _ = _padded(torch, a, pad_a, lower_only=True)
    wb, vb = _padded(torch, b, pad_b)
    torch.cuda.synchronize()
    rc = ctx._lib.corrla_chol_solve_dev_f64(ctx._h, wa.data_ptr(), n, n + pad_a, wb.data_ptr(), n_rhs, n_rhs + pad_b)
    torch.cuda.synchronize()
    assert bool((wb[:, n_rhs:] == SENTINEL).all()), "a padding column of b was written"
    return rc, _lower_and_untouched(wa, n), vb.cpu().numpy()


def last_chol(ctx):
    route, info = C.c_int(0), C.c_int64(0)
    mind, maxd, logdet = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    assert ctx._lib.corrla_ctx_last_chol(ctx._h, C.byref(route), C.byref(info), C.byref(mind), C.byref(maxd), C.byref(logdet)) == 0
    assert ctx._lib.corrla_ctx_last_chol(ctx._h, None, None, None, None, None) == 0  # any pointer may be NULL
    return route.value, info.value, mind.value, maxd.value, logdet.value


@functools.lru_cache(maxsize=None)
def _case(kind, n, n_rhs):
    return R.spd(kind, n), R.rhs(n, n_rhs)


@pytest.mark.parametrize("n,n_rhs,pad_a,pad_b,kind", GPU_CALLS)
def test_factorisation_logdet_and_solve_bounds(torch, ctx, n, n_rhs, pad_a, pad_b, kind):
    a, b = _case(kind, n, n_rhs)
    rc, l = factor_dev(torch, ctx, a, pad_a)
    assert rc == 0
    route, info, mind, maxd, logdet = last_chol(ctx)
    assert route == (1 if n <= SMALL_N else 2) and info == 0
    R.check_factorisation(a, l)
    assert mind == np.diag(l).min() and maxd == np.diag(l).max()
    R.check_logdet(np.diag(l), logdet)
    rc, l2, x = solve_dev(torch, ctx, a, b, pad_a, pad_b)
    assert rc == 0 and np.array_equal(l2, l)  # the solve factors as the factor entry does
    assert last_chol(ctx) == (route, 0, mind, maxd, logdet)
    R.check_solve(a, b, x, l)


@pytest.mark.parametrize("n,n_rhs", [(100, 3), (3 * NB + 1, 65)])
def test_entries_agree_bitwise(torch, ctx, n, n_rhs):
    a, b = _case("gram", n, n_rhs)
    rc, l_dev, x_dev = solve_dev(torch, ctx, a, b)
    assert rc == 0
    x_host = ctx.solve(a, b, assume="pos")
    assert isinstance(x_host, np.ndarray) and np.array_equal(x_host, x_dev)
    x_t = ctx.solve(torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda"), assume="pos")
    assert x_t.is_cuda and np.array_equal(x_t.cpu().numpy(), x_dev)
    assert np.array_equal(ctx.solve(a, b, assume="pos"), x_host)  # two identical calls, identical bits
    assert ctx.last_chol_route == ("small" if n <= SMALL_N else "blocked") and ctx.last_chol_info["info"] == 0
    assert set(ctx.last_chol_info) == {"info", "min_diag", "max_diag", "logdet"}
    assert ctx.last_chol_info["min_diag"] == np.diag(l_dev).min() and ctx.last_chol_info["max_diag"] == np.diag(l_dev).max()
    # a vector right-hand side, and the host entry with padded rows: x's gaps keep the sentinel, a is left untouched
    assert np.array_equal(ctx.solve(a, b[:, 0], assume="pos"), x_host[:, 0])
    wa = np.full((n, n + 3), SENTINEL)
    wa[:, :n] = a
    wx = np.full((n, n_rhs + 2), SENTINEL)
    rc = ctx._lib.corrla_chol_solve_f64(ctx._h, wa.ctypes.data, n, n + 3, b.ctypes.data, n_rhs, n_rhs, wx.ctypes.data, n_rhs + 2)
    assert rc == 0 and np.array_equal(wx[:, :n_rhs], x_host) and np.all(wx[:, n_rhs:] == SENTINEL) and np.array_equal(wa[:, :n], a)
    # Context.cholesky: the device factor with zeros above, from numpy, from a tensor, and from the raw host entry with padding
    lc = ctx.cholesky(a)
    assert isinstance(lc, np.ndarray) and np.array_equal(lc, l_dev) and not np.signbit(lc[np.triu_indices(n, 1)]).any()
    lt = ctx.cholesky(torch.tensor(a, device="cuda"))
    assert lt.is_cuda and np.array_equal(lt.cpu().numpy(), l_dev)
    wl = np.full((n, n + 2), SENTINEL)
    rc = ctx._lib.corrla_chol_factor_f64(ctx._h, wa.ctypes.data, n, n + 3, wl.ctypes.data, n + 2)
    assert rc == 0 and np.array_equal(wl[:, :n], l_dev) and np.all(wl[:, n:] == SENTINEL) and np.array_equal(wa[:, :n], a)
    assert ctx.cholesky(a.astype(np.float32)).dtype == np.float64
    # assume="general" is today's LU path
    x_lu = ctx.solve(a, b)
    assert np.array_equal(ctx.solve(a, b, assume="general"), x_lu)
    xw = np.empty((n, n_rhs))
    assert ctx._lib.corrla_lu_solve_f64(ctx._h, a.ctypes.data, n, n, b.ctypes.data, n_rhs, n_rhs, xw.ctypes.data, n_rhs) == 0
    assert np.array_equal(xw, x_lu)


def test_overwrite_factors_in_place_and_keeps_the_upper_triangle(torch, ctx):
    n = 3 * NB
    a, b = _case("gram", n, 3)
    _, l_ref, x_ref = solve_dev(torch, ctx, a, b)
    ta, _ = _padded(torch, a, 0, lower_only=True)
    out = ctx.cholesky(ta, overwrite=True)
    assert out is ta
    assert np.array_equal(_lower_and_untouched(ta, n), l_ref)
    ta, _ = _padded(torch, a, 0, lower_only=True)
    tb = torch.tensor(b, device="cuda")
    x = ctx.solve(ta, tb, assume="pos", overwrite=True)
    assert x.data_ptr() == tb.data_ptr()
    assert np.array_equal(_lower_and_untouched(ta, n), l_ref) and np.array_equal(tb.cpu().numpy(), x_ref)
    with pytest.raises(ValueError, match="overwrite"):
        ctx.cholesky(a, overwrite=True)
    with pytest.raises(ValueError, match="overwrite"):
        ctx.solve(a, b, assume="pos", overwrite=True)
    with pytest.raises(ValueError, match="overwrite"):
        ctx.cholesky(torch.tensor(a, device="cuda", dtype=torch.float32), overwrite=True)


# one in each route, and one in a panel other than the first; each runs to completion and reports its column
@pytest.mark.parametrize("pivot", [0.0, -1.0])
@pytest.mark.parametrize("n,col", [(100, 37), (3 * NB + 1, 5), (3 * NB + 1, 2 * NB + 2)])
def test_not_positive_definite_reports_its_column(torch, ctx, n, col, pivot):
    from corrla_rs_amd._lib import CorrlaError
    a, lt = R.not_spd_at(n, col, pivot)
    assert R.cholesky(a)[1] == col + 1
    rc, l = factor_dev(torch, ctx, a)
    assert rc == ENUMERIC
    route, info, mind, maxd, logdet = last_chol(ctx)
    assert info == col + 1 and logdet == 0.0 and route == (1 if n <= SMALL_N else 2)
    assert np.array_equal(l[:, :col], lt[:, :col])  # the columns before the failed one are final, and exact
    assert mind == np.diag(lt)[:col].min() and maxd == np.diag(lt)[:col].max()
    b = R.rhs(n, 3)
    with pytest.raises(CorrlaError, match=f"column {col + 1} ") as e:
        ctx.solve(a, b, assume="pos")
    assert e.value.code == ENUMERIC and isinstance(e.value, RuntimeError)
    assert ctx.last_chol_info["info"] == col + 1 and ctx.last_chol_info["logdet"] == 0.0
    with pytest.raises(CorrlaError, match=f"column {col + 1} "):
        ctx.cholesky(a)
    # the host entries write nothing
    wl = np.full((n, n), SENTINEL)
    assert ctx._lib.corrla_chol_factor_f64(ctx._h, a.ctypes.data, n, n, wl.ctypes.data, n) == ENUMERIC and np.all(wl == SENTINEL)
    wx = np.full((n, 3), SENTINEL)
    assert ctx._lib.corrla_chol_solve_f64(ctx._h, a.ctypes.data, n, n, b.ctypes.data, 3, 3, wx.ctypes.data, 3) == ENUMERIC
    assert np.all(wx == SENTINEL)
    # the context is usable afterwards
    good, gb = _case("gram", n, 3)
    rc, gl, gx = solve_dev(torch, ctx, good, gb)
    assert rc == 0
    R.check_solve(good, gb, gx, gl)


@pytest.mark.parametrize("n,where", [(5, (3, 1)), (100, (99, 0)), (3 * NB + 1, (150, 70))])
def test_non_finite_entry_is_enumeric(torch, ctx, n, where):
    a = np.array(R.spd("gram", n))
    for bad in (np.nan, np.inf):
        a[where] = bad
        rc, _ = factor_dev(torch, ctx, a)
        assert rc == ENUMERIC and 1 <= last_chol(ctx)[1] <= n
        rc, _, _ = solve_dev(torch, ctx, a, R.rhs(n, 1))
        assert rc == ENUMERIC and 1 <= last_chol(ctx)[1] <= n
    # the same entry mirrored into the UPPER triangle changes nothing: Context.cholesky passes the array as it is
    good = np.array(R.spd("gram", n))
    want = ctx.cholesky(good)
    good[where[1], where[0]] = np.nan
    assert np.array_equal(ctx.cholesky(good), want)
    assert np.array_equal(ctx.cholesky(torch.tensor(good, device="cuda")).cpu().numpy(), want)


def test_value_errors_and_their_einval_twins(torch, ctx):
    a, b = (np.array(v) for v in _case("gram", 5, 3))
    x, l = np.empty((5, 3)), np.empty((5, 5))
    h, pa, pb, px, pl = ctx._h, a.ctypes.data, b.ctypes.data, x.ctypes.data, l.ctypes.data

    def rejected(rc, text):
        assert rc == EINVAL and text in ctx._lib.corrla_last_error().decode(), ctx._lib.corrla_last_error()

    f = ctx._lib.corrla_chol_solve_f64
    rejected(f(h, None, 5, 5, pb, 3, 3, px, 3), "a is NULL")
    rejected(f(h, pa, 5, 5, None, 3, 3, px, 3), "b is NULL")
    rejected(f(h, pa, 5, 5, pb, 3, 3, None, 3), "x is NULL")
    rejected(f(h, pa, 0, 5, pb, 3, 3, px, 3), "n must be >= 1")
    rejected(f(h, pa, (1 << 17) + 1, 1 << 18, pb, 3, 3, px, 3), "n must be <= 131072")
    rejected(f(h, pa, 5, 5, pb, 0, 3, px, 3), "n_rhs must be >= 1")
    rejected(f(h, pa, 5, 5, pb, (1 << 20) + 1, 1 << 21, px, 1 << 21), "n_rhs must be <= 1048576")
    rejected(f(h, pa, 5, 4, pb, 3, 3, px, 3), "lda < n")
    rejected(f(h, pa, 5, 5, pb, 3, 2, px, 3), "ldb < n_rhs")
    rejected(f(h, pa, 5, 5, pb, 3, 3, px, 2), "ldx < n_rhs")
    rejected(f(h, pa, 5, 5, pb, 3, 3, pb, 3), "x overlaps b")
    rejected(f(h, pa, 5, 5, pb, 3, 3, pa, 3), "x overlaps a")
    f = ctx._lib.corrla_chol_factor_f64
    rejected(f(h, None, 5, 5, pl, 5), "a is NULL")
    rejected(f(h, pa, 5, 5, None, 5), "l is NULL")
    rejected(f(h, pa, 0, 5, pl, 5), "n must be >= 1")
    rejected(f(h, pa, (1 << 17) + 1, 1 << 18, pl, 1 << 18), "n must be <= 131072")
    rejected(f(h, pa, 5, 4, pl, 5), "lda < n")
    rejected(f(h, pa, 5, 5, pl, 4), "ldl < n")
    rejected(f(h, pa, 5, 5, pa, 5), "l overlaps a")
    ta, tb = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")
    g = ctx._lib.corrla_chol_solve_dev_f64
    rejected(g(h, ta.data_ptr(), 5, 5, ta.data_ptr(), 3, 5), "a overlaps b")
    rejected(g(h, ta.data_ptr(), 5, 4, tb.data_ptr(), 3, 3), "lda < n")
    rejected(g(h, None, 5, 5, tb.data_ptr(), 3, 3), "a is NULL")
    rejected(g(h, ta.data_ptr(), 5, 5, None, 3, 3), "b is NULL")
    rejected(g(h, ta.data_ptr(), 5, 5, tb.data_ptr(), 3, 2), "ldb < n_rhs")
    g = ctx._lib.corrla_chol_factor_dev_f64
    rejected(g(h, None, 5, 5), "a is NULL")
    rejected(g(h, ta.data_ptr(), 5, 4), "lda < n")
    rejected(g(h, ta.data_ptr(), 0, 5), "n must be >= 1")
    torch.cuda.synchronize()
    assert np.array_equal(ta.cpu().numpy(), a) and np.array_equal(tb.cpu().numpy(), b)  # a rejected call touches nothing
    for bad_a, bad_b in ((a[:, :4], b), (a, b[:4]), (np.empty((0, 0)), np.empty((0, 1))), (a, np.empty((5, 0)))):
        with pytest.raises(ValueError):
            ctx.solve(bad_a, bad_b, assume="pos")
    for bad_a in (a[:, :4], np.empty((0, 0))):
        with pytest.raises(ValueError):
            ctx.cholesky(bad_a)
    with pytest.raises(ValueError):
        ctx.solve(a, b, assume="pos", overwrite=1)
    with pytest.raises(ValueError):
        ctx.cholesky(a, overwrite=1)
    for bad in ("sym", "POS", None, 1):
        with pytest.raises(ValueError, match="assume"):
            ctx.solve(a, b, assume=bad)
    assert ctx.solve(a.astype(np.float32), b, assume="pos").dtype == np.float64
