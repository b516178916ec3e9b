"""Covariance and Pearson correlation matrices (corrla_cov_*, csrc/syrk_kernels.hpp) on the GPU.  Run with -m gpu on an MI355X.

Every case runs in f32 and f64, with host pointers (numpy) and with CUDA tensors, and asserts the route that served it, so
that no other path can stand in for the symmetric kernel.  tests/test_syrk_plan.py pins on the CPU what plan each call of
this file gets (GPU_CALLS there).

Bounds.  u = 2^-24 (f32) / 2^-53 (f64), gamma_k = k u / (1 - k u).  Against numpy in f64 on the same stored values:
  covariance    |C^ - C|_ij <= gamma_{m+8} (|X~|^T |X~|)_ij / (m - ddof) + 4 u |C_ij|,  X~ = X centred in f64
                (the componentwise bound of a dot product of length m in any order, tests/test_gpu_gemm_routes.py, with 8
                more roundings for the centring, the slab sums and the division); doubled for f64, whose reference carries
                the same bound
  correlation   that bound / (sd_i sd_j) + 8 u
  means         |mu^ - mu| <= 4 u |mu| + gamma64_{m+8} mean_i |x_ij - x_0j|: one rounding to T of a sum accumulated in f64
                about the column's first row (the second term is that accumulation's own bound, 2^-53-sized)
  scales        relative error <= 4 u + gamma64_{m+8} kappa_j, kappa_j = sum_i (x_ij - x_0j)^2 / ss_j >= 1: the same
                accumulation, of the shifted sum of squares, amplified by its cancellation against m (mu - x_0)^2; the
                reference sums are correctly rounded (math.fsum).  Against Context.pca(standardize=True) on the f32
                case: 4 u, as both are then single roundings of nearly the same number
The exact cases use integers in [-3, 3]: every sum stays below 2^14 and C (m - 1) rounds back to the integer X^T X."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests.test_syrk_plan import CENTRED_SHAPES, EDGE_CASES, EXACT_SHAPES, LAYOUTS, REFERENCE_SHAPE, SLAB_ROWS

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
KINDS = ("host", "dev")


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


@pytest.fixture(scope="module")
def ctx_slabs():
    """the plan knobs are read when a context is created"""
    import corrla_rs_amd as cr
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CORRLA_SYRK_SLAB_ROWS", str(SLAB_ROWS))
        c = cr.Context(0)
    yield c
    c.close()


def _u(dtype):
    return 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53


def _gamma(k, u):
    return k * u / (1.0 - k * u)


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _give(torch, x, kind):
    """x (a numpy view of any layout) as the host or device operand with the SAME strides and the same offset of its base
    from a 16-byte boundary"""
    if kind == "host":
        return x
    span = (x.shape[0] - 1) * x.strides[0] // x.itemsize + (x.shape[1] - 1) * x.strides[1] // x.itemsize + 1
    off = (x.ctypes.data % 16) // x.itemsize
    flat = torch.empty(span + off, dtype=torch.float32 if x.dtype == np.float32 else torch.float64, device="cuda")
    t = torch.as_strided(flat, x.shape, tuple(s // x.itemsize for s in x.strides), off)
    t.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert t.data_ptr() % 16 == x.ctypes.data % 16
    return t


def _route(x):
    """the route the plan gives this layout (syrk_plan.hpp): unit stride along the features reads in place -- with 16-byte
    loads when base and row stride allow them -- anything else is repacked"""
    m, n = x.shape
    rs, cs = x.strides[0] // x.itemsize, x.strides[1] // x.itemsize
    vec = 16 // x.itemsize
    if cs == 1 and (rs >= n or m == 1):
        return "inplace" if x.ctypes.data % 16 == 0 and rs % vec == 0 else "inplace_checked"
    return "repacked"


def _cov(torch, ctx, x, kind, **kw):
    want_route = _route(x)
    c, means, scales = ctx.cov(_give(torch, x, kind), **kw)
    assert ctx.last_cov_route() == want_route, (ctx.last_cov_route(), want_route, x.shape, x.strides, kind)
    if kind == "dev":
        assert c.is_cuda and (means is None or means.is_cuda) and (scales is None or scales.is_cuda)
    else:
        assert type(c) is np.ndarray
    c = _np(c)
    assert c.dtype == x.dtype and c.shape == (x.shape[1], x.shape[1])
    assert np.array_equal(c, c.T), "C is not bitwise symmetric"
    return c, None if means is None else _np(means), None if scales is None else _np(scales)


# ---- exact, center=False ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ints(m, n):
    x = np.random.default_rng(7 * m + n).integers(-3, 4, size=(m, n)).astype(np.float64)
    ref = (x.T @ x).astype(np.int64)
    assert np.abs(ref).max() < 1 << 14
    x.setflags(write=False)
    return x, ref


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("slabs", (False, True), ids=("one_slab_plan", "forced_slabs"))
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_second_moments_of_integers_are_exact(torch, ctx, ctx_slabs, shape, slabs, dtype, kind):
    m, n = shape
    x64, ref = _ints(m, n)
    x = x64.astype(dtype)
    c, means, scales = _cov(torch, ctx_slabs if slabs else ctx, x, kind, center=False, ddof=1)
    assert means is None and scales is None
    got = np.rint(c.astype(np.float64) * (m - 1)).astype(np.int64)
    if not np.array_equal(got, ref):
        i, j = [int(v[0]) for v in np.nonzero(got != ref)]
        kt = 32 if dtype == np.float32 else 16
        rows = (SLAB_ROWS + kt - 1) // kt * kt if slabs else m
        # which slab's partial sum, left out or taken twice, would explain the difference
        parts = [int(x64[s:s + rows, i] @ x64[s:s + rows, j]) for s in range(0, m, rows)]
        blame = [s for s, p in enumerate(parts) if p != 0 and abs(int(ref[i, j] - got[i, j])) == abs(p)]
        pytest.fail("%d of %d entries differ, first at (%d, %d): %d instead of %d -- tile pair (%d, %d), %d slab(s) of %d rows, "
                    "slab(s) whose partial sum equals the difference: %s"
                    % (int((got != ref).sum()), got.size, i, j, got[i, j], ref[i, j], min(i, j) // 128, max(i, j) // 128, len(parts),
                       rows, blame or "none"))


# ---- centred, against np.cov in f64 of the same stored values --------------------------------------------------------------
def _gauss(m, n, dtype, seed=0):
    return np.random.default_rng(1000 * m + n + seed).standard_normal((m, n)).astype(dtype)


def _layouts(x):
    """name -> a view with the values of x: contiguous, padded rows (ld = n + 3), base offset by one element, column-major"""
    m, n = x.shape
    padded = np.zeros((m, n + 3), dtype=x.dtype)
    padded[:, :n] = x
    flat = np.zeros(m * n + 1 + 4, dtype=x.dtype)
    start = 1 if flat.ctypes.data % 16 == 0 else 1 + (16 - flat.ctypes.data % 16) // x.itemsize   # one element past a boundary
    off = flat[start:start + m * n].reshape(m, n)
    off[...] = x
    return {"contiguous": x, "ld_n_plus_3": padded[:, :n], "base_plus_1": off, "column_major": np.asfortranarray(x)}


def _check_cov(x, c, means, ddof, what):
    dtype, (m, n) = x.dtype, x.shape
    u = _u(dtype)
    x64 = x.astype(np.float64)
    mu = np.array([math.fsum(x64[:, j]) / m for j in range(n)])
    xt = x64 - mu
    ref = xt.T @ xt / (m - ddof)
    bound = _gamma(m + 8, u) * (np.abs(xt).T @ np.abs(xt)) / (m - ddof) + 4 * u * np.abs(ref)
    if dtype == np.float64:
        bound = 2 * bound
    err = np.abs(c.astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print("%s: max |C^ - C| / bound = %.3e" % (what, worst))
    assert np.all(err <= bound), (what, worst)
    if means is not None:
        assert means.shape == (1, n) and means.dtype == dtype
        tol = 4 * u * np.abs(mu) + _gamma(m + 8, 2.0 ** -53) * np.abs(x64 - x64[0]).mean(axis=0)
        merr = np.abs(means[0].astype(np.float64) - mu)
        print("%s: max |mu^ - mu| / tol = %.3e" % (what, float((merr / np.maximum(tol, 1e-300)).max())))
        assert np.all(merr <= tol), what
    return ref


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", CENTRED_SHAPES, ids=lambda s: "%dx%d" % s)
def test_covariance_of_gaussians_in_every_layout(torch, ctx, shape, layout, dtype, kind):
    x = _layouts(_gauss(*shape, dtype))[layout]
    if layout == "column_major":
        assert _route(x) == "repacked"
    if layout == "base_plus_1":
        assert _route(x) == "inplace_checked"
    c, means, scales = _cov(torch, ctx, x, kind)
    assert scales is None
    _check_cov(x, c, means, 1, "%s %s %s %s" % (shape, layout, dtype.__name__, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_columns_far_from_zero_are_centred_in_registers(torch, ctx, dtype, kind):
    """(1031, 77) with column j shifted by 1e4 (j mod 3).  This is the case that tells centring before the product from any
    sum x y - m mu nu form: there the products are ~4e8 for a covariance of ~1, so the uncentred form in f32 is off by the
    order of 4e8 u m^(1/2) or more -- every digit of the result (a numpy f32 restatement is printed below for comparison), while the centred operands are exact differences (Sterbenz) and the
    bound of a plain Gaussian matrix holds."""
    m, n = 1031, 77
    x = (_gauss(m, n, np.float64, seed=5) + 1.0e4 * (np.arange(n) % 3)).astype(dtype)
    c, means, _ = _cov(torch, ctx, x, kind)
    ref = _check_cov(x, c, means, 1, "shifted %s %s" % (dtype.__name__, kind))
    mu_t = x.astype(np.float64).mean(axis=0).astype(dtype)
    naive = ((x.T @ x) - dtype(m) * np.outer(mu_t, mu_t)) / dtype(m - 1)
    print("uncentred form in %s: max |C - ref| = %.3e (%.1e u); this kernel: %.3e"
          % (dtype.__name__, float(np.abs(naive - ref).max()), float(np.abs(naive - ref).max()) / _u(dtype),
             float(np.abs(c - ref).max())))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_covariance_edge_shapes(torch, ctx, case, dtype, kind):
    m, n, ddof = EDGE_CASES[case]
    x = _gauss(m, n, dtype, seed=11)
    c, means, _ = _cov(torch, ctx, x, kind, ddof=ddof)
    ref = _check_cov(x, c, means, ddof, "%s %s %s" % (case, dtype.__name__, kind))
    npref = np.cov(x.astype(np.float64), rowvar=False, ddof=ddof).reshape(n, n)
    assert np.allclose(ref, npref, rtol=1e-12, atol=1e-14)


# ---- correlation -------------------------------------------------------------------------------------------------------------
def _check_corr(x, r, scales, what, dead=()):
    dtype, (m, n) = x.dtype, x.shape
    u = _u(dtype)
    x64 = x.astype(np.float64)
    mu = np.array([math.fsum(x64[:, j]) / m for j in range(n)])
    xt = x64 - mu
    ss = np.array([math.fsum(xt[:, j] ** 2) for j in range(n)])          # correctly rounded sums: the reference adds no error
    sd = np.sqrt(ss / (m - 1))
    live = np.array([j not in dead for j in range(n)])
    sd_l = np.where(live, sd, 1.0)
    cov = xt.T @ xt / (m - 1)
    ref = cov / np.outer(sd_l, sd_l)
    bound = (_gamma(m + 8, u) * (np.abs(xt).T @ np.abs(xt)) / (m - 1) + 4 * u * np.abs(cov)) / np.outer(sd_l, sd_l) + 8 * u
    if dtype == np.float64:
        bound = 2 * bound
    ll = np.outer(live, live)
    err = np.abs(r.astype(np.float64) - ref)
    print("%s: max |R^ - R| / bound = %.3e" % (what, float((err[ll] / bound[ll]).max())))
    assert np.all(err[ll] <= bound[ll]), what
    assert np.all(np.diag(r)[live] == 1), "the diagonal is not exactly 1"
    assert np.all(np.abs(r) <= 1)
    for j in dead:
        assert not r[j].any() and not r[:, j].any() and r[j, j] == 0 and scales[0, j] == 1
    # scales: one rounding to T of sqrt(ss / (m - 1)), ss accumulated in f64 about the column's first row
    kappa = ((x64 - x64[0]) ** 2).sum(axis=0)[live] / ss[live]
    tol = 4 * u + _gamma(m + 8, 2.0 ** -53) * kappa
    rel = np.abs(scales[0].astype(np.float64)[live] - sd[live]) / sd[live]
    print("%s: max relative error of the scales / tolerance = %.3e" % (what, float((rel / tol).max())))
    assert np.all(rel <= tol), (what, float(rel.max()))
    if not dead:
        npref = np.corrcoef(x64, rowvar=False).reshape(n, n)
        assert np.allclose(ref, npref, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("shape", CENTRED_SHAPES, ids=lambda s: "%dx%d" % s)
def test_correlation_of_gaussians(torch, ctx, shape, dtype, kind):
    m, n = shape
    x = _gauss(m, n, np.float64, seed=2)
    x[:, 1] += 0.8 * x[:, 0]                       # some real correlation, scales over 1e-2 .. 1e2, means within 3 sd
    x = ((x + np.linspace(-3, 3, n)) * np.logspace(-2, 2, n)).astype(dtype)
    r, means, scales = _cov(torch, ctx, x, kind, correlation=True)
    assert means.shape == scales.shape == (1, n)
    _check_corr(x, r, scales, "corr %s %s %s" % (shape, dtype.__name__, kind))
    if dtype == np.float32 and shape == (1031, 77):
        pca_scales = _np(ctx.pca(_give(torch, x, kind), 2, seed=1, standardize=True)[3])
        rel = np.abs(scales.astype(np.float64) - pca_scales.astype(np.float64)) / pca_scales.astype(np.float64)
        print("scales against Context.pca(standardize=True): max relative difference %.3e (4 u = %.3e)" % (float(rel.max()), 4 * _u(dtype)))
        assert np.all(rel <= 4 * _u(dtype))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_constant_and_zero_columns_and_a_column_scaled_by_a_million(torch, ctx, dtype, kind):
    m, n = 1031, 77
    x = _gauss(m, n, dtype, seed=3)
    x[:, 5] = 3.25
    x[:, 70] = 0.0
    x[:, 9] *= dtype(1.0e6)
    r, means, scales = _cov(torch, ctx, x, kind, correlation=True)
    _check_corr(x, r, scales, "corr constant/zero/1e6 %s %s" % (dtype.__name__, kind), dead=(5, 70))
    assert means[0, 5] == dtype(3.25) and means[0, 70] == 0


# ---- structure -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_repeatable_and_independent_of_the_padding_of_c(torch, ctx, dtype):
    """two calls are bitwise equal; with ldc > n the result does not depend on what the padding held, and the padding is
    left as it was (the raw device entry: Context.cov always passes ldc = n)"""
    m, n, ldc = 1031, 200, 211
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    x = torch.from_numpy(_gauss(m, n, dtype, seed=4)).cuda()
    a, _, _ = ctx.cov(x)
    b, _, _ = ctx.cov(x)
    assert ctx.last_cov_route() == "inplace" and torch.equal(a, b) and torch.equal(a, a.t())
    fn = getattr(ctx._lib, "corrla_cov_dev_f32" if dtype == np.float32 else "corrla_cov_dev_f64")
    outs = []
    for fill in (float("nan"), 7.0):
        cbuf = torch.full((n, ldc), fill, dtype=tdt, device="cuda")
        means = torch.empty(n, dtype=tdt, device="cuda")
        route = C.c_int(0)
        torch.cuda.synchronize()
        rc = fn(ctx._h, x.data_ptr(), m, n, n, 1, 0, 1, means.data_ptr(), None, cbuf.data_ptr(), ldc, C.byref(route))
        assert rc == 0 and route.value == 1
        assert ctx._lib.corrla_ctx_synchronize(ctx._h) == 0
        pad = cbuf[:, n:]
        assert bool(torch.isnan(pad).all()) if math.isnan(fill) else bool((pad == fill).all()), "the padding of c was written"
        outs.append(cbuf[:, :n].clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], a)


# ---- the reference's own tests (stats_corr.rs:259-298, 394-415) ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_reference_cov_and_pearson_of_uncorrelated_gaussians(torch, ctx, dtype):
    import corrla_rs_amd as cr
    x = torch.empty(REFERENCE_SHAPE, dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
    ctx.fill_normal(x, 20241008)
    for fn in (cr.mat_cov_centered, cr.pearson_corr):
        got = _np(fn(x, ctx=ctx))
        assert ctx.last_cov_route() == "inplace_checked"       # rows of 5 elements are not 16-byte multiples
        assert got.shape == (5, 5) and np.abs(got - np.eye(5)).max() < 1e-1, got
        assert np.abs(_np(fn(_np(x), ctx=ctx)) - got).max() <= 1e-5


def test_reference_rsquared_sens(ctx):
    import corrla_rs_amd as cr
    rng = np.random.default_rng(394)
    x = (np.array([[0.9, 0.5], [0.5, 0.9]]) @ rng.standard_normal((2, 100))).T.copy()    # sample_mv_normal(cov, 100)
    y = (x[:, 0] + x[:, 1] ** 2).reshape(-1, 1)
    got = cr.rsquared_sens(x, y, True, ctx=ctx)
    assert ctx.last_cov_route() in ("inplace", "inplace_checked") and got.shape == (1, 1)
    r = np.corrcoef(np.hstack([x, y]), rowvar=False)
    u, s, vt = np.linalg.svd(r[:2, :2])
    want = r[:2, 2:].T @ ((vt.T * (1.0 / (s + 1.0e-14))) @ u.T) @ r[:2, 2:]
    want = 1.0 - (1.0 - want) * (99.0 / 97.0)
    print("rsquared_sens: %.12f (numpy restatement %.12f)" % (got[0, 0], want[0, 0]))
    assert abs(got[0, 0] - want[0, 0]) <= 1e-10 and 0.0 < got[0, 0] < 1.0
