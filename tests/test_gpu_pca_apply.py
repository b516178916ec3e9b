"""The fitted PCA model on the GPU: Context.pca_transform / pca_inverse_transform and the PcaRsvd methods over them
(corrla_pca_transform_*, corrla_pca_inverse_*, csrc/pca_apply_kernels.hpp).  Run with -m gpu on an MI355X.

Every case runs in f32 and f64, with host pointers (numpy) and with CUDA tensors, and asserts the route of the back-projection
kernel (last_pca_apply_route) and the centring of the forward product (last_pca_apply_centring), so that no other path can
stand in for them.  tests/test_pca_apply_plan.py pins on the CPU what plan each call of this file gets (GPU_CALLS there); the
shapes come from its tables: m, n around the tile (BM, BN), k around the chunk (KC).

Bounds.  u = 2^-24 (f32) / 2^-53 (f64), gamma_p = p u / (1 - p u); z = (x - mu) / sigma; the reference is numpy in f64 on the
same stored values.  The f64 cases evaluate that reference in numpy's extended precision (longdouble; 2^-64 on x86): an f64
reference carries an error of the size of the bound it is to judge (at k = 1 its three roundings against the kernel's two),
and which of the two is off would depend on the order numpy's matmul happens to sum in.  The bounds are not widened for it.
  scores, fused  |t^ - t|_ic <= gamma_{n+8} sum_j (|x_ij| + |mu_j|) / sigma_j |V_cj|
  scores, copy   |t^ - t|_ic <= gamma_{n+8} sum_j |z_ij| |V_cj| + 4 u |t_ic|
  inverse        |xh^ - xh|_ij <= gamma_{k+4} sigma_j sum_c |t_ic| |V_cj| + 2 u |xh_ij|
  residual       q_i is taken from the scores AS STORED (t^, rounded to T): q_i = ||z_i - t^_i V||^2.  With
                 e_ij = gamma_{k+8} (|z_ij| + sum_c |t^_ic| |V_cj|) and E_i = ||e_i||_2:
                 |q^_i - q_i| <= 2 sqrt(q_i) E_i + E_i^2 + gamma_{n+8} q_i
The exact cases use integers in [-3, 3] for x, mu and V with sigma = 1: scores and reconstruction sums stay below 2^14.  The
residual squares a difference that holds t V, so with a dense V its sums would leave the exactly representable integers of
f32 (2^24); its exact case takes V with one entry of [-3, 3] per row, in distinct columns: every sum stays below 2^20."""
import functools

import numpy as np
import pytest

from tests.test_pca_apply_plan import (BM, BN, CHECKED, CSR_SHAPE, INPLACE, LAYOUTS, LOWRANK_SHAPE, REPACKED, RESID, STORE,
                                       layout_call, layout_shapes, shapes)

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
KINDS = ("host", "dev")
ROUTE_NAME = {INPLACE: "inplace", CHECKED: "inplace_checked", REPACKED: "repacked"}
# the PCA parity tolerance of tests/test_gpu_pca_standardize.py (projector): f64 / f32
PCA_PARITY_TOL = {np.float64: 1e-7, np.float32: 2e-3}


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


def _u(dtype):
    return 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53


def _gamma(p, u):
    return p * u / (1.0 - p * u)


def _wide(dtype):
    """the type the reference is evaluated in: f64 for the f32 cases, extended precision for the f64 cases"""
    return np.float64 if dtype == np.float32 else np.longdouble


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _esz(dtype):
    return np.dtype(dtype).itemsize


def _in_layout(a, layout):
    """the values of a (m x n) in a fresh array of `layout`, its base 16-byte aligned (one element past for base_plus_1)"""
    m, n = a.shape
    it = a.itemsize

    def flat(count, off):
        raw = np.zeros(count + 16 // it + 2, dtype=a.dtype)
        start = (-raw.ctypes.data % 16) // it + off
        return raw[start:start + count]
    if layout == "contiguous":
        v = flat(m * n, 0).reshape(m, n)
    elif layout == "row_stride_n_plus_1":
        v = flat(m * (n + 1), 0).reshape(m, n + 1)[:, :n]
    elif layout == "base_plus_1":
        v = flat(m * n, 1).reshape(m, n)
    else:
        v = flat(m * n, 0).reshape(n, m).T
    v[...] = a
    assert v.ctypes.data % 16 == (it if layout == "base_plus_1" else 0)
    return v


def _give(torch, x, kind):
    """x (a numpy view of any layout) as the host or device operand with the SAME strides and the same offset of its base
    from a 16-byte boundary"""
    if kind == "host":
        return x
    span = (x.shape[0] - 1) * x.strides[0] // x.itemsize + (x.shape[1] - 1) * x.strides[1] // x.itemsize + 1
    off = (x.ctypes.data % 16) // x.itemsize
    flat = torch.zeros(span + off, dtype=torch.float32 if x.dtype == np.float32 else torch.float64, device="cuda")
    t = torch.as_strided(flat, x.shape, tuple(s // x.itemsize for s in x.strides), off)
    t.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert t.data_ptr() % 16 == x.ctypes.data % 16
    return t


@functools.lru_cache(maxsize=None)
def _case(m, n, k, dtype, seed=0):
    """x, mu, sigma, V as stored in dtype (read-only): columns of different scale and offset, a model that is NOT the fit of
    x (the bounds hold for any model) and a V that is not orthonormal (the direct residual does not need it to be)"""
    rng = np.random.default_rng(1000 * m + 10 * n + k + seed)
    sd = rng.uniform(0.5, 2.0, n)
    mu = rng.standard_normal(n) * sd
    x = (rng.standard_normal((m, n)) * sd + mu + 0.3 * sd * rng.standard_normal(n)).astype(dtype)
    v = (rng.standard_normal((k, n)) / np.sqrt(n)).astype(dtype)
    out = (x, mu.astype(dtype), sd.astype(dtype), v)
    for a in out:
        a.setflags(write=False)
    return out


def _ref(dtype, *arrs):
    return [None if a is None else np.asarray(a, dtype=_wide(dtype)) for a in arrs]


def _z(x, mu, sd, dtype=np.float32):
    x, mu, sd = _ref(dtype, x, mu, sd)
    z = x if mu is None else x - mu
    return z if sd is None else z / sd


def _check_scores(t_hat, x, mu, sd, v, centring, dtype, what):
    x64, mu64, sd64, v64 = _ref(dtype, x, mu, sd, v)
    n = x64.shape[1]
    u = _u(dtype)
    z = _z(x, mu, sd, dtype)
    t = z @ v64.T
    if centring == "fused":
        spread = np.abs(x64) + (0.0 if mu64 is None else np.abs(mu64))
        bound = _gamma(n + 8, u) * ((spread if sd64 is None else spread / sd64) @ np.abs(v64).T)
    else:
        bound = _gamma(n + 8, u) * (np.abs(z) @ np.abs(v64).T) + 4 * u * np.abs(t)
    err = np.abs(np.asarray(t_hat, dtype=_wide(dtype)) - t)
    worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
    print(f"{what}: scores ({centring}) worst error / bound {worst:.3e}")
    assert np.all(err <= bound), (what, centring, worst)
    return bound


def _check_resid(q_hat, t_hat, x, mu, sd, v, dtype, what):
    v64, t64 = _ref(dtype, v, t_hat)
    k, n = v64.shape
    u = _u(dtype)
    z = _z(x, mu, sd, dtype)
    q = np.sum((z - t64 @ v64) ** 2, axis=1)
    e = _gamma(k + 8, u) * (np.abs(z) + np.abs(t64) @ np.abs(v64))
    big_e = np.sqrt(np.sum(e * e, axis=1))
    bound = 2 * np.sqrt(q) * big_e + big_e ** 2 + _gamma(n + 8, u) * q
    err = np.abs(np.asarray(q_hat, dtype=_wide(dtype)) - q)
    worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
    print(f"{what}: residual worst error / bound {worst:.3e}")
    assert np.all(err <= bound), (what, worst)
    return q, bound


def _check_inverse(xh_hat, t, mu, sd, v, dtype, what):
    t64, mu64, sd64, v64 = _ref(dtype, t, mu, sd, v)
    k = v64.shape[0]
    u = _u(dtype)
    back, mag = t64 @ v64, np.abs(t64) @ np.abs(v64)
    if sd64 is not None:
        back, mag = back * sd64, mag * sd64
    if mu64 is not None:
        back = back + mu64
    bound = _gamma(k + 4, u) * mag + 2 * u * np.abs(back)
    err = np.abs(np.asarray(xh_hat, dtype=_wide(dtype)) - back)
    worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
    print(f"{what}: inverse worst error / bound {worst:.3e}")
    assert np.all(err <= bound), (what, worst)
    return back, bound


def _default_centring(dtype):
    return "copy" if dtype == np.float32 else "fused"


def _transform(torch, ctx, xv, mu, sd, v, kind, route, **kw):
    """Context.pca_transform on xv (a numpy view in the layout under test) -> numpy results; asserts kinds and the route"""
    res = ctx.pca_transform(_give(torch, xv, kind), mu, v, sd, **kw)
    res = res if isinstance(res, tuple) else (res,)
    assert ctx.last_pca_apply_route() == (ROUTE_NAME[route] if kw.get("residuals") else None), (ctx.last_pca_apply_route(), route)
    for r in res:
        assert (r.is_cuda if kind == "dev" else type(r) is np.ndarray) and _np(r).dtype == xv.dtype
    return tuple(_np(r) for r in res)


# ---- every shape of the table: bounds -------------------------------------------------------------------------------------
def _shape_params():
    return [pytest.param(dt, c, id="%s-%dx%dx%d" % (("f32", "f64")[dt == np.float64], *c)) for dt in DTYPES for c in shapes(_esz(dt))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,case", _shape_params())
def test_scores_residuals_and_inverse_meet_their_bounds(torch, ctx, dtype, case, kind):
    m, n, k = case
    x, mu, sd, v = _case(m, n, k, dtype)
    what = f"{np.dtype(dtype).name} {kind} {m}x{n} k={k}"
    xv = _in_layout(x, "contiguous")
    route = layout_call(m, n, k, _esz(dtype), "contiguous", RESID)[-1]
    t_hat, q_hat = _transform(torch, ctx, xv, mu, sd, v, kind, route, residuals=True)
    assert ctx.last_pca_apply_centring() == _default_centring(dtype)
    assert t_hat.shape == (m, k) and q_hat.shape == (m,)
    _check_scores(t_hat, x, mu, sd, v, _default_centring(dtype), dtype, what)
    _check_resid(q_hat, t_hat, x, mu, sd, v, dtype, what)
    # the inverse of the stored scores; its output is contiguous, so the route follows n
    xh = ctx.pca_inverse_transform(_give(torch, np.asfortranarray(t_hat), kind), mu, v, sd)
    assert ctx.last_pca_apply_route() == ROUTE_NAME[layout_call(m, n, k, _esz(dtype), "contiguous", STORE)[-1]]
    assert (xh.is_cuda if kind == "dev" else type(xh) is np.ndarray) and tuple(xh.shape) == (m, n) and _np(xh).dtype == dtype
    _check_inverse(_np(xh), t_hat, mu, sd, v, dtype, what)


# ---- every shape of the table: integers are exact -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ints(m, n, k):
    rng = np.random.default_rng(7 * m + 3 * n + k)
    x = rng.integers(-3, 4, size=(m, n)).astype(np.float64)
    mu = rng.integers(-3, 4, size=n).astype(np.float64)
    v = rng.integers(-3, 4, size=(k, n)).astype(np.float64)
    t_small = rng.integers(-3, 4, size=(m, k)).astype(np.float64)
    # one entry per row, in distinct columns: the V of the exact residual
    v1 = np.zeros((k, n))
    v1[np.arange(k), rng.permutation(n)[:k]] = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], size=k)
    t, t1 = (x - mu) @ v.T, (x - mu) @ v1.T
    q1 = np.sum(((x - mu) - t1 @ v1) ** 2, axis=1)
    assert max(np.abs(t).max(), np.abs(t_small @ v + mu).max()) < 1 << 14 and q1.max() < 1 << 20
    return x, mu, v, t, t_small, t_small @ v + mu, v1, t1, q1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,case", _shape_params())
def test_integer_models_are_exact(torch, ctx, dtype, case, kind):
    """the lane map of the MFMA tiles and the predication of the edge tiles: any slip moves an integer"""
    m, n, k = case
    x, mu, v, t, t_small, back, v1, t1, q1 = _ints(m, n, k)
    xv = _in_layout(x.astype(dtype), "contiguous")
    route = layout_call(m, n, k, _esz(dtype), "contiguous", RESID)[-1]
    for center in (None, "fused", "copy"):
        (t_hat,) = _transform(torch, ctx, xv, mu.astype(dtype), None, v.astype(dtype), kind, route, center=center)
        assert np.array_equal(t_hat, t), (center, np.abs(t_hat - t).max())
    t_hat, q_hat = _transform(torch, ctx, xv, mu.astype(dtype), None, v1.astype(dtype), kind, route, residuals=True)
    assert np.array_equal(t_hat, t1) and np.array_equal(q_hat, q1), np.abs(q_hat - q1).max()
    xh = ctx.pca_inverse_transform(_give(torch, np.asfortranarray(t_small.astype(dtype)), kind), mu.astype(dtype), v.astype(dtype))
    assert np.array_equal(_np(xh), back), np.abs(_np(xh) - back).max()


# ---- layouts of x (residuals) and of the output (inverse) --------------------------------------------------------------------
def _inverse_raw(torch, ctx, t, mu, sd, v, out_view, kind):
    """corrla_pca_inverse_* itself, so that the output can be a view of any row stride and alignment (the Python surface
    always allocates a contiguous one) -> the output as numpy"""
    from corrla_rs_amd import _lib as L
    from corrla_rs_amd import api
    m, k = t.shape
    n = v.shape[1]
    tf, vf = np.asfortranarray(t), np.asfortranarray(v)
    keep = [_give(torch, a.reshape(1, -1) if a.ndim == 1 else a, kind) for a in (tf.T, mu, sd, vf.T)]   # (k, m) / (n, k) row-major
    out = _give(torch, out_view, kind)
    if kind == "dev":
        torch.cuda.synchronize()
    fn = ctx._entry("corrla_pca_inverse_", kind == "dev", out_view.dtype)
    L.check(fn(ctx._h, api._ptr(keep[0]), m, k, m, api._ptr(keep[1]), api._ptr(keep[2]), api._ptr(keep[3]), k, n, api._ptr(out),
               out_view.strides[0] // out_view.itemsize))
    ctx._pca_apply_done(kind == "dev")
    return _np(out)


def _layout_params():
    return [pytest.param(dt, c, id="%s-%dx%dx%d" % (("f32", "f64")[dt == np.float64], *c)) for dt in DTYPES for c in layout_shapes(_esz(dt))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype,case", _layout_params())
def test_layouts_take_their_routes_and_meet_the_bounds(torch, ctx, dtype, case, layout, kind):
    m, n, k = case
    x, mu, sd, v = _case(m, n, k, dtype, seed=1)
    what = f"{np.dtype(dtype).name} {kind} {m}x{n} k={k} {layout}"
    route = layout_call(m, n, k, _esz(dtype), layout, RESID)[-1]
    xv = _in_layout(x, layout)
    t_hat, q_hat = _transform(torch, ctx, xv, mu, sd, v, kind, route, residuals=True)
    _check_scores(t_hat, x, mu, sd, v, _default_centring(dtype), dtype, what)
    _check_resid(q_hat, t_hat, x, mu, sd, v, dtype, what)
    if layout == "column_major":
        return
    out_view = _in_layout(np.full((m, n), -7.5, dtype=dtype), layout)
    xh = _inverse_raw(torch, ctx, t_hat, mu, sd, v, out_view, kind)
    assert ctx.last_pca_apply_route() == ROUTE_NAME[layout_call(m, n, k, _esz(dtype), layout, STORE)[-1]]
    _check_inverse(xh, t_hat, mu, sd, v, dtype, what)
    if layout == "row_stride_n_plus_1" and kind == "host":
        # the element between two rows of the view (zero since _in_layout made the array) was not written
        gaps = np.lib.stride_tricks.as_strided(out_view[:, n - 1:], shape=(m - 1, 2), strides=out_view.strides)[:, 1]
        assert np.all(gaps == 0), "the padding between the rows was written"


# ---- the switches of the forward product ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_centring_switches_own_means_and_missing_model_parts(torch, ctx, dtype, kind):
    m, n, k = 2 * BM + 3, BN + 1, 5
    x, mu, sd, v = _case(m, n, k, dtype, seed=2)
    xv = _in_layout(x, "contiguous")
    route = layout_call(m, n, k, _esz(dtype), "contiguous", RESID)[-1]
    what = f"{np.dtype(dtype).name} {kind}"
    for center in ("fused", "copy"):
        for scales in (sd, None):
            t_hat, q_hat = _transform(torch, ctx, xv, mu, scales, v, kind, route, residuals=True, center=center)
            assert ctx.last_pca_apply_centring() == center
            _check_scores(t_hat, x, mu, scales, v, center, dtype, f"{what} {center} scales={scales is not None}")
            _check_resid(q_hat, t_hat, x, mu, scales, v, dtype, what)
    # no means: no centring at all without scales, scaling about zero with them
    (t_hat,) = _transform(torch, ctx, xv, None, None, v, kind, route)
    assert ctx.last_pca_apply_centring() is None
    _check_scores(t_hat, x, None, None, v, "copy", dtype, what + " plain")
    t_hat, q_hat = _transform(torch, ctx, xv, None, sd, v, kind, route, residuals=True)
    _check_scores(t_hat, x, None, sd, v, _default_centring(dtype), dtype, what + " scales only")
    _check_resid(q_hat, t_hat, x, None, sd, v, dtype, what + " scales only")
    # own means: what the reference's apply_tr does; the means of x come back, within one rounding of the f64 mean plus
    # the bound of the length-m dot product that formed them
    for center in ("fused", "copy"):
        t_hat, q_hat, own = _transform(torch, ctx, xv, mu, sd, v, kind, route, residuals=True, own_means=True, center=center)
        assert own.shape == (1, n)
        xw = x.astype(_wide(dtype))
        assert np.all(np.abs(own[0] - xw.mean(axis=0)) <= _gamma(m + 8, _u(dtype)) * np.abs(xw).mean(axis=0))
        _check_scores(t_hat, x, own[0], sd, v, center, dtype, what + " own means " + center)
        _check_resid(q_hat, t_hat, x, own[0], sd, v, dtype, what + " own means")


@pytest.mark.parametrize("kind", KINDS)
def test_the_f32_default_centres_a_copy_when_the_means_dwarf_the_spread(torch, ctx, kind):
    """mu_j = 10^3 sigma_j: the fused form's own bound is 10^3 times the copy's here, so meeting the copy bound on the default
    route pins the default"""
    m, n, k = 2 * BM + 3, BN + 1, 5
    rng = np.random.default_rng(11)
    sd = rng.uniform(0.5, 2.0, n).astype(np.float32)
    mu = (1.0e3 * sd).astype(np.float32)
    x = (mu + sd * rng.standard_normal((m, n))).astype(np.float32)
    v = (rng.standard_normal((k, n)) / np.sqrt(n)).astype(np.float32)
    xv = _in_layout(x, "contiguous")
    (t_hat,) = _transform(torch, ctx, xv, mu, sd, v, kind, CHECKED)
    assert ctx.last_pca_apply_centring() == "copy"
    _check_scores(t_hat, x, mu, sd, v, "copy", np.float32, "mu = 1e3 sigma")


# ---- Q-residuals where they matter: data the model explains almost fully --------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_low_rank_plus_noise_residuals(torch, ctx, kind):
    m, n, r = LOWRANK_SHAPE
    rng = np.random.default_rng(2024)
    x = (rng.standard_normal((m, r)) @ rng.standard_normal((r, n)) + 1e-3 * rng.standard_normal((m, n))).astype(np.float32)
    x64 = x.astype(np.float64)
    mu64 = x64.mean(axis=0)
    v64 = np.linalg.svd(x64 - mu64, full_matrices=False)[2][:r]
    mu, v = mu64.astype(np.float32), v64.astype(np.float32)
    t_hat, q_hat = _transform(torch, ctx, _in_layout(x, "contiguous"), mu, None, v, kind,
                              layout_call(m, n, r, 4, "contiguous", RESID)[-1], residuals=True)
    q, _ = _check_resid(q_hat, t_hat, x, mu, None, v, np.float32, "low rank + noise")
    rel = np.abs(q_hat - q) / q
    z = _z(x, mu, None)
    q_pure = np.sum((z - (z @ v.astype(np.float64).T) @ v.astype(np.float64)) ** 2, axis=1)   # f64 scores instead of the stored ones
    rel_pure = np.abs(q_hat - q_pure) / q_pure
    # the difference form in f32, for contrast: what the direct form is there to avoid
    zf = (x - mu).astype(np.float32)
    diff = np.sum(zf * zf, axis=1, dtype=np.float32) - np.sum(t_hat * t_hat, axis=1, dtype=np.float32)
    rel_diff = np.abs(diff - q) / q
    print(f"low rank + noise: q relative error direct {rel.max():.3e} (against f64 scores {rel_pure.max():.3e}), difference form {rel_diff.max():.3e}")
    assert rel.max() <= 1e-2 and rel_pure.max() <= 1e-2
    assert rel_diff.max() > 1e-2, "the difference form was expected to fail on this case"


# ---- reproducibility, round trip ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_two_runs_are_bitwise_equal_and_the_round_trip_returns_x(torch, ctx, dtype, kind):
    m, n = 2 * BM + 3, BN + 1
    k = n
    rng = np.random.default_rng(5)
    x, mu, sd, _ = _case(m, n, 5, dtype, seed=3)
    v64 = np.linalg.qr(rng.standard_normal((n, n)))[0]
    v = v64.astype(dtype)
    xv = _in_layout(x, "contiguous")
    route = layout_call(m, n, k, _esz(dtype), "contiguous", RESID)[-1]
    a = _transform(torch, ctx, xv, mu, sd, v, kind, route, residuals=True)
    b = _transform(torch, ctx, xv, mu, sd, v, kind, route, residuals=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    t_hat = a[0]
    give_t = _give(torch, np.asfortranarray(t_hat), kind)
    xh, xh2 = (_np(ctx.pca_inverse_transform(give_t, mu, v, sd)) for _ in range(2))
    assert np.array_equal(xh, xh2)
    # the sum of the two bounds: the scores' error carried through V and sigma, plus the inverse's own; the defect of the
    # rounded V from orthogonality separates the f64 round trip from x and is added as it is
    what = f"{np.dtype(dtype).name} {kind} round trip"
    bt = _check_scores(t_hat, x, mu, sd, v, _default_centring(dtype), dtype, what)
    _, bx = _check_inverse(xh, t_hat, mu, sd, v, dtype, what)
    vd, sdw = v.astype(_wide(dtype)), sd.astype(_wide(dtype))
    defect = (np.abs(_z(x, mu, sd, dtype)) @ np.abs(vd.T @ vd - np.eye(n))) * sdw
    err = np.abs(xh.astype(_wide(dtype)) - x.astype(_wide(dtype)))
    assert np.all(err <= (bt @ np.abs(vd)) * sdw + bx + defect + 2 * _u(dtype) * np.abs(x)), float(err.max())
    # k = n with an orthogonal V explains everything: the residual is rounding, and the bound knows
    _check_resid(a[1], t_hat, x, mu, sd, v, dtype, what)


# ---- CSR -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_csr_scores_equal_the_dense_calls(torch, ctx, dtype, kind):
    m, n, k = CSR_SHAPE
    rng = np.random.default_rng(9)
    dense = np.where(rng.random((m, n)) < 0.05, rng.standard_normal((m, n)), 0.0).astype(dtype)
    dense[0, 0] = 1.0
    _, mu, sd, v = _case(m, n, k, dtype, seed=4)
    indptr = np.concatenate([[0], np.cumsum((dense != 0).sum(axis=1))]).astype(np.int64)
    indices = np.nonzero(dense)[1].astype(np.int32)
    data = dense[dense != 0]
    if kind == "dev":
        a = torch.sparse_csr_tensor(torch.from_numpy(indptr), torch.from_numpy(indices.astype(np.int64)), torch.from_numpy(data),
                                    size=(m, n)).cuda()
    else:
        a = (data, indices, indptr, (m, n))
    t_csr = ctx.pca_transform(a, mu, v, sd)
    assert ctx.last_pca_apply_centring() == "fused" and ctx.last_pca_apply_route() is None
    assert t_csr.is_cuda if kind == "dev" else type(t_csr) is np.ndarray
    (t_dense,) = _transform(torch, ctx, _in_layout(dense, "contiguous"), mu, sd, v, kind, CHECKED, center="fused")
    what = f"{np.dtype(dtype).name} {kind} csr"
    bound = _check_scores(_np(t_csr), dense, mu, sd, v, "fused", dtype, what)
    assert np.all(np.abs(_np(t_csr).astype(np.float64) - t_dense.astype(np.float64)) <= bound)
    own = ctx.pca_transform(a, None, v, sd, own_means=True)
    _check_scores(_np(own[0]), dense, _np(own[1])[0], sd, v, "fused", dtype, what + " own means")
    with pytest.raises(ValueError, match="residuals=True on sparse input"):
        ctx.pca_transform(a, mu, v, sd, residuals=True)


# ---- PcaRsvd end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_pca_rsvd_fits_a_cuda_tensor_and_transforms_on_the_device(torch, ctx, dtype):
    import corrla_rs_amd as cr
    m, n, k = 400, 96, 4
    rng = np.random.default_rng(21)
    # rank k after centring, well separated: U diag(S) of the centred matrix IS its projection on the components
    x = ((rng.standard_normal((m, k)) * np.array([8.0, 4.0, 2.0, 1.0])) @ np.linalg.qr(rng.standard_normal((n, k)))[0].T
         + rng.standard_normal(n)).astype(dtype)
    omega = rng.standard_normal((n, k + 10))
    xt = torch.tensor(x, device="cuda")
    model = cr.PcaRsvd(xt, k, omega=omega, ctx=ctx)
    for part in (model.means, model.pca_s, model.components_):
        assert part.is_cuda and _np(part).dtype == dtype
    assert model.scales_ is None and model.n_samples == m
    t = model.transform(xt)
    assert t.is_cuda and tuple(t.shape) == (m, k)
    centred = xt - xt.mean(dim=0, keepdim=True)
    u, s, _vt = ctx.rsvd(centred, k, 20, 10, omega=omega)
    us, t_np = _np(u) * _np(s).reshape(1, k), _np(t).astype(np.float64)
    tol = PCA_PARITY_TOL[dtype] * float(_np(s)[0, 0])
    for c in range(k):
        d = min(np.abs(t_np[:, c] - us[:, c]).max(), np.abs(t_np[:, c] + us[:, c]).max())
        assert d <= tol, (c, d, tol)
    # fit_transform is fit + transform; the residual of rank-k data under a rank-k model is rounding
    model2 = cr.PcaRsvd.__new__(cr.PcaRsvd)
    t2 = model2.fit_transform(xt, k, omega=omega, ctx=ctx)
    assert torch.equal(t2, t)
    q = model.residuals(xt)
    assert q.is_cuda and tuple(q.shape) == (m,)
    _check_resid(_np(q), _np(t), x, _np(model.means)[0], None, _np(model.components_), dtype, "PcaRsvd residuals")
    back = model.inverse_transform(t)
    _check_inverse(_np(back), _np(t), _np(model.means)[0], None, _np(model.components_), dtype, "PcaRsvd inverse")
    # apply_tr on a tensor against the numpy apply_tr of a host-fitted model, each with its own (nearly equal) components
    host = cr.PcaRsvd(x, k, omega=omega, ctx=ctx)
    assert type(host.components_) is np.ndarray
    targ = (x[:100] + 0.1 * rng.standard_normal((100, n))).astype(dtype)
    want = host.apply_tr(targ)
    got = host.apply_tr(torch.tensor(targ, device="cuda"))     # a CUDA argument takes the device path on a host-fitted model
    assert got.is_cuda
    t_direct, own = ctx.pca_transform(torch.tensor(targ, device="cuda"), None, host.components_, own_means=True)
    assert torch.equal(t_direct, got)
    bound = _check_scores(_np(got), targ, _np(own)[0], None, host.components_, _default_centring(dtype), dtype, "apply_tr")
    gap = np.abs(_np(got).astype(np.float64) - want.astype(np.float64))
    print(f"apply_tr tensor against numpy: worst difference / scores bound {float(np.max(gap / bound)):.3e}")
    assert np.all(gap <= bound)
    # numpy in, numpy out -- on the host-fitted model by the numpy formula, on the device-fitted one through the kernel
    back_host, back_dev = host.apply_inv_tr(want), model.apply_inv_tr(want)
    assert type(back_host) is np.ndarray and type(back_dev) is np.ndarray and ctx.last_pca_apply_route() is not None
    _check_inverse(back_dev, want, _np(model.means)[0], None, _np(model.components_), dtype, "apply_inv_tr")
    assert model.apply_inv_tr(got).is_cuda
