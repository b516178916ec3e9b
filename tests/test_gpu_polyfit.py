"""The polynomial response-surface kernels on the GPU (Context.polyfit_gram / poly_eval and the callers linear_fit, quad_fit,
quad_eval, jac_from_lin, jac_from_quad) against numpy in extended precision and the restated reference
(tests/polyfit_reference.py).  The shapes come from tests/test_polyfit_plan.py, which pins what each of them exercises.

Bounds, none of them tuned:
  Gram        every entry within (m + 8) 2^-53 sum_i |w_i| |w_j| of the np.longdouble Gram of the SAME f64 W -- the bound of a
              dot product of m terms in any order.  W is formed here as the kernel forms it, z = (x - means) * (1 / scales)
              in f64 from the means and scales the call returned, and each column as one f64 product.
  evaluation  (2 k + 8) 2^-53 |xt|^T |C| |xt| for the values and likewise per gradient component; one more rounding of the
              result for float32 output.
  fits        10 x the discrepancy the same host solve shows against the reference route when it is fed numpy's own f64
              Gram of that input, floor 1e-13 relative; both sides of that come from the reference, never from the device.
  jac_from_quad against the reference's forward difference: 4 * 2^-52 max|y| / 1e-10, the rounding error of that difference."""
import numpy as np
import pytest

from tests import polyfit_reference as R
from tests.test_polyfit_host import KNOWN, host_fit, rel
from tests.test_polyfit_plan import SLAB_COUNT, SLAB_KNOB, SLAB_M, gpu_eval_shapes, gpu_gram_shapes, poly_terms

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
KINDS = ("host", "dev")
U = 2.0 ** -53


def _combos(shapes):
    """(shape, dtype, kind): every pairing for the small shapes; for those whose extended-precision reference takes a
    noticeable part of a second (order of G above 300) each dtype and each kind once"""
    out = []
    for sh in shapes:
        big = poly_terms(sh[1], sh[3]) + sh[2] > 300
        out += [(sh, dt, kd) for dt in DTYPES for kd in KINDS if not big or (dt is np.float64) == (kd == "host")]
    return out


def _combo_id(c):
    return f"{c[0]}-{c[1].__name__}-{c[2]}"


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


def _ctx_with_slab_rows(rows):
    """the plan knobs are read when a context is created"""
    import corrla_rs_amd as cr
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CORRLA_POLYFIT_SLAB_ROWS", str(rows))
        return cr.Context(0)


@pytest.fixture(scope="module")
def ctx_slabs():
    c = _ctx_with_slab_rows(SLAB_KNOB)
    yield c
    c.close()


def _layout(a, layout):
    """the same values as a view: 'tight', 'padded' (row stride > columns) or 'offset' (base one element off the buffer)"""
    m, n = a.shape
    if layout == "tight":
        return np.ascontiguousarray(a)
    if layout == "padded":
        buf = np.full((m, n + 3), np.nan, dtype=a.dtype)
        buf[:, :n] = a
        return buf[:, :n]
    buf = np.empty(m * n + 1, dtype=a.dtype)
    v = buf[1:].reshape(m, n)
    v[...] = a
    return v


def _give(torch, a, kind):
    """numpy stays numpy (host entries); 'dev': a CUDA tensor with the same strides and the same offset from its buffer"""
    if kind == "host" or a is None:
        return a
    base = a.base if a.base is not None else a
    t = torch.from_numpy(np.ascontiguousarray(base).copy()).cuda()
    off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // a.itemsize
    return torch.as_strided(t, a.shape, tuple(s // a.itemsize for s in a.strides), off)


def _np(v):
    return None if v is None else (v if isinstance(v, np.ndarray) else v.cpu().numpy())


def w_of(x, y, degree, means, scales):
    """W = [V(z), y] in f64, operation for operation what the kernel stages"""
    z = x.astype(np.float64)
    if means is not None:
        z = (z - means.reshape(-1)) * (1.0 / scales.reshape(-1))
    cols = [R.build_full_vandermonde(z, degree)]
    if y is not None:
        cols.append(y.astype(np.float64))
    return np.hstack(cols)


def assert_gram_within_bound(g, w, what):
    wl = w.astype(np.longdouble)
    ref = wl.T @ wl
    bound = (w.shape[0] + 8) * U * (np.abs(wl).T @ np.abs(wl))
    err = np.abs(g.astype(np.longdouble) - ref)
    worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert np.all(err <= bound), what
    assert np.array_equal(g, g.T), what


def _data(m, k, r, dtype, seed, integers=False):
    rng = np.random.default_rng(seed)
    if integers:
        x = rng.integers(-3, 4, size=(m, k)).astype(dtype)
        y = rng.integers(-5, 6, size=(m, r)).astype(dtype) if r else None
    else:
        x = (rng.random((m, k)) * 2.0 + 0.5).astype(dtype)
        y = rng.standard_normal((m, r)).astype(dtype) if r else None
    return x, y


# ---- 1. exact Gram ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", _combos(gpu_gram_shapes()), ids=_combo_id)
def test_exact_gram_of_small_integers(ctx, torch, combo):
    (m, k, r, degree), dtype, kind = combo
    x, y = _data(m, k, r, dtype, m * 131 + k, integers=True)
    w = w_of(x, y, degree, None, None).astype(np.int64)
    want = w.T @ w                                           # |entries| <= 81 m: exact in f64 in any order
    for layout in ("tight", "padded", "offset"):
        g, means, scales = ctx.polyfit_gram(_give(torch, _layout(x, layout), kind), _give(torch, y, kind), degree, normalize=False)
        assert means is None and scales is None
        g = _np(g)
        assert g.dtype == np.float64 and g.shape == (poly_terms(k, degree) + r,) * 2
        assert np.array_equal(g, want.astype(np.float64)), (layout, np.argwhere(g != want)[:4])
        if layout == "tight" and (k * x.itemsize) % 16 == 0:
            assert ctx.last_polyfit_route() == "inplace"
        if layout == "offset":
            assert ctx.last_polyfit_route() == "inplace_checked"


def test_exact_gram_across_slabs(ctx_slabs):
    x, y = _data(SLAB_M, 3, 1, np.float64, 7, integers=True)
    w = w_of(x, y, 2, None, None).astype(np.int64)
    g, _, _ = ctx_slabs.polyfit_gram(x, y, normalize=False)  # 5 slabs, the last of 44 samples
    assert np.array_equal(g, (w.T @ w).astype(np.float64))
    y1 = np.ones((SLAB_M, 1))
    g, _, _ = ctx_slabs.polyfit_gram(np.ones((SLAB_M, 1)), y1, 1, normalize=False)
    assert np.array_equal(g, np.full((3, 3), float(SLAB_M)))  # every sample counted once


# ---- 2. / 3. error bound, symmetry, repeatability ---------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("combo", _combos(gpu_gram_shapes()), ids=_combo_id)
def test_gram_error_bound_symmetry_and_repeatability(ctx, torch, combo, normalize):
    shape, dtype, kind = combo
    m, k, r, degree = shape
    x, y = _data(m, k, r, dtype, m * 17 + k + r)
    layout = "padded" if (m + k) % 2 else "tight"
    xa, ya = _give(torch, _layout(x, layout), kind), _give(torch, y, kind)
    g, means, scales = ctx.polyfit_gram(xa, ya, degree, normalize=normalize)
    g2, means2, scales2 = ctx.polyfit_gram(xa, ya, degree, normalize=normalize)
    g, means, scales = _np(g), _np(means), _np(scales)
    assert np.array_equal(g, _np(g2))
    if normalize:
        assert means.shape == scales.shape == (1, k) and means.dtype == scales.dtype == np.float64
        assert np.array_equal(means, _np(means2)) and np.array_equal(scales, _np(scales2))
        x64 = x.astype(np.float64)
        sd = x64.std(axis=0)
        if m > 1:
            assert np.allclose(means.ravel(), x64.mean(axis=0), rtol=1e-12, atol=0)
            assert np.allclose(scales.ravel(), np.where(sd > 0, sd, 1.0), rtol=1e-9, atol=0)
        else:
            assert np.array_equal(scales, np.ones((1, k)))   # one sample: every column is constant
    else:
        assert means is None and scales is None
    assert_gram_within_bound(g, w_of(x, y, degree, means, scales), f"{shape} normalize={normalize} {dtype.__name__} {kind}")


def test_a_constant_column_gets_scale_one(ctx):
    x, y = _data(70, 4, 1, np.float64, 3)
    x[:, 1] = 2.5
    g, means, scales = ctx.polyfit_gram(x, y)
    assert scales[0, 1] == 1.0 and means[0, 1] == 2.5
    assert_gram_within_bound(g, w_of(x, y, 2, means, scales), "constant column")
    assert np.all(g[1, :] == 0.0)                            # z = x - mean = 0 exactly


@pytest.mark.parametrize("normalize", [False, True])
def test_slab_settings(ctx, ctx_slabs, normalize):
    """Bitwise equal across two slab settings only where the plan is the same plan (test_polyfit_plan.test_slab_knob: 50
    samples round up to the 64 of the knob); with another split the order of the additions changes and the bound holds."""
    x, y = _data(SLAB_M, 3, 1, np.float64, 11)
    g_default, means, scales = ctx.polyfit_gram(x, y, normalize=normalize)
    g_five, _, _ = ctx_slabs.polyfit_gram(x, y, normalize=normalize)
    c50 = _ctx_with_slab_rows(50)
    try:
        g_same, _, _ = c50.polyfit_gram(x, y, normalize=normalize)
    finally:
        c50.close()
    assert np.array_equal(g_five, g_same)
    w = w_of(x, y, 2, means, scales)
    assert_gram_within_bound(g_default, w, "default split")
    assert_gram_within_bound(g_five, w, f"{SLAB_COUNT} slabs")


# ---- 4. evaluation -----------------------------------------------------------------------------------------------------------
def _eval_reference(x, c, degree):
    """values (m, r), gradients (r, m, k) and their bounds in np.longdouble"""
    m, k = x.shape
    xt = np.hstack([x.astype(np.float64), np.ones((m, 1))]).astype(np.longdouble)
    vals, grads, vb, gb = [], [], [], []
    for j in range(c.shape[1]):
        cm = R.poly_sym(c[:, j].astype(np.longdouble), k, degree)
        t, ta = xt @ cm, np.abs(xt) @ np.abs(cm)
        vals.append((t * xt).sum(axis=1))
        grads.append(2 * t[:, :k])
        vb.append((2 * k + 8) * U * (ta * np.abs(xt)).sum(axis=1))
        gb.append((2 * k + 8) * U * 2 * ta[:, :k])
    return np.stack(vals, axis=1), np.stack(grads), np.stack(vb, axis=1), np.stack(gb)


def assert_eval_within_bound(v, jac, x, c, degree, what):
    vals, grads, vb, gb = _eval_reference(x, c, degree)
    if x.dtype == np.float32:                                # the result is rounded once more, to float32
        vb, gb = vb + 2.0 ** -24 * np.abs(vals), gb + 2.0 ** -24 * np.abs(grads)
    ev = np.abs(v.astype(np.longdouble) - vals)
    print(f"{what}: values worst error / bound = {float(np.max(ev / np.maximum(vb, 1e-300))):.3f}")
    assert np.all(ev <= vb), what
    if jac is not None:
        jac = jac[None] if jac.ndim == 2 else jac
        eg = np.abs(jac.astype(np.longdouble) - grads)
        print(f"{what}: gradients worst error / bound = {float(np.max(eg / np.maximum(gb, 1e-300))):.3f}")
        assert np.all(eg <= gb), what


@pytest.mark.parametrize("combo", _combos(gpu_eval_shapes()), ids=_combo_id)
def test_poly_eval_values_and_gradients(ctx, torch, combo):
    shape, dtype, kind = combo
    m, k, r, degree = shape
    x, _ = _data(m, k, 0, dtype, m * 7 + k)
    c = np.random.default_rng(k * 3 + r).standard_normal((poly_terms(k, degree), r))
    for layout in ("tight", "padded", "offset"):
        xa = _give(torch, _layout(x, layout), kind)
        v, jac = ctx.poly_eval(xa, _give(torch, c, kind), degree, jac=True)
        v2 = ctx.poly_eval(xa, c, degree)
        v, jac, v2 = _np(v), _np(jac), _np(v2)
        assert v.dtype == jac.dtype == dtype and v.shape == (m, r) and jac.shape == ((m, k) if r == 1 else (r, m, k))
        assert np.array_equal(v, v2)                         # rows are independent: with or without the gradient, the same bits
        assert_eval_within_bound(v, jac, x, c, degree, f"{shape} {layout} {dtype.__name__} {kind}")
        if layout == "offset":
            assert ctx.last_polyfit_route() == "inplace_checked"


# ---- 5. end-to-end fits --------------------------------------------------------------------------------------------------------
def _fit_case(name):
    g = np.load(KNOWN)
    if name in ("lin1", "lin2"):
        return g[name + "_x"], g[name + "_y"], 1
    if name == "quad":
        return g["quad_x"], g["quad_y"], 2
    k = int(name[1:].replace("lin", ""))                     # "u3", "u8": quad_fit; "u3lin", "u8lin": linear_fit on the same data
    rng = np.random.default_rng(k)
    x = rng.random((500, k))
    y = np.stack([np.sin(x.sum(axis=1)), 1.0 + x[:, 0] * x[:, -1] + 0.05 * rng.standard_normal(500)], axis=1)
    return x, y, 1 if name.endswith("lin") else 2


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["lin1", "lin2", "quad", "u3", "u8", "u3lin", "u8lin"])
def test_fits_against_the_reference(ctx, torch, name, kind):
    from corrla_rs_amd import callers
    x, y, degree = _fit_case(name)
    fit = callers.quad_fit if degree == 2 else callers.linear_fit
    c_ref = (R.quad_fit if degree == 2 else R.linear_fit)(x, y)
    v = R.build_full_vandermonde(x, degree)
    full_rank = np.linalg.matrix_rank(v) == v.shape[1]
    assert full_rank == (name != "quad")
    for normalize in (True, False):
        # the yardstick: the same host solve on numpy's own Gram against the reference route -- nothing from the device
        c_cpu = host_fit(x, y, degree, normalize)
        tol_pred = max(10.0 * rel(v @ c_cpu, v @ c_ref), 1e-13)
        tol_coef = max(10.0 * rel(c_cpu, c_ref), 1e-13)
        c = _np(fit(_give(torch, x, kind), _give(torch, y, kind), normalize=normalize, ctx=ctx))
        assert c.shape == c_ref.shape
        print(f"{name} normalize={normalize}: predictions {rel(v @ c, v @ c_ref):.3e} (tol {tol_pred:.3e})"
              + (f", coefficients {rel(c, c_ref):.3e} (tol {tol_coef:.3e})" if full_rank else ""))
        assert rel(v @ c, v @ c_ref) <= tol_pred
        if full_rank:                                        # where V is rank-deficient the coefficients are not determined
            assert rel(c, c_ref) <= tol_coef
        # quad_eval / poly_eval at the training points is the same surface
        assert_eval_within_bound(_np(ctx.poly_eval(_give(torch, x, kind), c, degree)), None, x, c, degree, f"{name} at the training points")


@pytest.mark.parametrize("name", ["lin1", "lin2"])
def test_jac_from_lin_on_the_reference_cases(ctx, name):
    from corrla_rs_amd import callers
    g = np.load(KNOWN)
    jac = callers.jac_from_lin(g[name + "_x"], g[name + "_y"], ctx=ctx)
    assert jac.shape == g[name + "_jac"].shape
    assert np.max(np.abs(jac - g[name + "_jac"])) <= float(g["lin_tol"])      # the reference's own 1e-8


@pytest.mark.parametrize("k", [3, 8])
def test_shifted_data_meets_the_unshifted_tolerance(ctx, k):
    """x in [10, 11]: with the default normalisation the fitted surface is the one of the unshifted problem to the
    unshifted tolerance (the polynomials of a degree are the same space after a shift); without it the normal equations
    lose the digits the issue measured (4e-10), which is why normalize=True is the default."""
    from corrla_rs_amd import callers
    x, y, _ = _fit_case(f"u{k}")
    v = R.build_vandermonde(x)
    want = v @ R.quad_fit(x, y)
    tol = max(10.0 * rel(v @ host_fit(x, y, 2, True), want), 1e-13)          # the unshifted tolerance
    xs = x + 10.0
    # the coefficients come back in the coordinates of xs, where the terms of V(xs) c are a hundred times their sum: the
    # test's own evaluation is done in extended precision so that it adds nothing to what it measures
    vs = R.build_vandermonde(xs.astype(np.longdouble))
    got = (vs @ callers.quad_fit(xs, y, ctx=ctx).astype(np.longdouble)).astype(np.float64)
    raw = (vs @ callers.quad_fit(xs, y, normalize=False, ctx=ctx).astype(np.longdouble)).astype(np.float64)
    print(f"k={k}: shifted, normalised {rel(got, want):.3e} (tol {tol:.3e}); shifted, raw {rel(raw, want):.3e}")
    assert rel(got, want) <= tol


# ---- 6. analytic gradient ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 8])
def test_jac_from_quad_is_the_analytic_gradient(ctx, k):
    from corrla_rs_amd import callers
    x, y, _ = _fit_case(f"u{k}")
    c_ref = R.quad_fit(x, y[:, 1:2])
    x0 = x[:97]
    jac = callers.jac_from_quad(x0, c_ref, ctx=ctx)
    assert jac.shape == x0.shape
    # the reference's forward difference: (y(x + eps) - y(x)) / eps carries the rounding of the two values
    fd = R.jac_from_quad(x0, c_ref)
    ymax = float(np.max(np.abs(R.quad_eval(x0, c_ref))))
    bound = 4 * 2.0 ** -52 * ymax / 1.0e-10
    print(f"k={k}: analytic vs forward difference {float(np.max(np.abs(jac - fd))):.3e} (bound {bound:.3e})")
    assert np.max(np.abs(jac - fd)) <= bound
    # ... and against the analytic gradient of the same coefficients in extended precision, to the bound of the evaluation
    assert_eval_within_bound(callers.quad_eval(x0, c_ref, ctx=ctx), jac, x0, c_ref, 2, f"jac_from_quad k={k}")


# ---- 7. device residency -----------------------------------------------------------------------------------------------------
def test_tensors_in_tensors_out_and_routes(ctx, torch):
    from corrla_rs_amd import callers
    x = torch.rand((200, 4), dtype=torch.float64, device="cuda")
    y = torch.rand((200, 2), dtype=torch.float64, device="cuda")
    g, means, scales = ctx.polyfit_gram(x, y)
    for t in (g, means, scales):
        assert torch.is_tensor(t) and t.device == x.device and t.dtype == torch.float64
    assert ctx.last_polyfit_route() == "inplace"
    c = callers.quad_fit(x, y, ctx=ctx)
    assert torch.is_tensor(c) and c.device == x.device and c.shape == (15, 2)
    v, jac = ctx.poly_eval(x, c, jac=True)
    assert torch.is_tensor(v) and v.device == x.device and jac.device == x.device and jac.shape == (2, 200, 4)
    assert ctx.last_polyfit_route() == "inplace"
    assert torch.is_tensor(callers.quad_eval(x, c, ctx=ctx)) and torch.is_tensor(callers.jac_from_quad(x, c[:, :1], ctx=ctx))
    assert torch.is_tensor(callers.jac_from_lin(x, y, ctx=ctx))
    flat = torch.rand(200 * 4 + 1, dtype=torch.float64, device="cuda")
    xo = flat[1:].view(200, 4)                               # the base one element off a 16-byte boundary
    g2, _, _ = ctx.polyfit_gram(xo, y)
    assert ctx.last_polyfit_route() == "inplace_checked"
    ctx.poly_eval(xo, c)
    assert ctx.last_polyfit_route() == "inplace_checked"
    x32 = x.float()
    g32, m32, _ = ctx.polyfit_gram(x32, y)                   # y follows x: float32 in, float64 Gram out
    assert g32.dtype == torch.float64 and m32.dtype == torch.float64 and ctx.poly_eval(x32, c).dtype == torch.float32
    # the same values through the checked route: the same bits
    ga, _, _ = ctx.polyfit_gram(xo.contiguous(), y)
    assert torch.equal(ga, g2)
