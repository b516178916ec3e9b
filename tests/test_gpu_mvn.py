"""Multivariate normal rows and sandwich variances on the GPU: Context.mvn_sample / sandwich_diag and the callers over them
(corrla_mvn_sample_*, corrla_sandwich_diag_*, csrc/mvn_kernels.hpp).  Run with -m gpu on an MI355X; -s prints the measured
share of every bound.

The z of every expected value is taken from Context.fill_normal on the same device (its own parity: tests/test_gpu_parity.py),
so what is tested here is the fused generation's counters and the products, never a second implementation of Box-Muller.
Shapes come from tests/test_mvn_plan.py, which pins on the CPU the plan each of them gets: widths around the MFMA step and
the column pass, row counts around the row tile BM, the largest fused r and the first staged one, both tiles for the sandwich.

Bounds.  u = 2^-24 (f32) / 2^-53 (f64); references in float64 (f32 cases) or numpy's extended precision (f64 cases).
  identity   F = I, mu = 0: products by 1 and sums with exact zeros are exact -- bitwise fill_normal.
  general    |x^ - x|_ic <= (r + 2) u (sum_k |z_ik| |F_ck| + |mu_c|): an r-term dot product in any order, plus the final sum.
  sandwich   |v^ - v|_i <= (2 d + 2) u sum_ab |j_ia| |C_ab| |j_ib|: d terms inside, one product, d terms outside.
No factor in them is fitted to the device."""
import numpy as np
import pytest

from tests.test_mvn_plan import BM, FIRSTS, IDENTITY_D, MAX_FUSED_R, SANDWICH_D, n_values

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
KINDS = ("host", "dev")
SEED = 20241008


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


def _wide(dtype):
    return np.float64 if dtype == np.float32 else np.longdouble


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _z(ctx, torch, n, r, dtype, first, seed=SEED):
    """rows [first, first + n) of the stream of width r, from the library's own generator"""
    t = torch.empty((n, r), dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
    ctx.fill_normal(t, seed, row0=first, global_cols=r)
    ctx._lib.corrla_ctx_synchronize(ctx._h)
    return t.cpu().numpy()


def _arg(torch, a, kind):
    return torch.tensor(a, device="cuda") if kind == "dev" and a is not None else a


def _bits(a):
    a = np.ascontiguousarray(_np(a))
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- the stream ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", IDENTITY_D)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_factor_is_fill_normal_bitwise(ctx, torch, dtype, kind, d):
    bm = BM(d, np.dtype(dtype).itemsize)
    eye = _arg(torch, np.eye(d, dtype=dtype), kind)
    for n in n_values(bm):
        for first in FIRSTS:
            x = ctx.mvn_sample(n, eye, seed=SEED, first=first)
            assert ctx.last_mvn_route() == "fused"
            assert (kind == "dev") == hasattr(x, "cpu") and tuple(x.shape) == (n, d)
            assert np.array_equal(_bits(x), _bits(_z(ctx, torch, n, d, dtype, first))), (n, first)


def _general_case(ctx, torch, dtype, kind, n, d, r, first, lower=False, with_mean=True, route="fused", out_layout=None, rng=None):
    rng = rng or np.random.default_rng(d * 1000 + r)
    f = rng.standard_normal((d, r)).astype(dtype)
    if lower:
        f = np.tril(f)
    mu = rng.standard_normal(d).astype(dtype) if with_mean else None
    out = None
    if out_layout == "odd":  # row stride d + 1, base one element past an aligned address: the element-store path
        if kind == "dev":
            buf = torch.full((n * (d + 1) + 1,), float("nan"), dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
            out = buf[1:].as_strided((n, d), (d + 1, 1))
        else:
            buf = np.full(n * (d + 1) + 1, np.nan, dtype=dtype)
            out = np.lib.stride_tricks.as_strided(buf[1:], (n, d), ((d + 1) * buf.itemsize, buf.itemsize))
    x = ctx.mvn_sample(n, _arg(torch, f, kind), _arg(torch, mu, kind), seed=SEED, first=first, lower=lower, out=out)
    assert ctx.last_mvn_route() == route
    if out is not None:
        gaps = _np(buf)[1:].reshape(n, d + 1)[:, d] if n * (d + 1) + 1 > 1 else np.empty(0)
        assert np.all(np.isnan(gaps)) and np.isnan(_np(buf)[0]), "an element outside the n x d window was written"
    w = _wide(dtype)
    z = _z(ctx, torch, n, r, dtype, first).astype(w)
    want = z @ f.astype(w).T + (0 if mu is None else mu.astype(w))
    bound = (r + 2) * _u(dtype) * (np.abs(z) @ np.abs(f.astype(w)).T + (0 if mu is None else np.abs(mu.astype(w))))
    err = np.abs(_np(x).astype(w) - want)
    share = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
    print(f"mvn {np.dtype(dtype).name} {kind} n={n} d={d} r={r} lower={lower} {route}: {share:.3f} of the bound")
    assert np.all(err <= bound), share
    return x


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_general_factor_dense_lower_and_thin(ctx, torch, dtype, kind):
    esz = np.dtype(dtype).itemsize
    bm = BM(17, esz)
    _general_case(ctx, torch, dtype, kind, 3 * bm + 5, 17, 17, 7)                       # dense, square
    _general_case(ctx, torch, dtype, kind, bm + 1, 17, 3, 2 ** 33 + 3)                  # r < d
    _general_case(ctx, torch, dtype, kind, bm + 1, 131, 131, 0, lower=True)             # triangular, three column passes
    _general_case(ctx, torch, dtype, kind, bm - 1, 130, 5, 0, with_mean=False)          # no mean
    _general_case(ctx, torch, dtype, kind, 3 * bm + 5, 17, 5, 7, out_layout="odd")      # element stores
    _general_case(ctx, torch, dtype, kind, bm + 1, 16, 16, 7, out_layout="odd")


@pytest.mark.parametrize("dtype", DTYPES)
def test_largest_fused_r_and_the_first_staged_one(ctx, torch, dtype):
    esz = np.dtype(dtype).itemsize
    rmax = MAX_FUSED_R[esz]
    bm = BM(rmax, esz)
    assert bm == 64
    _general_case(ctx, torch, dtype, "dev", bm + 1, rmax, rmax, 7, route="fused")
    _general_case(ctx, torch, dtype, "dev", bm + 1, rmax, rmax, 7, lower=True, route="fused")
    _general_case(ctx, torch, dtype, "dev", 64 + 1, rmax + 1, rmax + 1, 7, route="staged")
    _general_case(ctx, torch, dtype, "host", 64 + 1, rmax + 1, rmax + 1, 7, route="staged", out_layout="odd")


# ---- bitwise invariances ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (17, 131, 144, 300))
@pytest.mark.parametrize("dtype", DTYPES)
def test_lower_equals_dense_bitwise(ctx, torch, dtype, d):
    rng = np.random.default_rng(d)
    f = torch.tensor(np.tril(rng.standard_normal((d, d))).astype(dtype), device="cuda")
    mu = torch.tensor(rng.standard_normal(d).astype(dtype), device="cuda")
    n = 3 * 64 + 5
    a = ctx.mvn_sample(n, f, mu, seed=SEED, first=7, lower=True)
    b = ctx.mvn_sample(n, f, mu, seed=SEED, first=7, lower=False)
    assert ctx.last_mvn_route() == ("fused" if d <= MAX_FUSED_R[np.dtype(dtype).itemsize] else "staged")
    assert np.array_equal(_bits(a), _bits(b))
    # the strict upper triangle is never read with lower=True
    g = f.clone()
    g += torch.triu(torch.full_like(g, float("nan")), diagonal=1)
    assert np.array_equal(_bits(ctx.mvn_sample(n, g, mu, seed=SEED, first=7, lower=True)), _bits(a))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_do_not_depend_on_the_call_they_come_from(ctx, torch, dtype, kind):
    rng = np.random.default_rng(5)
    d, r, n = 19, 6, 2 * 101
    f, mu = _arg(torch, rng.standard_normal((d, r)).astype(dtype), kind), _arg(torch, rng.standard_normal(d).astype(dtype), kind)
    whole = _bits(ctx.mvn_sample(n, f, mu, seed=3, first=2 ** 33 + 3))
    again = _bits(ctx.mvn_sample(n, f, mu, seed=3, first=2 ** 33 + 3))
    lo = _bits(ctx.mvn_sample(n // 2, f, mu, seed=3, first=2 ** 33 + 3))
    hi = _bits(ctx.mvn_sample(n // 2, f, mu, seed=3, first=2 ** 33 + 3 + n // 2))
    assert np.array_equal(whole, again)
    assert np.array_equal(whole[: n // 2], lo) and np.array_equal(whole[n // 2:], hi)
    assert not np.array_equal(whole, _bits(ctx.mvn_sample(n, f, mu, seed=4, first=2 ** 33 + 3)))


def test_empty_call_and_rejections(ctx, torch):
    f = np.eye(3)
    x = ctx.mvn_sample(0, f)
    assert x.shape == (0, 3) and ctx.last_mvn_route() == "empty"
    for bad in (dict(n=4, factor=np.ones((3, 4))), dict(n=-1, factor=f), dict(n=4, factor=f, first=-1),
                dict(n=2, factor=f, first=2 ** 62), dict(n=4, factor=np.ones((3, 2)), lower=True),
                dict(n=4, factor=torch.ones((3, 3), dtype=torch.bfloat16, device="cuda")),
                dict(n=4, factor=torch.eye(3).to_sparse_csr()), dict(n=4, factor=f, mean=np.zeros(3, dtype=np.float32)),
                dict(n=4, factor=np.ones((3, 0)))):
        with pytest.raises(ValueError):
            ctx.mvn_sample(**bad)
    with pytest.raises(ValueError, match="512"):
        ctx.sandwich_diag(np.ones((4, 513)), np.eye(513))


# ---- sandwich_diag ------------------------------------------------------------------------------------------------------
def _sandwich_check(ctx, dtype, j_arg, c_arg, j, c, tag):
    v = ctx.sandwich_diag(j_arg, c_arg)
    v2 = ctx.sandwich_diag(j_arg, c_arg)
    assert tuple(v.shape) == (j.shape[0],) and np.array_equal(_bits(v), _bits(v2))
    w = np.longdouble
    jw, cw = j.astype(w), c.astype(w)
    want = np.einsum("ia,ab,ib->i", jw, cw, jw)
    bound = (2 * j.shape[1] + 2) * _u(dtype) * np.einsum("ia,ab,ib->i", np.abs(jw), np.abs(cw), np.abs(jw))
    err = np.abs(_np(v).astype(w) - want)
    share = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
    print(f"sandwich {np.dtype(dtype).name} {tag}: {share:.3f} of the bound")
    assert np.all(err <= bound), share


@pytest.mark.parametrize("d", SANDWICH_D)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_sandwich_diag(ctx, torch, dtype, kind, d):
    rng = np.random.default_rng(d)
    bm = BM(d, np.dtype(dtype).itemsize)
    c = rng.standard_normal((d, d)).astype(dtype)     # not symmetric: it must not be symmetrised
    for m in (1, bm + 1):
        j = rng.standard_normal((m, d)).astype(dtype)
        _sandwich_check(ctx, dtype, _arg(torch, j, kind), _arg(torch, c, kind), j, c, f"{kind} m={m} d={d}")
    if d > 1:  # an upper-triangular cov and its symmetric completion give different values: cov is used as given
        j = rng.standard_normal((5, d)).astype(dtype)
        a = _np(ctx.sandwich_diag(_arg(torch, j, kind), _arg(torch, np.triu(c), kind)))
        assert not np.allclose(a, _np(ctx.sandwich_diag(_arg(torch, j, kind), _arg(torch, np.triu(c) + np.triu(c, 1).T, kind))))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_sandwich_diag_on_a_gradient_block_of_poly_eval(ctx, torch, dtype, kind):
    rng = np.random.default_rng(11)
    m, k, r = 65, 5, 2
    x = rng.standard_normal((m, k)).astype(dtype)
    coeffs = rng.standard_normal((k + k * (k + 1) // 2 + 1, r))
    _vals, grads = ctx.poly_eval(_arg(torch, x, kind), coeffs, 2, jac=True)
    assert tuple(grads.shape) == (r, m, k)
    a = rng.standard_normal((k, 3 * k)).astype(dtype)
    c = (a @ a.T / (3 * k)).astype(dtype)
    block = grads[1]
    _sandwich_check(ctx, dtype, block, _arg(torch, c, kind), _np(block), c, f"{kind} poly_eval block")
    # ... and on a view with a padded row stride
    wide = np.zeros((m, k + 3), dtype=dtype)
    wide[:, :k] = _np(block)
    view = _arg(torch, wide, kind)[:, :k]
    _sandwich_check(ctx, dtype, view, _arg(torch, c, kind), _np(block), c, f"{kind} strided view")


# ---- callers ------------------------------------------------------------------------------------------------------------
def test_sample_mv_normal_on_a_cuda_covariance(ctx, torch):
    from corrla_rs_amd import sample_mv_normal
    rng = np.random.default_rng(2)
    a = rng.standard_normal((4, 4))
    c = a @ a.T + 0.5 * np.eye(4)
    mu = np.array([1.0, -2.0, 0.5, 3.0])
    n = 200_000
    x = sample_mv_normal(torch.tensor(c, device="cuda"), n, mean=mu, seed=12345, ctx=ctx)
    assert hasattr(x, "cpu") and tuple(x.shape) == (n, 4) and x.dtype == torch.float64 and ctx.last_mvn_route() == "fused"
    x = x.cpu().numpy()
    assert np.all(np.abs(x.mean(0) - mu) <= 6.0 * np.sqrt(np.diag(c) / n))
    s = np.cov(x, rowvar=False)
    band = 6.0 * np.sqrt((np.outer(np.diag(c), np.diag(c)) + c * c) / n)
    print("sample covariance, share of the 6 sigma band:", float(np.max(np.abs(s - c) / band)))
    assert np.all(np.abs(s - c) <= band)
    # a singular covariance: rank 2 in 4 dimensions, thin factor
    b = rng.standard_normal((4, 2))
    xs = sample_mv_normal(b @ b.T, 1000, seed=1, ctx=ctx)
    assert isinstance(xs, np.ndarray) and np.linalg.matrix_rank(xs - xs.mean(0), tol=1e-8) == 2


def test_sandwich_prop_diag_is_the_diagonal_of_the_full_product(ctx, torch):
    from corrla_rs_amd import sandwich_prop
    rng = np.random.default_rng(3)
    d, m = 9, 70
    a = rng.standard_normal((d, d))
    c, j = a @ a.T, rng.standard_normal((m, d))
    full = sandwich_prop(c, j)
    assert full.shape == (m, m)
    for jj in (j, torch.tensor(j, device="cuda")):
        v = _np(sandwich_prop(c, jj, diag=True, ctx=ctx))
        bound = (2 * d + 2) * 2.0 ** -53 * np.einsum("ia,ab,ib->i", np.abs(j), np.abs(c), np.abs(j))
        assert np.all(np.abs(v - np.diag(full)) <= 2 * bound)   # both sides carry the rounding of a d x d contraction


@pytest.mark.parametrize("dtype", DTYPES)
def test_pca_model_sample_is_the_back_projection_of_the_stream(ctx, torch, dtype):
    import corrla_rs_amd as cr
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((300, 6)) @ rng.standard_normal((6, 40)) + rng.standard_normal(40)).astype(dtype)
    model = cr.PcaRsvd(torch.tensor(x, device="cuda"), 5, seed=1, ctx=ctx)
    got = model.sample(77, seed=9, first=11)
    z = torch.empty((77, 5), dtype=model.components_.dtype, device="cuda")
    ctx.fill_normal(z, 9, row0=11, global_cols=5)
    ctx._lib.corrla_ctx_synchronize(ctx._h)
    sig = (model.pca_s.reshape(1, -1) / float(np.sqrt(model.n_samples - 1.0))).to(z.dtype)
    want = ctx.pca_inverse_transform(z * sig, model.means, model.components_, model.scales_)
    assert tuple(got.shape) == (77, 40) and np.array_equal(_bits(got), _bits(want))
