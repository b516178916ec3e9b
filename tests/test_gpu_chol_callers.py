"""The callers of the device Cholesky on the GPU: mvn_factor(device=True), sample_mv_normal(factor="device") and
RbfInterp(solver="chol") (corrla_rs_amd/callers.py over Context.cholesky / Context.solve(assume="pos")).  Run with -m gpu on an
MI355X.  No tolerance is tuned (tests/chol_reference.py): with u = 2^-53 and gamma_k = k u / (1 - k u),
  covariance factor  |C - F F^T| <= gamma_(d+8) |F||F^T| componentwise: gamma_(d+1) is Higham's Thm 10.3 for the equilibrated
                     matrix, and the 7 beyond it cover the roundings of the equilibration and the rescaling -- the outer
                     product and the quotient on C, and one per entry of F on either side of the product
  RBF fit            the coefficients satisfy the solve bound of tests/test_gpu_chol.py against Context.rbf_system's matrix, and
                     predict at the supports reproduces y within that same bound
The defaults are pinned too: mvn_factor(device=False) is bitwise the host formula restated here."""
import numpy as np
import pytest

from tests import chol_reference as R

pytestmark = pytest.mark.gpu


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


def host_factor(cov):
    """mvn_factor as it stood before the device route, restated: the fixture of the default's bits"""
    c = np.asarray(cov, dtype=np.float64)
    d = c.shape[0]
    big = float(np.max(np.abs(c)))
    assert float(np.max(np.abs(c - c.T))) <= 8.0 * 2.0 ** -52 * big
    c = 0.5 * (c + c.T)
    sd = np.sqrt(np.diag(c).clip(min=0.0))
    sd = np.where(sd > 0.0, sd, 1.0)
    try:
        return sd[:, None] * np.linalg.cholesky(c / np.outer(sd, sd)), True
    except np.linalg.LinAlgError:
        pass
    w, v = np.linalg.eigh(c)
    cut = d * 2.0 ** -52 * max(float(w[-1]), 0.0)
    assert float(w[0]) >= -cut
    keep = w > cut
    return v[:, keep] * np.sqrt(w[keep])[None, :], False


@pytest.mark.parametrize("d", [5, 193, 704])
@pytest.mark.parametrize("kind", R.KINDS)
def test_device_covariance_factor_bound(torch, ctx, kind, d):
    from corrla_rs_amd import callers
    cov = R.spd(kind, d)
    given = torch.tensor(cov, device="cuda") if d != 193 else cov  # a CUDA tensor, and at 193 a numpy array
    f, lower = callers.mvn_factor(given, device=True, ctx=ctx)
    assert torch.is_tensor(f) and f.is_cuda and f.dtype == torch.float64 and tuple(f.shape) == (d, d) and lower is True
    assert ctx.last_chol_route == ("small" if d <= 128 else "blocked") and ctx.last_chol_info["info"] == 0
    R.check_factorisation(cov, f.cpu().numpy(), k=d + 8)


@pytest.mark.parametrize("kind,d", [("gram", 5), ("lehmer", 193), ("scaled", 64)])
def test_host_covariance_factor_keeps_its_bits(ctx, kind, d):
    from corrla_rs_amd import callers
    cov = R.spd(kind, d)
    want, want_lower = host_factor(cov)
    for got, lower in (callers.mvn_factor(cov), callers.mvn_factor(cov, device=False), callers.mvn_factor(cov, device=False, ctx=ctx)):
        assert isinstance(got, np.ndarray) and lower is want_lower and np.array_equal(got, want)


def test_rank_deficient_covariance_takes_the_eigendecomposition(torch, ctx):
    """A Gram of 3 samples in d = 8 whose first two features coincide with variance 4: the equilibrated matrix starts with
    [[1, 1], [1, 1]] exactly, so the pivot of column 2 is exactly zero on the host and on the device alike."""
    from corrla_rs_amd import callers
    x = np.random.default_rng(5).standard_normal((3, 8))
    x[:, 0] = x[:, 1] = [2.0, 0.0, 0.0]
    cov = x.T @ x
    cov = np.tril(cov) + np.tril(cov, -1).T
    want, want_lower = callers.mvn_factor(cov)
    assert want_lower is False and want.shape[0] == 8 and want.shape[1] <= 3
    for given in (cov, torch.tensor(cov, device="cuda")):
        f, lower = callers.mvn_factor(given, device=True, ctx=ctx)
        assert ctx.last_chol_info["info"] == 2  # the factorisation was tried and reported its column
        assert lower is False and f.is_cuda and np.array_equal(f.cpu().numpy(), want)
    # an indefinite matrix is still a ValueError on this route
    with pytest.raises(ValueError, match="positive semi-definite"):
        callers.mvn_factor(np.diag([1.0, -1.0, 2.0]), device=True, ctx=ctx)
    with pytest.raises(ValueError, match="symmetric"):
        callers.mvn_factor(np.array([[1.0, 0.5], [0.25, 1.0]]), device=True, ctx=ctx)


def test_sample_mv_normal_with_the_device_factor(torch, ctx):
    from corrla_rs_amd import callers
    d, n = 193, 37
    cov, mean = R.spd("gram", d), np.linspace(-1.0, 1.0, d)
    f, lower = callers.mvn_factor(cov, device=True, ctx=ctx)
    want = ctx.mvn_sample(n, f, torch.tensor(mean, device="cuda"), seed=11, lower=True).cpu().numpy()
    default = callers.sample_mv_normal(cov, n, mean=mean, seed=11, ctx=ctx)
    got = callers.sample_mv_normal(cov, n, mean=mean, seed=11, ctx=ctx, factor="device")
    assert isinstance(got, np.ndarray) and got.shape == default.shape == (n, d) and got.dtype == default.dtype == np.float64
    assert np.array_equal(got, want)
    got_t = callers.sample_mv_normal(torch.tensor(cov, device="cuda"), n, mean=mean, seed=11, ctx=ctx, factor="device")
    assert got_t.is_cuda and np.array_equal(got_t.cpu().numpy(), want)
    assert np.array_equal(callers.sample_mv_normal(cov, n, mean=mean, seed=11, ctx=ctx, factor="host"), default)
    with pytest.raises(ValueError, match="factor"):
        callers.sample_mv_normal(cov, n, factor="gpu", ctx=ctx)


def _rbf_case():
    """150 supports on a jittered 15 x 10 grid of the unit square (spacing ~0.07 and ~0.1, jitter 0.01) and a Gaussian kernel
    exp(-(12 r)^2): neighbours correlate at about 0.5, the kernel matrix is comfortably positive definite"""
    rng = np.random.default_rng(150)
    gx, gy = np.meshgrid(np.linspace(0.0, 1.0, 15), np.linspace(0.0, 1.0, 10), indexing="ij")
    x = np.stack([gx.ravel(), gy.ravel()], axis=1) + 0.01 * rng.standard_normal((150, 2))
    y = np.stack([np.sin(3.0 * x[:, 0]) * np.cos(2.0 * x[:, 1]), x[:, 0] ** 2 - x[:, 1]], axis=1)
    return x, y, 12.0


def test_rbf_interp_with_the_cholesky_solver(torch, ctx):
    from corrla_rs_amd import callers
    x, y, eps = _rbf_case()
    r = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
    assert R.cholesky(np.exp(-((r * eps) ** 2)))[1] == 0  # the numpy restatement factors the system
    system = ctx.rbf_system(x, 4, eps, poly_degree=None)
    assert system.shape == (150, 150)
    system = np.tril(system) + np.tril(system, -1).T  # what the factorisation reads
    l = ctx.cholesky(system)
    for given_x, given_y in ((x, y), (torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda"))):
        m = callers.RbfInterp(4, eps, 2, None, solver="chol", ctx=ctx)
        m.fit(given_x, given_y)
        on_gpu = torch.is_tensor(given_x)
        assert (torch.is_tensor(m.coeffs) and m.coeffs.is_cuda) == on_gpu
        coeffs = m.coeffs.cpu().numpy() if on_gpu else m.coeffs
        assert coeffs.shape == (150, 2) and ctx.last_chol_route == "blocked" and ctx.last_chol_info["info"] == 0
        R.check_solve(system, y, coeffs, l)
        pred = m.predict(given_x)
        pred = pred.cpu().numpy() if on_gpu else pred
        bound = R.gamma(3 * 150 + 1) * (np.abs(l) @ (np.abs(l).T @ np.abs(coeffs))) + R.gamma(150 + 1) * (np.abs(system) @ np.abs(coeffs) + np.abs(y))
        print("predict at the supports: max |pred - y| / bound =", float(np.max(np.abs(pred - y) / bound)))
        assert np.all(np.abs(pred - y) <= bound)
    # a single right-hand side given as a vector
    m = callers.RbfInterp(4, eps, 2, None, solver="chol", ctx=ctx)
    m.fit(x, y[:, 0])
    assert m.coeffs.shape == (150, 1)


def test_rbf_interp_cholesky_solver_rejections(torch, ctx):
    from corrla_rs_amd import callers
    from corrla_rs_amd._lib import CorrlaError
    for kernel in (1, 2, 3):
        with pytest.raises(ValueError, match="chol"):
            callers.RbfInterp(kernel, 1.0, 2, None, solver="chol", ctx=ctx)
    for degree in (0, 1, 2):
        with pytest.raises(ValueError, match="chol"):
            callers.RbfInterp(4, 1.0, 2, degree, solver="chol", ctx=ctx)
    with pytest.raises(ValueError, match="solver"):
        callers.RbfInterp(4, 1.0, 2, 1, solver="qr", ctx=ctx)
    # coincident supports: two equal rows and columns, the second pivot is exactly zero
    x = np.array([[0.0, 0.0], [0.0, 0.0], [1.0, 0.5]])
    m = callers.RbfInterp(4, 1.0, 2, None, solver="chol", ctx=ctx)
    with pytest.raises(CorrlaError, match="column 2 "):
        m.fit(x, np.ones(3))
