"""The host side of the multivariate normal sampler, on the CPU: the covariance factor (callers.mvn_factor), the stream the
device kernels draw from restated in numpy, and PcaRsvd.sample on a host-fitted model.

The stream is restated from tests/dirichlet_reference.py (philox4x32_10, uniform_pair, box_muller; imported, not edited):
z_i[j] is the Box-Muller value of the Philox4x32-10 block with counter ((first + i) r + j, 0, 0) and key seed -- what
include/corrla_rsvd.h defines and Context.fill_normal writes.  Seeds are fixed, so every test here is deterministic."""
import numpy as np
import pytest

from corrla_rs_amd import PcaRsvd, mvn_factor
from corrla_rs_amd.api import normal_stream_host
from tests import dirichlet_reference as R

U = 2.0 ** -52


def stream(seed, first, n, r):
    t = (np.uint64(first) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(r) + np.arange(r, dtype=np.uint64)[None, :]
    z = np.zeros_like(t)
    u1, u2 = R.uniform_pair(*R.philox4x32_10(t & R.M32, t >> np.uint64(32), z, z, seed & 0xFFFFFFFF, seed >> 32))
    return R.box_muller(u1, u2)


def _factor_bound(c):
    d = c.shape[0]
    return (d + 2) * U * d * np.max(np.abs(c))


def test_factor_accuracy():
    rng = np.random.default_rng(1)
    a = rng.standard_normal((7, 7))
    spd = a @ a.T + 0.1 * np.eye(7)
    spd *= np.outer(10.0 ** np.arange(-3, 4), 10.0 ** np.arange(-3, 4))  # badly scaled: the equilibration matters
    f, lower = mvn_factor(spd)
    assert lower and f.shape == (7, 7) and np.array_equal(f, np.tril(f))
    assert np.all(np.abs(f @ f.T - spd) <= _factor_bound(spd))

    b = rng.standard_normal((6, 3))
    psd = b @ b.T                                    # rank 3 in 6 dimensions
    f, lower = mvn_factor(psd)
    assert not lower and f.shape == (6, 3)
    assert np.all(np.abs(f @ f.T - psd) <= _factor_bound(psd))

    indefinite = np.diag([2.0, 1.0, -0.5])
    with pytest.raises(ValueError, match="positive semi-definite"):
        mvn_factor(indefinite)
    asym = spd.copy()
    asym[5, 6] *= 1.0 + 1e-10                        # far beyond 8 * 2^-52 * max|C|, which is what the rule is relative to
    with pytest.raises(ValueError, match="symmetric"):
        mvn_factor(asym)
    with pytest.raises(ValueError, match="square"):
        mvn_factor(np.ones((2, 3)))
    f, lower = mvn_factor(np.zeros((3, 3)))          # the degenerate law: one column of zeros
    assert f.shape == (3, 1) and not lower and not f.any()


def test_stream_moments():
    rng = np.random.default_rng(2)
    a = rng.standard_normal((4, 4))
    c = a @ a.T + 0.5 * np.eye(4)
    mu = np.array([1.0, -2.0, 0.5, 3.0])
    n, seed = 200_000, 20241008
    f, lower = mvn_factor(c)
    assert lower
    z = stream(seed, 5, n, 4)
    x = mu + z @ f.T
    assert np.all(np.abs(x.mean(0) - mu) <= 6.0 * np.sqrt(np.diag(c) / n))
    s = np.cov(x, rowvar=False)
    band = 6.0 * np.sqrt((np.outer(np.diag(c), np.diag(c)) + c * c) / n)
    assert np.all(np.abs(s - c) <= band), np.max(np.abs(s - c) / band)
    # the package's own host restatement is this stream: the integer part exactly, the transcendental part to a few ulp
    mine = normal_stream_host(seed, 5, 1000, 4)
    assert np.all(np.abs(mine - z[:1000]) <= 8 * U * np.maximum(np.abs(z[:1000]), 1.0))
    # slices of the stream do not depend on the call they come from
    assert np.array_equal(normal_stream_host(seed, 5 + 300, 50, 4), mine[300:350])
    f32 = normal_stream_host(seed, 5, 1000, 4, np.float32)
    assert f32.dtype == np.float32 and abs(float(f32.mean())) < 0.1 and abs(float(f32.std()) - 1.0) < 0.1


def _host_model(rng, n_samples, n_dim, k, dtype, scales):
    """a host-fitted model without a device: the fields the fit leaves behind"""
    m = PcaRsvd.__new__(PcaRsvd)
    q, _ = np.linalg.qr(rng.standard_normal((n_dim, k)))
    m.pca_rank, m._ctx, m.n_samples = k, None, n_samples
    m.components_ = np.ascontiguousarray(q.T).astype(dtype)
    m.pca_s = np.sort(rng.uniform(1.0, 30.0, (k, 1)))[::-1].astype(dtype)
    m.means = rng.standard_normal((1, n_dim)).astype(dtype)
    m.scales_ = rng.uniform(0.5, 2.0, (1, n_dim)).astype(dtype) if scales else None
    return m


@pytest.mark.parametrize("scales", [False, True])
def test_model_sampling_on_a_host_fitted_model(scales):
    rng = np.random.default_rng(3)
    n_samples, n_dim, k, n = 500, 37, 5, 300
    m = _host_model(rng, n_samples, n_dim, k, np.float64, scales)
    x = m.sample(n, seed=77, first=13)
    assert isinstance(x, np.ndarray) and x.shape == (n, n_dim) and x.dtype == np.float64
    w = np.longdouble
    z = stream(77, 13, n, k).astype(w)
    sig = m.pca_s.reshape(1, -1).astype(w) / np.sqrt(w(n_samples - 1.0))
    sd = np.ones((1, n_dim), dtype=w) if m.scales_ is None else m.scales_.astype(w)
    want = m.means.astype(w) + sd * ((z * sig) @ m.components_.astype(w))
    # z to 8 ulp (two library functions and their product), its scaling, a k-term product, the scale and the final sum
    mag = np.abs(m.means).astype(w) + sd * ((np.abs(z) * sig) @ np.abs(m.components_).astype(w))
    assert np.all(np.abs(x - want) <= (k + 12) * 2.0 ** -53 * mag)
    assert np.array_equal(m.sample(n, seed=77, first=13), x)
    assert np.array_equal(m.sample(100, seed=77, first=13 + 100), x[100:200])
    # the law: the covariance of the draws is V^T diag(s^2 / (n_samples - 1)) V in the scaled coordinates
    big = m.sample(100_000, seed=5)
    var = (np.asarray(m.pca_s).ravel() ** 2) / (n_samples - 1.0)
    t = ((big - m.means) / (1.0 if m.scales_ is None else m.scales_)) @ m.components_.T
    assert np.all(np.abs(t.var(0, ddof=1) - var) <= 6.0 * var * np.sqrt(2.0 / 100_000))
    with pytest.raises(ValueError):
        m.sample(-1)
