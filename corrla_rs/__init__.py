"""Drop-in module name of the reference's pyo3 extension (`import corrla_rs as hrl;
hrl.rsvd(A, 4, 8, 10)`, examples/benchmark_rsvd.py:13,101; `from corrla_rs import PyDMDc`, examples/benchmark_dmd.py:12).
The RSVD hot path and its callers are provided -- rpca (PCA), PyDMDc, PyPodI (with the PyRbfInterp its mode weights
are interpolated by) -- and everything m- or n-sized is forwarded to corrla_rs_amd (HIP, gfx950).  active_ss
(gradient stage on the GPU) is provided too, and so are the samplers cs_dirichlet_sample and cs_mcmc_dirichlet_sample
(lib_math_utils_py.rs:89-168): the Dirichlet draws, the box test and the count run on the device behind
``Context.dirichlet_sample``, the differential-evolution chains on the host.  With them every function and class of the
pyo3 module is provided.  mat_cov_centered, pearson_corr and rsquared_sens (stats_corr.rs) are ADDITIVE: the pyo3
module does not expose them; here they run on the symmetric MFMA kernel behind ``Context.cov``.  linear_fit, quad_fit,
quad_eval, jac_from_lin and jac_from_quad (stats_corr.rs:146-249) are additive in the same way, on the fused
normal-equation and evaluation kernels behind ``Context.polyfit_gram`` / ``poly_eval``.  sample_mv_normal and
sandwich_prop (stats_corr.rs:46-68) are additive too, on the fused kernels behind ``Context.mvn_sample`` /
``sandwich_diag`` (samples have covariance cov, not the reference's cov^2).  KdeRv and build_kde
(univariate_rv.rs:384-497: the Gaussian kernel density estimate, its likelihood and the cross-validated bandwidth) are
additive too, on the fused pairwise-sum kernels behind ``Context.kde_eval`` / ``kde_nll``; the other univariate random
variables of that module (NormalRv, BetaRv, ExponentialRv, mlefit) stay outside this build's scope.  rbf_fit is additive
as well: the coefficients of an RBF interpolant by an LU solve on the device (``Context.rbf_fit``), where PyRbfInterp
keeps the reference's pseudo-inverse.  cholesky is additive too: the Cholesky factor of a symmetric positive definite matrix on
the device (``Context.cholesky``; ``Context.solve(a, b, assume="pos")`` solves with it), which mvn_factor(device=True),
sample_mv_normal(factor="device") and corrla_rs_amd.RbfInterp(solver="chol") take on request; every default is unchanged."""
import numpy as _np

from corrla_rs_amd.api import PcaRsvd, power_iter, random_svd, rpca, rsvd  # noqa: F401
from corrla_rs_amd.callers import DMDc as _DMDc
from corrla_rs_amd.callers import PodI as _PodI
from corrla_rs_amd.callers import RbfInterp as _RbfInterp
from corrla_rs_amd.callers import mat_cov_centered, pearson_corr, rsquared_sens  # noqa: F401
from corrla_rs_amd.callers import jac_from_lin, jac_from_quad, linear_fit, quad_eval, quad_fit  # noqa: F401
from corrla_rs_amd.callers import KdeRv, build_kde  # noqa: F401
from corrla_rs_amd.callers import mvn_factor, sample_mv_normal, sandwich_prop  # noqa: F401
from corrla_rs_amd.callers import cholesky, rbf_fit  # noqa: F401
from corrla_rs_amd.callers import constr_dirichlet_sample as _constr_dirichlet_sample
from corrla_rs_amd.callers import cs_mcmc_dirichlet_sample as _cs_mcmc_dirichlet_sample

__all__ = ["rsvd", "rpca", "random_svd", "power_iter", "PcaRsvd", "PyDMDc", "PyPodI", "PyRbfInterp", "active_ss",
           "mat_cov_centered", "pearson_corr", "rsquared_sens", "linear_fit", "quad_fit", "quad_eval", "jac_from_lin",
           "jac_from_quad", "KdeRv", "build_kde", "cs_dirichlet_sample", "cs_mcmc_dirichlet_sample", "mvn_factor",
           "sample_mv_normal", "sandwich_prop", "rbf_fit", "cholesky"]


def active_ss(a_mat, y, order, n_nbr, n_comps):
    """pyo3 ``active_ss(a_mat, y, order, n_nbr, n_comps)`` (src/lib_math_utils_py.rs:57-86): local polynomial gradients
    (GPU), eigendecomposition of G G^T / N (``ActiveSsRsvd::fit``); returns (components, singular values as a diagonal
    matrix, diagonal sensitivity).  Any number of input parameters and neighbours (above 64 / 512 on the wide kernels)."""
    from corrla_rs_amd.callers import ActiveSsRsvd, PolyGradientEstimator
    x = _np.asarray(a_mat, dtype=_np.float64)
    fit = ActiveSsRsvd(PolyGradientEstimator(x, _np.asarray(y, dtype=_np.float64), int(order), int(n_nbr)), int(n_comps)).fit(x)
    return fit.components(), fit.singular_vals(), fit.var_diag_evd_sensi()


def _alphas_1d(np_alphas):
    a = _np.asarray(np_alphas, dtype=_np.float64)
    if a.ndim != 1:
        raise TypeError(f"np_alphas must be a 1-D array, got shape {tuple(a.shape)}")
    return a


def cs_dirichlet_sample(np_bounds, n_samples, max_zshots, chunk_size, c_scale, np_alphas):
    """pyo3 ``cs_dirichlet_sample(np_bounds, n_samples, max_zshots, chunk_size, c_scale, np_alphas)``
    (src/lib_math_utils_py.rs:89-105): n_samples points with sum x = c_scale inside the (d, 2) box, by rejection from
    Dirichlet(np_alphas) (d values, or one for the symmetric case) on the GPU.  Rows that were not found in max_zshots shots of
    chunk_size stay zero, as in the reference, with a RuntimeWarning.  Every call takes a fresh seed, as the reference's
    thread_rng does; ``corrla_rs_amd.callers.constr_dirichlet_sample`` takes one."""
    return _constr_dirichlet_sample(_np.asarray(np_bounds, dtype=_np.float64), int(n_samples), int(max_zshots), int(chunk_size),
                                    float(c_scale), _alphas_1d(np_alphas))


def cs_mcmc_dirichlet_sample(np_bounds, n_samples, n_seed_samples, max_zshots, chunk_size, c_scale, np_alphas, gamma, var_epsilon):
    """pyo3 ``cs_mcmc_dirichlet_sample(np_bounds, n_samples, n_seed_samples, max_zshots, chunk_size, c_scale, np_alphas, gamma,
    var_epsilon)`` (src/lib_math_utils_py.rs:107-168) -> (samples, accept_ratio): n_seed_samples seeds by rejection on the
    GPU, then n_samples steps of differential-evolution chains towards the uniform distribution on the boxed simplex;
    samples is (n_samples * n_seed_samples, d).  The differences from the reference are those of
    ``corrla_rs_amd.callers.DeMcSampler``."""
    return _cs_mcmc_dirichlet_sample(_np.asarray(np_bounds, dtype=_np.float64), int(n_samples), int(n_seed_samples), int(max_zshots),
                                     int(chunk_size), float(c_scale), _alphas_1d(np_alphas), float(gamma), float(var_epsilon))


class PyRbfInterp:
    """pyo3 ``PyRbfInterp(kernel_type, kernel_param, dim, poly_degree)`` / ``fit(x, y)`` / ``predict(x)``
    (src/lib_math_utils_py.rs:178-220)."""

    def __init__(self, kernel_type, kernel_param, dim, poly_degree):
        self.rbfi = _RbfInterp(int(kernel_type), float(kernel_param), int(dim), int(poly_degree))

    def fit(self, x_np, y_np):
        self.rbfi.fit(_np.asarray(x_np, dtype=_np.float64), _np.asarray(y_np, dtype=_np.float64))

    def predict(self, x_np):
        return self.rbfi.predict(_np.asarray(x_np, dtype=_np.float64))


class PyPodI:
    """pyo3 ``PyPodI(x, t, n_modes)`` / ``predict(t)`` (src/lib_math_utils_py.rs:222-250): the randomized SVD and the
    N-sized products on the GPU."""

    def __init__(self, x_np, t_np, n_modes):
        self.pod = _PodI(_np.asarray(x_np, dtype=_np.float64), _np.asarray(t_np, dtype=_np.float64), int(n_modes))

    def predict(self, t_np):
        return self.pod.predict(_np.asarray(t_np, dtype=_np.float64))


class PyDMDc:
    """pyo3 ``PyDMDc(x, u, n_modes, n_iters)`` / ``predict(x0, u)`` (src/lib_math_utils_py.rs:254-283): DMDc with dt = 1,
    both randomized SVDs on the GPU; ``predict`` is ``DMDc::predict_multiple``."""

    def __init__(self, x_np, u_np, n_modes, n_iters):
        self.dmd = _DMDc(_np.asarray(x_np, dtype=_np.float64), _np.asarray(u_np, dtype=_np.float64), 1.0, int(n_modes),
                         int(n_iters))

    def predict(self, x0_np, u_np):
        return self.dmd.predict_multiple(_np.asarray(x0_np, dtype=_np.float64), _np.asarray(u_np, dtype=_np.float64))
