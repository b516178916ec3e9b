"""corrla_rs_amd -- MI355X (gfx950) randomized-SVD engine behind the RSVD hot path of
wgurecky/CORRLA_RS.  The compute path is libcorrla_rsvd.so (hand-written HIP kernels); this package
is the thin host-side mirror of the reference's Python/Rust surfaces.  No CPU fallback.
Dense solves: ``Context.solve`` (LU, or Cholesky with assume="pos"), ``Context.cholesky`` / ``cholesky`` (the factor of a
symmetric positive definite matrix, log det in ``Context.last_chol_info``), ``mvn_factor(device=True)``,
``sample_mv_normal(factor="device")`` and ``RbfInterp(solver="chol")`` on top of them.
Symmetric eigendecomposition: ``Context.eigh`` and the pseudo-inverse solve ``Context.eigh_solve``, with
``quad_fit(solve="device")``, ``mvn_factor(device=True, eig="device")`` and ``RbfInterp(solver="eigh")`` on top of them."""
from .api import (Context, PcaRsvd, algorithmic_flops, default_context, power_iter, random_svd, rpca,  # noqa: F401
                  rsvd)

__version__ = "0.1.0"
from .callers import (ActiveSsRsvd, DeMcSampler, DMDc, FittedActiveSsRsvd, KdeRv, PodI, PolyGradientEstimator, RbfInterp,  # noqa: E402,F401
                      active_ss_fit_svd, build_kde, cholesky, constr_dirichlet_sample, cs_mcmc_dirichlet_sample, jac_from_lin, jac_from_quad, linear_fit, mat_cov_centered, pearson_corr, pod_modes,
                      mvn_factor, polyfit_solve, quad_eval, quad_fit, rbf_apply, rbf_fit, rbf_matrix, rsquared_sens, sample_mv_normal, sandwich_prop)
