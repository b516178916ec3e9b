"""Host-side mirrors of the reference callers that sit on the RSVD hot path.
Every m- or n-sized decomposition goes through the GPU `rsvd`; what remains here is the k-wide algebra the
reference also does after its random_svd calls (k = n_modes, a few tens), written with numpy.

  pod_modes(x, n_modes)                       <- PodI::_modes            src/lib_math_utils/pod_rom.rs:53-58
  active_ss_fit_svd(grad_mat, n_comps, ...)   <- ActiveSsRsvd::fit_svd   src/lib_math_utils/active_subspaces.rs:233-250
  DMDc(x, u, dt, n_modes, n_iters)            <- DMDc::new               src/lib_math_utils/dmd_rom.rs:45-226
                                                 (pyo3 PyDMDc, src/lib_math_utils_py.rs:222-283); CUDA tensors in ->
                                                 device-resident factors and a factored predictor
  PodI(x, t, n_modes) / RbfInterp             <- PodI, RbfInterp         src/lib_math_utils/pod_rom.rs:36-117,
                                                 src/lib_math_utils/interp_utils.rs:11-160 (pyo3 PyPodI, PyRbfInterp)
  PolyGradientEstimator / ActiveSsRsvd / FittedActiveSsRsvd
                                              <- src/lib_math_utils/active_subspaces.rs:21-277 (the
                                                 neighbour search and the local fits run on the GPU)
  mat_cov_centered(x) / pearson_corr(x) / rsquared_sens(x, y, cor_dof)
                                              <- src/lib_math_utils/stats_corr.rs:14-43, 75-107 (the n x n matrix from
                                                 the symmetric MFMA kernel, ``Context.cov``)
  linear_fit / quad_fit / quad_eval / jac_from_lin / jac_from_quad
                                              <- src/lib_math_utils/stats_corr.rs:146-249 (the normal equations and the
                                                 evaluation from the fused kernels, ``Context.polyfit_gram`` /
                                                 ``poly_eval``; the p-sized solve on the host)
  KdeRv(bandwidth, samples) / build_kde(...)  <- KdeRv, build_kde        src/lib_math_utils/univariate_rv.rs:165-170,
                                                 384-497 (the pairwise sums from ``Context.kde_eval`` / ``kde_nll``; the
                                                 bandwidth search on the host over (nll, dnll) evaluations)
  constr_dirichlet_sample / DeMcSampler / cs_mcmc_dirichlet_sample
                                              <- src/lib_math_utils/space_samplers.rs:14-418, lib_math_utils_py.rs:89-168 (the
                                                 draws, the box test and the count on the device, ``Context.dirichlet_sample``;
                                                 the chains, which advance one step after the other, on the host)
  mvn_factor(cov) / sample_mv_normal(cov, n) / sandwich_prop(cov, jac)
                                              <- src/lib_math_utils/stats_corr.rs:46-68 (the d-sized factorisation on the host;
                                                 the rows from the fused kernel, ``Context.mvn_sample``; the per-sample
                                                 variances from ``Context.sandwich_diag``)
Every product with an n_x- or N-sized dimension goes through the library's HIP GEMMs (``Context.matmul``); only
snapshot-count- and n_modes-sized matrices are touched by numpy."""
import numpy as np

from .api import _is_torch, _poly_terms, default_context, rsvd

__all__ = ["pod_modes", "active_ss_fit_svd", "DMDc", "PodI", "RbfInterp", "PolyGradientEstimator", "ActiveSsRsvd",
           "FittedActiveSsRsvd", "mat_cov_centered", "pearson_corr", "rsquared_sens", "rbf_matrix", "rbf_apply",
           "linear_fit", "quad_fit", "quad_eval", "jac_from_lin", "jac_from_quad", "polyfit_solve", "KdeRv", "build_kde",
           "constr_dirichlet_sample", "DeMcSampler", "cs_mcmc_dirichlet_sample", "mvn_factor", "sample_mv_normal",
           "sandwich_prop", "cholesky"]


def _on_gpu(x):
    return _is_torch(x) and x.is_cuda


def pod_modes(x_data, n_modes, *, seed=None, omega=None, ctx=None):
    """(_u, _s, v) = random_svd(x_data, n_modes, 10, 10); modes = v^T, shape (N, n_modes)."""
    _u, _s, vt = (ctx or default_context()).rsvd(np.asarray(x_data, np.float64), n_modes, 10, 10, seed=seed, omega=omega)
    return np.ascontiguousarray(vt.T)


def active_ss_fit_svd(grad_mat, n_comps, n_iter=8, n_oversamples=10, *, seed=None, omega=None, ctx=None):
    """RSVD variant of the active-subspace fit, given the k x N gradient matrix: scale by 1/sqrt(N),
    random_svd(., min(k, n_comps), n_iter, n_oversamples).  Returns (components U (k, r), diag(S) (r, r))."""
    g = np.asarray(grad_mat, np.float64)
    k_features, n_samples = g.shape
    u, s, _vt = (ctx or default_context()).rsvd(g * (1.0 / np.sqrt(float(n_samples))), min(k_features, n_comps), n_iter,
                                                n_oversamples, seed=seed, omega=omega)
    return u, np.diag(s.ravel())


def mat_cov_centered(x, *, ctx=None):
    """``mat_cov_centered(x)`` (stats_corr.rs:32-43): covariance matrix (n, n) of the columns of x, divisor n_samples - 1."""
    return (ctx or default_context()).cov(x)[0]


def pearson_corr(x, *, ctx=None):
    """``pearson_corr(x)`` (stats_corr.rs:14-28): Pearson correlation matrix (n, n) of the columns of x (the standard
    deviations with the divisor n_samples - 1, as ``mat_std``)."""
    return (ctx or default_context()).cov(x, correlation=True)[0]


def rsquared_sens(x, y, cor_dof, *, ctx=None):
    """``rsquared_sens(x, y, cor_dof)`` (stats_corr.rs:75-107): R^2 = r_y^T pinv(r_xx) r_y from the correlation matrix of
    [x | y] (GPU); cor_dof applies 1 - (1 - R^2) (n - 1) / (n - k - 1).  Returns a (1, 1) array."""
    xa, ya = np.asarray(x, np.float64), np.asarray(y, np.float64).reshape(len(y), -1)
    n_samples, k_features = xa.shape
    r_xy = np.asarray((ctx or default_context()).cov(np.hstack([xa, ya]), correlation=True)[0])
    r_xx, r_y = r_xy[:-1, :-1], r_xy[:-1, -1:]
    r_sqr = r_y.T @ _pinv_reg(r_xx) @ r_y
    if cor_dof:
        r_sqr = 1.0 - (1.0 - r_sqr) * ((n_samples - 1.0) / (n_samples - k_features - 1.0))
    return r_sqr


# ---- global polynomial response surfaces (stats_corr.rs:146-249) -----------------------------------------------------------
def _poly_sym(c, k, degree):
    """The coefficient columns c (p, r) in the column order [x, x_a x_b (a <= b, a outer), 1] (degree 1: [x, 1]) as r
    symmetric matrices C (r, k + 1, k + 1) with V(x) c = xt^T C xt, xt = [x, 1]: C(a, a) = c_aa, C(a, b) = c_ab / 2,
    C(a, k) = c_a / 2, C(k, k) = c_0."""
    r = c.shape[1]
    out = np.zeros((r, k + 1, k + 1))
    out[:, :k, k] = out[:, k, :k] = 0.5 * c[:k].T
    out[:, k, k] = c[-1]
    if degree >= 2:
        ia, ib = np.triu_indices(k)  # a-major, b >= a: the order of mat_col_interactions
        q = c[k:-1].T
        out[:, ia, ib] = 0.5 * q
        out[:, ib, ia] += 0.5 * q    # the diagonal gets both halves
    return out


def _poly_unsym(cm, k, degree):
    """the inverse of _poly_sym: (r, k + 1, k + 1) -> (p, r)"""
    rows = [2.0 * cm[:, :k, k].T]
    if degree >= 2:
        ia, ib = np.triu_indices(k)
        rows.append((cm[:, ia, ib] * np.where(ia == ib, 1.0, 2.0)).T)
    rows.append(cm[:, k, k][None, :])
    return np.vstack(rows)


def polyfit_solve(g, k, degree, means=None, scales=None, *, device=False, ctx=None):
    """Coefficients (p, r) of the least-squares polynomial from the Gram matrix G of ``Context.polyfit_gram`` (order p + r),
    in the coordinates of the raw x.  p-sized host work:
      1. V^T V = G[:p, :p] is equilibrated by its diagonal (D^-1/2 A D^-1/2, unit diagonal);
      2. its symmetric eigendecomposition is taken;
      3. only eigenvalues above p 2^-52 lambda_max are inverted -- the minimum-norm solution of the equilibrated system.
         This is the one deliberate difference from the reference: ``mat_pinv`` (mat_utils.rs:37-53) divides by s + 1e-14,
         which turns an exactly rank-deficient V into coefficients of order 1e14 times rounding noise; here the null
         directions are dropped;
      4. the coefficients of the normalised samples z = (x - means) / scales are mapped back to x by the congruence
         C_x = M^T C_z M, M = [[diag(1 / scales), -means / scales], [0, 1]], on the symmetric form of every column.
    device=True: steps 1 to 3 run on the device -- g (a numpy array, which is uploaded, or the CUDA tensor of ``polyfit_gram``,
    which then never visits the host) is equilibrated elementwise and solved by ``Context.eigh_solve`` of `ctx` or the default context, whose default rule
    is the cut of step 3 on |lambda|; only the (p, r) coefficients come back for step 4, which stays as it is.  The device
    eigenvalues carry absolute errors of order p u |A| (``Context.eigh``), which is the scale of the cut, so a direction at the
    cut may fall on either side: compare predictions with the host solve, not coefficients."""
    p = _poly_terms(k, degree)
    if device:
        import torch
        c = ctx or default_context()
        gt = g.detach().to(torch.float64) if _on_gpu(g) else torch.as_tensor(
            np.asarray(g.detach().numpy() if _is_torch(g) else g, dtype=np.float64), device=f"cuda:{c.device}")
        at, bt = gt[:p, :p], gt[:p, p:]
        dt = torch.sqrt(torch.diagonal(at))
        dt = torch.where(dt > 0.0, dt, torch.ones_like(dt))
        cz = (c.eigh_solve((at / torch.outer(dt, dt)).contiguous(), (bt / dt[:, None]).contiguous()) / dt[:, None]).cpu().numpy()
    else:
        g = np.asarray(g, dtype=np.float64)
        a, b = g[:p, :p], g[:p, p:]
        d = np.sqrt(np.diag(a))
        d = np.where(d > 0.0, d, 1.0)
        w, q = np.linalg.eigh(a / np.outer(d, d))
        keep = w > p * 2.0 ** -52 * w[-1]
        qk = q[:, keep]
        cz = (qk @ ((qk.T @ (b / d[:, None])) / w[keep][:, None])) / d[:, None]
    if means is None and scales is None:
        return cz
    host = lambda v: v.detach().cpu().numpy() if _is_torch(v) else v  # noqa: E731
    mu = np.zeros(k) if means is None else np.asarray(host(means), dtype=np.float64).reshape(-1)
    sg = np.ones(k) if scales is None else np.asarray(host(scales), dtype=np.float64).reshape(-1)
    # In extended precision, rounded once: for data far from the origin the intercept of the raw coordinates is a sum of
    # terms (mean / scale)^2 times larger than itself, and (k + 1)^2 numbers per column cost nothing.
    mm = np.zeros((k + 1, k + 1), dtype=np.longdouble)
    inv = (1.0 / sg).astype(np.longdouble)          # the kernel's z = (x - means) * fl(1 / scales)
    mm[np.arange(k), np.arange(k)] = inv
    mm[:k, k] = -mu.astype(np.longdouble) * inv
    mm[k, k] = 1.0
    return _poly_unsym(mm.T @ _poly_sym(cz, k, degree).astype(np.longdouble) @ mm, k, degree).astype(np.float64)


def _poly_fit(x, y, degree, normalize, ctx, solve="host"):
    if solve not in ("host", "device"):
        raise ValueError("solve must be 'host' or 'device'")
    c = ctx or default_context()
    g, means, scales = c.polyfit_gram(x, y, degree, normalize=normalize)
    k = int(x.shape[1])
    on_gpu = _is_torch(g)
    host = (lambda v: None if v is None else v.cpu().numpy()) if on_gpu else (lambda v: v)
    if solve == "device":
        coeffs = polyfit_solve(g, k, degree, means, scales, device=True, ctx=c)  # a CUDA Gram matrix stays on the device
    else:
        coeffs = polyfit_solve(host(g), k, degree, host(means), host(scales))
    if on_gpu:
        import torch
        return torch.from_numpy(coeffs).to(g.device)
    return coeffs


def linear_fit(x, y, *, normalize=True, ctx=None, solve="host"):
    """``linear_fit(x, y)`` (stats_corr.rs:146-160): least-squares coefficients (k + 1, r) of y = [x, 1] c -- slopes, then
    the intercept -- from the fused normal-equation kernel (``Context.polyfit_gram``) and the host solve of
    ``polyfit_solve``; the (m, k + 1) Vandermonde matrix is never stored.  The coefficients are in the coordinates of the
    raw x whether or not the kernel normalises.  numpy in -> numpy out, CUDA tensors in -> a tensor on their device.
    solve="device": the p-sized solve runs on the device too (``polyfit_solve(device=True)``)."""
    return _poly_fit(x, y, 1, normalize, ctx, solve)


def quad_fit(x, y, *, normalize=True, ctx=None, solve="host"):
    """``quad_fit(x, y)`` (stats_corr.rs:213-219): least-squares coefficients (p, r), p = k + k (k + 1) / 2 + 1, of
    y = [x, x_a x_b (a <= b, a outer), 1] c, as ``linear_fit``.  Where V is rank-deficient the reference's
    ``pinv`` with 1 / (s + 1e-14) returns noise along the null directions; this returns the minimum-norm solution of the
    equilibrated system (``polyfit_solve``), so compare predictions there, not coefficients.  solve="device": the p-sized
    solve runs on the device too (``polyfit_solve(device=True)``: ``Context.eigh_solve``).  With CUDA tensors the Gram matrix
    never visits the host; with numpy inputs ``polyfit_gram`` returns it as a numpy array and it is uploaded again for the
    solve.  Compare it with the host solve on predictions as well."""
    return _poly_fit(x, y, 2, normalize, ctx, solve)


def quad_eval(x, coeffs, *, ctx=None):
    """``quad_eval(x, coeffs)`` (stats_corr.rs:222-226): the quadratic at the rows of x, (m, r), on the device
    (``Context.poly_eval``)."""
    return (ctx or default_context()).poly_eval(x, coeffs, 2)


def jac_from_lin(x, y, *, normalize=True, ctx=None):
    """``jac_from_lin(x, y)`` (stats_corr.rs:164-169): the slopes of ``linear_fit`` as a row per column of y, (r, k)."""
    c = linear_fit(x, y, normalize=normalize, ctx=ctx)
    return c[:x.shape[1]].T


def jac_from_quad(x0, coeffs, *, ctx=None):
    """``jac_from_quad(x0, coeffs)`` (stats_corr.rs:230-249): the gradient of the quadratic at the rows of x0, (m, k) for one
    coefficient column and (r, m, k) for r of them.  This is the ANALYTIC gradient 2 (C xt)[:k] from the evaluation kernel;
    the reference differences forward with eps = 1e-10 and so carries a rounding error of about 4 * 2^-52 max|y| / 1e-10."""
    return (ctx or default_context()).poly_eval(x0, coeffs, 2, jac=True)[1]


class PolyGradientEstimator:
    """Mirror of ``PolyGradientEstimator`` (active_subspaces.rs:21-141): local polynomial gradient estimates over a
    point cloud.  The nearest-neighbour search and the per-point least-squares fits run on the GPU
    (``corrla_grad_mat_f64``) for any number of features and neighbours, like the reference; ``grad_at`` returns the
    reference's 1 x k row."""

    def __init__(self, x_mat, y, est_order, n_nbrs, *, ctx=None):
        self.x_mat = np.ascontiguousarray(np.asarray(x_mat, dtype=np.float64))
        self.y = np.asarray(y, dtype=np.float64).reshape(-1)
        self.est_order, self.n_nbrs, self.k = int(est_order), int(n_nbrs), self.x_mat.shape[1]
        self._ctx = ctx
        if self.est_order not in (1, 2):
            raise ValueError("Not implemented est order")   # the reference panics (active_subspaces.rs:60)

    def grad_mat(self, x_query=None, scale=1.0):
        """k x n_q gradient matrix (create_grad_mat, active_subspaces.rs:215-229)."""
        g, self.n_regularised = (self._ctx or default_context()).grad_mat(self.x_mat, self.y, self.est_order, self.n_nbrs,
                                                                           x_query, scale=scale)
        return g

    def grad_at(self, x0):
        return self.grad_mat(np.asarray(x0, dtype=np.float64).reshape(1, -1)).T.copy()


class FittedActiveSsRsvd:
    """active_subspaces.rs:41-47, 143-201."""

    def __init__(self, components, singular_vals, n_comps):
        self.components_, self.singular_vals_, self.n_comps = components, singular_vals, int(n_comps)

    def components(self):
        return self.components_[:, : self.n_comps]

    def singular_vals(self):
        return self.singular_vals_[:, : self.n_comps]

    def transform(self, x_mat):
        return np.asarray(x_mat, dtype=np.float64) @ self.components()

    def inv_transform(self, x_mat):
        x = np.asarray(x_mat, dtype=np.float64)
        if x.shape[1] != self.n_comps:
            raise ValueError("x_mat must have n_comps columns")     # assert at active_subspaces.rs:186
        return x @ self.components().T

    def var_diag_evd_sensi(self):
        m = self.components_.T @ self.singular_vals_ @ self.components_   # as written at active_subspaces.rs:162-164
        return np.diag(m).copy()


class ActiveSsRsvd:
    """Mirror of ``ActiveSsRsvd`` (active_subspaces.rs:35-277): gradient matrix on the GPU, then either the RSVD of
    G / sqrt(N) (``fit_svd``, on the GPU) or the eigendecomposition of the k x k matrix G G^T / N (``fit``; the Gram
    product runs on the GPU through the RSVD library's GEMM, the k x k symmetric eigenproblem in numpy)."""

    def __init__(self, grad_est, n_comps, *, ctx=None):
        self.grad_est, self.n_comps, self._ctx = grad_est, int(n_comps), ctx

    def fit_svd(self, x_mat, n_iter=None, n_oversamples=None, *, seed=None, omega=None):
        x = np.asarray(x_mat, dtype=np.float64)
        g = self.grad_est.grad_mat(x, scale=1.0 / np.sqrt(float(x.shape[0])))       # :238-239
        u, s, _vt = rsvd(g, min(x.shape[1], self.n_comps), 8 if n_iter is None else n_iter,
                         10 if n_oversamples is None else n_oversamples, seed=seed, omega=omega, ctx=self._ctx)   # :242-244
        return FittedActiveSsRsvd(u, np.diag(s.ravel()), self.n_comps)

    def fit_svd_sharded(self, x_mat, rank, world, n_iter=None, n_oversamples=None, *, seed=1):
        """``fit_svd`` with the sample points sharded over `world` GPUs, one process per GPU (BASELINE config 5): the
        support cloud is replicated, rank r estimates the gradients of its contiguous slice of the samples (no
        exchange), and the RSVD of G / sqrt(N) runs on the row-sharded N x k tall view (``rsvd_sharded``: all-reduces of
        k x l blocks only).  The context must carry a communicator (``Context.comm_init``).  Every rank returns the
        same fitted object."""
        import torch
        x = np.asarray(x_mat, dtype=np.float64)
        n = x.shape[0]
        lo, hi = (n * rank) // world, (n * (rank + 1)) // world
        ctx = self._ctx or default_context()
        dev = torch.device(f"cuda:{ctx.device}")
        xs = torch.as_tensor(np.ascontiguousarray(self.grad_est.x_mat), device=dev)
        ys = torch.as_tensor(self.grad_est.y, device=dev)
        g_loc, self.grad_est.n_regularised = ctx.grad_mat(xs, ys, self.grad_est.est_order, self.grad_est.n_nbrs,
                                                          torch.as_tensor(np.ascontiguousarray(x[lo:hi]), device=dev),
                                                          scale=1.0 / np.sqrt(float(n)))
        k_comp = min(x.shape[1], self.n_comps)
        _u_loc, s, vt = ctx.rsvd_sharded(g_loc.t(), k_comp, 8 if n_iter is None else n_iter,
                                         10 if n_oversamples is None else n_oversamples, seed=seed)
        # the tall view is G^T (N x k): its right singular vectors are the k x r components `ur` of fit_svd
        return FittedActiveSsRsvd(vt.t().cpu().numpy().copy(), np.diag(s.cpu().numpy().ravel()), self.n_comps)

    def fit(self, x_mat):
        import torch
        x = np.asarray(x_mat, dtype=np.float64)
        ctx = self._ctx or self.grad_est._ctx or default_context()
        dev = torch.device(f"cuda:{ctx.device}")
        ge = self.grad_est
        g, ge.n_regularised = ctx.grad_mat(torch.as_tensor(ge.x_mat, device=dev), torch.as_tensor(ge.y, device=dev),
                                           ge.est_order, ge.n_nbrs, torch.as_tensor(np.ascontiguousarray(x), device=dev))
        gt = g.t()                                                                   # N x k row-major, on the device
        c = ctx.matmul(gt, gt, trans=True).cpu().numpy() * (1.0 / x.shape[0])        # G G^T / N  (k x k), :256
        c = 0.5 * (c + c.T)
        w, v = np.linalg.eigh(c)
        order = np.argsort(-w, kind="stable")                                        # sort_evd, mat_utils.rs:459-478
        return FittedActiveSsRsvd(v[:, order], np.diag(w[order]), self.n_comps)


def _pinv_diag(d):  # mat_pinv_diag, mat_utils.rs:386-402
    out = np.zeros_like(d)
    idx = np.arange(d.shape[1])
    v = d[idx, idx]
    big = np.abs(v) >= 1e-20
    out[idx[big], idx[big]] = 1.0 / (v[big] + 1e-20)
    return out


class DMDc:
    """Dynamic mode decomposition with control (Proctor et al.), dmd_rom.rs:20-226: two randomized SVDs with 12
    oversamples (input space [x; u][:, :-1] and output space x[:, 1:]) on the GPU, then the n_modes-wide
    operator algebra and the complex eigendecomposition of the n_modes x n_modes A~ on the host."""

    def __init__(self, x_data, u_data, dt, n_modes, n_iters, *, seed=None, omega_x=None, omega_y=None, ctx=None):
        c = ctx or default_context()
        self.on_device = _on_gpu(x_data)
        if self.on_device:
            self._init_device(c, x_data, u_data, float(dt), int(n_modes), int(n_iters), seed, omega_x, omega_y)
            return
        x_data = np.asarray(x_data, np.float64)
        u_data = np.asarray(u_data, np.float64)
        self.n_snapshots, self.n_x, self.n_u = x_data.shape[1], x_data.shape[0], u_data.shape[0]
        self.n_modes, self.dt_snapshots = int(n_modes), float(dt)
        omega = np.vstack([x_data, u_data])
        xin, yout = omega[:, :-1], omega[: self.n_x, 1:]
        u_til, s_til, vt_til = c.rsvd(xin, n_modes, n_iters, 12, seed=seed, omega=omega_x)
        u_hat, _s_hat, _vt_hat = c.rsvd(yout, n_modes, n_iters, 12, seed=None if seed is None else seed + 1, omega=omega_y)
        v_til = vt_til.T
        u1, u2 = u_til[: self.n_x], u_til[self.n_x:]
        s_inv = _pinv_diag(np.diag(s_til.ravel()))
        tmp = u_hat.T @ yout @ v_til @ s_inv          # eq. 29
        self._A = tmp @ u1.T @ u_hat
        self._B = u_hat @ (tmp @ u2.T)                # eq. 30, lifted back
        lam, w = np.linalg.eig(self._A)
        self.lambdas = lam.reshape(-1, 1)
        scale = yout @ (v_til @ (s_inv @ (u1.T @ u_hat)))   # eq. 36
        modes = scale @ w
        self.modes_re, self.modes_im = np.real(modes).copy(), np.imag(modes).copy()

    # ---- device-resident variant: x_data / u_data are CUDA tensors ------------------------------
    def _init_device(self, c, x_data, u_data, dt, n_modes, n_iters, seed, omega_x, omega_y):
        """Same algebra as the host path with every n_x-sized factor left on the GPU: the two randomized SVDs return
        device tensors, the products that contract or produce an n_x-sized dimension run through ``Context.matmul``
        (the library's HIP GEMMs), and only snapshot-count x n_modes and n_modes x n_modes matrices visit the host
        (diag pinv, the complex eigendecomposition of A~).  The dense n_x x n_x operator of ``est_a_til`` is never
        needed for prediction: A = Re(Phi Lambda Phi^+) = Pc K Pc^T with Pc = [Re Phi | Im Phi] (n_x x 2 n_modes) and
        a 2 n_modes x 2 n_modes real K, so ``predict_multiple`` runs its recurrence in 2 n_modes dimensions."""
        import torch
        dev = torch.device(f"cuda:{c.device}")
        self._ctx, self._dev = c, dev
        x = x_data.to(device=dev, dtype=torch.float64)
        u = torch.as_tensor(u_data, dtype=torch.float64, device=dev)
        self.n_snapshots, self.n_x, self.n_u = x.shape[1], x.shape[0], u.shape[0]
        self.n_modes, self.dt_snapshots = n_modes, dt
        k = n_modes
        omega = torch.cat([x, u], dim=0)                         # mat_vstack, dmd_rom.rs:66
        xin, yout = omega[:, :-1], omega[: self.n_x, 1:]         # _X / _Y: strided views, no copies
        u_til, s_til, vt_til = c.rsvd(xin, k, n_iters, 12, seed=seed, omega=omega_x)
        u_hat, _s, _v = c.rsvd(yout, k, n_iters, 12, seed=None if seed is None else seed + 1, omega=omega_y)
        u1, u2 = u_til[: self.n_x], u_til[self.n_x:]
        up = lambda h: torch.as_tensor(np.ascontiguousarray(h), dtype=torch.float64, device=dev)  # noqa: E731
        s_inv = _pinv_diag(np.diag(s_til.cpu().numpy().ravel()))
        v_til = vt_til.t().cpu().numpy()                         # (n_t - 1, k)
        ytu = c.matmul(yout, u_hat, trans=True).cpu().numpy()    # Y^T U^ (n_t - 1, k)
        tmp = ytu.T @ v_til @ s_inv                              # eq. 29: U^^T Y V~ S~^-1
        m1 = c.matmul(u1, u_hat, trans=True).cpu().numpy()       # U~1^T U^ (k, k)
        self._A = tmp @ m1
        b_til = c.matmul(u2, up(tmp.T))                          # (n_u, k) = U~2 tmp^T = (tmp U~2^T)^T, eq. 30
        self._B = c.matmul(u_hat, b_til.t()).contiguous()        # U^ b~  (n_x, n_u), on the device
        lam, w = np.linalg.eig(self._A)
        self.lambdas = lam.reshape(-1, 1)
        scale = c.matmul(yout, up(v_til @ (s_inv @ m1)))         # eq. 36 (n_x, k)
        self._pc = c.matmul(scale, up(np.hstack([w.real, w.imag]))).contiguous()   # [Re Phi | Im Phi]
        self.modes_re, self.modes_im = self._pc[:, :k], self._pc[:, k:]
        # Phi^+ = (Phi^H Phi)^+ Phi^H from the 2k x 2k Gram of Pc.  Columns of Phi are scaled to unit length first
        # (a Gram matrix squares the condition number; the scaling removes the part of it that is mere column
        # scaling); modes whose norm is below 1e-8 of the largest are rounding noise of null eigen-directions of A~
        # (n_modes beyond the rank of the data) and are dropped, as the truncated pseudo-inverse would.
        gc = c.matmul(self._pc, self._pc, trans=True).cpu().numpy()
        g = (gc[:k, :k] + gc[k:, k:]) + 1j * (gc[:k, k:] - gc[k:, :k])
        d = np.sqrt(np.maximum(np.real(np.diag(g)), 0.0))
        keep = d > 1e-8 * max(d.max(), 1e-300)
        dinv = np.where(keep, 1.0 / np.where(keep, d, 1.0), 0.0)
        g_inv = (dinv[:, None] * np.linalg.pinv(g * np.outer(dinv, dinv), hermitian=True)) * dinv[None, :]
        h = np.diag(lam) @ g_inv                                 # Lambda (Phi^H Phi)^+ ;  A = Re(Phi h Phi^H)
        self._K = np.block([[h.real, h.imag], [-h.imag, h.real]])
        self._gc = gc
        self._pcb = torch.cat([self._pc, self._B], dim=1).contiguous()   # [Pc | B]: one GEMM per prediction batch

    def _est_a_til_device(self):
        c = self._ctx
        import torch
        t = c.matmul(self._pc, torch.as_tensor(self._K, dtype=torch.float64, device=self._dev))
        return c.matmul(t, self._pc.t())

    def _predict_multiple_device(self, x_0, u_seq):
        import torch
        c, dev = self._ctx, self._dev
        x0 = torch.as_tensor(x_0, dtype=torch.float64, device=dev).reshape(-1, 1)
        useq = u_seq.detach().cpu().numpy() if _is_torch(u_seq) else np.asarray(u_seq, np.float64)
        useq = useq.reshape(self.n_u, -1).astype(np.float64)
        if x0.shape[0] != self.n_x:
            raise ValueError("x_0 must have n_x rows")           # assert_eq at dmd_rom.rs:199
        z = c.matmul(self._pc, x0, trans=True).cpu().numpy()     # Pc^T x_0           (2k, 1)
        bz = c.matmul(self._pc, self._B, trans=True).cpu().numpy()   # Pc^T B         (2k, n_u)
        n_s = useq.shape[1]
        coef = np.empty((self._K.shape[0] + self.n_u, n_s))
        for j in range(n_s):                                     # x_{j+1} = Pc (K Pc^T x_j) + B u_j
            kz = self._K @ z
            coef[:, j] = np.concatenate([kz.ravel(), useq[:, j]])
            z = self._gc @ kz + bz @ useq[:, j:j + 1]
        return c.matmul(self._pcb, torch.as_tensor(coef, dtype=torch.float64, device=dev))

    def est_a_til(self):
        if self.on_device:
            return self._est_a_til_device()
        modes = self.modes_re + 1j * self.modes_im
        return np.real(modes @ np.diag(self.lambdas.ravel()) @ np.linalg.pinv(modes))

    def est_b_til(self):
        return self._B

    def predict(self, x_0, u_input):
        if self.on_device:
            u1 = u_input.detach().cpu().numpy() if _is_torch(u_input) else np.asarray(u_input, np.float64)
            return self._predict_multiple_device(x_0, u1.reshape(self.n_u, 1))
        return self.est_a_til() @ np.asarray(x_0, np.float64).reshape(-1, 1) + self._B @ np.asarray(u_input, np.float64).reshape(-1, 1)

    def predict_multiple(self, x_0, u_seq):
        if self.on_device:
            return self._predict_multiple_device(x_0, u_seq)
        a = self.est_a_til()
        u_seq = np.asarray(u_seq, np.float64)
        x = np.asarray(x_0, np.float64).reshape(-1, 1)
        out = np.zeros((self.n_x, u_seq.shape[1]))
        for j in range(u_seq.shape[1]):
            x = a @ x + self._B @ u_seq[:, j:j + 1]
            out[:, j] = x[:, 0]
        return out


# ---- POD with interpolated mode weights ---------------------------------------------------------------
def _poly_block(x, degree):
    """build_full_vandermonde (stats_corr.rs:183-207): [x, 1] below degree 2, else [x, x_a x_b (a <= b), 1]."""
    cols = [x]
    if degree >= 2:
        d = x.shape[1]
        cols += [x[:, a:a + 1] * x[:, b:b + 1] for a in range(d) for b in range(a, d)]
    return np.hstack(cols + [np.ones((x.shape[0], 1))])


def _pinv_reg(m):  # mat_pinv, mat_utils.rs:37-53: every singular value inverted as 1 / (s + 1e-14)
    u, sv, vt = np.linalg.svd(m, full_matrices=False)
    return (vt.T * (1.0 / (sv + 1.0e-14))) @ u.T


def rbf_matrix(x_query, x_support, kernel_type, kernel_param=0.0, *, ctx=None):
    """The kernel matrix phi(||x_query_i - x_support_j||), (n_q, n_s), on the device: ``Context.rbf_matrix``."""
    return (ctx or default_context()).rbf_matrix(x_query, x_support, kernel_type, kernel_param)


def rbf_apply(x_query, x_support, coeffs, kernel_type, kernel_param=0.0, *, poly_degree=None, ctx=None):
    """Phi(x_query, x_support) @ W_rbf + P(x_query) @ W_poly without the (n_q, n_s) matrix: ``Context.rbf_apply``."""
    return (ctx or default_context()).rbf_apply(x_query, x_support, coeffs, kernel_type, kernel_param, poly_degree=poly_degree)


def rbf_fit(x, y, kernel_type, kernel_param=0.0, *, poly_degree=None, ctx=None):
    """The coefficients of the RBF interpolant through (x, y) by an LU solve on the device: ``Context.rbf_fit``."""
    return (ctx or default_context()).rbf_fit(x, y, kernel_type, kernel_param, poly_degree=poly_degree)


def cholesky(a, *, overwrite=False, ctx=None):
    """The Cholesky factor L of a symmetric positive definite matrix, a = L L^T, on the device: ``Context.cholesky`` (only the
    lower triangle of `a` is read).  ``Context.solve(a, b, assume="pos")`` solves with it."""
    return (ctx or default_context()).cholesky(a, overwrite=overwrite)


class RbfInterp:
    """Radial-basis-function interpolant with a polynomial tail (interp_utils.rs:11-160; pyo3 ``PyRbfInterp(kernel_type,
    kernel_param, dim, poly_degree)``: 1 linear r, 2 multiquadric sqrt(1 + (eps r)^2), 3 cubic r^3, otherwise Gaussian
    exp(-(eps r)^2)).  ``fit`` accepts several right-hand-side columns at once (PodI fits one interpolant per mode weight
    over the same support points).

    device=False and numpy arguments: the numpy code, sized by the number of support points (snapshots), on the host.
    device=True, or whenever ``fit`` / ``predict`` is handed a CUDA tensor: the kernel matrix of the fit comes from
    ``Context.rbf_matrix(x, x)`` and ``predict`` is one ``Context.rbf_apply`` -- the (n_q, n_s) kernel matrix of the
    queries is never stored, so 10^5 queries against 10^4 supports need no 8 GB temporary.  The solve of the
    (n_s + n_poly)-sized block system stays on the host in float64: its SVD pseudo-inverse with every singular value
    inverted as 1 / (s + 1e-14) (``mat_pinv``) is what parity with the reference means.  numpy in -> numpy out, a tensor
    in -> a tensor out; ``predict`` with a CUDA query on a host-fitted model uploads the small model per call.

    solver="pinv" (the default) is that route, bit for bit.  solver="lu" is opt-in and always runs on the device: ``fit`` is
    one ``Context.rbf_fit`` -- the block system is built in device workspace and solved there by LU with partial pivoting;
    with the supports on the device only `y` crosses to it (if it was a host array) and no system-sized array returns.  Its
    coefficients differ from the pseudo-inverse's within the conditioning of the system (both are backward stable), not bit
    for bit.  A singular system (coincident supports, fewer supports than the polynomial tail needs) raises RuntimeError
    naming the column where the pseudo-inverse would return a minimum-norm answer; what is detected is an exactly zero or
    non-finite pivot -- a nearly singular system completes, and ``Context.last_solve_info["min_pivot"]`` is the witness.
    Measured on one MI355X (dim 3, cubic kernel, linear tail, 8 right-hand sides): "lu" 33 ms / 168 ms / 543 ms at 2048 /
    8192 / 16384 supports against 0.81 s / 25 s for "pinv" at the first two -- faster at every size from 2048 up.

    solver="chol" is opt-in too and is accepted only where the kernel matrix is positive definite and nothing else enters the
    system: the Gaussian kernel with poly_degree=None (no polynomial tail); anything else is a ValueError at construction.
    ``fit`` is ``Context.rbf_system`` followed by ``Context.solve(..., assume="pos", overwrite=True)`` on the device: a
    Cholesky factorisation of the lower triangle, half the work of "lu" and no pivot search.  A kernel matrix that is
    numerically not positive definite (supports too close together for the kernel parameter) raises the ``CorrlaError``
    naming the column of the failed pivot: "lu" and "pinv" remain for that case.

    solver="eigh" is opt-in and always runs on the device: ``fit`` is ``Context.rbf_system`` followed by
    ``Context.eigh_solve(..., reg=1e-14)``.  The block system is symmetric, and for a symmetric matrix the SVD pseudo-inverse
    with 1 / (s + 1e-14) is V diag(sign(l) / (|l| + 1e-14)) V^T: this is the reference's pseudo-inverse rule on the device, and
    unlike "lu" it returns the minimum-norm answer on a singular system (coincident supports) where "lu" raises.  Its
    coefficients agree with "pinv" within the conditioning of the system, not bit for bit: compare predictions."""

    def __init__(self, kernel_type, kernel_param, dim, poly_degree, *, device=False, ctx=None, solver="pinv"):
        if solver not in ("pinv", "lu", "chol", "eigh"):
            raise ValueError("solver must be 'pinv', 'lu', 'chol' or 'eigh'")
        if solver == "chol":
            if int(kernel_type) in (1, 2, 3) or poly_degree is not None:
                raise ValueError("solver='chol' takes a positive-definite system: the Gaussian kernel with poly_degree=None")
        else:
            poly_degree = int(poly_degree)
        self.kernel_type, self.eps, self.dim, self.poly_degree = int(kernel_type), float(kernel_param), int(dim), poly_degree
        self.x_known = self.coeffs = None
        self.device, self._ctx = bool(device), ctx
        self.solver = solver

    def _phi(self, r):
        if self.kernel_type == 1:
            return r
        if self.kernel_type == 2:
            return np.sqrt(1.0 + (self.eps * r) ** 2)
        if self.kernel_type == 3:
            return r * r * r
        return np.exp(-((r * self.eps) ** 2))

    def _upper(self, x):
        r = np.sqrt(((x[:, None, :] - self.x_known[None, :, :]) ** 2).sum(axis=2))
        return np.hstack([self._phi(r), _poly_block(x, self.poly_degree)])

    def _context(self):
        if self._ctx is None:
            self._ctx = default_context()
        return self._ctx

    def fit(self, x_in, y_in):
        if self.solver == "lu":
            return self._fit_lu(x_in, y_in)
        if self.solver == "chol":
            return self._fit_chol(x_in, y_in)
        if self.solver == "eigh":
            return self._fit_eigh(x_in, y_in)
        if self.device or _on_gpu(x_in) or _on_gpu(y_in):
            return self._fit_device(x_in, y_in)
        x = np.asarray(x_in, np.float64)
        y = np.asarray(y_in, np.float64).reshape(x.shape[0], -1)
        if x.shape[1] != self.dim:
            raise ValueError("x_in must have `dim` columns")     # assert_eq at interp_utils.rs:133
        self.x_known = x.copy()
        upper = self._upper(x)
        p = upper[:, x.shape[0]:]
        kp = np.vstack([upper, np.hstack([p.T, np.zeros((p.shape[1], p.shape[1]))])])
        self.coeffs = _pinv_reg(kp) @ np.vstack([y, np.zeros((p.shape[1], y.shape[1]))])

    def _fit_device(self, x_in, y_in):
        """K from the device (float64), the block system [[K, P], [P^T, 0]] and its regularised pseudo-inverse on the host;
        the model stays where the supports were given: on the device for a CUDA tensor, else on the host."""
        on_gpu = _on_gpu(x_in)
        x = x_in.detach().double() if on_gpu else np.asarray(x_in.detach().cpu().numpy() if _is_torch(x_in) else x_in, np.float64)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError("x_in must have `dim` columns")
        y = np.asarray(y_in.detach().cpu().numpy() if _is_torch(y_in) else y_in, np.float64).reshape(x.shape[0], -1)
        k = self._context().rbf_matrix(x, x, self.kernel_type, self.eps)
        x_host = x.cpu().numpy() if on_gpu else x
        k = k.cpu().numpy() if on_gpu else k
        p = _poly_block(x_host, self.poly_degree)
        kp = np.vstack([np.hstack([k, p]), np.hstack([p.T, np.zeros((p.shape[1], p.shape[1]))])])
        coeffs = _pinv_reg(kp) @ np.vstack([y, np.zeros((p.shape[1], y.shape[1]))])
        if on_gpu:
            import torch
            self.x_known, self.coeffs = x.clone(), torch.as_tensor(coeffs, device=x.device)
        else:
            self.x_known, self.coeffs = x.copy(), coeffs

    def _fit_lu(self, x_in, y_in):
        """one Context.rbf_fit in float64; the model stays where the supports were given"""
        on_gpu = _on_gpu(x_in)
        x = x_in.detach().double() if on_gpu else np.asarray(x_in.detach().cpu().numpy() if _is_torch(x_in) else x_in, np.float64)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError("x_in must have `dim` columns")
        y = y_in.detach() if _is_torch(y_in) else np.asarray(y_in, np.float64)
        coeffs = self._context().rbf_fit(x, y.reshape(x.shape[0], -1), self.kernel_type, self.eps, poly_degree=self.poly_degree)
        self.x_known, self.coeffs = (x.clone() if on_gpu else x.copy()), coeffs

    def _fit_chol(self, x_in, y_in):
        """Context.rbf_system, then the Cholesky solve in place, in float64 on the device; the model stays where the supports
        were given"""
        import torch
        ctx = self._context()
        on_gpu = _on_gpu(x_in)
        x = x_in.detach().double() if on_gpu else np.asarray(x_in.detach().cpu().numpy() if _is_torch(x_in) else x_in, np.float64)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError("x_in must have `dim` columns")
        xd = x if on_gpu else torch.tensor(x, device=f"cuda:{ctx.device}")  # (copies: the arrays may be read-only)
        y = y_in.detach() if _is_torch(y_in) else torch.tensor(np.asarray(y_in, np.float64))
        yd = y.to(device=xd.device, dtype=torch.float64).reshape(x.shape[0], -1).contiguous().clone()
        m = ctx.rbf_system(xd, self.kernel_type, self.eps, poly_degree=None)
        coeffs = ctx.solve(m, yd, assume="pos", overwrite=True)
        self.x_known, self.coeffs = (x.clone(), coeffs) if on_gpu else (x.copy(), coeffs.cpu().numpy())

    def _fit_eigh(self, x_in, y_in):
        """Context.rbf_system, then the regularised pseudo-inverse solve through the symmetric eigendecomposition, in float64
        on the device; the model stays where the supports were given"""
        import torch
        ctx = self._context()
        on_gpu = _on_gpu(x_in)
        x = x_in.detach().double() if on_gpu else np.asarray(x_in.detach().cpu().numpy() if _is_torch(x_in) else x_in, np.float64)
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError("x_in must have `dim` columns")
        xd = x if on_gpu else torch.tensor(x, device=f"cuda:{ctx.device}")  # (copies: the arrays may be read-only)
        y = y_in.detach() if _is_torch(y_in) else torch.tensor(np.asarray(y_in, np.float64))
        yd = y.to(device=xd.device, dtype=torch.float64).reshape(x.shape[0], -1)
        m = ctx.rbf_system(xd, self.kernel_type, self.eps, poly_degree=self.poly_degree)
        rhs = torch.zeros((m.shape[0], yd.shape[1]), dtype=torch.float64, device=xd.device)
        rhs[:x.shape[0]] = yd
        coeffs = ctx.eigh_solve(m, rhs, reg=1e-14)
        self.x_known, self.coeffs = (x.clone(), coeffs) if on_gpu else (x.copy(), coeffs.cpu().numpy())

    def predict(self, x_query):
        if self.device or self.solver in ("lu", "chol", "eigh") or _on_gpu(x_query) or _on_gpu(self.x_known):
            return self._predict_device(x_query)
        xq = np.asarray(x_query, np.float64)
        if xq.shape[1] != self.dim:
            raise ValueError("x_query must have `dim` columns")  # assert_eq at interp_utils.rs:149
        return self._upper(xq) @ self.coeffs

    def _predict_device(self, x_query):
        """one Context.rbf_apply in float64; the result is of the kind of the query"""
        if self.coeffs is None:
            raise ValueError("predict before fit")
        on_gpu = _on_gpu(x_query)
        xq = x_query.detach().double() if on_gpu else np.asarray(x_query.detach().cpu().numpy() if _is_torch(x_query) else x_query,
                                                                 np.float64)
        if xq.ndim != 2 or xq.shape[1] != self.dim:
            raise ValueError("x_query must have `dim` columns")
        return self._context().rbf_apply(xq, self.x_known, self.coeffs, self.kernel_type, self.eps, poly_degree=self.poly_degree)


class PodI:
    """Proper orthogonal decomposition with interpolated mode weights (pod_rom.rs:36-117; pyo3 ``PyPodI(x, t, n_modes)``):
    x_data is n_snapshots x N, t is n_snapshots x dim.  Modes = right singular vectors of random_svd(x, n_modes, 10, 10) on
    the GPU; the weights of snapshot i are pinv(modes) x_i^T -- the modes are orthonormal, so that is x_i modes, one HIP
    GEMM X * modes instead of the reference's N-sized pseudo-inverse; every weight column gets a linear-kernel RBF
    interpolant over t (host, n_snapshots-sized).  ``predict(t_query)`` returns modes * w(t_query), N x 1, as a numpy
    array, or as a CUDA tensor when x_data was one."""

    def __init__(self, x_data, t, n_modes, *, seed=None, omega=None, ctx=None):
        import torch
        c = ctx or default_context()
        self._ctx, self.on_device = c, _on_gpu(x_data)
        dev = torch.device(f"cuda:{c.device}")
        x = (x_data if self.on_device else torch.as_tensor(np.asarray(x_data, np.float64))).to(device=dev, dtype=torch.float64)
        t = np.asarray(t.detach().cpu().numpy() if _is_torch(t) else t, np.float64)
        if t.shape[0] != x.shape[0]:
            raise ValueError("t and x_data must have the same number of rows")   # assert_eq at pod_rom.rs:38
        self.n_snapshots, self.n_modes, self.t_abscissa = x.shape[0], int(n_modes), t
        _u, _s, vt = c.rsvd(x, self.n_modes, 10, 10, seed=seed, omega=omega)     # pod_rom.rs:53-58
        self._modes = vt.t()                                                     # (N, n_modes), on the device
        self.mode_weights = c.matmul(x, self._modes).cpu().numpy()               # (n_snapshots, n_modes)
        self._interp = RbfInterp(1, 0.0, t.shape[1], 1)                          # pod_rom.rs:78-95
        self._interp.fit(t, self.mode_weights)

    @property
    def modes(self):
        return self._modes if self.on_device else self._modes.cpu().numpy()

    def predict(self, t_query):
        tq = np.asarray(t_query.detach().cpu().numpy() if _is_torch(t_query) else t_query, np.float64)
        if tq.ndim != 2 or tq.shape[0] != 1:
            raise ValueError("t_query must be a single row")                     # assert_eq at pod_rom.rs:105
        return self.predict_many(tq)

    def predict_many(self, t_queries):
        """Additive: N x n_q fields for n_q query rows at once (one GEMM)."""
        import torch
        w = self._interp.predict(np.asarray(t_queries, np.float64)).T           # (n_modes, n_q)
        out = self._ctx.matmul(self._modes, torch.as_tensor(np.ascontiguousarray(w), dtype=torch.float64, device=self._modes.device))
        return out if self.on_device else out.cpu().numpy()


# ---- Gaussian kernel density estimates (univariate_rv.rs:165-170, 384-497) ------------------------------------------------------
_KDE_HOST_PAIRS = 1 << 21        # (point, support) pairs the numpy path holds at once: 16 MiB of float64 per temporary
_KDE_GRID = 64                   # bandwidths per likelihood evaluation: what one ``Context.kde_nll`` call takes
_KDE_MAX_CALLS = 12              # likelihood evaluations of one ``est_bandwidth``
_SQRT_2PI = float(np.sqrt(2.0 * np.pi))


def _kde_host_blocks(n_q, n_s):
    """row and support block lengths with rows x supports <= _KDE_HOST_PAIRS"""
    sc = min(n_s, _KDE_HOST_PAIRS)
    return max(1, _KDE_HOST_PAIRS // sc), sc


def _kde_host_dstar(x, s, sc):
    """min_j (x_i - s_j)^2 for a block of points, the supports taken sc at a time"""
    m = np.full(x.shape[0], np.inf)
    for j0 in range(0, s.shape[0], sc):
        d = x[:, None] - s[None, j0:j0 + sc]
        m = np.minimum(m, (d * d).min(axis=1))
    return m


def _kde_host_eval(x, s, h, what):
    """The stabilised formulas of corrla_kde_eval_* restated in numpy (float64), block by block."""
    import math
    n_q, n_s = x.shape[0], s.shape[0]
    rows, sc = _kde_host_blocks(n_q, n_s)
    out = np.empty(n_q)
    erfc = np.frompyfunc(math.erfc, 1, 1)  # numpy has no erfc
    c = 1.0 / (2.0 * h * h)
    for i0 in range(0, n_q, rows):
        xb = x[i0:i0 + rows]
        if what == "cdf":
            acc = np.zeros(xb.shape[0])
            for j0 in range(0, n_s, sc):
                z = -(xb[:, None] - s[None, j0:j0 + sc]) * (1.0 / (h * np.sqrt(2.0)))
                acc += erfc(z).astype(np.float64).sum(axis=1)
            out[i0:i0 + rows] = 0.5 * acc / n_s
            continue
        dstar = _kde_host_dstar(xb, s, sc)
        acc = np.zeros(xb.shape[0])
        for j0 in range(0, n_s, sc):
            d = xb[:, None] - s[None, j0:j0 + sc]
            acc += np.exp((dstar[:, None] - d * d) * c).sum(axis=1)
        tstar = dstar * c
        if what == "pdf":
            out[i0:i0 + rows] = np.exp(-tstar) * acc / (n_s * h * _SQRT_2PI)
        else:
            out[i0:i0 + rows] = -tstar + np.log(acc) - np.log(n_s * h * _SQRT_2PI)
    return out


def _kde_host_nll(x, s, hb):
    """-> (nll, dnll) over the bandwidths hb: corrla_kde_nll_* restated in numpy (float64), block by block"""
    n_t, n_s = x.shape[0], s.shape[0]
    rows, sc = _kde_host_blocks(n_t, n_s)
    nll, dnll = np.zeros(hb.shape[0]), np.zeros(hb.shape[0])
    for i0 in range(0, n_t, rows):
        xb = x[i0:i0 + rows]
        dstar = _kde_host_dstar(xb, s, sc)
        sk, se = np.zeros((hb.shape[0], xb.shape[0])), np.zeros((hb.shape[0], xb.shape[0]))
        for j0 in range(0, n_s, sc):
            d = xb[:, None] - s[None, j0:j0 + sc]
            a = dstar[:, None] - d * d
            for b, h in enumerate(hb):
                e = a * (1.0 / (2.0 * h * h))
                kk = np.exp(e)
                sk[b] += kk.sum(axis=1)
                se[b] += (e * kk).sum(axis=1)
        for b, h in enumerate(hb):
            tstar = dstar / (2.0 * h * h)
            nll[b] -= (-tstar + np.log(sk[b]) - np.log(n_s * h * _SQRT_2PI)).sum()
            dnll[b] -= ((2.0 * (tstar - se[b] / sk[b]) - 1.0) / h).sum()
    return nll, dnll


class KdeRv:
    """Gaussian kernel density estimate with uniform weights (``KdeRv``, univariate_rv.rs:384-460): ``pdf``, ``cdf``,
    ``logpdf``, ``nll``, ``sample``, and ``est_bandwidth`` by cross-validated likelihood.

    device=True, or whenever a CUDA tensor is involved: the pairwise sums come from ``Context.kde_eval`` / ``kde_nll`` (fused
    kernels, the (n, n_s) matrix is never stored; a CUDA tensor in -> a tensor out).  Otherwise numpy input runs the same
    formulas in numpy on the host, at most 2^21 pairs at a time.  Both use the stabilised sums
    exp(-t*) sum_j exp(-(t_j - t*)) with t* the term of the nearest support: ``logpdf`` and ``nll`` are finite wherever the
    reference's ``pdf(x).ln()`` is -inf (every term underflowed), which is what lets the bandwidth search start at small h.

    ``est_bandwidth`` differs from the reference on purpose.  There ``mlefit`` runs a local optimiser (L-BFGS on forward
    differences, a random particle swarm as fallback) from the initial bandwidth, with a quadratic penalty outside the bounds.
    Here the search is deterministic and global over the bounds, uses only (nll, dnll) evaluations of at most 64 bandwidths
    each with the analytic derivative, and clamps to the bounds: (1) a log-spaced grid over the bounds brackets the grid
    minimum; (2) grids inside the bracket, each keeping the cell where dnll/dh changes sign from - to + (the cells next to
    the grid minimum where it does not), until the bracket is narrower than rtol in ln h; (3) the zero of dnll/dh inside the
    final bracket by linear interpolation in ln h.  At most 12 evaluations; the result always lies inside the bounds.
    `method` is accepted for signature compatibility and ignored."""

    def __init__(self, bandwidth, samples, *, device=False, ctx=None):
        self.bandwidth = float(bandwidth)
        if not (np.isfinite(self.bandwidth) and self.bandwidth > 0.0):
            raise ValueError(f"bandwidth must be finite and > 0, got {bandwidth!r}")
        if _on_gpu(samples):
            import torch
            s = samples.detach().reshape(-1)
            self.supports = s if s.dtype in (torch.float32, torch.float64) else s.double()
        else:
            s = np.asarray(samples.detach().cpu().numpy() if _is_torch(samples) else samples)
            self.supports = np.ascontiguousarray(s.reshape(-1), dtype=np.float32 if s.dtype == np.float32 else np.float64)
        if self.supports.shape[0] == 0:
            raise ValueError("samples must be non-empty")
        self.device, self._ctx = bool(device), ctx

    def _context(self):
        if self._ctx is None:
            self._ctx = default_context()
        return self._ctx

    def _on_device(self, x):
        return self.device or _on_gpu(x) or _on_gpu(self.supports)

    def _device_pair(self, x):
        """x and the supports as ``Context.kde_*`` takes them: the kind of x decides, the dtype of the supports"""
        if _on_gpu(x) or _on_gpu(self.supports):
            import torch
            dev = x.device if _on_gpu(x) else self.supports.device
            dt = torch.float32 if str(self.supports.dtype).endswith("float32") else torch.float64
            xt = x.detach() if _is_torch(x) else torch.as_tensor(np.asarray(x))
            st = self.supports if _is_torch(self.supports) else torch.as_tensor(self.supports)
            return xt.to(device=dev, dtype=dt), st.to(device=dev, dtype=dt), not _on_gpu(x)
        return np.asarray(x.detach().numpy() if _is_torch(x) else x, dtype=self.supports.dtype), self.supports, False

    def _host_pair(self, x):
        return np.asarray(x, dtype=np.float64), np.asarray(self.supports, dtype=np.float64)

    def _eval(self, x, what):
        if self._on_device(x):
            xa, sa, to_host = self._device_pair(x)
            out = self._context().kde_eval(xa, sa, self.bandwidth, what)
            return out.cpu().numpy() if to_host else out
        xa, sa = self._host_pair(x)
        if xa.size == 0:
            raise ValueError("x must be non-empty")
        return _kde_host_eval(xa.reshape(-1), sa, self.bandwidth, what).reshape(xa.shape)

    def pdf(self, x):
        """the density at the points x, in the shape of x"""
        return self._eval(x, "pdf")

    def cdf(self, x):
        """the distribution function at the points x (through erfc)"""
        return self._eval(x, "cdf")

    def logpdf(self, x):
        """the log-density at the points x: finite for every finite x"""
        return self._eval(x, "logpdf")

    def nll_dnll(self, samples, bandwidths):
        """-> (nll, dnll), float64 numpy arrays over `bandwidths` (any number: evaluated 64 at a time)"""
        hb = np.atleast_1d(np.asarray(bandwidths, dtype=np.float64))
        if hb.ndim != 1 or hb.shape[0] == 0 or not (np.all(np.isfinite(hb)) and np.all(hb > 0.0)):
            raise ValueError("bandwidths must be finite and > 0")
        nll, dnll = np.empty(hb.shape[0]), np.empty(hb.shape[0])
        if self._on_device(samples):
            xa, sa, _ = self._device_pair(samples)
        else:
            xa, sa = self._host_pair(samples)
            xa = xa.reshape(-1)
            if xa.size == 0:
                raise ValueError("samples must be non-empty")
        for b0 in range(0, hb.shape[0], _KDE_GRID):
            part = hb[b0:b0 + _KDE_GRID]
            if self._on_device(samples):
                a, b = self._context().kde_nll(xa, sa, part)
                a, b = (a.cpu().numpy(), b.cpu().numpy()) if _is_torch(a) else (a, b)
            else:
                a, b = _kde_host_nll(xa, sa, part)
            nll[b0:b0 + _KDE_GRID], dnll[b0:b0 + _KDE_GRID] = a, b
        return nll, dnll

    def nll(self, samples, bandwidth=None):
        """``UniRv::nll`` (univariate_rv.rs:165-170): -sum_i ln pdf(samples_i), at this estimate's bandwidth or at the given
        one; a sequence of bandwidths gives an array.  Finite for every h > 0."""
        h = self.bandwidth if bandwidth is None else bandwidth
        out = self.nll_dnll(samples, h)[0]
        return float(out[0]) if np.ndim(h) == 0 else out

    def sample(self, n, *, seed=None):
        """n draws: a support picked uniformly plus h N(0, 1) (``KdeRv::sample``, univariate_rv.rs:445-459), on the host from
        ``numpy.random.default_rng(seed)``"""
        rng = np.random.default_rng(seed)
        s = self.supports.cpu().numpy() if _is_torch(self.supports) else self.supports
        return s[rng.integers(0, s.shape[0], int(n))].astype(np.float64) + self.bandwidth * rng.standard_normal(int(n))

    def est_bandwidth(self, test_samples, method=None, *, bounds=(1e-9, 1000.0), rtol=1e-6):
        """The bandwidth that minimises the negative log-likelihood of `test_samples` -- which should not be the supports --
        inside `bounds` (``KdeRv::est_bandwidth``, univariate_rv.rs:406-420); sets ``self.bandwidth`` and returns it.  See the
        class docstring for the search and its differences from the reference.  ``self.n_nll_calls`` counts the likelihood
        evaluations (at most 12, of at most 64 bandwidths each)."""
        lo, hi = float(bounds[0]), float(bounds[1])
        if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo < hi):
            raise ValueError(f"bounds must be finite with 0 < lower < upper, got {bounds!r}")
        rtol = float(rtol)
        if not rtol > 0.0:
            raise ValueError("rtol must be > 0")
        a, b = np.log(lo), np.log(hi)
        self.n_nll_calls = 0
        a_is_lo = b_is_hi = True  # the bracket's ends are still the bounds themselves
        while True:
            grid = np.exp(np.linspace(a, b, _KDE_GRID))
            grid[0], grid[-1] = np.exp(a), np.exp(b)
            nll, dnll = self.nll_dnll(test_samples, grid)
            self.n_nll_calls += 1
            i = int(np.argmin(nll))
            # the cells where the derivative goes from - to +: the one nearest the grid minimum
            cells = np.nonzero((dnll[:-1] < 0.0) & (dnll[1:] >= 0.0))[0]
            if cells.size:
                j = int(cells[np.argmin(np.abs(cells + 0.5 - i))])
                i0, i1 = j, j + 1
            else:
                i0, i1 = max(i - 1, 0), min(i + 1, _KDE_GRID - 1)
            a, b = np.log(grid[i0]), np.log(grid[i1])
            a_is_lo, b_is_hi = a_is_lo and i0 == 0, b_is_hi and i1 == _KDE_GRID - 1
            ga, gb, na, nb = dnll[i0], dnll[i1], nll[i0], nll[i1]
            if b - a <= rtol or self.n_nll_calls >= _KDE_MAX_CALLS:
                break
        if ga < 0.0 <= gb:      # the zero of dnll/dh inside the bracket, linear in ln h
            t = a + (b - a) * (-ga / (gb - ga))
        else:                   # no sign change: the minimum is at an end of the bracket
            t = a if na <= nb else b
        if (t == a and a_is_lo) or (t == b and b_is_hi):
            self.bandwidth = lo if t == a else hi
        else:
            self.bandwidth = float(min(max(np.exp(min(max(t, a), b)), lo), hi))
        return self.bandwidth


def build_kde(init_bandwidth, samples, n_iter, method=None, *, seed=None, device=False, ctx=None):
    """``build_kde`` (univariate_rv.rs:464-497): n_iter random splits of `samples` -- each sample goes to the supports with
    probability 0.7, else to the test set -- one ``est_bandwidth`` per split, and the estimate over ALL samples with the
    element sorted[n_iter // 2] of the per-split bandwidths.  The splits come from ``numpy.random.default_rng(seed)``: the
    same seed gives the same estimate.  The per-split bandwidths are kept, in split order, as ``bandwidth_estimates``."""
    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError("n_iter must be >= 1")
    flat = samples.detach().reshape(-1) if _is_torch(samples) else np.asarray(samples).reshape(-1)
    n = int(flat.shape[0])
    rng = np.random.default_rng(seed)
    ests = []
    for _ in range(n_iter):
        mask = rng.random(n) < 0.7
        if mask.all() or not mask.any():
            raise ValueError("a split left the supports or the test set empty: build_kde needs more samples")
        if _is_torch(flat):
            import torch
            m = torch.from_numpy(mask).to(flat.device)
            sup, test = flat[m], flat[~m]
        else:
            sup, test = flat[mask], flat[~mask]
        ests.append(KdeRv(init_bandwidth, sup, device=device, ctx=ctx).est_bandwidth(test, method))
    out = KdeRv(sorted(ests)[len(ests) // 2], flat, device=device, ctx=ctx)
    out.bandwidth_estimates = np.asarray(ests)
    return out


# ---- constrained Dirichlet sampling (space_samplers.rs, lib_math_utils_py.rs:89-168) -----------------------------------------
def _fresh_seed():
    """a 64-bit seed from the operating system's entropy: repeated calls differ, as with the reference's thread_rng"""
    return int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])


def constr_dirichlet_sample(bounds, n_samples, max_zshots, chunk_size, c_scale, alphas=None, *, seed=None, ctx=None):
    """``constr_dirichlet_sample`` (space_samplers.rs:64-126): n_samples points with sum x = c_scale and
    bounds[j, 0] <= x_j <= bounds[j, 1], by rejection from Dirichlet(alphas) -- None: all ones, one value: symmetric, else d
    values.  The draws are made, tested and counted on the device (``Context.dirichlet_sample``); the (n_samples, d) array
    that comes back holds the first n_samples accepted draws of at most max_zshots shots of chunk_size, and zeros in the rows
    that were not found, as the reference leaves them -- but here a RuntimeWarning says how many were found.  The reference
    splits the request over 10 workers of max_zshots shots each; here it is one stream, reproducible for a seed.  seed=None
    takes a fresh seed."""
    import warnings
    c = ctx or default_context()
    out, n_found, _n_drawn = c.dirichlet_sample(bounds, n_samples, alphas, c_scale=c_scale, seed=_fresh_seed() if seed is None else seed,
                                                max_zshots=max_zshots, chunk_size=chunk_size)
    if n_found < int(n_samples):
        warnings.warn(f"constr_dirichlet_sample found {n_found} of {int(n_samples)} samples in {int(max_zshots)} shots of "
                      f"{int(chunk_size)}: rows [{n_found}, {int(n_samples)}) are zero", RuntimeWarning, stacklevel=2)
    return out


class DeMcSampler:
    """``DeMcSampler`` (space_samplers.rs:252-418) for the target of ``cs_mcmc_dirichlet_sample``: differential-evolution
    Markov chains on the simplex sum x = c_scale inside a box, with the log-density ln Dirichlet(x / c_scale; alphas) plus the
    flat prior of the open box (``LnLikeDirichlet`` + ``LnPriorUniform``).  The chains advance in lock step
    (``sample_mcmc_par``): every proposal of a step is built from the heads at the start of the step.  For chain c
    (``step_chain``): two distinct other chains a, b; the proposal head_c + gamma (head_a - head_b) + e with e uniform in
    [0, var_epsilon)^d; the fix-up x <- c_scale x / sum x (lib_math_utils_py.rs:136-141); accepted with probability
    min(1, exp(lnp(proposal) - lnp(head_c))) (``accept_prob_ratio``, ``metropolis_accept``).  There is no hot path in this:
    it is numpy, vectorised over the chains, on ``numpy.random.Generator(Philox(seed))``.
    Deliberate differences from the reference: the dimension is that of the seeds (``McmcChain::new(3, ...)`` is hard-coded
    there); the likelihood is evaluated on x / c_scale (there it asserts sum x = 1 and panics for any other c_scale); the
    log-density is formed in logs, sum (alpha_j - 1) ln x_j - ln B(alpha), not as ln of a product that underflows, and a
    proposal with a component <= 0 has log-density -inf and is rejected.  At least 3 chains, as the reference asserts."""

    def __init__(self, bounds, seeds, alphas, gamma, var_epsilon, *, c_scale=1.0, seed=None):
        import math
        self.heads = np.array(seeds, dtype=np.float64)
        if self.heads.ndim != 2:
            raise ValueError(f"seeds must be (n_chains, d), got shape {tuple(self.heads.shape)}")
        self.n_chains, self.ndim = self.heads.shape
        if self.n_chains < 3:
            raise ValueError(f"at least 3 chains are needed, got {self.n_chains}")
        self.bounds = np.asarray(bounds, dtype=np.float64)
        if self.bounds.shape != (self.ndim, 2):
            raise ValueError(f"bounds must be ({self.ndim}, 2), got shape {tuple(self.bounds.shape)}")
        self.alphas = np.broadcast_to(np.asarray(alphas, dtype=np.float64), (self.ndim,)).copy()
        self.gamma, self.var_epsilon, self.c_scale = float(gamma), float(var_epsilon), float(c_scale)
        self._ln_beta = sum(math.lgamma(a) for a in self.alphas) - math.lgamma(float(self.alphas.sum()))
        self._rng = np.random.Generator(np.random.Philox(_fresh_seed() if seed is None else seed))
        self._history = [self.heads.copy()]
        self.n_accept = self.n_reject = 0

    def ln_prob(self, x):
        """(n, d) -> (n,): the Dirichlet log-density of x / c_scale plus 0 inside the open box, -inf outside"""
        inside = np.all((self.bounds[:, 0] < x) & (x < self.bounds[:, 1]), axis=1) & np.all(x > 0.0, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            like = np.sum((self.alphas - 1.0) * np.log(x / self.c_scale), axis=1) - self._ln_beta
        return np.where(inside, like, -np.inf)

    def _step(self):
        n, cur = self.n_chains, self.heads
        me = np.arange(n)
        r1, r2 = self._rng.integers(0, n - 1, size=n), self._rng.integers(0, n - 2, size=n)
        r2 = r2 + (r2 >= r1)                    # two distinct places among the n - 1 other chains ...
        a, b = r1 + (r1 >= me), r2 + (r2 >= me)  # ... as chain numbers
        prop = cur + self.gamma * (cur[a] - cur[b]) + self._rng.uniform(0.0, self.var_epsilon, size=cur.shape)
        prop = self.c_scale * prop / prop.sum(axis=1, keepdims=True)
        lp, lc = self.ln_prob(prop), self.ln_prob(cur)
        with np.errstate(invalid="ignore", over="ignore"):
            ratio = np.where(np.isneginf(lp), 0.0, np.minimum(np.exp(lp - lc), 1.0))
        accept = self._rng.random(n) < ratio
        self.heads = np.where(accept[:, None], prop, cur)
        self.n_accept += int(accept.sum())
        self.n_reject += int(n - accept.sum())
        self._history.append(self.heads.copy())

    def sample_mcmc(self, n_samples):
        for _ in range(int(n_samples)):
            self._step()

    def accept_ratio(self):
        return self.n_accept / float(self.n_accept + self.n_reject)

    def get_samples(self, n_tail):
        """the last n_tail heads of every chain, interleaved chain-fastest: (n_tail * n_chains, d)"""
        n_tail = int(n_tail)
        if not 1 <= n_tail <= len(self._history):
            raise ValueError(f"n_tail must be in [1, {len(self._history)}], got {n_tail}")
        return np.concatenate(self._history[-n_tail:], axis=0)


def cs_mcmc_dirichlet_sample(bounds, n_samples, n_seed_samples, max_zshots, chunk_size, c_scale, alphas, gamma, var_epsilon, *,
                             seed=None, ctx=None):
    """``cs_mcmc_dirichlet_sample`` (lib_math_utils_py.rs:107-168) -> (samples, accept_ratio): n_seed_samples seeds from
    ``constr_dirichlet_sample`` (on the device, with `alphas`), one chain of a ``DeMcSampler`` per seed with the target
    Dirichlet(1, ..., 1) -- uniform on the simplex, inside the box -- advanced n_samples steps; samples are the last n_samples
    heads of every chain, chain-fastest: (n_samples * n_seed_samples, d).  See ``DeMcSampler`` for the differences from the
    reference.  A seed that was not found would start a chain outside the box: RuntimeError instead of the reference's rows
    of zeros.  seed=None takes a fresh seed; one seed fixes both stages."""
    import warnings
    if int(n_seed_samples) < 3:
        raise ValueError(f"at least 3 chains (n_seed_samples) are needed, got {int(n_seed_samples)}")
    seed = _fresh_seed() if seed is None else int(seed)
    c = ctx or default_context()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        seeds, n_found, _ = c.dirichlet_sample(bounds, n_seed_samples, alphas, c_scale=c_scale, seed=seed, max_zshots=max_zshots,
                                               chunk_size=chunk_size)
    if n_found < int(n_seed_samples):
        raise RuntimeError(f"only {n_found} of {int(n_seed_samples)} seed samples were found in {int(max_zshots)} shots of {int(chunk_size)}")
    sampler = DeMcSampler(bounds, seeds, np.ones(seeds.shape[1]), gamma, var_epsilon, c_scale=c_scale, seed=seed)
    sampler.sample_mcmc(n_samples)
    return sampler.get_samples(n_samples), sampler.accept_ratio()


# ---- multivariate normal samples and sandwich variances (stats_corr.rs:46-68) ----------------------------------------------
def _mvn_eig_factor(c, d, big):
    """step 3 of ``mvn_factor`` on the host: c is the symmetrised (d, d) numpy matrix, big its largest magnitude"""
    w, v = np.linalg.eigh(c)
    cut = d * 2.0 ** -52 * max(float(w[-1]), 0.0)
    if float(w[0]) < -cut or float(w[-1]) <= 0.0 and big > 0.0:
        raise ValueError(f"cov is not positive semi-definite: smallest eigenvalue {float(w[0]):.3e}")
    keep = w > cut
    if not np.any(keep):  # the zero matrix: one column of zeros, so that r >= 1
        return np.zeros((d, 1)), False
    return v[:, keep] * np.sqrt(w[keep])[None, :], False


def _mvn_eig_factor_device(c, d, big, ctx):
    """step 3 of ``mvn_factor`` on the device: ``Context.eigh`` of the symmetrised (d, d) tensor c, the test and the cut of
    ``_mvn_eig_factor``; two eigenvalues are read back, the matrix is not"""
    import torch
    w, v = ctx.eigh(c)
    w0, w1 = float(w[0]), float(w[-1])
    cut = d * 2.0 ** -52 * max(w1, 0.0)
    if w0 < -cut or w1 <= 0.0 and big > 0.0:
        raise ValueError(f"cov is not positive semi-definite: smallest eigenvalue {w0:.3e}")
    keep = w > cut
    if not bool(keep.any()):  # the zero matrix: one column of zeros, so that r >= 1
        return torch.zeros((d, 1), dtype=torch.float64, device=c.device), False
    return v[:, keep] * torch.sqrt(w[keep])[None, :], False


def _mvn_factor_device(cov, ctx, eig="host"):
    """``mvn_factor`` with steps 1 and 2 -- and with eig="device" step 3 -- on the device; -> (F tensor, lower)"""
    import torch
    from ._lib import ENUMERIC, CorrlaError
    ctx = ctx or default_context()
    if _on_gpu(cov):
        c = cov.detach().to(torch.float64)
    else:
        c = torch.tensor(np.asarray(cov.detach().numpy() if _is_torch(cov) else cov, dtype=np.float64), device=f"cuda:{ctx.device}")
    if c.ndim != 2 or c.shape[0] != c.shape[1] or c.shape[0] == 0:
        raise ValueError(f"cov must be a non-empty square matrix, got shape {tuple(c.shape)}")
    if not bool(torch.isfinite(c).all()):
        raise ValueError("cov must be finite")
    d = int(c.shape[0])
    big = float(c.abs().max())
    if float((c - c.T).abs().max()) > 8.0 * 2.0 ** -52 * big:
        raise ValueError("cov is not symmetric")
    c = 0.5 * (c + c.T)
    sd = torch.sqrt(torch.diagonal(c).clamp(min=0.0))
    sd = torch.where(sd > 0.0, sd, torch.ones_like(sd))
    try:
        lo = ctx.cholesky(c / torch.outer(sd, sd), overwrite=True).tril_()  # in place: the quotient is a temporary of this call
        return sd[:, None] * lo, True
    except CorrlaError as e:
        if e.code != ENUMERIC:
            raise
    if eig == "device":
        return _mvn_eig_factor_device(c, d, big, ctx)
    f, lower = _mvn_eig_factor(c.cpu().numpy(), d, big)  # the one route that reads the matrix back
    return torch.as_tensor(f, device=c.device), lower


def mvn_factor(cov, *, device=False, ctx=None, eig="host"):
    """A factor F of a covariance matrix, F F^T = cov -> (F, lower), on the host in float64 (d-sized work).
      1. cov must be square and symmetric to 8 * 2^-52 * max|cov|, else ValueError;
      2. the Cholesky factor of the diagonally equilibrated matrix D^-1/2 cov D^-1/2 is tried: (D^1/2 L, True);
      3. otherwise the symmetric eigendecomposition: an eigenvalue below -d 2^-52 lambda_max is a ValueError (the matrix is
         indefinite); directions with lambda <= d 2^-52 lambda_max are dropped -- the rule of ``polyfit_solve`` -- and the rest
         gives (V sqrt(Lambda), False) with r < d columns.
    So a singular covariance (fewer samples than features, or the output of ``sandwich_prop``) can be sampled from.
    device=True: steps 1 and 2 -- the symmetry check, the equilibration, the Cholesky factorisation (``Context.cholesky`` of
    `ctx` or the default context) and the rescaling -- run on the device in float64 and F is a CUDA tensor; a CUDA `cov`
    never visits the host.  Only when the factorisation reports a pivot that is not positive does the matrix come back for
    step 3, whose F is uploaded again.  The device factor agrees with the host's within rounding, not bit for bit.
    eig="device" (with device=True): step 3 runs on the device as well -- ``Context.eigh``, the same test and the same cut --
    and a CUDA `cov` never visits the host on any branch.  Its eigenvalues carry absolute errors of order d u |cov|_F."""
    if eig not in ("host", "device"):
        raise ValueError("eig must be 'host' or 'device'")
    if eig == "device" and not device:
        raise ValueError("eig='device' needs device=True")
    if device:
        return _mvn_factor_device(cov, ctx, eig)
    c = np.asarray(cov.detach().cpu().numpy() if _is_torch(cov) else cov, dtype=np.float64)
    if c.ndim != 2 or c.shape[0] != c.shape[1] or c.shape[0] == 0:
        raise ValueError(f"cov must be a non-empty square matrix, got shape {tuple(c.shape)}")
    if not np.all(np.isfinite(c)):
        raise ValueError("cov must be finite")
    d = int(c.shape[0])
    big = float(np.max(np.abs(c)))
    if float(np.max(np.abs(c - c.T))) > 8.0 * 2.0 ** -52 * big:
        raise ValueError("cov is not symmetric")
    c = 0.5 * (c + c.T)
    sd = np.sqrt(np.diag(c).clip(min=0.0))
    sd = np.where(sd > 0.0, sd, 1.0)
    try:
        return sd[:, None] * np.linalg.cholesky(c / np.outer(sd, sd)), True
    except np.linalg.LinAlgError:
        pass
    w, v = np.linalg.eigh(c)
    cut = d * 2.0 ** -52 * max(float(w[-1]), 0.0)
    if float(w[0]) < -cut or float(w[-1]) <= 0.0 and big > 0.0:
        raise ValueError(f"cov is not positive semi-definite: smallest eigenvalue {float(w[0]):.3e}")
    keep = w > cut
    if not np.any(keep):  # the zero matrix: one column of zeros, so that r >= 1
        return np.zeros((d, 1)), False
    return v[:, keep] * np.sqrt(w[keep])[None, :], False


def sample_mv_normal(cov, n, *, mean=None, seed=None, device=False, ctx=None, factor="host", eig="host"):
    """``sample_mv_normal(cov, n)`` (stats_corr.rs:46-58): n rows of N(mean, cov), (n, d) float64.  The covariance is factored
    on the host (``mvn_factor``), the rows come from ``Context.mvn_sample``.  numpy in -> numpy out; a CUDA cov or device=True
    gives a tensor.  seed=None takes a fresh one from ``numpy.random.SeedSequence``.
    The one deliberate difference from the reference: it multiplies z by cov itself, so its samples have covariance cov^2;
    these have covariance cov.  ``Context.mvn_sample(n, cov)`` (factor = cov) reproduces the reference's law.
    factor="device" factors the covariance on the device instead (``mvn_factor(cov, device=True)``): nothing d x d is computed
    on the host; the rows are ``Context.mvn_sample(n, F, lower=True)`` of that F, in the kind the default returns.
    eig="device" (with factor="device") factors a singular covariance on the device too (``mvn_factor(eig="device")``)."""
    if factor not in ("host", "device"):
        raise ValueError("factor must be 'host' or 'device'")
    if eig not in ("host", "device") or (eig == "device" and factor != "device"):
        raise ValueError("eig must be 'host' or 'device', and 'device' needs factor='device'")
    if factor == "device":
        c = ctx or default_context()
        f, lower = mvn_factor(cov, device=True, ctx=c, eig=eig)
        mu = None if mean is None else np.asarray(mean.detach().cpu().numpy() if _is_torch(mean) else mean, dtype=np.float64).reshape(-1)
        out = c.mvn_sample(n, f, mu, seed=_fresh_seed() if seed is None else seed, lower=lower, device=True)
        return out if bool(device) or _on_gpu(cov) else out.cpu().numpy()
    f, lower = mvn_factor(cov)
    mu = None if mean is None else np.asarray(mean.detach().cpu().numpy() if _is_torch(mean) else mean, dtype=np.float64).reshape(-1)
    return (ctx or default_context()).mvn_sample(n, f, mu, seed=_fresh_seed() if seed is None else seed, lower=lower,
                                                 device=bool(device) or _on_gpu(cov))


def sandwich_prop(cov, jac, *, diag=False, ctx=None):
    """``sandwich_prop(cov, jac)`` (stats_corr.rs:64-68): jac @ cov @ jac.T, outputs x outputs -- plain numpy or torch, it is
    tiny.  diag=True: jac holds one gradient per SAMPLE (m, d) and only the m first-order variances jac[i] @ cov @ jac[i]
    are wanted: ``Context.sandwich_diag``, without the (m, m) product or an (m, d) temporary."""
    if diag:
        c = ctx or default_context()
        if _is_torch(jac) and not _is_torch(cov):
            import torch
            cov = torch.as_tensor(np.asarray(cov), dtype=jac.dtype, device=jac.device)
        elif not _is_torch(jac):
            jac = np.asarray(jac)
            jac = jac if jac.dtype == np.float32 else jac.astype(np.float64, copy=False)
            cov = np.asarray(cov.detach().cpu().numpy() if _is_torch(cov) else cov, dtype=jac.dtype)
        else:
            cov = cov.to(device=jac.device, dtype=jac.dtype)
        return c.sandwich_diag(jac, cov)
    if _is_torch(jac) or _is_torch(cov):
        import torch
        j = jac if _is_torch(jac) else torch.as_tensor(np.asarray(jac), dtype=cov.dtype, device=cov.device)
        cv = cov if _is_torch(cov) else torch.as_tensor(np.asarray(cov), dtype=j.dtype, device=j.device)
        return j @ cv.to(device=j.device, dtype=j.dtype) @ j.T
    j = np.asarray(jac, dtype=np.float64)
    return j @ np.asarray(cov, dtype=np.float64) @ j.T
