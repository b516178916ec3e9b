"""ctypes binding of libcorrla_rsvd.so (include/corrla_rsvd.h).  There is no fallback: if the
HIP library is missing or cannot be loaded, importing the compute API raises."""
import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
# CORRLA_RSVD_LIB: another build of the same library (kernel A/B measurements)
LIB_PATH = os.environ.get("CORRLA_RSVD_LIB") or os.path.join(PKG, "lib", "libcorrla_rsvd.so")

i64, u64, u32, i32, dbl, flt = C.c_int64, C.c_uint64, C.c_uint32, C.c_int32, C.c_double, C.c_float
vp = C.c_void_p

OK, EINVAL, ENOMEM, EHIP, ECOMM, ENUMERIC, ENODEV = range(7)
OMEGA_ON_DEVICE = 0x1
PCA_CENTER_FUSED = 0x2
PCA_CENTER_COPY = 0x4
QR_HOUSEHOLDER = 0x8
SEED_EXPLICIT = 0x10
POWER_FUSED = 0x20
SHARD_COLS = 0x40
SKETCH_BF16X3 = 0x80
SKETCH_BF16X6 = 0x100
PCA_STANDARDIZE = 0x200
# corrla_cov_*: the entry's own flag word and the routes it reports
COV_CORRELATION = 0x1
COV_NO_CENTER = 0x2
COV_ROUTE_INPLACE, COV_ROUTE_INPLACE_CHECKED, COV_ROUTE_REPACKED = 1, 2, 3
COV_ROUTES = {COV_ROUTE_INPLACE: "inplace", COV_ROUTE_INPLACE_CHECKED: "inplace_checked", COV_ROUTE_REPACKED: "repacked"}
# corrla_pca_transform_*: the entry's own flag word (the centre flags keep their corrla_opts values) and what
# corrla_ctx_last_pca_apply reports
PCA_APPLY_OWN_MEANS = 0x400
PCA_APPLY_ROUTE_INPLACE, PCA_APPLY_ROUTE_INPLACE_CHECKED, PCA_APPLY_ROUTE_REPACKED = 1, 2, 3
PCA_APPLY_ROUTES = {PCA_APPLY_ROUTE_INPLACE: "inplace", PCA_APPLY_ROUTE_INPLACE_CHECKED: "inplace_checked",
                    PCA_APPLY_ROUTE_REPACKED: "repacked"}
PCA_APPLY_CENTRINGS = {1: "fused", 2: "copy"}
# corrla_polyfit_gram_* / corrla_poly_eval_*: what corrla_ctx_last_polyfit reports
POLYFIT_ROUTES = {1: "inplace", 2: "inplace_checked"}
# corrla_kde_eval_* / corrla_kde_nll_*: what corrla_ctx_last_kde reports, and the `what` of the eval entries
KDE_ROUTES = {1: "single", 2: "split"}
KDE_WHAT = {"pdf": 0, "cdf": 1, "logpdf": 2}
KDE_MAX_BANDWIDTHS = 64
# corrla_dirichlet_draws_* / corrla_dirichlet_sample_*: the low byte of what corrla_ctx_last_dirichlet reports, and the limits
DIRICHLET_ROUTES = {1: "registers/exponential", 2: "registers/general", 3: "regenerate/exponential", 4: "regenerate/general"}
DIRICHLET_MAX_D = 128
DIRICHLET_MAX_DRAWS = 1 << 62
# corrla_mvn_sample_* / corrla_sandwich_diag_*: what corrla_ctx_last_mvn reports, and the limits
MVN_ROUTES = {1: "fused", 2: "staged", 3: "empty"}
MVN_MAX_D = 65536
SANDWICH_MAX_D = 512
# corrla_lu_solve_* / corrla_rbffit_*: what corrla_ctx_last_solve reports, and the limits
SOLVE_ROUTES = {1: "small", 2: "blocked"}
LU_SMALL_N = 128
LU_NB = 64
LU_MAX_N = 1 << 17
# corrla_chol_factor_* / corrla_chol_solve_*: what corrla_ctx_last_chol reports, and the limits
CHOL_ROUTES = {1: "small", 2: "blocked"}
CHOL_SMALL_N = 128
CHOL_NB = 64
CHOL_MAX_N = 1 << 17
# corrla_eigh_*: what corrla_ctx_last_eigh reports, and the limits
EIGH_ROUTES = {1: "small", 2: "blocked"}
EIGH_SMALL_N = 64
EIGH_B = 32
EIGH_MAX_N = 1 << 15
EIGH_MAX_SWEEPS = 40
UNIQUE_ID_BYTES = 128


class Opts(C.Structure):
    _fields_ = [("struct_size", u32), ("flags", u32), ("seed", u64), ("omega", vp), ("omega_ld", i64),
                ("scales_out", vp)]


class Timings(C.Structure):
    _fields_ = [("total_ms", dbl), ("sketch_ms", dbl), ("power_ms", dbl), ("qr_ms", dbl), ("project_ms", dbl),
                ("small_svd_ms", dbl), ("finalize_ms", dbl), ("qr_passes", i32), ("n_collectives", i32),
                ("sketch_kernel_ms", dbl), ("host_enqueue_ms", dbl), ("collective_bytes", dbl), ("n_mixed_products", i32),
                ("n_bf16_products", i32), ("knn_ms", dbl), ("fit_ms", dbl)]


# symbol -> (restype, argtypes); this table is also what tests/test_abi.py checks against the header
def _sigs():
    s = {
        "corrla_version": (C.c_char_p, []),
        "corrla_last_error": (C.c_char_p, []),
        "corrla_device_count": (C.c_int, []),
        "corrla_ctx_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "corrla_ctx_destroy": (None, [vp]),
        "corrla_ctx_synchronize": (C.c_int, [vp]),
        "corrla_ctx_get_timings": (C.c_int, [vp, C.POINTER(Timings)]),
        "corrla_ctx_set_phase_timings": (C.c_int, [vp, C.c_int]),
        "corrla_ctx_comm_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "corrla_comm_unique_id": (C.c_int, [vp]),
        "corrla_ctx_comm_init": (C.c_int, [vp, vp, C.c_int, C.c_int]),
        "corrla_ctx_last_pca_apply": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "corrla_ctx_last_polyfit": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "corrla_ctx_last_kde": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "corrla_ctx_last_dirichlet": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "corrla_ctx_last_mvn": (C.c_int, [vp, C.POINTER(C.c_int)]),
    }
    # constrained Dirichlet sampling, f64 only: alphas, d, c_scale, seed, first, n, out, ldo / bounds, alphas, d, c_scale, seed,
    # n_samples, max_zshots, chunk_size, out, ldo, n_found, n_drawn
    s["corrla_dirichlet_draws_f64"] = s["corrla_dirichlet_draws_dev_f64"] = (C.c_int, [vp, vp, i64, dbl, u64, i64, i64, vp, i64])
    s["corrla_dirichlet_sample_f64"] = s["corrla_dirichlet_sample_dev_f64"] = (
        C.c_int, [vp, vp, vp, i64, dbl, u64, i64, i64, i64, vp, i64, C.POINTER(i64), C.POINTER(i64)])
    # dense LU solve, f64 only, row-major: a, n, lda, b, n_rhs, ldb, then x, ldx (host) / ipiv (device, in place)
    s["corrla_lu_solve_f64"] = (C.c_int, [vp, vp, i64, i64, vp, i64, i64, vp, i64])
    s["corrla_lu_solve_dev_f64"] = (C.c_int, [vp, vp, i64, i64, vp, i64, i64, vp])
    # the RBF system and fit: xs, n_s, ldxs, dim, [y, n_rhs, ldy,] kernel, eps, poly_degree, m | coeffs, ld
    s["corrla_rbffit_system_f64"] = s["corrla_rbffit_system_dev_f64"] = (C.c_int, [vp, vp, i64, i64, i64, C.c_int, dbl, C.c_int, vp, i64])
    s["corrla_rbffit_f64"] = s["corrla_rbffit_dev_f64"] = (C.c_int, [vp, vp, i64, i64, i64, vp, i64, i64, C.c_int, dbl, C.c_int, vp, i64])
    s["corrla_ctx_last_solve"] = (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(i64), C.POINTER(dbl), C.POINTER(dbl)])
    # dense Cholesky factor and SPD solve, f64 only, row-major, lower triangle: a, n, lda, then l, ldl (host factor) / nothing
    # (device factor, in place); a, n, lda, b, n_rhs, ldb, then x, ldx (host solve) / nothing (device solve, in place)
    s["corrla_chol_factor_f64"] = (C.c_int, [vp, vp, i64, i64, vp, i64])
    s["corrla_chol_factor_dev_f64"] = (C.c_int, [vp, vp, i64, i64])
    s["corrla_chol_solve_f64"] = (C.c_int, [vp, vp, i64, i64, vp, i64, i64, vp, i64])
    s["corrla_chol_solve_dev_f64"] = (C.c_int, [vp, vp, i64, i64, vp, i64, i64])
    s["corrla_ctx_last_chol"] = (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(i64), C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl)])
    # symmetric eigendecomposition, f64 only, row-major, lower triangle: a, n, lda, w, v, ldv (host and device alike)
    s["corrla_eigh_f64"] = s["corrla_eigh_dev_f64"] = (C.c_int, [vp, vp, i64, i64, vp, vp, i64])
    s["corrla_ctx_last_eigh"] = (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(dbl), C.POINTER(dbl), C.POINTER(i64)])
    for suf, sc in (("f32", flt), ("f64", dbl)):
        rsvd = [vp, vp, i64, i64, i64, i64, i64, i64, i64, C.POINTER(Opts), vp, i64, vp, vp, i64]
        s["corrla_rsvd_" + suf] = (C.c_int, rsvd)
        s["corrla_rsvd_dev_" + suf] = (C.c_int, rsvd)
        s["corrla_rsvd_sharded_dev_" + suf] = (C.c_int, rsvd)
        pca = [vp, vp, i64, i64, i64, i64, i64, i64, i64, C.POINTER(Opts), vp, vp, vp, i64]
        s["corrla_pca_" + suf] = (C.c_int, pca)
        s["corrla_pca_dev_" + suf] = (C.c_int, pca)
        s["corrla_pca_sharded_dev_" + suf] = (C.c_int, pca)
        pw = [vp, vp, i64, i64, i64, i64, i64, i64, C.POINTER(Opts), vp, i64]
        s["corrla_power_iter_" + suf] = (C.c_int, pw)
        s["corrla_power_iter_dev_" + suf] = (C.c_int, pw)
        s["corrla_matmul_dev_" + suf] = (C.c_int, [vp, C.c_int, vp, i64, i64, i64, i64, vp, i64, i64, sc, vp, i64])
        # CSR input: values, int32 col_idx, int64 row_ptr, m, n, nnz in place of (a, m, n, rs, cs)
        rsvd_csr = [vp, vp, vp, vp, i64, i64, i64, i64, i64, i64, C.POINTER(Opts), vp, i64, vp, vp, i64]
        s["corrla_rsvd_csr_" + suf] = (C.c_int, rsvd_csr)
        s["corrla_rsvd_csr_dev_" + suf] = (C.c_int, rsvd_csr)
        pca_csr = [vp, vp, vp, vp, i64, i64, i64, i64, i64, i64, C.POINTER(Opts), vp, vp, vp, i64]
        s["corrla_pca_csr_" + suf] = (C.c_int, pca_csr)
        s["corrla_pca_csr_dev_" + suf] = (C.c_int, pca_csr)
        s["corrla_spmm_csr_dev_" + suf] = (C.c_int, [vp, C.c_int, vp, vp, vp, i64, i64, i64, vp, i64, i64, sc, vp, i64])
        cov = [vp, vp, i64, i64, i64, i64, u64, C.c_int, vp, vp, vp, i64, C.POINTER(C.c_int)]
        s["corrla_cov_" + suf] = (C.c_int, cov)
        s["corrla_cov_dev_" + suf] = (C.c_int, cov)
        # fitted PCA model: (x | CSR operand), means, scales, components, ldc, k, flags, scores, ld_scores, resid_out, means_out
        model = [vp, vp, vp, i64, i64, u64, vp, i64, vp, vp]
        s["corrla_pca_transform_" + suf] = s["corrla_pca_transform_dev_" + suf] = (C.c_int, [vp, vp, i64, i64, i64, i64] + model)
        s["corrla_pca_transform_csr_" + suf] = s["corrla_pca_transform_csr_dev_" + suf] = (C.c_int, [vp, vp, vp, vp, i64, i64, i64] + model)
        inverse = [vp, vp, i64, i64, i64, vp, vp, vp, i64, i64, vp, i64]
        s["corrla_pca_inverse_" + suf] = s["corrla_pca_inverse_dev_" + suf] = (C.c_int, inverse)
        # RBF kernel matrices: xq, n_q, ldq, xs, n_s, lds, dim, kernel, eps [, poly_degree, coeffs, ldw, n_rhs], out, ld_out
        points = [vp, vp, i64, i64, vp, i64, i64, i64, C.c_int, dbl]
        s["corrla_rbf_matrix_" + suf] = s["corrla_rbf_matrix_dev_" + suf] = (C.c_int, points + [vp, i64])
        s["corrla_rbf_apply_" + suf] = s["corrla_rbf_apply_dev_" + suf] = (C.c_int, points + [C.c_int, vp, i64, i64, vp, i64])
        # polynomial response surfaces: x, m, k, ldx, y, r, ldy, degree, normalize, G, ldg, means, scales /
        # x, m, k, ldx, coeffs, ldc, r, degree, out, ld_out, jac, ld_jac
        gram = [vp, vp, i64, i64, i64, vp, i64, i64, C.c_int, C.c_int, vp, i64, vp, vp]
        s["corrla_polyfit_gram_" + suf] = s["corrla_polyfit_gram_dev_" + suf] = (C.c_int, gram)
        peval = [vp, vp, i64, i64, i64, vp, i64, i64, C.c_int, vp, i64, vp, i64]
        s["corrla_poly_eval_" + suf] = s["corrla_poly_eval_dev_" + suf] = (C.c_int, peval)
        # kernel density estimates: x, n, incx, s, n_s, incs, then h, what, out, inco / h (host), n_h, nll, dnll
        kde = [vp, vp, i64, i64, vp, i64, i64]
        s["corrla_kde_eval_" + suf] = s["corrla_kde_eval_dev_" + suf] = (C.c_int, kde + [dbl, C.c_int, vp, i64])
        s["corrla_kde_nll_" + suf] = s["corrla_kde_nll_dev_" + suf] = (C.c_int, kde + [vp, i64, vp, vp])
        # multivariate normal rows: n, d, r, factor, ldf, mean, seed, first, lower, out, ldo / sandwich: jac, m, d, ldj, cov, ldc, v
        s["corrla_mvn_sample_" + suf] = s["corrla_mvn_sample_dev_" + suf] = (C.c_int, [vp, i64, i64, i64, vp, i64, vp, u64, i64, C.c_int, vp, i64])
        s["corrla_sandwich_diag_" + suf] = s["corrla_sandwich_diag_dev_" + suf] = (C.c_int, [vp, vp, i64, i64, i64, vp, i64, vp])
        s["corrla_fill_normal_dev_" + suf] =(C.c_int, [vp, vp, i64, i64, i64, i64, u64, i64, i64])
        s["corrla_time_sketch_dev_" + suf] = (C.c_int, [vp, vp, i64, i64, i64, i64, vp, i64, i64, vp, i64, C.c_int,
                                                         C.POINTER(dbl)])
    # dense bf16 input: A is uint16 bit patterns, every other array f32; argument lists of the f32 twins
    s["corrla_rsvd_bf16"] = s["corrla_rsvd_dev_bf16"] = s["corrla_rsvd_f32"]
    s["corrla_pca_bf16"] = s["corrla_pca_dev_bf16"] = s["corrla_pca_f32"]
    s["corrla_matmul_dev_bf16"] = s["corrla_matmul_dev_f32"]
    grad = [vp, vp, i64, i64, vp, vp, i64, C.c_int, i64, dbl, vp, i64, C.POINTER(C.c_int)]
    s["corrla_grad_mat_f64"] = (C.c_int, grad)
    s["corrla_grad_mat_dev_f64"] = (C.c_int, grad)
    return s


SIGNATURES = _sigs()
_lib = None


class CorrlaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"corrla_rsvd error {code}: {msg}")
        self.code = code


def load():
    """Load the HIP library.  Raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m corrla_rs_amd.build` (hipcc, gfx950). "
            "corrla_rs_amd has no CPU fallback.")
    # torch wheels bundle their own ROCm runtime (libamdhip64 / libhsa-runtime64 / librccl, same SONAMEs as
    # /opt/rocm).  One process must use ONE of them: when torch is installed, import it first so this
    # library binds to the copies torch already loaded (device pointers and RCCL are then shared with
    # torch.distributed); RTLD_GLOBAL keeps the reverse order working when torch is absent at load time.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the header and the library drift apart
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code):
    if code != OK:
        msg = load().corrla_last_error().decode("utf-8", "replace")
        if code == EINVAL:
            raise ValueError(f"corrla_rsvd: {msg}")
        if code == ENOMEM:
            raise MemoryError(f"corrla_rsvd: {msg}")
        raise CorrlaError(code, msg)
