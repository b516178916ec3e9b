//! `extern "C"` binding of include/corrla_rsvd.h plus wrappers that keep the reference's public signatures
//! (wgurecky/CORRLA_RS @ 2024_10_08):
//!
//!   pub fn random_svd<T>(a_mat: MatRef<T>, omega_rank: usize, n_iter: usize, n_oversamples: usize)
//!       -> (Mat<T>, Mat<T>, Mat<T>)                              src/lib_math_utils/random_svd.rs:63-66
//!   pub fn power_iter<T>(a_mat: MatRef<T>, omega_rank: usize, n_iter: usize) -> Mat<T>      random_svd.rs:15-18
//!
//! The `MatRef` is forwarded as (ptr, nrows, ncols, row_stride, col_stride) -- no copy, any strides, exactly the view
//! the pyo3 layer builds from a numpy array (src/lib_math_utils_py.rs:27-28).  The three results are freshly owned
//! column-major `Mat`s like the reference's (random_svd.rs:96-109); S is the k x 1 column.  A non-zero status panics
//! with the library's message, which is what the reference's unwrap()/slice panics do (random_svd.rs:98-107).
//!
//! NOT compiled here (no Rust toolchain in the build image); the C side of every prototype below is checked against
//! the header by tests/test_abi.py through the ctypes table, which this file mirrors one to one.
use faer::{Mat, MatRef};
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct CorrlaOpts {
    pub struct_size: u32,
    pub flags: u32,
    pub seed: u64,
    pub omega: *const c_void,
    pub omega_ld: i64,
    pub scales_out: *mut c_void, // written only with CORRLA_PCA_STANDARDIZE: n_dim column standard deviations (nullable)
}
pub const CORRLA_OMEGA_ON_DEVICE: u32 = 0x1;
pub const CORRLA_PCA_CENTER_FUSED: u32 = 0x2;
pub const CORRLA_PCA_CENTER_COPY: u32 = 0x4;
pub const CORRLA_QR_HOUSEHOLDER: u32 = 0x8;
pub const CORRLA_SEED_EXPLICIT: u32 = 0x10;
pub const CORRLA_POWER_FUSED: u32 = 0x20;
pub const CORRLA_SHARD_COLS: u32 = 0x40;
pub const CORRLA_SKETCH_BF16X3: u32 = 0x80; // opt-in: range finder on the bf16-split kernels (f32 inputs only)
pub const CORRLA_SKETCH_BF16X6: u32 = 0x100;
pub const CORRLA_PCA_STANDARDIZE: u32 = 0x200; // corrla_pca_* only: PCA on standardised columns (correlation PCA)
// corrla_cov_*: the entry's own 64-bit flag word and the routes it reports through route_out
pub const CORRLA_COV_CORRELATION: u64 = 0x1;
pub const CORRLA_COV_NO_CENTER: u64 = 0x2;
pub const CORRLA_COV_ROUTE_INPLACE: c_int = 1;
pub const CORRLA_COV_ROUTE_INPLACE_CHECKED: c_int = 2;
pub const CORRLA_COV_ROUTE_REPACKED: c_int = 3;
// corrla_pca_transform_*: the entry's own 64-bit flag word takes CORRLA_PCA_CENTER_FUSED / _COPY (values above) and
pub const CORRLA_PCA_APPLY_OWN_MEANS: u64 = 0x400; // centre the target by its own column means (pca_rsvd.rs:43-46)
pub const CORRLA_PCA_APPLY_ROUTE_INPLACE: c_int = 1;
pub const CORRLA_PCA_APPLY_ROUTE_INPLACE_CHECKED: c_int = 2;
pub const CORRLA_PCA_APPLY_ROUTE_REPACKED: c_int = 3;

extern "C" {
    fn corrla_ctx_create(device: c_int, out: *mut *mut c_void) -> c_int;
    fn corrla_ctx_destroy(ctx: *mut c_void);
    fn corrla_last_error() -> *const c_char;
    fn corrla_rsvd_f64(ctx: *mut c_void, a: *const f64, m: i64, n: i64, rs: i64, cs: i64, rank: i64, n_iter: i64,
                       n_over: i64, opts: *const CorrlaOpts, u: *mut f64, ldu: i64, s: *mut f64, vt: *mut f64,
                       ldvt: i64) -> c_int;
    fn corrla_rsvd_f32(ctx: *mut c_void, a: *const f32, m: i64, n: i64, rs: i64, cs: i64, rank: i64, n_iter: i64,
                       n_over: i64, opts: *const CorrlaOpts, u: *mut f32, ldu: i64, s: *mut f32, vt: *mut f32,
                       ldvt: i64) -> c_int;
    fn corrla_power_iter_f64(ctx: *mut c_void, a: *const f64, m: i64, n: i64, rs: i64, cs: i64, width: i64,
                             n_iter: i64, opts: *const CorrlaOpts, q: *mut f64, ldq: i64) -> c_int;
    fn corrla_power_iter_f32(ctx: *mut c_void, a: *const f32, m: i64, n: i64, rs: i64, cs: i64, width: i64,
                             n_iter: i64, opts: *const CorrlaOpts, q: *mut f32, ldq: i64) -> c_int;
    fn corrla_pca_f64(ctx: *mut c_void, x: *const f64, m: i64, n: i64, rs: i64, cs: i64, rank: i64, n_iter: i64,
                      n_over: i64, opts: *const CorrlaOpts, means: *mut f64, s: *mut f64, comps: *mut f64,
                      ldc: i64) -> c_int;
    fn corrla_grad_mat_f64(ctx: *mut c_void, x: *const f64, n_pts: i64, k: i64, y: *const f64, xq: *const f64,
                           n_q: i64, est_order: c_int, n_nbrs: i64, out_scale: f64, g: *mut f64, ldg: i64,
                           n_regularised: *mut c_int) -> c_int;
    // CSR sparse input (include/corrla_rsvd.h, "CSR sparse input"): values, int32 col_idx, int64 row_ptr (m + 1 entries)
    pub fn corrla_rsvd_csr_f32(ctx: *mut c_void, values: *const f32, col_idx: *const i32, row_ptr: *const i64, m: i64,
                               n: i64, nnz: i64, rank: i64, n_iter: i64, n_over: i64, opts: *const CorrlaOpts,
                               u: *mut f32, ldu: i64, s: *mut f32, vt: *mut f32, ldvt: i64) -> c_int;
    pub fn corrla_pca_csr_f32(ctx: *mut c_void, values: *const f32, col_idx: *const i32, row_ptr: *const i64, m: i64,
                              n: i64, nnz: i64, rank: i64, n_iter: i64, n_over: i64, opts: *const CorrlaOpts,
                              means: *mut f32, s: *mut f32, comps: *mut f32, ldc: i64) -> c_int;
    pub fn corrla_rsvd_csr_dev_f32(ctx: *mut c_void, values: *const f32, col_idx: *const i32, row_ptr: *const i64, m: i64,
                               n: i64, nnz: i64, rank: i64, n_iter: i64, n_over: i64, opts: *const CorrlaOpts,
                               u: *mut f32, ldu: i64, s: *mut f32, vt: *mut f32, ldvt: i64) -> c_int;
    pub fn corrla_pca_csr_dev_f32(ctx: *mut c_void, values: *const f32, col_idx: *const i32, row_ptr: *const i64, m: i64,
                              n: i64, nnz: i64, rank: i64, n_iter: i64, n_over: i64, opts: *const CorrlaOpts,
                              means: *mut f32, s: *mut f32, comps: *mut f32, ldc: i64) -> c_int;
    pub fn corrla_spmm_csr_dev_f32(ctx: *mut c_void, trans: c_int, values: *const f32, col_idx: *const i32,
                                   row_ptr: *const i64, m: i64, n: i64, nnz: i64, x: *const f32, ldx: i64, l: i64,
                                   beta: f32, res: *mut f32, ldres: i64) -> c_int;
    pub fn corrla_rsvd_csr_f64(ctx: *mut c_void, values: *const f64, col_idx: *const i32, row_ptr: *const i64, m: i64,
                               n: i64, nnz: i64, rank: i64, n_iter: i64, n_over: i64, opts: *const CorrlaOpts,
                               u: *mut f64, ldu: i64, s: *mut f64, vt: *mut f64, ldvt: i64) -> c_int;
    pub fn corrla_pca_csr_f64(ctx: *mut c_void, values: *const f64, col_idx: *const i32, row_ptr: *const i64, m: i64,
                              n: i64, nnz: i64, rank: i64, n_iter: i64, n_over: i64, opts: *const CorrlaOpts,
                              means: *mut f64, s: *mut f64, comps: *mut f64, ldc: i64) -> c_int;
    pub fn corrla_rsvd_csr_dev_f64(ctx: *mut c_void, values: *const f64, col_idx: *const i32, row_ptr: *const i64, m: i64,
                               n: i64, nnz: i64, rank: i64, n_iter: i64, n_over: i64, opts: *const CorrlaOpts,
                               u: *mut f64, ldu: i64, s: *mut f64, vt: *mut f64, ldvt: i64) -> c_int;
    pub fn corrla_pca_csr_dev_f64(ctx: *mut c_void, values: *const f64, col_idx: *const i32, row_ptr: *const i64, m: i64,
                              n: i64, nnz: i64, rank: i64, n_iter: i64, n_over: i64, opts: *const CorrlaOpts,
                              means: *mut f64, s: *mut f64, comps: *mut f64, ldc: i64) -> c_int;
    pub fn corrla_spmm_csr_dev_f64(ctx: *mut c_void, trans: c_int, values: *const f64, col_idx: *const i32,
                                   row_ptr: *const i64, m: i64, n: i64, nnz: i64, x: *const f64, ldx: i64, l: i64,
                                   beta: f64, res: *mut f64, ldres: i64) -> c_int;
    // covariance / Pearson correlation matrix (stats_corr.rs:14-43); host pointers, c is n x n with leading dimension ldc
    pub fn corrla_cov_f64(ctx: *mut c_void, x: *const f64, m: i64, n: i64, rs: i64, cs: i64, flags: u64, ddof: c_int,
                          means_out: *mut f64, scales_out: *mut f64, c: *mut f64, ldc: i64, route_out: *mut c_int) -> c_int;
    pub fn corrla_cov_f32(ctx: *mut c_void, x: *const f32, m: i64, n: i64, rs: i64, cs: i64, flags: u64, ddof: c_int,
                          means_out: *mut f32, scales_out: *mut f32, c: *mut f32, ldc: i64, route_out: *mut c_int) -> c_int;
    // ... device pointers; enqueues on the context's stream and returns without synchronising
    pub fn corrla_cov_dev_f64(ctx: *mut c_void, x: *const f64, m: i64, n: i64, rs: i64, cs: i64, flags: u64, ddof: c_int,
                              means_out: *mut f64, scales_out: *mut f64, c: *mut f64, ldc: i64, route_out: *mut c_int) -> c_int;
    pub fn corrla_cov_dev_f32(ctx: *mut c_void, x: *const f32, m: i64, n: i64, rs: i64, cs: i64, flags: u64, ddof: c_int,
                              means_out: *mut f32, scales_out: *mut f32, c: *mut f32, ldc: i64, route_out: *mut c_int) -> c_int;
    // the fitted PCA model (pca_rsvd.rs:43-52): scores (m x k, column-major ld_scores), optional Q-residuals and own means
    pub fn corrla_pca_transform_f64(ctx: *mut c_void, x: *const f64, m: i64, n: i64, rs: i64, cs: i64, means: *const f64,
                                     scales: *const f64, components: *const f64, ldc: i64, k: i64, flags: u64,
                                     scores: *mut f64, ld_scores: i64, resid_out: *mut f64, means_out: *mut f64) -> c_int;
    pub fn corrla_pca_transform_f32(ctx: *mut c_void, x: *const f32, m: i64, n: i64, rs: i64, cs: i64, means: *const f32,
                                     scales: *const f32, components: *const f32, ldc: i64, k: i64, flags: u64,
                                     scores: *mut f32, ld_scores: i64, resid_out: *mut f32, means_out: *mut f32) -> c_int;
    pub fn corrla_pca_transform_dev_f64(ctx: *mut c_void, x: *const f64, m: i64, n: i64, rs: i64, cs: i64, means: *const f64,
                                     scales: *const f64, components: *const f64, ldc: i64, k: i64, flags: u64,
                                     scores: *mut f64, ld_scores: i64, resid_out: *mut f64, means_out: *mut f64) -> c_int;
    pub fn corrla_pca_transform_dev_f32(ctx: *mut c_void, x: *const f32, m: i64, n: i64, rs: i64, cs: i64, means: *const f32,
                                     scales: *const f32, components: *const f32, ldc: i64, k: i64, flags: u64,
                                     scores: *mut f32, ld_scores: i64, resid_out: *mut f32, means_out: *mut f32) -> c_int;
    pub fn corrla_pca_transform_csr_f64(ctx: *mut c_void, values: *const f64, col_idx: *const i32, row_ptr: *const i64,
                                         m: i64, n: i64, nnz: i64, means: *const f64, scales: *const f64,
                                         components: *const f64, ldc: i64, k: i64, flags: u64, scores: *mut f64,
                                         ld_scores: i64, resid_out: *mut f64, means_out: *mut f64) -> c_int;
    pub fn corrla_pca_transform_csr_f32(ctx: *mut c_void, values: *const f32, col_idx: *const i32, row_ptr: *const i64,
                                         m: i64, n: i64, nnz: i64, means: *const f32, scales: *const f32,
                                         components: *const f32, ldc: i64, k: i64, flags: u64, scores: *mut f32,
                                         ld_scores: i64, resid_out: *mut f32, means_out: *mut f32) -> c_int;
    pub fn corrla_pca_transform_csr_dev_f64(ctx: *mut c_void, values: *const f64, col_idx: *const i32, row_ptr: *const i64,
                                         m: i64, n: i64, nnz: i64, means: *const f64, scales: *const f64,
                                         components: *const f64, ldc: i64, k: i64, flags: u64, scores: *mut f64,
                                         ld_scores: i64, resid_out: *mut f64, means_out: *mut f64) -> c_int;
    pub fn corrla_pca_transform_csr_dev_f32(ctx: *mut c_void, values: *const f32, col_idx: *const i32, row_ptr: *const i64,
                                         m: i64, n: i64, nnz: i64, means: *const f32, scales: *const f32,
                                         components: *const f32, ldc: i64, k: i64, flags: u64, scores: *mut f32,
                                         ld_scores: i64, resid_out: *mut f32, means_out: *mut f32) -> c_int;
    // out (m x n, unit stride along the features) = (scores V) D + 1 mu^T
    pub fn corrla_pca_inverse_f64(ctx: *mut c_void, scores: *const f64, m: i64, k: i64, ld_scores: i64, means: *const f64,
                                   scales: *const f64, components: *const f64, ldc: i64, n: i64, out: *mut f64,
                                   row_stride_out: i64) -> c_int;
    pub fn corrla_pca_inverse_f32(ctx: *mut c_void, scores: *const f32, m: i64, k: i64, ld_scores: i64, means: *const f32,
                                   scales: *const f32, components: *const f32, ldc: i64, n: i64, out: *mut f32,
                                   row_stride_out: i64) -> c_int;
    pub fn corrla_pca_inverse_dev_f64(ctx: *mut c_void, scores: *const f64, m: i64, k: i64, ld_scores: i64, means: *const f64,
                                   scales: *const f64, components: *const f64, ldc: i64, n: i64, out: *mut f64,
                                   row_stride_out: i64) -> c_int;
    pub fn corrla_pca_inverse_dev_f32(ctx: *mut c_void, scores: *const f32, m: i64, k: i64, ld_scores: i64, means: *const f32,
                                   scales: *const f32, components: *const f32, ldc: i64, n: i64, out: *mut f32,
                                   row_stride_out: i64) -> c_int;
    pub fn corrla_ctx_last_pca_apply(ctx: *mut c_void, centring_out: *mut c_int, route_out: *mut c_int) -> c_int;
    // RBF kernel matrices (interp_utils.rs:96-129, 146-153): out (n_q x n_s, row-major) = phi(||xq_i - xs_j||)
    pub fn corrla_rbf_matrix_f64(ctx: *mut c_void, xq: *const f64, n_q: i64, ldq: i64, xs: *const f64, n_s: i64, lds: i64,
                                  dim: i64, kernel: c_int, eps: f64, out: *mut f64, ld_out: i64) -> c_int;
    pub fn corrla_rbf_matrix_f32(ctx: *mut c_void, xq: *const f32, n_q: i64, ldq: i64, xs: *const f32, n_s: i64, lds: i64,
                                  dim: i64, kernel: c_int, eps: f64, out: *mut f32, ld_out: i64) -> c_int;
    pub fn corrla_rbf_matrix_dev_f64(ctx: *mut c_void, xq: *const f64, n_q: i64, ldq: i64, xs: *const f64, n_s: i64, lds: i64,
                                  dim: i64, kernel: c_int, eps: f64, out: *mut f64, ld_out: i64) -> c_int;
    pub fn corrla_rbf_matrix_dev_f32(ctx: *mut c_void, xq: *const f32, n_q: i64, ldq: i64, xs: *const f32, n_s: i64, lds: i64,
                                  dim: i64, kernel: c_int, eps: f64, out: *mut f32, ld_out: i64) -> c_int;
    // out (n_q x n_rhs, row-major) = Phi W_rbf + P(xq) W_poly; coeffs = [W_rbf; W_poly] as RbfInterp::fit lays them out
    pub fn corrla_rbf_apply_f64(ctx: *mut c_void, xq: *const f64, n_q: i64, ldq: i64, xs: *const f64, n_s: i64, lds: i64,
                                 dim: i64, kernel: c_int, eps: f64, poly_degree: c_int, coeffs: *const f64, ldw: i64,
                                 n_rhs: i64, out: *mut f64, ld_out: i64) -> c_int;
    pub fn corrla_rbf_apply_f32(ctx: *mut c_void, xq: *const f32, n_q: i64, ldq: i64, xs: *const f32, n_s: i64, lds: i64,
                                 dim: i64, kernel: c_int, eps: f64, poly_degree: c_int, coeffs: *const f32, ldw: i64,
                                 n_rhs: i64, out: *mut f32, ld_out: i64) -> c_int;
    pub fn corrla_rbf_apply_dev_f64(ctx: *mut c_void, xq: *const f64, n_q: i64, ldq: i64, xs: *const f64, n_s: i64, lds: i64,
                                 dim: i64, kernel: c_int, eps: f64, poly_degree: c_int, coeffs: *const f64, ldw: i64,
                                 n_rhs: i64, out: *mut f64, ld_out: i64) -> c_int;
    pub fn corrla_rbf_apply_dev_f32(ctx: *mut c_void, xq: *const f32, n_q: i64, ldq: i64, xs: *const f32, n_s: i64, lds: i64,
                                 dim: i64, kernel: c_int, eps: f64, poly_degree: c_int, coeffs: *const f32, ldw: i64,
                                 n_rhs: i64, out: *mut f32, ld_out: i64) -> c_int;
    // polynomial response surfaces (stats_corr.rs:146-249): G = [V(z), y]^T [V(z), y] without storing V; means, scales of z
    pub fn corrla_polyfit_gram_f64(ctx: *mut c_void, x: *const f64, m: i64, k: i64, ldx: i64, y: *const f64, r: i64, ldy: i64,
                                    degree: c_int, normalize: c_int, g: *mut f64, ldg: i64, means: *mut f64,
                                    scales: *mut f64) -> c_int;
    pub fn corrla_polyfit_gram_f32(ctx: *mut c_void, x: *const f32, m: i64, k: i64, ldx: i64, y: *const f32, r: i64, ldy: i64,
                                    degree: c_int, normalize: c_int, g: *mut f64, ldg: i64, means: *mut f64,
                                    scales: *mut f64) -> c_int;
    pub fn corrla_polyfit_gram_dev_f64(ctx: *mut c_void, x: *const f64, m: i64, k: i64, ldx: i64, y: *const f64, r: i64, ldy: i64,
                                    degree: c_int, normalize: c_int, g: *mut f64, ldg: i64, means: *mut f64,
                                    scales: *mut f64) -> c_int;
    pub fn corrla_polyfit_gram_dev_f32(ctx: *mut c_void, x: *const f32, m: i64, k: i64, ldx: i64, y: *const f32, r: i64, ldy: i64,
                                    degree: c_int, normalize: c_int, g: *mut f64, ldg: i64, means: *mut f64,
                                    scales: *mut f64) -> c_int;
    // out (m x r, row-major) = V(x) coeffs; jac (nullable): r slabs of m x k analytic gradients
    pub fn corrla_poly_eval_f64(ctx: *mut c_void, x: *const f64, m: i64, k: i64, ldx: i64, coeffs: *const f64, ldc: i64, r: i64,
                                 degree: c_int, out: *mut f64, ld_out: i64, jac: *mut f64, ld_jac: i64) -> c_int;
    pub fn corrla_poly_eval_f32(ctx: *mut c_void, x: *const f32, m: i64, k: i64, ldx: i64, coeffs: *const f64, ldc: i64, r: i64,
                                 degree: c_int, out: *mut f32, ld_out: i64, jac: *mut f32, ld_jac: i64) -> c_int;
    pub fn corrla_poly_eval_dev_f64(ctx: *mut c_void, x: *const f64, m: i64, k: i64, ldx: i64, coeffs: *const f64, ldc: i64, r: i64,
                                 degree: c_int, out: *mut f64, ld_out: i64, jac: *mut f64, ld_jac: i64) -> c_int;
    pub fn corrla_poly_eval_dev_f32(ctx: *mut c_void, x: *const f32, m: i64, k: i64, ldx: i64, coeffs: *const f64, ldc: i64, r: i64,
                                 degree: c_int, out: *mut f32, ld_out: i64, jac: *mut f32, ld_jac: i64) -> c_int;
    pub fn corrla_ctx_last_polyfit(ctx: *mut c_void, route_out: *mut c_int) -> c_int;
    // Gaussian kernel density estimates (univariate_rv.rs:165-170, 423-444): what 0 pdf, 1 cdf, 2 logpdf at the points x
    pub fn corrla_kde_eval_f64(ctx: *mut c_void, x: *const f64, n_q: i64, incx: i64, s: *const f64, n_s: i64, incs: i64, h: f64,
                                what: c_int, out: *mut f64, inco: i64) -> c_int;
    pub fn corrla_kde_eval_f32(ctx: *mut c_void, x: *const f32, n_q: i64, incx: i64, s: *const f32, n_s: i64, incs: i64, h: f64,
                                what: c_int, out: *mut f32, inco: i64) -> c_int;
    pub fn corrla_kde_eval_dev_f64(ctx: *mut c_void, x: *const f64, n_q: i64, incx: i64, s: *const f64, n_s: i64, incs: i64, h: f64,
                                what: c_int, out: *mut f64, inco: i64) -> c_int;
    pub fn corrla_kde_eval_dev_f32(ctx: *mut c_void, x: *const f32, n_q: i64, incx: i64, s: *const f32, n_s: i64, incs: i64, h: f64,
                                what: c_int, out: *mut f32, inco: i64) -> c_int;
    // nll[b] = -sum_i logpdf_i(h[b]) and dnll[b] = d nll / d h (nullable) for n_h <= 64 bandwidths; h is always a host pointer
    pub fn corrla_kde_nll_f64(ctx: *mut c_void, x: *const f64, n_t: i64, incx: i64, s: *const f64, n_s: i64, incs: i64,
                               h: *const f64, n_h: i64, nll: *mut f64, dnll: *mut f64) -> c_int;
    pub fn corrla_kde_nll_f32(ctx: *mut c_void, x: *const f32, n_t: i64, incx: i64, s: *const f32, n_s: i64, incs: i64,
                               h: *const f64, n_h: i64, nll: *mut f64, dnll: *mut f64) -> c_int;
    pub fn corrla_kde_nll_dev_f64(ctx: *mut c_void, x: *const f64, n_t: i64, incx: i64, s: *const f64, n_s: i64, incs: i64,
                               h: *const f64, n_h: i64, nll: *mut f64, dnll: *mut f64) -> c_int;
    pub fn corrla_kde_nll_dev_f32(ctx: *mut c_void, x: *const f32, n_t: i64, incx: i64, s: *const f32, n_s: i64, incs: i64,
                               h: *const f64, n_h: i64, nll: *mut f64, dnll: *mut f64) -> c_int;
    pub fn corrla_ctx_last_kde(ctx: *mut c_void, route_out: *mut c_int) -> c_int;
    // multivariate normal rows x_i = mean + factor z_i (stats_corr.rs:46-58; factor d x r, covariance factor factor^T -- the
    // reference's own law, covariance C^2, is factor = C) and the sandwich variances j_i^T C j_i (stats_corr.rs:64-68)
    pub fn corrla_mvn_sample_f64(ctx: *mut c_void, n: i64, d: i64, r: i64, factor: *const f64, ldf: i64, mean: *const f64, seed: u64,
                                 first: i64, lower: c_int, out: *mut f64, ldo: i64) -> c_int;
    pub fn corrla_mvn_sample_f32(ctx: *mut c_void, n: i64, d: i64, r: i64, factor: *const f32, ldf: i64, mean: *const f32, seed: u64,
                                 first: i64, lower: c_int, out: *mut f32, ldo: i64) -> c_int;
    pub fn corrla_mvn_sample_dev_f64(ctx: *mut c_void, n: i64, d: i64, r: i64, factor: *const f64, ldf: i64, mean: *const f64, seed: u64,
                                     first: i64, lower: c_int, out: *mut f64, ldo: i64) -> c_int;
    pub fn corrla_mvn_sample_dev_f32(ctx: *mut c_void, n: i64, d: i64, r: i64, factor: *const f32, ldf: i64, mean: *const f32, seed: u64,
                                     first: i64, lower: c_int, out: *mut f32, ldo: i64) -> c_int;
    pub fn corrla_sandwich_diag_f64(ctx: *mut c_void, jac: *const f64, m: i64, d: i64, ldj: i64, cov: *const f64, ldc: i64, v: *mut f64) -> c_int;
    pub fn corrla_sandwich_diag_f32(ctx: *mut c_void, jac: *const f32, m: i64, d: i64, ldj: i64, cov: *const f32, ldc: i64, v: *mut f32) -> c_int;
    pub fn corrla_sandwich_diag_dev_f64(ctx: *mut c_void, jac: *const f64, m: i64, d: i64, ldj: i64, cov: *const f64, ldc: i64, v: *mut f64) -> c_int;
    pub fn corrla_sandwich_diag_dev_f32(ctx: *mut c_void, jac: *const f32, m: i64, d: i64, ldj: i64, cov: *const f32, ldc: i64, v: *mut f32) -> c_int;
    pub fn corrla_ctx_last_mvn(ctx: *mut c_void, route_out: *mut c_int) -> c_int;
    // dense LU solve, partial pivoting, every matrix ROW-major: x = a^-1 b (host pointers, a and b untouched) / in place on the
    // device (a becomes LU, b becomes X, ipiv nullable)
    pub fn corrla_lu_solve_f64(ctx: *mut c_void, a: *const f64, n: i64, lda: i64, b: *const f64, n_rhs: i64, ldb: i64, x: *mut f64,
                               ldx: i64) -> c_int;
    pub fn corrla_lu_solve_dev_f64(ctx: *mut c_void, a: *mut f64, n: i64, lda: i64, b: *mut f64, n_rhs: i64, ldb: i64,
                                   ipiv: *mut i64) -> c_int;
    // the RBF block system [[K, P], [P^T, 0]] (N x N, N = n_s + n_poly) and the fit coeffs = M^-1 [y; 0] in rbf_apply's layout
    pub fn corrla_rbffit_system_f64(ctx: *mut c_void, xs: *const f64, n_s: i64, ldxs: i64, dim: i64, kernel: c_int, eps: f64,
                                 poly_degree: c_int, m: *mut f64, ldm: i64) -> c_int;
    pub fn corrla_rbffit_system_dev_f64(ctx: *mut c_void, xs: *const f64, n_s: i64, ldxs: i64, dim: i64, kernel: c_int, eps: f64,
                                     poly_degree: c_int, m: *mut f64, ldm: i64) -> c_int;
    pub fn corrla_rbffit_f64(ctx: *mut c_void, xs: *const f64, n_s: i64, ldxs: i64, dim: i64, y: *const f64, n_rhs: i64, ldy: i64,
                              kernel: c_int, eps: f64, poly_degree: c_int, coeffs: *mut f64, ldw: i64) -> c_int;
    pub fn corrla_rbffit_dev_f64(ctx: *mut c_void, xs: *const f64, n_s: i64, ldxs: i64, dim: i64, y: *const f64, n_rhs: i64, ldy: i64,
                                  kernel: c_int, eps: f64, poly_degree: c_int, coeffs: *mut f64, ldw: i64) -> c_int;
    pub fn corrla_ctx_last_solve(ctx: *mut c_void, route: *mut c_int, info: *mut i64, min_pivot: *mut f64, max_u: *mut f64) -> c_int;
    // dense Cholesky A = L L^T over the LOWER triangle, every matrix ROW-major: the factor (host pointers: l gets L and zeros above;
    // device: in place) and x = a^-1 b for a symmetric positive definite a (host pointers, a and b untouched / in place on the device)
    pub fn corrla_chol_factor_f64(ctx: *mut c_void, a: *const f64, n: i64, lda: i64, l: *mut f64, ldl: i64) -> c_int;
    pub fn corrla_chol_factor_dev_f64(ctx: *mut c_void, a: *mut f64, n: i64, lda: i64) -> c_int;
    pub fn corrla_chol_solve_f64(ctx: *mut c_void, a: *const f64, n: i64, lda: i64, b: *const f64, n_rhs: i64, ldb: i64, x: *mut f64,
                                 ldx: i64) -> c_int;
    pub fn corrla_chol_solve_dev_f64(ctx: *mut c_void, a: *mut f64, n: i64, lda: i64, b: *mut f64, n_rhs: i64, ldb: i64) -> c_int;
    pub fn corrla_ctx_last_chol(ctx: *mut c_void, route: *mut c_int, info: *mut i64, min_diag: *mut f64, max_diag: *mut f64,
                                logdet: *mut f64) -> c_int;
}

/// One context per thread (device 0): replaces faer's process-global `Parallelism` (mat_utils.rs:31).
struct Ctx(*mut c_void);
impl Drop for Ctx {
    fn drop(&mut self) {
        unsafe { corrla_ctx_destroy(self.0) }
    }
}
thread_local! {
    static CTX: Ctx = unsafe {
        let mut c = std::ptr::null_mut();
        check(corrla_ctx_create(0, &mut c));
        Ctx(c)
    };
}

fn check(rc: c_int) {
    if rc != 0 {
        let msg = unsafe { CStr::from_ptr(corrla_last_error()) }.to_string_lossy().into_owned();
        panic!("corrla_rsvd (status {}): {}", rc, msg);
    }
}

/// Element types the library is built for (the reference is generic over `faer::RealField + Float`, instantiated
/// with f64 everywhere and f32 in tests).
pub trait RsvdScalar: faer::Entity + Copy + Default {
    unsafe fn rsvd(ctx: *mut c_void, a: *const Self, m: i64, n: i64, rs: i64, cs: i64, k: i64, q: i64, p: i64,
                   u: *mut Self, ldu: i64, s: *mut Self, vt: *mut Self, ldvt: i64) -> c_int;
    unsafe fn power(ctx: *mut c_void, a: *const Self, m: i64, n: i64, rs: i64, cs: i64, w: i64, q: i64,
                    out: *mut Self, ldq: i64) -> c_int;
}
impl RsvdScalar for f64 {
    unsafe fn rsvd(ctx: *mut c_void, a: *const f64, m: i64, n: i64, rs: i64, cs: i64, k: i64, q: i64, p: i64,
                   u: *mut f64, ldu: i64, s: *mut f64, vt: *mut f64, ldvt: i64) -> c_int {
        corrla_rsvd_f64(ctx, a, m, n, rs, cs, k, q, p, std::ptr::null(), u, ldu, s, vt, ldvt)
    }
    unsafe fn power(ctx: *mut c_void, a: *const f64, m: i64, n: i64, rs: i64, cs: i64, w: i64, q: i64,
                    out: *mut f64, ldq: i64) -> c_int {
        corrla_power_iter_f64(ctx, a, m, n, rs, cs, w, q, std::ptr::null(), out, ldq)
    }
}
impl RsvdScalar for f32 {
    unsafe fn rsvd(ctx: *mut c_void, a: *const f32, m: i64, n: i64, rs: i64, cs: i64, k: i64, q: i64, p: i64,
                   u: *mut f32, ldu: i64, s: *mut f32, vt: *mut f32, ldvt: i64) -> c_int {
        corrla_rsvd_f32(ctx, a, m, n, rs, cs, k, q, p, std::ptr::null(), u, ldu, s, vt, ldvt)
    }
    unsafe fn power(ctx: *mut c_void, a: *const f32, m: i64, n: i64, rs: i64, cs: i64, w: i64, q: i64,
                    out: *mut f32, ldq: i64) -> c_int {
        corrla_power_iter_f32(ctx, a, m, n, rs, cs, w, q, std::ptr::null(), out, ldq)
    }
}

/// random_svd.rs:63-110 -- same name, argument order and result shapes: (U m x k, S k x 1, Vt k x n).
pub fn random_svd<T: RsvdScalar>(a_mat: MatRef<T>, omega_rank: usize, n_iter: usize, n_oversamples: usize)
    -> (Mat<T>, Mat<T>, Mat<T>)
{
    let (m, n, k) = (a_mat.nrows(), a_mat.ncols(), omega_rank);
    let mut u = Mat::<T>::zeros(m, k);
    let mut s = Mat::<T>::zeros(k, 1); // k x 1, as s_diagonal().as_2d() at random_svd.rs:99,106
    let mut vt = Mat::<T>::zeros(k, n);
    let rc = CTX.with(|c| unsafe {
        T::rsvd(c.0, a_mat.as_ptr(), m as i64, n as i64, a_mat.row_stride() as i64, a_mat.col_stride() as i64,
                k as i64, n_iter as i64, n_oversamples as i64, u.as_ptr_mut(), u.col_stride() as i64,
                s.as_ptr_mut(), vt.as_ptr_mut(), vt.col_stride() as i64)
    });
    check(rc);
    (u, s, vt)
}

/// random_svd.rs:15-59 -- `omega_rank` is the already-oversampled sketch width; returns the orthonormal Q (m x width).
pub fn power_iter<T: RsvdScalar>(a_mat: MatRef<T>, omega_rank: usize, n_iter: usize) -> Mat<T> {
    let (m, n) = (a_mat.nrows(), a_mat.ncols());
    let mut q = Mat::<T>::zeros(m, omega_rank);
    let rc = CTX.with(|c| unsafe {
        T::power(c.0, a_mat.as_ptr(), m as i64, n as i64, a_mat.row_stride() as i64, a_mat.col_stride() as i64,
                 omega_rank as i64, n_iter as i64, q.as_ptr_mut(), q.col_stride() as i64)
    });
    check(rc);
    q
}

/// The fit of `PcaRsvd::new(x_mat, rank)` (pca_rsvd.rs:56-82) in one call: column means, centring and
/// `random_svd(cx, rank, 20, min(n_dim, 10))`.  Returns (means 1 x n_dim, singular values k x 1, components k x n_dim).
pub fn pca_rsvd_fit(x_mat: MatRef<f64>, rank: usize) -> (Mat<f64>, Mat<f64>, Mat<f64>) {
    let (m, n) = (x_mat.nrows(), x_mat.ncols());
    let mut means = Mat::<f64>::zeros(n, 1); // n contiguous values; read as the reference's 1 x n row
    let mut s = Mat::<f64>::zeros(rank, 1);
    let mut comps = Mat::<f64>::zeros(rank, n);
    let rc = CTX.with(|c| unsafe {
        corrla_pca_f64(c.0, x_mat.as_ptr(), m as i64, n as i64, x_mat.row_stride() as i64, x_mat.col_stride() as i64,
                       rank as i64, 20, std::cmp::min(n, 10) as i64, std::ptr::null(), means.as_ptr_mut(),
                       s.as_ptr_mut(), comps.as_ptr_mut(), comps.col_stride() as i64)
    });
    check(rc);
    (means.transpose().to_owned(), s, comps)
}

/// `ActiveSsRsvd::create_grad_mat` with a `PolyGradientEstimator(x, y, est_order, n_nbrs)`
/// (active_subspaces.rs:66-141, 215-229).  `x` and `xq` must be row-major n x k (contiguous rows); returns the
/// column-major k x n_q gradient matrix and the number of queries whose fit needed the ridge.
pub fn create_grad_mat(x: MatRef<f64>, y: &[f64], xq: MatRef<f64>, est_order: i32, n_nbrs: usize) -> (Mat<f64>, i32) {
    assert!(x.col_stride() == 1 && xq.col_stride() == 1, "row-major point sets expected");
    assert!(x.row_stride() as usize == x.ncols() && xq.row_stride() as usize == xq.ncols());
    let (n, k, nq) = (x.nrows(), x.ncols(), xq.nrows());
    assert_eq!(y.len(), n);
    let mut g = Mat::<f64>::zeros(k, nq);
    let mut nreg: c_int = 0;
    let rc = CTX.with(|c| unsafe {
        corrla_grad_mat_f64(c.0, x.as_ptr(), n as i64, k as i64, y.as_ptr(), xq.as_ptr(), nq as i64, est_order,
                            n_nbrs as i64, 1.0, g.as_ptr_mut(), g.col_stride() as i64, &mut nreg)
    });
    check(rc);
    (g, nreg)
}

#[cfg(test)]
mod tests {
    use super::*;
    use faer::mat;

    /// test_rsvd_lowrank, random_svd.rs:153-196: S = (3, 2.2360679, 2, 0, 0) to 1e-3
    #[test]
    fn known_answer_5x5() {
        let a = mat![
            [1.0, 0.0, 0.0, 0.0, 2.0],
            [0.0, 0.0, 3.0, 0.0, 0.0],
            [0.0, 0.0, 0.0, 0.0, 0.0],
            [0.0, 0.0, 0.0, 0.0, 0.0],
            [0.0, 2.0, 0.0, 0.0, 0.0f64]
        ];
        let (_u, s, _vt) = random_svd(a.as_ref(), 5, 12, 10);
        let want = [3.0, 2.2360679, 2.0, 0.0, 0.0];
        for i in 0..5 {
            assert!((s.read(i, 0) - want[i]).abs() < 1e-3);
        }
    }
}
