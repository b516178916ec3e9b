// libcorrla_rsvd.so -- C ABI (include/corrla_rsvd.h) over the HIP backend.  This translation unit
// is the product: it contains no CPU compute path; without a gfx950 device every compute entry
// point returns CORRLA_ENODEV / CORRLA_EHIP.
#include <mutex>

#include "capi_impl.hpp"
#include "colstat_stage.hpp"
#include "core_svd_stage.hpp"
#include "cov_stage.hpp"
#include "dirichlet_stage.hpp"
#include "eigh_stage.hpp"
#include "grad_stage.hpp"
#include "hip_backend.hpp"
#include "kde_stage.hpp"
#include "chol_stage.hpp"
#include "lu_stage.hpp"
#include "mvn_stage.hpp"
#include "pca_apply_stage.hpp"
#include "polyfit_stage.hpp"
#include "rbf_stage.hpp"
#include "tall_stage.hpp"
#include "thinq_stage.hpp"

using namespace corrla;

struct corrla_ctx {
  HipDev dev;
  Timings last;
  std::mutex mu;
  bool profile;
  pca_apply_stage::Ran pca_apply;  // how the last corrla_pca_transform_* / corrla_pca_inverse_* call ran
  polyfit_stage::Ran polyfit;      // how the last corrla_polyfit_gram_* / corrla_poly_eval_* call ran
  kde_stage::Ran kde;              // how the last corrla_kde_eval_* / corrla_kde_nll_* call ran
  dirichlet_stage::Ran dirichlet;  // how the last corrla_dirichlet_draws_* / corrla_dirichlet_sample_* call ran
  mvn_stage::Ran mvn;              // how the last corrla_mvn_sample_* call ran
  lu_stage::Ran lu;                // how the last corrla_lu_solve_* / corrla_rbffit_* call ran
  chol_stage::Ran chol;            // how the last corrla_chol_factor_* / corrla_chol_solve_* call ran
  eigh_stage::Ran eigh;            // how the last corrla_eigh_* call ran
  explicit corrla_ctx(int ordinal) : dev(ordinal), profile(env_int("CORRLA_PROFILE_PHASES", 0) != 0) {}
};

namespace {
inline corrla_ctx* need(corrla_ctx* c) {
  if (!c) throw Error(ST_EINVAL, "ctx is NULL");
  return c;
}
// Runs one entry point under the context lock.  On the exception path the stream is drained before the status is
// returned: kernels that write the caller's outputs, or still read the caller's Omega, may be queued, and the
// caller is free to release those buffers as soon as the call has failed.
template <class F>
inline void locked_call(corrla_ctx* c, F&& f) {
  std::lock_guard<std::mutex> lk(c->mu);
  try {
    f();
  } catch (...) {
    (void)hipSetDevice(c->dev.device);
    if (c->dev.stream) (void)hipStreamSynchronize(c->dev.stream);
    (void)hipGetLastError();
    throw;
  }
}

// One entry point: status and message from what `f` throws (guarded), a context (need), the lock (locked_call); `after`
// runs once the lock is released.
template <class F, class After>
inline corrla_status ctx_call(corrla_ctx* ctx, F&& f, After&& after) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    locked_call(c, [&] { f(*c); });
    after(*c);
  });
}
template <class F>
inline corrla_status ctx_call(corrla_ctx* ctx, F&& f) {
  return ctx_call(ctx, f, [](corrla_ctx&) {});
}
inline void debug_qr_breakdown(const corrla_ctx& c) {
  if (c.profile && env_int("CORRLA_DEBUG", 0))
    std::fprintf(stderr, "[corrla] qr breakdown (ms): gram %.3f  download+check %.3f  host chol/inv %.3f  upload+apply %.3f  (%d passes)\n",
                 c.last.qr_gram_ms, c.last.qr_down_ms, c.last.qr_host_ms, c.last.qr_apply_ms, c.last.qr_passes);
}
template <class T>
corrla_status fill_c(corrla_ctx* ctx, T* p, int64_t rows, int64_t cols, int64_t rs, int64_t cs, uint64_t seed,
                     int64_t row0, int64_t global_cols) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    if (!p) throw Error(ST_EINVAL, "p is NULL");
    if (rows < 0 || cols < 0 || rs < 0 || cs < 0 || global_cols < cols) throw Error(ST_EINVAL, "bad fill_normal shape");
    std::lock_guard<std::mutex> lk(c->mu);
    CORRLA_HIP(hipSetDevice(c->dev.device));
    c->dev.fill_normal(p, rows, cols, rs, cs, seed, row0, global_cols);
    c->dev.sync();
  });
}
template <class T>
corrla_status time_sketch_c(corrla_ctx* ctx, const T* a, int64_t m, int64_t n, int64_t rs, int64_t cs, const T* x,
                            int64_t ldx, int64_t l, T* y, int64_t ldy, int reps, double* avg_ms) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    if (!x || !y || !avg_ms) throw Error(ST_EINVAL, "NULL argument");
    if (reps < 1 || l < 1 || ldx < n || ldy < m) throw Error(ST_EINVAL, "bad time_sketch arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    HipDev& dev = c->dev;
    dev.begin_call();
    TallA<T> ta = stage_input<HipDev, T>(dev, false, a, m, n, rs, cs, true);
    RsvdDriver<HipDev, T> drv(dev, false);
    drv.mixed_planes_ = parse_opts(nullptr, true).mixed_planes;  // CORRLA_SKETCH_MIXED (the hook takes no opts)
    Skinny<T> xs = dev.alloc_skinny<T>(n, l);
    dev.copy_in_skinny(x, ldx, xs);
    Skinny<T> out = dev.alloc_skinny<T>(m, l);
    *avg_ms = dev.time_on_stream(reps, [&] { drv.a_times(ta, xs, out, nullptr); });
    dev.copy_out(out, l, y, ldy, false, false);
    dev.end_call();
  });
}
}  // namespace

extern "C" {

CORRLA_API const char* corrla_version(void) { return "corrla_rsvd 0.1.0 gfx950"; }
CORRLA_API const char* corrla_last_error(void) { return last_error_slot().c_str(); }
CORRLA_API int corrla_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

CORRLA_API corrla_status corrla_ctx_create(int device_ordinal, corrla_ctx** out) {
  return guarded([&] {
    if (!out) throw Error(ST_EINVAL, "out is NULL");
    *out = nullptr;
    *out = new corrla_ctx(device_ordinal);
  });
}
CORRLA_API void corrla_ctx_destroy(corrla_ctx* ctx) { delete ctx; }
CORRLA_API corrla_status corrla_ctx_synchronize(corrla_ctx* ctx) {
  return guarded([&] { need(ctx)->dev.sync(); });
}
CORRLA_API corrla_status corrla_ctx_comm_info(corrla_ctx* ctx, int* rank, int* nranks) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    if (!rank || !nranks) throw Error(ST_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    c->dev.comm_info(rank, nranks);
  });
}
CORRLA_API corrla_status corrla_ctx_set_phase_timings(corrla_ctx* ctx, int on) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    std::lock_guard<std::mutex> lk(c->mu);  // not while a call is in flight: its marks would be left half recorded
    c->dev.set_phase_events(on != 0);
  });
}
CORRLA_API corrla_status corrla_ctx_get_timings(corrla_ctx* ctx, corrla_timings* out) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    if (!out) throw Error(ST_EINVAL, "out is NULL");
    const Timings& t = c->last;
    out->total_ms = t.total_ms;
    out->sketch_ms = t.sketch_ms;
    out->power_ms = t.power_ms;
    out->qr_ms = t.qr_ms;
    out->project_ms = t.project_ms;
    out->small_svd_ms = t.small_svd_ms;
    out->finalize_ms = t.finalize_ms;
    out->qr_passes = t.qr_passes;
    out->n_collectives = t.n_collectives;
    out->collective_bytes = t.collective_bytes;
    out->sketch_kernel_ms = t.sketch_kernel_ms;
    out->host_enqueue_ms = t.host_enqueue_ms;
    out->n_mixed_products = t.n_mixed_products;
    out->n_bf16_products = t.n_bf16_products;
    out->knn_ms = t.knn_ms;
    out->fit_ms = t.fit_ms;
  });
}

// parameter lists of include/corrla_rsvd.h, after the context
#define CORRLA_DENSE(T, A) const T *A, int64_t m, int64_t n, int64_t rs, int64_t cs
#define CORRLA_CSR_A(T) const T *values, const int32_t *col_idx, const int64_t *row_ptr, int64_t m, int64_t n, int64_t nnz
#define CORRLA_RSVD_REST(T) int64_t rank, int64_t n_iter, int64_t p, const corrla_opts *o, T *u, int64_t ldu, T *s, T *vt, int64_t ldvt
#define CORRLA_PCA_REST(T) int64_t rank, int64_t n_iter, int64_t p, const corrla_opts *o, T *means, T *s, T *comps, int64_t ldc
#define CORRLA_PRODUCT_REST(T) const T *x, int64_t ldx, int64_t l, T beta, T *res, int64_t ldres

#define CORRLA_DEFINE_RSVD(NAME, T, HOST, SHARDED)                                                                      \
  CORRLA_API corrla_status NAME(corrla_ctx* ctx, CORRLA_DENSE(T, a), CORRLA_RSVD_REST(T)) {                              \
    return ctx_call(ctx, [&](corrla_ctx& c) {                                                                           \
      rsvd_entry<HipDev, T>(c.dev, HOST, SHARDED, a, m, n, rs, cs, rank, n_iter, p, o, u, ldu, s, vt, ldvt, &c.last,     \
                            c.profile);                                                                                 \
    }, debug_qr_breakdown);                                                                                             \
  }
#define CORRLA_DEFINE_PCA(NAME, T, HOST, SHARDED)                                                                       \
  CORRLA_API corrla_status NAME(corrla_ctx* ctx, CORRLA_DENSE(T, x), CORRLA_PCA_REST(T)) {                             \
    return ctx_call(ctx, [&](corrla_ctx& c) {                                                                           \
      pca_entry<HipDev, T>(c.dev, HOST, x, m, n, rs, cs, rank, n_iter, p, o, means, s, comps, ldc, &c.last, c.profile,   \
                           SHARDED);                                                                                    \
    });                                                                                                                 \
  }
#define CORRLA_DEFINE_POWER(NAME, T, HOST)                                                                              \
  CORRLA_API corrla_status NAME(corrla_ctx* ctx, CORRLA_DENSE(T, a), int64_t width, int64_t n_iter, const corrla_opts* o, \
                                T* q, int64_t ldq) {                                                                    \
    return ctx_call(ctx, [&](corrla_ctx& c) {                                                                           \
      power_iter_entry<HipDev, T>(c.dev, HOST, a, m, n, rs, cs, width, n_iter, o, q, ldq);                              \
    });                                                                                                                 \
  }

#define CORRLA_DEFINE(SUF, T)                                                                                          \
  CORRLA_DEFINE_RSVD(corrla_rsvd_##SUF, T, true, false)                                                                \
  CORRLA_DEFINE_RSVD(corrla_rsvd_dev_##SUF, T, false, false)                                                           \
  CORRLA_DEFINE_RSVD(corrla_rsvd_sharded_dev_##SUF, T, false, true)                                                    \
  CORRLA_DEFINE_PCA(corrla_pca_##SUF, T, true, false)                                                                  \
  CORRLA_DEFINE_PCA(corrla_pca_dev_##SUF, T, false, false)                                                             \
  CORRLA_DEFINE_PCA(corrla_pca_sharded_dev_##SUF, T, false, true)                                                      \
  CORRLA_DEFINE_POWER(corrla_power_iter_##SUF, T, true)                                                                \
  CORRLA_DEFINE_POWER(corrla_power_iter_dev_##SUF, T, false)                                                           \
  CORRLA_API corrla_status corrla_matmul_dev_##SUF(corrla_ctx* ctx, int trans, CORRLA_DENSE(T, a), CORRLA_PRODUCT_REST(T)) { \
    return ctx_call(ctx, [&](corrla_ctx& c) {                                                                          \
      matmul_entry<HipDev, T>(c.dev, trans, a, m, n, rs, cs, x, ldx, l, beta, res, ldres, &c.last);                    \
    });                                                                                                                \
  }                                                                                                                    \
  CORRLA_API corrla_status corrla_fill_normal_dev_##SUF(corrla_ctx* ctx, T* p, int64_t rows, int64_t cols, int64_t rs,            \
                                             int64_t cs, uint64_t seed, int64_t row0, int64_t global_cols) {           \
    return fill_c<T>(ctx, p, rows, cols, rs, cs, seed, row0, global_cols);                                             \
  }                                                                                                                    \
  CORRLA_API corrla_status corrla_time_sketch_dev_##SUF(corrla_ctx* ctx, const T* a, int64_t m, int64_t n, int64_t rs,            \
                                             int64_t cs, const T* x, int64_t ldx, int64_t l, T* y, int64_t ldy,        \
                                             int reps, double* avg_ms) {                                               \
    return time_sketch_c<T>(ctx, a, m, n, rs, cs, x, ldx, l, y, ldy, reps, avg_ms);                                    \
  }

CORRLA_DEFINE(f32, float)
CORRLA_DEFINE(f64, double)

// ---- CSR sparse input (values, int32 column indices, int64 row_ptr) ----------------------------------------------
#define CORRLA_DEFINE_RSVD_CSR(NAME, T, HOST)                                                                           \
  CORRLA_API corrla_status NAME(corrla_ctx* ctx, CORRLA_CSR_A(T), CORRLA_RSVD_REST(T)) {                                \
    return ctx_call(ctx, [&](corrla_ctx& c) {                                                                           \
      rsvd_csr_entry<HipDev, T>(c.dev, HOST, values, col_idx, row_ptr, m, n, nnz, rank, n_iter, p, o, u, ldu, s, vt,     \
                                ldvt, &c.last, c.profile);                                                              \
    });                                                                                                                 \
  }
#define CORRLA_DEFINE_PCA_CSR(NAME, T, HOST)                                                                            \
  CORRLA_API corrla_status NAME(corrla_ctx* ctx, CORRLA_CSR_A(T), CORRLA_PCA_REST(T)) {                                 \
    return ctx_call(ctx, [&](corrla_ctx& c) {                                                                           \
      pca_csr_entry<HipDev, T>(c.dev, HOST, values, col_idx, row_ptr, m, n, nnz, rank, n_iter, p, o, means, s, comps,    \
                               ldc, &c.last, c.profile);                                                                \
    });                                                                                                                 \
  }

#define CORRLA_DEFINE_CSR(SUF, T)                                                                                      \
  CORRLA_DEFINE_RSVD_CSR(corrla_rsvd_csr_##SUF, T, true)                                                               \
  CORRLA_DEFINE_RSVD_CSR(corrla_rsvd_csr_dev_##SUF, T, false)                                                          \
  CORRLA_DEFINE_PCA_CSR(corrla_pca_csr_##SUF, T, true)                                                                 \
  CORRLA_DEFINE_PCA_CSR(corrla_pca_csr_dev_##SUF, T, false)                                                            \
  CORRLA_API corrla_status corrla_spmm_csr_dev_##SUF(corrla_ctx* ctx, int trans, CORRLA_CSR_A(T), CORRLA_PRODUCT_REST(T)) { \
    return ctx_call(ctx, [&](corrla_ctx& c) {                                                                          \
      spmm_entry<HipDev, T>(c.dev, trans, values, col_idx, row_ptr, m, n, nnz, x, ldx, l, beta, res, ldres);           \
    });                                                                                                                \
  }

CORRLA_DEFINE_CSR(f32, float)
CORRLA_DEFINE_CSR(f64, double)

// ---- dense bf16 input (A: bfloat16 bit patterns; every other array f32) --------------------------------------------------
#define CORRLA_DEFINE_RSVD_BF16(NAME, HOST)                                                                             \
  CORRLA_API corrla_status NAME(corrla_ctx* ctx, CORRLA_DENSE(uint16_t, a), CORRLA_RSVD_REST(float)) {                  \
    return ctx_call(ctx, [&](corrla_ctx& c) {                                                                           \
      rsvd_bf16_entry<HipDev>(c.dev, HOST, a, m, n, rs, cs, rank, n_iter, p, o, u, ldu, s, vt, ldvt, &c.last, c.profile); \
    });                                                                                                                 \
  }
#define CORRLA_DEFINE_PCA_BF16(NAME, HOST)                                                                              \
  CORRLA_API corrla_status NAME(corrla_ctx* ctx, CORRLA_DENSE(uint16_t, x), CORRLA_PCA_REST(float)) {                   \
    return ctx_call(ctx, [&](corrla_ctx& c) {                                                                           \
      pca_bf16_entry<HipDev>(c.dev, HOST, x, m, n, rs, cs, rank, n_iter, p, o, means, s, comps, ldc, &c.last, c.profile); \
    });                                                                                                                 \
  }
CORRLA_DEFINE_RSVD_BF16(corrla_rsvd_bf16, true)
CORRLA_DEFINE_RSVD_BF16(corrla_rsvd_dev_bf16, false)
CORRLA_DEFINE_PCA_BF16(corrla_pca_bf16, true)
CORRLA_DEFINE_PCA_BF16(corrla_pca_dev_bf16, false)
CORRLA_API corrla_status corrla_matmul_dev_bf16(corrla_ctx* ctx, int trans, CORRLA_DENSE(uint16_t, a), CORRLA_PRODUCT_REST(float)) {
  return ctx_call(ctx, [&](corrla_ctx& c) {
    matmul_bf16_entry<HipDev>(c.dev, trans, a, m, n, rs, cs, x, ldx, l, beta, res, ldres, &c.last);
  });
}

// ---- covariance / correlation matrices (stats_corr.rs:14-43) -------------------------------------------------------------
#define CORRLA_DEFINE_COV(NAME, T, HOST)                                                                                \
  CORRLA_API corrla_status NAME(corrla_ctx* ctx, CORRLA_DENSE(T, x), uint64_t flags, int ddof, T* means_out, T* scales_out, \
                                T* c, int64_t ldc, int* route_out) {                                                    \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      const CovCall<T> call{x, m, n, rs, cs, flags, ddof, means_out, scales_out, c, ldc, route_out};                    \
      cov_entry<HipDev, T>(cx.dev, call, [&] { cov_stage::run<T>(cx.dev, HOST, call); });                               \
    });                                                                                                                 \
  }
CORRLA_DEFINE_COV(corrla_cov_f32, float, true)
CORRLA_DEFINE_COV(corrla_cov_f64, double, true)
CORRLA_DEFINE_COV(corrla_cov_dev_f32, float, false)
CORRLA_DEFINE_COV(corrla_cov_dev_f64, double, false)

// ---- the fitted PCA model: transform, inverse transform, Q-residuals (pca_rsvd.rs:43-52) -----------------------------------
#define CORRLA_PCA_MODEL(T) const T *means, const T *scales, const T *components, int64_t ldc, int64_t k, uint64_t flags, T *scores, \
                            int64_t ld_scores, T *resid_out, T *means_out
#define CORRLA_PCA_MODEL_CALL(T) PcaTransformCall<T>{m, n, means, scales, components, ldc, k, flags, scores, ld_scores, resid_out, means_out}
#define CORRLA_DEFINE_PCA_TRANSFORM(NAME, T, HOST)                                                                      \
  CORRLA_API corrla_status NAME(corrla_ctx* ctx, CORRLA_DENSE(T, x), CORRLA_PCA_MODEL(T)) {                             \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      cx.pca_apply = pca_apply_stage::Ran();                                                                            \
      const PcaTransformCall<T> c = CORRLA_PCA_MODEL_CALL(T);                                                           \
      if (!x) throw Error(ST_EINVAL, "pca_transform: x is NULL");                                                       \
      if (m < 1 || n < 1) throw Error(ST_EINVAL, "pca_transform: m and n must be >= 1");                                \
      if (rs < 0 || cs < 0) throw Error(ST_EINVAL, "pca_transform: negative strides are not supported");                \
      const Span xr(x, m, n, rs, cs, "x");                                                                              \
      pca_transform_entry<HipDev, T>(cx.dev, c, false, &xr, 1,                                                          \
                                     [&] { pca_apply_stage::run_dense<T>(cx.dev, HOST, x, rs, cs, c, &cx.pca_apply); }); \
    });                                                                                                                 \
  }
#define CORRLA_DEFINE_PCA_TRANSFORM_CSR(NAME, T, HOST)                                                                  \
  CORRLA_API corrla_status NAME(corrla_ctx* ctx, CORRLA_CSR_A(T), CORRLA_PCA_MODEL(T)) {                                \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      cx.pca_apply = pca_apply_stage::Ran();                                                                            \
      const PcaTransformCall<T> c = CORRLA_PCA_MODEL_CALL(T);                                                           \
      validate_csr_args(values, col_idx, row_ptr, m, n, nnz);                                                           \
      const Span op[3] = {Span(values, 1, nnz, nnz, "values"), Span(col_idx, 1, nnz, nnz, "col_idx"),                   \
                          Span(row_ptr, 1, m + 1, m + 1, "row_ptr")};                                                   \
      pca_transform_entry<HipDev, T>(cx.dev, c, true, op, 3, [&] {                                                      \
        pca_apply_stage::run_csr<T>(cx.dev, HOST, values, col_idx, row_ptr, nnz, c, &cx.pca_apply);                     \
      });                                                                                                               \
    });                                                                                                                 \
  }
#define CORRLA_DEFINE_PCA_INVERSE(NAME, T, HOST)                                                                        \
  CORRLA_API corrla_status NAME(corrla_ctx* ctx, const T* scores, int64_t m, int64_t k, int64_t ld_scores, const T* means, \
                                const T* scales, const T* components, int64_t ldc, int64_t n, T* out, int64_t row_stride_out) { \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      cx.pca_apply = pca_apply_stage::Ran();                                                                            \
      const PcaInverseCall<T> c{scores, m, k, ld_scores, means, scales, components, ldc, n, out, row_stride_out};       \
      pca_inverse_entry<HipDev, T>(cx.dev, c, [&] { pca_apply_stage::run_inverse<T>(cx.dev, HOST, c, &cx.pca_apply); }); \
    });                                                                                                                 \
  }
#define CORRLA_DEFINE_PCA_APPLY(SUF, T)                                  \
  CORRLA_DEFINE_PCA_TRANSFORM(corrla_pca_transform_##SUF, T, true)       \
  CORRLA_DEFINE_PCA_TRANSFORM(corrla_pca_transform_dev_##SUF, T, false)  \
  CORRLA_DEFINE_PCA_TRANSFORM_CSR(corrla_pca_transform_csr_##SUF, T, true)      \
  CORRLA_DEFINE_PCA_TRANSFORM_CSR(corrla_pca_transform_csr_dev_##SUF, T, false) \
  CORRLA_DEFINE_PCA_INVERSE(corrla_pca_inverse_##SUF, T, true)           \
  CORRLA_DEFINE_PCA_INVERSE(corrla_pca_inverse_dev_##SUF, T, false)
CORRLA_DEFINE_PCA_APPLY(f32, float)
CORRLA_DEFINE_PCA_APPLY(f64, double)
CORRLA_API corrla_status corrla_ctx_last_pca_apply(corrla_ctx* ctx, int* centring_out, int* route_out) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    std::lock_guard<std::mutex> lk(c->mu);
    if (centring_out) *centring_out = c->pca_apply.centring;
    if (route_out) *route_out = c->pca_apply.route;
  });
}

// ---- radial-basis-function kernel matrices (interp_utils.rs:96-129, 146-153) -----------------------------------------------
#define CORRLA_RBF_POINTS(T) const T *xq, int64_t n_q, int64_t ldq, const T *xs, int64_t n_s, int64_t lds, int64_t dim, int kernel, double eps
#define CORRLA_DEFINE_RBF(SUF, DEV, T, HOST)                                                                            \
  CORRLA_API corrla_status corrla_rbf_matrix_##DEV##SUF(corrla_ctx* ctx, CORRLA_RBF_POINTS(T), T* out, int64_t ld_out) { \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      const RbfCall<T> c{xq, n_q, ldq, xs, n_s, lds, dim, kernel, eps, -1, nullptr, 0, 0, out, ld_out};                 \
      rbf_matrix_entry<HipDev, T>(cx.dev, c, [&] { rbf_stage::run_matrix<T>(cx.dev, HOST, c); });                       \
    });                                                                                                                 \
  }                                                                                                                     \
  CORRLA_API corrla_status corrla_rbf_apply_##DEV##SUF(corrla_ctx* ctx, CORRLA_RBF_POINTS(T), int poly_degree, const T* coeffs, \
                                                       int64_t ldw, int64_t n_rhs, T* out, int64_t ld_out) {            \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      const RbfCall<T> c{xq, n_q, ldq, xs, n_s, lds, dim, kernel, eps, poly_degree, coeffs, ldw, n_rhs, out, ld_out};   \
      rbf_apply_entry<HipDev, T>(cx.dev, c, [&] { rbf_stage::run_apply<T>(cx.dev, HOST, c); });                         \
    });                                                                                                                 \
  }
CORRLA_DEFINE_RBF(f32, , float, true)
CORRLA_DEFINE_RBF(f64, , double, true)
CORRLA_DEFINE_RBF(f32, dev_, float, false)
CORRLA_DEFINE_RBF(f64, dev_, double, false)

// ---- polynomial response surfaces (linear_fit / quad_fit / quad_eval / jac_from_quad, stats_corr.rs:146-249) ---------------
#define CORRLA_DEFINE_POLYFIT(SUF, DEV, T, HOST)                                                                        \
  CORRLA_API corrla_status corrla_polyfit_gram_##DEV##SUF(corrla_ctx* ctx, const T* x, int64_t m, int64_t k, int64_t ldx, const T* y, \
                                                          int64_t r, int64_t ldy, int degree, int normalize, double* G, int64_t ldg, \
                                                          double* means, double* scales) {                               \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      cx.polyfit = polyfit_stage::Ran();                                                                                \
      const PolyGramCall<T> c{x, m, k, ldx, y, r, ldy, degree, normalize, G, ldg, means, scales};                       \
      polyfit_gram_entry<HipDev, T>(cx.dev, c, [&] { polyfit_stage::run_gram<T>(cx.dev, HOST, c, &cx.polyfit); });      \
    });                                                                                                                 \
  }                                                                                                                     \
  CORRLA_API corrla_status corrla_poly_eval_##DEV##SUF(corrla_ctx* ctx, const T* x, int64_t m, int64_t k, int64_t ldx,   \
                                                       const double* coeffs, int64_t ldc, int64_t r, int degree, T* out, \
                                                       int64_t ld_out, T* jac, int64_t ld_jac) {                         \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      cx.polyfit = polyfit_stage::Ran();                                                                                \
      const PolyEvalCall<T> c{x, m, k, ldx, coeffs, ldc, r, degree, out, ld_out, jac, ld_jac};                          \
      poly_eval_entry<HipDev, T>(cx.dev, c, [&] { polyfit_stage::run_eval<T>(cx.dev, HOST, c, &cx.polyfit); });         \
    });                                                                                                                 \
  }
CORRLA_DEFINE_POLYFIT(f32, , float, true)
CORRLA_DEFINE_POLYFIT(f64, , double, true)
CORRLA_DEFINE_POLYFIT(f32, dev_, float, false)
CORRLA_DEFINE_POLYFIT(f64, dev_, double, false)
CORRLA_API corrla_status corrla_ctx_last_polyfit(corrla_ctx* ctx, int* route_out) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    std::lock_guard<std::mutex> lk(c->mu);
    if (route_out) *route_out = c->polyfit.route;
  });
}

// ---- kernel density estimates (KdeRv::pdf / cdf, UniRv::nll, univariate_rv.rs:165-170, 423-444) ------------------------------
#define CORRLA_KDE_POINTS(T, N) const T *x, int64_t N, int64_t incx, const T *s, int64_t n_s, int64_t incs
#define CORRLA_DEFINE_KDE(SUF, DEV, T, HOST)                                                                            \
  CORRLA_API corrla_status corrla_kde_eval_##DEV##SUF(corrla_ctx* ctx, CORRLA_KDE_POINTS(T, n_q), double h, int what, T* out, \
                                                      int64_t inco) {                                                   \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      cx.kde = kde_stage::Ran();                                                                                        \
      const KdeEvalCall<T> c{x, n_q, incx, s, n_s, incs, h, what, out, inco};                                           \
      kde_eval_entry<HipDev, T>(cx.dev, c, [&] { kde_stage::run_eval<T>(cx.dev, HOST, c, &cx.kde); });                  \
    });                                                                                                                 \
  }                                                                                                                     \
  CORRLA_API corrla_status corrla_kde_nll_##DEV##SUF(corrla_ctx* ctx, CORRLA_KDE_POINTS(T, n_t), const double* h, int64_t n_h, \
                                                     double* nll, double* dnll) {                                       \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      cx.kde = kde_stage::Ran();                                                                                        \
      const KdeNllCall<T> c{x, n_t, incx, s, n_s, incs, h, n_h, nll, dnll};                                             \
      kde_nll_entry<HipDev, T>(cx.dev, c, [&] { kde_stage::run_nll<T>(cx.dev, HOST, c, &cx.kde); });                    \
    });                                                                                                                 \
  }
CORRLA_DEFINE_KDE(f32, , float, true)
CORRLA_DEFINE_KDE(f64, , double, true)
CORRLA_DEFINE_KDE(f32, dev_, float, false)
CORRLA_DEFINE_KDE(f64, dev_, double, false)
CORRLA_API corrla_status corrla_ctx_last_kde(corrla_ctx* ctx, int* route_out) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    std::lock_guard<std::mutex> lk(c->mu);
    if (route_out) *route_out = c->kde.route;
  });
}

// ---- constrained Dirichlet sampling (constr_dirichlet_sample, space_samplers.rs:14-126) -------------------------------------
#define CORRLA_DEFINE_DIRICHLET(DEV, HOST)                                                                              \
  CORRLA_API corrla_status corrla_dirichlet_draws_##DEV##f64(corrla_ctx* ctx, const double* alphas, int64_t d, double c_scale, \
                                                             uint64_t seed, int64_t first, int64_t n, double* out, int64_t ldo) { \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      const DirichletDrawsCall c{alphas, d, c_scale, seed, first, n, out, ldo};                                         \
      dirichlet_draws_entry<HipDev>(cx.dev, c, [&](const DirPlan& p) {                                                  \
        cx.dirichlet = dirichlet_stage::Ran();                                                                          \
        dirichlet_stage::run_draws(cx.dev, HOST, c, p, &cx.dirichlet);                                                  \
      });                                                                                                               \
    });                                                                                                                 \
  }                                                                                                                     \
  CORRLA_API corrla_status corrla_dirichlet_sample_##DEV##f64(corrla_ctx* ctx, const double* bounds, const double* alphas, int64_t d, \
                                                              double c_scale, uint64_t seed, int64_t n_samples, int64_t max_zshots, \
                                                              int64_t chunk_size, double* out, int64_t ldo, int64_t* n_found, \
                                                              int64_t* n_drawn) {                                        \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      const DirichletSampleCall c{bounds, alphas, d, c_scale, seed, n_samples, max_zshots, chunk_size, out, ldo, n_found, n_drawn}; \
      dirichlet_sample_entry<HipDev>(cx.dev, HOST, c, [&](const DirPlan& p) {                                           \
        cx.dirichlet = dirichlet_stage::Ran();                                                                          \
        dirichlet_stage::run_sample(cx.dev, HOST, c, p, &cx.dirichlet);                                                 \
      });                                                                                                               \
    });                                                                                                                 \
  }
CORRLA_DEFINE_DIRICHLET(, true)
CORRLA_DEFINE_DIRICHLET(dev_, false)
// route_out: the route (1 registers / exponential-only, 2 registers / general, 3 regenerate / exponential-only, 4 regenerate /
// general) in the low byte, the read-backs of the state the call made above it.  A rejected call leaves it as it was.
CORRLA_API corrla_status corrla_ctx_last_dirichlet(corrla_ctx* ctx, int* route_out) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    std::lock_guard<std::mutex> lk(c->mu);
    if (route_out) *route_out = c->dirichlet.route | (c->dirichlet.readbacks << 8);
  });
}

// ---- multivariate normal rows and sandwich variances (sample_mv_normal / sandwich_prop, stats_corr.rs:46-68) -----------------
#define CORRLA_DEFINE_MVN(DEV, SUF, T, HOST)                                                                            \
  CORRLA_API corrla_status corrla_mvn_sample_##DEV##SUF(corrla_ctx* ctx, int64_t n, int64_t d, int64_t r, const T* factor, int64_t ldf, \
                                                        const T* mean, uint64_t seed, int64_t first, int lower, T* out, int64_t ldo) { \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      const MvnSampleCall<T> c{n, d, r, factor, ldf, mean, seed, first, lower, out, ldo};                               \
      mvn_sample_entry<HipDev, T>(cx.dev, c, [&](const MvnPlan& p) {                                                    \
        cx.mvn = mvn_stage::Ran();                                                                                      \
        mvn_stage::run_sample<T>(cx.dev, HOST, c, p, &cx.mvn);                                                          \
      });                                                                                                               \
    });                                                                                                                 \
  }                                                                                                                     \
  CORRLA_API corrla_status corrla_sandwich_diag_##DEV##SUF(corrla_ctx* ctx, const T* jac, int64_t m, int64_t d, int64_t ldj, const T* cov, \
                                                           int64_t ldc, T* v) {                                         \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      const SandwichDiagCall<T> c{jac, m, d, ldj, cov, ldc, v};                                                         \
      sandwich_diag_entry<HipDev, T>(cx.dev, c, [&](const SandwichPlan& p) { mvn_stage::run_sandwich<T>(cx.dev, HOST, c, p); }); \
    });                                                                                                                 \
  }
CORRLA_DEFINE_MVN(, f32, float, true)
CORRLA_DEFINE_MVN(, f64, double, true)
CORRLA_DEFINE_MVN(dev_, f32, float, false)
CORRLA_DEFINE_MVN(dev_, f64, double, false)
// route_out: 1 fused, 2 staged, 3 no rows (nothing launched), 0 before the first call.  A rejected call leaves it as it was.
CORRLA_API corrla_status corrla_ctx_last_mvn(corrla_ctx* ctx, int* route_out) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    std::lock_guard<std::mutex> lk(c->mu);
    if (route_out) *route_out = c->mvn.route;
  });
}

// ---- dense LU solve (P A = L U, partial pivoting) and the RBF fit on it ---------------------------------------------------------
CORRLA_API corrla_status corrla_lu_solve_f64(corrla_ctx* ctx, const double* a, int64_t n, int64_t lda, const double* b, int64_t n_rhs,
                                             int64_t ldb, double* x, int64_t ldx) {
  return ctx_call(ctx, [&](corrla_ctx& cx) {
    const LuSolveCall c{a, n, lda, b, n_rhs, ldb, x, ldx, nullptr, nullptr, nullptr};
    lu_solve_entry<HipDev>(cx.dev, true, c, [&] {
      cx.lu = lu_stage::Ran();
      lu_stage::run_solve(cx.dev, true, c, &cx.lu);
    });
  });
}
CORRLA_API corrla_status corrla_lu_solve_dev_f64(corrla_ctx* ctx, double* a, int64_t n, int64_t lda, double* b, int64_t n_rhs, int64_t ldb,
                                                 int64_t* ipiv) {
  return ctx_call(ctx, [&](corrla_ctx& cx) {
    const LuSolveCall c{a, n, lda, b, n_rhs, ldb, nullptr, 0, a, b, ipiv};
    lu_solve_entry<HipDev>(cx.dev, false, c, [&] {
      cx.lu = lu_stage::Ran();
      lu_stage::run_solve(cx.dev, false, c, &cx.lu);
    });
  });
}
#define CORRLA_DEFINE_RBF_FIT(DEV, HOST)                                                                                \
  CORRLA_API corrla_status corrla_rbffit_system_##DEV##f64(corrla_ctx* ctx, const double* xs, int64_t n_s, int64_t ldxs, int64_t dim, \
                                                        int kernel, double eps, int poly_degree, double* m, int64_t ldm) { \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      const RbfFitCall c{xs, n_s, ldxs, dim, nullptr, 0, 0, kernel, eps, poly_degree, nullptr, 0, m, ldm};              \
      rbf_fit_entry<HipDev>(cx.dev, c, false, [&] { lu_stage::run_rbf_system(cx.dev, HOST, c); });                      \
    });                                                                                                                 \
  }                                                                                                                     \
  CORRLA_API corrla_status corrla_rbffit_##DEV##f64(corrla_ctx* ctx, const double* xs, int64_t n_s, int64_t ldxs, int64_t dim, \
                                                     const double* y, int64_t n_rhs, int64_t ldy, int kernel, double eps, \
                                                     int poly_degree, double* coeffs, int64_t ldw) {                    \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      const RbfFitCall c{xs, n_s, ldxs, dim, y, n_rhs, ldy, kernel, eps, poly_degree, coeffs, ldw, nullptr, 0};         \
      rbf_fit_entry<HipDev>(cx.dev, c, true, [&] {                                                                      \
        cx.lu = lu_stage::Ran();                                                                                        \
        lu_stage::run_rbf_fit(cx.dev, HOST, c, &cx.lu);                                                                 \
      });                                                                                                               \
    });                                                                                                                 \
  }
CORRLA_DEFINE_RBF_FIT(, true)
CORRLA_DEFINE_RBF_FIT(dev_, false)
// route: 1 small, 2 blocked, 0 before the first call; info, min_pivot, max_u: the status record of that call.  A call rejected
// for its arguments leaves them as they were; one that ended with CORRLA_ENUMERIC has set them.
CORRLA_API corrla_status corrla_ctx_last_solve(corrla_ctx* ctx, int* route, int64_t* info, double* min_pivot, double* max_u) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    std::lock_guard<std::mutex> lk(c->mu);
    if (route) *route = c->lu.route;
    if (info) *info = c->lu.info;
    if (min_pivot) *min_pivot = c->lu.min_pivot;
    if (max_u) *max_u = c->lu.max_u;
  });
}

// ---- dense Cholesky factor and SPD solve (A = L L^T over the lower triangle) ----------------------------------------------------
CORRLA_API corrla_status corrla_chol_factor_f64(corrla_ctx* ctx, const double* a, int64_t n, int64_t lda, double* l, int64_t ldl) {
  return ctx_call(ctx, [&](corrla_ctx& cx) {
    const CholFactorCall c{a, n, lda, l, ldl, nullptr};
    chol_factor_entry<HipDev>(cx.dev, true, c, [&] {
      cx.chol = chol_stage::Ran();
      chol_stage::run_factor(cx.dev, true, c, &cx.chol);
    });
  });
}
CORRLA_API corrla_status corrla_chol_factor_dev_f64(corrla_ctx* ctx, double* a, int64_t n, int64_t lda) {
  return ctx_call(ctx, [&](corrla_ctx& cx) {
    const CholFactorCall c{a, n, lda, nullptr, 0, a};
    chol_factor_entry<HipDev>(cx.dev, false, c, [&] {
      cx.chol = chol_stage::Ran();
      chol_stage::run_factor(cx.dev, false, c, &cx.chol);
    });
  });
}
CORRLA_API corrla_status corrla_chol_solve_f64(corrla_ctx* ctx, const double* a, int64_t n, int64_t lda, const double* b, int64_t n_rhs,
                                               int64_t ldb, double* x, int64_t ldx) {
  return ctx_call(ctx, [&](corrla_ctx& cx) {
    const LuSolveCall c{a, n, lda, b, n_rhs, ldb, x, ldx, nullptr, nullptr, nullptr};
    chol_solve_entry<HipDev>(cx.dev, true, c, [&] {
      cx.chol = chol_stage::Ran();
      chol_stage::run_solve(cx.dev, true, c, &cx.chol);
    });
  });
}
CORRLA_API corrla_status corrla_chol_solve_dev_f64(corrla_ctx* ctx, double* a, int64_t n, int64_t lda, double* b, int64_t n_rhs, int64_t ldb) {
  return ctx_call(ctx, [&](corrla_ctx& cx) {
    const LuSolveCall c{a, n, lda, b, n_rhs, ldb, nullptr, 0, a, b, nullptr};
    chol_solve_entry<HipDev>(cx.dev, false, c, [&] {
      cx.chol = chol_stage::Ran();
      chol_stage::run_solve(cx.dev, false, c, &cx.chol);
    });
  });
}
// route: 1 small, 2 blocked, 0 before the first call; info, min_diag, max_diag, logdet: the status record of that call.  A call
// rejected for its arguments leaves them as they were; one that ended with CORRLA_ENUMERIC has set them.
CORRLA_API corrla_status corrla_ctx_last_chol(corrla_ctx* ctx, int* route, int64_t* info, double* min_diag, double* max_diag, double* logdet) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    std::lock_guard<std::mutex> lk(c->mu);
    if (route) *route = c->chol.route;
    if (info) *info = c->chol.info;
    if (min_diag) *min_diag = c->chol.min_diag;
    if (max_diag) *max_diag = c->chol.max_diag;
    if (logdet) *logdet = c->chol.logdet;
  });
}

// ---- symmetric eigendecomposition (A = V diag(w) V^T over the lower triangle) -----------------------------------------------------
CORRLA_API corrla_status corrla_eigh_f64(corrla_ctx* ctx, const double* a, int64_t n, int64_t lda, double* w, double* v, int64_t ldv) {
  return ctx_call(ctx, [&](corrla_ctx& cx) {
    const EighCall c{a, n, lda, w, v, ldv};
    eigh_entry<HipDev>(cx.dev, c, [&] {
      cx.eigh = eigh_stage::Ran();
      eigh_stage::run(cx.dev, true, c, &cx.eigh);
    });
  });
}
CORRLA_API corrla_status corrla_eigh_dev_f64(corrla_ctx* ctx, const double* a, int64_t n, int64_t lda, double* w, double* v, int64_t ldv) {
  return ctx_call(ctx, [&](corrla_ctx& cx) {
    const EighCall c{a, n, lda, w, v, ldv};
    eigh_entry<HipDev>(cx.dev, c, [&] {
      cx.eigh = eigh_stage::Ran();
      eigh_stage::run(cx.dev, false, c, &cx.eigh);
    });
  });
}
// route: 1 small, 2 blocked, 0 before the first call; sweeps, off, shift, info: the record of that call.  A call rejected for its
// arguments leaves them as they were; one that ended with CORRLA_ENUMERIC has set them.
CORRLA_API corrla_status corrla_ctx_last_eigh(corrla_ctx* ctx, int* route, int* sweeps, double* off, double* shift, int64_t* info) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    std::lock_guard<std::mutex> lk(c->mu);
    if (route) *route = c->eigh.route;
    if (sweeps) *sweeps = c->eigh.sweeps;
    if (off) *off = c->eigh.off;
    if (shift) *shift = c->eigh.shift;
    if (info) *info = c->eigh.info;
  });
}

// ---- active-subspace gradient stage ------------------------------------------------------
#define CORRLA_DEFINE_GRAD(NAME, HOST)                                                                                  \
  CORRLA_API corrla_status NAME(corrla_ctx* ctx, const double* x, int64_t n_pts, int64_t k, const double* y, const double* xq, \
                                int64_t n_q, int est_order, int64_t n_nbrs, double out_scale, double* g, int64_t ldg,   \
                                int* n_regularised) {                                                                   \
    return ctx_call(ctx, [&](corrla_ctx& cx) {                                                                          \
      const GradMatCall c{x, n_pts, k, y, xq, n_q, est_order, n_nbrs, out_scale, g, ldg, n_regularised};                \
      grad_entry(cx.dev, c, [&] { grad_stage::run_entry(cx.dev, HOST, c, &cx.last); });                                 \
    });                                                                                                                 \
  }
CORRLA_DEFINE_GRAD(corrla_grad_mat_f64, true)
CORRLA_DEFINE_GRAD(corrla_grad_mat_dev_f64, false)

CORRLA_API corrla_status corrla_comm_unique_id(void* out128) {
  return guarded([&] {
    if (!out128) throw Error(ST_EINVAL, "out128 is NULL");
    ncclUniqueId id;
    CORRLA_NCCL(ncclGetUniqueId(&id));
    std::memset(out128, 0, CORRLA_UNIQUE_ID_BYTES);
    std::memcpy(out128, &id, sizeof(id));
  });
}
CORRLA_API corrla_status corrla_ctx_comm_init(corrla_ctx* ctx, const void* unique_id128, int rank, int nranks) {
  return guarded([&] {
    corrla_ctx* c = need(ctx);
    if (!unique_id128 || nranks < 1 || rank < 0 || rank >= nranks) throw Error(ST_EINVAL, "bad communicator arguments");
    std::lock_guard<std::mutex> lk(c->mu);
    c->dev.comm_init(unique_id128, rank, nranks);
  });
}

}  // extern "C"
