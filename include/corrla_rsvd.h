/*
 * corrla_rsvd.h -- C ABI of libcorrla_rsvd.so, the MI355X (gfx950) randomized-SVD engine
 * that drops in behind the RSVD hot path of wgurecky/CORRLA_RS.
 *
 * Every entry point cites the reference interface it replaces (paths relative to the
 * reference checkout).  Signatures use plain pointers and sizes only (no C++/torch types),
 * so the Rust shim, the Python `corrla_rs` module (ctypes) and bench.py
 * bind the same symbols.
 *
 * Conventions
 *   - Input A is described exactly like a faer `MatRef<T>`: (ptr, nrows, ncols, row_stride,
 *     col_stride), strides in ELEMENTS.  numpy C-order arrives as (rs=n, cs=1); a native faer
 *     `Mat` is column-major (rs=1, cs=m).  A is never modified.
 *   - Outputs are column-major like the reference's owned `Mat<T>` results
 *     (random_svd.rs:96-109): U m x k (leading dim ldu >= m), S k values (the k x 1 column),
 *     Vt k x n (leading dim ldvt >= k).  The caller allocates them.
 *   - l = min(rank + n_oversamples, min(m, n))   (random_svd.rs:77)
 *   - Signs: the reference returns whatever signs faer's SVD produced.  Here every triplet (u_i, s_i, v_i)
 *     is normalised so that the largest-magnitude component (first on ties) of the SHORT-side singular
 *     vector (length min(m, n): v_i for tall A, u_i for fat A) is positive.
 *   - Every function returns a corrla_status; corrla_last_error() gives the thread-local
 *     message.  The reference panics instead (random_svd.rs:98-107, mat_utils.rs:170-171).
 *   - `_dev` variants take DEVICE pointers (HIP) for A and the outputs and enqueue on the
 *     context's stream; host variants copy H2D/D2H around the same device path.
 *   - There is NO CPU fallback: without a usable gfx950 device every compute entry point
 *     fails with CORRLA_ENODEV.
 */
#ifndef CORRLA_RSVD_H
#define CORRLA_RSVD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Only the C ABI below is exported; every C++ symbol of the library has hidden visibility. */
#if defined(__GNUC__)
#define CORRLA_API __attribute__((visibility("default")))
#else
#define CORRLA_API
#endif

typedef struct corrla_ctx corrla_ctx;

typedef enum corrla_status {
  CORRLA_OK = 0,
  CORRLA_EINVAL = 1,   /* bad argument (rank == 0, rank > min(m,n), null pointer, bad stride ...) */
  CORRLA_ENOMEM = 2,   /* host or device allocation failed */
  CORRLA_EHIP = 3,     /* HIP runtime error */
  CORRLA_ECOMM = 4,    /* RCCL error / communicator not initialised */
  CORRLA_ENUMERIC = 5, /* non-finite data encountered in the small host factorizations */
  CORRLA_ENODEV = 6    /* no usable gfx950 device */
} corrla_status;

/* opts.flags */
#define CORRLA_OMEGA_ON_DEVICE 0x1u /* opts.omega is a device pointer (only for *_dev entry points) */
/* corrla_pca_*: how the column centring of center_mat_col (mat_utils.rs:482-502) is applied.
 * FUSED: the matrix is never rewritten; every product with the centred matrix is corrected by a rank-1 term,
 *        (A - 1 mu^T) X = A X - 1 (mu^T X), (A - 1 mu^T)^T Y = A^T Y - mu (1^T Y)  (SURVEY section 8 f1).
 * COPY : a centred copy is formed first, as the reference does (one more m x n buffer).
 * Default (neither flag): FUSED for f64, COPY for f32 (the fused form cancels digits when |mean| >> spread). */
#define CORRLA_PCA_CENTER_FUSED 0x2u
#define CORRLA_PCA_CENTER_COPY 0x4u
/* Thin-Q of the sketch (`y_mat.qr().compute_thin_q()`, random_svd.rs:38,57) by Householder TSQR with an explicit Q
 * (row panels reduced in LDS, pairwise tree over the R factors, reflectors applied in reverse) instead of the default
 * CholeskyQR2.  One panel holds l = min(rank + n_oversamples, n) <= 142 (f32) / 99 (f64) columns; wider sketches go
 * through column blocks of that width (projection against the finished blocks + panel, repeated).  On the row-sharded
 * entry points every rank reduces its rows, the root R factors are exchanged (one all-reduce of an nranks * l x l
 * buffer) and their stack is reduced redundantly; a call in which some shard has fewer than l rows keeps the default
 * path.  The environment variable CORRLA_QR=householder sets the flag for every call. */
#define CORRLA_QR_HOUSEHOLDER 0x8u
/* opts.seed is to be used as given even when it is 0.  Without this flag seed == 0 (and opts == NULL) means "no seed":
 * the library then draws a fresh sketch on every call, like the reference's unseeded thread_rng
 * (mat_utils.rs:161-175); on the row-sharded entry points that fresh seed is a function of the number of seedless
 * sharded calls made on the context only, so every rank draws the same Omega. */
#define CORRLA_SEED_EXPLICIT 0x10u
/* One-sweep power iteration: for a row-major f32 A with at most 512 columns, the pair
 * Y = A X, Z = A^T Y of random_svd.rs:42-51 (and of the sketch, :31) is computed as Z = A^T (A X) from ONE pass over A
 * with the 32-row tile of A held in LDS, wherever Y itself is not needed (the iterations without the in-loop thin-Q).
 * Same result up to rounding (the intermediate stays in f32 registers instead of being rounded to memory).  Other
 * shapes / dtypes / layouts ignore the flag.  The environment variable CORRLA_POWER_FUSED=1 sets it for every call. */
#define CORRLA_POWER_FUSED 0x20u
/* corrla_rsvd_sharded_dev_*: the local block is a COLUMN shard (m x n_local) of a fat matrix (m < sum of n_local)
 * instead of a row shard of a tall one.  The algorithm works on the tall view A^T (random_svd.rs:69-74), whose row shard
 * is this block transposed (a stride swap).  Outputs: U m x rank and S replicated on every rank, Vt rank x n_local =
 * this rank's columns of V^T.  opts->omega, when given, is m x l (the short side). */
#define CORRLA_SHARD_COLS 0x40u
/* Mixed-precision tall products (f32 row-major inputs, l <= 144; ignored elsewhere): the
 * products of the whole matrix with an l-wide factor -- power_iter's Y = A Omega, Z = A^T Y, Y = A Z (random_svd.rs:31,
 * 42-51) and the projection B = Q^T A (:80; CORRLA_MIXED_PROJECT=0 keeps that one exact) -- run on the bf16 matrix units
 * with an f32 accumulator, each f32 operand split on the fly into bf16 pieces whose products are exact in f32:
 *   BF16X6: three pieces (24 bits), six products -- the f32 product to f32 rounding (measured 3.5e-7 relative against
 *           3.2e-7 for the exact kernel) at 16/6 of the exact-f32 MFMA rate;
 *   BF16X3: two pieces (16 bits), three products -- 4.5e-6 relative, twice that rate again.
 * The thin-Qs, the core SVD and U = Q U~ stay in exact f32.  Off by default (the exact f32 path is the reference's
 * arithmetic); measured effect on the result: profiles/r03_mixed_accuracy.jsonl, DESIGN.md section 3.  The environment
 * variable CORRLA_SKETCH_MIXED=bf16x3|bf16x6 sets it for every call.  Mutually exclusive. */
#define CORRLA_SKETCH_BF16X3 0x80u
#define CORRLA_SKETCH_BF16X6 0x100u
/* corrla_pca_* (every entry: dense host / device, sharded, bf16, CSR): PCA on STANDARDISED columns -- every column is
 * divided by its sample standard deviation after centring, i.e. PCA of the correlation matrix (scikit-learn's
 * StandardScaler -> PCA, R's prcomp(scale. = TRUE)).  x is never rewritten: one more pass over it, next to the one for the
 * means, gives ss_j = sum_i (x_ij - mu_j)^2 (centred two-pass form, f64 accumulation, fixed summation order), then
 *   sd_j = sqrt(ss_j / (n_samples - 1))          (the divisor of explained_var, pca_rsvd.rs:91-99),
 * and the fused centring carries the diagonal D^-1 = diag(1 / sd) on the skinny side of every product,
 *   ((A - 1 mu^T) D^-1) X = A (D^-1 X) - 1 (mu^T D^-1 X),   ((A - 1 mu^T) D^-1)^T Y = D^-1 (A^T Y - mu (1^T Y)),
 * (fat input: the mirrored pair); CORRLA_PCA_CENTER_COPY forms the centred and scaled copy instead.  The
 * CORRLA_PCA_CENTER_* flags and their defaults keep their meaning.  A column that cannot be told from a constant one
 * (ss_j / m <= m eps ss_j / m + (m mu_j eps)^2, eps of the output type: scikit-learn's rule) gets sd_j = 1 and contributes
 * exact zeros.  The components are directions in standardised coordinates; corrla_opts.scales_out receives sd.
 * A bf16 operand that is read in place stays in place; CSR input is never densified (the implicit zeros are counted);
 * the sample-sharded entries add one all-reduce of n_dim doubles.  On any other entry point: CORRLA_EINVAL. */
#define CORRLA_PCA_STANDARDIZE 0x200u

/*
 * Options block.  Zero-initialise, set struct_size = sizeof(corrla_opts).  NULL opts == defaults.
 *   seed   : seed of the device Philox4x32-10 + Box-Muller generator that replaces
 *            random_mat_normal (mat_utils.rs:161-175; the reference draws from an unseeded
 *            thread_rng, so no seed value can reproduce it -- any N(0,1) draw is equivalent).
 *            A given seed makes the call deterministic; 0 without CORRLA_SEED_EXPLICIT = fresh draw per call.
 *   omega  : optional sketch matrix that replaces the draw at random_svd.rs:24 -- column-major
 *            n_t x l, n_t = min(m, n), leading dimension omega_ld (>= n_t), dtype of A.
 *            This is the test hook that lets the CPU oracle and the GPU share one Omega.
 *   scales_out : optional (may be NULL); written only with CORRLA_PCA_STANDARDIZE: the n_dim column standard
 *            deviations the columns were divided by (1 for a constant column), dtype of the outputs, host or device
 *            memory exactly as `means` is for that entry.
 * The struct grows at the end only.  struct_size == 32 (the layout through omega_ld, the first release of this header) is
 * accepted as well: the later fields then read as zero, so a caller built against that header keeps working.
 */
typedef struct corrla_opts {
  uint32_t struct_size;
  uint32_t flags;
  uint64_t seed;
  const void* omega;
  int64_t omega_ld;
  void* scales_out;
} corrla_opts;

/* Phase timings of the last rsvd / pca call on a context, milliseconds of DEVICE time: hipEvents are recorded on the
 * context's stream at the phase boundaries and resolved after the call has completed (no synchronisation inside the
 * call; replaces the SystemTime prints of random_svd.rs:125-140).  The phases add up to total_ms. */
typedef struct corrla_timings {
  double total_ms;      /* first to last event of the call */
  double sketch_ms;     /* Omega draw, Y = A*Omega            random_svd.rs:24,31   */
  double power_ms;      /* q x {Z = A^T Y, Y = A Z, norm}    random_svd.rs:35-56   */
  double qr_ms;         /* thin-Q orthonormalisations        random_svd.rs:38,57   */
  double project_ms;    /* B = Q^T A                         random_svd.rs:80      */
  double small_svd_ms;  /* svd of the l-wide core            random_svd.rs:89      */
  double finalize_ms;   /* U = Q*Ut, signs, output copies    random_svd.rs:92-109  */
  int32_t qr_passes;    /* Gram/whitening passes used by all orthonormalisations */
  int32_t n_collectives; /* all-reduces this rank issued during the call (row-sharded entry points; else 0) */
  double sketch_kernel_ms; /* device time of the sketch GEMM launch(es) of this call: hipEvents recorded on the
                              context's stream around Y = A*Omega (no extra synchronisation) */
  double host_enqueue_ms;  /* host wall clock spent enqueueing the call: the host runs ahead of the device */
  double collective_bytes; /* payload bytes of those all-reduces (n x l factors, l x l Gram matrices, scalars) */
  int32_t n_mixed_products; /* tall products of this call that ran on the bf16-split kernels (CORRLA_SKETCH_BF16X3 / X6) */
  int32_t n_bf16_products;  /* tall products of this call that ran on the bf16-input kernel (corrla_*_bf16); 0 when the call was widened */
  double knn_ms;        /* corrla_grad_mat_*: device time of the neighbour scan (hipEvents around its launches) */
  double fit_ms;        /* corrla_grad_mat_*: device time of the local least-squares fits; both 0 after any other call */
} corrla_timings;

/* ---- library / context ------------------------------------------------------------- */

/* "corrla_rsvd <version> gfx950" */
CORRLA_API const char* corrla_version(void);
/* thread-local message of the last failing call on this thread */
CORRLA_API const char* corrla_last_error(void);
/* number of visible HIP devices (0 when none / no driver) */
CORRLA_API int corrla_device_count(void);

/* One context = one device, one stream, one workspace arena (and optionally one RCCL
 * communicator).  Replaces faer's process-global Parallelism (mat_utils.rs:31,
 * random_svd.rs:122).  Calls on one context serialise. */
CORRLA_API corrla_status corrla_ctx_create(int device_ordinal, corrla_ctx** out);
CORRLA_API void corrla_ctx_destroy(corrla_ctx* ctx);
CORRLA_API corrla_status corrla_ctx_synchronize(corrla_ctx* ctx);
/* Per-phase device times cost one hipEvent record per phase boundary (~5 us of idle GPU each, 7 per call).  on = 0:
 * only total_ms, sketch_kernel_ms, the counters and host_enqueue_ms are filled in, the *_ms of the phases read 0.
 * Default: on.  (The reference prints wall-clock phase times unconditionally, random_svd.rs:125-140.) */
CORRLA_API corrla_status corrla_ctx_set_phase_timings(corrla_ctx* ctx, int on);
CORRLA_API corrla_status corrla_ctx_get_timings(corrla_ctx* ctx, corrla_timings* out);
/* Rank and size of the context's RCCL communicator as RCCL reports them (ncclCommUserRank / ncclCommCount);
 * nranks = 0 when corrla_ctx_comm_init has not been called. */
CORRLA_API corrla_status corrla_ctx_comm_info(corrla_ctx* ctx, int* rank, int* nranks);

/* ---- the hot path: random_svd -------------------------------------------------------
 * Replaces  pub fn random_svd<T>(a_mat: MatRef<T>, omega_rank, n_iter, n_oversamples)
 *             -> (Mat<T>, Mat<T>, Mat<T>)                      src/lib_math_utils/random_svd.rs:63-110
 * and, through it, the pyo3 surface corrla_rs.rsvd(a, n_rank, n_iters, n_oversamples)
 *                                                              src/lib_math_utils_py.rs:21-36
 * Host-pointer variants (A, U, S, Vt, opts->omega in host memory). */
CORRLA_API corrla_status corrla_rsvd_f32(corrla_ctx* ctx, const float* a, int64_t m, int64_t n, int64_t row_stride,
                              int64_t col_stride, int64_t rank, int64_t n_iter, int64_t n_oversamples,
                              const corrla_opts* opts, float* u, int64_t ldu, float* s, float* vt, int64_t ldvt);
CORRLA_API corrla_status corrla_rsvd_f64(corrla_ctx* ctx, const double* a, int64_t m, int64_t n, int64_t row_stride,
                              int64_t col_stride, int64_t rank, int64_t n_iter, int64_t n_oversamples,
                              const corrla_opts* opts, double* u, int64_t ldu, double* s, double* vt, int64_t ldvt);
/* Device-pointer variants: A, U, S, Vt are HIP device pointers on the context's device. */
CORRLA_API corrla_status corrla_rsvd_dev_f32(corrla_ctx* ctx, const float* a, int64_t m, int64_t n, int64_t row_stride,
                                  int64_t col_stride, int64_t rank, int64_t n_iter, int64_t n_oversamples,
                                  const corrla_opts* opts, float* u, int64_t ldu, float* s, float* vt, int64_t ldvt);
CORRLA_API corrla_status corrla_rsvd_dev_f64(corrla_ctx* ctx, const double* a, int64_t m, int64_t n, int64_t row_stride,
                                  int64_t col_stride, int64_t rank, int64_t n_iter, int64_t n_oversamples,
                                  const corrla_opts* opts, double* u, int64_t ldu, double* s, double* vt, int64_t ldvt);

/* ---- PCA caller ---------------------------------------------------
 * Replaces  PcaRsvd::new(x_mat, rank)                           src/lib_math_utils/pca_rsvd.rs:56-82
 *   means = mat_mean(x, 1); cx = center_mat_col(x); (_, s, vt) = random_svd(cx, rank, n_iter, n_oversamples)
 * and pyo3  rpca(a, n_rank, n_iters, n_oversamples)             src/lib_math_utils_py.rs:38-55
 * The reference hard-codes n_iter = 20, n_oversamples = min(n, 10) (pca_rsvd.rs:65-66; rpca ignores its last two
 * arguments); this ABI takes them explicitly and the Rust / Python shims pass the reference's values.
 * x: n_samples x n_dim, strided like a MatRef.  Outputs: means (n_dim values), s (rank values, the k x 1
 * column), components (rank x n_dim, column-major, leading dimension ldc >= rank).  The centred matrix is
 * formed on the device (one extra read + write of x); the columns' means come from the same MFMA kernel as
 * A^T Y.  Host-pointer and device-pointer variants. */
CORRLA_API corrla_status corrla_pca_f32(corrla_ctx* ctx, const float* x, int64_t n_samples, int64_t n_dim,
                                        int64_t row_stride, int64_t col_stride, int64_t rank, int64_t n_iter,
                                        int64_t n_oversamples, const corrla_opts* opts, float* means, float* s,
                                        float* components, int64_t ldc);
CORRLA_API corrla_status corrla_pca_f64(corrla_ctx* ctx, const double* x, int64_t n_samples, int64_t n_dim,
                                        int64_t row_stride, int64_t col_stride, int64_t rank, int64_t n_iter,
                                        int64_t n_oversamples, const corrla_opts* opts, double* means, double* s,
                                        double* components, int64_t ldc);
CORRLA_API corrla_status corrla_pca_dev_f32(corrla_ctx* ctx, const float* x, int64_t n_samples, int64_t n_dim,
                                            int64_t row_stride, int64_t col_stride, int64_t rank, int64_t n_iter,
                                            int64_t n_oversamples, const corrla_opts* opts, float* means, float* s,
                                            float* components, int64_t ldc);
CORRLA_API corrla_status corrla_pca_dev_f64(corrla_ctx* ctx, const double* x, int64_t n_samples, int64_t n_dim,
                                            int64_t row_stride, int64_t col_stride, int64_t rank, int64_t n_iter,
                                            int64_t n_oversamples, const corrla_opts* opts, double* means, double* s,
                                            double* components, int64_t ldc);
/* Sample-sharded PCA (one process per GPU, communicator from corrla_ctx_comm_init): x holds THIS rank's samples
 * (m_local x n_dim); the column means are all-reduced partial sums over the global sample count, and both centring
 * forms work unchanged (the rank-1 corrections of the fused form are linear in the rows: each rank corrects its own
 * partial product before the all-reduce).  means, s and components come out replicated on every rank. */
CORRLA_API corrla_status corrla_pca_sharded_dev_f32(corrla_ctx* ctx, const float* x, int64_t m_local, int64_t n, int64_t row_stride,
                                         int64_t col_stride, int64_t rank, int64_t n_iter, int64_t n_oversamples,
                                         const corrla_opts* opts, float* means, float* s, float* components, int64_t ldc);
CORRLA_API corrla_status corrla_pca_sharded_dev_f64(corrla_ctx* ctx, const double* x, int64_t m_local, int64_t n, int64_t row_stride,
                                         int64_t col_stride, int64_t rank, int64_t n_iter, int64_t n_oversamples,
                                         const corrla_opts* opts, double* means, double* s, double* components, int64_t ldc);

/* ---- the range finder: power_iter ---------------------------------------------------
 * Replaces  pub fn power_iter<T>(a_mat: MatRef<T>, omega_rank, n_iter) -> Mat<T>
 *                                                              src/lib_math_utils/random_svd.rs:15-59
 * `width` is the ALREADY OVERSAMPLED sketch width (the reference's `omega_rank` argument of
 * power_iter), width <= n.  Q: column-major m x width, leading dimension ldq.  Requires m >= 1,
 * n >= 1 (no fat->tall transpose here, exactly as in the reference). */
CORRLA_API corrla_status corrla_power_iter_f32(corrla_ctx* ctx, const float* a, int64_t m, int64_t n, int64_t row_stride,
                                    int64_t col_stride, int64_t width, int64_t n_iter, const corrla_opts* opts,
                                    float* q, int64_t ldq);
CORRLA_API corrla_status corrla_power_iter_f64(corrla_ctx* ctx, const double* a, int64_t m, int64_t n, int64_t row_stride,
                                    int64_t col_stride, int64_t width, int64_t n_iter, const corrla_opts* opts,
                                    double* q, int64_t ldq);
CORRLA_API corrla_status corrla_power_iter_dev_f32(corrla_ctx* ctx, const float* a, int64_t m, int64_t n, int64_t row_stride,
                                        int64_t col_stride, int64_t width, int64_t n_iter, const corrla_opts* opts,
                                        float* q, int64_t ldq);
CORRLA_API corrla_status corrla_power_iter_dev_f64(corrla_ctx* ctx, const double* a, int64_t m, int64_t n, int64_t row_stride,
                                        int64_t col_stride, int64_t width, int64_t n_iter, const corrla_opts* opts,
                                        double* q, int64_t ldq);

/* ---- the GEMM shim: par_matmul_helper -----------------------------------------------
 * Replaces  par_matmul_helper(res, lhs, rhs, beta, n_threads)  src/lib_math_utils/mat_utils.rs:20-33
 * for the two shapes the hot path uses it with (random_svd.rs:42-51): a large strided
 * matrix A (m x n, any of the two unit-stride layouts) times / transposed-times a skinny
 * column-major matrix.  res is OVERWRITTEN (alpha = None), res = beta * op(A) * X.
 *   trans == 0 : res (m x l) = beta * A   * X (n x l)
 *   trans == 1 : res (n x l) = beta * A^T * X (m x l)
 * X and res are column-major with leading dimensions ldx / ldres.  DEVICE pointers. */
CORRLA_API corrla_status corrla_matmul_dev_f32(corrla_ctx* ctx, int trans, const float* a, int64_t m, int64_t n,
                                    int64_t row_stride, int64_t col_stride, const float* x, int64_t ldx, int64_t l,
                                    float beta, float* res, int64_t ldres);
CORRLA_API corrla_status corrla_matmul_dev_f64(corrla_ctx* ctx, int trans, const double* a, int64_t m, int64_t n,
                                    int64_t row_stride, int64_t col_stride, const double* x, int64_t ldx, int64_t l,
                                    double beta, double* res, int64_t ldres);

/* ---- dense bfloat16 input -------------------------------------------------------------
 * random_svd, PcaRsvd::new and the product hook for a dense matrix STORED in bfloat16 (the upper 16 bits of an IEEE
 * binary32; torch.bfloat16).  A is `const uint16_t*` (bit patterns), strides in ELEMENTS; every other pointer -- U, S,
 * Vt, means, components, Omega (corrla_opts.omega), x, res -- is float, with the shapes and layouts of the f32 entries.
 * The result is what the f32 entry gives on the same matrix widened to float, to f32 rounding: the products accumulate
 * in f32 and the skinny operand keeps all 24 bits (three bf16 pieces).
 * When the memory rows of the tall view have unit stride, a 16-byte aligned base, a leading dimension and a length
 * that are multiples of 8 elements, and l = min(rank + n_oversamples, min(m, n)) <= 144, both tall products of the call
 * read A in place at 2 bytes per element and A is never copied or widened; corrla_timings.n_bf16_products counts them.
 * Any other call (and CORRLA_PCA_CENTER_COPY) widens A once into an f32 workspace and runs as the f32 call
 * (n_bf16_products == 0); a call is never half and half.  corrla_pca_*_bf16 defaults to CORRLA_PCA_CENTER_FUSED.
 * CORRLA_QR_HOUSEHOLDER is honoured; CORRLA_POWER_FUSED and CORRLA_SKETCH_BF16X3 / X6 are ignored, as for every operand
 * outside their domain.  The host-pointer entries stage the 2-byte matrix (H2D of 2 bytes per element).
 * No sharded variants and no power_iter variant. */
CORRLA_API corrla_status corrla_rsvd_bf16(corrla_ctx* ctx, const uint16_t* a, int64_t m, int64_t n, int64_t row_stride,
                                    int64_t col_stride, int64_t rank, int64_t n_iter, int64_t n_oversamples,
                                    const corrla_opts* opts, float* u, int64_t ldu, float* s, float* vt, int64_t ldvt);
CORRLA_API corrla_status corrla_rsvd_dev_bf16(corrla_ctx* ctx, const uint16_t* a, int64_t m, int64_t n, int64_t row_stride,
                                    int64_t col_stride, int64_t rank, int64_t n_iter, int64_t n_oversamples,
                                    const corrla_opts* opts, float* u, int64_t ldu, float* s, float* vt, int64_t ldvt);
CORRLA_API corrla_status corrla_pca_bf16(corrla_ctx* ctx, const uint16_t* x, int64_t n_samples, int64_t n_dim, int64_t row_stride,
                                    int64_t col_stride, int64_t rank, int64_t n_iter, int64_t n_oversamples,
                                    const corrla_opts* opts, float* means, float* s, float* components, int64_t ldc);
CORRLA_API corrla_status corrla_pca_dev_bf16(corrla_ctx* ctx, const uint16_t* x, int64_t n_samples, int64_t n_dim, int64_t row_stride,
                                    int64_t col_stride, int64_t rank, int64_t n_iter, int64_t n_oversamples,
                                    const corrla_opts* opts, float* means, float* s, float* components, int64_t ldc);
/* res = beta * op(A) * X as corrla_matmul_dev_f32, A in bfloat16, X and res float.  DEVICE pointers. */
CORRLA_API corrla_status corrla_matmul_dev_bf16(corrla_ctx* ctx, int trans, const uint16_t* a, int64_t m, int64_t n,
                                    int64_t row_stride, int64_t col_stride, const float* x, int64_t ldx, int64_t l,
                                    float beta, float* res, int64_t ldres);

/* ---- CSR sparse input ----------------------------------------------------------------
 * random_svd (random_svd.rs:63-110) and PcaRsvd::new (pca_rsvd.rs:56-82) for a matrix that is not dense: the
 * reference takes a dense faer Mat only; its own comparator in examples/benchmark_rsvd.py
 * (sklearn.utils.extmath.randomized_svd) accepts sparse input, and this is that surface.  A (m x n) is given in CSR:
 *   values  : nnz entries
 *   col_idx : nnz column indices, int32, each in [0, n)
 *   row_ptr : m + 1 offsets, int64, row_ptr[0] == 0, non-decreasing, row_ptr[m] == nnz
 * Column indices need not be sorted within a row; duplicate entries add.  The two products of the range finder
 * (random_svd.rs:31, 42-51, 80) are row gathers over A and over a CSR of A^T that the call builds once on the
 * device; A is never densified.  The arrays are validated ON THE DEVICE before anything is gathered through them: a
 * violation returns CORRLA_EINVAL (message in corrla_last_error()).  Outputs, l = min(rank + n_oversamples, min(m, n)),
 * the fat (m < n) handling, the sign convention and the status codes are those of corrla_rsvd_* / corrla_pca_*.
 * opts: seed, omega, CORRLA_OMEGA_ON_DEVICE, CORRLA_SEED_EXPLICIT and CORRLA_QR_HOUSEHOLDER work unchanged;
 * CORRLA_POWER_FUSED and CORRLA_SKETCH_BF16X3 / X6 are ignored.  Results are bitwise reproducible for a fixed seed (no
 * floating-point atomics; sums run in stored order within a row).
 * Limits: m, n < 2^31; 1 <= nnz < 2^31 -- an all-zero matrix (nnz == 0) returns CORRLA_EINVAL.  No sharded variant.
 * The *_dev variants take HIP device pointers for the three arrays and every output. */
CORRLA_API corrla_status corrla_rsvd_csr_f32(corrla_ctx* ctx, const float* values, const int32_t* col_idx,
                                    const int64_t* row_ptr, int64_t m, int64_t n, int64_t nnz, int64_t rank,
                                    int64_t n_iter, int64_t n_oversamples, const corrla_opts* opts, float* u, int64_t ldu,
                                    float* s, float* vt, int64_t ldvt);
CORRLA_API corrla_status corrla_rsvd_csr_dev_f32(corrla_ctx* ctx, const float* values, const int32_t* col_idx,
                                    const int64_t* row_ptr, int64_t m, int64_t n, int64_t nnz, int64_t rank,
                                    int64_t n_iter, int64_t n_oversamples, const corrla_opts* opts, float* u, int64_t ldu,
                                    float* s, float* vt, int64_t ldvt);
CORRLA_API corrla_status corrla_rsvd_csr_f64(corrla_ctx* ctx, const double* values, const int32_t* col_idx,
                                    const int64_t* row_ptr, int64_t m, int64_t n, int64_t nnz, int64_t rank,
                                    int64_t n_iter, int64_t n_oversamples, const corrla_opts* opts, double* u, int64_t ldu,
                                    double* s, double* vt, int64_t ldvt);
CORRLA_API corrla_status corrla_rsvd_csr_dev_f64(corrla_ctx* ctx, const double* values, const int32_t* col_idx,
                                    const int64_t* row_ptr, int64_t m, int64_t n, int64_t nnz, int64_t rank,
                                    int64_t n_iter, int64_t n_oversamples, const corrla_opts* opts, double* u, int64_t ldu,
                                    double* s, double* vt, int64_t ldvt);

/* PCA of CSR data (pca_rsvd.rs:56-82): the centring of center_mat_col (mat_utils.rs:482-502) is ALWAYS applied as
 * implicit rank-1 corrections (CORRLA_PCA_CENTER_FUSED; the means are A^T 1 / n_samples through the same gather), so
 * the matrix stays sparse.  CORRLA_PCA_CENTER_COPY returns CORRLA_EINVAL: a centred copy would densify the matrix. */
CORRLA_API corrla_status corrla_pca_csr_f32(corrla_ctx* ctx, const float* values, const int32_t* col_idx,
                                    const int64_t* row_ptr, int64_t n_samples, int64_t n_dim, int64_t nnz, int64_t rank,
                                    int64_t n_iter, int64_t n_oversamples, const corrla_opts* opts, float* means,
                                    float* s, float* components, int64_t ldc);
CORRLA_API corrla_status corrla_pca_csr_dev_f32(corrla_ctx* ctx, const float* values, const int32_t* col_idx,
                                    const int64_t* row_ptr, int64_t n_samples, int64_t n_dim, int64_t nnz, int64_t rank,
                                    int64_t n_iter, int64_t n_oversamples, const corrla_opts* opts, float* means,
                                    float* s, float* components, int64_t ldc);
CORRLA_API corrla_status corrla_pca_csr_f64(corrla_ctx* ctx, const double* values, const int32_t* col_idx,
                                    const int64_t* row_ptr, int64_t n_samples, int64_t n_dim, int64_t nnz, int64_t rank,
                                    int64_t n_iter, int64_t n_oversamples, const corrla_opts* opts, double* means,
                                    double* s, double* components, int64_t ldc);
CORRLA_API corrla_status corrla_pca_csr_dev_f64(corrla_ctx* ctx, const double* values, const int32_t* col_idx,
                                    const int64_t* row_ptr, int64_t n_samples, int64_t n_dim, int64_t nnz, int64_t rank,
                                    int64_t n_iter, int64_t n_oversamples, const corrla_opts* opts, double* means,
                                    double* s, double* components, int64_t ldc);

/* The sparse twin of corrla_matmul_dev_* (par_matmul_helper, mat_utils.rs:20-33), a test hook:
 *   trans == 0 : res (m x l) = beta * A   * X (n x l)
 *   trans == 1 : res (n x l) = beta * A^T * X (m x l)
 * A in CSR as above; X and res column-major with leading dimensions ldx / ldres.  DEVICE pointers.  res is the
 * destination of the SpMM kernels themselves: only rows [0, m or n) of its l columns are written, whatever else the
 * caller's buffer holds (rows up to ldres, further columns) is left as it was. */
CORRLA_API corrla_status corrla_spmm_csr_dev_f32(corrla_ctx* ctx, int trans, const float* values, const int32_t* col_idx,
                                    const int64_t* row_ptr, int64_t m, int64_t n, int64_t nnz, const float* x,
                                    int64_t ldx, int64_t l, float beta, float* res, int64_t ldres);
CORRLA_API corrla_status corrla_spmm_csr_dev_f64(corrla_ctx* ctx, int trans, const double* values, const int32_t* col_idx,
                                    const int64_t* row_ptr, int64_t m, int64_t n, int64_t nnz, const double* x,
                                    int64_t ldx, int64_t l, double beta, double* res, int64_t ldres);

/* ---- covariance and Pearson correlation matrices -----------------------------------------------
 * Replaces  mat_cov_centered(x)                                src/lib_math_utils/stats_corr.rs:32-43
 *           pearson_corr(x)                                    src/lib_math_utils/stats_corr.rs:14-28
 * and serves rsquared_sens (stats_corr.rs:75-107), whose correlation of [x | y] is this call.
 * x: n_samples (m) x n_dim (n), strided like a MatRef, never modified and never copied when its features have unit stride
 * (col_stride == 1, any row_stride >= n): one symmetric rank-k kernel on the exact f32 / f64 MFMAs computes only the tile
 * pairs on and above the diagonal, takes both operands from the same staged rows of x and centres them in registers
 *   C = (x - 1 mu^T)^T (x - 1 mu^T) / (m - ddof),            mu = column means (f64 accumulation, rounded once to T),
 * then both triangles are written from the same value: C(i, j) and C(j, i) are bitwise equal.  The effect of rounding mu
 * to T is removed exactly (a rank-1 term in f64).  No floating-point atomics: a fixed input gives a bitwise fixed result.
 * A base or row_stride that is not 16-byte aligned is read in place through bounds-checked element loads
 * (CORRLA_COV_ROUTE_INPLACE_CHECKED); a feature-strided x (column-major) is repacked once into workspace by a transposing
 * copy (CORRLA_COV_ROUTE_REPACKED).
 *   flags      : this entry's own flag word (NOT corrla_opts.flags), CORRLA_COV_* below
 *   ddof       : 0 or 1, the divisor is m - ddof (>= 1)
 *   means_out  : optional (may be NULL), n values; not written with CORRLA_COV_NO_CENTER
 *   scales_out : optional (may be NULL), n values, written only with CORRLA_COV_CORRELATION: sd_j = sqrt(ss_j / (m - ddof)),
 *                1 for a column that the rule of CORRLA_PCA_STANDARDIZE calls constant
 *   c          : n x n, leading dimension ldc >= n (symmetric: row- and column-major read the same); entries of the padding
 *                [n, ldc) are left as they were
 *   route_out  : optional (may be NULL), receives the CORRLA_COV_ROUTE_* that served the call (0 when it failed)
 * CORRLA_COV_CORRELATION: C(i, j) / (sd_i sd_j) clipped to [-1, 1], exactly 1 on the diagonal; a constant column gives a
 * zero row and column and a zero diagonal.  CORRLA_COV_NO_CENTER: the second-moment matrix x^T x / (m - ddof).
 * CORRLA_EINVAL: both flags, an unknown flag, ddof outside {0, 1}, m - ddof < 1, n < 1, NULL x or c, overlapping buffers,
 * ldc < n, negative strides.  Host-pointer entries copy x to the device as it lies (same strides, same alignment, so the
 * same route serves) and the results back; the *_dev entries take HIP device pointers, enqueue on the context's stream and
 * return WITHOUT synchronising: corrla_ctx_synchronize (or any later call on the context) orders the results.
 * (One exception: the first call that needs more workspace than the context's arena holds grows it with hipMalloc, which
 * synchronises the device implicitly; later calls of that size do not.)  The host-pointer entries copy the whole strided
 * span of x, first to last element with the gaps between rows: a narrow column view of a wide array stages the wide rows.
 * The environment variable CORRLA_SYRK_SLAB_ROWS (read when the context is created) forces the rows per slab. */
#define CORRLA_COV_CORRELATION 0x1ull /* 64-bit, as the flags parameter */
#define CORRLA_COV_NO_CENTER 0x2ull
#define CORRLA_COV_ROUTE_INPLACE 1
#define CORRLA_COV_ROUTE_INPLACE_CHECKED 2
#define CORRLA_COV_ROUTE_REPACKED 3
CORRLA_API corrla_status corrla_cov_f32(corrla_ctx* ctx, const float* x, int64_t m, int64_t n, int64_t row_stride,
                                        int64_t col_stride, uint64_t flags, int ddof, float* means_out, float* scales_out,
                                        float* c, int64_t ldc, int* route_out);
CORRLA_API corrla_status corrla_cov_f64(corrla_ctx* ctx, const double* x, int64_t m, int64_t n, int64_t row_stride,
                                        int64_t col_stride, uint64_t flags, int ddof, double* means_out, double* scales_out,
                                        double* c, int64_t ldc, int* route_out);
CORRLA_API corrla_status corrla_cov_dev_f32(corrla_ctx* ctx, const float* x, int64_t m, int64_t n, int64_t row_stride,
                                            int64_t col_stride, uint64_t flags, int ddof, float* means_out, float* scales_out,
                                            float* c, int64_t ldc, int* route_out);
CORRLA_API corrla_status corrla_cov_dev_f64(corrla_ctx* ctx, const double* x, int64_t m, int64_t n, int64_t row_stride,
                                            int64_t col_stride, uint64_t flags, int ddof, double* means_out, double* scales_out,
                                            double* c, int64_t ldc, int* route_out);

/* ---- the fitted PCA model on the device: transform, inverse transform, Q-residuals -------------------
 * Replaces  PcaRsvd::apply_tr(targ_mat)                        src/lib_math_utils/pca_rsvd.rs:43-46
 *           PcaRsvd::apply_inv_tr(red_mat)                     src/lib_math_utils/pca_rsvd.rs:49-52
 * The model: means mu (n values), components V (k x n, column-major with leading dimension ldc, as corrla_pca_* writes
 * it) and optional scales sigma (n values, CORRLA_PCA_STANDARDIZE; NULL: sigma = 1).  With z = (x - 1 mu^T) D^-1,
 * D = diag(sigma):
 *   scores         t = z V^T                       (m x k, column-major with leading dimension ld_scores >= m, like U)
 *   reconstruction xh = (t V) D + 1 mu^T           (m x n, unit stride along the features, row stride row_stride_out)
 *   Q-residual     q_i = || z_i - t_i V ||_2^2     (m values; the SPE statistic of PCA-based outlier detection)
 * corrla_pca_transform_*: the forward product runs on the tall kernels of corrla_pca_* with the centring of that entry:
 * CORRLA_PCA_CENTER_FUSED (x read in place, rank-1 corrections; the f64 default) or CORRLA_PCA_CENTER_COPY (a centred and
 * scaled m x n copy in workspace; the f32 default) -- the numeric values and defaults of corrla_opts.flags, passed in this
 * entry's own 64-bit word.  CORRLA_PCA_APPLY_OWN_MEANS: the target is centred by its OWN column means, which is what the
 * reference's apply_tr does; `means` is then ignored and the means go to means_out when it is given.  means == NULL
 * without that flag: no centring.  scales, resid_out, means_out may be NULL.
 * resid_out: q from the scores AS STORED (rounded to T), formed directly from z_i - t_i V in registers by the
 * back-projection kernel -- never as ||z_i||^2 - ||t_i||^2, which cancels where the model explains the data, and never
 * through an m x n temporary.  x is read in place with 16-byte loads, in place with checked element loads (base or row
 * stride not 16-byte aligned), or from one repacked copy (feature-strided x).  No atomics: q is bitwise reproducible.
 * corrla_pca_transform_csr_*: the same for a CSR target (operand description of corrla_pca_csr_*): always the fused
 * centring, the matrix is never densified; resid_out must be NULL (a residual over the implicit zeros is a dense
 * computation).  The CSR validation synchronises once, as in every CSR entry.
 * corrla_pca_inverse_*: out = (scores V) D + 1 mu^T in one kernel and one write of m x n; means / scales may be NULL.
 * CORRLA_EINVAL (the message names the argument): m, n < 1; k < 1 or k > n; NULL x, components, scores or out; ldc < k;
 * ld_scores < m; row_stride_out < n; both centre flags; an unknown flag; an output overlapping an input or another output.
 * Host-pointer entries copy x to the device as it lies (the whole strided span, as corrla_cov_*) and the results back;
 * the *_dev entries enqueue on the context's stream and return WITHOUT synchronising (but for a first-time growth of the
 * workspace arena): corrla_ctx_synchronize orders the results.  Row-sharded data needs no entry of its own: every rank
 * transforms its rows with the replicated model.
 * corrla_ctx_last_pca_apply: how the context's last transform / inverse call ran: centring_out 0 none, 1 fused, 2 copy;
 * route_out the CORRLA_PCA_APPLY_ROUTE_* of the back-projection kernel (0: the call ran none).  Either may be NULL. */
#define CORRLA_PCA_APPLY_OWN_MEANS 0x400ull /* 64-bit, as the flags parameter */
#define CORRLA_PCA_APPLY_ROUTE_INPLACE 1
#define CORRLA_PCA_APPLY_ROUTE_INPLACE_CHECKED 2
#define CORRLA_PCA_APPLY_ROUTE_REPACKED 3
CORRLA_API corrla_status corrla_pca_transform_f32(corrla_ctx* ctx, const float* x, int64_t m, int64_t n, int64_t row_stride,
                                                  int64_t col_stride, const float* means, const float* scales, const float* components,
                                                  int64_t ldc, int64_t k, uint64_t flags, float* scores, int64_t ld_scores, float* resid_out,
                                                  float* means_out);
CORRLA_API corrla_status corrla_pca_transform_f64(corrla_ctx* ctx, const double* x, int64_t m, int64_t n, int64_t row_stride,
                                                  int64_t col_stride, const double* means, const double* scales, const double* components,
                                                  int64_t ldc, int64_t k, uint64_t flags, double* scores, int64_t ld_scores, double* resid_out,
                                                  double* means_out);
CORRLA_API corrla_status corrla_pca_transform_dev_f32(corrla_ctx* ctx, const float* x, int64_t m, int64_t n, int64_t row_stride,
                                                      int64_t col_stride, const float* means, const float* scales, const float* components,
                                                      int64_t ldc, int64_t k, uint64_t flags, float* scores, int64_t ld_scores, float* resid_out,
                                                      float* means_out);
CORRLA_API corrla_status corrla_pca_transform_dev_f64(corrla_ctx* ctx, const double* x, int64_t m, int64_t n, int64_t row_stride,
                                                      int64_t col_stride, const double* means, const double* scales, const double* components,
                                                      int64_t ldc, int64_t k, uint64_t flags, double* scores, int64_t ld_scores, double* resid_out,
                                                      double* means_out);
CORRLA_API corrla_status corrla_pca_transform_csr_f32(corrla_ctx* ctx, const float* values, const int32_t* col_idx,
                                                      const int64_t* row_ptr, int64_t m, int64_t n, int64_t nnz, const float* means,
                                                      const float* scales, const float* components, int64_t ldc, int64_t k, uint64_t flags,
                                                      float* scores, int64_t ld_scores, float* resid_out, float* means_out);
CORRLA_API corrla_status corrla_pca_transform_csr_f64(corrla_ctx* ctx, const double* values, const int32_t* col_idx,
                                                      const int64_t* row_ptr, int64_t m, int64_t n, int64_t nnz, const double* means,
                                                      const double* scales, const double* components, int64_t ldc, int64_t k, uint64_t flags,
                                                      double* scores, int64_t ld_scores, double* resid_out, double* means_out);
CORRLA_API corrla_status corrla_pca_transform_csr_dev_f32(corrla_ctx* ctx, const float* values, const int32_t* col_idx,
                                                          const int64_t* row_ptr, int64_t m, int64_t n, int64_t nnz, const float* means,
                                                          const float* scales, const float* components, int64_t ldc, int64_t k, uint64_t flags,
                                                          float* scores, int64_t ld_scores, float* resid_out, float* means_out);
CORRLA_API corrla_status corrla_pca_transform_csr_dev_f64(corrla_ctx* ctx, const double* values, const int32_t* col_idx,
                                                          const int64_t* row_ptr, int64_t m, int64_t n, int64_t nnz, const double* means,
                                                          const double* scales, const double* components, int64_t ldc, int64_t k, uint64_t flags,
                                                          double* scores, int64_t ld_scores, double* resid_out, double* means_out);
CORRLA_API corrla_status corrla_pca_inverse_f32(corrla_ctx* ctx, const float* scores, int64_t m, int64_t k, int64_t ld_scores,
                                                const float* means, const float* scales, const float* components, int64_t ldc, int64_t n,
                                                float* out, int64_t row_stride_out);
CORRLA_API corrla_status corrla_pca_inverse_f64(corrla_ctx* ctx, const double* scores, int64_t m, int64_t k, int64_t ld_scores,
                                                const double* means, const double* scales, const double* components, int64_t ldc, int64_t n,
                                                double* out, int64_t row_stride_out);
CORRLA_API corrla_status corrla_pca_inverse_dev_f32(corrla_ctx* ctx, const float* scores, int64_t m, int64_t k, int64_t ld_scores,
                                                    const float* means, const float* scales, const float* components, int64_t ldc, int64_t n,
                                                    float* out, int64_t row_stride_out);
CORRLA_API corrla_status corrla_pca_inverse_dev_f64(corrla_ctx* ctx, const double* scores, int64_t m, int64_t k, int64_t ld_scores,
                                                    const double* means, const double* scales, const double* components, int64_t ldc, int64_t n,
                                                    double* out, int64_t row_stride_out);
CORRLA_API corrla_status corrla_ctx_last_pca_apply(corrla_ctx* ctx, int* centring_out, int* route_out);

/* ---- radial-basis-function kernel matrices: the kernel block of the fit and the prediction ------------
 * Replaces  RbfInterp::fit's kernel matrix                      src/lib_math_utils/interp_utils.rs:96-129
 *           RbfInterp::predict                                  src/lib_math_utils/interp_utils.rs:146-153
 * With Phi_ij = phi(||xq_i - xs_j||_2) over n_q queries and n_s support points of `dim` coordinates:
 *   corrla_rbf_matrix_*: out = Phi                              (n_q x n_s, row-major, row stride ld_out >= n_s)
 *   corrla_rbf_apply_* : out = Phi W_rbf + P(Xq) W_poly         (n_q x n_rhs, row-major, row stride ld_out >= n_rhs)
 * Phi is never stored by the apply entries: a workgroup forms a tile of it in registers and feeds it to the exact f32 / f64
 * matrix instructions, so 10^5 queries against 10^4 supports need no n_q x n_s temporary.
 * kernel: 1 linear r, 2 multiquadric sqrt(1 + (eps r)^2), 3 cubic r^3, 4 Gaussian exp(-(eps r)^2) (interp_utils.rs:37-80),
 * evaluated from the squared distance with the library sqrt / exp of the type.
 * Layouts: xq (n_q x dim) and xs (n_s x dim) row-major with unit stride along the coordinates and row strides ldq, lds >= dim;
 * any base alignment.  coeffs is (n_s + n_poly) x n_rhs, row-major with row stride ldw >= n_rhs: the first n_s rows are
 * W_rbf, the rest W_poly -- the layout RbfInterp::fit produces.  n_poly follows poly_degree: < 0 no tail (n_s rows),
 * 0 or 1 the dim + 1 terms [x, 1], >= 2 the dim + dim (dim + 1) / 2 + 1 terms [x, x_a x_b (a <= b, a outer), 1] of
 * build_full_vandermonde (stats_corr.rs:183-209).  The padding columns of out, [n_rhs, ld_out) or [n_s, ld_out), are left
 * as they were.
 * Limits: 1 <= dim <= 128; f32 and f64.
 * Exactness: distances are always the direct form sum_d (xq_id - xs_jd)^2 summed in index order, never the Gram form
 * ||a||^2 + ||b||^2 - 2 a.b.  So when xq and xs are the same array, corrla_rbf_matrix_* returns a matrix that equals its
 * transpose bitwise, with the exact diagonal phi(0) (0, 1, 0, 1 for kernels 1 to 4) and exact zeros where two rows coincide
 * (kernels 1 and 3).  No atomics: the supports may be split over workgroups, whose partials a finishing kernel adds in index
 * order together with the tail; a fixed input gives a bitwise fixed output.
 * CORRLA_EINVAL (the message names the argument): NULL xq, xs, coeffs or out; n_q, n_s, n_rhs < 1; dim outside [1, 128];
 * kernel outside [1, 4]; ldq, lds < dim; ldw, ld_out < n_rhs (matrix: ld_out < n_s); a non-finite eps; out overlapping an
 * input.  Host-pointer entries copy the operands to the device as they lie and the result back; the *_dev entries enqueue
 * on the context's stream and return WITHOUT synchronising (but for a first-time growth of the workspace arena):
 * corrla_ctx_synchronize orders the results. */
CORRLA_API corrla_status corrla_rbf_matrix_f32(corrla_ctx* ctx, const float* xq, int64_t n_q, int64_t ldq, const float* xs, int64_t n_s,
                                               int64_t lds, int64_t dim, int kernel, double eps, float* out, int64_t ld_out);
CORRLA_API corrla_status corrla_rbf_matrix_f64(corrla_ctx* ctx, const double* xq, int64_t n_q, int64_t ldq, const double* xs, int64_t n_s,
                                               int64_t lds, int64_t dim, int kernel, double eps, double* out, int64_t ld_out);
CORRLA_API corrla_status corrla_rbf_matrix_dev_f32(corrla_ctx* ctx, const float* xq, int64_t n_q, int64_t ldq, const float* xs, int64_t n_s,
                                                   int64_t lds, int64_t dim, int kernel, double eps, float* out, int64_t ld_out);
CORRLA_API corrla_status corrla_rbf_matrix_dev_f64(corrla_ctx* ctx, const double* xq, int64_t n_q, int64_t ldq, const double* xs, int64_t n_s,
                                                   int64_t lds, int64_t dim, int kernel, double eps, double* out, int64_t ld_out);
CORRLA_API corrla_status corrla_rbf_apply_f32(corrla_ctx* ctx, const float* xq, int64_t n_q, int64_t ldq, const float* xs, int64_t n_s,
                                              int64_t lds, int64_t dim, int kernel, double eps, int poly_degree, const float* coeffs,
                                              int64_t ldw, int64_t n_rhs, float* out, int64_t ld_out);
CORRLA_API corrla_status corrla_rbf_apply_f64(corrla_ctx* ctx, const double* xq, int64_t n_q, int64_t ldq, const double* xs, int64_t n_s,
                                              int64_t lds, int64_t dim, int kernel, double eps, int poly_degree, const double* coeffs,
                                              int64_t ldw, int64_t n_rhs, double* out, int64_t ld_out);
CORRLA_API corrla_status corrla_rbf_apply_dev_f32(corrla_ctx* ctx, const float* xq, int64_t n_q, int64_t ldq, const float* xs, int64_t n_s,
                                                  int64_t lds, int64_t dim, int kernel, double eps, int poly_degree, const float* coeffs,
                                                  int64_t ldw, int64_t n_rhs, float* out, int64_t ld_out);
CORRLA_API corrla_status corrla_rbf_apply_dev_f64(corrla_ctx* ctx, const double* xq, int64_t n_q, int64_t ldq, const double* xs, int64_t n_s,
                                                  int64_t lds, int64_t dim, int kernel, double eps, int poly_degree, const double* coeffs,
                                                  int64_t ldw, int64_t n_rhs, double* out, int64_t ld_out);

/* ---- polynomial response surfaces: the normal equations of the fit and the evaluation --------------
 * Replaces  linear_fit / jac_from_lin                            src/lib_math_utils/stats_corr.rs:146-169
 *           build_full_vandermonde / build_vandermonde           src/lib_math_utils/stats_corr.rs:183-209
 *           quad_fit / quad_eval / jac_from_quad                 src/lib_math_utils/stats_corr.rs:213-249
 * The reference stores the m x p Vandermonde matrix V = [x, x_a x_b (a <= b, a outer), 1] (degree 2, p = k + k (k + 1) / 2 + 1;
 * mat_col_interactions, stats_corr.rs:112-142) or [x, 1] (degree 1, p = k + 1) and applies pinv(V).  Here V is never stored.
 *   corrla_polyfit_gram_*: G = W^T W of order p + r with W = [V(z), y], z = (x - mu) * fl(1 / sigma) when normalize is 1 (mu the
 *     column means, sigma the population standard deviations, 1 for a constant column; the column pass of corrla_cov_*) and z = x
 *     when it is 0.  One output holds V^T V (the leading p x p block), V^T y (its last r columns) and y^T y.  Every column of
 *     W is the product of two entries of the augmented row [z, 1, y]; a workgroup stages those rows, forms its operands in
 *     registers and feeds v_mfma_f64_16x16x4_f64.  All arithmetic is f64: an f32 x or y is read in place and widened, which
 *     is exact.  G (row-major, row stride ldg >= p + r), means and scales (k each; written when normalize is 1; either may be
 *     NULL) are double for both element types.  No atomics: the samples may be split over workgroups whose partial tiles a
 *     finishing kernel adds in index order, writing G(i, j) and G(j, i) from one value -- G is bitwise symmetric and a fixed
 *     input gives a bitwise fixed output.  CORRLA_POLYFIT_SLAB_ROWS (read when the context is created) sets the samples per
 *     workgroup.
 *   corrla_poly_eval_*: out (m x r, row stride ld_out) = V(x) coeffs, and when jac is not NULL the gradients
 *     jac[(j m + i) ld_jac + a] = d out(i, j) / d x_a -- r slabs of m x k.  coeffs is double, p x r, row stride ldc, in the
 *     column order of V above.  V(x) c = xt^T C xt with xt = [x, 1] and C the symmetric (k + 1) x (k + 1) matrix of c, and
 *     the gradient is 2 (C xt)[:k]: analytic, where jac_from_quad differences forward with eps = 1e-10.
 * Layouts: x (m x k) and y (m x r) row-major with unit stride along the columns, row strides ldx >= k, ldy >= r; any base
 * alignment (an x whose base or row stride is off a 16-byte boundary is read with element loads: corrla_ctx_last_polyfit
 * reports route 2, else 1; y is read by its own alignment).
 * Limits: 1 <= k <= 128; degree 1 or 2; 0 <= r <= 64 (corrla_poly_eval_*: 1 <= r <= 64); m >= 1; f32 and f64.
 * CORRLA_EINVAL (the message names the argument): NULL x, G, coeffs, out, or y with r > 0; m < 1; k, degree, r outside the
 * limits; normalize not 0 or 1; ldx < k; ldy, ldc, ld_out < r; ldg < p + r; ld_jac < k; an output overlapping an input or
 * another output.  Host-pointer entries copy the operands to the device as they lie and the results back; the *_dev entries
 * take device pointers for every array, enqueue on the context's stream and return WITHOUT synchronising (but for a first-time
 * growth of the workspace arena, and the upload of the column table when (k, r, degree) changes): corrla_ctx_synchronize
 * orders the results. */
CORRLA_API corrla_status corrla_polyfit_gram_f32(corrla_ctx* ctx, const float* x, int64_t m, int64_t k, int64_t ldx, const float* y,
                                                 int64_t r, int64_t ldy, int degree, int normalize, double* G, int64_t ldg,
                                                 double* means, double* scales);
CORRLA_API corrla_status corrla_polyfit_gram_f64(corrla_ctx* ctx, const double* x, int64_t m, int64_t k, int64_t ldx, const double* y,
                                                 int64_t r, int64_t ldy, int degree, int normalize, double* G, int64_t ldg,
                                                 double* means, double* scales);
CORRLA_API corrla_status corrla_polyfit_gram_dev_f32(corrla_ctx* ctx, const float* x, int64_t m, int64_t k, int64_t ldx, const float* y,
                                                     int64_t r, int64_t ldy, int degree, int normalize, double* G, int64_t ldg,
                                                     double* means, double* scales);
CORRLA_API corrla_status corrla_polyfit_gram_dev_f64(corrla_ctx* ctx, const double* x, int64_t m, int64_t k, int64_t ldx, const double* y,
                                                     int64_t r, int64_t ldy, int degree, int normalize, double* G, int64_t ldg,
                                                     double* means, double* scales);
CORRLA_API corrla_status corrla_poly_eval_f32(corrla_ctx* ctx, const float* x, int64_t m, int64_t k, int64_t ldx, const double* coeffs,
                                              int64_t ldc, int64_t r, int degree, float* out, int64_t ld_out, float* jac, int64_t ld_jac);
CORRLA_API corrla_status corrla_poly_eval_f64(corrla_ctx* ctx, const double* x, int64_t m, int64_t k, int64_t ldx, const double* coeffs,
                                              int64_t ldc, int64_t r, int degree, double* out, int64_t ld_out, double* jac, int64_t ld_jac);
CORRLA_API corrla_status corrla_poly_eval_dev_f32(corrla_ctx* ctx, const float* x, int64_t m, int64_t k, int64_t ldx, const double* coeffs,
                                                  int64_t ldc, int64_t r, int degree, float* out, int64_t ld_out, float* jac, int64_t ld_jac);
CORRLA_API corrla_status corrla_poly_eval_dev_f64(corrla_ctx* ctx, const double* x, int64_t m, int64_t k, int64_t ldx, const double* coeffs,
                                                  int64_t ldc, int64_t r, int degree, double* out, int64_t ld_out, double* jac, int64_t ld_jac);
CORRLA_API corrla_status corrla_ctx_last_polyfit(corrla_ctx* ctx, int* route_out);

/* ---- Gaussian kernel density estimates: density, distribution, likelihood of a bandwidth --------------
 * Replaces  UniRv::nll                                           src/lib_math_utils/univariate_rv.rs:165-170
 *           KdeRv::pdf / KdeRv::cdf                              src/lib_math_utils/univariate_rv.rs:423-444
 * With supports s_j (j < n_s, uniform weights), points x_i, bandwidth h, d_ij = x_i - s_j and t_ij = d_ij^2 / (2 h^2):
 *   corrla_kde_eval_*: what 0  pdf_i    = (n_s h sqrt(2 pi))^-1 sum_j exp(-t_ij)
 *                      what 1  cdf_i    = n_s^-1 sum_j erfc(-d_ij / (h sqrt 2)) / 2
 *                      what 2  logpdf_i = ln pdf_i
 *   corrla_kde_nll_* : nll[b]  = -sum_i logpdf_i(h_b)            for each of the n_h bandwidths h_b
 *                      dnll[b] = d nll / d h at h_b = -sum_i (R_i - 1) / h_b,  R_i = sum_j 2 t_ij K_ij / sum_j K_ij
 * The n x n_s matrix of kernel values is never stored: a thread keeps a few points in registers and sweeps the supports;
 * d^2 is formed once per pair and serves a group of bandwidths.
 * Stabilised form: every sum is taken as exp(-t*_i) sum_j exp(-(t_ij - t*_i)) with t*_i = d*_i / (2 h^2) and
 * d*_i = min_j d_ij^2, the squared distance to the nearest support, which does not depend on h and is computed once per
 * call.  The nearest support contributes exactly 1, so logpdf, nll and dnll are finite for every finite input and every
 * h > 0 (while (x - s)^2 is finite in the element type), and pdf is correct down to the underflow of the final product.
 * This is the one deliberate difference from the reference: pdf(x).ln() is -inf there as soon as every term underflows, a
 * few tens of bandwidths outside the supports.  dnll is analytic where the reference's optimiser differences forward.
 * The cdf uses erfc, which keeps relative accuracy in the lower tail.
 * Layouts: x, s and out are vectors with element strides incx, incs, inco >= 1, read and written in place whatever the
 * alignment of their bases; the elements between the strided ones are never written.  h of corrla_kde_nll_* is ALWAYS a host
 * pointer (the bandwidths travel in the kernel arguments); nll and dnll (n_h doubles each; dnll may be NULL) are host
 * pointers for the host entries and device pointers for the *_dev entries, double for both element types: the sums over the
 * supports are taken in the element type, the reduction over the points in f64.
 * Limits: n_q, n_t, n_s >= 1; 1 <= n_h <= 64; f32 and f64.
 * No atomics: the supports may be split over workgroups, whose partial sums a finishing kernel adds in index order; the
 * likelihood is reduced over the points by a tree of fixed shape.  A fixed input gives a bitwise fixed output, and a
 * bandwidth's nll and dnll do not depend on the other bandwidths of the call.  corrla_ctx_last_kde reports 1 when the last
 * call swept the supports in one range and 2 when it split them.
 * CORRLA_EINVAL (the message names the argument): NULL x, s, out, h or nll; n_q, n_t, n_s < 1; incx, incs, inco < 1; h not
 * finite or <= 0; what outside [0, 2]; n_h outside [1, 64]; an output overlapping an input or the other output.  Host-pointer
 * entries copy the strided spans to the device as they lie and the results back; the *_dev entries enqueue on the context's
 * stream and return WITHOUT synchronising (but for a first-time growth of the workspace arena): corrla_ctx_synchronize
 * orders the results. */
CORRLA_API corrla_status corrla_kde_eval_f32(corrla_ctx* ctx, const float* x, int64_t n_q, int64_t incx, const float* s, int64_t n_s,
                                             int64_t incs, double h, int what, float* out, int64_t inco);
CORRLA_API corrla_status corrla_kde_eval_f64(corrla_ctx* ctx, const double* x, int64_t n_q, int64_t incx, const double* s, int64_t n_s,
                                             int64_t incs, double h, int what, double* out, int64_t inco);
CORRLA_API corrla_status corrla_kde_eval_dev_f32(corrla_ctx* ctx, const float* x, int64_t n_q, int64_t incx, const float* s, int64_t n_s,
                                                 int64_t incs, double h, int what, float* out, int64_t inco);
CORRLA_API corrla_status corrla_kde_eval_dev_f64(corrla_ctx* ctx, const double* x, int64_t n_q, int64_t incx, const double* s, int64_t n_s,
                                                 int64_t incs, double h, int what, double* out, int64_t inco);
CORRLA_API corrla_status corrla_kde_nll_f32(corrla_ctx* ctx, const float* x, int64_t n_t, int64_t incx, const float* s, int64_t n_s,
                                            int64_t incs, const double* h, int64_t n_h, double* nll, double* dnll);
CORRLA_API corrla_status corrla_kde_nll_f64(corrla_ctx* ctx, const double* x, int64_t n_t, int64_t incx, const double* s, int64_t n_s,
                                            int64_t incs, const double* h, int64_t n_h, double* nll, double* dnll);
CORRLA_API corrla_status corrla_kde_nll_dev_f32(corrla_ctx* ctx, const float* x, int64_t n_t, int64_t incx, const float* s, int64_t n_s,
                                                int64_t incs, const double* h, int64_t n_h, double* nll, double* dnll);
CORRLA_API corrla_status corrla_kde_nll_dev_f64(corrla_ctx* ctx, const double* x, int64_t n_t, int64_t incx, const double* s, int64_t n_s,
                                                int64_t incs, const double* h, int64_t n_h, double* nll, double* dnll);
CORRLA_API corrla_status corrla_ctx_last_kde(corrla_ctx* ctx, int* route_out);

/* ---- dense linear solve: LU with partial pivoting; the RBF fit on it -----------------------------------
 * Replaces  the solve of RbfInterp::fit (opt-in: the reference takes mat_pinv)   src/lib_math_utils/interp_utils.rs:96-143
 * P A = L U with LAPACK getrf semantics: unit lower L and upper U stored over A, ipiv[j] (0-based, >= j) the row exchanged with
 * row j at step j.  f64 only.
 * STORAGE ORDER: every matrix here is ROW-major -- a is n x n with row stride lda >= n, b and x are n x n_rhs with row strides
 * ldb, ldx >= n_rhs, ipiv is n int64.  (The RBF system is symmetric: row-major and column-major hold the same matrix.)
 * Pivot rule: the entry of largest magnitude on or below the diagonal, ties to the lowest row index; the comparisons are
 * exact and the multipliers are quotients, so |l_ij| <= 1 holds exactly.  No atomics: a fixed input gives bitwise fixed
 * output.  Routes (corrla_ctx_last_solve): 1 small, n <= 128, one workgroup factors the matrix in LDS; 2 blocked, right-looking
 * with panels of 64 columns, the trailing update on v_mfma_f64_16x16x4_f64.  Then the interchanges are applied to B and L and U
 * are substituted block row by block row, for any n_rhs.
 *   corrla_lu_solve_f64    : host pointers; a and b are left untouched, x = A^-1 b is written (its padding columns are not).
 *   corrla_lu_solve_dev_f64: device pointers, in place: a becomes LU, b becomes X, ipiv (NULL: not wanted) the interchanges.
 *   corrla_rbffit_system_*    : m = [[K, P], [P^T, 0]], N x N with N = n_s + n_poly, row stride ldm >= N: K = Phi(xs, xs) exactly
 *                            as corrla_rbf_matrix_* forms it, P the polynomial tail of corrla_rbf_apply_* (poly_degree < 0: none,
 *                            0 or 1: [x, 1], >= 2: [x, x_a x_b (a <= b), 1]; one rounding per product), the corner exactly zero.
 *   corrla_rbffit_*       : coeffs (N x n_rhs, row stride ldw >= n_rhs) = M^-1 [y; 0] with M as above, built in workspace:
 *                            the layout corrla_rbf_apply_* reads.  y is n_s x n_rhs with row stride ldy.  Bitwise what
 *                            corrla_rbffit_system_* followed by corrla_lu_solve_* gives.
 * An exactly zero or non-finite pivot ends the call with CORRLA_ENUMERIC; the message carries the 1-based column, and the
 * outputs then hold a partial factorisation (device entries) or are not written (host entries).  The one read-back of a solve
 * or fit carries info (0 or that column), the smallest |pivot| and the largest |u_ij|: corrla_ctx_last_solve returns them
 * (any pointer may be NULL).  So the *_dev solve and fit entries synchronise once; corrla_rbffit_system_dev_f64 only enqueues.
 * Limits: 1 <= n (N) <= 131072; 1 <= n_rhs <= 1048576; dim, kernel and eps as for corrla_rbf_matrix_*.
 * CORRLA_EINVAL (the message names the argument): a NULL array, n or n_rhs outside the limits, lda < n, ldb / ldx / ldy / ldw
 * < n_rhs, ldxs < dim, ldm < N, an output overlapping an input or another output. */
CORRLA_API corrla_status corrla_lu_solve_f64(corrla_ctx* ctx, const double* a, int64_t n, int64_t lda, const double* b, int64_t n_rhs,
                                             int64_t ldb, double* x, int64_t ldx);
CORRLA_API corrla_status corrla_lu_solve_dev_f64(corrla_ctx* ctx, double* a, int64_t n, int64_t lda, double* b, int64_t n_rhs, int64_t ldb,
                                                 int64_t* ipiv);
CORRLA_API corrla_status corrla_rbffit_system_f64(corrla_ctx* ctx, const double* xs, int64_t n_s, int64_t ldxs, int64_t dim, int kernel,
                                               double eps, int poly_degree, double* m, int64_t ldm);
CORRLA_API corrla_status corrla_rbffit_system_dev_f64(corrla_ctx* ctx, const double* xs, int64_t n_s, int64_t ldxs, int64_t dim, int kernel,
                                                   double eps, int poly_degree, double* m, int64_t ldm);
CORRLA_API corrla_status corrla_rbffit_f64(corrla_ctx* ctx, const double* xs, int64_t n_s, int64_t ldxs, int64_t dim, const double* y,
                                            int64_t n_rhs, int64_t ldy, int kernel, double eps, int poly_degree, double* coeffs, int64_t ldw);
CORRLA_API corrla_status corrla_rbffit_dev_f64(corrla_ctx* ctx, const double* xs, int64_t n_s, int64_t ldxs, int64_t dim, const double* y,
                                                int64_t n_rhs, int64_t ldy, int kernel, double eps, int poly_degree, double* coeffs,
                                                int64_t ldw);
CORRLA_API corrla_status corrla_ctx_last_solve(corrla_ctx* ctx, int* route, int64_t* info, double* min_pivot, double* max_u);

/* ---- dense Cholesky factor and symmetric positive definite solve ------------------------------------------
 * Replaces  the host Cholesky of the covariance factor (numpy) and, opt-in, the solve of a positive definite RBF system
 * A = L L^T, L lower triangular with a positive diagonal.  f64 only.
 * STORAGE ORDER: every matrix here is ROW-major -- a and l are n x n with row strides lda, ldl >= n, b and x are n x n_rhs with
 * row strides ldb, ldx >= n_rhs.  Only the LOWER triangle of a (i >= j) is read; the in-place entries write only it: the strict
 * upper triangle is neither read nor written and may hold anything.
 * No pivoting and no atomics: a fixed input gives bitwise fixed output.  Square roots and quotients are correctly rounded.
 * Routes (corrla_ctx_last_chol): 1 small, n <= 128, one workgroup factors the triangle in LDS; 2 blocked, right-looking with
 * panels of 64 columns -- the diagonal block in LDS, L21 = A21 L11^-T, and the trailing update of the lower-triangle tiles on
 * v_mfma_f64_16x16x4_f64: 3 launches per panel, 3 ceil(n / 64) - 1 in all.  A solve then substitutes L and L^T block row by
 * block row, for any n_rhs.
 *   corrla_chol_factor_f64    : host pointers; a is left untouched; the full n x n of l is written -- L on and below the
 *                               diagonal, exact zeros above; its padding columns are not.
 *   corrla_chol_factor_dev_f64: device pointer, in place: the lower triangle of a becomes L.
 *   corrla_chol_solve_f64     : host pointers; a and b are left untouched, x = A^-1 b is written (its padding columns are not).
 *   corrla_chol_solve_dev_f64 : device pointers, in place: a becomes L (lower triangle), b becomes X.
 * A pivot a_jj - sum_k l_jk^2 that is <= 0 or not finite ends the call with CORRLA_ENUMERIC; the message carries the 1-based
 * column of the first such pivot.  The device entries then leave a partial factor whose columns before that one are final; the
 * host entries write nothing.  The one read-back of a call carries info (0 or that column), the smallest and the largest l_jj
 * of the columns factored, and logdet = log det A = 2 sum_j log l_jj, summed on the device in a fixed order (0 when info != 0):
 * corrla_ctx_last_chol returns them (any pointer may be NULL).  So the *_dev entries synchronise once.
 * Limits: 1 <= n <= 131072; 1 <= n_rhs <= 1048576.
 * CORRLA_EINVAL (the message names the argument): a NULL array, n or n_rhs outside the limits, lda / ldl < n, ldb / ldx < n_rhs,
 * an output overlapping an input or another output. */
CORRLA_API corrla_status corrla_chol_factor_f64(corrla_ctx* ctx, const double* a, int64_t n, int64_t lda, double* l, int64_t ldl);
CORRLA_API corrla_status corrla_chol_factor_dev_f64(corrla_ctx* ctx, double* a, int64_t n, int64_t lda);
CORRLA_API corrla_status corrla_chol_solve_f64(corrla_ctx* ctx, const double* a, int64_t n, int64_t lda, const double* b, int64_t n_rhs,
                                               int64_t ldb, double* x, int64_t ldx);
CORRLA_API corrla_status corrla_chol_solve_dev_f64(corrla_ctx* ctx, double* a, int64_t n, int64_t lda, double* b, int64_t n_rhs, int64_t ldb);
CORRLA_API corrla_status corrla_ctx_last_chol(corrla_ctx* ctx, int* route, int64_t* info, double* min_diag, double* max_diag, double* logdet);

/* ---- symmetric eigendecomposition A = V diag(w) V^T on the device, f64 -------------------------------------
 * Replaces  numpy.linalg.eigh in the provided callers (polyfit_solve, mvn_factor) and the symmetric pseudo-inverse of mat_pinv.
 * a is n x n row-major with row stride lda >= n; only its LOWER triangle (i >= j) is read, the strict upper triangle may hold
 * anything, and a is never written.  w (n) receives the eigenvalues in ascending order, as numpy.linalg.eigh returns them
 * (eigenvalues that are equal as doubles are ranked by the index of their column of the rotated factor); v (n x n, row stride ldv >= n, row-major) receives the eigenvectors in its columns,
 * each with its component of largest magnitude positive (the lowest index wins a tie).  The padding columns of v are not written.
 * Algorithm: sigma = 1.5 min(|A|_F, |A|_inf) makes B = A + sigma I positive definite with a condition number of at most 5;
 * B = L L^T by the blocked Cholesky of corrla_chol_factor_*; one-sided block Jacobi with right rotations on W = L -- column
 * blocks of 32, a round-robin tournament of disjoint block pairs, per pair the 64 x 64 Gram matrix on v_mfma_f64_16x16x4_f64,
 * one sweep of a cyclic threshold Jacobi in LDS and the rotation of both panels on the same MFMA -- until every pair's measure
 * max |g_ij| / sqrt(g_ii g_jj) is <= 2 sqrt(n) 2^-53.  The columns of W are then orthogonal: v_i is column i divided by its
 * norm, and the eigenvalue is its Rayleigh quotient v_i^T A v_i / v_i^T v_i over the caller's matrix -- not |column|^2 - sigma,
 * which carries the rounding of every rotation the column went through.  The norms and quotients are summed in two doubles.
 * Accuracy: normwise backward stable; absolute errors of order n u (sigma + |A|_2) in w, like LAPACK's for an indefinite
 * matrix.  It is NOT relatively accurate for eigenvalues much smaller than |A|.
 * No atomics: a fixed input gives bitwise fixed output, and the host entry gives the bits of the device entry.
 * Routes (corrla_ctx_last_eigh): 1 small, n <= 64, one workgroup and one launch: the same algorithm with one pair that holds
 * every column -- B, its Cholesky factor W, and per sweep W^T W, the LDS Jacobi and W <- W R, all in LDS; 2 blocked.
 *   corrla_eigh_f64    : host pointers; nothing is written when the call fails.
 *   corrla_eigh_dev_f64: device pointers; the working copy lives in workspace (about 16 n^2 bytes).  The entry synchronises.
 * CORRLA_ENUMERIC: a non-finite entry in the lower triangle (info 1), a pivot reported by the Cholesky factorisation (info 2,
 * cannot happen on a finite matrix), more than 40 sweeps (info 3).  The zero matrix returns w = 0, V = I without a sweep.
 * corrla_ctx_last_eigh returns the route, the sweeps that rotated, the largest measure of the last sweep, sigma and info of the
 * context's last call (any pointer may be NULL).
 * Limits: 1 <= n <= 32768.  CORRLA_ENOMEM: the workspace could not be allocated; nothing was launched.
 * CORRLA_EINVAL (the message names the argument): a NULL array, n outside the limits, lda / ldv < n, an output overlapping the
 * input or the other output. */
CORRLA_API corrla_status corrla_eigh_f64(corrla_ctx* ctx, const double* a, int64_t n, int64_t lda, double* w, double* v, int64_t ldv);
CORRLA_API corrla_status corrla_eigh_dev_f64(corrla_ctx* ctx, const double* a, int64_t n, int64_t lda, double* w, double* v, int64_t ldv);
CORRLA_API corrla_status corrla_ctx_last_eigh(corrla_ctx* ctx, int* route, int* sweeps, double* off, double* shift, int64_t* info);

/* ---- constrained Dirichlet sampling: draws on the simplex, rejection against a box ---------------------
 * Replaces  dirichlet_shot_sample / constr_dirichlet_sample       src/lib_math_utils/space_samplers.rs:14-126
 * THE STREAM.  Draw t (0 <= t < 2^62) of (seed, alphas[0..d), c_scale) is the row x[0..d), all in IEEE double:
 *   U(t, j, a, p) = (u1, u2): the two uniforms of ONE Philox4x32-10 block with key (seed mod 2^32, seed >> 32) and counter
 *     (t mod 2^32, t >> 32, j + 65536 p, a) -- component j, attempt a, purpose p (0 the normal of an attempt, 1 the
 *     uniform of its acceptance test, 2 the component's own uniform, with a = 0); from the output words w0..w3,
 *     u1 = (((w0 << 32 | w1) >> 11) + 0.5) 2^-53 and u2 likewise from w2, w3, as corrla_fill_normal_dev_f64 maps them.
 *   g_j ~ Gamma(alphas[j], 1), the method chosen by alphas[j] alone:
 *     = 1:  g = -log(u1) with (u1, .) = U(t, j, 0, 2).
 *     > 1:  Marsaglia-Tsang at shape s = alphas[j]: D = s - 1/3, C = 1 / sqrt(9 D).  Attempt a = 0, 1, ...:
 *           (u1, u2) = U(t, j, a, 0), z = sqrt(-2 log(u1)) * cospi(2 u2), w = 1 + C z, rejected if w <= 0;
 *           v = (w w) w, (q, .) = U(t, j, a, 1), z2 = z z; accepted if q < 1 - 0.0331 (z2 z2), else if
 *           log(q) < 0.5 z2 + D ((1 - v) + log(v)).  g = D v of the first accepted attempt (g = D after 64 rejected
 *           attempts, which has probability below 1e-83).
 *     < 1:  the same at shape s = alphas[j] + 1, then g = (D v) * pow(u1, 1 / alphas[j]) with (u1, .) = U(t, j, 0, 2).
 *   S = ((g_0 + g_1) + g_2) + ... in index order, x_j = (c_scale g_j) / S.  Every operation is rounded once, in the order
 *   written; no FMA is formed.  A draw depends on nothing but (seed, alphas, c_scale, t).
 * corrla_dirichlet_draws_*: rows i < n of out are the draws first + i.
 * corrla_dirichlet_sample_*: the draws of shot s are [s chunk_size, (s + 1) chunk_size); a draw is accepted when
 *   bounds[2 j] <= x_j <= bounds[2 j + 1] for every j, compared on the very doubles that are stored, so a returned row
 *   lies inside its box exactly.  out receives the first n_samples accepted draws among the draws
 *   [0, max_zshots chunk_size) in increasing draw index, whatever chunk_size is; *n_found = how many there were
 *   (<= n_samples); rows [n_found, n_samples) are written as zeros, which is what the reference leaves there;
 *   *n_drawn = chunk_size times the shots that were needed (max_zshots when n_found < n_samples).
 *   Nothing data-sized is stored: a workgroup generates 1024 draws, tests them and writes one bit per draw and a count;
 *   a one-block scan ranks the counts; the accepted draws below rank n_samples are generated again into their rows.  No
 *   atomics: the result is bitwise reproducible for a seed.  The call reads a 24-byte state back once per batch of
 *   launches; batches at least double from 1024 workgroups, so at most 1 + ceil(log2(workgroups / 1024)) read-backs.
 * Layouts: alphas (d doubles) and bounds (d x 2 row-major) are ALWAYS host pointers, as are n_found and n_drawn.  out is
 * n x d (n_samples x d) with row stride ldo >= d, a host pointer for the plain entries and a device pointer for *_dev;
 * the elements between d and ldo are never written.  Both kinds of corrla_dirichlet_sample_* synchronise;
 * corrla_dirichlet_draws_dev_f64 enqueues after one synchronising copy of the component table.
 * Limits: 2 <= d <= 128; alphas[j] and c_scale finite and > 0; first >= 0, n >= 1, first + n <= 2^62; n_samples,
 * max_zshots, chunk_size >= 1; max_zshots chunk_size < 2^62.
 * CORRLA_EINVAL (the message names the argument): any of these limits; NULL alphas, bounds, out, n_found or n_drawn;
 * ldo < d; bounds[2 j] > bounds[2 j + 1]; a bound that is not finite; an infeasible box (sum of the lower bounds above
 * c_scale or of the upper bounds below it, with 8 d ulp of slack); out overlapping a host input.
 * corrla_ctx_last_dirichlet: the low byte of *route_out is the route of the last accepted call -- 1 registers /
 * exponential-only (d <= 16, every alpha 1), 2 registers / general, 3 regenerate / exponential-only (d > 16: one sweep
 * forms S, a second draws each g_j again from its counter), 4 regenerate / general -- and the bits above it the
 * read-backs it made. */
CORRLA_API corrla_status corrla_dirichlet_draws_f64(corrla_ctx* ctx, const double* alphas, int64_t d, double c_scale, uint64_t seed,
                                                    int64_t first, int64_t n, double* out, int64_t ldo);
CORRLA_API corrla_status corrla_dirichlet_draws_dev_f64(corrla_ctx* ctx, const double* alphas, int64_t d, double c_scale, uint64_t seed,
                                                        int64_t first, int64_t n, double* out, int64_t ldo);
CORRLA_API corrla_status corrla_dirichlet_sample_f64(corrla_ctx* ctx, const double* bounds, const double* alphas, int64_t d, double c_scale,
                                                     uint64_t seed, int64_t n_samples, int64_t max_zshots, int64_t chunk_size, double* out,
                                                     int64_t ldo, int64_t* n_found, int64_t* n_drawn);
CORRLA_API corrla_status corrla_dirichlet_sample_dev_f64(corrla_ctx* ctx, const double* bounds, const double* alphas, int64_t d, double c_scale,
                                                         uint64_t seed, int64_t n_samples, int64_t max_zshots, int64_t chunk_size, double* out,
                                                         int64_t ldo, int64_t* n_found, int64_t* n_drawn);
CORRLA_API corrla_status corrla_ctx_last_dirichlet(corrla_ctx* ctx, int* route_out);

/* ---- multivariate normal rows and sandwich variances ----------------------------------------------------
 * Replaces  sample_mv_normal / sandwich_prop (its diagonal)        src/lib_math_utils/stats_corr.rs:46-58, 64-68
 * corrla_mvn_sample_*: row i < n of out is x_i = mean + factor z_i, factor d x r (1 <= r <= d), so the rows have
 *   covariance factor factor^T.  (The reference multiplies z by the covariance itself, which gives covariance C^2; pass
 *   factor = C for that law.)
 * THE STREAM.  z_i[j] (0 <= j < r) of (seed, first, r) is the N(0,1) value of counter t = (first + i) r + j:
 *   ONE Philox4x32-10 block with key (seed mod 2^32, seed >> 32) and counter (t mod 2^32, t >> 32, 0, 0), output words
 *   w0..w3;  f64: u1 = (((w0 << 32 | w1) >> 11) + 0.5) 2^-53, u2 likewise from w2, w3;  f32: u1 = ((w0 >> 8) + 0.5) 2^-24,
 *   u2 likewise from w1;  z = sqrt(-2 log(u1)) * cospi(2 u2) in the element type.  These are the values
 *   corrla_fill_normal_dev_* writes into an n x r matrix with row0 = first and global_cols = r.  The result is a pure
 *   function of (seed, first, factor, mean): rows [a, b) of a call are, bit for bit, the call with first + a and n = b - a,
 *   and a call repeated gives the same bits.  No atomics, and nothing is read back inside the call.
 * Routes (corrla_ctx_last_mvn: 1 fused, 2 staged, 3 n = 0, nothing launched):
 *   fused, r <= 288 (f32) / 144 (f64): a workgroup generates the z of 64 rows once into LDS -- no z is generated twice,
 *     none reaches global memory --, walks the columns of out on the exact f32 / f64 MFMAs with factor^T read in chunks,
 *     and writes acc + mean once.  The limit is what lets two such workgroups share the 160 KiB of LDS of a compute unit.
 *   staged, any larger r with d <= 65536: z of a row chunk is filled into a workspace of at most max(256 MiB, 64 r
 *     elements) and multiplied by the back-projection kernel of corrla_pca_inverse_*.  The same stream; against the fused
 *     route equal to rounding (both sum r products in their own order), not bitwise.
 *   lower != 0: factor is square lower-triangular (a Cholesky factor); its strict upper triangle is taken as zero and never
 *     read, and the fused route skips the MFMA steps that lie wholly above the diagonal.  The result is bitwise that of
 *     lower = 0 on the same triangular matrix: the skipped terms are exact zeros.
 * corrla_sandwich_diag_*: v[i] = sum_a sum_b jac[i][a] cov[a][b] jac[i][b], i < m; cov is used as given, never symmetrised.
 *   The row tile of jac is staged in LDS once, jac cov runs on the MFMAs a column tile at a time and is multiplied by the
 *   staged tile and summed along the row in a fixed order: no m x d temporary, no atomics, bitwise reproducible.
 * Layouts: factor d x r with row stride ldf >= r; mean d contiguous values or NULL (zeros); out n x d with unit stride
 *   along d and row stride ldo >= d, the elements between d and ldo are never written (16-byte stores where the base and
 *   ldo allow, element stores otherwise); jac m x d with row stride ldj >= d, cov d x d with row stride ldc >= d, v m
 *   contiguous values.  Host pointers for the plain entries, device pointers for *_dev, which enqueue and return.
 * Limits: n >= 0 (n = 0 returns without a launch), first >= 0, (first + n) r < 2^63; sandwich: m >= 1, 1 <= d <= 512.
 * CORRLA_EINVAL (the message names the argument): any of these limits; r < 1, r > d; lower with r != d; a negative stride
 *   or one below the row length; NULL factor, out, jac, cov or v; an output overlapping an input. */
CORRLA_API corrla_status corrla_mvn_sample_f32(corrla_ctx* ctx, int64_t n, int64_t d, int64_t r, const float* factor, int64_t ldf,
                                               const float* mean, uint64_t seed, int64_t first, int lower, float* out, int64_t ldo);
CORRLA_API corrla_status corrla_mvn_sample_f64(corrla_ctx* ctx, int64_t n, int64_t d, int64_t r, const double* factor, int64_t ldf,
                                               const double* mean, uint64_t seed, int64_t first, int lower, double* out, int64_t ldo);
CORRLA_API corrla_status corrla_mvn_sample_dev_f32(corrla_ctx* ctx, int64_t n, int64_t d, int64_t r, const float* factor, int64_t ldf,
                                                   const float* mean, uint64_t seed, int64_t first, int lower, float* out, int64_t ldo);
CORRLA_API corrla_status corrla_mvn_sample_dev_f64(corrla_ctx* ctx, int64_t n, int64_t d, int64_t r, const double* factor, int64_t ldf,
                                                   const double* mean, uint64_t seed, int64_t first, int lower, double* out, int64_t ldo);
CORRLA_API corrla_status corrla_sandwich_diag_f32(corrla_ctx* ctx, const float* jac, int64_t m, int64_t d, int64_t ldj, const float* cov,
                                                  int64_t ldc, float* v);
CORRLA_API corrla_status corrla_sandwich_diag_f64(corrla_ctx* ctx, const double* jac, int64_t m, int64_t d, int64_t ldj, const double* cov,
                                                  int64_t ldc, double* v);
CORRLA_API corrla_status corrla_sandwich_diag_dev_f32(corrla_ctx* ctx, const float* jac, int64_t m, int64_t d, int64_t ldj, const float* cov,
                                                      int64_t ldc, float* v);
CORRLA_API corrla_status corrla_sandwich_diag_dev_f64(corrla_ctx* ctx, const double* jac, int64_t m, int64_t d, int64_t ldj, const double* cov,
                                                      int64_t ldc, double* v);
CORRLA_API corrla_status corrla_ctx_last_mvn(corrla_ctx* ctx, int* route_out);

/* ---- the Gaussian generator: random_mat_normal --------------------------------------
 * Replaces  random_mat_normal<T>(n_rows, n_cols)               src/lib_math_utils/mat_utils.rs:161-175
 * Fills a DEVICE matrix with i.i.d. N(0,1) from a counter-based Philox4x32-10 + Box-Muller
 * stream: element (i, j) of the logical matrix depends only on (seed, (row0 + i) * global_cols + j),
 * so any row shard generates its own rows bit-identically.  Storage strides in elements. */
CORRLA_API corrla_status corrla_fill_normal_dev_f32(corrla_ctx* ctx, float* p, int64_t rows, int64_t cols, int64_t row_stride,
                                         int64_t col_stride, uint64_t seed, int64_t row0, int64_t global_cols);
CORRLA_API corrla_status corrla_fill_normal_dev_f64(corrla_ctx* ctx, double* p, int64_t rows, int64_t cols, int64_t row_stride,
                                         int64_t col_stride, uint64_t seed, int64_t row0, int64_t global_cols);

/* ---- active-subspace gradient stage --------------------------------
 * Replaces  PolyGradientEstimator::new / grad_at            src/lib_math_utils/active_subspaces.rs:66-141
 *           ActiveSsRsvd::create_grad_mat                    src/lib_math_utils/active_subspaces.rs:215-229
 *           (linear_fit / quad_fit / jac_from_lin / jac_from_quad, src/lib_math_utils/stats_corr.rs:146-249)
 * x  : n_pts x k support points, row-major contiguous (ld = k); y: n_pts values of the scalar function;
 * xq : n_q x k query points (the reference uses the support points themselves);
 * est_order 1: least-squares hyper-plane through the n_nbrs nearest support points of each query (needs n_pts,
 *              n_nbrs > k + 1); 2: full quadratic [x, x_a x_b (a <= b), 1], build_vandermonde (stats_corr.rs:198-207;
 *              needs n_pts, n_nbrs > k (k + 3) / 2).  Any k and any n_nbrs <= n_pts: calls with k <= 64,
 *              n_nbrs <= 512 whose neighbours fit in 160 KiB of LDS take the limited kernels, all others the wide
 *              kernels (features streamed, lists and normal equations in global memory).  Still rejected: n_pts >
 *              2^31 - 1, n_q * n_nbrs > 2^40, and normal equations of one query ((P + 1)^2 doubles, P = k + 1 or
 *              k + k (k + 1) / 2 + 1 design columns) above a 4 GiB workspace budget (order 1 to k ~ 23000, order 2 to
 *              k = 213).  Order 2 at large k is expensive by nature: ~P^2 n_nbrs + P^3 / 3 flops per query.
 * g  : out_scale * gradients in the reference's k x n_q column-major layout: n_q rows of k contiguous values, row
 *      stride ldg >= k.  fit_svd (active_subspaces.rs:233-250) passes out_scale = 1 / sqrt(n_q) and hands g to
 *      corrla_rsvd_dev_f64 as the k x n_q matrix (row_stride 1, col_stride ldg).
 * n_regularised (optional): queries whose design is numerically rank deficient -- a Cholesky pivot of the normal equations
 *      below 1e-13 once every column is scaled to unit size, so a feature's units do not enter: a constant feature or too
 *      few distinct neighbours are counted, a full-rank design whose features are small, large or differ in scale is not
 *      (the reference's pinv returns the minimum-norm fit there; this build retries with a ridge of 1e-10 on the scaled
 *      diagonal, and writes a zero gradient if that fails too).
 *      Nearest neighbours are exact (brute force); equal distances are ordered by index.
 *      Scale: any coordinates whose squares and pairwise squared distances are finite, normal f64 numbers; features may
 *      differ in scale (micrometres beside pascals), points may differ in size (outliers), and nothing needs to be
 *      normalised.  The neighbours are those of the coordinates as passed. */
CORRLA_API corrla_status corrla_grad_mat_f64(corrla_ctx* ctx, const double* x, int64_t n_pts, int64_t k, const double* y,
                                             const double* xq, int64_t n_q, int est_order, int64_t n_nbrs, double out_scale,
                                             double* g, int64_t ldg, int* n_regularised);
CORRLA_API corrla_status corrla_grad_mat_dev_f64(corrla_ctx* ctx, const double* x, int64_t n_pts, int64_t k, const double* y,
                                                 const double* xq, int64_t n_q, int est_order, int64_t n_nbrs,
                                                 double out_scale, double* g, int64_t ldg, int* n_regularised);

/* ---- measurement hook ---------------------------------------------------------------
 * Times `reps` back-to-back launches of the sketch GEMM Y = A * X (random_svd.rs:31) with
 * hipEvents recorded on the context's stream (the stream the kernel runs on) and returns the
 * average kernel-sequence duration in milliseconds.  DEVICE pointers, layouts as in
 * corrla_matmul_dev_*.  Used by bench.py for roofline.achieved. */
CORRLA_API corrla_status corrla_time_sketch_dev_f32(corrla_ctx* ctx, const float* a, int64_t m, int64_t n, int64_t row_stride,
                                         int64_t col_stride, const float* x, int64_t ldx, int64_t l, float* y,
                                         int64_t ldy, int reps, double* avg_ms);
CORRLA_API corrla_status corrla_time_sketch_dev_f64(corrla_ctx* ctx, const double* a, int64_t m, int64_t n, int64_t row_stride,
                                         int64_t col_stride, const double* x, int64_t ldx, int64_t l, double* y,
                                         int64_t ldy, int reps, double* avg_ms);

/* ---- multi-GPU: row-sharded tall matrices ---------------------
 * One process per GPU.  Rank 0 calls corrla_comm_unique_id, the 128 bytes are broadcast by the
 * host program (torch.distributed / MPI / a file), then every rank calls corrla_ctx_comm_init.
 * The communicator is RCCL; collectives are enqueued on the context's stream. */
#define CORRLA_UNIQUE_ID_BYTES 128
CORRLA_API corrla_status corrla_comm_unique_id(void* out128);
CORRLA_API corrla_status corrla_ctx_comm_init(corrla_ctx* ctx, const void* unique_id128, int rank, int nranks);

/* Row-sharded random_svd: this rank holds rows [row0, row0 + m_local) of the TALL matrix
 * A (m_global x n, m_global >= n), unit column stride or unit row stride as above.
 * U_local: m_local x k (this rank's rows of U); S and Vt are replicated on every rank.
 * Exchanges per call: q+1 all-reduces of n x l (Z and B^T), the l x l Gram all-reduces of the
 * orthonormalisations, one scalar per power iteration.  DEVICE pointers. */
CORRLA_API corrla_status corrla_rsvd_sharded_dev_f32(corrla_ctx* ctx, const float* a_local, int64_t m_local, int64_t n,
                                          int64_t row_stride, int64_t col_stride, int64_t rank, int64_t n_iter,
                                          int64_t n_oversamples, const corrla_opts* opts, float* u_local, int64_t ldu,
                                          float* s, float* vt, int64_t ldvt);
CORRLA_API corrla_status corrla_rsvd_sharded_dev_f64(corrla_ctx* ctx, const double* a_local, int64_t m_local, int64_t n,
                                          int64_t row_stride, int64_t col_stride, int64_t rank, int64_t n_iter,
                                          int64_t n_oversamples, const corrla_opts* opts, double* u_local, int64_t ldu,
                                          double* s, double* vt, int64_t ldvt);

#ifdef __cplusplus
}
#endif
#endif /* CORRLA_RSVD_H */
