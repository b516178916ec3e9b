// C-ABI glue shared by the product library (HIP backend) and the test-only emulation library:
// argument validation, fat/tall + stride classification, staging of A, output orientation
// (random_svd.rs:69-74, 96-109).  Templated on the backend; contains no m-/n-sized arithmetic.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/corrla_rsvd.h"
#include "call_spans.hpp"
#include "driver.hpp"
#include "rbf_plan.hpp"  // rbf_poly_terms, kRbfMaxDim
#include "polyfit_plan.hpp"  // poly_terms, kPolyMaxK, kPolyMaxRhs
#include "kde_plan.hpp"  // kKdeMaxH
#include "dirichlet_plan.hpp"  // dir_plan: the limits of the Dirichlet entries
#include "mvn_plan.hpp"  // mvn_plan, sandwich_plan: the limits of the multivariate normal entries
#include "chol_plan.hpp"  // chol_plan: the limits of the Cholesky entries
#include "eigh_plan.hpp"  // eigh_plan: the limits of the eigensolver entries
#include "lu_plan.hpp"  // lu_plan: the limits of the dense-solve entries

namespace corrla {

inline std::string& last_error_slot() {
  static thread_local std::string msg;
  return msg;
}

template <class F>
inline corrla_status guarded(F&& f) {
  try {
    f();
    return CORRLA_OK;
  } catch (const Error& e) {
    last_error_slot() = e.what();
    return (corrla_status)e.code;
  } catch (const std::bad_alloc&) {
    last_error_slot() = "host allocation failed";
    return CORRLA_ENOMEM;
  } catch (const std::exception& e) {
    last_error_slot() = e.what();
    return CORRLA_EINVAL;
  }
}

// The first 32 bytes of corrla_opts (through omega_ld) are the layout of the first release: a caller built against that
// header passes struct_size == 32 and the later fields read as zero.
constexpr uint32_t kOptsSizeV1 = 32;
static_assert(offsetof(corrla_opts, scales_out) == kOptsSizeV1, "corrla_opts grows at the end only");

// pca: the call is a corrla_pca_* entry (the only ones CORRLA_PCA_STANDARDIZE is valid on)
inline RunOpts parse_opts(const corrla_opts* o, bool dev_ptrs, bool pca = false) {
  RunOpts r;
  const char* qr_env = std::getenv("CORRLA_QR");
  r.qr_householder = qr_env && std::strcmp(qr_env, "householder") == 0;
  const char* fu_env = std::getenv("CORRLA_POWER_FUSED");
  r.power_fused = fu_env && std::atoi(fu_env) != 0;
  if (const char* pz = std::getenv("CORRLA_TEST_POISON_CORE")) r.poison_core = std::atoi(pz);  // test hook, see RunOpts
  if (const char* mx = std::getenv("CORRLA_SKETCH_MIXED"))
    r.mixed_planes = std::strcmp(mx, "bf16x3") == 0 ? 2 : (std::strcmp(mx, "bf16x6") == 0 ? 3 : 0);
  if (const char* mp = std::getenv("CORRLA_MIXED_PROJECT")) r.mixed_project = std::atoi(mp) != 0;
  if (!o) return r;
  if (o->struct_size != sizeof(corrla_opts) && o->struct_size != kOptsSizeV1) throw Error(ST_EINVAL, "corrla_opts.struct_size mismatch");
  // seed: used as given when it is non-zero or CORRLA_SEED_EXPLICIT is set (so 0 is a usable seed); otherwise every
  // call draws a fresh sketch like the reference's unseeded thread_rng (mat_utils.rs:161-175) -- see fresh_seed()
  r.seed_explicit = o->seed != 0 || (o->flags & CORRLA_SEED_EXPLICIT) != 0;
  if (r.seed_explicit) r.seed = o->seed;
  r.omega = o->omega;
  r.omega_ld = o->omega_ld;
  r.omega_on_device = (o->flags & CORRLA_OMEGA_ON_DEVICE) != 0;
  if (r.omega_on_device && !dev_ptrs) throw Error(ST_EINVAL, "CORRLA_OMEGA_ON_DEVICE is only valid for *_dev entry points");
  if ((o->flags & CORRLA_PCA_CENTER_FUSED) && (o->flags & CORRLA_PCA_CENTER_COPY))
    throw Error(ST_EINVAL, "CORRLA_PCA_CENTER_FUSED and CORRLA_PCA_CENTER_COPY are mutually exclusive");
  r.pca_center = (o->flags & CORRLA_PCA_CENTER_FUSED) ? 1 : ((o->flags & CORRLA_PCA_CENTER_COPY) ? 2 : 0);
  r.pca_standardize = (o->flags & CORRLA_PCA_STANDARDIZE) != 0;
  if (r.pca_standardize && !pca) throw Error(ST_EINVAL, "CORRLA_PCA_STANDARDIZE is only valid for corrla_pca_* entry points");
  r.qr_householder = r.qr_householder || (o->flags & CORRLA_QR_HOUSEHOLDER) != 0;
  r.power_fused = r.power_fused || (o->flags & CORRLA_POWER_FUSED) != 0;
  if ((o->flags & CORRLA_SKETCH_BF16X3) && (o->flags & CORRLA_SKETCH_BF16X6))
    throw Error(ST_EINVAL, "CORRLA_SKETCH_BF16X3 and CORRLA_SKETCH_BF16X6 are mutually exclusive");
  if (o->flags & CORRLA_SKETCH_BF16X3) r.mixed_planes = 2;
  if (o->flags & CORRLA_SKETCH_BF16X6) r.mixed_planes = 3;
  return r;
}

// A caller's column-major buffer (exactly `cols` columns, leading dimension ld) as the destination of a product: an
// `external` Skinny, see driver.hpp.
template <class T>
inline Skinny<T> caller_skinny(T* p, int64_t rows, int64_t cols, int64_t ld) {
  Skinny<T> s;
  s.p = p;
  s.rows = rows;
  s.cols = cols;
  s.ld = ld;
  s.cols_alloc = cols;
  s.external = true;
  return s;
}

// `rows` x `cols` row-major at p: cols_readable says how far a row may be read (the zero padding included).
template <class T>
inline TallA<T> tall_over(const T* p, bool row_major, int64_t mt, int64_t nt, int64_t rows, int64_t cols, int64_t ld,
                          int64_t cols_readable) {
  TallA<T> ta;
  ta.mt = mt;
  ta.nt = nt;
  ta.row_major = row_major;
  ta.mem.p = p;
  ta.mem.rows = rows;
  ta.mem.cols = cols;
  ta.mem.ld = ld;
  ta.mem.cols_readable = cols_readable;
  return ta;
}

// The stand-in for an EMPTY shard: ONE zero row of the tall view, which adds nothing to any sum.
template <class Dev, class T>
inline TallA<T> zero_row_tall(Dev& dev, int64_t nt) {
  const int64_t ldp = round_up(nt, kLdPad);
  T* zrow = (T*)dev.alloc_bytes((size_t)ldp * sizeof(T));
  dev.memset_zero(zrow, (size_t)ldp * sizeof(T));
  return tall_over<T>(zrow, true, 1, nt, 1, nt, ldp, ldp);
}

// Bring the strided input into one of the two layouts the kernels take and describe it as the
// TALL matrix.  Host pointers are always staged (H2D) into a padded row-major device buffer;
// device pointers are used in place when 16-byte vector loads are legal, else repacked.
// force_tall (sharded / power_iter / product hooks): never transpose, see classify.
template <class Dev, class T>
inline TallA<T> stage_input(Dev& dev, bool host_ptrs, const T* a, int64_t m, int64_t n, int64_t rs, int64_t cs,
                            bool force_tall) {
  validate_matrix(a, m, n, rs, cs);
  const Layout L = classify(m, n, rs, cs, force_tall);
  constexpr int64_t VEC = 16 / (int64_t)sizeof(T);
  const int64_t mem_rows = L.row_major ? L.mt : L.nt;
  const int64_t mem_cols = L.row_major ? L.nt : L.mt;
  // strides of the memory-row-major view in the ORIGINAL array
  int64_t vrs, vcs;
  {
    const int64_t trs = L.fat ? cs : rs, tcs = L.fat ? rs : cs;  // tall view strides
    vrs = L.row_major ? trs : tcs;
    vcs = L.row_major ? tcs : trs;
  }
  const bool aligned = !L.needs_pack && (((uintptr_t)a) % 16 == 0) && (L.ld % VEC == 0) && (mem_cols % VEC == 0);
  if (!host_ptrs && aligned) return tall_over<T>(a, L.row_major, L.mt, L.nt, mem_rows, mem_cols, L.ld, mem_cols);
  const int64_t ldp = round_up(mem_cols, kLdPad);
  T* buf = (T*)dev.alloc_bytes((size_t)mem_rows * (size_t)ldp * sizeof(T));
  dev.memset_zero(buf, (size_t)mem_rows * (size_t)ldp * sizeof(T));
  if (host_ptrs) {
    if (L.needs_pack || vcs != 1) {
      std::vector<T> packed((size_t)mem_rows * (size_t)mem_cols);
      for (int64_t r = 0; r < mem_rows; ++r)
        for (int64_t c = 0; c < mem_cols; ++c) packed[(size_t)r * mem_cols + c] = a[r * vrs + c * vcs];
      dev.h2d_2d(buf, ldp, packed.data(), mem_cols, mem_cols, mem_rows);
    } else {
      dev.h2d_2d(buf, ldp, a, mem_rows == 1 ? mem_cols : vrs, mem_cols, mem_rows);
    }
  } else {
    dev.pack_strided(a, mem_rows, mem_cols, vrs, vcs, buf, ldp);
  }
  return tall_over<T>(buf, L.row_major, L.mt, L.nt, mem_rows, mem_cols, ldp, ldp);
}

// The options of one rsvd / PCA call.  Sparse and bf16-stored operands (not_dense_f32): CORRLA_POWER_FUSED and
// CORRLA_SKETCH_BF16X3 / X6 only have dense f32 kernels and are ignored, as documented for every operand outside their domain.
inline RunOpts call_opts(const corrla_opts* o, bool host_ptrs, bool sharded, bool not_dense_f32, bool pca = false) {
  RunOpts ro = parse_opts(o, !host_ptrs, pca);
  if (not_dense_f32) {
    ro.power_fused = false;
    ro.mixed_planes = 0;
  }
  ro.sharded = sharded;
  return ro;
}
template <class Dev>
inline void draw_seed(Dev& dev, RunOpts& ro) {
  if (!ro.seed_explicit && !ro.omega) ro.seed = dev.fresh_seed(/*rank_invariant=*/ro.sharded);
}

// Everything that can fail on ONE rank only (arguments in `check`; staging and workspace in `stage`, inside the call
// that this helper begins) happens before the first collective; on the sharded entry points its outcome is then agreed
// by one small all-reduce, so that a rank-local failure ends the call on every rank instead of stranding the peers in
// a collective (Dev::sharded_handshake).
template <class Dev, class Check, class Stage>
inline void prepare_call(Dev& dev, bool sharded, Check&& check, Stage&& stage) {
  bool begun = false;
  auto prepare = [&] {
    check();
    dev.begin_call();
    begun = true;
    stage();
  };
  if (!sharded) {
    prepare();
    return;
  }
  if (dev.nranks() < 1) throw Error(ST_ECOMM, "communicator not initialised");
  int local = ST_OK;
  std::string local_msg;
  try {
    prepare();
  } catch (const Error& e) {
    local = e.code;
    local_msg = e.what();
  } catch (const std::bad_alloc&) {
    local = ST_ENOMEM;
    local_msg = "host allocation failed";
  }
  if (!begun) dev.begin_call();
  const int agreed = dev.sharded_handshake(local);
  if (local != ST_OK) throw Error(local, local_msg);
  if (agreed != ST_OK)
    throw Error(agreed, "sharded call abandoned: another rank failed before the first collective (status " + std::to_string(agreed) +
                            "); this rank's arguments were valid");
}

// The end of an rsvd / PCA call: the output copies that emit() enqueued, the call's timings and counters.
template <class Dev, class T>
inline void finish_call(RsvdDriver<Dev, T>& drv, Dev& dev, Timings* tm_out, bool with_sketch_kernel_ms) {
  PhaseTimer fin;
  drv.phase(drv.tm.finalize_ms, fin);  // output copies enqueued by emit()
  dev.phase_end();
  dev.end_call();
  dev.phase_resolve(&drv.tm.total_ms);
  drv.tm.n_collectives = dev.n_collectives;
  drv.tm.collective_bytes = dev.collective_bytes;
  if (with_sketch_kernel_ms) drv.tm.sketch_kernel_ms = dev.event_elapsed_ms(0, 1);
  if (tm_out) *tm_out = drv.tm;
}

// ---- random_svd ------------------------------------------------------------------------------------------------------
// What an rsvd call is, apart from its operand.  First the arguments every rsvd entry has, in the order of its
// prototype (m is the caller's row count, of U); then the kind of call, which the entries set BY NAME: `fat` = the tall
// view is the transpose of what the caller passed, `empty_shard` = the operand is the zero-row stand-in.
template <class T>
struct RsvdCall {
  bool host_ptrs;
  int64_t m, rank, n_iter, n_oversamples;
  const corrla_opts* opts;
  T* u;
  int64_t ldu;
  T* s;
  T* vt;
  int64_t ldvt;
  Timings* tm_out;
  bool profile;
  bool sharded = false, sparse = false, fat = false, empty_shard = false;
  bool bf16 = false;  // the operand arrived in bfloat16 (in place or widened: the stage decides)
};

// The one body of random_svd (random_svd.rs:63-110) for every operand.  `validate` checks the operand and the rank;
// `stage` returns the staged tall operand.
template <class Dev, class T, class Validate, class Stage>
inline void rsvd_body(Dev& dev, const RsvdCall<T>& c, Validate&& validate, Stage&& stage) {
  const bool shard_cols = c.sharded && c.fat;
  const int64_t k = c.rank;
  RunOpts ro;
  TallA<T> ta;
  bool u_in_place = false;
  int64_t l = 0;
  Skinny<T> ut, vtall;
  T* s_dev = nullptr;
  prepare_call(
      dev, c.sharded,
      [&] {
        // (an empty shard has no rows of its sharded output factor: that pointer may be NULL)
        if ((!c.u && !(c.empty_shard && !shard_cols)) || !c.s || (!c.vt && !(c.empty_shard && shard_cols)))
          throw Error(ST_EINVAL, "output pointer is NULL");
        validate();
        if (c.ldu < c.m) throw Error(ST_EINVAL, "ldu < m");
        if (c.ldvt < c.rank) throw Error(ST_EINVAL, "ldvt < rank");
        ro = call_opts(c.opts, c.host_ptrs, c.sharded, c.sparse || c.bf16);
        draw_seed(dev, ro);
      },
      [&] {
        ta = stage();
        l = std::min<int64_t>(c.rank + c.n_oversamples, ta.nt);  // random_svd.rs:77
        if (ro.omega && ro.omega_ld < ta.nt) throw Error(ST_EINVAL, "omega_ld < min(m, n)");
        // Tall input, device pointers: the m x k factor U is produced directly in the caller's buffer (column-major,
        // ldu) -- no staging copy of the largest output.
        u_in_place = !c.fat && !c.host_ptrs && !c.empty_shard;
        ut = u_in_place ? caller_skinny(c.u, ta.mt, k, c.ldu) : dev.template alloc_skinny<T>(ta.mt, k);
        vtall = dev.template alloc_skinny<T>(ta.nt, k);
        s_dev = dev.template alloc_scalar<T>((int)k);
      });
  RsvdDriver<Dev, T> drv(dev, c.profile);
  if (c.empty_shard) drv.m_local_override_ = 0;  // the stand-in zero row is not a row of the matrix
  drv.random_svd_tall(ta, k, l, c.n_iter, ro, ut, s_dev, vtall, [&] {
    // random_svd.rs:96-109: tall -> (U, S, V^T); fat -> (V, S, U^T) of the transposed problem
    if (!c.fat) {
      if (!u_in_place && !c.empty_shard) dev.copy_out(ut, k, c.u, c.ldu, /*transpose=*/false, c.host_ptrs);
      dev.copy_out(vtall, k, c.vt, c.ldvt, /*transpose=*/true, c.host_ptrs);
    } else {
      dev.copy_out(vtall, k, c.u, c.ldu, false, c.host_ptrs);
      if (!c.empty_shard) dev.copy_out(ut, k, c.vt, c.ldvt, true, c.host_ptrs);
    }
    dev.copy_values_out(s_dev, k, c.s, c.host_ptrs);
  });
  finish_call(drv, dev, c.tm_out, /*with_sketch_kernel_ms=*/true);
}

template <class Dev, class T>
inline void rsvd_entry(Dev& dev, bool host_ptrs, bool sharded, const T* a, int64_t m, int64_t n, int64_t rs, int64_t cs,
                       int64_t rank, int64_t n_iter, int64_t n_oversamples, const corrla_opts* opts, T* u, int64_t ldu,
                       T* s, T* vt, int64_t ldvt, Timings* tm_out, bool profile) {
  // Sharded calls: the LONG side of the global matrix is split over the ranks.  Default: row shards of a tall matrix
  // (local block m_local x n).  CORRLA_SHARD_COLS: column shards of a FAT matrix (local block m x n_local): the
  // tall view of random_svd.rs:69-74 is then A^T, whose row shard is this block transposed -- a stride swap, no copy.
  const bool shard_cols = sharded && opts && (opts->flags & CORRLA_SHARD_COLS) != 0;
  // An EMPTY shard (m_local == 0 rows, or n_local == 0 columns with CORRLA_SHARD_COLS) is legal on the sharded entry
  // points -- more ranks than row blocks, ragged partitions: the rank takes part in every collective with zero
  // contributions (zero_row_tall) and writes no row of the sharded output factor.
  const bool empty_shard = sharded && m >= 0 && n >= 0 && (shard_cols ? (n == 0 && m >= 1) : (m == 0 && n >= 1));
  const int64_t short_side = shard_cols ? m : n;
  RsvdCall<T> c{host_ptrs, m, rank, n_iter, n_oversamples, opts, u, ldu, s, vt, ldvt, tm_out, profile};
  c.sharded = sharded;
  c.fat = sharded ? shard_cols : m < n;
  c.empty_shard = empty_shard;
  rsvd_body(
      dev, c,
      [&] {
        if (!empty_shard) validate_matrix(a, m, n, rs, cs);
        if (!sharded && opts && (opts->flags & CORRLA_SHARD_COLS)) throw Error(ST_EINVAL, "CORRLA_SHARD_COLS is only valid for sharded entry points");
        if (sharded) {
          if (rank < 1 || rank > short_side) throw Error(ST_EINVAL, "rank must be in [1, short side] for the sharded path");
          if (n_iter < 0 || n_oversamples < 0) throw Error(ST_EINVAL, "n_iter and n_oversamples must be >= 0");
        } else {
          validate_rank(m, n, rank, n_iter, n_oversamples);
        }
      },
      [&] {
        if (empty_shard) return zero_row_tall<Dev, T>(dev, short_side);
        return shard_cols ? stage_input<Dev, T>(dev, host_ptrs, a, n, m, cs, rs, true)
                          : stage_input<Dev, T>(dev, host_ptrs, a, m, n, rs, cs, sharded);
      });
}

// ---- PCA -------------------------------------------------------------------------------------------------------------
inline void need_two_samples(int64_t m) {
  if (m < 2) throw Error(ST_EINVAL, "PCA needs at least two samples");
}

// as RsvdCall: the entries' arguments in prototype order, then the kind of call, set by name
template <class T>
struct PcaCall {
  bool host_ptrs;
  int64_t m, n, rank, n_iter, n_oversamples;
  const corrla_opts* opts;
  T* means;
  T* s;
  T* comps;
  int64_t ldc;
  Timings* tm_out;
  bool profile;
  bool sharded = false, sparse = false;
  bool bf16 = false;  // as RsvdCall::bf16; the default centring is the fused one
};

// The one body of PcaRsvd::new (pca_rsvd.rs:56-82) for every operand: means, centring (implicit rank-1 corrections or
// a centred copy, see CORRLA_PCA_CENTER_*), random_svd of the centred matrix; keeps S and V^T.
// sharded: the SAMPLES (rows of x) are sharded over the ranks; means, S and the components come out replicated.  The
// column means and every product with the centred matrix are linear in the rows, so they are all-reduced partial sums.
// An empty shard is not supported here (the centring has no zero-contribution stand-in): it fails validation, on every
// rank alike.
// CORRLA_PCA_STANDARDIZE: the columns are divided by their standard deviation as well (PCA of the correlation matrix).
// One more pass over the operand, next to the one for the means, gives the column sums of squares (Dev::col_ss, read in
// place; row-sharded: partial sums, all-reduced); the fused form then carries the diagonal 1 / sd on the skinny side of
// every product (TallA::inv_sd_*), the copy form scales the centred copy.  Needs a backend with those kernels
// (dev_has_colvar); without them the call ends with ST_EINVAL.
// sparse: always the fused centring -- the centred operator is A X - 1 (mu^T X), A itself is never
// rewritten, so the matrix stays sparse; the means are A^T 1 / m through the same SpMM as every other product.
template <class Dev, class T, class Validate, class Stage>
inline void pca_body(Dev& dev, const PcaCall<T>& c, Validate&& validate, Stage&& stage) {
  RunOpts ro;
  TallA<T> ta;
  T* scales_out = nullptr;  // corrla_opts.scales_out: n_dim values, host or device memory as `means`
  prepare_call(
      dev, c.sharded,
      [&] {
        if (!c.means || !c.s || !c.comps) throw Error(ST_EINVAL, "output pointer is NULL");
        validate();
        if (c.ldc < c.rank) throw Error(ST_EINVAL, "ldc < rank");
        if (c.sparse) need_two_samples(c.m);  // never sharded: the sample count is known before anything is staged
        ro = call_opts(c.opts, c.host_ptrs, c.sharded, c.sparse || c.bf16, /*pca=*/true);
        if (ro.pca_standardize && !dev_has_colvar<Dev>::value)
          throw Error(ST_EINVAL, "CORRLA_PCA_STANDARDIZE: this backend has no column-variance kernels");
        // (a caller of the 32-byte layout has no scales_out field: read it only when the struct holds it)
        if (ro.pca_standardize && c.opts->struct_size >= sizeof(corrla_opts)) scales_out = (T*)c.opts->scales_out;
        if (c.sparse && ro.pca_center == 2)
          throw Error(ST_EINVAL, "CORRLA_PCA_CENTER_COPY on CSR input: a centred copy would densify the matrix (use the fused centring)");
        draw_seed(dev, ro);
      },
      [&] { ta = stage(); });
  const int64_t m_global = c.sharded ? dev.allreduce_sum_host(c.m) : c.m;  // every rank makes this call (rank-invariant)
  need_two_samples(m_global);
  const bool fat = !c.sharded && c.m < c.n;  // the tall view is x^T: its ROWS are the data columns
  RsvdDriver<Dev, T> drv(dev, c.profile);
  Skinny<T> mu = drv.column_means(ta, fat, m_global, c.sharded);
  // data columns run along the memory columns iff (tall & row-major) or (fat & column-major): tall view element (i, j)
  // is memory (i, j) when row-major, else memory (j, i); the data column index of x is j for tall input, i for fat
  const bool data_cols_along_mem_cols = (ta.row_major != fat);
  Skinny<T> sd, inv_sd;  // column standard deviations (1 for a constant column) and their reciprocals
  if (ro.pca_standardize) {
    if constexpr (dev_has_colvar<Dev>::value) {
      double* ss = dev.alloc_f64(c.n);
      if (ta.sparse)
        dev.col_ss_csr(fat ? ta.csr : ta.csr_t, (const T*)mu.p, c.m, ss);  // the CSR whose rows are the data columns
      else if (ta.bf16)
        dev.col_ss(ta.mem16, data_cols_along_mem_cols, (const T*)mu.p, ss);
      else
        dev.col_ss(ta.mem, data_cols_along_mem_cols, (const T*)mu.p, ss);
      // with the global means ss is linear in the rows: every rank's partial sums, one all-reduce of n_dim values
      if (c.sharded) dev.allreduce(ss, (size_t)c.n);
      sd = dev.template alloc_skinny<T>(c.n, 1);
      inv_sd = dev.template alloc_skinny<T>(c.n, 1);
      dev.sd_from_ss((const double*)ss, (const T*)mu.p, c.n, m_global, sd.p, inv_sd.p);
    }
  }
  TallA<T> tc = ta;
  const bool fused = c.sparse || ro.pca_center == 1 || (ro.pca_center == 0 && (sizeof(T) == 8 || c.bf16));
  if (fused) {
    // the centred matrix is never formed.  Tall view (i, j) = x(i, j) for tall inputs (means run
    // along the SHORT side), = x(j, i) for fat inputs (means run along the TALL side).
    if (!fat)
      tc.mu_short = mu.p, tc.inv_sd_short = inv_sd.p;
    else
      tc.mu_tall = mu.p, tc.inv_sd_tall = inv_sd.p;
  } else {
    // centred copy (center_mat_col clones too, mat_utils.rs:484): memory rows/cols of the staged operand
    const int64_t ldp = round_up(ta.mem.cols, kLdPad);
    T* cbuf = (T*)dev.alloc_bytes((size_t)ta.mem.rows * (size_t)ldp * sizeof(T));
    dev.memset_zero(cbuf, (size_t)ta.mem.rows * (size_t)ldp * sizeof(T));
    if constexpr (dev_has_colvar<Dev>::value) {
      dev.center_rows_cols(ta.mem.p, ta.mem.rows, ta.mem.cols, ta.mem.ld, mu.p, data_cols_along_mem_cols, cbuf, ldp, (const T*)inv_sd.p);
    } else {
      dev.center_rows_cols(ta.mem.p, ta.mem.rows, ta.mem.cols, ta.mem.ld, mu.p, data_cols_along_mem_cols, cbuf, ldp);
    }
    tc.mem.p = cbuf;
    tc.mem.ld = ldp;
    tc.mem.cols_readable = ldp;
  }
  const int64_t k = c.rank;
  const int64_t l = std::min<int64_t>(c.rank + c.n_oversamples, tc.nt);
  if (ro.omega && ro.omega_ld < tc.nt) throw Error(ST_EINVAL, "omega_ld < min(m, n)");
  Skinny<T> ut = dev.template alloc_skinny<T>(tc.mt, k);
  Skinny<T> vtall = dev.template alloc_skinny<T>(tc.nt, k);
  T* s_dev = dev.template alloc_scalar<T>((int)k);
  // the skinny that carries D^-1 into the products (n_dim x l; allocated here, outside the attempts of random_svd_tall)
  if (tc.inv_sd_short || tc.inv_sd_tall) drv.set_scale_workspace(dev.template alloc_skinny<T>(c.n, l));
  drv.random_svd_tall(tc, k, l, c.n_iter, ro, ut, s_dev, vtall, [&] {
    // components_ = vr = V^T (k x n_dim)   pca_rsvd.rs:70-71
    dev.copy_out(fat ? ut : vtall, k, c.comps, c.ldc, /*transpose=*/true, c.host_ptrs);
    dev.copy_values_out(s_dev, k, c.s, c.host_ptrs);
    dev.copy_values_out(mu.p, c.n, c.means, c.host_ptrs);
    if (scales_out) dev.copy_values_out(sd.p, c.n, scales_out, c.host_ptrs);
  });
  finish_call(drv, dev, c.tm_out, /*with_sketch_kernel_ms=*/false);
}

template <class Dev, class T>
inline void pca_entry(Dev& dev, bool host_ptrs, const T* x, int64_t m, int64_t n, int64_t rs, int64_t cs, int64_t rank,
                      int64_t n_iter, int64_t n_oversamples, const corrla_opts* opts, T* means, T* s, T* comps,
                      int64_t ldc, Timings* tm_out, bool profile, bool sharded = false) {
  PcaCall<T> c{host_ptrs, m, n, rank, n_iter, n_oversamples, opts, means, s, comps, ldc, tm_out, profile};
  c.sharded = sharded;
  pca_body(
      dev, c,
      [&] {
        validate_matrix(x, m, n, rs, cs);
        if (sharded) {
          if (rank < 1 || rank > n) throw Error(ST_EINVAL, "rank must be in [1, n_dim] for the sample-sharded PCA");
          if (n_iter < 0 || n_oversamples < 0) throw Error(ST_EINVAL, "n_iter and n_oversamples must be >= 0");
        } else {
          validate_rank(m, n, rank, n_iter, n_oversamples);
        }
      },
      [&] { return stage_input<Dev, T>(dev, host_ptrs, x, m, n, rs, cs, sharded); });
}

template <class Dev, class T>
inline void power_iter_entry(Dev& dev, bool host_ptrs, const T* a, int64_t m, int64_t n, int64_t rs, int64_t cs,
                             int64_t width, int64_t n_iter, const corrla_opts* opts, T* q, int64_t ldq) {
  if (!q) throw Error(ST_EINVAL, "q is NULL");
  validate_matrix(a, m, n, rs, cs);
  if (width < 1 || width > n) throw Error(ST_EINVAL, "width must be in [1, n]");
  if (n_iter < 0) throw Error(ST_EINVAL, "n_iter must be >= 0");
  if (ldq < m) throw Error(ST_EINVAL, "ldq < m");
  RunOpts ro = parse_opts(opts, !host_ptrs);
  if (ro.omega && ro.omega_ld < n) throw Error(ST_EINVAL, "omega_ld < n");
  if (!ro.seed_explicit && !ro.omega) ro.seed = dev.fresh_seed(false);
  dev.begin_call();
  TallA<T> ta = stage_input<Dev, T>(dev, host_ptrs, a, m, n, rs, cs, /*force_tall=*/true);
  RsvdDriver<Dev, T> drv(dev, false);
  Skinny<T> y = dev.template alloc_skinny<T>(ta.mt, width);
  Skinny<T> y2 = dev.template alloc_skinny<T>(ta.mt, width);
  drv.power_iter(ta, width, n_iter, ro, y, y2);
  dev.copy_out(y, width, q, ldq, false, host_ptrs);
  dev.end_call();
}

// ---- product hooks ---------------------------------------------------------------------------------------------------
// res = beta * op(A) * X on device pointers, A as given (m x n, never transposed); `validate` checks the operand,
// `stage` returns it as the tall operand.  A dense product lands in a padded Skinny and is copied out; a sparse one is
// written straight into the caller's buffer (an `external` Skinny: ld = ldres, exactly l columns): the hook shows what
// the SpMM kernels store, and a caller who pads res can see that nothing else is touched.
template <class Dev, class T, class Validate, class Stage>
inline void product_body(Dev& dev, int trans, int64_t m, int64_t n, const T* x, int64_t ldx, int64_t l, T beta, T* res,
                         int64_t ldres, Timings* tm_out, Validate&& validate, Stage&& stage) {
  if (!x || !res) throw Error(ST_EINVAL, "x or res is NULL");
  validate();
  if (l < 1) throw Error(ST_EINVAL, "l must be >= 1");
  const int64_t xin = trans ? m : n, xout = trans ? n : m;
  if (ldx < xin || ldres < xout) throw Error(ST_EINVAL, "leading dimension too small");
  dev.begin_call();
  TallA<T> ta = stage();
  RsvdDriver<Dev, T> drv(dev, false);
  if (!ta.sparse) drv.mixed_planes_ = parse_opts(nullptr, true).mixed_planes;  // CORRLA_SKETCH_MIXED (the hooks take no opts)
  Skinny<T> xs = dev.template alloc_skinny<T>(xin, l);
  dev.copy_in_skinny(x, ldx, xs);
  Skinny<T> out = ta.sparse ? caller_skinny(res, xout, l, ldres) : dev.template alloc_skinny<T>(xout, l);
  T* beta_dev = dev.template alloc_scalar<T>(1);
  dev.store_values(&beta, (int64_t)1, beta_dev, /*dst_is_host=*/false);
  if (trans)
    drv.at_times(ta, xs, out, beta_dev, false);
  else
    drv.a_times(ta, xs, out, beta_dev);
  if (!out.external) dev.copy_out(out, l, res, ldres, false, false);
  dev.end_call();
  if (tm_out) {
    tm_out->n_mixed_products = drv.tm.n_mixed_products;
    tm_out->n_bf16_products = drv.tm.n_bf16_products;
  }
}

// mat_utils.rs:20-33 for the two hot-path shapes
template <class Dev, class T>
inline void matmul_entry(Dev& dev, int trans, const T* a, int64_t m, int64_t n, int64_t rs, int64_t cs, const T* x,
                         int64_t ldx, int64_t l, T beta, T* res, int64_t ldres, Timings* tm_out = nullptr) {
  product_body(
      dev, trans, m, n, x, ldx, l, beta, res, ldres, tm_out, [&] { validate_matrix(a, m, n, rs, cs); },
      [&] { return stage_input<Dev, T>(dev, false, a, m, n, rs, cs, true); });
}

// ---- CSR sparse input ------------------------------------------------------------------------------------------------
// A arrives as CSR (values, int32 column indices, int64 row_ptr), unsharded.  Host arrays are uploaded and take the
// device path, so there is one validation and one transposition path.  Only instantiated for backends that carry the
// SpMM kernels (dev_has_spmm).
inline void validate_csr_args(const void* values, const void* ci, const void* rp, int64_t m, int64_t n, int64_t nnz) {
  if (!values || !ci || !rp) throw Error(ST_EINVAL, "values, col_idx or row_ptr is NULL");
  if (m < 1 || n < 1) throw Error(ST_EINVAL, "matrix must have at least one row and one column");
  if (m > 0x7fffffff || n > 0x7fffffff) throw Error(ST_EINVAL, "CSR input: m and n must be below 2^31");
  // an all-zero matrix has no range to find (every sketch is zero); rejected rather than run
  if (nnz < 1) throw Error(ST_EINVAL, "CSR input: nnz must be >= 1");
  if (nnz > 0x7fffffff) throw Error(ST_EINVAL, "CSR input: nnz must be below 2^31");
}

// Uploads (host pointers), validates on the device, transposes once, and describes the result as the TALL operand:
// the caller's CSR is the tall view for m >= n and its transpose for a fat input (m < n, strict) -- the two simply swap.
template <class Dev, class T>
inline TallA<T> stage_csr(Dev& dev, bool host_ptrs, const T* values, const int32_t* ci, const int64_t* rp, int64_t m, int64_t n,
                          int64_t nnz, bool keep_orientation) {
  CsrView<T> a;
  a.rows = m;
  a.cols = n;
  a.nnz = nnz;
  if (host_ptrs) {
    // row_ptr[m] decides how much of the two nnz-sized arrays exists: check it on the host before the copies read them
    if (rp[m] != nnz) throw Error(ST_EINVAL, "invalid CSR matrix: row_ptr[m] != nnz");
    T* dv = (T*)dev.alloc_bytes(sizeof(T) * (size_t)nnz);
    int32_t* dc = (int32_t*)dev.alloc_bytes(sizeof(int32_t) * (size_t)nnz);
    int64_t* dr = (int64_t*)dev.alloc_bytes(sizeof(int64_t) * (size_t)(m + 1));
    dev.h2d_bytes(dv, values, sizeof(T) * (size_t)nnz);
    dev.h2d_bytes(dc, ci, sizeof(int32_t) * (size_t)nnz);
    dev.h2d_bytes(dr, rp, sizeof(int64_t) * (size_t)(m + 1));
    a.val = dv;
    a.ci = dc;
    a.rp = dr;
  } else {
    a.val = values;
    a.ci = ci;
    a.rp = rp;
  }
  dev.csr_plan(a, /*check_idx=*/true);  // throws ST_EINVAL before any gather
  CsrView<T> at = dev.csr_transpose(a);
  dev.csr_plan(at, /*check_idx=*/false);
  TallA<T> ta;
  ta.sparse = true;
  const bool fat = !keep_orientation && m < n;
  ta.mt = fat ? n : m;
  ta.nt = fat ? m : n;
  ta.csr = fat ? at : a;
  ta.csr_t = fat ? a : at;
  return ta;
}

template <class Dev, class T>
inline void rsvd_csr_entry(Dev& dev, bool host_ptrs, const T* values, const int32_t* ci, const int64_t* rp, int64_t m, int64_t n,
                           int64_t nnz, int64_t rank, int64_t n_iter, int64_t n_oversamples, const corrla_opts* opts, T* u,
                           int64_t ldu, T* s, T* vt, int64_t ldvt, Timings* tm_out, bool profile) {
  static_assert(dev_has_spmm<Dev>::value, "CSR entries need a backend with SpMM kernels");
  RsvdCall<T> c{host_ptrs, m, rank, n_iter, n_oversamples, opts, u, ldu, s, vt, ldvt, tm_out, profile};
  c.sparse = true;
  c.fat = m < n;
  rsvd_body(
      dev, c,
      [&] {
        validate_csr_args(values, ci, rp, m, n, nnz);
        validate_rank(m, n, rank, n_iter, n_oversamples);
      },
      [&] { return stage_csr<Dev, T>(dev, host_ptrs, values, ci, rp, m, n, nnz, false); });
}

template <class Dev, class T>
inline void pca_csr_entry(Dev& dev, bool host_ptrs, const T* values, const int32_t* ci, const int64_t* rp, int64_t m, int64_t n,
                          int64_t nnz, int64_t rank, int64_t n_iter, int64_t n_oversamples, const corrla_opts* opts, T* means,
                          T* s, T* comps, int64_t ldc, Timings* tm_out, bool profile) {
  static_assert(dev_has_spmm<Dev>::value, "CSR entries need a backend with SpMM kernels");
  PcaCall<T> c{host_ptrs, m, n, rank, n_iter, n_oversamples, opts, means, s, comps, ldc, tm_out, profile};
  c.sparse = true;
  pca_body(
      dev, c,
      [&] {
        validate_csr_args(values, ci, rp, m, n, nnz);
        validate_rank(m, n, rank, n_iter, n_oversamples);
      },
      [&] { return stage_csr<Dev, T>(dev, host_ptrs, values, ci, rp, m, n, nnz, false); });
}

// res = beta * op(S) * X for a device CSR matrix S (test hook, the sparse twin of matmul_entry)
template <class Dev, class T>
inline void spmm_entry(Dev& dev, int trans, const T* values, const int32_t* ci, const int64_t* rp, int64_t m, int64_t n, int64_t nnz,
                       const T* x, int64_t ldx, int64_t l, T beta, T* res, int64_t ldres) {
  static_assert(dev_has_spmm<Dev>::value, "CSR entries need a backend with SpMM kernels");
  product_body(
      dev, trans, m, n, x, ldx, l, beta, res, ldres, (Timings*)nullptr, [&] { validate_csr_args(values, ci, rp, m, n, nnz); },
      [&] { return stage_csr<Dev, T>(dev, false, values, ci, rp, m, n, nnz, /*keep_orientation=*/true); });
}

// ---- dense bf16 input ------------------------------------------------------------------------------------------------
// A arrives in bfloat16 (bit patterns, strides in elements); every other array of the call is f32 and the call is the f32
// call on the same values.  The stage decides ONCE, from the layout, the alignment and the sketch width l, whether both
// tall products of the call are in the domain of gemm_bf16a_kernel (Dev::bf16a_fits): then they run on A in place and
// A is never widened or copied (host pointers: the 2-byte matrix is staged, H2D of 2 bytes per element); otherwise A
// is widened once into a padded f32 workspace and the call proceeds as the plain f32 call it then is -- never half and
// half.  Only instantiated for backends that carry the kernel (dev_has_bf16in).
template <class Dev>
inline TallA<float> stage_bf16(Dev& dev, bool host_ptrs, const uint16_t* a, int64_t m, int64_t n, int64_t rs, int64_t cs,
                               bool force_tall, int64_t l, bool force_widen) {
  static_assert(dev_has_bf16in<Dev>::value, "bf16 entries need a backend with the bf16-input kernel");
  validate_matrix(a, m, n, rs, cs);
  const Layout L = classify(m, n, rs, cs, force_tall);
  const int64_t mem_rows = L.row_major ? L.mt : L.nt;
  const int64_t mem_cols = L.row_major ? L.nt : L.mt;
  const int64_t trs = L.fat ? cs : rs, tcs = L.fat ? rs : cs;  // tall view strides
  const int64_t vrs = L.row_major ? trs : tcs, vcs = L.row_major ? tcs : trs;  // strides of the memory-row-major view
  const int64_t ldp = round_up(mem_cols, kLdPad);
  // the 2-byte matrix as the device sees it: src + r * src_rs + c * src_cs
  const uint16_t* src = a;
  int64_t src_rs = vrs, src_cs = vcs;
  Big<uint16_t> b16;  // a row-major view of it, when there is one
  if (host_ptrs) {
    uint16_t* buf = (uint16_t*)dev.alloc_bytes((size_t)mem_rows * (size_t)ldp * sizeof(uint16_t));
    dev.memset_zero(buf, (size_t)mem_rows * (size_t)ldp * sizeof(uint16_t));
    if (L.needs_pack || vcs != 1) {
      std::vector<uint16_t> packed((size_t)mem_rows * (size_t)mem_cols);
      for (int64_t r = 0; r < mem_rows; ++r)
        for (int64_t c = 0; c < mem_cols; ++c) packed[(size_t)r * mem_cols + c] = a[r * vrs + c * vcs];
      dev.h2d_2d(buf, ldp, packed.data(), mem_cols, mem_cols, mem_rows);
    } else {
      dev.h2d_2d(buf, ldp, a, mem_rows == 1 ? mem_cols : vrs, mem_cols, mem_rows);
    }
    src = buf, src_rs = ldp, src_cs = 1;
    b16.p = buf, b16.rows = mem_rows, b16.cols = mem_cols, b16.ld = ldp, b16.cols_readable = ldp;
  } else if (!L.needs_pack) {
    b16.p = a, b16.rows = mem_rows, b16.cols = mem_cols, b16.ld = L.ld, b16.cols_readable = mem_cols;
  }
  if (!force_widen && b16.p && dev.bf16a_fits(b16, l)) {
    TallA<float> ta;
    ta.mt = L.mt;
    ta.nt = L.nt;
    ta.row_major = L.row_major;
    ta.bf16 = true;
    ta.mem16 = b16;
    return ta;
  }
  float* wide = (float*)dev.alloc_bytes((size_t)mem_rows * (size_t)ldp * sizeof(float));
  dev.memset_zero(wide, (size_t)mem_rows * (size_t)ldp * sizeof(float));
  dev.widen_bf16(src, mem_rows, mem_cols, src_rs, src_cs, wide, ldp);
  return tall_over<float>(wide, L.row_major, L.mt, L.nt, mem_rows, mem_cols, ldp, ldp);
}

template <class Dev>
inline void rsvd_bf16_entry(Dev& dev, bool host_ptrs, const uint16_t* a, int64_t m, int64_t n, int64_t rs, int64_t cs,
                            int64_t rank, int64_t n_iter, int64_t n_oversamples, const corrla_opts* opts, float* u, int64_t ldu,
                            float* s, float* vt, int64_t ldvt, Timings* tm_out, bool profile) {
  RsvdCall<float> c{host_ptrs, m, rank, n_iter, n_oversamples, opts, u, ldu, s, vt, ldvt, tm_out, profile};
  c.fat = m < n;
  c.bf16 = true;
  rsvd_body(
      dev, c,
      [&] {
        validate_matrix(a, m, n, rs, cs);
        if (opts && (opts->flags & CORRLA_SHARD_COLS)) throw Error(ST_EINVAL, "CORRLA_SHARD_COLS is only valid for sharded entry points");
        validate_rank(m, n, rank, n_iter, n_oversamples);
      },
      [&] {
        const int64_t l = std::min<int64_t>(rank + n_oversamples, std::min(m, n));
        return stage_bf16(dev, host_ptrs, a, m, n, rs, cs, false, l, false);
      });
}

// PCA of bf16 data: the fused centring by default (A stays in place, the means are A^T 1 / m through the same product
// kernel); CORRLA_PCA_CENTER_COPY needs an f32 copy to centre, so that call runs widened.
template <class Dev>
inline void pca_bf16_entry(Dev& dev, bool host_ptrs, const uint16_t* x, int64_t m, int64_t n, int64_t rs, int64_t cs, int64_t rank,
                           int64_t n_iter, int64_t n_oversamples, const corrla_opts* opts, float* means, float* s, float* comps,
                           int64_t ldc, Timings* tm_out, bool profile) {
  PcaCall<float> c{host_ptrs, m, n, rank, n_iter, n_oversamples, opts, means, s, comps, ldc, tm_out, profile};
  c.bf16 = true;
  pca_body(
      dev, c,
      [&] {
        validate_matrix(x, m, n, rs, cs);
        validate_rank(m, n, rank, n_iter, n_oversamples);
      },
      [&] {
        const int64_t l = std::min<int64_t>(rank + n_oversamples, std::min(m, n));
        const bool copy = opts && (opts->flags & CORRLA_PCA_CENTER_COPY) != 0;
        return stage_bf16(dev, host_ptrs, x, m, n, rs, cs, false, l, copy);
      });
}

// res = beta * op(A) * X for a device bf16 matrix A and f32 X (test hook, the bf16 twin of matmul_entry)
template <class Dev>
inline void matmul_bf16_entry(Dev& dev, int trans, const uint16_t* a, int64_t m, int64_t n, int64_t rs, int64_t cs, const float* x,
                              int64_t ldx, int64_t l, float beta, float* res, int64_t ldres, Timings* tm_out) {
  product_body(
      dev, trans, m, n, x, ldx, l, beta, res, ldres, tm_out, [&] { validate_matrix(a, m, n, rs, cs); },
      [&] { return stage_bf16(dev, false, a, m, n, rs, cs, true, l, false); });
}

// ---- covariance / correlation matrices (corrla_cov_*) -------------------------------------------------------------------
// Argument checks of every corrla_cov_* entry, then `run` -- on a backend that carries the symmetric rank-k kernel
// (dev_has_syrk); any other backend ends the call with EINVAL, never with another way of computing the matrix.

// The arguments of the prototype, in its order.  means_out / scales_out are written when the flags ask for them (the stage
// decides); the overlap check takes them as given.
template <class T>
struct CovCall {
  const T* x;
  int64_t m, n, rs, cs;
  uint64_t flags;
  int ddof;
  T* means_out;
  T* scales_out;
  T* c;
  int64_t ldc;
  int* route_out;
  Span x_span() const { return Span(x, m, n, rs, cs, "x"); }
  Span c_span() const { return Span(c, n, n, ldc, "c"); }
  Span means_span() const { return Span(means_out, 1, n, n, "means_out"); }
  Span scales_span() const { return Span(scales_out, 1, n, n, "scales_out"); }
};

template <class Dev, class T, class Run>
inline void cov_entry(Dev&, const CovCall<T>& c, Run&& run) {
  if (c.route_out) *c.route_out = 0;
  if (c.flags & ~(uint64_t)(CORRLA_COV_CORRELATION | CORRLA_COV_NO_CENTER)) throw Error(ST_EINVAL, "cov: unknown flag");
  if ((c.flags & CORRLA_COV_CORRELATION) && (c.flags & CORRLA_COV_NO_CENTER))
    throw Error(ST_EINVAL, "CORRLA_COV_CORRELATION and CORRLA_COV_NO_CENTER are mutually exclusive");
  if (c.ddof != 0 && c.ddof != 1) throw Error(ST_EINVAL, "cov: ddof must be 0 or 1");
  if (!c.x || !c.c) throw Error(ST_EINVAL, "cov: x or c is NULL");
  if (c.n < 1 || c.m < 1) throw Error(ST_EINVAL, "cov: empty matrix");
  if (c.m - c.ddof < 1) throw Error(ST_EINVAL, "cov: n_samples - ddof < 1");
  if (c.ldc < c.n) throw Error(ST_EINVAL, "cov: ldc < n");
  if (c.rs < 0 || c.cs < 0) throw Error(ST_EINVAL, "cov: negative strides are not supported");
  const Span in[1] = {c.x_span()};
  const Span out[3] = {c.c_span(), c.means_span(), c.scales_span()};
  no_overlap("cov", in, 1, out, 3);
  on_backend_with<dev_has_syrk<Dev>>(run, "symmetric rank-k kernel", "corrla_cov_*");
}

// ---- the fitted PCA model on the device (corrla_pca_transform_* / corrla_pca_inverse_*, pca_rsvd.rs:43-52) ---------------
// Argument checks of every entry, then `run` -- on a backend that carries the back-projection kernel (dev_has_pca_apply);
// any other backend ends the call with EINVAL, never with another way of computing the result.

// What a transform call is, apart from its operand: the arguments of the prototype after the operand, in its order.
template <class T>
struct PcaTransformCall {
  int64_t m, n;
  const T* means;
  const T* scales;
  const T* comps;
  int64_t ldc, k;
  uint64_t flags;
  T* scores;
  int64_t ld_scores;
  T* resid_out;
  T* means_out;
  bool own_means() const { return (flags & CORRLA_PCA_APPLY_OWN_MEANS) != 0; }
  // 1 fused, 2 centred-and-scaled copy; the defaults of corrla_pca_*: fused for f64, the copy for f32
  int centring() const {
    return (flags & CORRLA_PCA_CENTER_FUSED) ? 1 : ((flags & CORRLA_PCA_CENTER_COPY) ? 2 : (sizeof(T) == 8 ? 1 : 2));
  }
  // own_means: `means` is ignored and means_out is written; otherwise the other way round
  Span means_span() const { return own_means() ? Span() : Span(means, 1, n, n, "means"); }
  Span scales_span() const { return Span(scales, 1, n, n, "scales"); }
  Span comps_span() const { return Span(comps, n, k, ldc, "components"); }
  Span scores_span() const { return Span(scores, k, m, ld_scores, "scores"); }
  Span resid_span() const { return Span(resid_out, 1, m, m, "resid_out"); }
  Span means_out_span() const { return own_means() ? Span(means_out, 1, n, n, "means_out") : Span(); }
};

// `operand`: the spans of the target (x, or the three CSR arrays), checked for overlap with the outputs
template <class Dev, class T, class Run>
inline void pca_transform_entry(Dev&, const PcaTransformCall<T>& c, bool sparse, const Span* operand, int n_operand, Run&& run) {
  const char* who = sparse ? "pca_transform_csr" : "pca_transform";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  if (c.flags & ~(uint64_t)(CORRLA_PCA_CENTER_FUSED | CORRLA_PCA_CENTER_COPY | CORRLA_PCA_APPLY_OWN_MEANS)) bad("unknown flag");
  if ((c.flags & CORRLA_PCA_CENTER_FUSED) && (c.flags & CORRLA_PCA_CENTER_COPY))
    bad("CORRLA_PCA_CENTER_FUSED and CORRLA_PCA_CENTER_COPY are mutually exclusive");
  if (sparse && (c.flags & CORRLA_PCA_CENTER_COPY)) bad("CORRLA_PCA_CENTER_COPY on CSR input: a centred copy would densify the matrix");
  if (c.m < 1 || c.n < 1) bad("m and n must be >= 1");
  if (c.k < 1 || c.k > c.n) bad("k must be in [1, n]");
  if (!c.comps) bad("components is NULL");
  if (!c.scores) bad("scores is NULL");
  if (c.ldc < c.k) bad("ldc < k");
  if (c.ld_scores < c.m) bad("ld_scores < m");
  if (sparse && c.resid_out) bad("resid_out must be NULL: the residual over a sparse row's implicit zeros is a dense computation");
  Span in[6] = {c.means_span(), c.scales_span(), c.comps_span()};
  int n_in = 3;
  for (int i = 0; i < n_operand && n_in < 6; ++i) in[n_in++] = operand[i];
  const Span out[3] = {c.scores_span(), c.resid_span(), c.means_out_span()};
  no_overlap(who, in, n_in, out, 3);
  on_backend_with<dev_has_pca_apply<Dev>>(run, "PCA back-projection kernel", "corrla_pca_transform_*");
}

// the arguments of the prototype, in its order
template <class T>
struct PcaInverseCall {
  const T* scores;
  int64_t m, k, ld_scores;
  const T* means;
  const T* scales;
  const T* comps;
  int64_t ldc, n;
  T* out;
  int64_t row_stride_out;
  Span scores_span() const { return Span(scores, k, m, ld_scores, "scores"); }
  Span means_span() const { return Span(means, 1, n, n, "means"); }
  Span scales_span() const { return Span(scales, 1, n, n, "scales"); }
  Span comps_span() const { return Span(comps, n, k, ldc, "components"); }
  Span out_span() const { return Span(out, m, n, row_stride_out, "out"); }
};

template <class Dev, class T, class Run>
inline void pca_inverse_entry(Dev&, const PcaInverseCall<T>& c, Run&& run) {
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string("pca_inverse: ") + what); };
  if (c.m < 1 || c.n < 1) bad("m and n must be >= 1");
  if (c.k < 1 || c.k > c.n) bad("k must be in [1, n]");
  if (!c.scores) bad("scores is NULL");
  if (!c.comps) bad("components is NULL");
  if (!c.out) bad("out is NULL");
  if (c.ldc < c.k) bad("ldc < k");
  if (c.ld_scores < c.m) bad("ld_scores < m");
  if (c.row_stride_out < c.n && c.m > 1) bad("row_stride_out < n");
  const Span in[4] = {c.scores_span(), c.means_span(), c.scales_span(), c.comps_span()};
  const Span out[1] = {c.out_span()};
  no_overlap("pca_inverse", in, 4, out, 1);
  on_backend_with<dev_has_pca_apply<Dev>>(run, "PCA back-projection kernel", "corrla_pca_inverse_*");
}

// ---- radial-basis-function kernel matrices (corrla_rbf_matrix_* / corrla_rbf_apply_*, interp_utils.rs:96-129, 146-153) ------
// Argument checks of every entry, then `run` -- on a backend that carries the kernels (dev_has_rbf); any other backend ends
// the call with EINVAL, never with another way of computing the result.
template <class T>
struct RbfCall {
  const T* xq;
  int64_t n_q, ldq;
  const T* xs;
  int64_t n_s, ldxs, dim;
  int kernel;
  double eps;
  int poly_degree;  // APPLY: < 0 no tail
  const T* coeffs;  // APPLY: (n_s + n_poly) x n_rhs, row stride ldw
  int64_t ldw, n_rhs;
  T* out;           // MATRIX: n_q x n_s; APPLY: n_q x n_rhs; row stride ld_out
  int64_t ld_out;
  int64_t n_poly() const { return rbf_poly_terms(dim, poly_degree); }
  // apply: the call is corrla_rbf_apply_* (coefficients in, n_rhs columns out), else corrla_rbf_matrix_* (n_s columns out)
  Span xq_span() const { return Span(xq, n_q, dim, ldq, "xq"); }
  Span xs_span() const { return Span(xs, n_s, dim, ldxs, "xs"); }
  Span coeffs_span(bool apply) const { return apply ? Span(coeffs, n_s + n_poly(), n_rhs, ldw, "coeffs") : Span(); }
  Span out_span(bool apply) const { return Span(out, n_q, apply ? n_rhs : n_s, ld_out, "out"); }
};

template <class Dev, class T, class Run>
inline void rbf_entry(Dev&, const RbfCall<T>& c, bool apply, Run&& run) {
  const char* who = apply ? "rbf_apply" : "rbf_matrix";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  if (!c.xq) bad("xq is NULL");
  if (!c.xs) bad("xs is NULL");
  if (!c.out) bad("out is NULL");
  if (c.n_q < 1) bad("n_q must be >= 1");
  if (c.n_s < 1) bad("n_s must be >= 1");
  if (c.dim < 1 || c.dim > k::kRbfMaxDim) bad("dim must be in [1, 128]");
  if (c.kernel < 1 || c.kernel > 4) bad("kernel must be in [1, 4]");
  if (!std::isfinite(c.eps)) bad("eps must be finite");
  if (c.ldq < c.dim) bad("ldq < dim");
  if (c.ldxs < c.dim) bad("lds < dim");
  if (apply) {
    if (!c.coeffs) bad("coeffs is NULL");
    if (c.n_rhs < 1) bad("n_rhs must be >= 1");
    if (c.ldw < c.n_rhs) bad("ldw < n_rhs");
    if (c.ld_out < c.n_rhs) bad("ld_out < n_rhs");
  } else if (c.ld_out < c.n_s) {
    bad("ld_out < n_s");
  }
  const Span in[3] = {c.xq_span(), c.xs_span(), c.coeffs_span(apply)};
  const Span out[1] = {c.out_span(apply)};
  no_overlap(who, in, 3, out, 1);
  on_backend_with<dev_has_rbf<Dev>>(run, "radial-basis-function kernels", "corrla_rbf_*");
}
template <class Dev, class T, class Run>
inline void rbf_apply_entry(Dev& dev, const RbfCall<T>& c, Run&& run) {
  rbf_entry<Dev, T>(dev, c, true, run);
}
template <class Dev, class T, class Run>
inline void rbf_matrix_entry(Dev& dev, const RbfCall<T>& c, Run&& run) {
  rbf_entry<Dev, T>(dev, c, false, run);
}

// ---- polynomial response surfaces (corrla_polyfit_gram_* / corrla_poly_eval_*, stats_corr.rs:146-249) ------------------------
// Argument checks of every entry, then `run` -- on a backend that carries the kernels (dev_has_polyfit); any other backend
// ends the call with EINVAL, never with another way of computing the result.
template <class T>
struct PolyGramCall {
  const T* x;
  int64_t m, kf, ldx;
  const T* y;       // m x r, row stride ldy; ignored when r == 0
  int64_t r, ldy;
  int degree, normalize;
  double* g;        // (p + r) x (p + r), row stride ldg
  int64_t ldg;
  double* means;    // kf each, written when normalize is set; nullable
  double* scales;
  int64_t order() const { return poly_terms(kf, degree) + r; }
  Span x_span() const { return Span(x, m, kf, ldx, "x"); }
  Span y_span() const { return r > 0 ? Span(y, m, r, ldy, "y") : Span(); }
  Span g_span() const { return Span(g, order(), order(), ldg, "G"); }
  Span means_span() const { return normalize != 0 ? Span(means, 1, kf, kf, "means") : Span(); }
  Span scales_span() const { return normalize != 0 ? Span(scales, 1, kf, kf, "scales") : Span(); }
};

template <class Dev, class T, class Run>
inline void polyfit_gram_entry(Dev&, const PolyGramCall<T>& c, Run&& run) {
  const char* who = "polyfit_gram";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  if (!c.x) bad("x is NULL");
  if (!c.g) bad("G is NULL");
  if (c.m < 1) bad("m must be >= 1");
  if (c.kf < 1 || c.kf > k::kPolyMaxK) bad("k must be in [1, 128]");
  if (c.degree != 1 && c.degree != 2) bad("degree must be 1 or 2");
  if (c.r < 0 || c.r > k::kPolyMaxRhs) bad("r must be in [0, 64]");
  if (c.normalize != 0 && c.normalize != 1) bad("normalize must be 0 or 1");
  if (c.ldx < c.kf) bad("ldx < k");
  if (c.r > 0 && !c.y) bad("y is NULL");
  if (c.r > 0 && c.ldy < c.r) bad("ldy < r");
  if (c.ldg < c.order()) bad("ldg < p + r");
  const Span in[2] = {c.x_span(), c.y_span()};
  const Span out[3] = {c.g_span(), c.means_span(), c.scales_span()};
  no_overlap(who, in, 2, out, 3);
  on_backend_with<dev_has_polyfit<Dev>>(run, "polynomial response-surface kernels", "corrla_polyfit_gram_*");
}

template <class T>
struct PolyEvalCall {
  const T* x;
  int64_t m, kf, ldx;
  const double* coeffs;  // p x r, row stride ldc
  int64_t ldc, r;
  int degree;
  T* out;                // m x r, row stride ld_out
  int64_t ld_out;
  T* jac;                // nullable: r slabs of m x kf, row stride ld_jac
  int64_t ld_jac;
  int64_t p() const { return poly_terms(kf, degree); }
  Span x_span() const { return Span(x, m, kf, ldx, "x"); }
  Span coeffs_span() const { return Span(coeffs, p(), r, ldc, "coeffs"); }
  Span out_span() const { return Span(out, m, r, ld_out, "out"); }
  Span jac_span() const { return Span(jac, r * m, kf, ld_jac, "jac"); }  // empty without jac
};

template <class Dev, class T, class Run>
inline void poly_eval_entry(Dev&, const PolyEvalCall<T>& c, Run&& run) {
  const char* who = "poly_eval";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  if (!c.x) bad("x is NULL");
  if (!c.coeffs) bad("coeffs is NULL");
  if (!c.out) bad("out is NULL");
  if (c.m < 1) bad("m must be >= 1");
  if (c.kf < 1 || c.kf > k::kPolyMaxK) bad("k must be in [1, 128]");
  if (c.degree != 1 && c.degree != 2) bad("degree must be 1 or 2");
  if (c.r < 1 || c.r > k::kPolyMaxRhs) bad("r must be in [1, 64]");
  if (c.ldx < c.kf) bad("ldx < k");
  if (c.ldc < c.r) bad("ldc < r");
  if (c.ld_out < c.r) bad("ld_out < r");
  if (c.jac && c.ld_jac < c.kf) bad("ld_jac < k");
  const Span in[2] = {c.x_span(), c.coeffs_span()};
  const Span out[2] = {c.out_span(), c.jac_span()};
  no_overlap(who, in, 2, out, 2);
  on_backend_with<dev_has_polyfit<Dev>>(run, "polynomial response-surface kernels", "corrla_poly_eval_*");
}

// ---- kernel density estimates (corrla_kde_eval_* / corrla_kde_nll_*, univariate_rv.rs:165-170, 423-444) ----------------------
// Argument checks of every entry, then `run` -- on a backend that carries the kernels (dev_has_kde); any other backend ends
// the call with EINVAL, never with another way of computing the result.
template <class T>
struct KdeEvalCall {
  const T* x;  // n_q points, element stride incx
  int64_t n_q, incx;
  const T* s;  // n_s supports, element stride incs
  int64_t n_s, incs;
  double h;
  int what;    // 0 pdf, 1 cdf, 2 logpdf
  T* out;      // n_q values, element stride inco
  int64_t inco;
  Span x_span() const { return Span(x, n_q, 1, incx, "x"); }
  Span s_span() const { return Span(s, n_s, 1, incs, "s"); }
  Span out_span() const { return Span(out, n_q, 1, inco, "out"); }
};

template <class Dev, class T, class Run>
inline void kde_eval_entry(Dev&, const KdeEvalCall<T>& c, Run&& run) {
  const char* who = "kde_eval";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  if (!c.x) bad("x is NULL");
  if (!c.s) bad("s is NULL");
  if (!c.out) bad("out is NULL");
  if (c.n_q < 1) bad("n_q must be >= 1");
  if (c.n_s < 1) bad("n_s must be >= 1");
  if (c.incx < 1) bad("incx must be >= 1");
  if (c.incs < 1) bad("incs must be >= 1");
  if (c.inco < 1) bad("inco must be >= 1");
  if (!std::isfinite(c.h) || !(c.h > 0.0)) bad("h must be finite and > 0");
  if (c.what < 0 || c.what > 2) bad("what must be 0 (pdf), 1 (cdf) or 2 (logpdf)");
  const Span in[2] = {c.x_span(), c.s_span()};
  const Span out[1] = {c.out_span()};
  no_overlap(who, in, 2, out, 1);
  on_backend_with<dev_has_kde<Dev>>(run, "kernel-density kernels", "corrla_kde_eval_*");
}

template <class T>
struct KdeNllCall {
  const T* x;       // n_t test points, element stride incx
  int64_t n_t, incx;
  const T* s;
  int64_t n_s, incs;
  const double* h;  // n_h bandwidths, always on the host
  int64_t n_h;
  double* nll;      // n_h
  double* dnll;     // n_h, nullable
  Span x_span() const { return Span(x, n_t, 1, incx, "x"); }
  Span s_span() const { return Span(s, n_s, 1, incs, "s"); }
  Span nll_span() const { return Span(nll, 1, n_h, n_h, "nll"); }
  Span dnll_span() const { return Span(dnll, 1, n_h, n_h, "dnll"); }  // empty without dnll
};

template <class Dev, class T, class Run>
inline void kde_nll_entry(Dev&, const KdeNllCall<T>& c, Run&& run) {
  const char* who = "kde_nll";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  if (!c.x) bad("x is NULL");
  if (!c.s) bad("s is NULL");
  if (!c.h) bad("h is NULL");
  if (!c.nll) bad("nll is NULL");
  if (c.n_t < 1) bad("n_t must be >= 1");
  if (c.n_s < 1) bad("n_s must be >= 1");
  if (c.incx < 1) bad("incx must be >= 1");
  if (c.incs < 1) bad("incs must be >= 1");
  if (c.n_h < 1 || c.n_h > k::kKdeMaxH) bad("n_h must be in [1, 64]");
  for (int64_t b = 0; b < c.n_h; ++b)
    if (!std::isfinite(c.h[b]) || !(c.h[b] > 0.0)) bad("every h must be finite and > 0");
  const Span in[2] = {c.x_span(), c.s_span()};
  const Span out[2] = {c.nll_span(), c.dnll_span()};
  no_overlap(who, in, 2, out, 2);
  on_backend_with<dev_has_kde<Dev>>(run, "kernel-density kernels", "corrla_kde_nll_*");
}

// ---- dense LU solve and the RBF fit on it (corrla_lu_solve_* / corrla_rbffit_system_* / corrla_rbffit_*) ------------------------
// Argument checks of every entry -- the limits of n and n_rhs are the plan's (lu_plan names the argument it rejects) -- then
// `run`, on a backend that carries the kernels (dev_has_lu).  f64 only.
struct LuSolveCall {
  // host entry: a and b are read, x is written.  Device entry: a_rw becomes LU, b_rw becomes X, ipiv (nullable) is written.
  const double* a;
  int64_t n, lda;
  const double* b;
  int64_t n_rhs, ldb;
  double* x;
  int64_t ldx;
  double* a_rw;
  double* b_rw;
  int64_t* ipiv;
  Span a_span() const { return Span(a, n, n, lda, "a"); }
  Span b_span() const { return Span(b, n, n_rhs, ldb, "b"); }
  Span x_span() const { return Span(x, n, n_rhs, ldx, "x"); }
  Span ipiv_span() const { return Span(ipiv, 1, n, n, "ipiv"); }  // empty without ipiv
};

template <class Dev, class Run>
inline void lu_solve_entry(Dev&, bool host_ptrs, const LuSolveCall& c, Run&& run) {
  const char* who = "lu_solve";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  if (!c.a) bad("a is NULL");
  if (!c.b) bad("b is NULL");
  if (host_ptrs && !c.x) bad("x is NULL");
  if (c.n_rhs < 1) bad("n_rhs must be >= 1");
  LuShape s;
  s.n = c.n, s.n_rhs = c.n_rhs;
  const LuPlan p = lu_plan(s);
  if (!p.ok) throw Error(ST_EINVAL, p.error);
  if (c.lda < c.n) bad("lda < n");
  if (c.ldb < c.n_rhs) bad("ldb < n_rhs");
  if (host_ptrs && c.ldx < c.n_rhs) bad("ldx < n_rhs");
  if (host_ptrs) {
    const Span in[2] = {c.a_span(), c.b_span()};
    const Span out[1] = {c.x_span()};
    no_overlap(who, in, 2, out, 1);
  } else {  // all three are written
    const Span out[3] = {c.a_span(), c.b_span(), c.ipiv_span()};
    no_overlap(who, nullptr, 0, out, 3);
  }
  on_backend_with<dev_has_lu<Dev>>(run, "LU kernels", "corrla_lu_solve_*");
}

// corrla_rbffit_system_* (m, ldm; no y, no coeffs) and corrla_rbffit_* (y, coeffs; the system lives in workspace)
struct RbfFitCall {
  const double* xs;
  int64_t n_s, ldxs, dim;
  const double* y;  // n_s x n_rhs, row stride ldy
  int64_t n_rhs, ldy;
  int kernel;
  double eps;
  int poly_degree;  // < 0 no tail
  double* coeffs;   // (n_s + n_poly) x n_rhs, row stride ldw: the layout corrla_rbf_apply_* reads
  int64_t ldw;
  double* m;        // (n_s + n_poly)^2, row stride ldm
  int64_t ldm;
  int64_t n_poly() const { return rbf_poly_terms(dim, poly_degree); }
  int64_t order() const { return n_s + n_poly(); }
  Span xs_span() const { return Span(xs, n_s, dim, ldxs, "xs"); }
  Span y_span() const { return Span(y, n_s, n_rhs, ldy, "y"); }
  Span coeffs_span() const { return Span(coeffs, order(), n_rhs, ldw, "coeffs"); }
  Span system_span() const { return Span(m, order(), order(), ldm, "m"); }
};

template <class Dev, class Run>
inline void rbf_fit_entry(Dev&, const RbfFitCall& c, bool fit, Run&& run) {
  const char* who = fit ? "rbf_fit" : "rbf_system";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  if (!c.xs) bad("xs is NULL");
  if (c.n_s < 1) bad("n_s must be >= 1");
  if (c.dim < 1 || c.dim > k::kRbfMaxDim) bad("dim must be in [1, 128]");
  if (c.kernel < 1 || c.kernel > 4) bad("kernel must be in [1, 4]");
  if (!std::isfinite(c.eps)) bad("eps must be finite");
  if (c.ldxs < c.dim) bad("ldxs < dim");
  if (c.n_s > k::kLuMaxN || c.order() > k::kLuMaxN) bad("n_s + n_poly must be <= 131072");
  if (fit) {
    if (!c.y) bad("y is NULL");
    if (!c.coeffs) bad("coeffs is NULL");
    if (c.n_rhs < 1 || c.n_rhs > k::kLuMaxRhs) bad("n_rhs must be in [1, 1048576]");
    if (c.ldy < c.n_rhs) bad("ldy < n_rhs");
    if (c.ldw < c.n_rhs) bad("ldw < n_rhs");
    const Span in[2] = {c.xs_span(), c.y_span()};
    const Span out[1] = {c.coeffs_span()};
    no_overlap(who, in, 2, out, 1);
  } else {
    if (!c.m) bad("m is NULL");
    if (c.ldm < c.order()) bad("ldm < n_s + n_poly");
    const Span in[1] = {c.xs_span()};
    const Span out[1] = {c.system_span()};
    no_overlap(who, in, 1, out, 1);
  }
  on_backend_with<dev_has_lu<Dev>>(run, "LU kernels", fit ? "corrla_rbffit_*" : "corrla_rbffit_system_*");
}

// ---- dense Cholesky factor and SPD solve (corrla_chol_factor_* / corrla_chol_solve_*) -------------------------------------------
// Argument checks of every entry -- the limits of n and n_rhs are the plan's (chol_plan names the argument it rejects) -- then
// `run`, on a backend that carries the kernels (dev_has_chol).  f64 only.  A solve takes the call record of the LU solve
// (LuSolveCall, without an ipiv): the same arrays with the same roles, so the same spans and the same staging.
struct CholFactorCall {
  // host entry: a is read, l is written.  Device entry: a_rw's lower triangle becomes L.
  const double* a;
  int64_t n, lda;
  double* l;
  int64_t ldl;
  double* a_rw;
  Span a_span() const { return Span(a, n, n, lda, "a"); }
  Span l_span() const { return Span(l, n, n, ldl, "l"); }
};

inline void chol_limits(int64_t n, int64_t n_rhs) {
  CholShape s;
  s.n = n, s.n_rhs = n_rhs;
  const CholPlan p = chol_plan(s);
  if (!p.ok) throw Error(ST_EINVAL, p.error);
}

template <class Dev, class Run>
inline void chol_factor_entry(Dev&, bool host_ptrs, const CholFactorCall& c, Run&& run) {
  const char* who = "chol_factor";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  if (!c.a) bad("a is NULL");
  if (host_ptrs && !c.l) bad("l is NULL");
  chol_limits(c.n, 0);
  if (c.lda < c.n) bad("lda < n");
  if (host_ptrs && c.ldl < c.n) bad("ldl < n");
  if (host_ptrs) {
    const Span in[1] = {c.a_span()};
    const Span out[1] = {c.l_span()};
    no_overlap(who, in, 1, out, 1);
  }
  on_backend_with<dev_has_chol<Dev>>(run, "Cholesky kernels", "corrla_chol_factor_*");
}

template <class Dev, class Run>
inline void chol_solve_entry(Dev&, bool host_ptrs, const LuSolveCall& c, Run&& run) {
  const char* who = "chol_solve";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  if (!c.a) bad("a is NULL");
  if (!c.b) bad("b is NULL");
  if (host_ptrs && !c.x) bad("x is NULL");
  if (c.n_rhs < 1) bad("n_rhs must be >= 1");
  chol_limits(c.n, c.n_rhs);
  if (c.lda < c.n) bad("lda < n");
  if (c.ldb < c.n_rhs) bad("ldb < n_rhs");
  if (host_ptrs && c.ldx < c.n_rhs) bad("ldx < n_rhs");
  if (host_ptrs) {
    const Span in[2] = {c.a_span(), c.b_span()};
    const Span out[1] = {c.x_span()};
    no_overlap(who, in, 2, out, 1);
  } else {  // both are written
    const Span out[2] = {c.a_span(), c.b_span()};
    no_overlap(who, nullptr, 0, out, 2);
  }
  on_backend_with<dev_has_chol<Dev>>(run, "Cholesky kernels", "corrla_chol_solve_*");
}

// ---- symmetric eigendecomposition (corrla_eigh_*) ---------------------------------------------------------------------------------
// Argument checks of both entries -- the limits of n are the plan's (eigh_plan names the argument it rejects) -- then `run`, on
// a backend that carries the kernels (dev_has_eigh).  f64 only.  a is read in both kinds of call, w and v are written.
struct EighCall {
  const double* a;
  int64_t n, lda;
  double* w;
  double* v;
  int64_t ldv;
  Span a_span() const { return Span(a, n, n, lda, "a"); }
  Span w_span() const { return Span(w, 1, n, n, "w"); }
  Span v_span() const { return Span(v, n, n, ldv, "v"); }
};

template <class Dev, class Run>
inline void eigh_entry(Dev&, const EighCall& c, Run&& run) {
  const char* who = "eigh";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  if (!c.a) bad("a is NULL");
  if (!c.w) bad("w is NULL");
  if (!c.v) bad("v is NULL");
  EighShape s;
  s.n = c.n;
  const EighPlan p = eigh_plan(s);
  if (!p.ok) throw Error(ST_EINVAL, p.error);
  if (c.lda < c.n) bad("lda < n");
  if (c.ldv < c.n) bad("ldv < n");
  const Span in[1] = {c.a_span()};
  const Span out[2] = {c.w_span(), c.v_span()};
  no_overlap(who, in, 1, out, 2);
  on_backend_with<dev_has_eigh<Dev>>(run, "symmetric eigensolver kernels", "corrla_eigh_*");
}

// ---- constrained Dirichlet sampling (corrla_dirichlet_draws_* / corrla_dirichlet_sample_*, space_samplers.rs:14-126) ---------
// Argument checks of every entry -- the limits are the plan's (dir_plan names the argument it rejects) -- then `run` with
// that plan, on a backend that carries the kernels (dev_has_dirichlet).  alphas and bounds are host arrays in both kinds of call.
struct DirichletDrawsCall {
  const double* alphas;  // d, host
  int64_t d;
  double c_scale;
  uint64_t seed;
  int64_t first, n;
  double* out;  // n x d, row stride ldo
  int64_t ldo;
  Span out_span() const { return Span(out, n, d, ldo, "out"); }
};

template <class Dev, class Run>
inline void dirichlet_draws_entry(Dev&, const DirichletDrawsCall& c, Run&& run) {
  const char* who = "dirichlet_draws";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  if (!c.alphas) bad("alphas is NULL");
  if (!c.out) bad("out is NULL");
  DirShape s;
  s.d = c.d, s.alphas = c.alphas, s.c_scale = c.c_scale, s.first = c.first, s.n = c.n;
  const DirPlan p = dir_plan(s);
  if (!p.ok) throw Error(ST_EINVAL, p.error);
  if (c.ldo < c.d) bad("ldo must be >= d");
  const Span in[2] = {Span(c.alphas, 1, c.d, c.d, "alphas"), Span()};
  const Span out[1] = {c.out_span()};
  no_overlap(who, in, 1, out, 1);
  on_backend_with<dev_has_dirichlet<Dev>>([&] { run(p); }, "Dirichlet sampling kernels", "corrla_dirichlet_draws_*");
}

struct DirichletSampleCall {
  const double* bounds;  // d x 2 row-major (lb_j, ub_j), host
  const double* alphas;  // d, host
  int64_t d;
  double c_scale;
  uint64_t seed;
  int64_t n_samples, max_zshots, chunk_size;
  double* out;  // n_samples x d, row stride ldo
  int64_t ldo;
  int64_t* n_found;  // host
  int64_t* n_drawn;  // host
  Span out_span() const { return Span(out, n_samples, d, ldo, "out"); }
};

template <class Dev, class Run>
inline void dirichlet_sample_entry(Dev&, bool host_ptrs, const DirichletSampleCall& c, Run&& run) {
  const char* who = "dirichlet_sample";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  if (!c.bounds) bad("bounds is NULL");
  if (!c.alphas) bad("alphas is NULL");
  if (!c.out) bad("out is NULL");
  if (!c.n_found) bad("n_found is NULL");
  if (!c.n_drawn) bad("n_drawn is NULL");
  if (c.n_samples < 1) bad("n_samples must be >= 1");
  DirShape s;
  s.d = c.d, s.alphas = c.alphas, s.c_scale = c.c_scale, s.bounds = c.bounds;
  s.n_samples = c.n_samples, s.max_zshots = c.max_zshots, s.chunk_size = c.chunk_size;
  const DirPlan p = dir_plan(s);
  if (!p.ok) throw Error(ST_EINVAL, p.error);
  if (c.ldo < c.d) bad("ldo must be >= d");
  const Span in[4] = {Span(c.bounds, 1, 2 * c.d, 2 * c.d, "bounds"), Span(c.alphas, 1, c.d, c.d, "alphas"),
                      Span(c.n_found, 1, 1, 1, "n_found"), Span(c.n_drawn, 1, 1, 1, "n_drawn")};
  const Span out[1] = {c.out_span()};
  if (host_ptrs) no_overlap(who, in, 4, out, 1);  // a device `out` shares no address space with the host arrays
  on_backend_with<dev_has_dirichlet<Dev>>([&] { run(p); }, "Dirichlet sampling kernels", "corrla_dirichlet_sample_*");
}

// ---- multivariate normal rows and sandwich variances (corrla_mvn_sample_* / corrla_sandwich_diag_*, stats_corr.rs:46-68) -----
// Argument checks of every entry -- the limits are the plans' (mvn_plan / sandwich_plan name the argument they reject) -- then
// `run` with that plan, on a backend that carries the kernels (dev_has_mvn).
template <class T>
struct MvnSampleCall {
  int64_t n, d, r;
  const T* factor;  // d x r, row stride ldf
  int64_t ldf;
  const T* mean;    // d, or NULL (0)
  uint64_t seed;
  int64_t first;
  int lower;
  T* out;           // n x d, row stride ldo
  int64_t ldo;
  Span factor_span() const { return Span(factor, d, r, ldf, "factor"); }
  Span mean_span() const { return Span(mean, 1, d, d, "mean"); }
  Span out_span() const { return Span(out, n, d, ldo, "out"); }
};

template <class Dev, class T, class Run>
inline void mvn_sample_entry(Dev&, const MvnSampleCall<T>& c, Run&& run) {
  const char* who = "mvn_sample";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  MvnShape s;
  s.n = c.n, s.d = c.d, s.r = c.r, s.first = c.first, s.ldo = c.ldo, s.esz = (int)sizeof(T);
  s.out_aligned = (uintptr_t)c.out % 16 == 0;
  s.lower = c.lower != 0;
  const MvnPlan p = mvn_plan(s);
  if (p.route == MvnRoute::kReject) throw Error(ST_EINVAL, p.error);
  if (!c.factor) bad("factor is NULL");
  if (c.ldf < 0) bad("negative strides are not supported");
  if (c.ldf < c.r && c.d > 1) bad("ldf must be >= r");
  if (p.route != MvnRoute::kEmpty) {  // n = 0: no array of n rows is looked at
    if (!c.out) bad("out is NULL");
    const Span in[2] = {c.factor_span(), c.mean_span()};
    const Span out[1] = {c.out_span()};
    no_overlap(who, in, 2, out, 1);
  }
  on_backend_with<dev_has_mvn<Dev>>([&] { run(p); }, "multivariate normal kernels", "corrla_mvn_sample_*");
}

template <class T>
struct SandwichDiagCall {
  const T* jac;  // m x d, row stride ldj
  int64_t m, d, ldj;
  const T* cov;  // d x d, row stride ldc
  int64_t ldc;
  T* v;          // m
  Span jac_span() const { return Span(jac, m, d, ldj, "jac"); }
  Span cov_span() const { return Span(cov, d, d, ldc, "cov"); }
  Span v_span() const { return Span(v, 1, m, m, "v"); }
};

template <class Dev, class T, class Run>
inline void sandwich_diag_entry(Dev&, const SandwichDiagCall<T>& c, Run&& run) {
  const char* who = "sandwich_diag";
  auto bad = [&](const char* what) { throw Error(ST_EINVAL, std::string(who) + ": " + what); };
  SandwichShape s;
  s.m = c.m, s.d = c.d, s.ldj = c.ldj, s.ldc = c.ldc, s.esz = (int)sizeof(T);
  const SandwichPlan p = sandwich_plan(s);
  if (!p.ok) throw Error(ST_EINVAL, p.error);
  if (!c.jac) bad("jac is NULL");
  if (!c.cov) bad("cov is NULL");
  if (!c.v) bad("v is NULL");
  const Span in[2] = {c.jac_span(), c.cov_span()};
  const Span out[1] = {c.v_span()};
  no_overlap(who, in, 2, out, 1);
  on_backend_with<dev_has_mvn<Dev>>([&] { run(p); }, "multivariate normal kernels", "corrla_sandwich_diag_*");
}

// ---- active-subspace gradient stage (corrla_grad_mat_*) -------------------------------------------------------
// the arguments of the prototype, in its order
struct GradMatCall {
  const double* x;  // n_pts x k support points, row-major
  int64_t n_pts, k;
  const double* y;  // n_pts values
  const double* xq; // n_q x k queries, row-major
  int64_t n_q;
  int est_order;
  int64_t n_nbrs;
  double out_scale;
  double* g;        // n_q x k gradients, rows ldg apart
  int64_t ldg;
  int* n_regularised;  // host, nullable
  Span x_span() const { return Span(x, n_pts, k, k, "x"); }
  Span y_span() const { return Span(y, 1, n_pts, n_pts, "y"); }
  Span xq_span() const { return Span(xq, n_q, k, k, "xq"); }
  Span g_span() const { return Span(g, n_q, k, ldg, "g"); }
};

template <class Dev, class Run>
inline void grad_entry(Dev&, const GradMatCall& c, Run&& run) {
  if (!c.x || !c.y || !c.xq || !c.g) throw Error(ST_EINVAL, "NULL argument");
  if (c.n_pts < 1 || c.n_q < 1 || c.k < 1) throw Error(ST_EINVAL, "empty point set");
  if (c.ldg < c.k) throw Error(ST_EINVAL, "ldg < k");
  run();
}

}  // namespace corrla
