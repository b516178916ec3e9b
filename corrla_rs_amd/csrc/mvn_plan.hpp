// The plans of the multivariate-normal sampler behind corrla_mvn_sample_* (sample_mv_normal, stats_corr.rs:46-58) and of the
// sandwich variances behind corrla_sandwich_diag_* (sandwich_prop, stats_corr.rs:64-68); kernels in mvn_kernels.hpp,
// launchers in mvn_stage.hpp.  Both are the product of a row tile, held whole in LDS, with a small matrix that is read in
// chunks: the n x r normals z against F^T (r x d), the m x d gradients J against C (d x d).
// A workgroup owns BM rows and every column.  Its four waves stand as (BM / 16) x (64 / BM), each on 16 rows x 64 columns,
// so one pass covers BN = 64 * 64 / BM columns; the reduction is walked in chunks of KC indices of the small matrix
// (KC x BN elements of staging).  The LDS of a workgroup is therefore (round_up(r, 4) * BM + KC * BN) * esz, and the tiles
// follow from kLdsMaxBytes alone: BM = 64 while two workgroups of that size fit a compute unit, BM = 32 while one fits.
//   The sampler is fused on the 64-row tile only, r <= 288 (f32) / 144 (f64); any larger r takes the staged route
//   (fill_normal_kernel into a bounded workspace, then pca_back_kernel in STORE mode, a row chunk at a time).  The 32-row
//   tile would hold r up to 1152 / 576, but measured against the unfused route it loses (f64, r = d = 256, 10^6 rows:
//   8.53 ms against 6.31 ms), so that class is sent to the staged route, which is the unfused route.
//   The sandwich has no second route: its limit d <= 512 needs the 32-row tile beyond d = 288 / 144.
// Host code only, no HIP call: tests/test_mvn_plan.py compiles this header with the host compiler and pins the plans.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "core_svd_plan.hpp"   // kLdsMaxBytes, CORRLA_HD
#include "pca_apply_plan.hpp"  // the staged route's multiply

namespace corrla {
namespace k {

constexpr int kMvnThreads = 256;  // four MFMA waves; every wave generates and stages as well
constexpr int kMvnBmWide = 64, kMvnBmNarrow = 32;
CORRLA_HD constexpr int mvn_bn(int bm) { return 64 * (64 / bm); }
CORRLA_HD constexpr int mvn_kc(int esz) { return 128 / esz; }
CORRLA_HD constexpr int64_t mvn_pad4(int64_t r) { return (r + 3) / 4 * 4; }
CORRLA_HD constexpr size_t mvn_lds_bytes(int64_t r, int bm, int esz) {
  return ((size_t)mvn_pad4(r) * (size_t)bm + (size_t)mvn_kc(esz) * (size_t)mvn_bn(bm)) * (size_t)esz;
}
// the row tile: 64 while two workgroups fit a compute unit, 32 while one fits, 0: none fits
CORRLA_HD constexpr int mvn_bm(int64_t r, int esz) {
  return mvn_lds_bytes(r, kMvnBmWide, esz) <= kLdsMaxBytes / 2 ? kMvnBmWide
         : mvn_lds_bytes(r, kMvnBmNarrow, esz) <= kLdsMaxBytes ? kMvnBmNarrow
                                                               : 0;
}
// the largest reduction length of the fused sampler: two workgroups of the 64-row tile per compute unit -- 288 (f32), 144 (f64)
CORRLA_HD constexpr int64_t mvn_max_fused_r(int esz) {
  return (int64_t)((kLdsMaxBytes / 2 - (size_t)mvn_kc(esz) * mvn_bn(kMvnBmWide) * esz) / ((size_t)kMvnBmWide * esz)) / 4 * 4;
}

}  // namespace k

constexpr int64_t kMvnMaxD = 65536;                            // the staged route's limit
constexpr size_t kMvnStagedWsBytes = (size_t)256 << 20;        // the z workspace of the staged route, not more than this
constexpr int64_t kSandwichMaxD = 512;

enum class MvnRoute : int { kReject = 0, kFused = 1, kStaged = 2, kEmpty = 3 };

struct MvnShape {
  int64_t n = 0, d = 0, r = 0;  // rows, features, columns of the factor
  int64_t first = 0;            // stream row of the first output row
  int64_t ldo = 0;              // row stride of out, in elements
  int esz = 4;
  bool out_aligned = true;      // the base of out is 16-byte aligned
  bool lower = false;           // the factor is square lower-triangular
};

struct MvnPlan {
  MvnRoute route = MvnRoute::kReject;
  const char* error = nullptr;
  int bm = 0, bn = 0, kc = 0;
  unsigned grid_x = 0, block = k::kMvnThreads;  // fused: workgroup w owns the rows [w bm, min(n, (w + 1) bm))
  int64_t ncoltiles = 0;                        // fused: passes over the columns, bn apart
  size_t lds_bytes = 0;
  int wide = 0;               // 16-byte stores of out are legal
  int64_t ldft = 0;           // row stride of the repacked factor F^T (r rows of d features)
  size_t factor_bytes = 0;    // ... and its size
  int64_t chunk_rows = 0;     // staged: rows per fill + multiply
  int64_t nchunks = 0;
  size_t ws_bytes = 0;        // staged: the z workspace, chunk_rows x r column-major
  size_t ws_bound = 0;        // its stated upper bound
};

// Upper bound of the staged route's workspace: the budget, or one 64-row tile of the widest factor where that is more.
inline size_t mvn_ws_bound(int64_t r, int esz) {
  return std::max(kMvnStagedWsBytes, (size_t)k::kPcaBackBM * (size_t)r * (size_t)esz);
}

inline MvnPlan mvn_plan(const MvnShape& s) {
  MvnPlan p;
  auto reject = [&](const char* why) {
    p.route = MvnRoute::kReject;
    p.error = why;
    return p;
  };
  if (s.esz != 4 && s.esz != 8) return reject("mvn_sample: element size must be 4 or 8");
  if (s.n < 0) return reject("mvn_sample: n must be >= 0");
  if (s.d < 1) return reject("mvn_sample: d must be >= 1");
  if (s.r < 1) return reject("mvn_sample: the factor needs r >= 1 columns");
  if (s.r > s.d) return reject("mvn_sample: the factor has more columns than rows (r > d)");
  if (s.lower && s.r != s.d) return reject("mvn_sample: a lower-triangular factor is square");
  if (s.first < 0) return reject("mvn_sample: first must be >= 0");
  if (s.ldo < 0) return reject("mvn_sample: negative strides are not supported");
  if (s.ldo < s.d && s.n > 1) return reject("mvn_sample: the row stride of out must be >= d");
  // the last counter (first + n) r - 1 and every intermediate stay below 2^63
  if (s.n > INT64_MAX - s.first || (s.first + s.n) > INT64_MAX / s.r) return reject("mvn_sample: (first + n) * r does not fit 63 bits");
  p.kc = k::mvn_kc(s.esz);
  p.ldft = (s.d + 63) / 64 * 64;
  p.factor_bytes = (size_t)s.r * (size_t)p.ldft * (size_t)s.esz;
  if (s.n == 0) {
    p.route = MvnRoute::kEmpty;
    return p;
  }
  const int64_t vec = 16 / s.esz;
  const int64_t ld = s.n == 1 ? std::max(s.ldo, s.d) : s.ldo;
  p.wide = (s.out_aligned && ld % vec == 0) ? 1 : 0;
  if (s.r <= k::mvn_max_fused_r(s.esz)) {
    p.route = MvnRoute::kFused;
    p.bm = k::kMvnBmWide;
    p.bn = k::mvn_bn(p.bm);
    const int64_t nbm = (s.n + p.bm - 1) / p.bm;
    if (nbm > 0x7fffffff) return reject("mvn_sample: more than 2^31 - 1 row tiles");
    p.grid_x = (unsigned)nbm;
    p.ncoltiles = (s.d + p.bn - 1) / p.bn;
    p.lds_bytes = k::mvn_lds_bytes(s.r, p.bm, s.esz);
    return p;
  }
  if (s.d > kMvnMaxD) return reject("mvn_sample: d must be <= 65536 beyond the fused route");
  p.route = MvnRoute::kStaged;
  p.bm = k::kPcaBackBM, p.bn = k::kPcaBackBN;
  const int64_t fit = (int64_t)(kMvnStagedWsBytes / ((size_t)s.r * (size_t)s.esz)) / p.bm * p.bm;
  p.chunk_rows = std::min(s.n, std::max<int64_t>(fit, p.bm));
  p.nchunks = (s.n + p.chunk_rows - 1) / p.chunk_rows;
  p.ws_bytes = (size_t)p.chunk_rows * (size_t)s.r * (size_t)s.esz;
  p.ws_bound = mvn_ws_bound(s.r, s.esz);
  p.lds_bytes = (size_t)k::pca_back_lds_bytes(s.esz);
  return p;
}

struct SandwichShape {
  int64_t m = 0, d = 0;
  int64_t ldj = 0, ldc = 0;  // row strides of jac and cov
  int esz = 4;
};

struct SandwichPlan {
  bool ok = false;
  const char* error = nullptr;
  int bm = 0, bn = 0, kc = 0;
  unsigned grid_x = 0, block = k::kMvnThreads;
  int64_t ncoltiles = 0;
  size_t lds_bytes = 0;
};

inline SandwichPlan sandwich_plan(const SandwichShape& s) {
  SandwichPlan p;
  auto reject = [&](const char* why) {
    p.ok = false;
    p.error = why;
    return p;
  };
  if (s.esz != 4 && s.esz != 8) return reject("sandwich_diag: element size must be 4 or 8");
  if (s.m < 1) return reject("sandwich_diag: jac must have at least one row");
  if (s.d < 1) return reject("sandwich_diag: d must be >= 1");
  if (s.d > kSandwichMaxD) return reject("sandwich_diag: d must be <= 512");
  if (s.ldj < 0 || s.ldc < 0) return reject("sandwich_diag: negative strides are not supported");
  if ((s.ldj < s.d && s.m > 1) || (s.ldc < s.d && s.d > 1)) return reject("sandwich_diag: a row stride is below d");
  p.bm = k::mvn_bm(s.d, s.esz);
  static_assert(k::mvn_bm(kSandwichMaxD, 8) == k::kMvnBmNarrow && k::mvn_bm(kSandwichMaxD, 4) != 0, "the widest jac tile fits in LDS");
  p.bn = k::mvn_bn(p.bm);
  p.kc = k::mvn_kc(s.esz);
  const int64_t nbm = (s.m + p.bm - 1) / p.bm;
  if (nbm > 0x7fffffff) return reject("sandwich_diag: more than 2^31 - 1 row tiles");
  p.grid_x = (unsigned)nbm;
  p.ncoltiles = (s.d + p.bn - 1) / p.bn;
  p.lds_bytes = k::mvn_lds_bytes(s.d, p.bm, s.esz);
  p.ok = true;
  return p;
}

}  // namespace corrla
