// The plan of the polynomial response-surface kernels behind corrla_polyfit_gram_* and corrla_poly_eval_*
// (polyfit_kernels.hpp, polyfit_stage.hpp; linear_fit / quad_fit / quad_eval / jac_from_quad, stats_corr.rs:146-249).
//   GRAM  G = W^T W of order p + r, W = [V(z), y], V the Vandermonde matrix [z, z_a z_b (a <= b), 1] (degree 2) or [z, 1]
//         (degree 1) of the normalised samples z = (x - mu) / sigma.  V is never stored: with the augmented row
//         xt = [z_1 .. z_k, 1, y_1 .. y_r, 0] every column of W is the product of two entries of xt, and the plan's table
//         says which two.  The geometry is syrk_plan's: 128 x 128 tile pairs on and above the diagonal, the samples split
//         into slabs, per-slab partial tiles in workspace, one finishing launch that adds them in index order.
//   EVAL  V(x) c = xt^T C xt with xt = [x_1 .. x_k, 1] and C the symmetric (k + 1)^2 matrix of the coefficients; the
//         gradient is 2 (C xt)[:k].  A workgroup keeps a tile of rows in LDS and walks C in blocks of columns.
// Limits: 1 <= k <= 128, degree 1 or 2, 0 <= r <= 64, m >= 1.
// Host code only, no HIP call: tests/test_polyfit_plan.py compiles this header with the host compiler and pins the plan.
// The kernels take the tile sizes and the pair enumeration from it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "core_svd_plan.hpp"  // kLdsMaxBytes, CORRLA_HD
#include "syrk_plan.hpp"      // syrk_pair: the enumeration of the tile pairs

namespace corrla {
namespace k {

constexpr int kPolyMaxK = 128;     // features
constexpr int kPolyMaxRhs = 64;    // right-hand sides
constexpr int kPolyBT = 128;       // columns of W per tile: a workgroup owns one 128 x 128 tile of G
constexpr int kPolyKT = 32;        // samples per staged chunk: 8 reduction steps of an MFMA
constexpr int kPolyThreads = 256;  // four MFMA waves, each 64 x 64 of the tile; every wave stages as well
// entries of the augmented row: the features, the one, the right-hand sides and a zero (what the columns of a ragged last
// tile multiply)
CORRLA_HD constexpr int poly_aug_width(int kf, int r) { return kf + 1 + r + 1; }
// its row stride in LDS, odd: the four reduction rows of an MFMA step start in different banks
CORRLA_HD constexpr int poly_aug_ld(int kf, int r) { return poly_aug_width(kf, r) | 1; }
// GRAM: one chunk of augmented rows in f64, and the means and scales; 49.9 KiB + 2 KiB at k = 128, r = 64
CORRLA_HD constexpr int poly_gram_lds_bytes(int kf, int r) { return (kPolyKT * poly_aug_ld(kf, r) + 2 * kf) * 8; }

// EVAL: 64 rows per workgroup (one 16-row MFMA tile per wave), C in blocks of 32 columns
constexpr int kPolyEvalBM = 64;
constexpr int kPolyEvalCB = 32;        // columns of C per LDS image: two 16-wide MFMA column tiles
constexpr int kPolyEvalCLd = kPolyEvalCB + 8;  // its row stride: the four reduction rows 8 slots apart
// row stride of the staged rows: k + 1 rounded up to 8, plus 4 -- 4 mod 8, so that 16 rows x 4 reduction slots of one
// fragment read spread over all banks
CORRLA_HD constexpr int poly_eval_xld(int kf) { return (kf + 1 + 7) / 8 * 8 + 4; }
CORRLA_HD constexpr int poly_eval_k4(int kf) { return (kf + 1 + 3) / 4 * 4; }  // reduction length, whole MFMA steps
// the row tile and one block of C; 70 KiB + 41.25 KiB at k = 128
CORRLA_HD constexpr int poly_eval_lds_bytes(int kf) { return (kPolyEvalBM * poly_eval_xld(kf) + poly_eval_k4(kf) * kPolyEvalCLd) * 8; }
// what the plan allows for C beside the row tile: one block
CORRLA_HD constexpr int poly_eval_c_block_bytes(int kf) { return poly_eval_k4(kf) * kPolyEvalCLd * 8; }

}  // namespace k

// columns of V: [x, 1] for degree 1, [x, x_a x_b (a <= b), 1] for degree 2 (build_vandermonde, stats_corr.rs:201-209)
CORRLA_HD constexpr int64_t poly_terms(int64_t kf, int degree) { return degree < 2 ? kf + 1 : kf + kf * (kf + 1) / 2 + 1; }

enum class PolyRoute : int {
  kReject = 0,
  kInPlace = 1,         // x read where it lies, 16-byte loads
  kInPlaceChecked = 2   // x read where it lies, element loads (base or leading dimension not 16-byte aligned)
};

// Knobs, read once when a device context is created (hip_backend.hpp).
struct PolyKnobs {
  int64_t slab_rows = 0;  // CORRLA_POLYFIT_SLAB_ROWS: samples per slab (rounded up to the chunk; 0: by shape)
};

struct PolyGramShape {
  int64_t m = 0, kf = 0, r = 0;
  int64_t ldx = 0, ldy = 0;
  int degree = 2;
  int esz = 8;               // of x and y; G, the means and the scales are f64
  bool x_aligned = true;     // the base pointers are 16-byte aligned
  bool y_aligned = true;     // (y is the narrow operand: its loads follow its own alignment, the route is x's)
  int num_cus = 256;
};

struct PolyGramPlan {
  PolyRoute route = PolyRoute::kReject;
  const char* error = nullptr;
  int bt = k::kPolyBT, kt = k::kPolyKT;
  int64_t p = 0;           // columns of V
  int64_t order = 0;       // p + r, the order of G
  bool y_vec = false;      // y may be read with 16-byte loads
  int aug = 0, aug_ld = 0; // entries of the augmented row, its LDS stride
  int nb = 0;              // column tiles; tile b covers the columns [b bt, min(order, (b + 1) bt))
  int64_t npairs = 0;      // nb (nb + 1) / 2, enumerated by syrk_pair
  int64_t chunks = 0;      // chunks of kt samples over [0, m)
  int64_t nsplit = 1;      // slabs
  int64_t slab_rows = 0;   // a multiple of kt; slab s covers [s slab_rows, min(m, (s + 1) slab_rows)), none empty
  unsigned grid_x = 0, grid_y = 0, block = k::kPolyThreads;  // (pair, slab)
  size_t lds_bytes = 0;
  size_t table_bytes = 0;  // nb * bt packed pairs
  size_t ws_bytes = 0;     // nsplit * npairs partial tiles of bt * bt doubles
  size_t ws_bound = 0;     // the stated upper bound of ws_bytes for this shape
  unsigned finish_grid_x = 0, finish_grid_y = 0, finish_block = 256;  // (pair, 32 x 32 sub-tile)
};

// Column c of W as the two entries of the augmented row it multiplies, packed a | b << 16, in the reference's column
// order (mat_col_interactions and build_vandermonde, stats_corr.rs:112-142, 201-209): the features (a, one), the
// interactions a-major (a, b >= a), the intercept (one, one), the right-hand sides (k + 1 + j, one); padded with
// (zero, zero) to whole tiles.
inline std::vector<int32_t> poly_pair_table(int64_t kf, int64_t r, int degree) {
  const int32_t one = (int32_t)kf, zero = (int32_t)(kf + 1 + r);
  std::vector<int32_t> t;
  auto put = [&](int32_t a, int32_t b) { t.push_back(a | (b << 16)); };
  for (int32_t a = 0; a < kf; ++a) put(a, one);
  if (degree >= 2)
    for (int32_t a = 0; a < kf; ++a)
      for (int32_t b = a; b < kf; ++b) put(a, b);
  put(one, one);
  for (int32_t j = 0; j < r; ++j) put((int32_t)kf + 1 + j, one);
  while (t.size() % k::kPolyBT) put(zero, zero);
  return t;
}

// Upper bound of the partial-tile workspace, as syrk_ws_bound: the pairs alone once, or, where the samples are split to
// fill the chip, at most 4 * num_cus + npairs tiles.
inline size_t poly_ws_bound(int64_t npairs, int num_cus) {
  return (size_t)(npairs + 4 * (int64_t)num_cus) * k::kPolyBT * k::kPolyBT * sizeof(double);
}

inline PolyGramPlan poly_gram_plan(const PolyGramShape& s, const PolyKnobs& kn) {
  PolyGramPlan p;
  auto reject = [&](const char* why) {
    p.route = PolyRoute::kReject;
    p.error = why;
    return p;
  };
  if (s.esz != 4 && s.esz != 8) return reject("polyfit: element size (esz) must be 4 or 8");
  if (s.m < 1) return reject("polyfit: m must be >= 1");
  if (s.kf < 1 || s.kf > k::kPolyMaxK) return reject("polyfit: k must be in [1, 128]");
  if (s.degree != 1 && s.degree != 2) return reject("polyfit: degree must be 1 or 2");
  if (s.r < 0 || s.r > k::kPolyMaxRhs) return reject("polyfit: r must be in [0, 64]");
  if (s.ldx < s.kf) return reject("polyfit: ldx < k");
  if (s.r > 0 && s.ldy < s.r) return reject("polyfit: ldy < r");
  const int64_t vec = 16 / s.esz;
  p.route = (s.x_aligned && s.ldx % vec == 0) ? PolyRoute::kInPlace : PolyRoute::kInPlaceChecked;
  p.y_vec = s.r > 0 && s.y_aligned && s.ldy % vec == 0;
  p.p = poly_terms(s.kf, s.degree);
  p.order = p.p + s.r;
  p.aug = k::poly_aug_width((int)s.kf, (int)s.r);
  p.aug_ld = k::poly_aug_ld((int)s.kf, (int)s.r);
  p.nb = (int)((p.order + p.bt - 1) / p.bt);
  p.npairs = (int64_t)p.nb * (p.nb + 1) / 2;
  // sample split, the policy of syrk_plan: the pairs alone fill the chip when there are a few waves of them; else the
  // slabs carry the parallelism
  p.chunks = (s.m + p.kt - 1) / p.kt;
  int64_t cps;  // chunks per slab
  if (kn.slab_rows > 0) {
    cps = (kn.slab_rows + p.kt - 1) / p.kt;
  } else if (p.npairs >= 2 * (int64_t)s.num_cus) {
    cps = p.chunks;
  } else {
    const int64_t want = (4 * (int64_t)s.num_cus + p.npairs - 1) / p.npairs;  // slabs that give ~4 workgroups per CU
    cps = std::max<int64_t>((p.chunks + want - 1) / want, 8);                 // ... of at least 8 chunks each
  }
  cps = std::max<int64_t>(1, std::min(cps, p.chunks));
  p.nsplit = (p.chunks + cps - 1) / cps;
  if (p.nsplit > 65535) {
    cps = (p.chunks + 65534) / 65535;
    p.nsplit = (p.chunks + cps - 1) / cps;
  }
  p.slab_rows = cps * p.kt;
  p.grid_x = (unsigned)p.npairs;
  p.grid_y = (unsigned)p.nsplit;
  p.lds_bytes = (size_t)k::poly_gram_lds_bytes((int)s.kf, (int)s.r);
  p.table_bytes = (size_t)p.nb * p.bt * sizeof(int32_t);
  p.ws_bytes = (size_t)p.nsplit * (size_t)p.npairs * p.bt * p.bt * sizeof(double);
  p.ws_bound = kn.slab_rows > 0 ? p.ws_bytes : poly_ws_bound(p.npairs, s.num_cus);
  p.finish_grid_x = (unsigned)p.npairs;
  p.finish_grid_y = (unsigned)((p.bt / 32) * (p.bt / 32));
  return p;
}

struct PolyEvalPlan {
  bool ok = false;
  const char* error = nullptr;
  PolyRoute route = PolyRoute::kReject;
  int bm = k::kPolyEvalBM, cb = k::kPolyEvalCB;
  int64_t p = 0;        // rows of the coefficients
  int k1 = 0;           // k + 1, the order of C
  int k4 = 0;           // the reduction length: k1 rounded up to whole MFMA steps
  int xld = 0;          // row stride of the staged rows
  int ncb = 0;          // blocks of cb columns of C; more than one when C exceeds one LDS image
  int64_t ntiles = 0;   // row tiles; tile t covers the rows [t bm, min(m, (t + 1) bm))
  unsigned grid_x = 0, block = k::kPolyThreads;
  size_t lds_bytes = 0;
  size_t c_bytes = 0;   // workspace: r images of C, k4 rows x ncb cb columns, zero padded
  unsigned assemble_grid_x = 0;
};

inline PolyEvalPlan poly_eval_plan(int64_t m, int64_t kf, int64_t r, int degree, int64_t ldx, int esz, bool x_aligned) {
  PolyEvalPlan p;
  auto reject = [&](const char* why) {
    p.ok = false;
    p.error = why;
    return p;
  };
  if (esz != 4 && esz != 8) return reject("poly_eval: element size (esz) must be 4 or 8");
  if (m < 1) return reject("poly_eval: m must be >= 1");
  if (kf < 1 || kf > k::kPolyMaxK) return reject("poly_eval: k must be in [1, 128]");
  if (degree != 1 && degree != 2) return reject("poly_eval: degree must be 1 or 2");
  if (r < 1 || r > k::kPolyMaxRhs) return reject("poly_eval: r must be in [1, 64]");
  if (ldx < kf) return reject("poly_eval: ldx < k");
  p.route = (x_aligned && ldx % (16 / esz) == 0) ? PolyRoute::kInPlace : PolyRoute::kInPlaceChecked;
  p.p = poly_terms(kf, degree);
  p.k1 = (int)kf + 1;
  p.k4 = k::poly_eval_k4((int)kf);
  p.xld = k::poly_eval_xld((int)kf);
  p.ncb = (p.k1 + p.cb - 1) / p.cb;
  p.ntiles = (m + p.bm - 1) / p.bm;
  if (p.ntiles > 0x7fffffff) return reject("poly_eval: m gives more than 2^31 - 1 row tiles");
  p.grid_x = (unsigned)p.ntiles;
  p.lds_bytes = (size_t)k::poly_eval_lds_bytes((int)kf);
  p.c_bytes = (size_t)r * (size_t)p.k4 * (size_t)(p.ncb * p.cb) * sizeof(double);
  p.assemble_grid_x = (unsigned)((r * (int64_t)p.k4 * (p.ncb * p.cb) + 255) / 256);
  p.ok = true;
  return p;
}

}  // namespace corrla
