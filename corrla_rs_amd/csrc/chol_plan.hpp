// The plan of the dense Cholesky factorisation and SPD solve behind corrla_chol_factor_* and corrla_chol_solve_*
// (chol_kernels.hpp, chol_stage.hpp): A = L L^T, f64 only.  A is ROW-major (n x n, row stride lda); only its LOWER triangle
// (i >= j) is read and written -- the strict upper triangle is never touched.  B and X are n x n_rhs row-major.
//   SMALL    n <= kCholSmallN: one workgroup factors the triangle in LDS (one launch) and writes the status record.
//   BLOCKED  right-looking, panels of kCholNB columns.  Per panel three launches -- the diagonal block (one workgroup factors
//            the kCholNB x kCholNB block in LDS and leaves the panel's record), the panel solve L21 = A21 L11^-T (one workgroup
//            per chunk of kCholChunk rows below the block) and the trailing update A22 -= L21 L21^T over the tiles of the lower
//            triangle alone (workgroup p owns the tile pair chol_tile_pair(p), bi >= bj) -- of which the last panel has only
//            the first.  Then one launch that reduces the panel records to the status record.
//            So 3 npanels - 2 + 1 launches, where the LU plan needs 2 n + 3 npanels.
//   SOLVE    per block row of kCholNB a diagonal-block solve and a tall update (the last block of each sweep has no update),
//            forward with L and backward with L^T; any n_rhs.
// Host code only, no HIP call: tests/test_chol_plan.py compiles this header with the host compiler and pins the plan.  The
// kernels take the tile sizes and the tile map from it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "core_svd_plan.hpp"  // kLdsMaxBytes, CORRLA_HD

namespace corrla {
namespace k {

constexpr int kCholNB = 64;     // panel width = the K of every update: one LDS stage of both operands
constexpr int kCholTile = 64;   // rows and columns of an update tile: four waves x 16 rows, four 16-wide MFMA column tiles
constexpr int kCholChunk = 64;  // rows per workgroup of the panel solve: one lane per row
constexpr int kCholThreads = 256;
// SMALL: the triangle in an n x n image with a row stride of kCholSmallN + 1 (columns are walked: an odd stride keeps them
// on distinct banks) plus the scratch of the reductions.
constexpr int kCholSmallN = 128;
constexpr int kCholSmallLd = kCholSmallN + 1;
constexpr size_t kCholSmallLdsBytes = ((size_t)kCholSmallN * kCholSmallLd + 2 * kCholThreads) * 8;
// Operand images of the updates.  ds_read_b64 banks are (byte / 4) mod 64 per 32-lane half; a half holds 16 rows (or columns)
// x 2 consecutive k.  [row][k] image: a row stride of 66 doubles = 132 dwords = 4 mod 64 puts lane (r, kq) on dwords 4 r + 2 kq:
// all distinct.  [k][col] image: a row stride of 80 doubles = 160 dwords = 32 mod 64 puts lane (c, kq) on dwords 2 c + 32 kq.
constexpr int kCholRowLd = kCholNB + 2;
constexpr int kCholColLd = kCholTile + 16;
// trailing update: two row chunks of L21 as [row][k] images
constexpr size_t kCholUpdateLdsBytes = (size_t)2 * kCholTile * kCholRowLd * 8;
// tall updates of the solve: L as [row][k] (forward) or [k][row] (backward: L^T), X as [k][col]; sized for the larger
constexpr size_t kCholGemmLdsBytes = (size_t)2 * kCholNB * kCholColLd * 8;
// the diagonal block: [kCholNB][kCholNB + 1] plus the reduction scratch; static LDS
constexpr int kCholDiagLd = kCholNB + 1;
constexpr size_t kCholDiagLdsBytes = ((size_t)kCholNB * kCholDiagLd + 2 * kCholThreads) * 8;
// the panel solve: the triangular block [kCholNB][kCholNB] and the rows of A21 [kCholChunk][kCholNB + 1] (a lane walks a row:
// the odd stride keeps the lanes on distinct banks)
constexpr size_t kCholPanelLdsBytes = ((size_t)kCholNB * kCholNB + (size_t)kCholChunk * (kCholNB + 1)) * 8;
// the diagonal solves: the triangular block and the tile of X [kCholNB][kCholTile]; static LDS
constexpr size_t kCholTriLdsBytes = ((size_t)kCholNB * kCholNB + (size_t)kCholNB * kCholTile) * 8;
static_assert(kCholSmallLdsBytes <= kLdsMaxBytes && kCholUpdateLdsBytes <= kLdsMaxBytes && kCholGemmLdsBytes <= kLdsMaxBytes &&
                  kCholPanelLdsBytes <= kLdsMaxBytes,
              "LDS images fit");
static_assert(kCholDiagLdsBytes <= 65536 && kCholTriLdsBytes <= 65536, "static LDS images fit");
static_assert((size_t)kCholTile * kCholRowLd + (size_t)kCholNB * kCholColLd <= 2 * (size_t)kCholNB * kCholColLd, "forward images fit the gemm stage");
// The limits, as for LU.  n <= 2^17: the largest grid, the nt (nt + 1) / 2 < 2^21 tile pairs of the first trailing update
// (nt = n / kCholTile <= 2^11), stays inside 2^31 - 1; so do the (n / kCholTile) x (n_rhs / kCholTile) <= 2^25 tiles of a solve.
constexpr int64_t kCholMaxN = (int64_t)1 << 17;
constexpr int64_t kCholMaxRhs = (int64_t)1 << 20;

}  // namespace k

enum class CholRoute : int { kNone = 0, kSmall = 1, kBlocked = 2 };

struct CholShape {
  int64_t n = 0, n_rhs = 0;  // n_rhs == 0: factor only
};

// what the device leaves for the one read-back of a call (chol_kernels.hpp fills it)
struct CholFactorStatus {
  int64_t info;      // 0, or the 1-based column whose pivot a_jj - sum_k l_jk^2 was <= 0 or not finite (the first such)
  double min_diag;   // smallest and largest l_jj of the columns factored (before the failed one)
  double max_diag;
  double logdet;     // 2 sum_j log l_jj, summed in a fixed order; 0 when info != 0
};

// what the diagonal-block launch of panel p leaves for the finish launch: the same fields over the panel's columns, with
// logdet holding sum_j log l_jj of the panel (not doubled)
typedef CholFactorStatus CholPanelRecord;

struct CholPlan {
  bool ok = false;
  const char* error = nullptr;
  CholRoute route = CholRoute::kNone;
  int nb = k::kCholNB;
  int64_t npanels = 0;    // BLOCKED: panel p covers the columns [p nb, min(n, (p + 1) nb))
  int64_t nblocks = 0;    // SOLVE: block rows of nb
  int64_t rhs_tiles = 0;  // column tiles of B
  int64_t factor_launches = 0, solve_launches = 0;
  size_t lds_small = k::kCholSmallLdsBytes, lds_update = k::kCholUpdateLdsBytes, lds_gemm = k::kCholGemmLdsBytes;
  size_t lds_diag = k::kCholDiagLdsBytes, lds_panel = k::kCholPanelLdsBytes, lds_tri = k::kCholTriLdsBytes;
  // workspace: the status record and the panel records; each piece rounded up to 256 bytes
  size_t ws_status = 256, ws_panels = 0;
  size_t ws_bytes = 0;
  size_t ws_bound = 0;  // the stated upper bound of ws_bytes: n / 2 + 1024
};

CORRLA_HD constexpr int64_t chol_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// panel [j0, j1): the row chunks of the panel solve and the row / column tiles of the trailing update both cut [j1, n)
CORRLA_HD constexpr int64_t chol_chunks(int64_t n, int64_t j1) { return chol_ceil_div(n - j1, k::kCholChunk); }
CORRLA_HD constexpr int64_t chol_trail_tiles(int64_t n, int64_t j1) { return chol_ceil_div(n - j1, k::kCholTile); }
// piece i of width w of [base, n)
CORRLA_HD constexpr int64_t chol_piece_begin(int64_t base, int64_t i, int64_t w) { return base + i * w; }
CORRLA_HD constexpr int64_t chol_piece_end(int64_t base, int64_t i, int64_t w, int64_t n) { return base + (i + 1) * w < n ? base + (i + 1) * w : n; }
// the tile pairs of a trailing update over nt row tiles: the lower triangle, row by row
CORRLA_HD constexpr int64_t chol_tile_pairs(int64_t nt) { return nt * (nt + 1) / 2; }
// Pair p: p = bi (bi + 1) / 2 + bj with bi >= bj.  Neighbouring workgroups share the row chunk bi.  The square root gives bi
// to within one; the two corrections run at most twice each (p < 2^22: 8 p + 1 is exact in double).
CORRLA_HD inline void chol_tile_pair(int64_t p, int64_t* bi, int64_t* bj) {
  int64_t i = (int64_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
  if (i < 0) i = 0;
  while (i > 0 && i * (i + 1) / 2 > p) --i;
  while ((i + 1) * (i + 2) / 2 <= p) ++i;
  *bi = i;
  *bj = p - i * (i + 1) / 2;
}
inline size_t chol_round256(size_t b) { return (b + 255) / 256 * 256; }
inline size_t chol_ws_bound(int64_t n) { return (size_t)n / 2 + 1024; }

inline CholPlan chol_plan(const CholShape& s) {
  CholPlan p;
  auto reject = [&](const char* why) {
    p.ok = false;
    p.error = why;
    return p;
  };
  if (s.n < 1) return reject("chol: n must be >= 1");
  if (s.n > k::kCholMaxN) return reject("chol: n must be <= 131072");
  if (s.n_rhs < 0) return reject("chol: n_rhs must be >= 0");
  if (s.n_rhs > k::kCholMaxRhs) return reject("chol: n_rhs must be <= 1048576");
  p.route = s.n <= k::kCholSmallN ? CholRoute::kSmall : CholRoute::kBlocked;
  p.npanels = chol_ceil_div(s.n, p.nb);
  p.nblocks = p.npanels;
  p.rhs_tiles = chol_ceil_div(s.n_rhs, k::kCholTile);
  // 3 per panel but 1 for the last, 1 to reduce the panel records
  p.factor_launches = p.route == CholRoute::kSmall ? 1 : 3 * p.npanels - 2 + 1;
  // a diagonal solve per block and an update per block but the last, in both sweeps
  p.solve_launches = s.n_rhs == 0 ? 0 : 2 * (2 * p.nblocks - 1);
  p.ws_panels = chol_round256((size_t)p.npanels * sizeof(CholPanelRecord));
  p.ws_bytes = p.ws_status + p.ws_panels;
  p.ws_bound = chol_ws_bound(s.n);
  p.ok = true;
  return p;
}

}  // namespace corrla
