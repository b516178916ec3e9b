// The plan of the dense LU factorisation and solve behind corrla_lu_solve_* and corrla_rbffit_* (lu_kernels.hpp,
// lu_stage.hpp): P A = L U with partial pivoting, LAPACK getrf semantics (unit lower L and upper U over A, ipiv), f64 only.
// A is ROW-major (n x n, row stride lda); B and X are n x n_rhs row-major.
//   SMALL    n <= kLuSmallN: one workgroup factors the whole matrix in LDS (one launch).
//   BLOCKED  right-looking, panels of kLuNB columns.  Per column two launches -- the pivot kernel (one workgroup: finishes
//            the search, writes ipiv[j], swaps the two panel rows, checks the pivot) and the panel update (one workgroup per
//            chunk of kLuChunk rows of [j, n): scales column j, applies the rank-1 update to the panel columns to its right,
//            leaves the partial maxima of column j + 1).  Per panel three launches -- the row interchanges of the columns
//            left and right of the panel, the triangular solve U12 = L11^-1 A12 (one tile of kLuTile columns per workgroup)
//            and the trailing update A22 -= L21 U12 (one kLuTile x kLuTile tile per workgroup, K = kLuNB) -- of which the last
//            panel has only the first.  Then two launches that reduce max |u_ij|.
//   SOLVE    one launch that applies ipiv to B, then per block row of kLuNB a diagonal-block solve and a tall update
//            (the last block of each sweep has no update), forward with L and backward with U.
// Host code only, no HIP call: tests/test_lu_plan.py compiles this header with the host compiler and pins the plan.  The
// kernels take the tile sizes from it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "core_svd_plan.hpp"  // kLdsMaxBytes, CORRLA_HD

namespace corrla {
namespace k {

constexpr int kLuNB = 64;      // panel width = the K of the trailing update: one LDS stage of both operands
constexpr int kLuTile = 64;    // rows and columns of an update tile: four waves x 16 rows, four 16-wide MFMA column tiles
constexpr int kLuChunk = 64;   // rows of [j, n) per workgroup of the panel update
constexpr int kLuThreads = 256;
// SMALL: the n x n image with a row stride of kLuSmallN + 1 (columns are walked: an odd stride keeps them on distinct banks)
// plus the reduction scratch of the pivot search.  160 KiB hold the padded image up to n = 142; 128 is the largest multiple
// of the panel width below that.
constexpr int kLuSmallN = 128;
constexpr int kLuSmallLd = kLuSmallN + 1;
constexpr size_t kLuSmallLdsBytes = ((size_t)kLuSmallN * kLuSmallLd + 2 * kLuThreads) * 8;
// the update tile: L21 [kLuTile][kLuNB + 1] and U12 [kLuNB][kLuTile + 1]
constexpr int kLuOpLd = kLuNB + 1;
constexpr size_t kLuUpdateLdsBytes = ((size_t)kLuTile * kLuOpLd + (size_t)kLuNB * (kLuTile + 1)) * 8;
// the diagonal solves: the triangular block [kLuNB][kLuNB] and the tile of X [kLuNB][kLuTile], static LDS
constexpr size_t kLuTriLdsBytes = ((size_t)kLuNB * kLuNB + (size_t)kLuNB * kLuTile) * 8;
static_assert(kLuSmallLdsBytes <= kLdsMaxBytes && kLuUpdateLdsBytes <= kLdsMaxBytes && kLuTriLdsBytes <= kLdsMaxBytes, "LDS images fit");
// The limits.  n <= 2^17: n^2 elements (the system of corrla_rbffit_* in workspace, 128 GiB) stay far inside size_t, and the
// largest grid, the (n / kLuTile)^2 = 2^22 tiles of the first trailing update, inside 2^31 - 1.
constexpr int64_t kLuMaxN = (int64_t)1 << 17;
constexpr int64_t kLuMaxRhs = (int64_t)1 << 20;  // (n / kLuTile) x (n_rhs / kLuTile) <= 2^25 tiles

}  // namespace k

enum class LuRoute : int { kNone = 0, kSmall = 1, kBlocked = 2 };

struct LuShape {
  int64_t n = 0, n_rhs = 0;  // n_rhs == 0: factor only
};

// what the device leaves for the one read-back of a call (lu_kernels.hpp fills it)
struct LuStatus {
  int64_t info;      // 0, or the 1-based column whose pivot was exactly zero or not finite
  double min_pivot;  // smallest |pivot| of the columns factored
  double max_u;      // largest |u_ij| (0 when info != 0)
};

struct LuPlan {
  bool ok = false;
  const char* error = nullptr;
  LuRoute route = LuRoute::kNone;
  int nb = k::kLuNB;
  int64_t npanels = 0;      // BLOCKED: panel p covers the columns [p nb, min(n, (p + 1) nb))
  int64_t nblocks = 0;      // SOLVE: block rows of nb
  int64_t max_chunks = 0;   // chunks of the first panel step = entries of the partial maxima
  int64_t maxu_blocks = 0;  // workgroups of the max |u_ij| pass, kLuTile rows each
  int64_t rhs_tiles = 0;    // column tiles of B
  int64_t factor_launches = 0, solve_launches = 0;
  size_t lds_small = k::kLuSmallLdsBytes, lds_update = k::kLuUpdateLdsBytes, lds_tri = k::kLuTriLdsBytes;
  // workspace: the status record, the partial maxima (value, row), the partial max |u|, ipiv when the caller passes none;
  // every piece rounded up to 256 bytes
  size_t ws_status = 256, ws_partials = 0, ws_maxu = 0, ws_ipiv = 0;
  size_t ws_bytes = 0;
  size_t ws_bound = 0;      // the stated upper bound of ws_bytes: 9 n + 2048
};

CORRLA_HD constexpr int64_t lu_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// panel step j: chunk c covers the rows [j + c kLuChunk, min(n, j + (c + 1) kLuChunk)); row j itself is the pivot row
CORRLA_HD constexpr int64_t lu_step_chunks(int64_t n, int64_t j) { return lu_ceil_div(n - j, k::kLuChunk); }
// panel [j0, j1): the tiles of the triangular solve (columns [j1, n)) and of the trailing update (rows and columns [j1, n))
CORRLA_HD constexpr int64_t lu_trail_tiles(int64_t n, int64_t j1) { return lu_ceil_div(n - j1, k::kLuTile); }
// piece i of width w of [base, n): what chunk i of a panel step (base = j, w = kLuChunk) and tile i of a trailing update
// (base = j1, w = kLuTile) cover
CORRLA_HD constexpr int64_t lu_piece_begin(int64_t base, int64_t i, int64_t w) { return base + i * w; }
CORRLA_HD constexpr int64_t lu_piece_end(int64_t base, int64_t i, int64_t w, int64_t n) { return base + (i + 1) * w < n ? base + (i + 1) * w : n; }
inline size_t lu_round256(size_t b) { return (b + 255) / 256 * 256; }
inline size_t lu_ws_bound(int64_t n) { return (size_t)9 * (size_t)n + 2048; }

inline LuPlan lu_plan(const LuShape& s) {
  LuPlan p;
  auto reject = [&](const char* why) {
    p.ok = false;
    p.error = why;
    return p;
  };
  if (s.n < 1) return reject("lu: n must be >= 1");
  if (s.n > k::kLuMaxN) return reject("lu: n must be <= 131072");
  if (s.n_rhs < 0) return reject("lu: n_rhs must be >= 0");
  if (s.n_rhs > k::kLuMaxRhs) return reject("lu: n_rhs must be <= 1048576");
  p.route = s.n <= k::kLuSmallN ? LuRoute::kSmall : LuRoute::kBlocked;
  p.npanels = lu_ceil_div(s.n, p.nb);
  p.nblocks = p.npanels;
  p.max_chunks = lu_step_chunks(s.n, 0);
  p.maxu_blocks = lu_ceil_div(s.n, k::kLuTile);
  p.rhs_tiles = lu_ceil_div(s.n_rhs, k::kLuTile);
  // 2 per column, 3 per panel but 1 for the last, 2 for max |u|
  p.factor_launches = p.route == LuRoute::kSmall ? 1 : 2 * s.n + 3 * p.npanels - 2 + 2;
  // the interchanges of B, then a diagonal solve per block and an update per block but the last, in both sweeps
  p.solve_launches = s.n_rhs == 0 ? 0 : 1 + 2 * (2 * p.nblocks - 1);
  p.ws_partials = lu_round256((size_t)p.max_chunks * 16);
  p.ws_maxu = lu_round256((size_t)p.maxu_blocks * 8);
  p.ws_ipiv = lu_round256((size_t)s.n * 8);
  p.ws_bytes = p.ws_status + p.ws_partials + p.ws_maxu + p.ws_ipiv;
  p.ws_bound = lu_ws_bound(s.n);
  p.ok = true;
  return p;
}

}  // namespace corrla
