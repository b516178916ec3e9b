// The plan of the symmetric eigensolver behind corrla_eigh_* (eigh_kernels.hpp, eigh_stage.hpp): A = V diag(w) V^T, f64 only.
// A is ROW-major (n x n, row stride lda); only its LOWER triangle (i >= j) is ever read.  w ascending, V row-major with the
// eigenvectors in its columns.
//   SMALL    n <= kEighSmallN: one workgroup, one launch.  The blocked route with one pair that holds every column, in LDS:
//            B = A + sigma I, its Cholesky factor, and per sweep the Gram matrix, the threshold Jacobi and W <- W R.
//   BLOCKED  sigma = 1.5 min(|A|_F, |A|_inf) (2 launches and the first read-back), B = A + sigma I into workspace (1), the
//            blocked Cholesky B = L L^T by the launchers of chol_stage.hpp (the Cholesky plan's count), the repack of L into
//            column panels of kEighB (1), then one-sided block Jacobi on W = L: per round of the tournament three launches
//            (Gram, rotation, apply) and per sweep one that folds the pairs' measures into the sweep record.  The host reads
//            the record of the first sweep, then the records of every group of kEighGroup sweeps.  The finish is six launches (column norms, unit columns,
//            Rayleigh quotients, their sums, ranks, scatter).
// The tournament: nb column blocks, m = nb rounded up to even, m - 1 rounds.  Round r pairs the blocks (r + q) mod (m - 1)
// and (r - q) mod (m - 1) for q = 1 .. m / 2 - 1, and r itself with m - 1 -- which is a block when nb is even and the bye when
// nb is odd.  So a round has nb / 2 (rounded down) pairs, all disjoint, and a sweep visits every unordered pair exactly once.
// The same tournament over the 64 indices of a pair's Gram matrix orders the rotations of the LDS Jacobi.
// Host code only, no HIP call: tests/test_eigh_plan.py compiles this header with the host compiler and pins the plan.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "chol_plan.hpp"
#include "core_svd_plan.hpp"  // kLdsMaxBytes, kJmcMaxSweeps, CORRLA_HD

namespace corrla {
namespace k {

constexpr int kEighB = 32;             // columns of a block: a pair is 64 columns, one MFMA tile of four 16-wide column tiles
constexpr int kEighPair = 2 * kEighB;  // order of a pair's Gram matrix and of its rotation
constexpr int kEighSmallN = 64;
constexpr int kEighThreads = 256;
constexpr int kEighChunk = 64;        // rows of a panel per LDS stage of the Gram and apply kernels
constexpr int kEighMaxSweeps = kJmcMaxSweeps;
constexpr int kEighInnerSweeps = 1;   // sweeps of the LDS Jacobi on one pair's Gram matrix: more cost accuracy
constexpr int kEighGroup = 2;         // sweeps enqueued between two read-backs of the sweep records
constexpr int64_t kEighMaxN = 32768;
// LDS images.  The operand reads are those of the Cholesky updates: a [row][k] image with a row stride of 66 doubles and a
// [k][col] image with a row stride of 80 doubles are both free of bank conflicts (chol_plan.hpp).
constexpr int kEighRowLd = kCholRowLd;  // 66
constexpr int kEighColLd = kCholColLd;  // 80
constexpr int kEighJacLd = kEighPair + 1;  // the Jacobi walks rows and columns: an odd stride
// Gram: one [k][col] image of a chunk of both panels, which is both operands of X^T X
constexpr size_t kEighGramLdsBytes = (size_t)kEighChunk * kEighColLd * 8;
// apply: the chunk as [row][k] and R as [k][col]
constexpr size_t kEighApplyLdsBytes = ((size_t)kEighChunk * kEighRowLd + (size_t)kEighPair * kEighColLd) * 8;
// rotation: G and R as [64][65], the rotations of a step (c, s per pair), the reduction scratch; SMALL: W as well
constexpr size_t kEighJacLdsBytes = ((size_t)2 * kEighPair * kEighJacLd + 2 * kEighB + 2 * kEighThreads) * 8;
constexpr size_t kEighSmallLdsBytes = kEighJacLdsBytes + (size_t)kEighPair * kEighJacLd * 8;
// Rayleigh quotients: a tile of A as [row][k] or [k][row], 64 rows of a block of U as [k][col] with a row stride of 48 doubles
// (96 dwords = 32 mod 64, as 80 doubles are)
constexpr int kEighRayUld = kEighB + 16;
constexpr size_t kEighRayLdsBytes = ((size_t)64 * kEighColLd + (size_t)64 * kEighRayUld) * 8;
static_assert(kEighGramLdsBytes <= 65536 && kEighApplyLdsBytes <= kLdsMaxBytes && kEighJacLdsBytes <= kLdsMaxBytes &&
                  kEighSmallLdsBytes <= kLdsMaxBytes && kEighRayLdsBytes <= kLdsMaxBytes,
              "LDS images fit");

}  // namespace k

enum class EighRoute : int { kNone = 0, kSmall = 1, kBlocked = 2 };

struct EighShape {
  int64_t n = 0;
  int num_cus = 256;
};

// what the norm launches (BLOCKED) or the one launch (SMALL) leave for the host
struct EighHeader {
  double sigma;   // the shift; 0: the zero matrix
  double fro;     // |A|_F and |A|_inf over the mirrored lower triangle
  double inf;
  double bad;     // != 0: a non-finite entry in the lower triangle
  double sweeps;  // SMALL: the sweeps that rotated, the largest measure met by the last sweep, 1 when the cap was hit
  double off;
  double capped;
  double pad;
};
// what the fold launch leaves per sweep
struct EighSweepRecord {
  double max_measure;  // the largest measure of the sweep's pairs
  double rotated;      // the pairs that were not skipped
};

struct EighPlan {
  bool ok = false;
  const char* error = nullptr;
  EighRoute route = EighRoute::kNone;
  int64_t nb = 0;          // column blocks of kEighB; the last may be partial
  int64_t rounds = 0;      // of a sweep
  int64_t pairs = 0;       // of a round
  int64_t slabs = 0;       // row slabs of the Gram and apply kernels
  int64_t slab_rows = 0;   // a multiple of kEighChunk
  int64_t norm_groups = 0; // workgroups of the norm kernel: row blocks of 64
  int64_t chol_launches = 0;
  int64_t prologue_launches = 0;  // norms (2), shift (1), Cholesky, repack (1)
  int64_t sweep_launches = 0;     // 3 rounds + 1
  int64_t finish_launches = 0;    // 6
  double tol = 0.0;               // 2 sqrt(n) 2^-53: a pair at or below it is skipped; the inner threshold is half of it
  size_t lds_gram = k::kEighGramLdsBytes, lds_apply = k::kEighApplyLdsBytes, lds_jac = k::kEighJacLdsBytes;
  size_t lds_small = k::kEighSmallLdsBytes, lds_ray = k::kEighRayLdsBytes;
  // workspace, each piece rounded up to 256 bytes
  size_t ws_header = 256, ws_norms = 0, ws_b = 0, ws_w = 0, ws_gram = 0, ws_r = 0, ws_meas = 0, ws_records = 0, ws_cols = 0, ws_ray = 0, ws_chol = 0;
  size_t ws_bytes = 0;
  int64_t launches(int64_t sweeps_enqueued) const { return prologue_launches + sweeps_enqueued * sweep_launches + finish_launches; }
};

CORRLA_HD constexpr int64_t eigh_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
CORRLA_HD constexpr int64_t eigh_rounds(int64_t nb) { return nb < 2 ? 0 : (nb + (nb & 1)) - 1; }
CORRLA_HD constexpr int64_t eigh_pairs(int64_t nb) { return nb / 2; }
// pair p of round r over nb blocks: *i < *j
CORRLA_HD inline void eigh_pair(int64_t nb, int64_t r, int64_t p, int64_t* i, int64_t* j) {
  const int64_t m = nb + (nb & 1), q = p + (nb & 1);  // odd nb: q = 0 would meet the bye
  int64_t a, b;
  if (q == 0) {
    a = r, b = m - 1;
  } else {
    a = (r + q) % (m - 1), b = (r - q + (m - 1)) % (m - 1);
  }
  *i = a < b ? a : b;
  *j = a < b ? b : a;
}
// the columns of block b that exist
CORRLA_HD constexpr int eigh_block_width(int64_t n, int64_t b) { return (int)((b + 1) * k::kEighB <= n ? k::kEighB : n - b * k::kEighB); }
inline size_t eigh_round256(size_t b) { return (b + 255) / 256 * 256; }
inline double eigh_tol(int64_t n) { return 2.0 * std::sqrt((double)n) * 0x1p-53; }

inline EighPlan eigh_plan(const EighShape& s) {
  EighPlan p;
  auto reject = [&](const char* why) {
    p.ok = false;
    p.error = why;
    return p;
  };
  if (s.n < 1) return reject("eigh: n must be >= 1");
  if (s.n > k::kEighMaxN) return reject("eigh: n must be <= 32768");
  p.tol = eigh_tol(s.n);
  p.route = s.n <= k::kEighSmallN ? EighRoute::kSmall : EighRoute::kBlocked;
  if (p.route == EighRoute::kSmall) {
    p.prologue_launches = 1;
    p.ws_bytes = p.ws_header;
    p.ok = true;
    return p;
  }
  const int64_t n = s.n;
  p.nb = eigh_ceil_div(n, k::kEighB);
  p.rounds = eigh_rounds(p.nb);
  p.pairs = eigh_pairs(p.nb);
  const int64_t chunks = eigh_ceil_div(n, k::kEighChunk);
  int64_t slabs = eigh_ceil_div(2 * (int64_t)(s.num_cus > 0 ? s.num_cus : 1), p.pairs);  // pairs x slabs: two workgroups per CU where the rows allow
  if (slabs > chunks) slabs = chunks;
  p.slab_rows = eigh_ceil_div(chunks, slabs) * k::kEighChunk;
  p.slabs = eigh_ceil_div(n, p.slab_rows);
  p.norm_groups = chunks;
  CholShape cs;
  cs.n = n, cs.n_rhs = 0;
  const CholPlan cp = chol_plan(cs);
  p.chol_launches = cp.factor_launches;
  p.prologue_launches = 2 + 1 + p.chol_launches + 1;
  p.sweep_launches = 3 * p.rounds + 1;
  p.finish_launches = 6;
  p.ws_norms = eigh_round256((size_t)p.norm_groups * 4 * 8);
  p.ws_b = eigh_round256((size_t)n * n * 8);
  p.ws_w = eigh_round256((size_t)p.nb * n * k::kEighB * 8);
  p.ws_gram = eigh_round256((size_t)p.pairs * p.slabs * k::kEighPair * k::kEighPair * 8);
  p.ws_r = eigh_round256((size_t)p.pairs * k::kEighPair * k::kEighPair * 8);
  p.ws_meas = eigh_round256((size_t)p.rounds * p.pairs * 2 * 8);
  p.ws_records = eigh_round256((size_t)(k::kEighMaxSweeps + k::kEighGroup) * sizeof(EighSweepRecord));
  p.ws_cols = eigh_round256((size_t)p.nb * k::kEighB * 3 * 8);  // per column: lambda, the scale with its sign, the rank
  p.ws_ray = eigh_round256((size_t)p.nb * chunks * k::kEighB * 8);
  p.ws_chol = cp.ws_bytes;
  p.ws_bytes = p.ws_header + p.ws_norms + p.ws_b + p.ws_w + p.ws_gram + p.ws_r + p.ws_meas + p.ws_records + p.ws_cols + p.ws_ray + p.ws_chol;
  p.ok = true;
  return p;
}

}  // namespace corrla
