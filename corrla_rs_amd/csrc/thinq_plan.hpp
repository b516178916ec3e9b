// The plan of the thin-Q orthonormalisation (random_svd.rs:38,57): which factor-and-invert serves a sketch of l columns
// (one chol_inv_kernel, the 2 x 2 blocked form, or the host-controlled loop), whether the device-robust schedule applies
// and what each of its passes does, the shift of a robust pass, the panel tree of the Householder TSQR with the sizes of
// its buffers and the LDS of its four launches, and the grids of the small launches.  thinq_stage.hpp launches what the
// plan says, driver.hpp loops over the schedule, the host emulation of the tests answers the same fit questions from the
// same functions; none of them computes any of it again.
// Host code only, no HIP call: tests/test_thinq_plan.py compiles this header with the host compiler and pins the route at
// every l and every field.  The kernels that use the size helpers on the device include it through cholqr_kernels.hpp
// and tsqr_kernels.hpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

#include "gemm_plan.hpp"  // col_blocking; kLdsMaxBytes and CORRLA_HD through core_svd_plan.hpp

namespace corrla {
namespace k {

// ---- status records the kernels of the stage (and the core SVD's) leave for the host ----
struct CholStatus {
  int fail;
  float min_ratio;
  float dev_i;
  float gmax;
  long long clk, wall;  // shader-clock and 100 MHz wall-clock ticks spent in the elimination loop
};
// bits of a need_next word besides bit 0 ("run another pass"): what the pass saw, for the host's end-of-call verdict
constexpr int kNeedNonFinite = 2;  // a non-finite Gram matrix: the call ends with CORRLA_ENUMERIC, nothing to escalate
constexpr int kNeedNullCols = 4;   // null columns were found (and re-seeded at random): the sketch is rank deficient

// ---- chol_inv_kernel (cholqr_kernels.hpp) ----
// threads: one per 4 x 4 tile of the upper triangle.  f64 keeps 2 x 16 doubles of tile data per thread: at 1024 threads
// (128 VGPRs) the compiler spilled 22 of them into the elimination loop (287 us at r = 138 against 62 us in f32), so
// the f64 instantiation is bounded at 768 threads (170 VGPRs, r <= 152; wider f64 factors take the 2 x 2 blocked form)
template <class T>
CORRLA_HD constexpr int chol_inv_max_threads() { return sizeof(T) == 8 ? 768 : 1024; }
CORRLA_HD inline int chol_inv_threads(int r) {
  const int nt = (r + 3) / 4;
  return ((nt * (nt + 1) / 2 + 63) / 64) * 64;
}
// (the 32 floats are the kernel's reduction scratch; it also holds 16 wave maxima in the element type -- 128 bytes in f64)
CORRLA_HD inline size_t chol_inv_lds_bytes(int r, size_t esz) {
  return (size_t)6 * (((size_t)r + 3) / 4 * 4) * esz + 32 * sizeof(float) + 64;
}
CORRLA_HD inline bool chol_inv_fits(int r, size_t esz) {
  return r >= 1 && chol_inv_threads(r) <= (esz == 8 ? 768 : 1024);  // r <= 176 (f32) / 152 (f64)
}

// ---- Householder TSQR panels (tsqr_kernels.hpp) ----
constexpr int kHhThreads = 1024;  // 16 waves per panel: four per SIMD hide the load -> reduce -> update chain of a column group
constexpr int kHhMaxRowsPerLane = 5;  // ceil(2 * 138 / 64): panel rows a lane may own in one column
constexpr int kWyNb = 16;             // columns of a compact-WY block
constexpr int kWyExtra = 2 * kWyNb * kWyNb + kWyNb;  // Ts, Rs (parked diagonal block), tau_s (elements) in front of the panel
CORRLA_HD inline int hh_pitch(int rows) { return (rows + 3) & ~3; }
CORRLA_HD inline size_t hh_lds_bytes(int max_rows, int l, size_t esz) {
  return (size_t)hh_pitch(max_rows) * (size_t)l * esz + 64;
}
CORRLA_HD inline size_t hh_wy_lds_bytes(int max_rows, int l, size_t esz) {
  return hh_lds_bytes(max_rows, l, esz) + (size_t)kWyExtra * esz;
}
CORRLA_HD inline int hh_wy_panels(int l) { return (l + kWyNb - 1) / kWyNb; }
// rows of leaf i when m rows are cut into nleaf panels
CORRLA_HD inline int64_t hh_leaf_row0(int64_t m, int nleaf, int i) { return (m * (int64_t)i) / nleaf; }

}  // namespace k

constexpr int64_t kHhNoCap = std::numeric_limits<int64_t>::max();
// What the backend reads from the environment, once per context.
struct ThinQKnobs {
  bool host_chol = false;  // CORRLA_HOST_CHOL: no device factor at all, every thin-Q takes the host-controlled loop
  bool robust_qr = true;   // CORRLA_DEVICE_ROBUST_QR (0: the round-1 optimistic CholeskyQR2 + host-controlled repeat)
  int64_t hh_block = kHhNoCap;  // CORRLA_HH_BLOCK: cap on the width of a Householder column block
};

// ---- Cholesky-QR: the route of a sketch of l columns ----
enum class ThinQFactor {
  kSingle,      // one chol_inv_kernel factorises and inverts the l x l Gram
  kBlocked2x2,  // 2 x 2 blocked (driver.hpp: blocked_factor_inverse): one chol_inv_kernel per diagonal block
  kNone,        // the host-controlled loop of orthonormalize_core
};
struct CholInvLaunch {
  int n = 0;         // order of the block; 0: no launch
  unsigned threads = 0;
  size_t lds = 0;
};
inline CholInvLaunch chol_inv_launch(int r, size_t esz) {
  return {r, (unsigned)k::chol_inv_threads(r), k::chol_inv_lds_bytes(r, esz)};
}
struct ThinQRoute {
  ThinQFactor factor = ThinQFactor::kNone;
  int64_t n1 = 0, n2 = 0;   // orders of the diagonal blocks (single: l, 0)
  int records_per_pass = 0;  // status records a pass writes: 1 / 2 / 0
  bool robust = false;       // the device-robust schedule (orthonormalize_device) may take this sketch
  bool inplace = false;      // one column block: the products of a pass may run in place
  CholInvLaunch blk[2];      // the chol_inv_kernel launch of each diagonal block
};
// The split of the 2 x 2 blocked form: n1 = round_up((l + 1) / 2, 4), n2 = l - n1.
inline int64_t blocked_split_n1(int64_t l) { return ((l + 1) / 2 + 3) / 4 * 4; }
// Single wins where both fit: f32 l <= 176 single, 177 ... 352 blocked; f64 l <= 152 single, 153 ... 304 blocked.  The
// blocked form needs l > 8 (never chosen below: the single kernel takes those).
inline ThinQRoute thinq_route(size_t esz, int64_t l, const ThinQKnobs& kn) {
  ThinQRoute r;
  r.inplace = col_blocking(l).nblk == 1;
  if (kn.host_chol || l < 1 || l > 4096) return r;
  const int64_t n1 = blocked_split_n1(l);
  if (k::chol_inv_fits((int)l, esz)) {
    r.factor = ThinQFactor::kSingle;
    r.n1 = l;
    r.records_per_pass = 1;
    r.blk[0] = chol_inv_launch((int)l, esz);
  } else if (l > 8 && k::chol_inv_fits((int)n1, esz)) {
    r.factor = ThinQFactor::kBlocked2x2;
    r.n1 = n1;
    r.n2 = l - n1;
    r.records_per_pass = 2;
    r.blk[0] = chol_inv_launch((int)r.n1, esz);
    r.blk[1] = chol_inv_launch((int)r.n2, esz);
  }
  r.robust = kn.robust_qr && r.factor != ThinQFactor::kNone;
  return r;
}

// ---- the device-robust thin-Q (driver.hpp: orthonormalize_device): what each enqueued pass does ----
constexpr int kRobustMaxPasses = 8;  // most passes one thin-Q enqueues
enum class RobustMode {
  kFinal,   // the thin-Q of random_svd.rs:57: two unconditional passes, the rest conditional
  kInLoop,  // random_svd.rs:37-39 (rough): one shifted pass, judged by its pivots; the conditional chain is best effort
  kPolish,  // the input is orthonormal up to a small defect: no shift, every pass after the first conditional
};
struct RobustSchedule {
  int npass = 0, always = 0;  // passes enqueued / of them unconditional
  // slot (relative to the first need_next word of this thin-Q) the Pending record names; -1: best effort, not verified
  int flag_slot = 0;
  struct Pass {
    int gate;           // need_next word (relative) every launch of the pass carries as run_if; -1: none
    int shift_mode;     // CholRobust::shift_mode
    bool null_excess;   // the null excess applies (directions below the shift level are re-seeded)
    float need_ratio;   // CholRobust::need_ratio
    bool refill;        // refill_null follows the product
  } pass[kRobustMaxPasses] = {};
};
// passes: the context's count, 2 -> 4 -> 8 (HipDev::robust_passes).  In place a conditional pass is gated by the pass
// before; out of place the conditional passes come in PAIRS gated by the pass before the pair, so that a skipped pair
// leaves the data where the host expects it.
inline RobustSchedule robust_schedule(int passes, RobustMode mode, bool inplace) {
  const int level = std::max(2, std::min(passes, kRobustMaxPasses));
  const bool inloop = mode == RobustMode::kInLoop, polish = mode == RobustMode::kPolish;
  RobustSchedule s;
  s.npass = inloop ? (level <= 2 ? 1 : level - 1) : (polish ? (level <= 2 ? 1 : 3) : level);
  s.always = (polish || inloop) ? 1 : 2;
  // in-loop: only the single pass of a level-2 context is verified (so that the context escalates)
  s.flag_slot = (inloop && s.npass > 1) ? -1 : 0;
  for (int p = 0; p < s.npass; ++p) {
    RobustSchedule::Pass& q = s.pass[p];
    q.gate = p < s.always ? -1 : (inplace ? p - 1 : s.always + ((p - s.always) / 2) * 2 - 1);
    q.shift_mode = polish ? 2 : (p == 0 ? 1 : 0);
    q.null_excess = !polish && p >= 2;
    q.need_ratio = (inloop && p == 0) ? 1e-2f : 0.f;
    // (a re-seeded column needs a following pass to be orthonormalised: none after the last one; in-loop, the next
    // products with A and the next thin-Q take care of it)
    q.refill = p + 1 < s.npass || inloop;
  }
  return s;
}
// Relative shift of a robust pass: as small as the rounding error of the computed Gram allows (~ eps sqrt(rows)), never
// below the 16 eps of the host-controlled path; the Schur complement of the blocked form carries ~l eps.
inline double robust_shift_rel(size_t esz, int64_t rows, int64_t l, bool single) {
  const double eps = esz == 4 ? (double)std::numeric_limits<float>::epsilon() : std::numeric_limits<double>::epsilon();
  return eps * std::max({16.0, 0.25 * std::sqrt((double)std::max<int64_t>(rows, 1)), single ? 0.0 : 2.0 * (double)l});
}

// ---- grids of the small launches ----
struct Grid2 {
  unsigned x, y, block;
};
inline Grid2 refill_null_grid(int64_t rows, int64_t l) {
  return {(unsigned)std::max<int64_t>(std::min<int64_t>(64, (rows + 255) / 256), 1), (unsigned)l, 256u};
}
inline Grid2 series_grid(int64_t r) { return {(unsigned)((r + 63) / 64), (unsigned)r, 64u}; }

// ---- Householder TSQR ----
// One 2 l x l panel plus the 16 x 16 T and parked-R blocks of the compact-WY form must fit in LDS, and a lane owns at
// most kHhMaxRowsPerLane rows of a column: l <= 142 (f32) / 99 (f64).
inline bool hh_fits(size_t esz, int64_t l) {
  return l >= 1 && l <= 4096 && k::hh_wy_lds_bytes((int)(2 * l), (int)l, esz) <= k::kLdsMaxBytes && 2 * l <= 64 * k::kHhMaxRowsPerLane;
}
inline int hh_max_width(size_t esz) {
  int w = 1;
  while (hh_fits(esz, w + 1)) ++w;
  return w;
}
// ... and the widest column block under a cap (ThinQKnobs::hh_block): what a backend answers householder_max_width with
inline int64_t hh_capped_width(int64_t wmax, int64_t cap) { return std::max<int64_t>(1, std::min(wmax, cap)); }
constexpr int kHhMaxLevels = 32;
struct HhTreePlan {
  const char* error = nullptr;  // the launch is refused with this message
  bool fits = false;
  int nleaf = 0, max_rows = 0, levels = 0;
  int n_at[kHhMaxLevels] = {};  // nodes at level 0 (the leaves) ... levels (the root)
  // elements of the call-lifetime buffers of level k: R factors, coefficient blocks, tau, tree reflectors (none at the
  // leaves: theirs go to the caller's tmp), T factors of the 16-column blocks
  size_t r_elems[kHhMaxLevels] = {}, c_elems[kHhMaxLevels] = {}, tau_elems[kHhMaxLevels] = {}, v_elems[kHhMaxLevels] = {},
         t_elems[kHhMaxLevels] = {};
  size_t lds_up_leaf = 0, lds_up_tree = 0;      // factor kernels: panel + the WY blocks
  size_t lds_down_tree = 0, lds_down_leaf = 0;  // apply kernels: the panel alone
};
// The TSQR of an m x l sketch: row panels of at most 2 l rows, combined pairwise level by level.
inline HhTreePlan hh_tree_plan(size_t esz, int64_t m, int64_t l64) {
  HhTreePlan p;
  p.fits = hh_fits(esz, l64);
  if (m < l64) return p.error = "householder_thin_q: fewer rows than columns", p;
  if (!p.fits) return p.error = "householder_thin_q: panel does not fit in LDS", p;
  const int l = (int)l64;
  const int64_t br = 2 * l64;
  const int64_t nleaf64 = m <= br ? 1 : (m + br - 1) / br;
  if (nleaf64 > 0x3fffffff) return p.error = "householder_thin_q: too many panels", p;
  p.nleaf = (int)nleaf64;
  p.max_rows = (int)std::min<int64_t>(m, br);
  p.n_at[0] = p.nleaf;
  while (p.n_at[p.levels] > 1) p.n_at[p.levels + 1] = (p.n_at[p.levels] + 1) / 2, ++p.levels;
  const size_t ll = (size_t)l * l, tsz = (size_t)k::hh_wy_panels(l) * k::kWyNb * k::kWyNb;
  for (int k_ = 0; k_ <= p.levels; ++k_) {
    const size_t n = (size_t)p.n_at[k_];
    p.r_elems[k_] = p.c_elems[k_] = ll * n;
    p.tau_elems[k_] = (size_t)l * n;
    p.v_elems[k_] = k_ >= 1 ? 2 * ll * n : 0;
    p.t_elems[k_] = tsz * n;
  }
  p.lds_up_leaf = k::hh_wy_lds_bytes(p.max_rows, l, esz);
  p.lds_up_tree = k::hh_wy_lds_bytes(2 * l, l, esz);
  p.lds_down_leaf = k::hh_lds_bytes(p.max_rows, l, esz);
  p.lds_down_tree = k::hh_lds_bytes(2 * l, l, esz);
  return p;
}
// Sketches wider than one panel: nb column blocks of at most w columns (householder_thin_q_any_width); cap: ThinQKnobs::hh_block.
struct HhColumnBlocks {
  int64_t nb, w;
};
inline HhColumnBlocks hh_column_blocks(int64_t l, int64_t wmax, int64_t cap = kHhNoCap) {
  wmax = hh_capped_width(wmax, cap);
  if (l <= wmax) return {1, l};
  const int64_t nb = (l + wmax - 1) / wmax;
  return {nb, (l + nb - 1) / nb};
}

}  // namespace corrla
