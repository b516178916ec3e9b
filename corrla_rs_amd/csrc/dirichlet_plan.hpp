// The plan of the constrained Dirichlet sampler behind corrla_dirichlet_draws_* and corrla_dirichlet_sample_*
// (dirichlet_kernels.hpp, dirichlet_stage.hpp; constr_dirichlet_sample, space_samplers.rs:14-126).  Draw t of a call is a pure
// function of (seed, alphas, c_scale, t) -- the stream is defined in dirichlet_kernels.hpp -- so nothing data-sized is stored:
//   DRAW  one thread per draw writes its row (corrla_dirichlet_draws_*).
//   TEST  the draws of shot s are [s chunk, (s + 1) chunk).  A shot is cut into wps = ceil(chunk / R) ranges of R = 1024 draws
//         (the last may be short); range k of shot s is workgroup gw = s wps + k of the call, so the workgroups in the order of gw
//         walk the draws in increasing index, every draw once.  A workgroup generates its draws (4 per thread), tests them against
//         the box, and writes one bit per draw (16 words of 64) and its count.  No candidate row goes to memory.
//   SCAN  one block: the exclusive prefix of the counts of a launch on top of the running total of the call; sets the
//         "enough" word once the total reaches n_samples, and records the workgroup in which it did.
//   EMIT  one thread per word of the bitmask regenerates the accepted draws whose rank is below n_samples into row `rank`.
// A launch serves at most kDirLaunchWgs consecutive workgroups (TEST, SCAN, EMIT, in stream order, on one workspace), so the
// workspace does not depend on chunk_size or max_zshots.  Launches are queued in batches; after a batch the host reads the
// running state back once (24 bytes: the count, the workgroup that completed it, the "enough" word).  The first batch covers
// kDirFirstBatchWgs workgroups; batch b + 1 covers max(2 x batch b, 1.5 x the workgroups the acceptance seen so far asks for) -- 16 x batch b
// while nothing was accepted -- capped by what is left.  Batches at least double, so a call makes at most
// max_readbacks = 1 + ceil(log2(ceil(total_wgs / kDirFirstBatchWgs))) read-backs (dir_max_readbacks), kDirFirstBatchWgs = 1024.  The TEST and EMIT
// workgroups of launches queued behind the one that reached n_samples see the "enough" word and return at once.  The
// samples do not depend on the batching: they are the first n_samples set bits in the order of gw.
// Host code only, no HIP call: tests/test_dirichlet_plan.py compiles this header with the host compiler and pins the plan.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace corrla {
namespace k {

constexpr int kDirThreads = 256;
constexpr int kDirDPT = 4;                           // draws per thread of TEST
constexpr int kDirRange = kDirThreads * kDirDPT;     // R: draws per workgroup of TEST
constexpr int kDirWords = kDirRange / 64;            // 64-bit words of the bitmask per workgroup
constexpr int kDirRegD = 16;                         // widest row whose gammas stay in registers
constexpr int kDirMaxD = 128;
constexpr int64_t kDirLaunchWgs = 65536;             // workgroups per launch: 2^26 draws, 8 MiB of bits
constexpr int64_t kDirFirstBatchWgs = 1024;          // 2^20 draws before the first read-back: some 15 us of work, and an
                                                     // acceptance of 10^-5 already shows ten draws to estimate it from
constexpr int kDirMaxAttempts = 64;                  // of one Marsaglia-Tsang gamma (see dirichlet_kernels.hpp)
constexpr int kDirScanThreads = 256;

}  // namespace k

// how component j draws its gamma: from alpha_j alone, so every lane of a wave branches alike
enum class DirMethod : int { kExp = 0, kMt = 1, kBoost = 2 };  // alpha = 1; alpha > 1; alpha < 1
// corrla_ctx_last_dirichlet: registers or regenerate, times exponential-only or general
enum class DirRoute : int { kNone = 0, kRegExp = 1, kRegGeneral = 2, kRegenExp = 3, kRegenGeneral = 4 };

// One component as the kernels read it (a device table of d records).  d_mt and c_mt are the constants of Marsaglia-Tsang
// at shape a = alpha (kMt) or alpha + 1 (kBoost): d_mt = a - 1/3, c_mt = 1 / sqrt(9 d_mt); inv_alpha = 1 / alpha.  All in
// IEEE double, each operation rounded once, as written.
struct DirComp {
  double d_mt = 0.0, c_mt = 0.0, inv_alpha = 1.0;
  double lb = 0.0, ub = 0.0;  // the box of TEST; unused by DRAW
  int method = 0;
  int pad = 0;
};

inline DirComp dir_component(double alpha) {
  DirComp m;
  m.inv_alpha = 1.0 / alpha;
  if (alpha == 1.0) {
    m.method = (int)DirMethod::kExp;
    return m;
  }
  const double a = alpha > 1.0 ? alpha : alpha + 1.0;
  m.method = (int)(alpha > 1.0 ? DirMethod::kMt : DirMethod::kBoost);
  m.d_mt = a - 1.0 / 3.0;
  m.c_mt = 1.0 / std::sqrt(9.0 * m.d_mt);
  return m;
}

struct DirShape {
  int64_t d = 0;
  const double* alphas = nullptr;  // d values
  double c_scale = 1.0;
  // sampling only (n_samples = 0: a plan for corrla_dirichlet_draws_*, n draws from `first`)
  const double* bounds = nullptr;  // d x 2 row-major
  int64_t n_samples = 0, max_zshots = 1, chunk_size = 1;
  int64_t first = 0, n = 0;
};

struct DirPlan {
  bool ok = false;
  const char* error = nullptr;
  int reg_width = 0;          // the padded width of the register route (4 or 16); 0: regenerate
  bool exp_only = false;      // every alpha is 1
  DirRoute route = DirRoute::kNone;
  int dpt = k::kDirDPT, range = k::kDirRange, words = k::kDirWords;
  unsigned block = k::kDirThreads;
  unsigned draw_grid_x = 0;   // DRAW: thread i of the grid writes draw first + i
  int64_t wps = 0;            // workgroups per shot; range k of a shot covers [k R, min(chunk, (k + 1) R))
  int64_t total_wgs = 0;      // max_zshots * wps
  int64_t launch_wgs = 0;     // workgroups of a full launch: min(total_wgs, kDirLaunchWgs)
  int64_t first_batch_wgs = 0;
  int max_readbacks = 0;
  size_t ws_mask_bytes = 0;   // [launch_wgs][16] words
  size_t ws_count_bytes = 0;  // [launch_wgs] uint32
  size_t ws_prefix_bytes = 0; // [launch_wgs] uint64
  size_t ws_table_bytes = 0;  // [d] DirComp
  size_t ws_bytes = 0;        // their sum, each rounded up to 256 bytes, plus 256 for the state
  size_t ws_bound = 0;
};

// Upper bound of the workspace, whatever the call: 128 + 4 + 8 bytes per workgroup of a launch (8.75 MiB), the table of 128
// components, the state and the rounding.
inline size_t dir_ws_bound() {
  return (size_t)k::kDirLaunchWgs * (k::kDirWords * 8 + 4 + 8) + (size_t)k::kDirMaxD * sizeof(DirComp) + 5 * 256;
}

inline int dir_max_readbacks(int64_t total_wgs) {
  int n = 1;
  for (int64_t b = k::kDirFirstBatchWgs; b < total_wgs; b *= 2) ++n;  // total_wgs < 2^62: b does not overflow
  return n;
}

// The workgroups of the next batch: `done` of `total` workgroups ran and accepted `found` of the n_samples; `prev` is the
// size of the batch before (0 for the first).  The draws of a workgroup are taken as R, which only rounds the estimate.
inline int64_t dir_next_batch(int64_t total, int64_t done, int64_t found, int64_t n_samples, int64_t prev) {
  const int64_t left = total - done;
  if (prev == 0) return std::min(left, k::kDirFirstBatchWgs);
  double want = 16.0 * (double)prev;
  if (found > 0) want = 1.5 * (double)(n_samples - found) * ((double)done / (double)found);
  want = std::max(want, 2.0 * (double)prev);
  return want >= (double)left ? left : std::max<int64_t>(1, (int64_t)want);
}

inline DirPlan dir_plan(const DirShape& s) {
  DirPlan p;
  auto reject = [&](const char* why) {
    p.ok = false;
    p.error = why;
    return p;
  };
  auto round256 = [](size_t b) { return (b + 255) / 256 * 256; };
  if (s.d < 2 || s.d > k::kDirMaxD) return reject("dirichlet: d must be in [2, 128]");
  if (!s.alphas) return reject("dirichlet: alphas is NULL");
  for (int64_t j = 0; j < s.d; ++j)
    if (!std::isfinite(s.alphas[j]) || !(s.alphas[j] > 0.0)) return reject("dirichlet: every alphas[j] must be finite and > 0");
  if (!std::isfinite(s.c_scale) || !(s.c_scale > 0.0)) return reject("dirichlet: c_scale must be finite and > 0");
  p.exp_only = true;
  for (int64_t j = 0; j < s.d; ++j) p.exp_only = p.exp_only && s.alphas[j] == 1.0;
  p.reg_width = s.d <= 4 ? 4 : (s.d <= k::kDirRegD ? k::kDirRegD : 0);
  p.route = p.reg_width ? (p.exp_only ? DirRoute::kRegExp : DirRoute::kRegGeneral) : (p.exp_only ? DirRoute::kRegenExp : DirRoute::kRegenGeneral);
  p.ws_table_bytes = (size_t)s.d * sizeof(DirComp);
  if (s.n_samples == 0) {  // DRAW
    if (s.first < 0) return reject("dirichlet: first must be >= 0");
    if (s.n < 1) return reject("dirichlet: n must be >= 1");
    if (s.n > ((int64_t)1 << 62) - s.first) return reject("dirichlet: first + n must be <= 2^62");
    const int64_t blocks = (s.n + p.block - 1) / p.block;
    if (blocks > 0x7fffffff) return reject("dirichlet: n gives more than 2^31 - 1 workgroups");
    p.draw_grid_x = (unsigned)blocks;
    p.ws_bytes = round256(p.ws_table_bytes);
    p.ws_bound = dir_ws_bound();
    p.ok = true;
    return p;
  }
  if (!s.bounds) return reject("dirichlet: bounds is NULL");
  if (s.n_samples < 1) return reject("dirichlet: n_samples must be >= 1");
  if (s.max_zshots < 1) return reject("dirichlet: max_zshots must be >= 1");
  if (s.chunk_size < 1) return reject("dirichlet: chunk_size must be >= 1");
  if (s.max_zshots > (((int64_t)1 << 62) - 1) / s.chunk_size) return reject("dirichlet: max_zshots * chunk_size must be < 2^62");
  double sum_lb = 0.0, sum_ub = 0.0;
  for (int64_t j = 0; j < s.d; ++j) {
    const double lb = s.bounds[2 * j], ub = s.bounds[2 * j + 1];
    if (!std::isfinite(lb) || !std::isfinite(ub)) return reject("dirichlet: every bounds[j] must be finite");
    if (lb > ub) return reject("dirichlet: bounds[j][0] must be <= bounds[j][1]");
    sum_lb += lb;
    sum_ub += ub;
  }
  // the box must meet the simplex sum x = c_scale; 8 ulp of slack per component for the rounding of the two sums
  const double slack = 8.0 * 2.220446049250313e-16 * (double)s.d * s.c_scale;
  if (sum_lb > s.c_scale + slack || sum_ub < s.c_scale - slack)
    return reject("dirichlet: bounds leave no point with sum c_scale (infeasible box)");
  p.wps = (s.chunk_size + p.range - 1) / p.range;
  p.total_wgs = s.max_zshots * p.wps;  // <= max_zshots * chunk_size < 2^62
  p.launch_wgs = std::min(p.total_wgs, k::kDirLaunchWgs);
  p.first_batch_wgs = std::min(p.total_wgs, k::kDirFirstBatchWgs);
  p.max_readbacks = dir_max_readbacks(p.total_wgs);
  p.ws_mask_bytes = (size_t)p.launch_wgs * p.words * 8;
  p.ws_count_bytes = (size_t)p.launch_wgs * 4;
  p.ws_prefix_bytes = (size_t)p.launch_wgs * 8;
  p.ws_bytes = round256(p.ws_mask_bytes) + round256(p.ws_count_bytes) + round256(p.ws_prefix_bytes) + round256(p.ws_table_bytes) + 256;
  p.ws_bound = dir_ws_bound();
  p.ok = true;
  return p;
}

}  // namespace corrla
