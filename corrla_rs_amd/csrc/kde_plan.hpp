// The plan of the pairwise-sum kernels behind corrla_kde_eval_* and corrla_kde_nll_* (kde_kernels.hpp, kde_stage.hpp): a
// Gaussian kernel density estimate over n_s supports at n_q points, for one bandwidth (pdf, cdf, logpdf) or for up to 64 of
// them at once (the likelihood and its derivative).  The n_q x n_s kernel matrix is never stored.
//   NEAREST  d*_i = min_j (x_i - s_j)^2: a workgroup owns QT points (PP per thread) and one contiguous range of the supports
//            (a split), staged SC at a time; each split writes its partial minimum to workspace.  Not run for cdf.
//   SUM      the same tiles and splits, times the bandwidth groups of HG: the stabilised sums of a (tile, group, split) go to
//            workspace.  A call with more than HL bandwidths is served by several launches of HL, which reuse the workspace
//            of the sums in stream order.
//   FINISH   adds the splits in index order and applies ln, the normalisation and t*; the likelihood reduces over the points
//            in f64 by a fixed tree of `red_blocks` blocks, then one block per bandwidth.
// The splits depend on n_q and n_s only -- not on the number of bandwidths, so that a bandwidth's sums are the same bits
// whichever others it is grouped with.
// Host code only, no HIP call: tests/test_kde_plan.py compiles this header with the host compiler and pins the plan.  The
// kernels take the tile sizes from it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace corrla {
namespace k {

constexpr int kKdeThreads = 256;
constexpr int kKdePP = 2;                       // points a thread keeps in registers
constexpr int kKdeQT = kKdeThreads * kKdePP;    // points per workgroup
constexpr int kKdeSC = 1024;                    // supports per staged chunk: 4 KiB of LDS in f32, 8 KiB in f64
constexpr int kKdeHG = 4;                       // bandwidths per register pass: d^2 is formed once for all of them
constexpr int kKdeHL = 8;                       // bandwidths per launch: bounds the workspace of the sums
constexpr int kKdeMaxH = 64;                    // bandwidths per call
constexpr int kKdeRedMax = 256;                 // blocks of the likelihood's first reduction: one partial per thread of the second
// workgroups the splits aim at: four per CU of the 256, as kRbfTargetWgs
constexpr int64_t kKdeTargetWgs = 4 * 256;

}  // namespace k

enum class KdeMode : int { kPdf = 0, kCdf = 1, kLogpdf = 2, kNll = 3 };
enum class KdeRoute : int { kNone = 0, kSingle = 1, kSplit = 2 };  // corrla_ctx_last_kde: one range of supports, or several

struct KdeShape {
  int64_t n_q = 0, n_s = 0;
  int64_t n_h = 1;  // bandwidths: 1 for pdf, cdf and logpdf
  int esz = 8;
  KdeMode mode = KdeMode::kPdf;
};

struct KdePlan {
  bool ok = false;
  const char* error = nullptr;
  int qt = k::kKdeQT, sc = k::kKdeSC, hg = k::kKdeHG, hl = k::kKdeHL;
  int nacc = 1;           // sums per (point, bandwidth): 2 for the likelihood (sum K and sum e K), else 1
  bool nearest = true;    // the NEAREST pass runs (not for cdf)
  int64_t nqt = 0;        // point tiles: tile b covers the points [b qt, min(n_q, (b + 1) qt))
  int64_t nchunks = 0;    // chunks of sc supports in all
  int64_t nsplit = 1;     // split s covers the supports [s split_len, min(n_s, (s + 1) split_len)), none empty
  int64_t split_len = 0;  // a multiple of sc
  int64_t nlaunch = 1;    // SUM launches: launch l serves the bandwidths [l hl, min(n_h, (l + 1) hl))
  int nb_full = 1, nb_last = 1;  // bandwidths of every launch but the last, and of the last
  unsigned block = k::kKdeThreads;
  unsigned near_grid_x = 0;                    // workgroup w owns (tile w % nqt, split w / nqt); 0 when the pass is not run
  unsigned sum_grid_full = 0, sum_grid_last = 0;  // (tile w % nqt, group (w / nqt) % ngroups, split w / (nqt ngroups))
  unsigned finish_grid_x = 0, finish_block = 256;  // pdf, cdf, logpdf: one thread per point
  unsigned red_blocks = 0;  // likelihood: grid (red_blocks, bandwidths of the launch), block b reduces the points
  int64_t red_len = 0;      //   [b red_len, min(n_q, (b + 1) red_len)), a multiple of 256; then grid n_h of one block each
  size_t lds_bytes = 0;     // static: sc elements
  size_t ws_min_bytes = 0;  // [nsplit][n_q]
  size_t ws_sum_bytes = 0;  // [nsplit][nacc][nb_full][n_q]
  size_t ws_red_bytes = 0;  // doubles [n_h][red_blocks][2]
  size_t ws_bytes = 0;      // their sum, each rounded up to 256 bytes
  size_t ws_bound = 0;      // the stated upper bound of ws_bytes for this shape
  KdeRoute route = KdeRoute::kNone;
};

// Upper bound of the workspace.  With one split the partials have the size of the result, n_q elements per (sum, bandwidth
// of a launch) and n_q for the minima.  With more, nqt < target and nsplit <= 2 (target / nqt + 1) (whole chunks per split,
// rounded down), so nsplit n_q <= 2 (target + nqt) qt < 4 target qt.  At most 2 hl + 1 = 17 such arrays (272 MiB in f64
// while the supports are split), and two doubles per (bandwidth, reduction block): 256 KiB; 768 bytes of rounding.
inline size_t kde_ws_bound(int64_t n_q, int64_t n_h, int nacc, int esz) {
  const size_t rows = std::max((size_t)n_q, (size_t)(4 * k::kKdeTargetWgs) * k::kKdeQT);
  const size_t arrays = (size_t)nacc * (size_t)std::min<int64_t>(n_h, k::kKdeHL) + 1;
  return rows * arrays * (size_t)esz + (size_t)n_h * k::kKdeRedMax * 2 * sizeof(double) + 768;
}

inline KdePlan kde_plan(const KdeShape& s) {
  KdePlan p;
  auto reject = [&](const char* why) {
    p.ok = false;
    p.error = why;
    return p;
  };
  auto round256 = [](size_t b) { return (b + 255) / 256 * 256; };
  if (s.esz != 4 && s.esz != 8) return reject("kde: element size (esz) must be 4 or 8");
  if (s.n_q < 1) return reject("kde: n_q must be >= 1");
  if (s.n_s < 1) return reject("kde: n_s must be >= 1");
  const bool nll = s.mode == KdeMode::kNll;
  if (s.n_h < 1 || s.n_h > (nll ? k::kKdeMaxH : 1)) return reject(nll ? "kde: n_h must be in [1, 64]" : "kde: n_h must be 1 for pdf, cdf and logpdf");
  p.nacc = nll ? 2 : 1;
  p.nearest = s.mode != KdeMode::kCdf;
  p.nqt = (s.n_q + p.qt - 1) / p.qt;
  p.nchunks = (s.n_s + p.sc - 1) / p.sc;
  // from n_q and n_s alone: enough splits to reach the target (whole chunks per split, rounded down, so that the target is
  // reached and not only approached), never more than there are chunks, none empty
  const int64_t want = std::min(p.nchunks, (k::kKdeTargetWgs + p.nqt - 1) / p.nqt);
  const int64_t chunks_per_split = p.nchunks / want;
  p.nsplit = (p.nchunks + chunks_per_split - 1) / chunks_per_split;
  p.split_len = chunks_per_split * p.sc;
  p.route = p.nsplit > 1 ? KdeRoute::kSplit : KdeRoute::kSingle;
  p.nlaunch = (s.n_h + p.hl - 1) / p.hl;
  p.nb_full = (int)std::min<int64_t>(s.n_h, p.hl);
  p.nb_last = (int)(s.n_h - (p.nlaunch - 1) * p.hl);
  const int64_t tiles = p.nqt * p.nsplit;  // nqt <= 2^63 / 512 and nsplit < 4 target: no overflow
  const int64_t groups_full = (p.nb_full + p.hg - 1) / p.hg, groups_last = (p.nb_last + p.hg - 1) / p.hg;
  if (p.nqt > 0x7fffffff / p.nsplit || tiles > 0x7fffffff / groups_full)
    return reject("kde: n_q x splits x bandwidth groups gives more than 2^31 - 1 workgroups");
  p.near_grid_x = p.nearest ? (unsigned)tiles : 0u;
  p.sum_grid_full = (unsigned)(tiles * groups_full);
  p.sum_grid_last = (unsigned)(tiles * groups_last);
  p.lds_bytes = (size_t)p.sc * (size_t)s.esz;
  if (nll) {
    const int64_t blocks = std::min<int64_t>(k::kKdeRedMax, (s.n_q + 255) / 256);
    p.red_len = ((s.n_q + blocks - 1) / blocks + 255) / 256 * 256;
    p.red_blocks = (unsigned)((s.n_q + p.red_len - 1) / p.red_len);
    p.ws_red_bytes = (size_t)s.n_h * p.red_blocks * 2 * sizeof(double);
  } else {
    const int64_t blocks = (s.n_q + p.finish_block - 1) / p.finish_block;
    if (blocks > 0x7fffffff) return reject("kde: n_q gives more than 2^31 - 1 finishing workgroups");
    p.finish_grid_x = (unsigned)blocks;
  }
  p.ws_min_bytes = p.nearest ? (size_t)p.nsplit * (size_t)s.n_q * (size_t)s.esz : 0;
  p.ws_sum_bytes = (size_t)p.nsplit * (size_t)p.nacc * (size_t)p.nb_full * (size_t)s.n_q * (size_t)s.esz;
  p.ws_bytes = round256(p.ws_min_bytes) + round256(p.ws_sum_bytes) + round256(p.ws_red_bytes);
  p.ws_bound = kde_ws_bound(s.n_q, s.n_h, p.nacc, s.esz);
  p.ok = true;
  return p;
}

}  // namespace corrla
