// The gradient stage's plan (corrla_grad_mat_*): everything about the launches of a call -- which nearest-neighbour scan and
// which local-fit kernel serve it, their instantiation, grid, workgroup size, LDS and workspaces, or why the call is rejected
// -- and the LDS arithmetic those choices rest on.  grad_stage.hpp launches what the plan says and computes none of it again.
// Host code only, no HIP call: tests/test_grad_plan.py compiles this header with the host compiler and pins every field.
// The kernels that use the size helpers on the device include it through grad_kernels.hpp and knn2_kernels.hpp.
//
// Two families.  The LIMITED kernels (grad_kernels.hpp, knn2_kernels.hpp) keep per-query state in LDS and registers:
// k <= 64 features, n_nbrs <= 512 neighbours and one query's neighbours in 160 KiB of LDS.  Every call inside those limits
// takes them.  The WIDE kernels (grad_wide_kernels.hpp) stream the feature dimension and keep lists and normal equations in
// global memory, so they take any k and any n_nbrs; they serve exactly the calls the limited kernels cannot (a scan when
// k > 64 or n_nbrs > 512, a fit when the limited fits' check fails), and CORRLA_KNN=4 / CORRLA_FIT=2 force them.
// What is still rejected is about the arguments (the reference's own preconditions, the index range) or about memory:
// one wide-fit workspace slice of (P + 1)^2 + 2 (P + 1) doubles (P design columns) above the budget, kGradWideBudgetBytes.
#pragma once
#include <cstddef>
#include <cstdint>

#include "core_svd_plan.hpp"  // kLdsMaxBytes, CORRLA_HD

namespace corrla {
namespace k {

constexpr int kGradMaxDim = 64;    // features k
constexpr int kGradMaxNbr = 512;   // neighbours per query (register arrays of the list insertion; LDS is checked per call)
// design-matrix columns: k + 1 (order 1), k + k (k + 1) / 2 + 1 (order 2).  The neighbours of a query live in LDS
// (grad_fit_lds_bytes(k, n_nbrs, order, false) <= 160 KiB), its normal equations next to them when they fit (order 2 up
// to k = 14) and in a per-workgroup slice of global memory otherwise (order 2 up to k = 30, where n_nbrs <= 512 binds).
// Calls beyond these limits take the wide kernels (grad_wide_kernels.hpp).
constexpr int kKnnQueriesPerWave = 4, kKnnWaves = 4, kKnnQueries = kKnnQueriesPerWave * kKnnWaves;
constexpr int kKnnPitch = 80;  // LDS row pitch of knn_mfma_kernel's staged points

inline size_t knn_lds_bytes(int k, int n_nbrs) {
  return (size_t)k * 64 * 8 + (size_t)kKnnQueries * k * 8 + (size_t)kKnnQueries * n_nbrs * 12 + 64;
}
inline int knn_mfma_slices(int k) { return k <= 16 ? 4 : (k <= 32 ? 8 : 16); }
inline size_t knn_mfma_lds_bytes(int k, int n_nbrs, int waves) {
  const int k4 = (k + 3) & ~3, qt = 16 * waves, kd = 4 * knn_mfma_slices(k);
  return ((size_t)qt * k4 + qt + (size_t)kd * kKnnPitch + 64 + (size_t)qt * n_nbrs + qt) * 8 +
         ((size_t)kd * kKnnPitch + (size_t)qt * n_nbrs + 1 + qt) * 4 + 64;
}

// Rows of the packed lower triangle of grad_fit_lin_kernel (rows 0 .. P; row P = the right-hand side): row i holds columns
// 0 .. i in an even number of doubles, so every row starts on a 16-byte LDS slot; the rows are stored in a PERMUTED order
// chosen so that row i starts at a slot congruent to i modulo 16.  Lane r owns row r, and the 16 lanes a ds_read_b128 is
// serviced for together have distinct lane numbers modulo 16, so their reads of one column fall into 16 different slots of
// the 256-byte bank line: conflict-free (in index order the starts are m (m + 1) or (m + 1)^2 slots, which take 4 - 8
// residues: 4-way conflicts on every read, 12 % of the kernel's LDS cycles).  The greedy below always finds a row of the
// residue it needs while rows of every residue are left (no padding at P = 65; 2 % at P = 50).
struct FitRowTab {
  unsigned short off[68];  // start of row i in doubles
  unsigned short total;    // doubles in all
};
inline FitRowTab grad_fit_lin_row_table(int P) {
  FitRowTab t{};
  bool placed[68] = {};
  int end = 0;  // in 16-byte slots
  for (int n = 0; n <= P; ++n) {
    int pick = -1, pad = 0;
    for (pad = 0; pad < 16 && pick < 0; ++pad) {
      const int res = (end + pad) & 15;
      for (int r = P; r >= 0; --r)  // the longest unplaced row of that residue
        if (!placed[r] && (r & 15) == res) {
          pick = r;
          break;
        }
      if (pick >= 0) break;
    }
    placed[pick] = true;
    t.off[pick] = (unsigned short)(2 * (end + pad));
    end += pad + ((pick + 2) >> 1);
  }
  t.total = (unsigned short)(2 * end);
  return t;
}
inline size_t grad_fit_lin_lds_bytes(int k, int n_nbrs) {
  const int P = k + 1;
  return ((size_t)grad_fit_lin_row_table(P).total + 2 * P) * 8 + (size_t)(((n_nbrs + 15) & ~15) + 16) * 4 + 128 * 2 + 64;
}

// m_in_lds = false: the normal equations live in global memory (grad_fit_kernel's m_glob)
inline size_t grad_fit_lds_bytes(int k, int n_nbrs, int order, bool m_in_lds = true) {
  const int P = order == 1 ? k + 1 : k + k * (k + 1) / 2 + 1;
  const int LM = (P + 1) | 1;
  return ((size_t)n_nbrs * k + n_nbrs + (m_in_lds ? (size_t)P * LM : (size_t)0) + k + 2 * P) * 8 + (size_t)(2 * P + 4 + n_nbrs) * 4 + 64;
}
inline size_t grad_fit_m_elems(int k, int order) {
  const int P = order == 1 ? k + 1 : k + k * (k + 1) / 2 + 1;
  return (size_t)P * (size_t)((P + 1) | 1);
}

// ---- knn2_kernel geometry (knn2_kernels.hpp) ----
constexpr int kK2Waves = 12;            // scanning waves per workgroup = 3 per SIMD (168 VGPRs: at 4 per SIMD the query fragments spill;
                                        // 8 waves x 4 row tiles at 256 VGPRs measured 446 vs 436 ms at 1e6 points; two chunks
                                        // per ring slot and barrier 455 ms: the longer live ranges put scratch into the loop)
constexpr int kK2RowTiles = 2;          // 16-query MFMA row tiles per wave: every B fragment read from LDS serves both
                                        // (with one, the 16 waves' fragment reads -- 256 KiB per chunk and CU at 128 B/clk
                                        // -- outweighed the MFMAs)
constexpr int kK2WQ = 16 * kK2RowTiles; // queries per wave
constexpr int kK2Q = kK2WQ * kK2Waves;  // queries per workgroup tile
constexpr int kK2Cap = 256;             // candidate slots per query between flushes
constexpr int kK2List = 128;            // list entries per query (n_nbrs <= 128)
constexpr int kK2Chunk = 64;            // support points per chunk

CORRLA_HD constexpr int k2_chunk_bytes(int s) { return s * 8192; }            // s = 32-dimension MFMA steps
CORRLA_HD constexpr int k2_stage_bytes(int s) { return k2_chunk_bytes(s) + 1024; }  // + 64 x 4 f32: -c_p, replicated
// two stages + one 64-coordinate f64 row per wave (the query whose candidates are being re-checked)
constexpr int kK2Stages = 4;            // ring of staged chunks: three in flight behind the one being scanned (with one, every
                                        // chunk waited for its own DMA: 29 % of the scan at 1e6 points, CORRLA_KNN2_PROF)
CORRLA_HD constexpr int k2_lds_bytes(int s) { return kK2Stages * k2_stage_bytes(s) + kK2Waves * 512 + 1024; }

// ---- wide nearest-neighbour scan (knn_wide_kernel) ----
constexpr int kWsQ = 64;      // queries per workgroup tile
constexpr int kWsChunk = 64;  // support points per chunk
constexpr int kWsDs = 32;     // feature dimensions per LDS-staged slice
constexpr int kWsPitch = 65;  // LDS row pitch of a staged slice (doubles)
constexpr int kWsCap = 512;   // candidate slots per query between flushes (a flush when one query has > kWsCap - 64)
constexpr int kWsWaves = 4;
CORRLA_HD constexpr size_t ws_lds_bytes() {
  return (size_t)(2 * kWsDs * kWsPitch + kWsQ + kWsWaves * kWsCap) * 8 +
         (size_t)(2 * kWsQ + kWsWaves * kWsCap + kWsWaves * (kWsCap + 8) + 4) * 4 + 64;
}
// global memory per workgroup: the sorted distances of its kWsQ lists (the indices are kept in the output itself) and
// the candidate buffers
CORRLA_HD constexpr size_t ws_wg_bytes(int64_t n_nbrs) { return (size_t)kWsQ * ((size_t)n_nbrs * 8 + (size_t)kWsCap * 12); }

// ---- wide local fit (grad_fit_wide_kernel) ----
constexpr int kWfT = 64;      // tile edge of the normal equations (and Cholesky panel width)
constexpr int kWfKb = 32;     // inner-dimension chunk staged in LDS
constexpr int kWfPitch = 65;
CORRLA_HD constexpr size_t wf_lds_bytes() { return (size_t)(2 * kWfKb * kWfPitch + 2 * kWfT * kWfPitch) * 8 + (size_t)(kWfKb + 4) * 4 + 64; }
// design columns P; the workspace slice holds the augmented (P + 1) x (P + 1) normal equations [D y]^T [D y] (lower
// triangle used), the Jacobi scales and the solution
CORRLA_HD constexpr int64_t grad_design_cols(int64_t k, int order) { return order == 1 ? k + 1 : k + k * (k + 1) / 2 + 1; }
CORRLA_HD constexpr size_t wf_slice_bytes(int64_t P) { return ((size_t)(P + 1) * (size_t)(P + 1) + 2 * (size_t)(P + 1)) * 8; }

}  // namespace k

// Workspace the wide kernels may take, each: a fixed cap (MI355X has 288 GB; the limited kernels need far less)
constexpr size_t kGradWideBudgetBytes = (size_t)4 << 30;

enum class GradScan { kValu, kMfma, kKnn2, kWide };
enum class GradFit { kLin, kLds, kGlobal, kWide };
struct GradPlan {
  const char* error = nullptr;  // non-null: the call is rejected (CORRLA_EINVAL) with this message
  GradScan scan = GradScan::kValu;
  int scan_w = 0;               // kMfma: waves (4 or 2)
  int scan_nks = 0;             // kMfma: 4-dimension MFMA slices compiled in (4, 8, 16)
  int scan_s = 0;               // kKnn2: 32-dimension bf16 MFMA steps (1, 2)
  int scan_block = 0;           // threads per workgroup
  int64_t scan_wgs = 0;         // workgroups (kKnn2, kWide: persistent, each takes query tiles in turn)
  int64_t scan_tiles = 0;       // kKnn2, kWide: query tiles
  size_t scan_lds = 0;          // dynamic LDS of the scan kernel
  size_t scan_ws = 0;           // every workspace of the scan and of the kernels that prepare it, but for scale_ws
  size_t scale_ws = 0;          // kKnn2, kMfma: the block that holds the filter's power-of-two scale (zeroed before the scan)
  int64_t ldt = 0;              // limited scans: pitch of the transposed cloud (k x ldt doubles)
  int64_t pts_wgs = 0;          // limited scans: 256-thread blocks over the points (grad_transpose_kernel, point_norms_kernel)
  struct Knn2 {                 // kKnn2: the prepared cloud and the per-workgroup lists
    int64_t nchunks = 0;        //   chunks of kK2Chunk points = workgroups of knn2_prep_kernel
    int nb = 0;                 //   workgroups of knn2_colsum_kernel
    int64_t rpb = 0;            //   ... and the rows each one sums
    size_t pb = 0, pn = 0, cand = 0, list_d = 0, list_i = 0;  // bytes of Knn2Args' arrays of those names
  } k2;
  GradFit fit = GradFit::kLin;
  int fit_ntt = 0;              // kLin: 16-column tiles of the design
  size_t fit_lds = 0;
  size_t fit_ws = 0;            // kGlobal, kWide: per-workgroup slices in all
  int64_t fit_wgs = 0;          // workgroups (kLin, kLds: one per query; kGlobal, kWide: persistent)
};

// knn_mode = CORRLA_KNN (0 by size, 1 VALU, 2 f32-MFMA, 3 bf16-filter, 4 wide), fit_mode = CORRLA_FIT (0 default, 1 the
// general kernel for order 1 too, 2 wide).  budget = bytes the workspace of each wide kernel may take.
// knn2_wgs_per_cu = CORRLA_KNN2_WGS_PER_CU: persistent workgroups of knn2_kernel per CU (at least 1).
inline GradPlan grad_plan(int64_t n_pts, int64_t kf, int64_t n_q, int order, int64_t n_nbrs, int knn_mode, int fit_mode,
                          int num_cus, size_t budget, int knn2_wgs_per_cu = 1) {
  GradPlan p;
  auto reject = [&](const char* m) {
    p.error = m;
    return p;
  };
  const size_t kMax = k::kLdsMaxBytes;
  if (n_pts < 1 || n_q < 1 || kf < 1) return reject("empty point set");
  if (order != 1 && order != 2) return reject("est_order must be 1 or 2 (the reference panics otherwise)");
  const int64_t need_pts = order == 1 ? kf + 1 : kf * (kf + 3) / 2;  // active_subspaces.rs:118-119, 129-130
  if (!(n_pts > need_pts && n_nbrs > need_pts))
    return reject("n_pts and n_nbrs must exceed k + 1 (order 1) / k (k + 3) / 2 (order 2)");
  if (n_nbrs > n_pts) return reject("n_nbrs exceeds the number of support points");
  if (n_pts > 0x7fffffff || n_q * n_nbrs > ((int64_t)1 << 40)) return reject("point set too large");
  if (n_q > 0x7fffffff) return reject("too many query points for one launch");
  const bool small = kf <= k::kGradMaxDim && n_nbrs <= k::kGradMaxNbr;  // every limited scan's list fits
  const int kk = (int)(small ? kf : 0), nn = (int)(small ? n_nbrs : 0);
  const bool limited_fit = small && k::grad_fit_lds_bytes(kk, nn, order, /*m_in_lds=*/false) <= kMax;
  auto ceil_div = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
  // ---- scan ----
  if (knn_mode == 4 || !small) {
    p.scan = GradScan::kWide;
    p.scan_block = 64 * k::kWsWaves;
    p.scan_lds = k::ws_lds_bytes();
    const size_t per_wg = k::ws_wg_bytes(n_nbrs);
    if (per_wg > budget) return reject("the wide scan's lists of one workgroup exceed the 4 GiB workspace budget");
    p.scan_tiles = ceil_div(n_q, k::kWsQ);
    int64_t wgs = p.scan_tiles < 2 * (int64_t)num_cus ? p.scan_tiles : 2 * (int64_t)num_cus;
    if ((size_t)wgs * per_wg > budget) wgs = (int64_t)(budget / per_wg);
    p.scan_wgs = wgs;
    p.scan_ws = (size_t)wgs * per_wg;
  } else {
    // every limited scan is launched behind the transposed cloud (the bf16 scan does not read it)
    p.ldt = ceil_div(n_pts, 64) * 64;
    p.pts_wgs = ceil_div(n_pts, 256);
    p.scan_ws = (size_t)p.ldt * kk * sizeof(double);
    if ((knn_mode == 3 || (knn_mode == 0 && n_pts >= 8192)) && nn <= k::kK2List) {
      // small clouds keep the VALU scan: its lists live in LDS and there is too little work to amortise the split of the cloud
      p.scan = GradScan::kKnn2;
      p.scan_s = kk <= 32 ? 1 : 2;
      p.scan_block = 64 * k::kK2Waves;
      p.scan_lds = (size_t)k::k2_lds_bytes(p.scan_s);
      p.scan_tiles = ceil_div(n_q, k::kK2Q);
      const int64_t cap = (int64_t)num_cus * (knn2_wgs_per_cu > 1 ? knn2_wgs_per_cu : 1);
      p.scan_wgs = p.scan_tiles < cap ? p.scan_tiles : cap;
      GradPlan::Knn2& g = p.k2;
      g.nchunks = ceil_div(n_pts, k::kK2Chunk);
      const int64_t nb = ceil_div(n_pts, 4096);
      g.nb = (int)(nb < 1024 ? nb : 1024);
      g.rpb = ceil_div(n_pts, g.nb);
      g.pb = (size_t)g.nchunks * (size_t)k::k2_chunk_bytes(p.scan_s);
      g.pn = (size_t)g.nchunks * k::kK2Chunk * 4 * sizeof(float);  // -c_p, four copies per point
      const size_t lists = (size_t)p.scan_wgs * k::kK2Q;
      g.cand = lists * k::kK2Cap * sizeof(int);
      g.list_d = lists * k::kK2List * sizeof(double);
      g.list_i = lists * k::kK2List * sizeof(int);
      // + the column sums of the g.nb blocks and the mean, 64 doubles each
      p.scan_ws += g.pb + g.pn + (size_t)(g.nb + 1) * 64 * sizeof(double) + g.cand + g.list_d + g.list_i;
      p.scale_ws = 64 * sizeof(double);
    } else if (knn_mode == 1 || (knn_mode == 0 && n_pts < 131072) || k::knn_mfma_lds_bytes(kk, nn, 2) > kMax) {
      // (also when the MFMA scan's per-query lists outgrow LDS: n_nbrs > ~400 at k = 64)
      p.scan = GradScan::kValu;
      p.scan_block = 64 * k::kKnnWaves;
      p.scan_lds = k::knn_lds_bytes(kk, nn);
      p.scan_wgs = ceil_div(n_q, k::kKnnQueries);
    } else {
      // Both spend ~n_nbrs ln(n_pts / n_nbrs) list insertions per query; the MFMA distance tile only pays off once the scan
      // itself dominates (measured: 5e4 points 0.10 s VALU / 0.14 s MFMA, 1e5 0.28 / 0.30, 2e5 0.93 / 0.45)
      p.scan = GradScan::kMfma;
      p.scan_w = k::knn_mfma_lds_bytes(kk, nn, 4) <= kMax ? 4 : 2;
      p.scan_nks = k::knn_mfma_slices(kk);
      p.scan_block = 64 * p.scan_w;
      p.scan_lds = k::knn_mfma_lds_bytes(kk, nn, p.scan_w);
      p.scan_wgs = ceil_div(n_q, 16 * p.scan_w);
      p.scan_ws += (size_t)n_pts * sizeof(double);  // the points' squared norms
      p.scale_ws = sizeof(double);                  // the largest of them
    }
  }
  // ---- fit ----
  if (fit_mode == 2 || !limited_fit) {
    p.fit = GradFit::kWide;
    p.fit_lds = k::wf_lds_bytes();
    const size_t slice = k::wf_slice_bytes(k::grad_design_cols(kf, order));
    if (kf > 0x3fffffff || slice > budget)
      return reject("the normal equations of one query exceed the wide fit's 4 GiB workspace budget");
    int64_t wgs = n_q < (int64_t)num_cus ? n_q : (int64_t)num_cus;
    if ((size_t)wgs * slice > budget) wgs = (int64_t)(budget / slice);
    p.fit_wgs = wgs;
    p.fit_ws = (size_t)wgs * slice;
  } else if (order == 1 && fit_mode != 1) {
    p.fit = GradFit::kLin;  // order 1: the MFMA-built normal equations (CORRLA_FIT=1 keeps the general kernel)
    const int ntt = (kk + 2 + 15) / 16;
    p.fit_ntt = ntt < 5 ? ntt : 5;
    p.fit_lds = k::grad_fit_lin_lds_bytes(kk, nn);
    p.fit_wgs = n_q;
  } else if (k::grad_fit_lds_bytes(kk, nn, order, true) <= kMax) {
    p.fit = GradFit::kLds;
    p.fit_lds = k::grad_fit_lds_bytes(kk, nn, order, true);
    p.fit_wgs = n_q;
  } else {
    p.fit = GradFit::kGlobal;
    p.fit_lds = k::grad_fit_lds_bytes(kk, nn, order, false);
    p.fit_wgs = n_q < 2 * (int64_t)num_cus ? n_q : 2 * (int64_t)num_cus;
    p.fit_ws = (size_t)p.fit_wgs * k::grad_fit_m_elems(kk, order) * sizeof(double);
  }
  return p;
}

}  // namespace corrla
