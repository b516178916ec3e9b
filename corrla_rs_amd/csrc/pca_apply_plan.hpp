// The plan of the PCA back-projection kernel behind corrla_pca_inverse_* and the Q-residuals of corrla_pca_transform_*
// (pca_apply_kernels.hpp, pca_apply_stage.hpp): the tile of the m x n plane a workgroup owns (BM rows, BN columns), the
// chunks the reduction over k is walked in (KC, sized to LDS), the grid, the dynamic LDS, the workspace of the per-tile row
// partials with its bound, the finishing launch, and the route -- the m x n operand (the output of STORE, x of RESID)
// touched in place with 16-byte accesses, in place with checked element accesses, or (RESID only) read from a repacked copy.
// Host code only, no HIP call: tests/test_pca_apply_plan.py compiles this header with the host compiler and pins the plan.
// The kernels take the tile sizes from it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "core_svd_plan.hpp"  // kLdsMaxBytes, CORRLA_HD

namespace corrla {
namespace k {

constexpr int kPcaBackBM = 64;        // rows of the m x n plane per workgroup
constexpr int kPcaBackBN = 128;       // columns per workgroup: 2 x 2 waves of 32 x 64 each
constexpr int kPcaBackThreads = 256;  // four MFMA waves; every wave stages as well
// reduction indices per staged chunk: one image of KC x (BM + BN) elements is 24 KiB for both types
CORRLA_HD constexpr int pca_back_kc(int esz) { return 128 / esz; }
CORRLA_HD constexpr int pca_back_lds_bytes(int esz) { return pca_back_kc(esz) * (kPcaBackBM + kPcaBackBN) * esz; }

}  // namespace k

enum class PcaApplyRoute : int {
  kReject = 0,
  kInPlace = 1,         // the m x n operand touched where it lies, 16-byte accesses
  kInPlaceChecked = 2,  // ... element accesses (base or row stride not 16-byte aligned)
  kRepacked = 3         // RESID: x is feature-strided; one transposing copy into workspace, then the aligned kernel on it
};

enum class PcaApplyMode : int { kStore = 0, kResid = 1 };

struct PcaApplyShape {
  int64_t m = 0, n = 0, k = 0;             // samples x features, components
  int64_t row_stride = 0, col_stride = 1;  // of the m x n operand (out of STORE: col_stride 1), in elements
  int esz = 4;
  bool base_aligned = true;                // its base pointer is 16-byte aligned
  PcaApplyMode mode = PcaApplyMode::kStore;
};

constexpr size_t kPcaApplyRepackMaxBytes = (size_t)48 << 30;  // the repacked copy, not more than this

struct PcaApplyPlan {
  PcaApplyRoute route = PcaApplyRoute::kReject;
  const char* error = nullptr;
  int bm = k::kPcaBackBM, bn = k::kPcaBackBN, kc = 0;
  int64_t nbm = 0, nbn = 0;  // row tiles, column tiles; tile (bi, bj) covers rows [bi bm, min(m, (bi + 1) bm)) x the same in n
  int64_t nchunks = 0;       // chunk c covers the components [c kc, min(k, (c + 1) kc)); a chunk is zero-padded in LDS to a multiple of 4
  unsigned grid_x = 0, block = k::kPcaBackThreads;  // workgroup w owns tile (w / nbn, w % nbn)
  size_t lds_bytes = 0;
  int wide = 0;              // 16-byte accesses of the m x n operand are legal
  int64_t ld = 0;            // the row stride the kernel uses (of the operand in place, or of the repacked copy)
  size_t repack_bytes = 0;   // 0 unless kRepacked
  size_t ws_bytes = 0;       // RESID: nbn row partials of m elements; 0 for STORE
  size_t ws_bound = 0;       // the stated upper bound of ws_bytes for this shape
  unsigned finish_grid_x = 0, finish_block = 256;  // RESID: one thread per row
};

// Upper bound of the row-partial workspace: one value per row and started column tile.
inline size_t pca_apply_ws_bound(int64_t m, int64_t n, int esz) {
  return (size_t)m * (size_t)(n / k::kPcaBackBN + 1) * (size_t)esz;
}

inline PcaApplyPlan pca_apply_plan(const PcaApplyShape& s) {
  PcaApplyPlan p;
  auto reject = [&](const char* why) {
    p.route = PcaApplyRoute::kReject;
    p.error = why;
    return p;
  };
  if (s.esz != 4 && s.esz != 8) return reject("pca apply: element size must be 4 or 8");
  if (s.m < 1 || s.n < 1) return reject("pca apply: empty matrix");
  if (s.k < 1) return reject("pca apply: k must be >= 1");
  if (s.row_stride < 0 || s.col_stride < 0) return reject("pca apply: negative strides are not supported");
  const int64_t vec = 16 / s.esz;
  p.kc = k::pca_back_kc(s.esz);
  p.nbm = (s.m + p.bm - 1) / p.bm;
  p.nbn = (s.n + p.bn - 1) / p.bn;
  p.nchunks = (s.k + p.kc - 1) / p.kc;
  if (p.nbm > 0x7fffffff / p.nbn) return reject("pca apply: more than 2^31 - 1 tiles");
  const bool unit_cols = (s.col_stride == 1 || s.n == 1) && (s.row_stride >= s.n || s.m == 1);
  if (unit_cols) {
    p.ld = s.m == 1 ? std::max<int64_t>(s.row_stride, s.n) : s.row_stride;
    p.route = (s.base_aligned && p.ld % vec == 0) ? PcaApplyRoute::kInPlace : PcaApplyRoute::kInPlaceChecked;
  } else {
    if (s.mode == PcaApplyMode::kStore) return reject("pca apply: the output must have unit stride along the features");
    if (s.n > 1 && s.col_stride == 0) return reject("pca apply: zero feature stride");
    if (s.m > 1 && s.row_stride == 0) return reject("pca apply: zero sample stride");
    p.route = PcaApplyRoute::kRepacked;
    p.ld = (s.n + 63) / 64 * 64;
    p.repack_bytes = (size_t)s.m * (size_t)p.ld * (size_t)s.esz;
    if (p.repack_bytes > kPcaApplyRepackMaxBytes) return reject("pca apply: feature-strided x too large to repack");
  }
  p.wide = p.route == PcaApplyRoute::kInPlaceChecked ? 0 : 1;
  p.grid_x = (unsigned)(p.nbm * p.nbn);
  p.lds_bytes = (size_t)k::pca_back_lds_bytes(s.esz);
  if (s.mode == PcaApplyMode::kResid) {
    p.ws_bytes = (size_t)p.nbn * (size_t)s.m * (size_t)s.esz;
    p.finish_grid_x = (unsigned)((s.m + p.finish_block - 1) / p.finish_block);
  }
  p.ws_bound = s.mode == PcaApplyMode::kResid ? pca_apply_ws_bound(s.m, s.n, s.esz) : 0;
  return p;
}

}  // namespace corrla
