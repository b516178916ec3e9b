// The plan of the symmetric rank-k product behind corrla_cov_* (syrk_kernels.hpp, launched by cov_stage::syrk): the column tile width and
// the list of tile pairs (bi <= bj), the row split into slabs, the grid, the dynamic LDS, the workspace of the per-slab
// partial tiles with its bound, the finishing launch, and the route -- X in place, X in place through the checked staging
// path, a repacked copy, or a rejection with its reason.
// Host code only, no HIP call: tests/test_syrk_plan.py compiles this header with the host compiler and pins the plan.  The
// kernels take the tile sizes and the pair enumeration from it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "core_svd_plan.hpp"  // kLdsMaxBytes, CORRLA_HD

namespace corrla {
namespace k {

constexpr int kSyrkBT = 128;       // columns of X per tile: a workgroup owns one 128 x 128 tile of the result
constexpr int kSyrkThreads = 256;  // four MFMA waves, each 64 x 64 of the tile; every wave stages as well
// reduction rows per staged tile: one image of KT rows x 128 columns is 16 KiB for both types
CORRLA_HD constexpr int syrk_kt(int esz) { return 16 * 1024 / (kSyrkBT * esz); }
// one image per operand (a diagonal pair stages one and reads it twice; the size does not depend on it)
CORRLA_HD constexpr int syrk_lds_bytes(int esz) { return 2 * syrk_kt(esz) * kSyrkBT * esz; }

// Pair p of the enumeration: column bj of the upper triangle holds bi = 0 .. bj, p = bj (bj + 1) / 2 + bi.  Neighbouring
// workgroups share the J tile.
CORRLA_HD inline void syrk_pair(int64_t p, int* bi, int* bj) {
  int j = 0;
  while (p >= j + 1) {
    p -= j + 1;
    ++j;
  }
  *bi = (int)p;
  *bj = j;
}

}  // namespace k

enum class SyrkRoute : int {
  kReject = 0,
  kInPlace = 1,         // X read where it lies, 16-byte loads
  kInPlaceChecked = 2,  // X read where it lies, element loads with bounds checks (base or ld not 16-byte aligned)
  kRepacked = 3         // features are strided: one transposing copy into workspace, then the aligned kernel on it
};

// Knobs, read once when a device context is created (hip_backend.hpp).
struct SyrkKnobs {
  int64_t slab_rows = 0;  // CORRLA_SYRK_SLAB_ROWS: rows per slab (rounded up to the tile depth; 0: by shape)
};

struct SyrkShape {
  int64_t m = 0, n = 0;              // samples x features
  int64_t row_stride = 0, col_stride = 0;  // of the caller's X, in elements
  int esz = 4;
  bool base_aligned = true;          // the caller's base pointer is 16-byte aligned
  int num_cus = 256;
};

constexpr size_t kSyrkRepackMaxBytes = (size_t)48 << 30;  // the repacked copy, not more than this

struct SyrkPlan {
  SyrkRoute route = SyrkRoute::kReject;
  const char* error = nullptr;
  int bt = k::kSyrkBT, kt = 0;
  int nb = 0;            // column tiles
  int64_t npairs = 0;    // nb (nb + 1) / 2
  int64_t ktiles = 0;    // tiles of kt rows over [0, m)
  int64_t nsplit = 1;    // slabs
  int64_t slab_rows = 0; // rows per slab, a multiple of kt; slab s covers [s * slab_rows, min(m, (s + 1) * slab_rows))
  unsigned grid_x = 0, grid_y = 0, block = k::kSyrkThreads;  // (pair, slab)
  size_t lds_bytes = 0;
  int64_t ld = 0;        // leading dimension the kernel reads with (of X in place, or of the repacked copy)
  size_t repack_bytes = 0;       // 0 unless kRepacked
  size_t ws_bytes = 0;           // nsplit * npairs partial tiles of bt * bt elements
  size_t ws_bound = 0;           // the stated upper bound of ws_bytes for this shape
  unsigned finish_grid_x = 0, finish_grid_y = 0, finish_block = 256;  // (pair, 32 x 32 sub-tile of the 128 x 128 tile)
};

// Upper bound of the partial-tile workspace: the pairs alone once (nsplit == 1), or, where the rows are split to fill the
// chip, at most 4 * num_cus + npairs tiles.
inline size_t syrk_ws_bound(int64_t npairs, int esz, int num_cus) {
  return (size_t)(npairs + 4 * (int64_t)num_cus) * k::kSyrkBT * k::kSyrkBT * (size_t)esz;
}

inline SyrkPlan syrk_plan(const SyrkShape& s, const SyrkKnobs& kn) {
  SyrkPlan p;
  auto reject = [&](const char* why) {
    p.route = SyrkRoute::kReject;
    p.error = why;
    return p;
  };
  if (s.esz != 4 && s.esz != 8) return reject("cov: element size must be 4 or 8");
  if (s.m < 1 || s.n < 1) return reject("cov: empty matrix");
  if (s.row_stride < 0 || s.col_stride < 0) return reject("cov: negative strides are not supported");
  const int64_t vec = 16 / s.esz;
  p.kt = k::syrk_kt(s.esz);
  p.nb = (int)((s.n + p.bt - 1) / p.bt);
  if (p.nb > 32767) return reject("cov: more than 32767 column tiles");
  p.npairs = (int64_t)p.nb * (p.nb + 1) / 2;
  // route: unit stride along the features reads in place; anything else is repacked once
  const bool unit_cols = s.col_stride == 1 && (s.row_stride >= s.n || s.m == 1);
  if (s.n == 1 && s.col_stride != 1 && s.row_stride >= 1) {
    // a single feature has no feature stride to speak of: rows are row_stride apart
    p.route = (s.base_aligned && s.row_stride % vec == 0) ? SyrkRoute::kInPlace : SyrkRoute::kInPlaceChecked;
    p.ld = s.row_stride;
  } else if (unit_cols) {
    p.ld = s.m == 1 ? std::max<int64_t>(s.row_stride, s.n) : s.row_stride;
    p.route = (s.base_aligned && p.ld % vec == 0) ? SyrkRoute::kInPlace : SyrkRoute::kInPlaceChecked;
  } else {
    if (s.n > 1 && s.col_stride == 0) return reject("cov: zero feature stride");
    if (s.m > 1 && s.row_stride == 0) return reject("cov: zero sample stride");
    p.route = SyrkRoute::kRepacked;
    p.ld = (s.n + 63) / 64 * 64;
    p.repack_bytes = (size_t)s.m * (size_t)p.ld * (size_t)s.esz;
    if (p.repack_bytes > kSyrkRepackMaxBytes) return reject("cov: feature-strided X too large to repack");
  }
  // row split: the pairs alone fill the chip when there are a few waves of them; else the slabs carry the parallelism
  p.ktiles = (s.m + p.kt - 1) / p.kt;
  int64_t tps;  // tiles per slab
  if (kn.slab_rows > 0) {
    tps = (kn.slab_rows + p.kt - 1) / p.kt;
  } else if (p.npairs >= 2 * (int64_t)s.num_cus) {
    tps = p.ktiles;
  } else {
    const int64_t want = (4 * (int64_t)s.num_cus + p.npairs - 1) / p.npairs;  // slabs that give ~4 workgroups per CU
    tps = std::max<int64_t>((p.ktiles + want - 1) / want, 8);                 // ... of at least 8 tiles each
  }
  tps = std::max<int64_t>(1, std::min(tps, p.ktiles));
  p.nsplit = (p.ktiles + tps - 1) / tps;
  if (p.nsplit > 65535) {
    tps = (p.ktiles + 65534) / 65535;
    p.nsplit = (p.ktiles + tps - 1) / tps;
  }
  p.slab_rows = tps * p.kt;
  p.grid_x = (unsigned)p.npairs;
  p.grid_y = (unsigned)p.nsplit;
  p.lds_bytes = (size_t)k::syrk_lds_bytes(s.esz);
  p.ws_bytes = (size_t)p.nsplit * (size_t)p.npairs * p.bt * p.bt * (size_t)s.esz;
  p.ws_bound = kn.slab_rows > 0 ? p.ws_bytes : syrk_ws_bound(p.npairs, s.esz, s.num_cus);
  p.finish_grid_x = (unsigned)p.npairs;
  p.finish_grid_y = (unsigned)((p.bt / 32) * (p.bt / 32));
  return p;
}

}  // namespace corrla
