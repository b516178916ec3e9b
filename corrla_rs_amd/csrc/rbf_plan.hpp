// The plan of the kernel-matrix kernels behind corrla_rbf_apply_* and corrla_rbf_matrix_* (rbf_kernels.hpp, rbf_stage.hpp):
//   APPLY   out = Phi(Xq, Xs) W_rbf + P(Xq) W_poly, Phi_ij = phi(||xq_i - xs_j||_2) formed tile by tile in registers and never
//           stored: the tile of queries a workgroup owns (BM), the group of right-hand-side columns it serves (RG), the
//           chunks the supports are staged in (KC), the contiguous ranges the supports are split into when the queries alone
//           do not fill the device, the grid, the dynamic LDS, the workspace of the split partials with its bound, and the
//           finishing launch that adds the partials and the polynomial tail.
//   MATRIX  out = Phi(Xq, Xs) itself: BM queries x MN supports per workgroup, no workspace, no finishing launch.
// Host code only, no HIP call: tests/test_rbf_plan.py compiles this header with the host compiler and pins the plan.  The
// kernels take the tile sizes from it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "core_svd_plan.hpp"  // kLdsMaxBytes, CORRLA_HD

namespace corrla {
namespace k {

constexpr int kRbfBM = 64;        // queries per workgroup: one 16-row MFMA tile per wave
constexpr int kRbfKC = 32;        // support points per staged chunk: 4 reduction slots of an MFMA x 8 supports each
constexpr int kRbfRG = 64;        // right-hand-side columns per pass: four 16-wide MFMA column tiles
// row stride of the staged W: the reduction slots of an MFMA step read rows KC / 4 apart, which this stride puts half the
// banks apart for both element sizes (8 * 66 * esz = 128 mod 256 bytes in f64, 64 mod 128 in f32)
constexpr int kRbfWLd = kRbfRG + 2;
constexpr int kRbfMN = 64;        // MATRIX: supports per workgroup
constexpr int kRbfMaxDim = 128;
constexpr int kRbfThreads = 256;  // four waves; every wave stages as well
// The LDS images of one chunk: the query tile and the chunk's supports, coordinate-major, and KC rows of W.  At the
// largest dim (128) in f64 that is 64 KiB + 32 KiB + 16.5 KiB = 112.5 KiB of the 160; at dim 3 it is 18.75 KiB.
CORRLA_HD constexpr int rbf_apply_lds_bytes(int dim, int esz) { return (dim * (kRbfBM + kRbfKC) + kRbfKC * kRbfWLd) * esz; }
// MATRIX: the two coordinate images, 128 KiB at dim 128 in f64
CORRLA_HD constexpr int rbf_matrix_lds_bytes(int dim, int esz) { return dim * (kRbfBM + kRbfMN) * esz; }
// workgroups the splits aim at: four per CU of the 256
constexpr int64_t kRbfTargetWgs = 4 * 256;

}  // namespace k

enum class RbfMode : int { kApply = 0, kMatrix = 1 };

struct RbfShape {
  int64_t n_q = 0, n_s = 0, dim = 0;
  int64_t n_rhs = 1;   // APPLY: columns of the coefficients (MATRIX: ignored)
  int64_t n_poly = 0;  // APPLY: rows of W_poly, rbf_poly_terms(dim, degree)
  int esz = 8;
  RbfMode mode = RbfMode::kApply;
};

struct RbfPlan {
  bool ok = false;
  const char* error = nullptr;
  int bm = k::kRbfBM, kc = k::kRbfKC, rg = k::kRbfRG;
  int64_t nbm = 0;        // query tiles: tile b covers the queries [b bm, min(n_q, (b + 1) bm))
  int64_t nrg = 0;        // APPLY: column groups of rg; MATRIX: support tiles of kRbfMN.  A column group beyond the first
                          // RECOMPUTES phi for its queries and supports: phi is cheap next to a second pass over W only
                          // while n_rhs stays a small multiple of rg
  int64_t nchunks = 0;    // APPLY: chunks of kc supports in all
  int64_t nsplit = 1;     // APPLY: split s covers the supports [s split_len, min(n_s, (s + 1) split_len)), none empty
  int64_t split_len = 0;  // a multiple of kc
  unsigned grid_x = 0, block = k::kRbfThreads;  // APPLY: workgroup w owns (tile w % nbm, group (w / nbm) % nrg, split w / (nbm nrg))
                                                // MATRIX: (query tile w / nrg, support tile w % nrg)
  size_t lds_bytes = 0;
  size_t ws_bytes = 0;    // APPLY: the partials [nsplit][n_q][n_rhs]
  size_t ws_bound = 0;    // the stated upper bound of ws_bytes for this shape
  unsigned finish_grid_x = 0, finish_block = 256;  // APPLY: one thread per (query, column), always launched
};

// Rows of W_poly (build_full_vandermonde, stats_corr.rs:183-209): none for degree < 0, [x, 1] for degree 0 or 1,
// [x, x_a x_b (a <= b, a outer), 1] from degree 2 on.
CORRLA_HD constexpr int64_t rbf_poly_terms(int64_t dim, int degree) {
  return degree < 0 ? 0 : (degree < 2 ? dim + 1 : dim + dim * (dim + 1) / 2 + 1);
}

// Upper bound of the partials: the size of the result while there is one split; with more, nbm nrg < target and
// nsplit <= 2 (target / (nbm nrg) + 1) (whole chunks per split, rounded down), so nsplit n_q n_rhs
// <= 2 (target + nbm nrg) bm rg < 4 target bm rg elements (128 MiB in f64).
inline size_t rbf_ws_bound(int64_t n_q, int64_t n_rhs, int esz) {
  return std::max((size_t)n_q * (size_t)n_rhs, (size_t)(4 * k::kRbfTargetWgs) * k::kRbfBM * k::kRbfRG) * (size_t)esz;
}

inline RbfPlan rbf_plan(const RbfShape& s) {
  RbfPlan p;
  auto reject = [&](const char* why) {
    p.ok = false;
    p.error = why;
    return p;
  };
  if (s.esz != 4 && s.esz != 8) return reject("rbf: element size (esz) must be 4 or 8");
  if (s.n_q < 1) return reject("rbf: n_q must be >= 1");
  if (s.n_s < 1) return reject("rbf: n_s must be >= 1");
  if (s.dim < 1 || s.dim > k::kRbfMaxDim) return reject("rbf: dim must be in [1, 128]");
  p.nbm = (s.n_q + p.bm - 1) / p.bm;
  if (s.mode == RbfMode::kMatrix) {
    p.nrg = (s.n_s + k::kRbfMN - 1) / k::kRbfMN;
    if (p.nbm > 0x7fffffff / p.nrg) return reject("rbf: n_q x n_s gives more than 2^31 - 1 tiles");
    p.grid_x = (unsigned)(p.nbm * p.nrg);
    p.lds_bytes = (size_t)k::rbf_matrix_lds_bytes((int)s.dim, s.esz);
    p.ok = true;
    return p;
  }
  if (s.n_rhs < 1) return reject("rbf: n_rhs must be >= 1");
  if (s.n_poly < 0) return reject("rbf: n_poly must be >= 0");
  p.nrg = (s.n_rhs + p.rg - 1) / p.rg;
  p.nchunks = (s.n_s + p.kc - 1) / p.kc;
  if (p.nbm > 0x7fffffff / p.nrg) return reject("rbf: n_q x n_rhs gives more than 2^31 - 1 tiles");
  const int64_t tiles = p.nbm * p.nrg;
  // from the shape alone: enough splits to reach the target (whole chunks per split, rounded down, so that the target is
  // reached and not only approached), never more than there are chunks, none empty
  const int64_t want = std::min(p.nchunks, (k::kRbfTargetWgs + tiles - 1) / tiles);
  const int64_t chunks_per_split = p.nchunks / want;
  p.nsplit = (p.nchunks + chunks_per_split - 1) / chunks_per_split;
  p.split_len = chunks_per_split * p.kc;
  if (tiles > 0x7fffffff / p.nsplit) return reject("rbf: n_q x n_rhs x splits gives more than 2^31 - 1 workgroups");
  p.grid_x = (unsigned)(tiles * p.nsplit);
  p.lds_bytes = (size_t)k::rbf_apply_lds_bytes((int)s.dim, s.esz);
  p.ws_bytes = (size_t)p.nsplit * (size_t)s.n_q * (size_t)s.n_rhs * (size_t)s.esz;
  p.ws_bound = rbf_ws_bound(s.n_q, s.n_rhs, s.esz);
  const int64_t outs = s.n_q * s.n_rhs;
  if ((outs + p.finish_block - 1) / p.finish_block > 0x7fffffff) return reject("rbf: n_q x n_rhs gives more than 2^31 - 1 finishing workgroups");
  p.finish_grid_x = (unsigned)((outs + p.finish_block - 1) / p.finish_block);
  p.ok = true;
  return p;
}

}  // namespace corrla
