// Dense Cholesky A = L L^T and the triangular solves with L and L^T on the device (f64, row-major; the geometry is
// chol_plan.hpp's).  Only the lower triangle (i >= j) of A is ever loaded or stored: the strict upper triangle may hold
// anything.
//
// The pivot of column j is a_jj - sum_k l_jk^2 as the right-looking updates leave it; l_jj is its square root and the column
// below it is DIVIDED by l_jj (sqrt and the quotient correctly rounded: one rounding each, as the error bounds assume -- this
// file must not be compiled with approximate-math options).  A pivot that is <= 0 or not finite is recorded (the first such
// column wins) and stops nothing: the square root and the quotients go on with whatever they give, later panels run on those
// values, and the columns before the failed one are final.  No atomics and no workgroup waits on another: every reduction runs
// in a fixed order, dependencies between workgroups are separate launches on one stream, every loop is bounded by the shape.
//
//   chol_small_kernel    n <= kCholSmallN: the whole factorisation by one workgroup in LDS, and the status record
//   chol_diag_kernel     one workgroup: the kCholNB x kCholNB diagonal block of a panel in LDS, and the panel's record
//   chol_panel_kernel    L21 = A21 L11^-T: one wave per chunk of kCholChunk rows, L11 and the rows in LDS, one row per lane
//   chol_update_kernel   A22 -= L21 L21^T over the lower-triangle tile pairs on v_mfma_f64_16x16x4_f64 (MT<double>): both
//                        operands are row chunks of L21 (a diagonal tile stages one), K <= kCholNB in one LDS stage, edge
//                        tiles in-kernel
//   chol_finish_kernel   the panel records reduced to the status record, in a fixed order
//   chol_tri_kernel      X = L^-1 X or L^-T X for one kCholNB block: L and the tile of X in LDS, one column per lane
//   chol_gemm_kernel     C -= L X or C -= L^T X on the same MFMA, K <= kCholNB in one LDS stage, edge tiles in-kernel
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "chol_plan.hpp"
#include "hip_kernels.hpp"  // MT<double>

namespace corrla {
namespace k {

__device__ __forceinline__ bool chol_pivot_ok(double p) { return p > 0.0 && p < __builtin_inf(); }

// op over the kCholThreads values, in a fixed tree, to every thread; sv: kCholThreads entries
template <class Op>
__device__ __forceinline__ double chol_block_reduce(double v, double* sv, int tid, Op op) {
  sv[tid] = v;
  __syncthreads();
  for (int s = kCholThreads / 2; s > 0; s >>= 1) {
    if (tid < s) sv[tid] = op(sv[tid], sv[tid + s]);
    __syncthreads();
  }
  const double r = sv[0];
  __syncthreads();
  return r;
}

// The lower triangle of the n x n LDS image A (row stride LD), right-looking, by the whole workgroup.  Uniform results: info
// (0, or the 1-based local column of the first failed pivot) and the smallest / largest l_jj of the columns before it.
template <int LD>
__device__ __forceinline__ void chol_factor_lds(double* A, int n, int tid, int& info, double& mind, double& maxd) {
  info = 0;
  mind = __builtin_inf();
  maxd = 0.0;
  for (int j = 0; j < n; ++j) {
    const double piv = A[j * LD + j];
    if (!chol_pivot_ok(piv) && info == 0) info = j + 1;
    const double d = __builtin_sqrt(piv);
    if (info == 0) {
      mind = fmin(mind, d);
      maxd = fmax(maxd, d);
    }
    __syncthreads();  // every thread holds the pivot
    if (tid == 0) A[j * LD + j] = d;
    for (int r = j + 1 + tid; r < n; r += kCholThreads) A[r * LD + j] = A[r * LD + j] / d;
    __syncthreads();
    const int w = n - j - 1;
    for (int e = tid; e < w * w; e += kCholThreads) {
      const int r = j + 1 + e / w, c = j + 1 + e % w;
      if (c <= r) A[r * LD + c] = __builtin_fma(-A[r * LD + j], A[c * LD + j], A[r * LD + c]);
    }
    __syncthreads();
  }
}

// sum_j log l_jj of the factored image, fixed order (n <= kCholThreads)
template <int LD>
__device__ __forceinline__ double chol_log_sum(const double* A, int n, double* sv, int tid) {
  const double v = tid < n ? log(A[tid * LD + tid]) : 0.0;
  return chol_block_reduce(v, sv, tid, [](double x, double y) { return x + y; });
}

// ---- SMALL ------------------------------------------------------------------------------------------------------------------
struct CholSmallArgs {
  double* a;  // n x n, row stride lda: L over the lower triangle on return
  int64_t lda;
  int n;      // <= kCholSmallN
  CholFactorStatus* st;
};

__global__ __launch_bounds__(kCholThreads) void chol_small_kernel(CholSmallArgs g) {
  constexpr int LD = kCholSmallLd;
  extern __shared__ uint4 chol_smem[];
  double* A = reinterpret_cast<double*>(chol_smem);  // [n][LD]
  double* sv = A + kCholSmallN * LD;
  const int tid = (int)threadIdx.x, n = g.n;
  for (int e = tid; e < n * n; e += kCholThreads) {
    const int r = e / n, c = e - r * n;
    if (c <= r) A[r * LD + c] = g.a[(int64_t)r * g.lda + c];
  }
  __syncthreads();
  int info;
  double mind, maxd;
  chol_factor_lds<LD>(A, n, tid, info, mind, maxd);
  for (int e = tid; e < n * n; e += kCholThreads) {
    const int r = e / n, c = e - r * n;
    if (c <= r) g.a[(int64_t)r * g.lda + c] = A[r * LD + c];
  }
  const double ls = chol_log_sum<LD>(A, n, sv, tid);
  if (tid == 0) {
    g.st->info = info;
    g.st->min_diag = mind;
    g.st->max_diag = maxd;
    g.st->logdet = info ? 0.0 : 2.0 * ls;
  }
}

// ---- BLOCKED: the diagonal block ---------------------------------------------------------------------------------------------
struct CholDiagArgs {
  double* a;  // the whole matrix
  int64_t lda;
  int64_t j0;  // the block is rows and columns [j0, j0 + kv)
  int kv;      // 1 .. kCholNB
  CholPanelRecord* rec;  // this panel's record
};

__global__ __launch_bounds__(kCholThreads) void chol_diag_kernel(CholDiagArgs g) {
  constexpr int LD = kCholDiagLd;
  __shared__ double A[kCholNB * LD];
  __shared__ double sv[kCholThreads];
  const int tid = (int)threadIdx.x, n = g.kv;
  double* blk = g.a + g.j0 * g.lda + g.j0;
  for (int e = tid; e < n * n; e += kCholThreads) {
    const int r = e / n, c = e - r * n;
    if (c <= r) A[r * LD + c] = blk[(int64_t)r * g.lda + c];
  }
  __syncthreads();
  int info;
  double mind, maxd;
  chol_factor_lds<LD>(A, n, tid, info, mind, maxd);
  for (int e = tid; e < n * n; e += kCholThreads) {
    const int r = e / n, c = e - r * n;
    if (c <= r) blk[(int64_t)r * g.lda + c] = A[r * LD + c];
  }
  const double ls = chol_log_sum<LD>(A, n, sv, tid);
  if (tid == 0) {
    g.rec->info = info ? g.j0 + info : 0;
    g.rec->min_diag = mind;
    g.rec->max_diag = maxd;
    g.rec->logdet = ls;
  }
}

// ---- BLOCKED: L21 = A21 L11^-T ------------------------------------------------------------------------------------------------
struct CholPanelArgs {
  double* a;
  int64_t lda, n;
  int64_t j0, j1;  // the panel's columns; chunk c covers the rows [j1 + c kCholChunk, min(n, j1 + (c + 1) kCholChunk))
};

// Workgroup = one wave = kCholChunk rows of A21.  Row r of the result solves L11 x^T = a_r^T: a lane owns one row and walks it
// alone, so the substitution needs no barrier; every read of L11 is one address for the whole wave, and the rows lie
// kCholNB + 1 doubles apart, so the lanes of a half sit on distinct banks.
__global__ __launch_bounds__(64) void chol_panel_kernel(CholPanelArgs g) {
  constexpr int NB = kCholNB, XL = kCholNB + 1;
  static_assert(kCholChunk == 64 && (NB * NB + kCholChunk * XL) * 8 == kCholPanelLdsBytes, "a wave of rows; both images in the stage");
  extern __shared__ uint4 chol_smem[];
  double* T = reinterpret_cast<double*>(chol_smem);  // [NB][NB]
  double* X = T + NB * NB;                           // [kCholChunk][XL]
  const int tid = (int)threadIdx.x, kv = (int)(g.j1 - g.j0);
  const double* t = g.a + g.j0 * g.lda + g.j0;
  for (int e = tid; e < kv * kv; e += 64) {
    const int i = e / kv, q = e - i * kv;
    if (q <= i) T[i * NB + q] = t[(int64_t)i * g.lda + q];
  }
  const int64_t r0 = chol_piece_begin(g.j1, blockIdx.x, kCholChunk), r1 = chol_piece_end(g.j1, blockIdx.x, kCholChunk, g.n);
  const int rows = (int)(r1 - r0);
  double* blk = g.a + r0 * g.lda + g.j0;
  for (int r = 0; r < kCholChunk; ++r) X[r * XL + tid] = (r < rows && tid < kv) ? blk[(int64_t)r * g.lda + tid] : 0.0;
  __syncthreads();
  double* x = X + tid * XL;
  for (int q = 0; q < kv; ++q) {
    const double xq = x[q] / T[q * NB + q];
    x[q] = xq;
#pragma unroll 8
    for (int i = q + 1; i < kv; ++i) x[i] = __builtin_fma(-T[i * NB + q], xq, x[i]);
  }
  __syncthreads();
  if (tid < kv)
    for (int r = 0; r < rows; ++r) blk[(int64_t)r * g.lda + tid] = X[r * XL + tid];
}

// ---- the MFMA tile: 64 x 64 x 64 by four waves --------------------------------------------------------------------------------
// Wave w owns the rows 16 w .. 16 w + 15.  A lane feeds A[row lane & 15][k lane >> 4] and B[k lane >> 4][col lane & 15]; pa and
// pb point at the lane's first element of either image, SA / SB doubles lie between two steps of 4 k, TB between the four
// 16-wide column tiles of B.  D comes back with row (lane >> 4) + 4 r, col lane & 15.
template <int SA, int SB, int TB>
__device__ __forceinline__ void chol_mma_tile(const double* pa, const double* pb, MT<double>::acc_t (&acc)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = MT<double>::acc_t{0, 0, 0, 0};
#pragma unroll
  for (int s = 0; s < kCholNB / 4; ++s) {
    const double a = pa[s * SA];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = MT<double>::mma(a, pb[s * SB + t * TB], acc[t]);
  }
}

// ---- BLOCKED: A22 -= L21 L21^T over the lower triangle --------------------------------------------------------------------------
struct CholUpdateArgs {
  double* a;
  int64_t lda, n;
  int64_t j0, j1;  // L21: the rows [j1, n) of the columns [j0, j1); A22: the rows and columns [j1, n)
};

// Workgroup p owns the tile pair chol_tile_pair(p) = (bi, bj), bi >= bj.  Both operands are [row][k] images of row chunks of
// L21, rows beyond n and columns beyond the panel as zeros; a diagonal tile stages one chunk, computes the whole tile and
// stores the elements with column <= row alone.
__global__ __launch_bounds__(kCholThreads) void chol_update_kernel(CholUpdateArgs g) {
  constexpr int TM = kCholTile, NB = kCholNB, LD = kCholRowLd;
  static_assert(TM == 64 && NB == 64 && kCholThreads == 256, "four waves of 16 rows x 4 column tiles");
  extern __shared__ uint4 chol_smem[];
  double* Li = reinterpret_cast<double*>(chol_smem);  // [TM][LD]
  double* Lj = Li + TM * LD;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, fc = lane & 15, kq = lane >> 4;
  int64_t bi, bj;
  chol_tile_pair((int64_t)blockIdx.x, &bi, &bj);
  const int64_t m = g.n - g.j1, row0 = bi * TM, col0 = bj * TM;
  const int kv = (int)(g.j1 - g.j0);
  const double* l = g.a + g.j1 * g.lda + g.j0;
  double* c = g.a + g.j1 * g.lda + g.j1;
  for (int e = tid; e < TM * NB; e += kCholThreads) {
    const int r = e / NB, q = e % NB;
    Li[r * LD + q] = (row0 + r < m && q < kv) ? l[(row0 + r) * g.lda + q] : 0.0;
  }
  if (bi != bj) {  // uniform
    for (int e = tid; e < TM * NB; e += kCholThreads) {
      const int r = e / NB, q = e % NB;
      Lj[r * LD + q] = (col0 + r < m && q < kv) ? l[(col0 + r) * g.lda + q] : 0.0;
    }
  } else {
    Lj = Li;
  }
  __syncthreads();
  MT<double>::acc_t acc[4];
  chol_mma_tile<4, 4, 16 * LD>(Li + (16 * wave + fc) * LD + kq, Lj + fc * LD + kq, acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = row0 + 16 * wave + MT<double>::drow(lane, r);
    if (row >= m) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t col = col0 + 16 * t + fc;
      if (col <= row) c[row * g.lda + col] -= acc[t][r];
    }
  }
}

// ---- the status record ---------------------------------------------------------------------------------------------------------
struct CholFinishArgs {
  const CholPanelRecord* rec;
  int64_t npanels;
  CholFactorStatus* st;
};

// One workgroup.  The first failed panel decides info; min and max run over the panels up to it; the logarithms are summed
// thread by thread over the panels tid, tid + kCholThreads, ... and then in the fixed tree.
__global__ __launch_bounds__(kCholThreads) void chol_finish_kernel(CholFinishArgs g) {
  __shared__ double sv[kCholThreads];
  const int tid = (int)threadIdx.x;
  double first = (double)g.npanels;  // panel indices are below 2^11: exact
  for (int64_t p = tid; p < g.npanels; p += kCholThreads)
    if (g.rec[p].info != 0) first = fmin(first, (double)p);
  first = chol_block_reduce(first, sv, tid, [](double x, double y) { return fmin(x, y); });
  const int64_t fp = (int64_t)first, last = fp < g.npanels ? fp + 1 : g.npanels;
  double mn = __builtin_inf(), mx = 0.0, ls = 0.0;
  for (int64_t p = tid; p < last; p += kCholThreads) {
    mn = fmin(mn, g.rec[p].min_diag);
    mx = fmax(mx, g.rec[p].max_diag);
    ls += g.rec[p].logdet;
  }
  mn = chol_block_reduce(mn, sv, tid, [](double x, double y) { return fmin(x, y); });
  mx = chol_block_reduce(mx, sv, tid, [](double x, double y) { return fmax(x, y); });
  ls = chol_block_reduce(ls, sv, tid, [](double x, double y) { return x + y; });
  if (tid == 0) {
    const bool failed = fp < g.npanels;
    g.st->info = failed ? g.rec[fp].info : 0;
    g.st->min_diag = mn;
    g.st->max_diag = mx;
    g.st->logdet = failed ? 0.0 : 2.0 * ls;
  }
}

// ---- SOLVE: diagonal-block solves -----------------------------------------------------------------------------------------------
struct CholTriArgs {
  const double* t;  // kv x kv block of L, row stride ldt (its lower triangle is read)
  int64_t ldt;
  int kv;           // 1 .. kCholNB
  double* x;        // kv rows, row stride ldx; the columns [0, n_rhs)
  int64_t ldx, n_rhs;
};

// Workgroup = one wave = kCholTile columns of X; a lane owns one column and walks it alone.  TRANS: L^T x = y, backward.
template <bool TRANS>
__global__ __launch_bounds__(64) void chol_tri_kernel(CholTriArgs g) {
  constexpr int NB = kCholNB, TW = kCholTile;
  static_assert(TW == 64 && (NB * NB + NB * TW) * 8 <= kCholTriLdsBytes, "a wave of columns; both images in static LDS");
  __shared__ double T[NB * NB];
  __shared__ double X[NB * TW];
  const int tid = (int)threadIdx.x, kv = g.kv;
  for (int e = tid; e < kv * kv; e += 64) {
    const int i = e / kv, q = e - i * kv;
    if (q <= i) T[i * NB + q] = g.t[(int64_t)i * g.ldt + q];
  }
  const int64_t col = (int64_t)blockIdx.x * TW + tid;
  const bool live = col < g.n_rhs;
  for (int i = 0; i < kv; ++i) X[i * TW + tid] = live ? g.x[i * g.ldx + col] : 0.0;
  __syncthreads();
  double* x = X + tid;
  if (TRANS) {
    for (int q = kv - 1; q >= 0; --q) {
      const double xq = x[q * TW] / T[q * NB + q];
      x[q * TW] = xq;
#pragma unroll 8
      for (int i = 0; i < q; ++i) x[i * TW] = __builtin_fma(-T[q * NB + i], xq, x[i * TW]);
    }
  } else {
    for (int q = 0; q < kv; ++q) {
      const double xq = x[q * TW] / T[q * NB + q];
      x[q * TW] = xq;
#pragma unroll 8
      for (int i = q + 1; i < kv; ++i) x[i * TW] = __builtin_fma(-T[i * NB + q], xq, x[i * TW]);
    }
  }
  if (live)
    for (int i = 0; i < kv; ++i) g.x[i * g.ldx + col] = x[i * TW];
}

// ---- SOLVE: C -= L X, C -= L^T X ----------------------------------------------------------------------------------------------
struct CholGemmArgs {
  const double* l;  // !TRANS: m x kv, element (i, q) at l[i ldl + q]; TRANS: element (i, q) at l[q ldl + i]
  int64_t ldl;
  const double* x;  // kv x n, row stride ldx
  int64_t ldx;
  double* c;        // m x n, row stride ldc
  int64_t ldc;
  int64_t m, n;
  int kv;           // 1 .. kCholNB
  int64_t ntn;      // column tiles: workgroup w owns the tile (w / ntn, w % ntn)
};

// One kCholTile x kCholTile tile per workgroup, both operands staged whole with zeros beyond m, n and kv.  L is a [row][k]
// image; L^T is staged as the [k][row] image its rows in memory give, so the loads stay along the rows of L.
template <bool TRANS>
__global__ __launch_bounds__(kCholThreads) void chol_gemm_kernel(CholGemmArgs g) {
  constexpr int TM = kCholTile, NB = kCholNB, LDR = kCholRowLd, LDC = kCholColLd;
  extern __shared__ uint4 chol_smem[];
  double* At = reinterpret_cast<double*>(chol_smem);  // [TM][LDR] or [NB][LDC]
  double* Xt = At + NB * LDC;                         // [NB][LDC]
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, fc = lane & 15, kq = lane >> 4;
  const int64_t bi = (int64_t)blockIdx.x / g.ntn, bj = (int64_t)blockIdx.x % g.ntn;
  const int64_t row0 = bi * TM, col0 = bj * TM;
  for (int e = tid; e < TM * NB; e += kCholThreads) {
    if (TRANS) {
      const int q = e / TM, r = e % TM;
      At[q * LDC + r] = (row0 + r < g.m && q < g.kv) ? g.l[q * g.ldl + row0 + r] : 0.0;
    } else {
      const int r = e / NB, q = e % NB;
      At[r * LDR + q] = (row0 + r < g.m && q < g.kv) ? g.l[(row0 + r) * g.ldl + q] : 0.0;
    }
  }
  for (int e = tid; e < NB * TM; e += kCholThreads) {
    const int q = e / TM, cc = e % TM;
    Xt[q * LDC + cc] = (q < g.kv && col0 + cc < g.n) ? g.x[q * g.ldx + col0 + cc] : 0.0;
  }
  __syncthreads();
  MT<double>::acc_t acc[4];
  if (TRANS)
    chol_mma_tile<4 * LDC, 4 * LDC, 16>(At + kq * LDC + 16 * wave + fc, Xt + kq * LDC + fc, acc);
  else
    chol_mma_tile<4, 4 * LDC, 16>(At + (16 * wave + fc) * LDR + kq, Xt + kq * LDC + fc, acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = row0 + 16 * wave + MT<double>::drow(lane, r);
    if (row >= g.m) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t col = col0 + 16 * t + fc;
      if (col < g.n) g.c[row * g.ldc + col] -= acc[t][r];
    }
  }
}

}  // namespace k
}  // namespace corrla
