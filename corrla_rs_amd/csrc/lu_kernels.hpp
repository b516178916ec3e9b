// Dense LU with partial pivoting and the triangular solves on the device (f64, row-major; the geometry is lu_plan.hpp's).
//
// Pivot rule: the entry of largest magnitude on or below the diagonal, ties to the lowest row index (lu_better).  The
// comparisons are exact and the multipliers are formed by a DIVISION a_ij / pivot, not by a reciprocal and a product: with
// |a_ij| <= |pivot| the correctly rounded quotient is <= 1 in magnitude, so |l_ij| <= 1 holds exactly, and l_ij carries one
// rounding as the error bounds of the factorisation assume.  A NaN never wins a comparison: a column whose candidates are
// all NaN keeps the diagonal entry as its pivot, which the pivot check then reports.
// No atomics and no workgroup waits on another: every reduction runs in a fixed order, dependencies between workgroups are
// separate launches on one stream, and every loop is bounded by the shape.  Once a pivot is exactly zero or not finite the
// status record carries its column and every later kernel of the call returns at once, so nothing divides by it.
//
//   lu_small_kernel    n <= kLuSmallN: the whole factorisation by one workgroup in LDS
//   lu_pivot_kernel    one workgroup: finishes the pivot search of column j (from the partial maxima of the panel update,
//                      or from the column itself for the first column of a panel), writes ipiv[j], swaps the panel rows
//   lu_panel_kernel    one workgroup per chunk of rows: scales column j, rank-1 update of the panel columns to its right,
//                      partial maxima of column j + 1
//   lu_swap_kernel     row interchanges ipiv[j0, j1) applied to two column ranges of a matrix (A beside the panel, or B)
//   lu_tri_kernel      X = T^-1 X for one kLuNB block: T unit lower or upper and the tile of X in LDS, one column per lane
//   lu_update_kernel   C -= L U on v_mfma_f64_16x16x4_f64 (MT<double>), K <= kLuNB in one LDS stage, edge tiles in-kernel
//   lu_maxu_kernel / lu_maxu_finish_kernel   max |u_ij| into the status record
//   rbf_tail_kernel    the P, P^T and zero blocks of the RBF system; lu_rhs_kernel its right-hand side [y; 0]
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_kernels.hpp"  // MT<double>
#include "lu_plan.hpp"

namespace corrla {
namespace k {

struct LuBest {
  double v;   // |a|, -1 when the chunk had no comparable candidate
  int64_t i;  // its row
};

__device__ __forceinline__ bool lu_better(double v, int64_t i, double bv, int64_t bi) { return v > bv || (v == bv && i < bi); }

// the best (v, i) of the kLuThreads threads to every thread; sv / si: kLuThreads entries each
__device__ __forceinline__ void lu_block_best(double& v, int64_t& i, double* sv, long long* si, int tid) {
  sv[tid] = v;
  si[tid] = i;
  __syncthreads();
  for (int s = kLuThreads / 2; s > 0; s >>= 1) {
    if (tid < s && lu_better(sv[tid + s], si[tid + s], sv[tid], si[tid])) {
      sv[tid] = sv[tid + s];
      si[tid] = si[tid + s];
    }
    __syncthreads();
  }
  v = sv[0];
  i = si[0];
  __syncthreads();
}

__device__ __forceinline__ bool lu_pivot_ok(double ap) { return ap > 0.0 && ap < __builtin_inf(); }

// ---- SMALL ------------------------------------------------------------------------------------------------------------------
struct LuSmallArgs {
  double* a;  // n x n, row stride lda: LU on return
  int64_t lda;
  int n;      // <= kLuSmallN
  int64_t* ipiv;
  LuStatus* st;
};

__global__ __launch_bounds__(kLuThreads) void lu_small_kernel(LuSmallArgs g) {
  constexpr int LD = kLuSmallLd;
  extern __shared__ uint4 lu_smem[];
  double* A = reinterpret_cast<double*>(lu_smem);  // [n][LD]
  double* sv = A + kLuSmallN * LD;
  long long* si = reinterpret_cast<long long*>(sv + kLuThreads);
  const int tid = (int)threadIdx.x, n = g.n;
  for (int e = tid; e < n * n; e += kLuThreads) {
    const int r = e / n, c = e - r * n;
    A[r * LD + c] = g.a[(int64_t)r * g.lda + c];
  }
  __syncthreads();
  int64_t info = 0;
  double minp = __builtin_inf();
  int j = 0;
  for (; j < n; ++j) {
    double bv = -1.0;
    int64_t bi = j;
    for (int r = j + tid; r < n; r += kLuThreads) {
      const double v = fabs(A[r * LD + j]);
      if (lu_better(v, r, bv, bi)) bv = v, bi = r;
    }
    lu_block_best(bv, bi, sv, si, tid);
    const int p = (int)bi;
    if (p != j)
      for (int c = tid; c < n; c += kLuThreads) {
        const double t = A[j * LD + c];
        A[j * LD + c] = A[p * LD + c];
        A[p * LD + c] = t;
      }
    if (tid == 0) g.ipiv[j] = p;
    __syncthreads();
    const double piv = A[j * LD + j], ap = fabs(piv);
    if (!lu_pivot_ok(ap)) {  // uniform
      info = j + 1;
      if (ap == 0.0) minp = 0.0;
      break;
    }
    minp = fmin(minp, ap);
    for (int r = j + 1 + tid; r < n; r += kLuThreads) A[r * LD + j] = A[r * LD + j] / piv;
    __syncthreads();
    const int w = n - j - 1;
    for (int e = tid; e < w * w; e += kLuThreads) {
      const int r = j + 1 + e / w, c = j + 1 + e % w;
      A[r * LD + c] = __builtin_fma(-A[r * LD + j], A[j * LD + c], A[r * LD + c]);
    }
    __syncthreads();
  }
  for (int q = j + 1 + tid; q < n; q += kLuThreads) g.ipiv[q] = q;  // after a failed column: in range, no interchange
  double mu = 0.0;
  for (int e = tid; e < n * n; e += kLuThreads) {
    const int r = e / n, c = e - r * n;
    const double v = A[r * LD + c];
    g.a[(int64_t)r * g.lda + c] = v;
    if (c >= r) mu = fmax(mu, fabs(v));
  }
  int64_t unused = tid;
  lu_block_best(mu, unused, sv, si, tid);
  if (tid == 0) {
    g.st->info = info;
    g.st->min_pivot = minp;
    g.st->max_u = info ? 0.0 : mu;
  }
}

// ---- BLOCKED: the panel -----------------------------------------------------------------------------------------------------
struct LuPivotArgs {
  double* a;
  int64_t lda, n;
  int64_t j, j0, j1;   // column j of the panel [j0, j1)
  const LuBest* part;  // partial maxima of column j, nparts of them; nparts == 0: search the column itself
  int64_t nparts;
  int64_t* ipiv;
  LuStatus* st;
};

__global__ __launch_bounds__(kLuThreads) void lu_pivot_kernel(LuPivotArgs g) {
  __shared__ double sv[kLuThreads];
  __shared__ long long si[kLuThreads];
  const int tid = (int)threadIdx.x;
  const int64_t j = g.j;
  if (j > 0 && g.st->info != 0) {  // column 0 initialises the record
    if (tid == 0) g.ipiv[j] = j;
    return;
  }
  double bv = -1.0;
  int64_t bi = j;
  if (g.nparts == 0) {
    for (int64_t r = j + tid; r < g.n; r += kLuThreads) {
      const double v = fabs(g.a[r * g.lda + j]);
      if (lu_better(v, r, bv, bi)) bv = v, bi = r;
    }
  } else {
    for (int64_t c = tid; c < g.nparts; c += kLuThreads) {
      const LuBest b = g.part[c];
      if (b.i >= j && b.i < g.n && lu_better(b.v, b.i, bv, bi)) bv = b.v, bi = b.i;
    }
  }
  lu_block_best(bv, bi, sv, si, tid);
  const int64_t p = bi, col = g.j0 + tid;
  if (col < g.j1) {
    const double top = g.a[j * g.lda + col];
    double now = top;
    if (p != j) {
      now = g.a[p * g.lda + col];
      g.a[j * g.lda + col] = now;
      g.a[p * g.lda + col] = top;
    }
    if (col == j) {  // this thread holds the pivot
      g.ipiv[j] = p;
      const double ap = fabs(now);
      if (j == 0) {
        g.st->info = 0;
        g.st->min_pivot = __builtin_inf();
        g.st->max_u = 0.0;
      }
      if (lu_pivot_ok(ap))
        g.st->min_pivot = fmin(g.st->min_pivot, ap);
      else {
        g.st->info = j + 1;
        if (ap == 0.0) g.st->min_pivot = 0.0;
      }
    }
  }
}

struct LuPanelArgs {
  double* a;
  int64_t lda, n;
  int64_t j, j0, j1;
  LuBest* part;  // [chunk]: written when column j + 1 belongs to the panel
  const LuStatus* st;
};

// chunk c: the rows [j + c kLuChunk, min(n, j + (c + 1) kLuChunk)) without the pivot row j.  Lane = panel column, wave = row
// (four rows in flight).  Every lane of a row loads a_rj before the lane of column j stores l_rj: one wave, program order.
__global__ __launch_bounds__(kLuThreads) void lu_panel_kernel(LuPanelArgs g) {
  static_assert(kLuNB == 64 && kLuThreads == 256, "a lane per panel column, a wave per row");
  __shared__ double sv[4];
  __shared__ long long si[4];
  if (g.st->info != 0) return;  // uniform
  const int tid = (int)threadIdx.x, c = tid & 63, w = tid >> 6;
  const int64_t j = g.j, r0 = lu_piece_begin(j, blockIdx.x, kLuChunk), r1 = lu_piece_end(j, blockIdx.x, kLuChunk, g.n);
  const int64_t col = g.j0 + c;
  const bool live = col < g.j1;
  const double piv = g.a[j * g.lda + j];
  const double u = (live && col > j) ? g.a[j * g.lda + col] : 0.0;
  double bv = -1.0;
  int64_t bi = r0 > j ? r0 : j + 1;
  for (int64_t r = r0 + w; r < r1; r += 4) {
    if (r == j) continue;  // uniform over the wave
    double* row = g.a + r * g.lda;
    const double l = row[j] / piv;
    if (live && col == j) row[j] = l;
    if (live && col > j) {
      const double v = __builtin_fma(-l, u, row[col]);
      row[col] = v;
      const double av = fabs(v);
      if (lu_better(av, r, bv, bi)) bv = av, bi = r;
    }
  }
  if (j + 1 < g.j1) {  // uniform
    if (col == j + 1) sv[w] = bv, si[w] = bi;
    __syncthreads();
    if (tid == 0) {
      double v = sv[0];
      int64_t i = si[0];
      for (int q = 1; q < 4; ++q)
        if (lu_better(sv[q], si[q], v, i)) v = sv[q], i = si[q];
      g.part[blockIdx.x] = LuBest{v, i};
    }
  }
}

// ---- row interchanges ------------------------------------------------------------------------------------------------------
struct LuSwapArgs {
  double* m;
  int64_t ld;
  int64_t c0, c1, c2, c3;  // the columns [c0, c1) and [c2, c3)
  const int64_t* ipiv;
  int64_t j0, j1;          // the interchanges j0 .. j1 - 1, in this order
  int64_t n;               // rows of m
  const LuStatus* st;
};

__global__ __launch_bounds__(kLuThreads) void lu_swap_kernel(LuSwapArgs g) {
  if (g.st->info != 0) return;
  const int64_t t = (int64_t)blockIdx.x * kLuThreads + threadIdx.x, na = g.c1 - g.c0;
  if (t >= na + (g.c3 - g.c2)) return;
  const int64_t col = t < na ? g.c0 + t : g.c2 + (t - na);
  for (int64_t j = g.j0; j < g.j1; ++j) {
    const int64_t p = g.ipiv[j];
    if (p == j || p < 0 || p >= g.n) continue;
    const double top = g.m[j * g.ld + col];
    g.m[j * g.ld + col] = g.m[p * g.ld + col];
    g.m[p * g.ld + col] = top;
  }
}

// ---- diagonal-block solves ---------------------------------------------------------------------------------------------------
struct LuTriArgs {
  const double* t;  // kv x kv block of LU, row stride ldt
  int64_t ldt;
  int kv;           // 1 .. kLuNB
  double* x;        // kv rows, row stride ldx; the columns [c0, c1)
  int64_t ldx;
  int64_t c0, c1;
  const LuStatus* st;
};

// Workgroup = one wave = kLuTile columns of X.  The block T and the wave's kv x kLuTile tile of X are staged in LDS; a lane
// owns one column and walks it alone, so the substitution needs no barrier, and every read of T is one address for the whole
// wave.  (A column held in 64 registers with the loops unrolled spilt: the scheduler hoisted the LDS reads.)
template <bool UPPER>
__global__ __launch_bounds__(64) void lu_tri_kernel(LuTriArgs g) {
  constexpr int NB = kLuNB, TW = kLuTile;
  static_assert(TW == 64 && (NB * NB + NB * TW) * 8 <= 65536, "a wave of columns; both images in static LDS");
  __shared__ double T[NB * NB];
  __shared__ double X[NB * TW];
  if (g.st->info != 0) return;  // uniform
  const int tid = (int)threadIdx.x, kv = g.kv;
  for (int e = tid; e < kv * kv; e += 64) {
    const int i = e / kv, q = e - i * kv;
    T[i * NB + q] = g.t[i * g.ldt + q];
  }
  const int64_t col = g.c0 + (int64_t)blockIdx.x * TW + tid;
  const bool live = col < g.c1;
  for (int i = 0; i < kv; ++i) X[i * TW + tid] = live ? g.x[i * g.ldx + col] : 0.0;
  __syncthreads();
  double* x = X + tid;
  if (UPPER) {
    for (int q = kv - 1; q >= 0; --q) {
      const double xq = x[q * TW] / T[q * NB + q];
      x[q * TW] = xq;
#pragma unroll 8
      for (int i = 0; i < q; ++i) x[i * TW] = __builtin_fma(-T[i * NB + q], xq, x[i * TW]);
    }
  } else {
    for (int q = 0; q < kv; ++q) {
      const double xq = x[q * TW];
#pragma unroll 8
      for (int i = q + 1; i < kv; ++i) x[i * TW] = __builtin_fma(-T[i * NB + q], xq, x[i * TW]);
    }
  }
  if (live)
    for (int i = 0; i < kv; ++i) g.x[i * g.ldx + col] = x[i * TW];
}

// ---- C -= L U ---------------------------------------------------------------------------------------------------------------
struct LuUpdateArgs {
  const double* l;  // m x kv, row stride ldl
  int64_t ldl;
  const double* u;  // kv x n, row stride ldu
  int64_t ldu;
  double* c;        // m x n, row stride ldc
  int64_t ldc;
  int64_t m, n;
  int kv;           // 1 .. kLuNB
  int64_t ntn;      // column tiles: workgroup w owns the tile (w / ntn, w % ntn)
  const LuStatus* st;
};

// One kLuTile x kLuTile tile per workgroup.  Both operands are staged whole (K = kv <= kLuNB), rows and columns beyond m, n
// and kv as zeros: nothing is read or written out of bounds and no padding rows exist.  Wave w owns the rows 16 w .. 16 w + 15:
// a lane feeds A[row lane & 15][k lane >> 4] and B[k lane >> 4][col lane & 15]; D comes back with row (lane >> 4) + 4 r, col
// lane & 15, so 16 lanes read and write 128 contiguous bytes of C.
__global__ __launch_bounds__(kLuThreads) void lu_update_kernel(LuUpdateArgs g) {
  constexpr int TM = kLuTile, NB = kLuNB, LDL = kLuOpLd, LDU = kLuTile + 1;
  static_assert(TM == 64 && NB % 4 == 0 && kLuThreads == 256, "four waves of 16 rows x 4 column tiles");
  typedef MT<double>::acc_t acc_t;
  extern __shared__ uint4 lu_smem[];
  double* Lt = reinterpret_cast<double*>(lu_smem);  // [TM][LDL]
  double* Ut = Lt + TM * LDL;                       // [NB][LDU]
  if (g.st->info != 0) return;  // uniform
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, fc = lane & 15, kq = lane >> 4;
  const int64_t bi = (int64_t)blockIdx.x / g.ntn, bj = (int64_t)blockIdx.x % g.ntn;
  const int64_t row0 = bi * TM, col0 = bj * TM;
  for (int e = tid; e < TM * NB; e += kLuThreads) {
    const int r = e / NB, q = e % NB;
    Lt[r * LDL + q] = (row0 + r < g.m && q < g.kv) ? g.l[(row0 + r) * g.ldl + q] : 0.0;
  }
  for (int e = tid; e < NB * TM; e += kLuThreads) {
    const int q = e / TM, c = e % TM;
    Ut[q * LDU + c] = (q < g.kv && col0 + c < g.n) ? g.u[q * g.ldu + col0 + c] : 0.0;
  }
  __syncthreads();
  acc_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = acc_t{0, 0, 0, 0};
  const double* pl = Lt + (16 * wave + fc) * LDL + kq;
  const double* pu = Ut + kq * LDU + fc;
#pragma unroll
  for (int s = 0; s < NB / 4; ++s) {
    const double a = pl[4 * s];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = MT<double>::mma(a, pu[4 * s * LDU + 16 * t], acc[t]);
  }
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

// ---- max |u_ij| ---------------------------------------------------------------------------------------------------------------
struct LuMaxUArgs {
  const double* a;
  int64_t lda, n;
  double* part;  // [workgroup]
  int64_t nparts;
  LuStatus* st;
};

__device__ __forceinline__ double lu_block_max(double v, double* sv, int tid) {
  sv[tid] = v;
  __syncthreads();
  for (int s = kLuThreads / 2; s > 0; s >>= 1) {
    if (tid < s) sv[tid] = fmax(sv[tid], sv[tid + s]);
    __syncthreads();
  }
  return sv[0];
}

// workgroup b: the rows [b kLuTile, min(n, (b + 1) kLuTile)) of U
__global__ __launch_bounds__(kLuThreads) void lu_maxu_kernel(LuMaxUArgs g) {
  __shared__ double sv[kLuThreads];
  const int tid = (int)threadIdx.x;
  double m = 0.0;
  if (g.st->info == 0) {
    const int64_t r0 = (int64_t)blockIdx.x * kLuTile, r1 = min(g.n, r0 + kLuTile);
    for (int64_t r = r0; r < r1; ++r)
      for (int64_t c = r + tid; c < g.n; c += kLuThreads) m = fmax(m, fabs(g.a[r * g.lda + c]));
  }
  m = lu_block_max(m, sv, tid);
  if (tid == 0) g.part[blockIdx.x] = m;
}

__global__ __launch_bounds__(kLuThreads) void lu_maxu_finish_kernel(LuMaxUArgs g) {
  __shared__ double sv[kLuThreads];
  const int tid = (int)threadIdx.x;
  double m = 0.0;
  for (int64_t q = tid; q < g.nparts; q += kLuThreads) m = fmax(m, g.part[q]);
  m = lu_block_max(m, sv, tid);
  if (tid == 0 && g.st->info == 0) g.st->max_u = m;
}

// ---- the RBF system around its kernel block ---------------------------------------------------------------------------------
struct RbfTailArgs {
  const double* x;  // n_s x dim, row stride ldx
  int64_t ldx, n_s;
  int dim;
  int tail;         // 1 [x, 1], 2 [x, x_a x_b (a <= b, a outer), 1]
  int64_t n_poly;
  double* m;        // (n_s + n_poly) x (n_s + n_poly), row stride ldm
  int64_t ldm;
};

// One thread per entry of P (written to P and to P^T: one value, so the two blocks agree bitwise) and per entry of the zero
// corner; the terms in build_full_vandermonde's order, one rounding per product.
__global__ __launch_bounds__(kLuThreads) void rbf_tail_kernel(RbfTailArgs g) {
  const int64_t idx = (int64_t)blockIdx.x * kLuThreads + threadIdx.x, np = g.n_s * g.n_poly;
  if (idx >= np + g.n_poly * g.n_poly) return;
  if (idx >= np) {
    const int64_t e = idx - np, a = e / g.n_poly, b = e - a * g.n_poly;
    g.m[(g.n_s + a) * g.ldm + g.n_s + b] = 0.0;
    return;
  }
  const int64_t i = idx / g.n_poly, t = idx - i * g.n_poly;
  const double* x = g.x + i * g.ldx;
  double v = 1.0;
  if (t < g.dim) {
    v = x[t];
  } else if (t < g.n_poly - 1) {  // tail == 2: the pair (a, b) of term t
    int64_t q = t - g.dim;
    int a = 0;
    while (a < g.dim - 1 && q >= g.dim - a) q -= g.dim - a, ++a;
    v = x[a] * x[a + q];
  }
  g.m[i * g.ldm + g.n_s + t] = v;
  g.m[(g.n_s + t) * g.ldm + i] = v;
}

struct LuRhsArgs {
  const double* y;  // n_s x n_rhs, row stride ldy
  int64_t ldy, n_s, n, n_rhs;
  double* b;        // n x n_rhs, row stride ldb: [y; 0]
  int64_t ldb;
};

__global__ __launch_bounds__(kLuThreads) void lu_rhs_kernel(LuRhsArgs g) {
  const int64_t idx = (int64_t)blockIdx.x * kLuThreads + threadIdx.x;
  if (idx >= g.n * g.n_rhs) return;
  const int64_t i = idx / g.n_rhs, c = idx - i * g.n_rhs;
  g.b[i * g.ldb + c] = i < g.n_s ? g.y[i * g.ldy + c] : 0.0;
}

}  // namespace k
}  // namespace corrla
