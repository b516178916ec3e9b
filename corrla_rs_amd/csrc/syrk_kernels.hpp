// Covariance / correlation matrices (corrla_cov_*): the symmetric rank-k product C = (X - 1 mu^T)^T (X - 1 mu^T) on the exact
// MFMAs (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 through MT<T>), the column moments it centres with, and the
// finishing kernel.  The geometry is syrk_plan.hpp's.
//
// syrk_kernel<T, CENTER>: one workgroup per (tile pair bi <= bj, row slab).  Both operands are 128 columns of the same rows
// of X; a tile of KT rows is loaded into registers (16-byte loads in place; element loads with bounds checks for an
// unaligned base or leading dimension), centred THERE -- X is never rewritten or copied, and rows and columns beyond the
// matrix become exact zeros, not -mu -- and stored to a row-linear LDS image.  The loads of the next tile are in flight
// while the MFMAs of this one run.  Each of the four waves owns 64 x 64 of the tile as 4 x 4 MFMA tiles; tile t of a lane
// belongs to column 4 fc + t (fc = lane & 15), so the four operand values of a reduction row are ONE 16-byte (f32) /
// 32-byte (f64) LDS read per operand for 16 MFMAs.  The partial tile goes to the slab workspace with vector stores.
// No floating-point atomics: a fixed input gives a bitwise fixed output.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>

#include "colvar_kernels.hpp"  // cv_load, CvIn
#include "hip_kernels.hpp"     // MT<T>
#include "syrk_plan.hpp"

namespace corrla {
namespace k {

// ---- column moments -------------------------------------------------------------------------------------------------------
// One pass over X (rows x cols row-major, ld) with the data shifted by the column's first row s_c = x(0, c):
//   psum[slab * cols + c] = sum over the slab's rows of (x - s_c),   psq[...] = sum of (x - s_c)^2
// f64 accumulation, the fixed LDS tree of colss_down_kernel, per-slab partials: bitwise reproducible.
template <class T>
__global__ __launch_bounds__(kCvThreads) void colmom_down_kernel(const T* __restrict__ x, int64_t rows, int64_t cols, int64_t ld,
                                                                 int aligned, int groups, int64_t rows_per_slab,
                                                                 double* __restrict__ psum, double* __restrict__ psq) {
  constexpr int VEC = CvIn<T>::kVec;
  __shared__ double red[2 * kCvThreads * VEC];
  const int tx = (int)threadIdx.x & (groups - 1), ty = (int)threadIdx.x / groups, ny = kCvThreads / groups;
  const int64_t c0 = ((int64_t)blockIdx.x * groups + tx) * VEC;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_slab, r1 = min(rows, r0 + rows_per_slab);
  const int nvalid = c0 < cols ? (int)min((int64_t)VEC, cols - c0) : 0;
  const bool vec = aligned && c0 + VEC <= cols;
  double a1[VEC], a2[VEC], sh[VEC];
#pragma unroll
  for (int u = 0; u < VEC; ++u) {
    a1[u] = a2[u] = 0.0;
    sh[u] = u < nvalid ? (double)x[c0 + u] : 0.0;
  }
  if (nvalid > 0) {
#pragma unroll 4
    for (int64_t r = r0 + ty; r < r1; r += ny) {
      T e[VEC];
      cv_load<T, VEC>(x + r * ld + c0, vec, nvalid, e);
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        const double d = (double)e[u] - sh[u];
        a1[u] += d;
        a2[u] += d * d;
      }
    }
  }
  double* red2 = red + kCvThreads * VEC;
#pragma unroll
  for (int u = 0; u < VEC; ++u) {
    red[(ty * groups + tx) * VEC + u] = a1[u];
    red2[(ty * groups + tx) * VEC + u] = a2[u];
  }
  __syncthreads();
  for (int off = ny >> 1; off > 0; off >>= 1) {
    if (ty < off) {
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        red[(ty * groups + tx) * VEC + u] += red[((ty + off) * groups + tx) * VEC + u];
        red2[(ty * groups + tx) * VEC + u] += red2[((ty + off) * groups + tx) * VEC + u];
      }
    }
    __syncthreads();
  }
  if (ty != 0) return;
#pragma unroll
  for (int u = 0; u < VEC; ++u)
    if (u < nvalid) {
      psum[(int64_t)blockIdx.y * cols + c0 + u] = red[tx * VEC + u];
      psq[(int64_t)blockIdx.y * cols + c0 + u] = red2[tx * VEC + u];
    }
}

// The partials in index order, then mu = s + sum(x - s) / m and ss = sum (x - s)^2 - m (mu - s)^2 in f64.
//   mu64: the f64 mean;  mu_t: it rounded once to T (what the product centres with and what the caller gets)
//   sd64: sqrt(ss / denom), or 1 for a column that the rule of CORRLA_PCA_STANDARDIZE (sd_from_ss_kernel) calls constant;
//   sd_t: it rounded to T (the scales the caller gets)
//   is_const: that verdict
template <class T>
__global__ void colmom_final_kernel(const double* __restrict__ psum, const double* __restrict__ psq, int64_t nslab, int64_t n,
                                    const T* __restrict__ x, double m, double denom, double* __restrict__ mu64,
                                    T* __restrict__ mu_t, double* __restrict__ sd64, T* __restrict__ sd_t,
                                    int* __restrict__ is_const) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t b = 0; b < nslab; ++b) {
    s1 += psum[b * n + j];
    s2 += psq[b * n + j];
  }
  const double sh = (double)x[j], dm = s1 / m;
  const double mu = sh + dm;
  const double ss = fmax(s2 - m * dm * dm, 0.0);
  const double eps = (double)std::numeric_limits<T>::epsilon();
  const double var = ss / m, me = m * (double)(T)mu * eps;
  const bool constant = var <= m * eps * var + me * me;
  mu64[j] = mu;
  mu_t[j] = (T)mu;
  const double sd = constant ? 1.0 : sqrt(ss / denom);
  sd64[j] = sd;
  sd_t[j] = (T)sd;
  is_const[j] = constant ? 1 : 0;
}

// ---- the symmetric product ------------------------------------------------------------------------------------------------
template <class T>
struct SyrkArgs {
  const T* x;       // rows x n row-major
  int64_t m, n, ld;
  int aligned;      // 16-byte loads are legal: base 16-byte aligned and ld a multiple of the vector width
  const T* mu;      // n column means (CENTER), rounded to T
  int64_t slab_rows;
  int64_t npairs;
  T* ws;            // [slab][pair][128][128] partial tiles
};

// T e[VEC] <- x(row, col .. col + VEC), centred; zeros for row >= r_end and for columns >= n
template <class T, bool CENTER, int VEC>
__device__ __forceinline__ void syrk_load(const SyrkArgs<T>& g, int64_t row, int64_t r_end, int64_t col, bool vec_ok, int nvalid,
                                          const T (&mu)[VEC], T (&e)[VEC]) {
  if (row < r_end && nvalid > 0) {
    cv_load<T, VEC>(g.x + row * g.ld + col, vec_ok, nvalid, e);
    if (CENTER) {
#pragma unroll
      for (int u = 0; u < VEC; ++u) e[u] = u < nvalid ? e[u] - mu[u] : (T)0;
    }
  } else {
#pragma unroll
    for (int u = 0; u < VEC; ++u) e[u] = (T)0;
  }
}

template <class T, bool CENTER>
__global__ __launch_bounds__(kSyrkThreads) void syrk_kernel(SyrkArgs<T> g) {
  constexpr int BT = kSyrkBT, KT = syrk_kt((int)sizeof(T)), VEC = 16 / (int)sizeof(T);
  constexpr int CH = BT / VEC;             // 16-byte chunks per image row
  constexpr int NQ = KT * CH / kSyrkThreads;  // chunks per thread per image (4)
  constexpr int RQ = kSyrkThreads / CH;    // image rows between a thread's chunks
  static_assert(NQ * kSyrkThreads == KT * CH && RQ * CH == kSyrkThreads, "chunks must split evenly over the threads");
  typedef typename MT<T>::acc_t acc_t;
  extern __shared__ uint4 syrk_smem[];
  T* lds_i = reinterpret_cast<T*>(syrk_smem);
  int bi, bj;
  syrk_pair((int64_t)blockIdx.x, &bi, &bj);
  const bool diag = bi == bj;
  T* lds_j = diag ? lds_i : lds_i + KT * BT;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1, fc = lane & 15, kq = lane >> 4;

  // staging: this thread's chunk column is the same for every chunk and every tile
  const int cc = tid % CH, kr0 = tid / CH;
  const int64_t col_i = (int64_t)bi * BT + cc * VEC, col_j = (int64_t)bj * BT + cc * VEC;
  const int nv_i = col_i < g.n ? (int)min((int64_t)VEC, g.n - col_i) : 0;
  const int nv_j = col_j < g.n ? (int)min((int64_t)VEC, g.n - col_j) : 0;
  const bool vec_i = g.aligned && nv_i == VEC, vec_j = g.aligned && nv_j == VEC;
  T mu_i[VEC], mu_j[VEC];
#pragma unroll
  for (int u = 0; u < VEC; ++u) {
    mu_i[u] = (CENTER && u < nv_i) ? g.mu[col_i + u] : (T)0;
    mu_j[u] = (CENTER && u < nv_j) ? g.mu[col_j + u] : (T)0;
  }
  const int64_t r_begin = (int64_t)blockIdx.y * g.slab_rows;
  const int64_t r_end = min(g.m, r_begin + g.slab_rows);
  const int64_t ntiles = r_end > r_begin ? (r_end - r_begin + KT - 1) / KT : 0;

  acc_t acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = acc_t{0, 0, 0, 0};

  T ri[NQ][VEC], rj[NQ][VEC];
  auto fetch = [&](int64_t t) {
    const int64_t r0 = r_begin + t * KT + kr0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      syrk_load<T, CENTER, VEC>(g, r0 + q * RQ, r_end, col_i, vec_i, nv_i, mu_i, ri[q]);
      if (!diag) syrk_load<T, CENTER, VEC>(g, r0 + q * RQ, r_end, col_j, vec_j, nv_j, mu_j, rj[q]);
    }
  };
  if (ntiles > 0) fetch(0);
  for (int64_t t = 0; t < ntiles; ++t) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      uint4 raw;
      __builtin_memcpy(&raw, ri[q], sizeof(raw));
      *reinterpret_cast<uint4*>(lds_i + (kr0 + q * RQ) * BT + cc * VEC) = raw;
      if (!diag) {
        __builtin_memcpy(&raw, rj[q], sizeof(raw));
        *reinterpret_cast<uint4*>(lds_j + (kr0 + q * RQ) * BT + cc * VEC) = raw;
      }
    }
    __syncthreads();
    if (t + 1 < ntiles) fetch(t + 1);  // in flight while the MFMAs below run
    const T* pa = lds_i + kq * BT + 64 * wi + 4 * fc;
    const T* pb = lds_j + kq * BT + 64 * wj + 4 * fc;
#pragma unroll
    for (int kk = 0; kk < KT / 4; ++kk) {
      T a[4], b[4];
      __builtin_memcpy(a, pa + kk * 4 * BT, sizeof(a));
      __builtin_memcpy(b, pb + kk * 4 * BT, sizeof(b));
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = MT<T>::mma(a[ti], b[tj], acc[ti][tj]);
    }
    __syncthreads();
  }

  // D of MFMA tile (ti, tj): row = drow(lane, r) <-> I column 64 wi + 4 row + ti; col = fc <-> J column 64 wj + 4 fc + tj.
  // The four tj of a lane are four consecutive J columns: one vector store.
  T* out = g.ws + ((int64_t)blockIdx.y * g.npairs + (int64_t)blockIdx.x) * (BT * BT);
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 64 * wi + 4 * MT<T>::drow(lane, r) + ti;
      T v[4] = {acc[ti][0][r], acc[ti][1][r], acc[ti][2][r], acc[ti][3][r]};
      T* dst = out + row * BT + 64 * wj + 4 * fc;
      if constexpr (sizeof(T) == 4) {
        uint4 raw;
        __builtin_memcpy(&raw, v, sizeof(raw));
        *reinterpret_cast<uint4*>(dst) = raw;
      } else {
        uint4 raw[2];
        __builtin_memcpy(raw, v, sizeof(raw));
        reinterpret_cast<uint4*>(dst)[0] = raw[0];
        reinterpret_cast<uint4*>(dst)[1] = raw[1];
      }
    }
}

// ---- finish ----------------------------------------------------------------------------------------------------------------
// One workgroup per (pair, 32 x 32 sub-tile).  value(i, j) = sum over the slabs in index order (f64)
//   - m delta_i delta_j, delta = mu - fl_T(mu): sum (x - mu)(y - nu) = sum (x - fl mu)(y - fl nu) - m delta_i delta_j, exactly
//   / (m - ddof);  correlation: / (sd_i sd_j), clipped to [-1, 1], exactly 1 on the diagonal; a constant column gives a zero
//   row and column and a zero diagonal.
// C(i, j) and C(j, i) are written from the same value (the mirror goes through LDS so that both writes are coalesced); on a
// diagonal pair only the sub-tiles on and above the diagonal are taken, and inside a diagonal sub-tile every entry reads
// the partial sums of its upper-triangle twin.
template <class T>
struct SyrkFinishArgs {
  const T* ws;
  int64_t nsplit, npairs, n;
  double m, denom;
  const double* mu64;   // nullptr: no centring
  const T* mu_t;
  const double* sd64;   // nullptr: covariance
  const int* is_const;
  T* c;
  int64_t ldc;
};

template <class T>
__global__ __launch_bounds__(256) void syrk_finish_kernel(SyrkFinishArgs<T> g) {
  constexpr int BT = kSyrkBT;
  __shared__ T tile[32][33];
  int bi, bj;
  syrk_pair((int64_t)blockIdx.x, &bi, &bj);
  const int si = (int)blockIdx.y >> 2, sj = (int)blockIdx.y & 3;
  const bool diag_pair = bi == bj;
  if (diag_pair && si > sj) return;
  const bool diag_sub = diag_pair && si == sj;
  const int tx = (int)threadIdx.x & 31, ty = (int)threadIdx.x >> 5;
  const int64_t i0 = (int64_t)bi * BT + si * 32, j0 = (int64_t)bj * BT + sj * 32;
  const T* base = g.ws + (int64_t)blockIdx.x * (BT * BT);
  const int64_t slab_stride = g.npairs * (BT * BT);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int li = ty + 8 * q, lj = tx;
    const int64_t i = i0 + li, j = j0 + lj;
    T out = (T)0;
    if (i < g.n && j < g.n) {
      // a diagonal sub-tile: the entry below the diagonal takes the partial sums of its twin above
      const int ui = (diag_sub && li > lj) ? lj : li, uj = (diag_sub && li > lj) ? li : lj;
      const T* p = base + (si * 32 + ui) * BT + sj * 32 + uj;
      double s = 0.0;
      // the loads of four slabs in flight, the additions still in index order
#pragma unroll 4
      for (int64_t b = 0; b < g.nsplit; ++b) s += (double)p[b * slab_stride];
      if (g.mu64) {
        const double di = g.mu64[i] - (double)g.mu_t[i], dj = g.mu64[j] - (double)g.mu_t[j];
        s -= g.m * di * dj;
      }
      double v = s / g.denom;
      if (g.sd64) {
        const bool dead = g.is_const[i] || g.is_const[j];
        if (dead)
          v = 0.0;
        else if (i == j)
          v = 1.0;
        else
          v = fmin(1.0, fmax(-1.0, v / (g.sd64[i] * g.sd64[j])));
      }
      out = (T)v;
      g.c[i * g.ldc + j] = out;
    }
    tile[li][lj] = out;
  }
  if (diag_sub) return;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int lj = ty + 8 * q, li = tx;  // C(j, i), coalesced along i
    const int64_t i = i0 + li, j = j0 + lj;
    if (i < g.n && j < g.n) g.c[j * g.ldc + i] = tile[li][lj];
  }
}

}  // namespace k
}  // namespace corrla
