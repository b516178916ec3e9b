// Column second moments for PCA on standardised columns (CORRLA_PCA_STANDARDIZE): ss_j = sum_i (x_ij - mu_j)^2 per data
// column j of the staged operand, given the column means mu.  The centred two-pass form (never sum x^2 - m mu^2), f64
// accumulation for every input type, and a fixed summation order: every launch writes per-slab partial sums, a final
// kernel adds them in index order.  No floating-point atomics, so the result is bitwise reproducible for a fixed input.
// The kernels are bandwidth-bound single reads of A: 16-byte loads where the alignment allows, no LDS beyond the block
// reduction, no MFMA.  A is read in place, in its own type: f32, f64 or bfloat16 bit patterns (widened in registers).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>

#include "colstat_plan.hpp"  // kCvThreads, cv_vec

namespace corrla {
namespace k {

// how an operand element is loaded and widened: kVec elements make one 16-byte load (colstat_plan.hpp: cv_vec)
template <class TI>
struct CvIn;
template <>
struct CvIn<float> {
  static constexpr int kVec = cv_vec(sizeof(float));
  static __device__ inline double widen(float v) { return (double)v; }
};
template <>
struct CvIn<double> {
  static constexpr int kVec = cv_vec(sizeof(double));
  static __device__ inline double widen(double v) { return v; }
};
template <>
struct CvIn<uint16_t> {  // bfloat16: the upper 16 bits of a binary32
  static constexpr int kVec = cv_vec(sizeof(uint16_t));
  static __device__ inline double widen(uint16_t v) { return (double)__uint_as_float((uint32_t)v << 16); }
};

// e[0 .. VEC) <- p[0 .. VEC): one 16-byte load (vec: p is 16-byte aligned and all VEC elements may be read), else the
// first nvalid elements one by one and zeros behind them
template <class TI, int VEC>
__device__ inline void cv_load(const TI* __restrict__ p, bool vec, int nvalid, TI (&e)[VEC]) {
  if (vec) {
    const uint4 raw = *reinterpret_cast<const uint4*>(p);
    __builtin_memcpy(e, &raw, sizeof(raw));
  } else {
#pragma unroll
    for (int u = 0; u < VEC; ++u) e[u] = u < nvalid ? p[u] : (TI)0;
  }
}

// ---- data columns run along the memory columns: reduce DOWN the memory rows ------------------------------------------
// x: rows x cols row-major (ld, cols_readable).  A workgroup covers `groups` (a power of two, <= 256) column groups of
// VEC columns and 256 / groups row lanes (added by a fixed LDS tree); blockIdx.y is the slab of rows_per_slab rows.  A wave reads whole 16-byte
// groups of consecutive columns, so the loads are coalesced along the rows of memory.
//   partial[slab * cols + c] = sum over the slab's rows r of (x(r, c) - mu[c])^2
template <class TI, class T>
__global__ __launch_bounds__(kCvThreads) void colss_down_kernel(const TI* __restrict__ x, int64_t rows, int64_t cols, int64_t ld,
                                                                int64_t cols_readable, int aligned, const T* __restrict__ mu,
                                                                int groups, int64_t rows_per_slab, double* __restrict__ partial) {
  constexpr int VEC = CvIn<TI>::kVec;
  __shared__ double red[kCvThreads * VEC];
  const int tx = (int)threadIdx.x & (groups - 1), ty = (int)threadIdx.x / groups, ny = kCvThreads / groups;
  const int64_t c0 = ((int64_t)blockIdx.x * groups + tx) * VEC;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_slab, r1 = min(rows, r0 + rows_per_slab);
  const int nvalid = c0 < cols ? (int)min((int64_t)VEC, cols - c0) : 0;
  const bool vec = aligned && c0 + VEC <= cols_readable;
  double acc[VEC], m[VEC];
#pragma unroll
  for (int u = 0; u < VEC; ++u) {
    acc[u] = 0.0;
    m[u] = u < nvalid ? (double)mu[c0 + u] : 0.0;
  }
  if (nvalid > 0) {
#pragma unroll 4
    for (int64_t r = r0 + ty; r < r1; r += ny) {
      TI e[VEC];
      cv_load<TI, VEC>(x + r * ld + c0, vec, nvalid, e);
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        const double d = CvIn<TI>::widen(e[u]) - m[u];
        acc[u] += d * d;
      }
    }
  }
  // the ny row lanes of one column are added by a tree of fixed shape over LDS (ny is a power of two)
#pragma unroll
  for (int u = 0; u < VEC; ++u) red[(ty * groups + tx) * VEC + u] = acc[u];
  __syncthreads();
  for (int off = ny >> 1; off > 0; off >>= 1) {
    if (ty < off) {
#pragma unroll
      for (int u = 0; u < VEC; ++u) red[(ty * groups + tx) * VEC + u] += red[((ty + off) * groups + tx) * VEC + u];
    }
    __syncthreads();
  }
  if (ty != 0) return;
#pragma unroll
  for (int u = 0; u < VEC; ++u)
    if (u < nvalid) partial[(int64_t)blockIdx.y * cols + c0 + u] = red[tx * VEC + u];
}

// sum over the 64 lanes of a wave, the same tree every time
__device__ inline double cv_wave_sum(double s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  return s;
}

// ---- data columns are the memory rows: reduce ALONG the memory rows --------------------------------------------------
// One wave per (row, segment) unit: a row is cut into `segs` segments of seg_len elements (a multiple of 64 * VEC, so
// that every segment starts on a 16-byte group); the waves of the grid stride over the units.
//   partial[seg * rows + r] = sum over the segment's columns c of (x(r, c) - mu[r])^2
template <class TI, class T>
__global__ __launch_bounds__(kCvThreads) void colss_along_kernel(const TI* __restrict__ x, int64_t rows, int64_t cols, int64_t ld,
                                                                 int64_t cols_readable, int aligned, const T* __restrict__ mu,
                                                                 int segs, int64_t seg_len, double* __restrict__ partial) {
  constexpr int VEC = CvIn<TI>::kVec;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int64_t units = rows * segs;
  for (int64_t unit = (int64_t)blockIdx.x * (kCvThreads / 64) + wave; unit < units; unit += (int64_t)gridDim.x * (kCvThreads / 64)) {
    const int64_t r = unit / segs, sg = unit - r * segs;
    const int64_t cbeg = sg * seg_len, cend = min(cols, cbeg + seg_len);
    const double m = (double)mu[r];
    const TI* __restrict__ row = x + r * ld;
    double acc[VEC];
#pragma unroll
    for (int u = 0; u < VEC; ++u) acc[u] = 0.0;
#pragma unroll 4
    for (int64_t c0 = cbeg + (int64_t)lane * VEC; c0 < cend; c0 += 64 * VEC) {
      const int nvalid = (int)min((int64_t)VEC, cend - c0);
      TI e[VEC];
      cv_load<TI, VEC>(row + c0, aligned && c0 + VEC <= cols_readable, nvalid, e);
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        const double d = CvIn<TI>::widen(e[u]) - m;
        acc[u] += u < nvalid ? d * d : 0.0;
      }
    }
    double s = acc[0];
#pragma unroll
    for (int u = 1; u < VEC; ++u) s += acc[u];
    s = cv_wave_sum(s);
    if (lane == 0) partial[sg * rows + r] = s;
  }
}

// ss[j] = partial[0][j] + partial[1][j] + ... in index order
__global__ void colss_final_kernel(const double* __restrict__ partial, int64_t nslab, int64_t n, double* __restrict__ ss) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double s = 0.0;
  for (int64_t b = 0; b < nslab; ++b) s += partial[b * n + j];
  ss[j] = s;
}

// ---- CSR whose ROWS are the data columns -------------------------------------------------------------------------------
// ss_j = sum over the stored entries of (v - mu_j)^2 + (n_samples - nnz_j) mu_j^2: the implicit zeros are counted, the
// matrix is never densified.  The CSR is the transpose the call built (csr_transpose): the entries of a row are ordered
// by sample index, so duplicate entries -- which add, as in every product -- are neighbours: the first entry of a run
// of equal indices takes the sum of the run, the others nothing, and nnz_j counts the runs.
// One wave per (row, segment) unit, a row cut into `segs` segments of equal entry counts.
template <class T>
__global__ __launch_bounds__(kCvThreads) void csr_colss_kernel(const T* __restrict__ val, const int32_t* __restrict__ ci,
                                                               const int64_t* __restrict__ rp, int64_t rows,
                                                               const T* __restrict__ mu, int segs, double* __restrict__ psum,
                                                               double* __restrict__ pcnt) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int64_t units = rows * segs;
  for (int64_t unit = (int64_t)blockIdx.x * (kCvThreads / 64) + wave; unit < units; unit += (int64_t)gridDim.x * (kCvThreads / 64)) {
    const int64_t r = unit / segs, sg = unit - r * segs;
    const int64_t b = rp[r], e = rp[r + 1];
    const int64_t per = (e - b + segs - 1) / segs;
    const int64_t s0 = b + sg * per, s1 = min(e, s0 + per);
    const double m = (double)mu[r];
    double acc = 0.0, cnt = 0.0;
    for (int64_t i = s0 + lane; i < s1; i += 64) {
      const int32_t c = ci[i];
      if (i > b && ci[i - 1] == c) continue;  // inside a run of duplicates: its first entry has taken it
      double v = (double)val[i];
      for (int64_t q = i + 1; q < e && ci[q] == c; ++q) v += (double)val[q];
      const double d = v - m;
      acc += d * d;
      cnt += 1.0;
    }
    acc = cv_wave_sum(acc);
    cnt = cv_wave_sum(cnt);
    if (lane == 0) {
      psum[sg * rows + r] = acc;
      pcnt[sg * rows + r] = cnt;
    }
  }
}
template <class T>
__global__ void csr_colss_final_kernel(const double* __restrict__ psum, const double* __restrict__ pcnt, int64_t nslab, int64_t n,
                                       const T* __restrict__ mu, double n_samples, double* __restrict__ ss) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double s = 0.0, cnt = 0.0;
  for (int64_t b = 0; b < nslab; ++b) {
    s += psum[b * n + j];
    cnt += pcnt[b * n + j];
  }
  const double m = (double)mu[j];
  ss[j] = s + (n_samples - cnt) * m * m;
}

// ---- ss -> sd and 1 / sd -----------------------------------------------------------------------------------------------
// sd_j = sqrt(ss_j / (m - 1)) (the n - 1 divisor of explained_var, pca_rsvd.rs:91-99: Gram / (m - 1) of the standardised
// matrix is then the correlation matrix).  A column that cannot be told from a constant one gets sd = 1, so that it
// contributes exact zeros after centring instead of rounding noise at unit variance: with var = ss / m it is constant
// when var <= m eps var + (m mu eps)^2, the error bound of the two-pass variance (Chan, Golub, LeVeque; scikit-learn's
// _is_constant_feature), eps that of the output type T.
template <class T>
__global__ void sd_from_ss_kernel(const double* __restrict__ ss, const T* __restrict__ mu, int64_t n, double m, T* __restrict__ sd,
                                  T* __restrict__ inv_sd) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const double eps = (double)std::numeric_limits<T>::epsilon();
  const double var = ss[j] / m, me = m * (double)mu[j] * eps;
  const bool constant = var <= m * eps * var + me * me;
  const double s = constant ? 1.0 : sqrt(ss[j] / (m - 1.0));
  sd[j] = (T)s;
  inv_sd[j] = (T)(1.0 / s);
}

}  // namespace k
}  // namespace corrla
