// Gaussian kernel density estimates on the device (KdeRv, univariate_rv.rs:165-170, 423-444): pdf, cdf, logpdf at n_q
// points over n_s supports for one bandwidth h, and the negative log-likelihood with its derivative in h for up to 64
// bandwidths at once.  The pairwise work is exp / erfc on the VALU and the transcendental unit, there is no matrix product
// in it; the n_q x n_s matrix is never stored.  The geometry is kde_plan.hpp's.
//
// With d_ij = x_i - s_j and t_ij = d_ij^2 / (2 h^2) the sums are taken in the stabilised form
//   S_i = sum_j exp(-(t_ij - t*_i)),  t*_i = d*_i / (2 h^2),  d*_i = min_j d_ij^2,
// so the nearest support contributes exactly 1 and ln S_i is finite for every h > 0.  d*_i does not depend on h:
// kde_nearest_kernel computes it once per call (sub, mul, min per pair), one partial minimum per split of the supports, and
// the prologue of kde_sum_kernel takes the minimum over the partials -- a minimum does not depend on the order.  Both kernels
// form d^2 as fl(fl(x - s)^2) with contraction off, so the d^2 the sum kernel subtracts d* from is the bit pattern the
// minimum was taken over: the exponent of the nearest support is exactly zero and every exponent is <= 0.
//
// kde_sum_kernel<T, MODE>: a thread keeps PP points in registers and sweeps the supports of its split, staged SC at a time
// in LDS; every lane reads the same support at the same time, a broadcast read.  Per pair d^2 is formed once and serves the
// NB <= HG bandwidths of the workgroup's group: e = (d* - d^2) c_b with the wave-uniform c_b from the kernel arguments, in
// f32 c_b = log2(e) / (2 h_b^2) so that K = v_exp_f32(e) directly, in f64 c_b = 1 / (2 h_b^2) and K = exp(e).
//   MODE kKdeSum (pdf, logpdf)  one accumulator per (point, bandwidth): sum K
//   MODE kKdeNll                two: sum K and sum e K.  (R_i = sum 2 t K / sum K = 2 t* - 2 sum (e K) / sum K in natural
//                               units: the second sum carries the far supports at their own small weight.)  e is clamped
//                               from below where K is zero anyway, so that e K is never (-inf) 0.
//   MODE kKdeCdf                one: sum erfc(-d c), c = 1 / (h sqrt 2); no d*.
// Sums run over the supports in index order in the element type; the partials of a split go to workspace.  A bandwidth's
// arithmetic does not depend on its group: NB only says how many are live.
// kde_finish_kernel adds the splits in index order in f64 and applies ln, the normalisation and t*; kde_nll_points_kernel
// does the same per (point, bandwidth) and reduces over a fixed range of points by a fixed tree, kde_nll_reduce_kernel
// reduces the ranges.  No atomics: a fixed input gives a bitwise fixed output.
// Every global access is guarded by the point count or the split's end; strides are element strides, any base alignment.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kde_plan.hpp"

namespace corrla {
namespace k {

constexpr int kKdeSum = 0, kKdeCdf = 1, kKdeNll = 2;

template <class T>
struct KdeNearArgs {
  const T* x;  // n_q points, element stride incx
  int64_t incx;
  const T* s;  // n_s supports, element stride incs
  int64_t incs;
  int64_t n_q, n_s, nqt, split_len;
  T* ws_min;   // [nsplit][n_q]
};

// the chunk [j0, j0 + kv) of the supports in LDS
template <class T>
__device__ __forceinline__ void kde_stage_chunk(T* lds_s, const T* s, int64_t incs, int64_t j0, int kv, int tid) {
  for (int e = tid; e < kv; e += kKdeThreads) lds_s[e] = s[(j0 + e) * incs];
}

template <class T>
__global__ __launch_bounds__(kKdeThreads) void kde_nearest_kernel(KdeNearArgs<T> g) {
#pragma clang fp contract(off)
  constexpr int PP = kKdePP, QT = kKdeQT, SC = kKdeSC;
  __shared__ T lds_s[SC];
  const int tid = (int)threadIdx.x;
  const int64_t tile = (int64_t)blockIdx.x % g.nqt, sp = (int64_t)blockIdx.x / g.nqt;
  const int64_t j_begin = sp * g.split_len, j_end = min(g.n_s, j_begin + g.split_len);
  T xv[PP], m[PP];
#pragma unroll
  for (int p = 0; p < PP; ++p) {
    const int64_t i = tile * QT + p * kKdeThreads + tid;
    xv[p] = i < g.n_q ? g.x[i * g.incx] : (T)0;
    m[p] = (T)__builtin_huge_val();
  }
  for (int64_t j0 = j_begin; j0 < j_end; j0 += SC) {
    const int kv = (int)min((int64_t)SC, j_end - j0);
    kde_stage_chunk(lds_s, g.s, g.incs, j0, kv, tid);
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < kv; ++j) {
      const T sj = lds_s[j];
#pragma unroll
      for (int p = 0; p < PP; ++p) {
        const T d = xv[p] - sj;
        m[p] = fmin(m[p], d * d);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < PP; ++p) {
    const int64_t i = tile * QT + p * kKdeThreads + tid;
    if (i < g.n_q) g.ws_min[sp * g.n_q + i] = m[p];
  }
}

template <class T>
struct KdeSumArgs {
  const T* x;
  int64_t incx;
  const T* s;
  int64_t incs;
  int64_t n_q, n_s, nqt, split_len, nsplit;
  int ngroups, nb;  // bandwidth groups and bandwidths of this launch
  const T* ws_min;  // [nsplit][n_q]; not read by kKdeCdf
  T* ws_sum;        // [nsplit][nacc][nb][n_q]
  T c[kKdeHL];      // the exponent scale of each bandwidth (see above)
};

template <class T>
__device__ __forceinline__ T kde_exp_scaled(T e);
template <>
__device__ __forceinline__ float kde_exp_scaled<float>(float e) {
  return __builtin_amdgcn_exp2f(e);  // v_exp_f32, 1 ulp; e <= 0, results below 2^-126 flush to zero
}
template <>
__device__ __forceinline__ double kde_exp_scaled<double>(double e) {
  return exp(e);
}
__device__ __forceinline__ float kde_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double kde_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
// below this K is zero in the type (2^-160 in f32, e^-800 in f64): the clamp of the likelihood's exponent
template <class T>
__device__ __forceinline__ constexpr T kde_exp_floor() {
  return sizeof(T) == 4 ? (T)-160 : (T)-800;
}

// one (tile, group, split) with NB live bandwidths b0 .. b0 + NB - 1 of the launch
template <class T, int MODE, int NB>
__device__ __forceinline__ void kde_sum_body(const KdeSumArgs<T>& g, T* lds_s, int64_t tile, int b0, int64_t sp) {
#pragma clang fp contract(off)
  constexpr int PP = kKdePP, QT = kKdeQT, SC = kKdeSC, NACC = MODE == kKdeNll ? 2 : 1;
  const int tid = (int)threadIdx.x;
  const int64_t j_begin = sp * g.split_len, j_end = min(g.n_s, j_begin + g.split_len);
  T xv[PP], dstar[PP], acc[PP][NB], acc2[PP][NB], c[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) c[b] = g.c[b0 + b];
#pragma unroll
  for (int p = 0; p < PP; ++p) {
    const int64_t i = tile * QT + p * kKdeThreads + tid;
    const bool live = i < g.n_q;
    xv[p] = live ? g.x[i * g.incx] : (T)0;
    dstar[p] = (T)0;
    if (MODE != kKdeCdf && live) {  // the minimum over the splits' partial minima
      T m = g.ws_min[i];
      for (int64_t q = 1; q < g.nsplit; ++q) m = fmin(m, g.ws_min[q * g.n_q + i]);
      dstar[p] = m;
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[p][b] = acc2[p][b] = (T)0;
  }
  for (int64_t j0 = j_begin; j0 < j_end; j0 += SC) {
    const int kv = (int)min((int64_t)SC, j_end - j0);
    kde_stage_chunk(lds_s, g.s, g.incs, j0, kv, tid);
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < kv; ++j) {
      const T sj = lds_s[j];
#pragma unroll
      for (int p = 0; p < PP; ++p) {
        const T d = xv[p] - sj;
        if (MODE == kKdeCdf) {
          acc[p][0] = acc[p][0] + erfc(-d * c[0]);
        } else {
          const T a = dstar[p] - d * d;  // <= 0; exactly 0 at the nearest support
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            T e = a * c[b];
            if (MODE == kKdeNll) e = fmax(e, kde_exp_floor<T>());
            const T kk = kde_exp_scaled<T>(e);
            acc[p][b] = acc[p][b] + kk;
            if (MODE == kKdeNll) acc2[p][b] = kde_fma(e, kk, acc2[p][b]);
          }
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < PP; ++p) {
    const int64_t i = tile * QT + p * kKdeThreads + tid;
    if (i >= g.n_q) continue;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      g.ws_sum[((sp * NACC + 0) * g.nb + b0 + b) * g.n_q + i] = acc[p][b];
      if (MODE == kKdeNll) g.ws_sum[((sp * NACC + 1) * g.nb + b0 + b) * g.n_q + i] = acc2[p][b];
    }
  }
}

template <class T, int MODE>
__global__ __launch_bounds__(kKdeThreads) void kde_sum_kernel(KdeSumArgs<T> g) {
  static_assert(kKdeHG == 4, "the switch below lists the live counts of a group");
  __shared__ T lds_s[kKdeSC];
  int64_t w = (int64_t)blockIdx.x;
  const int64_t tile = w % g.nqt;
  w /= g.nqt;
  const int grp = (int)(w % g.ngroups);
  const int64_t sp = w / g.ngroups;
  const int b0 = grp * kKdeHG;
  if constexpr (MODE == kKdeNll) {
    switch (min(kKdeHG, g.nb - b0)) {  // uniform, once per workgroup
      case 1: kde_sum_body<T, MODE, 1>(g, lds_s, tile, b0, sp); break;
      case 2: kde_sum_body<T, MODE, 2>(g, lds_s, tile, b0, sp); break;
      case 3: kde_sum_body<T, MODE, 3>(g, lds_s, tile, b0, sp); break;
      default: kde_sum_body<T, MODE, 4>(g, lds_s, tile, b0, sp); break;
    }
  } else {
    kde_sum_body<T, MODE, 1>(g, lds_s, tile, b0, sp);
  }
}

template <class T>
struct KdeFinishArgs {
  const T* ws_min;  // [nsplit][n_q]
  const T* ws_sum;  // [nsplit][n_q]
  int64_t nsplit, n_q, n_s;
  int what;         // 0 pdf, 1 cdf, 2 logpdf
  double h;
  T* out;
  int64_t inco;
};

// the squared distance to the nearest support and the sum over the splits, in index order, of the sum `a` of bandwidth `b`
template <class T>
__device__ __forceinline__ double kde_dstar(const T* ws_min, int64_t nsplit, int64_t n_q, int64_t i) {
  T m = ws_min[i];
  for (int64_t q = 1; q < nsplit; ++q) m = fmin(m, ws_min[q * n_q + i]);
  return (double)m;
}
template <class T>
__device__ __forceinline__ double kde_split_sum(const T* ws_sum, int64_t nsplit, int nacc, int nb, int a, int b, int64_t n_q, int64_t i) {
  double s = 0.0;
  for (int64_t q = 0; q < nsplit; ++q) s += (double)ws_sum[((q * nacc + a) * nb + b) * n_q + i];
  return s;
}

constexpr double kKdeSqrt2Pi = 2.5066282746310005024;

// pdf_i = exp(-t*) S norm, logpdf_i = -t* + ln S + ln norm, norm = 1 / (n_s h sqrt(2 pi)); cdf_i = S / (2 n_s).  f64, one
// rounding to the element type at the store.  One thread per point.
template <class T>
__global__ __launch_bounds__(256) void kde_finish_kernel(KdeFinishArgs<T> g) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n_q) return;
  const double s = kde_split_sum(g.ws_sum, g.nsplit, 1, 1, 0, 0, g.n_q, i);
  double v;
  if (g.what == 1) {
    v = 0.5 * s / (double)g.n_s;
  } else {
    const double tstar = kde_dstar(g.ws_min, g.nsplit, g.n_q, i) / (2.0 * g.h * g.h);
    const double scale = (double)g.n_s * g.h * kKdeSqrt2Pi;
    v = g.what == 0 ? exp(-tstar) * s / scale : -tstar + log(s) - log(scale);
  }
  g.out[i * g.inco] = (T)v;
}

template <class T>
struct KdeNllArgs {
  const T* ws_min;  // [nsplit][n_t]
  const T* ws_sum;  // [nsplit][2][nb][n_t]
  int64_t nsplit, n_t, n_s, red_len;
  int nb, b_first;  // bandwidths of this launch, and the index of its first in the call
  unsigned red_blocks;
  double escale;    // the second sum in natural units: -ln 2 in f32 (e is a base-2 exponent), -1 in f64
  double h[kKdeHL];
  double* part;     // [n_h][red_blocks][2]
};

// a fixed tree over the 256 threads of a block; the result is in red[0]
__device__ __forceinline__ void kde_tree(double* red, int tid) {
  for (int w = 128; w > 0; w >>= 1) {
    __syncthreads();
    if (tid < w) red[tid] += red[tid + w];
  }
  __syncthreads();
}

// grid (red_blocks, nb): block (r, b) covers the points [r red_len, min(n_t, (r + 1) red_len)) for bandwidth b of the
// launch: thread t adds the points t, t + 256, ... of the range in that order, the tree adds the threads.
template <class T>
__global__ __launch_bounds__(256) void kde_nll_points_kernel(KdeNllArgs<T> g) {
  __shared__ double red[2][256];
  const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
  const int64_t i_begin = (int64_t)blockIdx.x * g.red_len, i_end = min(g.n_t, i_begin + g.red_len);
  const double h = g.h[b], c = 1.0 / (2.0 * h * h), lognorm = log((double)g.n_s * h * kKdeSqrt2Pi);
  double nl = 0.0, dn = 0.0;
  for (int64_t i = i_begin + tid; i < i_end; i += 256) {
    const double tstar = kde_dstar(g.ws_min, g.nsplit, g.n_t, i) * c;
    const double sk = kde_split_sum(g.ws_sum, g.nsplit, 2, g.nb, 0, b, g.n_t, i);
    const double se = kde_split_sum(g.ws_sum, g.nsplit, 2, g.nb, 1, b, g.n_t, i);
    const double r = 2.0 * (tstar + g.escale * se / sk);
    nl -= -tstar + log(sk) - lognorm;
    dn -= (r - 1.0) / h;
  }
  red[0][tid] = nl;
  red[1][tid] = dn;
  kde_tree(red[0], tid);
  kde_tree(red[1], tid);
  if (tid == 0) {
    double* out = g.part + ((int64_t)(g.b_first + b) * g.red_blocks + blockIdx.x) * 2;
    out[0] = red[0][0];
    out[1] = red[1][0];
  }
}

struct KdeReduceArgs {
  const double* part;  // [n_h][red_blocks][2]
  unsigned red_blocks;  // <= 256
  double* nll;          // n_h
  double* dnll;         // n_h, or nullptr
};

// grid n_h: the tree over the (at most 256) range partials of one bandwidth
__global__ __launch_bounds__(256) inline void kde_nll_reduce_kernel(KdeReduceArgs g) {
  __shared__ double red[2][256];
  const int tid = (int)threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x;
  const bool live = (unsigned)tid < g.red_blocks;
  red[0][tid] = live ? g.part[(b * g.red_blocks + tid) * 2] : 0.0;
  red[1][tid] = live ? g.part[(b * g.red_blocks + tid) * 2 + 1] : 0.0;
  kde_tree(red[0], tid);
  kde_tree(red[1], tid);
  if (tid == 0) {
    g.nll[b] = red[0][0];
    if (g.dnll) g.dnll[b] = red[1][0];
  }
}

}  // namespace k
}  // namespace corrla
