// The fitted PCA model applied backwards (pca_rsvd.rs:49-52): the product t V of the m x k scores with the k x n components on
// the exact MFMAs (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 through MT<T>), finished in registers as the
// reconstruction (STORE) or as the per-sample Q-residual against x (RESID).  The geometry is pca_apply_plan.hpp's.
//
// pca_back_kernel<T, MODE>: one workgroup per BM x BN tile of the m x n plane.  k is walked in chunks of KC: the chunk's
// rows of t (column-major: contiguous along the samples) and of V (staged by the caller as k rows of n contiguous features)
// go to two k-major LDS images; rows and columns beyond the matrix and the components beyond a chunk's end, up to the next
// multiple of 4, are written as zeros -- nothing is read out of bounds.  Each of the four waves owns 32 x 64 of the tile as
// 2 x 4 MFMA tiles; tile (ti, tj) of a lane belongs to row 2 i + ti and column 4 fc + tj (fc = lane & 15), so the operand
// values of a reduction index are ONE LDS read per operand for 8 MFMAs and the four tj of a lane are four consecutive
// features: one 16-byte (f32) / two 16-byte (f64) accesses of the m x n operand.
//   STORE: out = acc sigma_j + mu_j.
//   RESID: (x_ij - mu_j) / sigma_j - acc, squared and summed along the row: over the lane's columns, over the 16 lanes of a
//          row by a fixed shuffle tree, over the two wave columns through LDS; the row partial of the tile goes to workspace
//          and pca_resid_finish_kernel adds the column tiles in index order.
// No atomics: a fixed input gives a bitwise fixed output.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_kernels.hpp"  // MT<T>
#include "pca_apply_plan.hpp"

namespace corrla {
namespace k {

constexpr int kPcaStore = 0, kPcaResid = 1;

template <class T>
struct PcaBackArgs {
  const T* t;     // scores, m x k column-major
  int64_t ldt;
  const T* v;     // components, k rows of n contiguous features
  int64_t ldv;
  const T* mu;    // n means, or nullptr (0)
  const T* sd;    // n scales, or nullptr (1)
  int64_t m, n, k, nbn;
  T* big;         // STORE: out (written); RESID: x (read), m x n with unit stride along the features
  int64_t ld;
  int wide;       // 16-byte accesses of `big` are legal: base 16-byte aligned and ld a multiple of the vector width
  T* ws;          // RESID: [column tile][m] row partials
};

template <class T>
__device__ __forceinline__ void pca_load4(const T* p, bool vec, int nv, T (&e)[4]) {
  if (vec) {
    if constexpr (sizeof(T) == 4) {
      const uint4 raw = *reinterpret_cast<const uint4*>(p);
      __builtin_memcpy(e, &raw, sizeof(raw));
    } else {
      uint4 raw[2] = {reinterpret_cast<const uint4*>(p)[0], reinterpret_cast<const uint4*>(p)[1]};
      __builtin_memcpy(e, raw, sizeof(raw));
    }
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) e[u] = u < nv ? p[u] : (T)0;
  }
}

template <class T>
__device__ __forceinline__ void pca_store4(T* p, bool vec, int nv, const T (&e)[4]) {
  if (vec) {
    if constexpr (sizeof(T) == 4) {
      uint4 raw;
      __builtin_memcpy(&raw, e, sizeof(raw));
      *reinterpret_cast<uint4*>(p) = raw;
    } else {
      uint4 raw[2];
      __builtin_memcpy(raw, e, sizeof(raw));
      reinterpret_cast<uint4*>(p)[0] = raw[0];
      reinterpret_cast<uint4*>(p)[1] = raw[1];
    }
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (u < nv) p[u] = e[u];
  }
}

template <class T, int MODE>
__global__ __launch_bounds__(kPcaBackThreads) void pca_back_kernel(PcaBackArgs<T> g) {
  constexpr int BM = kPcaBackBM, BN = kPcaBackBN, KC = pca_back_kc((int)sizeof(T));
  static_assert(BM == 64 && BN == 128 && kPcaBackThreads == 256, "2 x 2 waves of 32 x 64");
  static_assert(2 * BM <= KC * (BM + BN), "the row partials of RESID reuse the staging images");
  typedef typename MT<T>::acc_t acc_t;
  extern __shared__ uint4 pca_back_smem[];
  T* lds_t = reinterpret_cast<T*>(pca_back_smem);  // [KC][BM]
  T* lds_v = lds_t + KC * BM;                      // [KC][BN]
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1, fc = lane & 15, kq = lane >> 4;
  const int64_t bi = (int64_t)blockIdx.x / g.nbn, bj = (int64_t)blockIdx.x % g.nbn;
  const int64_t row0 = bi * BM, col0 = bj * BN;

  acc_t acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = acc_t{0, 0, 0, 0};

  for (int64_t k0 = 0; k0 < g.k; k0 += KC) {
    const int kv = (int)min((int64_t)KC, g.k - k0);  // components of this chunk
    const int kpad = (kv + 3) & ~3;                  // ... zero-padded to whole MFMAs
    for (int e = tid; e < kpad * BM; e += kPcaBackThreads) {
      const int kk = e / BM;
      const int64_t row = row0 + (e % BM);
      lds_t[e] = (kk < kv && row < g.m) ? g.t[(k0 + kk) * g.ldt + row] : (T)0;
    }
    for (int e = tid; e < kpad * BN; e += kPcaBackThreads) {
      const int kk = e / BN;
      const int64_t col = col0 + (e % BN);
      lds_v[e] = (kk < kv && col < g.n) ? g.v[(k0 + kk) * g.ldv + col] : (T)0;
    }
    __syncthreads();
    const T* pa = lds_t + kq * BM + 32 * wi + 2 * fc;
    const T* pb = lds_v + kq * BN + 64 * wj + 4 * fc;
    for (int ks = 0; ks < kpad / 4; ++ks) {
      T a[2], b[4];
      __builtin_memcpy(a, pa + ks * 4 * BM, sizeof(a));
      __builtin_memcpy(b, pb + ks * 4 * BN, sizeof(b));
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = MT<T>::mma(a[ti], b[tj], acc[ti][tj]);
    }
    __syncthreads();
  }

  // D of MFMA tile (ti, tj): row = drow(lane, r) <-> tile row 32 wi + 2 row + ti; col = fc <-> tile column 64 wj + 4 fc + tj.
  // mu and sigma of the lane's four columns: loaded once per tile.
  const int64_t c0 = col0 + 64 * wj + 4 * fc;
  const int nv = c0 < g.n ? (int)min((int64_t)4, g.n - c0) : 0;
  const bool vec = g.wide && nv == 4;
  T mu4[4], sd4[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    mu4[u] = (g.mu && u < nv) ? g.mu[c0 + u] : (T)0;
    sd4[u] = (g.sd && u < nv) ? g.sd[c0 + u] : (T)1;
  }
  T* red = lds_t;  // RESID: [2][BM] row partials of the two wave columns (the last barrier of the loop freed the images)
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lrow = 32 * wi + 2 * MT<T>::drow(lane, r) + ti;
      const int64_t row = row0 + lrow;
      const bool live = row < g.m && nv > 0;
      if (MODE == kPcaStore) {
        if (live) {
          T o[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) o[u] = acc[ti][u][r] * sd4[u] + mu4[u];
          pca_store4<T>(g.big + row * g.ld + c0, vec, nv, o);
        }
      } else {
        T s = (T)0;
        if (live) {
          T xv[4];
          pca_load4<T>(g.big + row * g.ld + c0, vec, nv, xv);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const T d = (xv[u] - mu4[u]) / sd4[u] - acc[ti][u][r];
            if (u < nv) s += d * d;
          }
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 16);
        if (fc == 0) red[wj * BM + lrow] = s;
      }
    }
  if (MODE == kPcaResid) {
    __syncthreads();
    if (tid < BM && row0 + tid < g.m) g.ws[bj * g.m + row0 + tid] = red[tid] + red[BM + tid];
  }
}

// q[i] = sum over the column tiles, in index order (f64), of the row partials
template <class T>
__global__ __launch_bounds__(256) void pca_resid_finish_kernel(const T* __restrict__ ws, int64_t nbn, int64_t m, T* __restrict__ q) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double s = 0.0;
  for (int64_t b = 0; b < nbn; ++b) s += (double)ws[b * m + i];
  q[i] = (T)s;
}

// inv[j] = 1 / sd[j]: the diagonal the fused and the copy centring multiply with
template <class T>
__global__ __launch_bounds__(256) void pca_reciprocal_kernel(const T* __restrict__ sd, int64_t n, T* __restrict__ inv) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) inv[j] = (T)1 / sd[j];
}

}  // namespace k
}  // namespace corrla
