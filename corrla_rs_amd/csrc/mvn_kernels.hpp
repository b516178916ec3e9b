// Multivariate normal rows x_i = mu + F z_i (corrla_mvn_sample_*; sample_mv_normal, stats_corr.rs:46-58) and the sandwich
// variances v_i = j_i^T C j_i (corrla_sandwich_diag_*; the diagonal of sandwich_prop, stats_corr.rs:64-68) on the exact MFMAs
// (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 through MT<T>).  The geometry is mvn_plan.hpp's.
//
// Both kernels are one skeleton.  A workgroup owns BM rows and every column.  Its row tile -- the BM x r normals, generated
// here and never stored to global memory, or the BM x d gradients -- is written ONCE into a k-major LDS image (mvn_zoff),
// rows beyond the matrix and reduction indices up to the next multiple of 4 as zeros.  Then it walks the columns BN at a time
// (mvn_tile_product): the small matrix (F^T as r rows of d features, C as it lies) is staged KC reduction rows at a time,
// columns beyond the matrix as zeros -- nothing is read out of bounds -- and each wave accumulates its 16 rows x 64 columns
// as four MFMA tiles; tile tj of a lane holds column 4 fc + tj (fc = lane & 15), so the lane's four values of a row are four
// consecutive columns: one 16-byte (f32) / two 16-byte (f64) stores.
//   mvn_fused_kernel:    out = acc + mu, written once.
//   sandwich_kernel:     acc (a tile of J C) times the matching entries of the staged J tile, summed over the lane's columns
//                        tile after tile in column order, over the 16 lanes of a row by a fixed shuffle tree, over the wave
//                        columns through LDS in index order; one value per row is written.
// No atomics, no m x d temporary: a fixed input gives a bitwise fixed output.
//
// LOWER (the factor is a Cholesky factor, F[c][k] = 0 for k > c; mvn_pack_factor_kernel writes those zeros itself): the
// chunks beyond the last column of the pass are not staged and a wave leaves the chunk at the first MFMA step whose four
// reduction indices all lie beyond its own last column.  The steps that remain are the same steps on the same operands in the
// same order, and the skipped ones would have added products with exact zeros: the bits of the dense walk.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_kernels.hpp"         // MT<T>, normal_from_index<T>
#include "mvn_plan.hpp"
#include "pca_apply_kernels.hpp"   // pca_store4

namespace corrla {
namespace k {

// Element (reduction index kk, tile row) of the row-tile image.  The MFMA A operand is read by 16 consecutive rows for each of
// four consecutive kk; rows a multiple of 32 elements apart share their banks, so odd kk swap the two 16-row halves of
// every 32 rows and the two kk of a 32-lane group never meet.
template <int BM>
__device__ __forceinline__ int mvn_zoff(int kk, int row) {
  return kk * BM + (row ^ ((kk & 1) << 4));
}

// acc = (row tile) x b[:, col0 : col0 + BN): b holds kdim rows of ncols contiguous elements, row stride ldb.
// Ends with a barrier: lds_b is free when it returns.
template <class T, int BM, bool LOWER>
__device__ __forceinline__ void mvn_tile_product(const T* lds_a, T* lds_b, const T* __restrict__ b, int64_t ldb, int kdim, int64_t ncols,
                                                 int64_t col0, typename MT<T>::acc_t (&acc)[4]) {
  constexpr int BN = mvn_bn(BM), KC = mvn_kc((int)sizeof(T)), WI = BM / 16;
  typedef typename MT<T>::acc_t acc_t;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave % WI, wj = wave / WI, fc = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = acc_t{0, 0, 0, 0};
  // LOWER: reduction indices at or beyond the end of the pass (of the wave's columns) meet zeros of F only
  const int kend = LOWER ? (int)min((int64_t)kdim, col0 + BN) : kdim;
  const int kwave = LOWER ? (int)min((int64_t)kdim, col0 + 64 * wj + 64) : kdim;
  for (int k0 = 0; k0 < kend; k0 += KC) {
    const int kv = min(KC, kend - k0);
    const int kpad = (kv + 3) & ~3;
    for (int e = tid; e < kpad * BN; e += kMvnThreads) {
      const int kk = e / BN;
      const int64_t col = col0 + (e % BN);
      lds_b[e] = (kk < kv && col < ncols) ? b[(int64_t)(k0 + kk) * ldb + col] : (T)0;
    }
    __syncthreads();
    const T* pb = lds_b + kq * BN + 64 * wj + 4 * fc;
    for (int ks = 0; ks < kpad / 4; ++ks) {
      if (LOWER && k0 + 4 * ks >= kwave) break;  // the same for every lane of the wave
      const T a = lds_a[mvn_zoff<BM>(k0 + 4 * ks + kq, 16 * wi + fc)];
      T bv[4];
      __builtin_memcpy(bv, pb + ks * 4 * BN, sizeof(bv));
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) acc[tj] = MT<T>::mma(a, bv[tj], acc[tj]);
    }
    __syncthreads();
  }
}

template <class T>
struct MvnArgs {
  const T* ft;    // F^T: r rows of d contiguous features (mvn_pack_factor_kernel)
  int64_t ldft;
  const T* mu;    // d means, or nullptr (0)
  int64_t n, d;
  int r;
  uint64_t seed;
  int64_t first;  // stream row of output row 0: z_i[j] = normal_from_index<T>((first + i) r + j, seed)
  T* out;
  int64_t ldo;
  int wide;       // 16-byte stores of out are legal
};

template <class T, int BM, bool LOWER>
__global__ __launch_bounds__(kMvnThreads) void mvn_fused_kernel(MvnArgs<T> g) {
  constexpr int BN = mvn_bn(BM), WI = BM / 16;
  static_assert(BM == 64 || BM == 32, "four waves as (BM / 16) x (64 / BM)");
  typedef typename MT<T>::acc_t acc_t;
  extern __shared__ uint4 mvn_smem[];
  const int rpad = (g.r + 3) & ~3;
  T* lds_z = reinterpret_cast<T*>(mvn_smem);  // [rpad][BM], mvn_zoff
  T* lds_f = lds_z + rpad * BM;               // [KC][BN]
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave % WI, wj = wave / WI, fc = lane & 15;
  const int64_t row0 = (int64_t)blockIdx.x * BM;

  // every normal of the tile once; consecutive threads take consecutive rows of one reduction index
  for (int e = tid; e < rpad * BM; e += kMvnThreads) {
    const int kk = e / BM, lr = e % BM;
    const int64_t row = row0 + lr;
    T z = (T)0;
    if (kk < g.r && row < g.n) z = normal_from_index<T>((uint64_t)(g.first + row) * (uint64_t)g.r + (uint64_t)kk, g.seed);
    lds_z[mvn_zoff<BM>(kk, lr)] = z;
  }
  __syncthreads();

  for (int64_t col0 = 0; col0 < g.d; col0 += BN) {
    acc_t acc[4];
    mvn_tile_product<T, BM, LOWER>(lds_z, lds_f, g.ft, g.ldft, g.r, g.d, col0, acc);
    const int64_t c0 = col0 + 64 * wj + 4 * fc;
    const int nv = c0 < g.d ? (int)min((int64_t)4, g.d - c0) : 0;
    const bool vec = g.wide && nv == 4;
    T mu4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) mu4[u] = (g.mu && u < nv) ? g.mu[c0 + u] : (T)0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t row = row0 + 16 * wi + MT<T>::drow(lane, q);
      if (row < g.n && nv > 0) {
        T o[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) o[u] = acc[u][q] + mu4[u];
        pca_store4<T>(g.out + row * g.ldo + c0, vec, nv, o);
      }
    }
  }
}

template <class T>
struct SandwichArgs {
  const T* jac;  // m x d, unit stride along d
  int64_t ldj;
  const T* cov;  // d x d as given: never symmetrised
  int64_t ldc;
  int64_t m;
  int d;
  T* v;          // m values
};

template <class T, int BM>
__global__ __launch_bounds__(kMvnThreads) void sandwich_kernel(SandwichArgs<T> g) {
  constexpr int BN = mvn_bn(BM), WI = BM / 16, WJ = 64 / BM, KC = mvn_kc((int)sizeof(T));
  static_assert(BM == 64 || BM == 32, "four waves as (BM / 16) x (64 / BM)");
  static_assert(WJ * BM <= KC * BN, "the row partials reuse the staging image");
  typedef typename MT<T>::acc_t acc_t;
  extern __shared__ uint4 mvn_smem[];
  const int dpad = (g.d + 3) & ~3;
  T* lds_j = reinterpret_cast<T*>(mvn_smem);  // [dpad][BM], mvn_zoff
  T* lds_c = lds_j + dpad * BM;               // [KC][BN]
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave % WI, wj = wave / WI, fc = lane & 15;
  const int64_t row0 = (int64_t)blockIdx.x * BM;

  // consecutive threads read consecutive features of one row
  for (int e = tid; e < dpad * BM; e += kMvnThreads) {
    const int a = e % dpad, lr = e / dpad;
    const int64_t row = row0 + lr;
    lds_j[mvn_zoff<BM>(a, lr)] = (a < g.d && row < g.m) ? g.jac[row * g.ldj + a] : (T)0;
  }
  __syncthreads();

  T s[4] = {(T)0, (T)0, (T)0, (T)0};  // of the rows 16 wi + drow(lane, q)
  for (int col0 = 0; col0 < g.d; col0 += BN) {
    acc_t acc[4];
    mvn_tile_product<T, BM, false>(lds_j, lds_c, g.cov, g.ldc, g.d, (int64_t)g.d, (int64_t)col0, acc);
    const int c0 = col0 + 64 * wj + 4 * fc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int lrow = 16 * wi + MT<T>::drow(lane, q);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (c0 + u < g.d) s[q] += acc[u][q] * lds_j[mvn_zoff<BM>(c0 + u, lrow)];
    }
  }
  T* red = lds_c;  // [WJ][BM]: the last barrier of the product freed the staging image
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    T t = s[q];
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) t += __shfl_xor(t, off, 16);
    if (fc == 0) red[wj * BM + 16 * wi + MT<T>::drow(lane, q)] = t;
  }
  __syncthreads();
  if (tid < BM && row0 + tid < g.m) {
    T t = red[tid];
#pragma unroll
    for (int w = 1; w < WJ; ++w) t += red[w * BM + tid];
    g.v[row0 + tid] = t;
  }
}

// ft[kk][c] = f[c][kk] (f: d rows of r, row stride ldf), zero for c >= d up to ldft and, lower, for kk > c: the strict upper
// triangle of a lower-triangular factor is never read.
template <class T>
__global__ __launch_bounds__(256) void mvn_pack_factor_kernel(const T* __restrict__ f, int64_t d, int64_t r, int64_t ldf, int lower,
                                                              T* __restrict__ ft, int64_t ldft) {
  const int64_t total = r * ldft;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t kk = t / ldft, c = t - kk * ldft;
    ft[t] = (c < d && !(lower && kk > c)) ? f[c * ldf + kk] : (T)0;
  }
}

}  // namespace k
}  // namespace corrla
