// Radial-basis-function kernel matrices on the device (interp_utils.rs:37-80, 96-129, 146-153): the product
// Phi(Xq, Xs) W with Phi_ij = phi(||xq_i - xs_j||_2) formed in registers and fed straight to the exact MFMAs
// (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 through MT<T>), and Phi itself.  The geometry is rbf_plan.hpp's.
//
// Distances are always the direct form s = sum_d (xq_id - xs_jd)^2, summed over d in index order with one fma per
// coordinate -- never ||a||^2 + ||b||^2 - 2 a.b, which cancels exactly where the linear and the cubic kernel need r -> 0.
// (a - b) and (b - a) differ in sign only, so s(i, j) == s(j, i) bitwise, and s(i, i) == 0.  Coordinates reach LDS through
// element loads: any row stride >= dim and any base alignment serve, there are no routes.
//
// rbf_apply_kernel<T, KERNEL>: one workgroup per (query tile of BM, column group of RG, split of the supports).  The
// tile's query coordinates go to LDS once; the split's supports are walked in chunks of KC: the chunk's coordinates and the
// matching KC x RG rows of W are staged, rows beyond the split's end and columns beyond n_rhs as zeros -- nothing is read
// out of bounds.  Wave w owns the queries 16 w .. 16 w + 15 of the tile: a lane evaluates phi for the pairs of its MFMA
// A-operand slots (row lane & 15, reduction slot kq = lane >> 4; of a chunk the slot kq holds the KC / 4 consecutive
// supports from KC / 4 * kq on) and issues the MFMAs against the staged W for every live column tile of the group, so one
// phi evaluation serves up to 64 output columns.  A support slot beyond the split's end contributes zero: its phi is set
// to zero (phi(r) of the multiquadric and the Gaussian is not) and its W row is zero.
// The accumulators go to the split's partial in workspace; rbf_finish_kernel adds the splits in index order, adds the
// polynomial tail and writes out once.  No atomics: a fixed input gives a bitwise fixed output.
// rbf_matrix_kernel<T, KERNEL>: out[i, j] = phi(s(i, j)), BM x MN per workgroup with the same staging and the same rbf_phi,
// stores coalesced along the supports.  With Xq == Xs the result equals its transpose bitwise and its diagonal is phi(0).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_kernels.hpp"  // MT<T>
#include "rbf_plan.hpp"

namespace corrla {
namespace k {

// phi from the SQUARED distance s (interp_utils.rs:37-80): 1 linear r, 2 multiquadric sqrt(1 + (eps r)^2), 3 cubic r^3,
// 4 Gaussian exp(-(eps r)^2).  The library sqrt / exp of the type (<= 2 ulp), not the fast intrinsics.  `kernel` is a
// template argument of every caller: the switch folds away.
template <class T>
__device__ __forceinline__ T rbf_phi(int kernel, T s, T eps) {
  switch (kernel) {
    case 1:
      return sqrt(s);
    case 2:
      return sqrt((T)1 + (eps * eps) * s);
    case 3: {
      const T r = sqrt(s);
      return r * r * r;
    }
    default:
      return exp(-((eps * eps) * s));
  }
}

template <class T>
struct RbfApplyArgs {
  const T* xq;  // n_q x dim, row stride ldq
  int64_t ldq;
  const T* xs;  // n_s x dim, row stride ldxs
  int64_t ldxs;
  const T* w;   // n_s x n_rhs, row stride ldw (W_rbf: the first n_s rows of the coefficients)
  int64_t ldw;
  int64_t n_q, n_s, n_rhs;
  int dim;
  T eps;
  int64_t nbm, nrg, split_len;
  T* ws;        // [split][n_q][n_rhs]
};

// One staged chunk for one lane: the squared distances of the lane's query (row qr of the tile) to its NS = KC / 4 supports
// NS kq + i grow together, one coordinate at a time (index order), from one LDS read of the query's coordinate and one wide
// read of the supports'; then MFMA step i reduces over the supports NS kq + i of the four kq, against NT column tiles of the
// staged W.  No branch: a slot beyond the chunk's kv supports has phi = 0 and a zero W row.
template <class T, int KERNEL, int NT>
__device__ __forceinline__ void rbf_chunk(const T* lds_q, const T* lds_s, const T* lds_w, int dim, int qr, int kq, int fc, int kv, T eps,
                                          typename MT<T>::acc_t (&acc)[4]) {
  constexpr int BM = kRbfBM, KC = kRbfKC, WLD = kRbfWLd, NS = KC / 4;
  T s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = (T)0;
  for (int d = 0; d < dim; ++d) {
    const T q = lds_q[d * BM + qr];
    T x[NS];
    __builtin_memcpy(x, __builtin_assume_aligned(lds_s + d * KC + NS * kq, 16), sizeof(x));
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const T diff = q - x[i];
      s[i] = __builtin_fma(diff, diff, s[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int j = NS * kq + i;
    const T phi = j < kv ? rbf_phi<T>(KERNEL, s[i], eps) : (T)0;
    const T* pw = lds_w + j * WLD + fc;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = MT<T>::mma(phi, pw[16 * t], acc[t]);
  }
}

// (at least three waves per SIMD: left alone, the compiler interleaves the eight sqrt / exp expansions of a chunk and takes
// more than 200 f64 registers for it -- two waves per SIMD; held to three it takes 115 to 138 and needs no scratch)
template <class T, int KERNEL>
__global__ __launch_bounds__(kRbfThreads) __attribute__((amdgpu_waves_per_eu(3, 8))) void rbf_apply_kernel(RbfApplyArgs<T> g) {
  constexpr int BM = kRbfBM, KC = kRbfKC, RG = kRbfRG, WLD = kRbfWLd;
  static_assert(BM == 64 && RG == 64 && kRbfThreads == 256 && KC % 16 == 0, "four waves of 16 queries x 4 column tiles");
  typedef typename MT<T>::acc_t acc_t;
  extern __shared__ uint4 rbf_smem[];
  const int dim = g.dim;
  T* lds_w = reinterpret_cast<T*>(rbf_smem);  // [KC][WLD]
  T* lds_q = lds_w + KC * WLD;                // [dim][BM]
  T* lds_s = lds_q + dim * BM;                // [dim][KC]
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, fc = lane & 15, kq = lane >> 4;
  int64_t wg = (int64_t)blockIdx.x;
  const int64_t bi = wg % g.nbm;
  wg /= g.nbm;
  const int64_t rgi = wg % g.nrg, sp = wg / g.nrg;
  const int64_t row0 = bi * BM, col0 = rgi * RG;
  const int64_t j_begin = sp * g.split_len, j_end = min(g.n_s, j_begin + g.split_len);
  const int ntile = (int)((min((int64_t)RG, g.n_rhs - col0) + 15) / 16);  // live column tiles of this group, 1..4

  for (int e = tid; e < BM * dim; e += kRbfThreads) {
    const int r = e / dim, d = e - r * dim;
    const int64_t row = row0 + r;
    lds_q[d * BM + r] = row < g.n_q ? g.xq[row * g.ldq + d] : (T)0;
  }
  const int qr = 16 * wave + fc;  // the lane's query row of the tile

  acc_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = acc_t{0, 0, 0, 0};

  for (int64_t j0 = j_begin; j0 < j_end; j0 += KC) {
    const int kv = (int)min((int64_t)KC, j_end - j0);  // supports of this chunk; the slots beyond are staged as zeros
    for (int e = tid; e < KC * dim; e += kRbfThreads) {
      const int j = e / dim, d = e - j * dim;
      lds_s[d * KC + j] = j < kv ? g.xs[(j0 + j) * g.ldxs + d] : (T)0;
    }
    for (int e = tid; e < KC * RG; e += kRbfThreads) {
      const int j = e / RG, c = e % RG;
      lds_w[j * WLD + c] = (j < kv && col0 + c < g.n_rhs) ? g.w[(j0 + j) * g.ldw + col0 + c] : (T)0;
    }
    __syncthreads();
    switch (ntile) {  // uniform, once per chunk: the compute of a chunk is straight-line code for its count of column tiles
      case 1: rbf_chunk<T, KERNEL, 1>(lds_q, lds_s, lds_w, dim, qr, kq, fc, kv, g.eps, acc); break;
      case 2: rbf_chunk<T, KERNEL, 2>(lds_q, lds_s, lds_w, dim, qr, kq, fc, kv, g.eps, acc); break;
      case 3: rbf_chunk<T, KERNEL, 3>(lds_q, lds_s, lds_w, dim, qr, kq, fc, kv, g.eps, acc); break;
      default: rbf_chunk<T, KERNEL, 4>(lds_q, lds_s, lds_w, dim, qr, kq, fc, kv, g.eps, acc); break;
    }
    __syncthreads();
  }

  // D of column tile t: row = drow(lane, r) <-> query row0 + 16 wave + row; col = fc <-> column col0 + 16 t + fc
  T* part = g.ws + sp * g.n_q * g.n_rhs;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = row0 + 16 * wave + MT<T>::drow(lane, r);
    if (row >= g.n_q) continue;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t col = col0 + 16 * t + fc;
      if (col < g.n_rhs) part[row * g.n_rhs + col] = acc[t][r];
    }
  }
}

template <class T>
struct RbfFinishArgs {
  const T* ws;  // [nsplit][n_q][n_rhs]
  int64_t nsplit, n_q, n_rhs;
  const T* xq;  // the queries, for the tail
  int64_t ldq;
  int dim;
  int tail;     // 0 none, 1 [x, 1], 2 [x, x_a x_b (a <= b, a outer), 1]
  const T* wp;  // W_poly: the rows of the coefficients behind W_rbf, row stride ldw
  int64_t ldw;
  T* out;
  int64_t ld_out;
};

// out[i, c] = sum over the splits, in index order (f64), of the partials, + the polynomial tail P(xq_i) W_poly[:, c] with the
// terms in build_full_vandermonde's order.  One thread per (query, column); the padding columns of out are not touched.
template <class T>
__global__ __launch_bounds__(256) void rbf_finish_kernel(RbfFinishArgs<T> g) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= g.n_q * g.n_rhs) return;
  const int64_t i = idx / g.n_rhs, c = idx - i * g.n_rhs;
  double s = 0.0;
  for (int64_t sp = 0; sp < g.nsplit; ++sp) s += (double)g.ws[(sp * g.n_q + i) * g.n_rhs + c];
  if (g.tail) {
    const T* x = g.xq + i * g.ldq;
    const T* wp = g.wp + c;
    int64_t t = 0;
    for (int d = 0; d < g.dim; ++d, ++t) s += (double)x[d] * (double)wp[t * g.ldw];
    if (g.tail == 2)
      for (int a = 0; a < g.dim; ++a)
        for (int b = a; b < g.dim; ++b, ++t) s += (double)x[a] * (double)x[b] * (double)wp[t * g.ldw];
    s += (double)wp[t * g.ldw];
  }
  g.out[i * g.ld_out + c] = (T)s;
}

template <class T>
struct RbfMatrixArgs {
  const T* xq;
  int64_t ldq;
  const T* xs;
  int64_t ldxs;
  int64_t n_q, n_s;
  int dim;
  T eps;
  int64_t nbs;  // support tiles
  T* out;       // n_q x n_s, row stride ld_out
  int64_t ld_out;
};

template <class T, int KERNEL>
__global__ __launch_bounds__(kRbfThreads) void rbf_matrix_kernel(RbfMatrixArgs<T> g) {
  constexpr int BM = kRbfBM, MN = kRbfMN;
  static_assert(MN == 64 && kRbfThreads == 256 && BM % 4 == 0, "a wave per row, 64 supports wide");
  extern __shared__ uint4 rbf_smem[];
  const int dim = g.dim;
  T* lds_q = reinterpret_cast<T*>(rbf_smem);  // [dim][BM]
  T* lds_s = lds_q + dim * BM;                // [dim][MN]
  const int tid = (int)threadIdx.x;
  const int64_t bi = (int64_t)blockIdx.x / g.nbs, bj = (int64_t)blockIdx.x % g.nbs;
  const int64_t row0 = bi * BM, col0 = bj * MN;
  for (int e = tid; e < BM * dim; e += kRbfThreads) {
    const int r = e / dim, d = e - r * dim;
    const int64_t row = row0 + r;
    lds_q[d * BM + r] = row < g.n_q ? g.xq[row * g.ldq + d] : (T)0;
  }
  for (int e = tid; e < MN * dim; e += kRbfThreads) {
    const int j = e / dim, d = e - j * dim;
    const int64_t col = col0 + j;
    lds_s[d * MN + j] = col < g.n_s ? g.xs[col * g.ldxs + d] : (T)0;
  }
  __syncthreads();
  const int j = tid & 63;
  const int64_t col = col0 + j;
  if (col >= g.n_s) return;
  for (int r = tid >> 6; r < BM; r += 4) {
    const int64_t row = row0 + r;
    if (row >= g.n_q) break;
    T s = (T)0;
    for (int d = 0; d < dim; ++d) {
      const T diff = lds_q[d * BM + r] - lds_s[d * MN + j];
      s = __builtin_fma(diff, diff, s);
    }
    g.out[row * g.ld_out + col] = rbf_phi<T>(KERNEL, s, g.eps);
  }
}

}  // namespace k
}  // namespace corrla
