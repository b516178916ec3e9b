// CSR sparse operand of the range finder: Y (rows x L) = scale * S * X (cols x L) for a CSR matrix S, the device
// transposition of S, and the validation of a caller's CSR arrays.  gfx950, wave64.  These stand in for the two tall
// products of random_svd.rs:31,42-51,80 (par_matmul_helper, mat_utils.rs:20-33) when A is sparse.
//
// Scheme (row gather through a transposed X and an LDS output tile):
//   * Skinny operands are column-major, so the L values one nonzero (r, c, v) needs -- X(c, 0..L) -- lie ld elements
//     apart.  spmm_xt_kernel first writes X as a ROW-major scratch XT (cols x Lp, Lp = L rounded up to 16): one pass
//     over an l-wide matrix, after which the L values of a nonzero are one contiguous run and a wave (lane = sketch
//     column j) loads them with one coalesced access.
//   * spmm_rows_kernel: a workgroup owns a tile of 64 rows x 64 sketch columns; each of its four waves walks 16 rows.
//     The nonzeros of a row are fetched 64 at a time (coalesced loads of col_idx / values, one per lane) and broadcast
//     lane by lane, so the gather itself issues only XT loads.  The 64 x 64 results go through LDS and leave
//     transposed: the stores to the column-major Y are 64 consecutive rows of one column.
//   * Long rows (more than kSpLong nonzeros) are NOT walked by one wave: spmm_long_partial_kernel gives every chunk of
//     kSpLong nonzeros its own workgroup (work balanced over nonzeros) and spmm_long_reduce_kernel adds the partial
//     sums of a row in chunk order.  The lists of long rows and chunks are built once per matrix (csr_long_build).
//   * Every sum runs in a fixed order (position within the row; chunk, wave and chunk order for long rows): no
//     floating-point atomics, bitwise-reproducible results.  The integer atomics of the plan kernels only decide WHERE a
//     long row's partial sums are stored, never the order in which anything is added.
//   * Only rows [0, rows) x columns [0, L) of Y are written: the zero padding of a Skinny stays zero and nothing is
//     written past the columns of an external destination.
//   * Unsorted and duplicate column indices are legal (duplicates add).  No index is dereferenced before
//     csr_validate_kernel has checked it (tall_stage.hpp: csr_plan runs first and ends the call on a violation).
//
// Transposition: a stable LSD radix sort (8-bit digits) of the nonzero positions keyed by column index; stability keeps
// the entries of a column ordered by original row, then original position, which fixes the summation order of A^T Y.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gemm_plan.hpp"  // kSpTile (rows and sketch columns of one output tile), with the plan of the launches (spmm_plan)

namespace corrla {
namespace k {

constexpr int kSpLong = 2048;      // a row with more nonzeros is split into chunks of this many
constexpr int kSortTile = 4096;    // keys per (single-wave) workgroup of the radix sort

// written by csr_validate_kernel, read back by the host before anything is gathered
struct CsrCounts {
  int bad;  // bit 0: row_ptr[0] != 0, 1: row_ptr not monotone / out of [0, nnz], 2: row_ptr[m] != nnz, 3: index outside [0, n)
  int pad_;
  unsigned long long n_long, n_chunks;          // rows longer than kSpLong and the chunks they split into
  unsigned long long cursor_long, cursor_chunk; // csr_long_build_kernel's allocation cursors
};

// Reads row_ptr[0..m] and col_idx[0..nnz) only.
__global__ __launch_bounds__(256) void csr_validate_kernel(const int64_t* __restrict__ rp, const int32_t* __restrict__ ci, int64_t m,
                                                           int64_t n, int64_t nnz, int check_idx, CsrCounts* out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t top = m > nnz ? m : nnz;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < top; i += stride) {
    if (i < m) {
      const int64_t a = rp[i], b = rp[i + 1];
      if (a < 0 || b < a || b > nnz) {
        bad |= 2;
      } else if (b - a > kSpLong) {
        atomicAdd(&out->n_long, 1ull);
        atomicAdd(&out->n_chunks, (unsigned long long)((b - a + kSpLong - 1) / kSpLong));
      }
      if (i == 0 && a != 0) bad |= 1;
      if (i == m - 1 && b != nnz) bad |= 4;
    }
    if (check_idx && i < nnz) {
      const int32_t c = ci[i];
      if (c < 0 || (int64_t)c >= n) bad |= 8;
    }
  }
  if (bad) atomicOr(&out->bad, bad);
}

// Lists of the long rows (row, first chunk) and of their chunks (chunk -> entry of the long-row list).  Runs only on
// a row_ptr that passed csr_validate_kernel, so the totals equal the counts the host sized the lists with.
__global__ __launch_bounds__(256) void csr_long_build_kernel(const int64_t* __restrict__ rp, int64_t m, CsrCounts* cnt, int64_t* long_row,
                                                             int64_t* long_base, int32_t* chunk_long) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
    const int64_t len = rp[i + 1] - rp[i];
    if (len <= kSpLong) continue;
    const unsigned long long nch = (unsigned long long)((len + kSpLong - 1) / kSpLong);
    const unsigned long long idx = atomicAdd(&cnt->cursor_long, 1ull);
    const unsigned long long base = atomicAdd(&cnt->cursor_chunk, nch);
    long_row[idx] = i;
    long_base[idx] = (int64_t)base;
    for (unsigned long long c = 0; c < nch; ++c) chunk_long[base + c] = (int32_t)idx;
  }
}

// XT (rows x Lp, row-major) <- X (rows x L, column-major, ld); columns [L, Lp) of XT are zero.
template <class T>
__global__ __launch_bounds__(256) void spmm_xt_kernel(const T* __restrict__ x, int64_t ld, int64_t rows, int64_t L, T* __restrict__ xt,
                                                      int64_t Lp) {
  __shared__ T tile[kSpTile][kSpTile + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * kSpTile, j0 = (int64_t)blockIdx.y * kSpTile;
  for (int jj = wave * 16; jj < wave * 16 + 16; ++jj) {
    const int64_t j = j0 + jj, r = r0 + lane;
    tile[jj][lane] = (j < L && r < rows) ? x[j * ld + r] : (T)0;
  }
  __syncthreads();
  for (int rr = wave * 16; rr < wave * 16 + 16; ++rr) {
    const int64_t r = r0 + rr, j = j0 + lane;
    if (r < rows && j < Lp) xt[r * Lp + j] = tile[lane][rr];
  }
}

// sum over the nonzeros [a, b) of one row of v * XT(c, j), in position order; all 64 lanes of the wave take part
template <class T>
__device__ __forceinline__ T spmm_gather(const int32_t* __restrict__ ci, const T* __restrict__ val, const T* __restrict__ xt, int64_t Lp,
                                         int64_t a, int64_t b, int64_t j, bool jok, int lane) {
  T acc = (T)0;
  for (int64_t p = a; p < b; p += 64) {
    const int64_t pp = p + lane;
    int32_t c = 0;
    T v = (T)0;
    if (pp < b) {
      c = ci[pp];
      v = val[pp];
    }
    const int cnt = (int)((b - p) < 64 ? (b - p) : 64);
    for (int t = 0; t < cnt; ++t) {
      const int32_t cc = __shfl(c, t, 64);
      const T vv = __shfl(v, t, 64);
      if (jok) acc += vv * xt[(int64_t)cc * Lp + j];
    }
  }
  return acc;
}

template <class T>
__global__ __launch_bounds__(256) void spmm_rows_kernel(const int64_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                                        const T* __restrict__ val, const T* __restrict__ xt, int64_t Lp, int64_t rows,
                                                        int64_t L, T* __restrict__ y, int64_t ldy, const T* __restrict__ scale_dev) {
  __shared__ T tile[kSpTile][kSpTile + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * kSpTile, j0 = (int64_t)blockIdx.y * kSpTile;
  const int64_t j = j0 + lane;
  const bool jok = j < L;
  for (int rr = wave * 16; rr < wave * 16 + 16; ++rr) {
    const int64_t r = r0 + rr;
    T acc = (T)0;
    if (r < rows) {  // wave-uniform
      const int64_t a = rp[r], b = rp[r + 1];
      if (b - a <= kSpLong) acc = spmm_gather<T>(ci, val, xt, Lp, a, b, j, jok, lane);  // long rows: the two kernels below
    }
    tile[lane][rr] = acc;
  }
  __syncthreads();
  const T s = scale_dev ? *scale_dev : (T)1;
  for (int jj = wave * 16; jj < wave * 16 + 16; ++jj) {
    const int64_t jc = j0 + jj, r = r0 + lane;
    if (jc < L && r < rows) y[jc * ldy + r] = s * tile[jj][lane];
  }
}

// one workgroup per chunk of a long row: the four waves take a quarter of the chunk each, the quarters are added in
// wave order.  part: n_chunks x Lpart, row-major (Lpart = 64 * gridDim.y).
template <class T>
__global__ __launch_bounds__(256) void spmm_long_partial_kernel(const int64_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                                                const T* __restrict__ val, const T* __restrict__ xt, int64_t Lp, int64_t L,
                                                                const int64_t* __restrict__ long_row, const int64_t* __restrict__ long_base,
                                                                const int32_t* __restrict__ chunk_long, T* __restrict__ part,
                                                                int64_t Lpart) {
  __shared__ T red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q = blockIdx.x, j = (int64_t)blockIdx.y * 64 + lane;
  const int32_t li = chunk_long[q];
  const int64_t r = long_row[li];
  const int64_t a = rp[r] + (q - long_base[li]) * kSpLong;
  const int64_t end = rp[r + 1];
  const int64_t b = a + kSpLong < end ? a + kSpLong : end;
  const int64_t wa = a + (int64_t)wave * (kSpLong / 4);
  const int64_t wb = wa + kSpLong / 4 < b ? wa + kSpLong / 4 : b;
  red[wave][lane] = spmm_gather<T>(ci, val, xt, Lp, wa, wb, j, j < L, lane);  // (an empty range when wa >= b)
  __syncthreads();
  if (wave == 0) part[q * Lpart + j] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// Y(row, j) = scale * sum of the row's chunk sums, in chunk order
template <class T>
__global__ __launch_bounds__(64) void spmm_long_reduce_kernel(const int64_t* __restrict__ rp, const int64_t* __restrict__ long_row,
                                                              const int64_t* __restrict__ long_base, const T* __restrict__ part,
                                                              int64_t Lpart, int64_t L, T* __restrict__ y, int64_t ldy,
                                                              const T* __restrict__ scale_dev) {
  const int64_t li = blockIdx.x, j = (int64_t)blockIdx.y * 64 + threadIdx.x;
  const int64_t r = long_row[li], base = long_base[li];
  const int64_t nch = (rp[r + 1] - rp[r] + kSpLong - 1) / kSpLong;
  T acc = (T)0;
  for (int64_t c = 0; c < nch; ++c) acc += part[(base + c) * Lpart + j];
  const T s = scale_dev ? *scale_dev : (T)1;
  if (j < L) y[j * ldy + r] = s * acc;
}

// ---- transposition: stable LSD radix sort of (key = column index, payload = position) -----------------------------
// hist[d * nb + block] = number of keys of this block's tile whose digit is d
__global__ __launch_bounds__(64) void csr_radix_hist_kernel(const uint32_t* __restrict__ keys, int64_t nnz, int shift, uint32_t* hist,
                                                            int64_t nb) {
  __shared__ uint32_t h[256];
  const int lane = threadIdx.x;
  for (int d = lane; d < 256; d += 64) h[d] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kSortTile;
  for (int i = 0; i < kSortTile / 64; ++i) {
    const int64_t p = base + (int64_t)i * 64 + lane;
    if (p < nnz) atomicAdd(&h[(keys[p] >> shift) & 255u], 1u);
  }
  __syncthreads();
  for (int d = lane; d < 256; d += 64) hist[(int64_t)d * nb + blockIdx.x] = h[d];
}

// in-place exclusive prefix sum of N counts (their total is below 2^31); one workgroup
__global__ __launch_bounds__(1024) void csr_scan_kernel(uint32_t* a, int64_t N) {
  __shared__ uint32_t sh[1024];
  const int tid = threadIdx.x;
  const int64_t per = (N + 1023) / 1024;
  const int64_t s = (int64_t)tid * per < N ? (int64_t)tid * per : N;
  const int64_t e = s + per < N ? s + per : N;
  uint32_t sum = 0;
  for (int64_t i = s; i < e; ++i) sum += a[i];
  sh[tid] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const uint32_t v = tid >= off ? sh[tid - off] : 0u;
    __syncthreads();
    sh[tid] += v;
    __syncthreads();
  }
  uint32_t run = sh[tid] - sum;
  for (int64_t i = s; i < e; ++i) {
    const uint32_t t = a[i];
    a[i] = run;
    run += t;
  }
}

// One wave per tile, 64 keys per round in position order: a key's destination is the running offset of its digit plus
// the number of lower lanes of the round that hold the same digit -- a stable scatter.  pay_in == nullptr: the payload is
// the position itself (first pass).
__global__ __launch_bounds__(64) void csr_radix_scatter_kernel(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ pay_in,
                                                               int64_t nnz, int shift, const uint32_t* __restrict__ offs, int64_t nb,
                                                               uint32_t* __restrict__ keys_out, uint32_t* __restrict__ pay_out) {
  __shared__ uint32_t run[256];
  const int lane = threadIdx.x;
  for (int d = lane; d < 256; d += 64) run[d] = offs[(int64_t)d * nb + blockIdx.x];
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kSortTile;
  for (int i = 0; i < kSortTile / 64; ++i) {
    const int64_t p = base + (int64_t)i * 64 + lane;
    const bool active = p < nnz;
    const uint32_t key = active ? keys_in[p] : 0u;
    const uint32_t d = (key >> shift) & 255u;
    unsigned long long peers = __ballot(active);
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1u;
      const unsigned long long bm = __ballot(on);
      peers &= on ? bm : ~bm;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    uint32_t pos = 0;
    if (active) pos = run[d] + (uint32_t)rank;
    __syncthreads();
    if (active && rank == 0) run[d] += (uint32_t)__popcll(peers);
    __syncthreads();
    if (active) {
      keys_out[pos] = key;
      pay_out[pos] = pay_in ? pay_in[p] : (uint32_t)p;
    }
  }
}

// CSR of the transpose from the sorted (column, position) pairs: values and original row indices are gathered through
// the permutation (row of a position: binary search in row_ptr), and row_ptr of the transpose is read off the
// boundaries of the sorted keys (no atomics; empty columns are filled by the thread behind them).
template <class T>
__global__ __launch_bounds__(256) void csr_transpose_finish_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm,
                                                                   const int64_t* __restrict__ rp, int64_t m, const T* __restrict__ val,
                                                                   int64_t nnz, int64_t n, int64_t* __restrict__ t_rp,
                                                                   int32_t* __restrict__ t_ci, T* __restrict__ t_val) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nnz) return;
  const int64_t p = perm[q];
  t_val[q] = val[p];
  int64_t lo = 0, hi = m;  // largest r with rp[r] <= p
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (rp[mid] <= p)
      lo = mid;
    else
      hi = mid;
  }
  t_ci[q] = (int32_t)lo;
  const int64_t key = keys[q];
  const int64_t prev = q > 0 ? (int64_t)keys[q - 1] : -1;
  for (int64_t c = prev + 1; c <= key; ++c) t_rp[c] = q;
  if (q == nnz - 1)
    for (int64_t c = key + 1; c <= n; ++c) t_rp[c] = nnz;
}

}  // namespace k
}  // namespace corrla
