// The gradient stage's WIDE kernels (grad_plan.hpp): the calls the limited kernels of grad_kernels.hpp and
// knn2_kernels.hpp cannot take -- any number of features k, any number of neighbours n_nbrs <= n_pts, any design width.
//
// knn_wide_kernel: exact brute-force n nearest neighbours, the contract of knn_kernel.  A workgroup owns kWsQ queries and
//   walks the support points in chunks of 64; the feature dimension is streamed in LDS-staged slices of kWsDs, so k has no
//   cap.  Each thread holds a 4 x 4 block of the 64 x 64 distance tile in registers and accumulates  dist += df * df,
//   df = p_d - q_d,  over d in order: the same sequential f64 sum as knn_kernel, so both scans see the same distances and
//   agree on ties.  Direct differences instead of |q|^2 + |p|^2 - 2 q.p need no filter margin, no centring and no
//   re-check, and hold at any coordinate scale f64 can square (1e-25 .. 1e+25 included).  Each query's sorted list
//   (distance, index) lives in global memory, of any length (the distances in a workspace, the indices in the output);
//   pairs below the list's current n-th entry tau go to a candidate buffer, and a flush -- one wave per query -- sorts the
//   candidates (bitonic, LDS), merges them into the list in place and refreshes tau.  Order is (distance, index);
//   non-finite distances count as +inf and so sort last, behind every finite one.
// grad_fit_wide_kernel: the least-squares fit of grad_fit_kernel for any number of design columns P, one query per
//   workgroup of 256 threads on a bounded persistent grid.  The workgroup's global-memory slice holds the augmented normal
//   equations [D y]^T [D y] (lower triangle), formed in 64 x 64 tiles from 32-neighbour chunks whose design columns --
//   x - x0, the products (x_a - x0_a)(x_b - x0_b) of order 2, the constant, y -- are generated while they are staged and
//   never stored.  Jacobi scaling makes the diagonal one; a right-looking blocked Cholesky (64-column panels: diagonal
//   block and its inverse in LDS, panel and trailing update as tiled products) factors it, and since the right-hand side
//   is the last row of the augmented matrix, that row of the factor is L^-1 D^T y.  One blocked back substitution gives
//   the coefficients; the first k, unscaled, are the gradient (grad_kernels.hpp explains why).  A failed pivot retries
//   with a 1e-10 relative ridge; a second failure writes a zero gradient (status 1 and 2, as grad_fit_kernel).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grad_plan.hpp"

namespace corrla {
namespace k {

struct WideScanArgs {
  const double* x;   // n_pts x k, row-major
  const double* xq;  // n_q x k, row-major
  int64_t n_pts, n_q, n_nbrs, ntiles;
  int k;
  double* list_d;    // [gridDim.x][kWsQ][n_nbrs] sorted distances
  double* cand_d;    // [gridDim.x][kWsQ][kWsCap]
  int* cand_i;       // [gridDim.x][kWsQ][kWsCap]
  int* nbr;          // [n_q][n_nbrs] output: the indices of the sorted lists
};

// (d, i) < (e, j) in the list order
__device__ __forceinline__ bool ws_less(double d, int i, double e, int j) { return d < e || (d == e && i < j); }

// One wave merges the c candidates of one query (cd / ci in LDS, c <= kWsCap) into its sorted list ld / li (global, n
// entries).  Returns nothing; the new n-th entry goes to *tau_d / *tau_i.
__device__ void ws_merge(double* cd, int* ci, int* hist, int c, double* ld, int* li, int64_t n, double* tau_d, int* tau_i) {
  const int lane = threadIdx.x & 63;
  int m = 64;
  while (m < c) m <<= 1;
  for (int e = c + lane; e < m; e += 64) {
    cd[e] = __builtin_huge_val();
    ci[e] = 0x7fffffff;
  }
  __builtin_amdgcn_wave_barrier();
  // bitonic sort of the m keys, ascending (the wave's LDS operations complete in order)
  for (int size = 2; size <= m; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = lane; t < (m >> 1); t += 64) {
        const int lo = 2 * stride * (t / stride) + (t % stride), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const double a = cd[lo], b = cd[hi];
        const int ia = ci[lo], ib = ci[hi];
        if (ws_less(b, ib, a, ia) == up) {
          cd[lo] = b;
          ci[lo] = ib;
          cd[hi] = a;
          ci[hi] = ia;
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  for (int e = lane; e <= c; e += 64) hist[e] = 0;
  __builtin_amdgcn_wave_barrier();
  // list entry e moves to e + r(e), r(e) = candidates before it.  Walking the list from the top in 64-entry steps, every
  // step reads its entries before it writes, and it writes only at or above its own start: in place.
  for (int64_t e0 = ((n - 1) >> 6) << 6; e0 >= 0; e0 -= 64) {
    const int64_t e = e0 + lane;
    if (e < n) {
      const double d = ld[e];
      const int i = li[e];
      int lo = 0, hi = c;  // r = number of candidates < (d, i)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ws_less(cd[mid], ci[mid], d, i)) lo = mid + 1;
        else hi = mid;
      }
      atomicAdd(&hist[lo], 1);
      const int64_t np = e + lo;
      if (lo > 0 && np < n) {
        ld[np] = d;
        li[np] = i;
      }
      if (np == n - 1) {
        *tau_d = d;
        *tau_i = i;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  __builtin_amdgcn_wave_barrier();
  // candidate j goes to j + #{list entries with r(e) <= j}: an inclusive scan of hist, kWsCap / 64 entries per lane
  constexpr int PER = kWsCap / 64;
  int run = 0;
  int loc[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int j = lane * PER + u;
    run += j < c ? hist[j] : 0;
    loc[u] = run;
  }
  int incl = run;
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  const int excl = incl - run;
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int j = lane * PER + u;
    if (j < c) {
      const int64_t np = (int64_t)j + excl + loc[u];
      if (np < n) {
        ld[np] = cd[j];
        li[np] = ci[j];
        if (np == n - 1) {
          *tau_d = cd[j];
          *tau_i = ci[j];
        }
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(64 * kWsWaves) void knn_wide_kernel(WideScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* ps = (double*)smem;                    // [kWsDs][kWsPitch] points of the chunk, one dimension slice
  double* qs = ps + kWsDs * kWsPitch;            // [kWsDs][kWsPitch] queries of the tile, same slice
  double* taud = qs + kWsDs * kWsPitch;          // [kWsQ] current n-th distance
  double* sd = taud + kWsQ;                      // [kWsWaves][kWsCap] candidates being merged
  int* taui = (int*)(sd + kWsWaves * kWsCap);    // [kWsQ] its index
  int* cnt = taui + kWsQ;                        // [kWsQ] candidates buffered
  int* si = cnt + kWsQ;                          // [kWsWaves][kWsCap]
  int* hist = si + kWsWaves * kWsCap;            // [kWsWaves][kWsCap + 8]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = tid & 15, ty = tid >> 4;        // points tx + 16 b, queries ty + 16 a of the 64 x 64 tile
  const int k = a.k;
  const int64_t n = a.n_nbrs;
  const int64_t nchunks = (a.n_pts + kWsChunk - 1) / kWsChunk;
  double* const wl = a.list_d + (int64_t)blockIdx.x * kWsQ * n;
  double* const wcd = a.cand_d + (int64_t)blockIdx.x * kWsQ * kWsCap;
  int* const wci = a.cand_i + (int64_t)blockIdx.x * kWsQ * kWsCap;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t q0 = tile * kWsQ;
    const int nqt = (int)(a.n_q - q0 < kWsQ ? a.n_q - q0 : kWsQ);
    for (int64_t e = tid; e < (int64_t)nqt * n; e += blockDim.x) {
      const int qq = (int)(e / n);
      wl[e] = __builtin_huge_val();
      a.nbr[(q0 + qq) * n + (e - (int64_t)qq * n)] = 0x7fffffff;
    }
    if (tid < kWsQ) {
      taud[tid] = __builtin_huge_val();
      taui[tid] = 0x7fffffff;
      cnt[tid] = 0;
    }
    for (int64_t c = 0; c < nchunks; ++c) {
      const int64_t base = c * kWsChunk;
      double acc[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
      for (int d0 = 0; d0 < k; d0 += kWsDs) {
        const int dn = k - d0 < kWsDs ? k - d0 : kWsDs;
        __syncthreads();  // the previous slice has been consumed
        for (int idx = tid; idx < kWsChunk * kWsDs; idx += blockDim.x) {
          const int j = idx / kWsDs, dd = idx - j * kWsDs;  // consecutive threads: consecutive dimensions of one row
          double pv = 0.0, qv = 0.0;
          if (dd < dn) {
            if (base + j < a.n_pts) pv = a.x[(base + j) * k + d0 + dd];
            if (j < nqt) qv = a.xq[(q0 + j) * k + d0 + dd];
          }
          ps[dd * kWsPitch + j] = pv;
          qs[dd * kWsPitch + j] = qv;
        }
        __syncthreads();
        for (int dd = 0; dd < dn; ++dd) {
          double qv[4], pv[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) qv[i] = qs[dd * kWsPitch + ty + 16 * i];
#pragma unroll
          for (int j = 0; j < 4; ++j) pv[j] = ps[dd * kWsPitch + tx + 16 * j];
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const double df = pv[j] - qv[i];
              acc[i][j] += df * df;
            }
        }
      }
      // admission: (dist, index) below the query's current n-th entry (points arrive in increasing index order)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int qq = ty + 16 * i;
        if (qq >= nqt) continue;
        const double td = taud[qq];
        const int ti = taui[qq];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t pt = base + tx + 16 * j;
          double d = acc[i][j];
          if (!(d == d)) d = __builtin_huge_val();  // NaN: sorts with +inf, behind every finite distance
          if (pt < a.n_pts && ws_less(d, (int)pt, td, ti)) {
            const int pos = atomicAdd(&cnt[qq], 1);
            wcd[qq * kWsCap + pos] = d;
            wci[qq * kWsCap + pos] = (int)pt;
          }
        }
      }
      __threadfence_block();
      const bool last = c + 1 == nchunks;
      if (__syncthreads_or(tid < kWsQ && cnt[tid] > kWsCap - kWsChunk) || last) {
        for (int qq = wave; qq < nqt; qq += kWsWaves) {
          const int cc = cnt[qq];
          if (cc == 0) continue;
          double* cd = sd + wave * kWsCap;
          int* ci = si + wave * kWsCap;
          for (int e = lane; e < cc; e += 64) {
            cd[e] = wcd[qq * kWsCap + e];
            ci[e] = wci[qq * kWsCap + e];
          }
          __builtin_amdgcn_wave_barrier();
          ws_merge(cd, ci, hist + wave * (kWsCap + 8), cc, wl + (int64_t)qq * n, a.nbr + (q0 + qq) * n, n, &taud[qq], &taui[qq]);
        }
        __syncthreads();
        if (tid < kWsQ) cnt[tid] = 0;
      }
    }
    __syncthreads();  // the tile's lists are final; the LDS state is free for the next tile
  }
}

// ---- wide fit ----
struct WideFitArgs {
  const double* x;   // n_pts x k
  const double* y;   // n_pts
  const double* xq;  // n_q x k
  const int* nbr;    // n_q x n_nbrs
  int64_t n_q, n_nbrs, P;
  int k, order;
  double out_scale;
  double* g;
  int64_t ldg;
  int* status;
  double* ws;        // [gridDim.x] slices of wf_slice_bytes(P)
};

// design column c of the augmented design [D y] for one neighbour row: (x_a - x0_a) (order 1 and the first k of order 2),
// (x_a - x0_a)(x_b - x0_b) for the (a <= b) pairs in a-major order (mat_col_interactions), 1 for c = P - 1, y for c = P
struct WfCol {
  int a, b;  // a >= 0: coordinate a (times coordinate b when b >= 0); a == -1: constant; a == -2: y; a == -3: zero
};
__device__ __forceinline__ WfCol wf_col(int64_t c, int64_t P, int k) {
  if (c < k) return {(int)c, -1};
  if (c < P - 1) {  // pair index t = c - k; row a holds k - a pairs, starting at a k - a (a - 1) / 2
    const int64_t t = c - k;
    const double kk = (double)k + 0.5;
    int64_t a = (int64_t)(kk - sqrt(kk * kk - 2.0 * (double)t));
    if (a < 0) a = 0;
    if (a > k - 1) a = k - 1;
    while (a > 0 && a * k - a * (a - 1) / 2 > t) --a;
    while (a + 1 < k && (a + 1) * k - (a + 1) * a / 2 <= t) ++a;
    return {(int)a, (int)(a + (t - (a * k - a * (a - 1) / 2)))};
  }
  if (c == P - 1) return {-1, -1};
  if (c == P) return {-2, -1};
  return {-3, -1};
}
__device__ __forceinline__ double wf_val(const WfCol& col, const double* __restrict__ xr, const double* __restrict__ x0,
                                         double yv) {
  if (col.a >= 0) {
    double v = xr[col.a] - x0[col.a];
    if (col.b >= 0) v *= xr[col.b] - x0[col.b];
    return v;
  }
  return col.a == -1 ? 1.0 : (col.a == -2 ? yv : 0.0);
}

// acc (4 x 4 per thread, rows ty + 16 i, columns tx + 16 j) += sum_p A(p, row) B(p, col) over p < inner, staged kWfKb at
// a time: fa(p, r) / fb(p, c) give the operand values (r, c < 64)
template <class FA, class FB>
__device__ __forceinline__ void wf_tile_product(double (&acc)[4][4], double* As, double* Bs, int64_t inner, FA fa, FB fb) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  for (int64_t p0 = 0; p0 < inner; p0 += kWfKb) {
    const int pn = inner - p0 < kWfKb ? (int)(inner - p0) : kWfKb;
    __syncthreads();
    for (int idx = tid; idx < kWfKb * kWfT; idx += blockDim.x) {
      const int p = idx / kWfT, r = idx - p * kWfT;
      As[p * kWfPitch + r] = p < pn ? fa(p0 + p, r) : 0.0;
      Bs[p * kWfPitch + r] = p < pn ? fb(p0 + p, r) : 0.0;
    }
    __syncthreads();
    for (int p = 0; p < pn; ++p) {
      double av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) av[i] = As[p * kWfPitch + ty + 16 * i];
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = Bs[p * kWfPitch + tx + 16 * j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * bv[j];
    }
  }
}

__global__ __launch_bounds__(256) void grad_fit_wide_kernel(WideFitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* As = (double*)smem;                  // [kWfKb][kWfPitch]
  double* Bs = As + kWfKb * kWfPitch;          // [kWfKb][kWfPitch]
  double* Dg = Bs + kWfKb * kWfPitch;          // [kWfT][kWfPitch] diagonal block -> its Cholesky factor
  double* Li = Dg + kWfT * kWfPitch;           // [kWfT][kWfPitch] inverse of that factor
  int* nidx = (int*)(Li + kWfT * kWfPitch);    // [kWfKb] neighbour rows of the chunk being staged
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int k = a.k;
  const int64_t P = a.P, Pa = P + 1, LD = Pa, n = a.n_nbrs;
  double* const M = a.ws + (int64_t)blockIdx.x * (Pa * Pa + 2 * Pa);  // [Pa][LD] lower triangle
  double* const s = M + Pa * Pa;                                      // [Pa] Jacobi scales
  double* const beta = s + Pa;                                        // [Pa] solution
  const int64_t nt = (Pa + kWfT - 1) / kWfT;                          // tiles per edge
  for (int64_t q = blockIdx.x; q < a.n_q; q += gridDim.x) {
    const double* x0 = a.xq + q * k;
    const int* nq = a.nbr + q * n;
    int fl = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
      // ---- normal equations, tile by tile: M(i, j) = sum_r v(r, i) v(r, j), i >= j ----
      for (int64_t ti = 0; ti < nt; ++ti)
        for (int64_t tj = 0; tj <= ti; ++tj) {
          const int r = tid & 63;
          const WfCol ca = wf_col(ti * kWfT + r, P, k), cb = wf_col(tj * kWfT + r, P, k);
          double acc[4][4] = {};
          for (int64_t p0 = 0; p0 < n; p0 += kWfKb) {
            const int pn = n - p0 < kWfKb ? (int)(n - p0) : kWfKb;
            __syncthreads();
            if (tid < kWfKb) nidx[tid] = tid < pn ? nq[p0 + tid] : 0;
            __syncthreads();
            for (int p = tid >> 6; p < kWfKb; p += 4) {  // this thread's column r is fixed: its descriptor is hoisted
              double va = 0.0, vb = 0.0;
              if (p < pn) {
                const int64_t row = nidx[p];
                const double* xr = a.x + row * k;
                const double yv = a.y[row];
                va = wf_val(ca, xr, x0, yv);
                vb = wf_val(cb, xr, x0, yv);
              }
              As[p * kWfPitch + r] = va;
              Bs[p * kWfPitch + r] = vb;
            }
            __syncthreads();
            for (int p = 0; p < pn; ++p) {
              double av[4], bv[4];
#pragma unroll
              for (int i = 0; i < 4; ++i) av[i] = As[p * kWfPitch + ty + 16 * i];
#pragma unroll
              for (int j = 0; j < 4; ++j) bv[j] = Bs[p * kWfPitch + tx + 16 * j];
#pragma unroll
              for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += av[i] * bv[j];
            }
          }
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int64_t gi = ti * kWfT + ty + 16 * i, gj = tj * kWfT + tx + 16 * j;
              if (gi < Pa && gj <= gi) M[gi * LD + gj] = acc[i][j];
            }
        }
      __syncthreads();
      // ---- Jacobi scaling (unit diagonal; a zero column keeps scale 1) and the ridge of the second attempt ----
      for (int64_t i = tid; i < Pa; i += blockDim.x) {
        const double dii = M[i * LD + i];
        s[i] = (i < P && dii > 0.0) ? 1.0 / sqrt(dii) : 1.0;
      }
      __syncthreads();
      for (int64_t e = tid; e < Pa * Pa; e += blockDim.x) {
        const int64_t i = e / Pa, j = e - i * Pa;
        if (j <= i) M[i * LD + j] *= s[i] * s[j];
      }
      __syncthreads();
      double dmax = 0.0;
      for (int64_t i = 0; i < P; ++i) dmax = fmax(dmax, M[i * LD + i]);
      if (attempt == 1)
        for (int64_t i = tid; i < P; i += blockDim.x) M[i * LD + i] += 1e-10 * dmax;
      __syncthreads();
      // ---- blocked right-looking Cholesky of the leading P x P block; row P rides along (it becomes L^-1 D^T y) ----
      bool ok = true;
      for (int64_t j0 = 0; j0 < P && ok; j0 += kWfT) {
        const int jb = P - j0 < kWfT ? (int)(P - j0) : kWfT;
        for (int e = tid; e < kWfT * kWfT; e += blockDim.x) {
          const int i = e / kWfT, j = e - i * kWfT;
          Dg[i * kWfPitch + j] = (i < jb && j <= i) ? M[(j0 + i) * LD + j0 + j] : 0.0;
          Li[i * kWfPitch + j] = 0.0;
        }
        __syncthreads();
        int done = 0;                   // columns factorised (the same in every thread: the pivot test is uniform)
        for (int j = 0; j < jb; ++j) {  // unblocked, in LDS; the relative pivot test of grad_fit_kernel
          const double piv = Dg[j * kWfPitch + j];
          if (!(piv > 1e-13 * dmax)) break;
          const double dj = sqrt(piv);
          __syncthreads();
          if (tid == 0) Dg[j * kWfPitch + j] = dj;
          for (int i = j + 1 + tid; i < jb; i += blockDim.x) Dg[i * kWfPitch + j] /= dj;
          __syncthreads();
          const int tw = jb - j - 1;
          for (int e = tid; e < tw * tw; e += blockDim.x) {
            const int i = j + 1 + e / tw, l = j + 1 + e % tw;
            if (l <= i) Dg[i * kWfPitch + l] -= Dg[i * kWfPitch + j] * Dg[l * kWfPitch + j];
          }
          __syncthreads();
          ++done;
        }
        ok = done == jb;
        if (!ok) break;
        // inverse of the diagonal factor: column c solves L x = e_c by forward substitution
        if (tid < jb) {
          const int c = tid;
          for (int r = c; r < jb; ++r) {
            double t = r == c ? 1.0 : 0.0;
            for (int p = c; p < r; ++p) t -= Dg[r * kWfPitch + p] * Li[p * kWfPitch + c];
            Li[r * kWfPitch + c] = t / Dg[r * kWfPitch + r];
          }
        }
        __syncthreads();
        for (int e = tid; e < jb * jb; e += blockDim.x) {  // the factor of the diagonal block back to the slice
          const int i = e / jb, j = e - i * jb;
          if (j <= i) M[(j0 + i) * LD + j0 + j] = Dg[i * kWfPitch + j];
        }
        // panel: L(i, j0 + l) = sum_p M(i, j0 + p) Linv(l, p) for the rows i >= j0 + jb (row P included)
        const int64_t r0 = j0 + jb;
        for (int64_t i0 = r0; i0 < Pa; i0 += kWfT) {
          double acc[4][4] = {};
          wf_tile_product(
              acc, As, Bs, jb,
              [&](int64_t p, int r) { return i0 + r < Pa ? M[(i0 + r) * LD + j0 + p] : 0.0; },
              [&](int64_t p, int c) { return c < jb ? Li[c * kWfPitch + p] : 0.0; });
          __syncthreads();  // every read of this row block is done before it is overwritten
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int64_t gi = i0 + ty + 16 * i;
              const int gj = tx + 16 * j;
              if (gi < Pa && gj < jb) M[gi * LD + j0 + gj] = acc[i][j];
            }
        }
        __syncthreads();
        // trailing update: M(i, j) -= sum_p L(i, j0 + p) L(j, j0 + p) for r0 <= j <= i, j < P
        for (int64_t i0 = r0; i0 < Pa; i0 += kWfT)
          for (int64_t c0 = r0; c0 <= i0 && c0 < P; c0 += kWfT) {
            double acc[4][4] = {};
            wf_tile_product(
                acc, As, Bs, jb,
                [&](int64_t p, int r) { return i0 + r < Pa ? M[(i0 + r) * LD + j0 + p] : 0.0; },
                [&](int64_t p, int c) { return c0 + c < P ? M[(c0 + c) * LD + j0 + p] : 0.0; });
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int64_t gi = i0 + ty + 16 * i, gj = c0 + tx + 16 * j;
                if (gi < Pa && gj < P && gj <= gi) M[gi * LD + gj] -= acc[i][j];
              }
          }
        __syncthreads();
      }
      if (ok) break;
      fl = attempt == 0 ? 1 : 2;
      if (attempt == 1) break;
      __syncthreads();
    }
    // ---- back substitution L^T beta = z, z = row P of the factor, 64 rows at a time from the bottom ----
    if (fl != 2) {
      for (int64_t i1 = P; i1 > 0; i1 -= kWfT) {
        const int64_t i0 = i1 - kWfT > 0 ? i1 - kWfT : 0;
        const int ib = (int)(i1 - i0);
        // t(i) = z(i) - sum_{p >= i1} L(p, i) beta(p): lane = i, the four waves split p
        const int i = tid & 63, w = tid >> 6;
        double t = 0.0;
        if (i < ib)
          for (int64_t p = i1 + w; p < P; p += 4) t += M[p * LD + i0 + i] * beta[p];
        As[w * kWfPitch + i] = t;
        __syncthreads();
        if (tid < 64) {
          double ti = 0.0;
          if (i < ib) ti = M[P * LD + i0 + i] - (As[i] + As[kWfPitch + i] + As[2 * kWfPitch + i] + As[3 * kWfPitch + i]);
          for (int r = ib - 1; r >= 0; --r) {  // the 64 x 64 triangle, one wave
            const double br = __shfl(ti, r, 64) / M[(i0 + r) * LD + i0 + r];
            if (i < r) ti -= M[(i0 + r) * LD + i0 + i] * br;
            if (i == r) ti = br;
          }
          if (i < ib) beta[i0 + i] = ti;
        }
        __syncthreads();
      }
    }
    for (int m = tid; m < k; m += blockDim.x) a.g[q * a.ldg + m] = fl == 2 ? 0.0 : a.out_scale * beta[m] * s[m];
    if (tid == 0 && a.status) a.status[q] = fl;
    __syncthreads();  // the slice is free for the next query of this workgroup
  }
}

}  // namespace k
}  // namespace corrla
