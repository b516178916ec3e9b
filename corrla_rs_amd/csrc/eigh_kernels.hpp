// The symmetric eigensolver A = V diag(w) V^T on the device (f64, row-major; the geometry is eigh_plan.hpp's).  Only the lower
// triangle (i >= j) of A is ever loaded: the strict upper triangle may hold anything.
//
// The route: B = A + sigma I with sigma = 1.5 min(|A|_F, |A|_inf) is positive definite with a condition number of at most 5,
// B = L L^T (chol_kernels.hpp), and one-sided block Jacobi with right rotations on W = L keeps W W^T = B while the columns of W
// become orthogonal: then v_i = w_i / |w_i| and w_i is the Rayleigh quotient v_i^T A v_i / v_i^T v_i (|w_i|^2 - sigma carries the rounding
// of every rotation the column went through; the quotient does not).  The result is normwise backward stable -- absolute
// errors of order n u (sigma + |A|_2), as LAPACK's for an indefinite matrix -- and NOT relatively accurate for small
// eigenvalues.  No atomics, no workgroup waits on another, every reduction runs in a fixed order, every loop is bounded by the
// shape and the sweep caps: a call is bitwise reproducible.  This file must not be compiled with approximate-math options.
//
//   eigh_small_kernel     n <= kEighSmallN: everything by one workgroup in LDS, as one pair that holds every column
//   eigh_norm_kernel      per block of 64 rows of the mirrored lower triangle: the largest absolute row sum, the sum of squares
//   eigh_sigma_kernel     those records reduced to the header (sigma, the norms, the non-finite flag)
//   eigh_shift_kernel     the lower triangle of B = A + sigma I into workspace
//   eigh_identity_kernel  sigma = 0: w = 0, V = I
//   eigh_repack_kernel    L into column panels: block b is the contiguous row-major n x kEighB range of its columns
//   eigh_gram_kernel      per pair and row slab: the partial 64 x 64 Gram tile of [W_I W_J] on v_mfma_f64_16x16x4_f64
//   eigh_rot_kernel       per pair: the slab partials added in order, the measure, the threshold Jacobi in LDS -> R, measure, flag
//   eigh_apply_kernel     per pair and row slab: [W_I W_J] <- [W_I W_J] R on the same MFMA, in place; returns for a flagged pair
//   eigh_sweep_kernel     the measures of a sweep's pairs folded into the sweep record
//   eigh_colnorm_kernel   per block: |w_i|, the component of largest magnitude and its sign
//   eigh_unit_kernel      u_i = w_i / (sign_i |w_i|), in place
//   eigh_rayleigh_kernel  per block and 64 rows: the partial quotients u_i^T A u_i over the mirrored lower triangle, on the MFMA
//   eigh_lambda_kernel    the partial quotients added in order and divided by u_i^T u_i
//   eigh_rank_kernel      ranks by counting (ties to the lower column index), w in ascending order
//   eigh_scatter_kernel   V[:, rank_i] = u_i
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "chol_kernels.hpp"  // chol_factor_lds
#include "eigh_plan.hpp"
#include "hip_kernels.hpp"  // MT<double>

namespace corrla {
namespace k {

// op over the kEighThreads values, in a fixed tree, to every thread; sv: kEighThreads entries
template <class Op>
__device__ __forceinline__ double eigh_block_reduce(double v, double* sv, int tid, Op op) {
  sv[tid] = v;
  __syncthreads();
  for (int s = kEighThreads / 2; s > 0; s >>= 1) {
    if (tid < s) sv[tid] = op(sv[tid], sv[tid + s]);
    __syncthreads();
  }
  const double r = sv[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ double eigh_max(double x, double y) { return x > y ? x : y; }
// a comparison, no arithmetic: x - x == 0 on a product is contracted into an fma that returns the product's rounding error
__device__ __forceinline__ bool eigh_finite(double x) { return fabs(x) < __builtin_inf(); }
// A sum kept in two doubles (hi, lo), |lo| of the order of a rounding of hi: the column norms and the Rayleigh quotients are
// sums of n terms of one sign, and a plain running sum loses sqrt(n / 3) roundings of the result -- a norm that is off by delta
// moves the quotient of the "unit" vector by 2 delta lambda, which is the scale the eigenvalues are held to.  add: the rounding
// error of hi + x recovered exactly (Knuth); add_product: x y split by one fma into its rounded product and the exact remainder.
struct EighSum {
  double hi = 0.0, lo = 0.0;
  __device__ __forceinline__ void add(double x) {
#pragma clang fp contract(off)
    const double t = hi + x, z = t - hi;
    lo += (hi - (t - z)) + (x - z);
    hi = t;
  }
  __device__ __forceinline__ void add_product(double x, double y) {
#pragma clang fp contract(off)
    const double p = x * y;
    lo += __builtin_fma(x, y, -p);
    add(p);
  }
  __device__ __forceinline__ void add_sum(const EighSum& o) {
    add(o.hi);
    lo += o.lo;
  }
  __device__ __forceinline__ double value() const { return hi + lo; }
};

__device__ __forceinline__ double eigh_sigma_of(double fro, double inf) { return 1.5 * (fro > 0.0 && fro < inf ? fro : inf); }

// index i of a pair's 64: the first wi of the first block and the first wj of the second exist
__device__ __forceinline__ bool eigh_active(int i, int wi, int wj) { return i < wi || (i >= kEighB && i < kEighB + wj); }

// the tournament of eigh_pair over the 64 indices, in 32-bit arithmetic: pair q of step r, *a < *b
__device__ __forceinline__ void eigh_inner_pair(int r, int q, int* a, int* b) {
  int x, y;
  if (q == 0) {
    x = r, y = kEighPair - 1;
  } else {
    x = r + q;
    if (x >= kEighPair - 1) x -= kEighPair - 1;
    y = r - q;
    if (y < 0) y += kEighPair - 1;
  }
  *a = x < y ? x : y;
  *b = x < y ? y : x;
}

// max over the active i != j of |g_ij| / sqrt(g_ii g_jj), to every thread
__device__ __forceinline__ double eigh_measure_lds(const double* G, int wi, int wj, double* sv, int tid) {
  constexpr int JL = kEighJacLd;
  double m = 0.0;
  for (int e = tid; e < kEighPair * kEighPair; e += kEighThreads) {
    const int i = e >> 6, j = e & 63;
    if (i == j || !eigh_active(i, wi, wj) || !eigh_active(j, wi, wj)) continue;
    const double d = G[i * JL + i] * G[j * JL + j];
    const double q = d > 0.0 ? fabs(G[i * JL + j]) / __builtin_sqrt(d) : 0.0;
    m = eigh_max(m, q);
  }
  return eigh_block_reduce(m, sv, tid, eigh_max);
}

// Cyclic threshold Jacobi on the symmetric 64 x 64 LDS image G (row stride kEighJacLd) by the whole workgroup: G <- J^T G J and
// R <- R J, rotation by rotation, in the order of the tournament (63 steps of 32 disjoint rotations per sweep).  A rotation is
// made where |g_pq| > thr sqrt(g_pp g_qq), with the smaller of the two angles (|tan| <= 1), and leaves g_pq = 0; no row or
// column is ever exchanged, so R -> I as G -> diagonal.  Ends with the first sweep that rotates nothing, or at max_sweeps.
// cs: 2 kEighB doubles; pq: 2 kEighB ints; flag: one int.  Returns the sweeps that rotated; *capped: the last one still did.
__device__ __forceinline__ int eigh_jacobi_lds(double* G, double* R, double* cs, int* pq, int* flag, int wi, int wj, double thr, int max_sweeps,
                                               int tid, bool* capped) {
  constexpr int JL = kEighJacLd;
  int rotated_sweeps = 0;
  *capped = false;
  for (int sw = 0; sw < max_sweeps; ++sw) {
    if (tid == 0) *flag = 0;
    __syncthreads();
    for (int r = 0; r < kEighPair - 1; ++r) {
      if (tid < kEighB) {
        int p, q;
        eigh_inner_pair(r, tid, &p, &q);
        double c = 1.0, s = 0.0;
        if (eigh_active(p, wi, wj) && eigh_active(q, wi, wj)) {
          const double gpp = G[p * JL + p], gqq = G[q * JL + q], gpq = G[p * JL + q];
          if (fabs(gpq) > thr * __builtin_sqrt(fabs(gpp * gqq))) {
            const double zeta = (gqq - gpp) / (2.0 * gpq);
            const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + __builtin_sqrt(1.0 + zeta * zeta));
            c = 1.0 / __builtin_sqrt(1.0 + t * t);
            s = c * t;
            if (!(s != 0.0)) c = 1.0, s = 0.0;  // an overflowed zeta: no rotation
            else *flag = 1;                     // every writer stores the same value
          }
        }
        cs[2 * tid] = c, cs[2 * tid + 1] = s;
        pq[2 * tid] = p, pq[2 * tid + 1] = q;
      }
      __syncthreads();
      // columns: G <- G J, R <- R J
      for (int e = tid; e < kEighB * kEighPair; e += kEighThreads) {
        const int kk = e >> 6, i = e & 63;
        const double c = cs[2 * kk], s = cs[2 * kk + 1];
        if (s == 0.0) continue;
        const int p = pq[2 * kk], q = pq[2 * kk + 1];
        const double x = G[i * JL + p], y = G[i * JL + q];
        G[i * JL + p] = c * x - s * y;
        G[i * JL + q] = s * x + c * y;
        const double u = R[i * JL + p], v = R[i * JL + q];
        R[i * JL + p] = c * u - s * v;
        R[i * JL + q] = s * u + c * v;
      }
      __syncthreads();
      // rows: G <- J^T G; the rotated entry is an exact zero
      for (int e = tid; e < kEighB * kEighPair; e += kEighThreads) {
        const int kk = e >> 6, j = e & 63;
        const double c = cs[2 * kk], s = cs[2 * kk + 1];
        if (s == 0.0) continue;
        const int p = pq[2 * kk], q = pq[2 * kk + 1];
        const double x = G[p * JL + j], y = G[q * JL + j];
        G[p * JL + j] = j == q ? 0.0 : c * x - s * y;
        G[q * JL + j] = j == p ? 0.0 : s * x + c * y;
      }
      __syncthreads();
    }
    const int any = *flag;
    __syncthreads();
    if (!any) break;
    ++rotated_sweeps;
    if (sw + 1 == max_sweeps) *capped = true;
  }
  return rotated_sweeps;
}

// ---- SMALL ------------------------------------------------------------------------------------------------------------------
struct EighSmallArgs {
  const double* a;  // n x n, row stride lda: the lower triangle is read
  int64_t lda;
  int n;            // <= kEighSmallN
  double* w;        // n
  double* v;        // n x n, row stride ldv
  int64_t ldv;
  EighHeader* hdr;
  double tol, thr;
};

// C = A^T B (TRANS_A) or A B over the 64 x 64 LDS images, by the whole workgroup; rows of A beyond `rows` are not read
template <bool TRANS_A>
__device__ __forceinline__ void eigh_lds_product(const double* A, const double* Bm, double* C, int rows, int tid) {
  constexpr int JL = kEighJacLd;
  for (int e = tid; e < kEighPair * kEighPair; e += kEighThreads) {
    const int i = e >> 6, j = e & 63;
    double s = 0.0;
    if (TRANS_A) {
      for (int r = 0; r < rows; ++r) s = __builtin_fma(A[r * JL + i], Bm[r * JL + j], s);
    } else {
      if (i < rows)
        for (int q = 0; q < kEighPair; ++q) s = __builtin_fma(A[i * JL + q], Bm[q * JL + j], s);
    }
    C[i * JL + j] = s;
  }
}

// the lower triangle of a mirrored into the 64 x 64 image M, zeros beyond n
__device__ __forceinline__ void eigh_load_mirrored(const EighSmallArgs& g, double* M, int tid) {
  constexpr int JL = kEighJacLd;
  for (int e = tid; e < kEighPair * kEighPair; e += kEighThreads) {
    const int r = e >> 6, c = e & 63;
    M[r * JL + c] = (r < g.n && c < g.n) ? (c <= r ? g.a[(int64_t)r * g.lda + c] : g.a[(int64_t)c * g.lda + r]) : 0.0;
  }
}

// BLOCKED with one pair that holds every column (block 0 the first 32, block 1 the rest), in LDS: the norms and sigma, the
// Cholesky factor of B by the routine of the Cholesky kernels, then per sweep G = W^T W, the measure, one LDS Jacobi and W <- W R.
__global__ __launch_bounds__(kEighThreads) void eigh_small_kernel(EighSmallArgs g) {
  constexpr int JL = kEighJacLd, NP = kEighPair;
  static_assert(kEighSmallN == NP && kCholThreads == kEighThreads, "every column in one pair; chol_factor_lds strides by kCholThreads");
  extern __shared__ uint4 eigh_smem[];
  double* W = reinterpret_cast<double*>(eigh_smem);  // [NP][JL] each
  double* G = W + NP * JL;
  double* R = G + NP * JL;
  double* cs = R + NP * JL;
  double* sv = cs + 2 * kEighB;  // 2 kEighThreads
  __shared__ int pq[2 * kEighB];
  __shared__ int flag;
  const int tid = (int)threadIdx.x, n = g.n;
  eigh_load_mirrored(g, G, tid);
  __syncthreads();
  double bad = 0.0, f2 = 0.0;
  for (int e = tid; e < NP * NP; e += kEighThreads) {
    const double x = G[(e >> 6) * JL + (e & 63)];
    if (!eigh_finite(x)) bad = 1.0;
    f2 = __builtin_fma(x, x, f2);
  }
  double rs = 0.0;
  if (tid < n)
    for (int c = 0; c < n; ++c) rs += fabs(G[tid * JL + c]);
  bad = eigh_block_reduce(bad, sv, tid, eigh_max);
  f2 = eigh_block_reduce(f2, sv, tid, [](double x, double y) { return x + y; });
  const double inf = eigh_block_reduce(rs, sv, tid, eigh_max);
  const double fro = __builtin_sqrt(f2);
  const double sigma = eigh_sigma_of(fro, inf);
  const bool stop = bad != 0.0 || !eigh_finite(sigma);
  if (stop || sigma == 0.0) {  // uniform
    if (tid == 0) {
      g.hdr->sigma = stop ? 0.0 : sigma, g.hdr->fro = fro, g.hdr->inf = inf, g.hdr->bad = stop ? 1.0 : 0.0;
      g.hdr->sweeps = 0.0, g.hdr->off = 0.0, g.hdr->capped = 0.0, g.hdr->pad = 0.0;
    }
    if (!stop) {
      for (int e = tid; e < n * n; e += kEighThreads) {
        const int r = e / n, c = e - r * n;
        g.v[(int64_t)r * g.ldv + c] = r == c ? 1.0 : 0.0;
      }
      if (tid < n) g.w[tid] = 0.0;
    }
    return;
  }
  if (tid < n) G[tid * JL + tid] += sigma;
  __syncthreads();
  int info;
  double mind, maxd;
  chol_factor_lds<JL>(G, n, tid, info, mind, maxd);
  for (int e = tid; e < NP * NP; e += kEighThreads) {
    const int r = e >> 6, c = e & 63;
    W[r * JL + c] = (r < n && c <= r) ? G[r * JL + c] : 0.0;
  }
  __syncthreads();
  const int wi = n < kEighB ? n : kEighB, wj = n - wi;
  int sweeps = 0;
  double off = 0.0;
  bool capped = false;
  for (int it = 0; it <= kEighMaxSweeps; ++it) {
    eigh_lds_product<true>(W, W, G, n, tid);
    for (int e = tid; e < NP * NP; e += kEighThreads) R[(e >> 6) * JL + (e & 63)] = (e >> 6) == (e & 63) ? 1.0 : 0.0;
    __syncthreads();
    off = eigh_measure_lds(G, wi, wj, sv, tid);
    if (!(off > g.tol)) break;  // uniform
    if (it == kEighMaxSweeps) {
      capped = true;
      break;
    }
    bool inner_capped;
    (void)eigh_jacobi_lds(G, R, cs, pq, &flag, wi, wj, g.thr, kEighInnerSweeps, tid, &inner_capped);
    eigh_lds_product<false>(W, R, G, n, tid);
    __syncthreads();
    double* t = W;
    W = G;
    G = t;
    ++sweeps;
  }
  // unit columns with the component of largest magnitude positive (the lowest row wins a tie)
  if (tid < n) {
    EighSum s2;
    double best = -1.0, sgn = 1.0;
    for (int r = 0; r < n; ++r) {
      const double x = W[r * JL + tid];
      s2.add_product(x, x);
      if (fabs(x) > best) best = fabs(x), sgn = x < 0.0 ? -1.0 : 1.0;
    }
    sv[tid] = sgn * __builtin_sqrt(s2.value());
  }
  __syncthreads();
  for (int e = tid; e < n * n; e += kEighThreads) {
    const int r = e / n, c = e - r * n;
    W[r * JL + c] = W[r * JL + c] / sv[c];
  }
  eigh_load_mirrored(g, R, tid);
  __syncthreads();
  eigh_lds_product<false>(R, W, G, n, tid);  // A U
  __syncthreads();
  double* lam = sv + kEighThreads;
  if (tid < n) {
    EighSum s, q;  // u^T A u over u^T u of the rounded u: the rounding of the normalisation cancels
    for (int r = 0; r < n; ++r) {
      s.add_product(W[r * JL + tid], G[r * JL + tid]);
      q.add_product(W[r * JL + tid], W[r * JL + tid]);
    }
    lam[tid] = s.value() / q.value();
  }
  __syncthreads();
  if (tid < n) {
    const double li = lam[tid];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += (lam[j] < li || (lam[j] == li && j < tid)) ? 1 : 0;
    g.w[rank] = li;
    for (int r = 0; r < n; ++r) g.v[(int64_t)r * g.ldv + rank] = W[r * JL + tid];
  }
  if (tid == 0) {
    g.hdr->sigma = sigma, g.hdr->fro = fro, g.hdr->inf = inf, g.hdr->bad = info != 0 ? 2.0 : 0.0;
    g.hdr->sweeps = (double)sweeps, g.hdr->off = off, g.hdr->capped = capped ? 1.0 : 0.0, g.hdr->pad = 0.0;
  }
}

// ---- BLOCKED: the norms and the shift ---------------------------------------------------------------------------------------
struct EighNormArgs {
  const double* a;
  int64_t lda, n;
  double* norms;  // per workgroup: the largest absolute row sum, the sum of squares, the non-finite flag, unused
};

// Workgroup bi owns the rows [64 bi, 64 bi + 64) of the mirrored matrix.  Tile t <= bi is read along those rows of the lower
// triangle; tile t > bi is the block below the diagonal block whose columns are those rows.  The squares are counted over the
// tiles t <= bi alone, twice below the diagonal.
__global__ __launch_bounds__(kEighThreads) void eigh_norm_kernel(EighNormArgs g) {
  constexpr int TL = 65;
  __shared__ double T[64 * TL];
  __shared__ double sv[kEighThreads];
  const int tid = (int)threadIdx.x, x = tid & 63, part = tid >> 6;
  const int64_t bi = blockIdx.x, nt = eigh_ceil_div(g.n, 64);
  double bad = 0.0, f2 = 0.0, acc = 0.0;
  for (int64_t t = 0; t < nt; ++t) {
    const int64_t r0 = t <= bi ? bi * 64 : t * 64, c0 = t <= bi ? t * 64 : bi * 64;
    for (int e = tid; e < 64 * 64; e += kEighThreads) {
      const int rr = e >> 6, cc = e & 63;
      const int64_t row = r0 + rr, col = c0 + cc;
      double val = 0.0;
      if (row < g.n && col <= row) {
        val = g.a[row * g.lda + col];
        if (!eigh_finite(val)) bad = 1.0;
        if (t <= bi) f2 += (col < row ? 2.0 : 1.0) * val * val;
      }
      T[rr * TL + cc] = val;
    }
    __syncthreads();
    if (t <= bi)
      for (int cc = 16 * part; cc < 16 * part + 16; ++cc) acc += fabs(T[x * TL + cc]);
    if (t >= bi)  // the diagonal tile holds zeros above the diagonal: the row part took its diagonal
      for (int rr = 16 * part; rr < 16 * part + 16; ++rr) acc += (t > bi || rr > x) ? fabs(T[rr * TL + x]) : 0.0;
    __syncthreads();
  }
  sv[tid] = acc;
  __syncthreads();
  const double rs = tid < 64 ? ((sv[tid] + sv[tid + 64]) + sv[tid + 128]) + sv[tid + 192] : 0.0;
  __syncthreads();
  const double mx = eigh_block_reduce(rs, sv, tid, eigh_max);
  f2 = eigh_block_reduce(f2, sv, tid, [](double p, double q) { return p + q; });
  bad = eigh_block_reduce(bad, sv, tid, eigh_max);
  if (tid == 0) {
    double* o = g.norms + 4 * bi;
    o[0] = mx, o[1] = f2, o[2] = bad, o[3] = 0.0;
  }
}

struct EighSigmaArgs {
  const double* norms;
  int64_t groups;
  EighHeader* hdr;
};

__global__ __launch_bounds__(kEighThreads) void eigh_sigma_kernel(EighSigmaArgs g) {
  __shared__ double sv[kEighThreads];
  const int tid = (int)threadIdx.x;
  double mx = 0.0, f2 = 0.0, bad = 0.0;
  for (int64_t i = tid; i < g.groups; i += kEighThreads) {
    mx = eigh_max(mx, g.norms[4 * i]);
    f2 += g.norms[4 * i + 1];
    bad = eigh_max(bad, g.norms[4 * i + 2]);
  }
  mx = eigh_block_reduce(mx, sv, tid, eigh_max);
  f2 = eigh_block_reduce(f2, sv, tid, [](double p, double q) { return p + q; });
  bad = eigh_block_reduce(bad, sv, tid, eigh_max);
  if (tid == 0) {
    const double fro = __builtin_sqrt(f2), sigma = eigh_sigma_of(fro, mx);
    const bool stop = bad != 0.0 || !eigh_finite(sigma);
    g.hdr->sigma = stop ? 0.0 : sigma, g.hdr->fro = fro, g.hdr->inf = mx, g.hdr->bad = stop ? 1.0 : 0.0;
    g.hdr->sweeps = 0.0, g.hdr->off = 0.0, g.hdr->capped = 0.0, g.hdr->pad = 0.0;
  }
}

struct EighShiftArgs {
  const double* a;
  int64_t lda, n;
  double* b;  // n x n, row stride n: its lower triangle is written
  const EighHeader* hdr;
};

// grid (tiles, tiles) of 64 x 64; the tiles above the diagonal return
__global__ __launch_bounds__(kEighThreads) void eigh_shift_kernel(EighShiftArgs g) {
  if (blockIdx.x > blockIdx.y) return;
  const double sigma = g.hdr->sigma;
  const int64_t r0 = (int64_t)blockIdx.y * 64, c0 = (int64_t)blockIdx.x * 64;
  for (int e = (int)threadIdx.x; e < 64 * 64; e += kEighThreads) {
    const int64_t row = r0 + (e >> 6), col = c0 + (e & 63);
    if (row < g.n && col <= row) g.b[row * g.n + col] = g.a[row * g.lda + col] + (row == col ? sigma : 0.0);
  }
}

struct EighIdentityArgs {
  double* w;
  double* v;
  int64_t ldv, n;
};

__global__ __launch_bounds__(kEighThreads) void eigh_identity_kernel(EighIdentityArgs g) {
  const int64_t r0 = (int64_t)blockIdx.y * 64, c0 = (int64_t)blockIdx.x * 64;
  for (int e = (int)threadIdx.x; e < 64 * 64; e += kEighThreads) {
    const int64_t row = r0 + (e >> 6), col = c0 + (e & 63);
    if (row < g.n && col < g.n) g.v[row * g.ldv + col] = row == col ? 1.0 : 0.0;
    if (blockIdx.x == 0 && (e & 63) == 0 && row < g.n) g.w[row] = 0.0;
  }
}

struct EighRepackArgs {
  const double* b;  // L over the lower triangle, row stride n
  int64_t n;
  double* w;        // panels: element (row, column c of block blk) at (blk n + row) kEighB + c
};

// grid (blocks, chunks of 64 rows)
__global__ __launch_bounds__(kEighThreads) void eigh_repack_kernel(EighRepackArgs g) {
  const int64_t blk = blockIdx.x, r0 = (int64_t)blockIdx.y * 64;
  for (int e = (int)threadIdx.x; e < 64 * kEighB; e += kEighThreads) {
    const int64_t row = r0 + e / kEighB, col = blk * kEighB + e % kEighB;
    if (row < g.n) g.w[(blk * g.n + row) * kEighB + e % kEighB] = (col < g.n && col <= row) ? g.b[row * g.n + col] : 0.0;
  }
}

// ---- BLOCKED: a round of the tournament -------------------------------------------------------------------------------------
struct EighRoundArgs {
  double* w;        // the panels
  int64_t n, nb;
  int64_t round;
  int64_t slabs, slab_rows;
  double* gram;     // per pair and slab a 64 x 64 tile, row-major
  double* rot;      // per pair R, 64 x 64 row-major
  double* meas;     // this round's: per pair the measure and the skip flag
  double tol, thr;
};

// Workgroup = pair x slab.  A chunk of 64 rows of both panels is staged as one [k][col] image, which is both operands of
// X^T X: wave w owns the rows 16 w .. 16 w + 15 of the tile.  Rows beyond n are zeros.
__global__ __launch_bounds__(kEighThreads) void eigh_gram_kernel(EighRoundArgs g) {
  constexpr int LD = kEighColLd;
  static_assert(kEighChunk == 64 && kEighPair == 64 && kEighThreads == 256, "four waves of 16 rows x 4 column tiles");
  __shared__ double X[kEighChunk * LD];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, fc = lane & 15, kq = lane >> 4;
  const int64_t p = (int64_t)blockIdx.x / g.slabs, sl = (int64_t)blockIdx.x % g.slabs;
  int64_t bi, bj;
  eigh_pair(g.nb, g.round, p, &bi, &bj);
  const double* wi = g.w + bi * g.n * kEighB;
  const double* wj = g.w + bj * g.n * kEighB;
  const int64_t rbeg = sl * g.slab_rows, rend = rbeg + g.slab_rows < g.n ? rbeg + g.slab_rows : g.n;
  MT<double>::acc_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = MT<double>::acc_t{0, 0, 0, 0};
  for (int64_t r0 = rbeg; r0 < rend; r0 += kEighChunk) {
    __syncthreads();
    for (int e = tid; e < kEighChunk * kEighPair; e += kEighThreads) {
      const int kk = e >> 6, cc = e & 63;
      const int64_t row = r0 + kk;
      X[kk * LD + cc] = row < rend ? (cc < kEighB ? wi[row * kEighB + cc] : wj[row * kEighB + cc - kEighB]) : 0.0;
    }
    __syncthreads();
    const double* pa = X + kq * LD + 16 * wave + fc;
    const double* pb = X + kq * LD + fc;
#pragma unroll
    for (int s = 0; s < kEighChunk / 4; ++s) {
      const double a = pa[s * 4 * LD];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = MT<double>::mma(a, pb[s * 4 * LD + 16 * t], acc[t]);
    }
  }
  double* out = g.gram + (int64_t)blockIdx.x * kEighPair * kEighPair;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * wave + MT<double>::drow(lane, r);
#pragma unroll
    for (int t = 0; t < 4; ++t) out[row * kEighPair + 16 * t + fc] = acc[t][r];
  }
}

// Workgroup = pair.
__global__ __launch_bounds__(kEighThreads) void eigh_rot_kernel(EighRoundArgs g) {
  constexpr int JL = kEighJacLd, NP = kEighPair;
  extern __shared__ uint4 eigh_smem[];
  double* G = reinterpret_cast<double*>(eigh_smem);
  double* R = G + NP * JL;
  double* cs = R + NP * JL;
  double* sv = cs + 2 * kEighB;
  __shared__ int pq[2 * kEighB];
  __shared__ int flag;
  const int tid = (int)threadIdx.x;
  const int64_t p = blockIdx.x;
  int64_t bi, bj;
  eigh_pair(g.nb, g.round, p, &bi, &bj);
  const int wi = eigh_block_width(g.n, bi), wj = eigh_block_width(g.n, bj);
  const double* part = g.gram + p * g.slabs * NP * NP;
  for (int e = tid; e < NP * NP; e += kEighThreads) {
    double s = 0.0;
    for (int64_t sl = 0; sl < g.slabs; ++sl) s += part[sl * NP * NP + e];
    G[(e >> 6) * JL + (e & 63)] = s;
    R[(e >> 6) * JL + (e & 63)] = (e >> 6) == (e & 63) ? 1.0 : 0.0;
  }
  __syncthreads();
  const double m = eigh_measure_lds(G, wi, wj, sv, tid);
  if (!(m > g.tol)) {  // uniform
    if (tid == 0) g.meas[2 * p] = m, g.meas[2 * p + 1] = 1.0;
    return;
  }
  bool capped;
  (void)eigh_jacobi_lds(G, R, cs, pq, &flag, wi, wj, g.thr, kEighInnerSweeps, tid, &capped);
  double* out = g.rot + p * NP * NP;
  for (int e = tid; e < NP * NP; e += kEighThreads) out[e] = R[(e >> 6) * JL + (e & 63)];
  if (tid == 0) g.meas[2 * p] = m, g.meas[2 * p + 1] = 0.0;
}

// Workgroup = pair x slab.  R is staged once as a [k][col] image, every chunk of 64 rows as a [row][k] image; the chunk is
// whole in LDS before its rows are stored, and no other workgroup touches those rows of those panels.
__global__ __launch_bounds__(kEighThreads) void eigh_apply_kernel(EighRoundArgs g) {
  constexpr int LDR = kEighRowLd, LDC = kEighColLd;
  extern __shared__ uint4 eigh_smem[];
  double* X = reinterpret_cast<double*>(eigh_smem);  // [kEighChunk][LDR]
  double* RL = X + kEighChunk * LDR;                 // [kEighPair][LDC]
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, fc = lane & 15, kq = lane >> 4;
  const int64_t p = (int64_t)blockIdx.x / g.slabs, sl = (int64_t)blockIdx.x % g.slabs;
  if (g.meas[2 * p + 1] != 0.0) return;  // uniform
  int64_t bi, bj;
  eigh_pair(g.nb, g.round, p, &bi, &bj);
  double* wi = g.w + bi * g.n * kEighB;
  double* wj = g.w + bj * g.n * kEighB;
  const double* rot = g.rot + p * kEighPair * kEighPair;
  for (int e = tid; e < kEighPair * kEighPair; e += kEighThreads) RL[(e >> 6) * LDC + (e & 63)] = rot[e];
  const int64_t rbeg = sl * g.slab_rows, rend = rbeg + g.slab_rows < g.n ? rbeg + g.slab_rows : g.n;
  for (int64_t r0 = rbeg; r0 < rend; r0 += kEighChunk) {
    __syncthreads();
    for (int e = tid; e < kEighChunk * kEighPair; e += kEighThreads) {
      const int rr = e >> 6, kk = e & 63;
      const int64_t row = r0 + rr;
      X[rr * LDR + kk] = row < rend ? (kk < kEighB ? wi[row * kEighB + kk] : wj[row * kEighB + kk - kEighB]) : 0.0;
    }
    __syncthreads();
    MT<double>::acc_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = MT<double>::acc_t{0, 0, 0, 0};
    const double* pa = X + (16 * wave + fc) * LDR + kq;
    const double* pb = RL + kq * LDC + fc;
#pragma unroll
    for (int s = 0; s < kEighPair / 4; ++s) {
      const double a = pa[s * 4];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = MT<double>::mma(a, pb[s * 4 * LDC + 16 * t], acc[t]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = r0 + 16 * wave + MT<double>::drow(lane, r);
      if (row >= rend) continue;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int col = 16 * t + fc;
        if (col < kEighB)
          wi[row * kEighB + col] = acc[t][r];
        else
          wj[row * kEighB + col - kEighB] = acc[t][r];
      }
    }
  }
}

struct EighSweepArgs {
  const double* meas;  // rounds x pairs x 2
  int64_t count;       // rounds x pairs
  EighSweepRecord* rec;  // this sweep's
};

__global__ __launch_bounds__(kEighThreads) void eigh_sweep_kernel(EighSweepArgs g) {
  __shared__ double sv[kEighThreads];
  const int tid = (int)threadIdx.x;
  double mx = 0.0, rotated = 0.0;
  for (int64_t i = tid; i < g.count; i += kEighThreads) {
    mx = eigh_max(mx, g.meas[2 * i]);
    rotated += g.meas[2 * i + 1] == 0.0 ? 1.0 : 0.0;
  }
  mx = eigh_block_reduce(mx, sv, tid, eigh_max);
  rotated = eigh_block_reduce(rotated, sv, tid, [](double p, double q) { return p + q; });
  if (tid == 0) g.rec->max_measure = mx, g.rec->rotated = rotated;
}

// ---- BLOCKED: the finish ----------------------------------------------------------------------------------------------------
struct EighFinishArgs {
  double* wp;        // the panels: W, then U in place
  int64_t n, nb;
  const double* a;   // the caller's matrix: the Rayleigh quotients read its lower triangle
  int64_t lda;
  double* cols;      // [0, nc): lambda; [nc, 2 nc): the signed norm; [2 nc, 3 nc): the rank; nc = nb kEighB
  double* ray;       // per block and row block of 64: the kEighB partial quotients
  double* w;
  double* v;
  int64_t ldv;
};

// Workgroup = block.  Thread (c, part) walks the rows part, part + 8, ... of column c; the eight parts are added in order.
// The sums of squares are kept in two doubles (EighSum): the norm decides the length of u_i and with it the quotient.
__global__ __launch_bounds__(kEighThreads) void eigh_colnorm_kernel(EighFinishArgs g) {
  __shared__ double ssum[kEighThreads], slo[kEighThreads], sbest[kEighThreads], ssgn[kEighThreads];
  __shared__ int64_t srow[kEighThreads];
  const int tid = (int)threadIdx.x, c = tid & (kEighB - 1), part = tid / kEighB;
  constexpr int kParts = kEighThreads / kEighB;
  const int64_t blk = blockIdx.x, nc = g.nb * kEighB;
  const double* wp = g.wp + blk * g.n * kEighB;
  EighSum sum;
  double best = -1.0, sgn = 1.0;
  int64_t brow = 0;
  for (int64_t row = part; row < g.n; row += kParts) {
    const double x = wp[row * kEighB + c];
    sum.add_product(x, x);
    if (fabs(x) > best) best = fabs(x), sgn = x < 0.0 ? -1.0 : 1.0, brow = row;
  }
  ssum[tid] = sum.hi, slo[tid] = sum.lo, sbest[tid] = best, ssgn[tid] = sgn, srow[tid] = brow;
  __syncthreads();
  if (part == 0) {
    for (int q = 1; q < kParts; ++q) {
      const int o = q * kEighB + c;
      EighSum other;
      other.hi = ssum[o], other.lo = slo[o];
      sum.add_sum(other);
      if (sbest[o] > best || (sbest[o] == best && srow[o] < brow)) best = sbest[o], sgn = ssgn[o], brow = srow[o];
    }
    g.cols[nc + blk * kEighB + c] = sgn * __builtin_sqrt(sum.value());
  }
}

// grid (blocks, chunks of 64 rows): u_i = w_i / (sign_i |w_i|), in place
__global__ __launch_bounds__(kEighThreads) void eigh_unit_kernel(EighFinishArgs g) {
  const int64_t blk = blockIdx.x, r0 = (int64_t)blockIdx.y * 64, nc = g.nb * kEighB;
  for (int e = (int)threadIdx.x; e < 64 * kEighB; e += kEighThreads) {
    const int64_t row = r0 + e / kEighB, col = blk * kEighB + e % kEighB;
    if (row < g.n && col < g.n) {
      double* x = g.wp + (blk * g.n + row) * kEighB + e % kEighB;
      *x = *x / g.cols[nc + col];
    }
  }
}

// grid (blocks, row blocks of 64).  Workgroup (blk, R): Y = A[R, :] U[:, blk] over the mirrored lower triangle of a on the MFMA
// -- the tile left of the diagonal as a [row][k] image, the diagonal tile mirrored into one, the tile right of it read as the
// block below the diagonal block into a [k][row] image -- then the partial quotients sum_r u_ri y_ri of the 64 rows, in order.
__global__ __launch_bounds__(kEighThreads) void eigh_rayleigh_kernel(EighFinishArgs g) {
  constexpr int LDR = kEighRowLd, LDC = kEighColLd, LDU = kEighRayUld, LDP = kEighB + 1;
  extern __shared__ uint4 eigh_smem[];
  double* At = reinterpret_cast<double*>(eigh_smem);  // [64][LDR] or [64][LDC]; then the products [64][LDP]
  double* Ut = At + 64 * LDC;                         // [64][LDU]; then the rows of U [64][LDP]
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, fc = lane & 15, kq = lane >> 4;
  const int64_t blk = blockIdx.x, rb = blockIdx.y, nt = eigh_ceil_div(g.n, 64), r0 = rb * 64;
  const double* up = g.wp + blk * g.n * kEighB;
  MT<double>::acc_t acc[2];
  acc[0] = acc[1] = MT<double>::acc_t{0, 0, 0, 0};
  for (int64_t cb = 0; cb < nt; ++cb) {
    const int64_t c0 = cb * 64;
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += kEighThreads) {
      const int hi = e >> 6, lo = e & 63;  // lo runs along the rows of memory
      if (cb < rb) {
        At[hi * LDR + lo] = r0 + hi < g.n ? g.a[(r0 + hi) * g.lda + c0 + lo] : 0.0;
      } else if (cb == rb) {
        const int r = hi >= lo ? hi : lo, c = hi >= lo ? lo : hi;
        At[hi * LDR + lo] = r0 + r < g.n ? g.a[(r0 + r) * g.lda + r0 + c] : 0.0;
      } else {
        At[hi * LDC + lo] = (c0 + hi < g.n && r0 + lo < g.n) ? g.a[(c0 + hi) * g.lda + r0 + lo] : 0.0;
      }
    }
    for (int e = tid; e < 64 * kEighB; e += kEighThreads) {
      const int kk = e / kEighB, cc = e % kEighB;
      Ut[kk * LDU + cc] = c0 + kk < g.n ? up[(c0 + kk) * kEighB + cc] : 0.0;
    }
    __syncthreads();
    const double* pa = cb <= rb ? At + (16 * wave + fc) * LDR + kq : At + kq * LDC + 16 * wave + fc;
    const int sa = cb <= rb ? 4 : 4 * LDC;
    const double* pb = Ut + kq * LDU + fc;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const double av = pa[s * sa];
      acc[0] = MT<double>::mma(av, pb[s * 4 * LDU], acc[0]);
      acc[1] = MT<double>::mma(av, pb[s * 4 * LDU + 16], acc[1]);
    }
  }
  __syncthreads();
  for (int e = tid; e < 64 * kEighB; e += kEighThreads) {
    const int rr = e / kEighB, cc = e % kEighB;
    Ut[rr * LDP + cc] = r0 + rr < g.n ? up[(r0 + rr) * kEighB + cc] : 0.0;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 16 * wave + MT<double>::drow(lane, r);
    At[row * LDP + fc] = acc[0][r];
    At[row * LDP + 16 + fc] = acc[1][r];
  }
  __syncthreads();
  if (tid < kEighB) {
    EighSum s;
    for (int rr = 0; rr < 64; ++rr) s.add_product(Ut[rr * LDP + tid], At[rr * LDP + tid]);
    g.ray[(blk * nt + rb) * kEighB + tid] = s.value();
  }
}

// thread = column: the partial quotients added over the row blocks, in order, and divided by u^T u of the rounded u -- the
// rounding of the normalisation (delta in the norm is 2 delta lambda in the quotient) cancels
__global__ __launch_bounds__(kEighThreads) void eigh_lambda_kernel(EighFinishArgs g) {
  const int64_t i = (int64_t)blockIdx.x * kEighThreads + threadIdx.x, nt = eigh_ceil_div(g.n, 64);
  if (i >= g.n) return;
  const double* part = g.ray + (i / kEighB) * nt * kEighB + i % kEighB;
  EighSum s, q;
  for (int64_t rb = 0; rb < nt; ++rb) s.add(part[rb * kEighB]);
  const double* u = g.wp + (i / kEighB) * g.n * kEighB + i % kEighB;
  for (int64_t row = 0; row < g.n; ++row) q.add_product(u[row * kEighB], u[row * kEighB]);
  g.cols[i] = s.value() / q.value();
}

// thread = column
__global__ __launch_bounds__(kEighThreads) void eigh_rank_kernel(EighFinishArgs g) {
  const int64_t i = (int64_t)blockIdx.x * kEighThreads + threadIdx.x, nc = g.nb * kEighB;
  if (i >= g.n) return;
  const double li = g.cols[i];
  int64_t rank = 0;
  for (int64_t j = 0; j < g.n; ++j) {
    const double lj = g.cols[j];
    rank += (lj < li || (lj == li && j < i)) ? 1 : 0;
  }
  g.cols[2 * nc + i] = (double)rank;
  g.w[rank] = li;
}

// grid (blocks, chunks of 64 rows): V[:, rank_i] = u_i
__global__ __launch_bounds__(kEighThreads) void eigh_scatter_kernel(EighFinishArgs g) {
  const int64_t blk = blockIdx.x, r0 = (int64_t)blockIdx.y * 64, nc = g.nb * kEighB;
  for (int e = (int)threadIdx.x; e < 64 * kEighB; e += kEighThreads) {
    const int64_t row = r0 + e / kEighB, col = blk * kEighB + e % kEighB;
    if (row < g.n && col < g.n) g.v[row * g.ldv + (int64_t)g.cols[2 * nc + col]] = g.wp[(blk * g.n + row) * kEighB + e % kEighB];
  }
}

}  // namespace k
}  // namespace corrla
