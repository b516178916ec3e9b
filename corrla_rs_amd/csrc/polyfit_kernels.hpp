// Polynomial response surfaces (corrla_polyfit_gram_* / corrla_poly_eval_*; linear_fit, quad_fit, quad_eval and
// jac_from_quad, stats_corr.rs:146-249) on v_mfma_f64_16x16x4_f64.  The geometry is polyfit_plan.hpp's.
//
// polyfit_gram_kernel<T, NORM>: one workgroup per (tile pair bi <= bj, slab of samples).  A chunk of 32 samples is staged
// once as AUGMENTED rows xt = [z_1 .. z_k, 1, y_1 .. y_r, 0] in f64 (z = (x - mu) * fl(1 / sigma) with NORM, x itself without; an
// f32 x or y is read in place and widened here, which is exact; rows beyond the slab are exact zeros, the one included);
// the loads of the next chunk are in flight, in registers, while the MFMAs of this one run.
// Every column of W = [V(z), y] is the product of two entries of that row, named by the plan's table, so a wave forms its
// operand fragments with two LDS reads and one multiply per element and the m x p Vandermonde matrix never exists.  Each
// of the four waves owns 64 x 64 of the tile as 4 x 4 MFMA tiles, as syrk_kernel does; the partial tile goes to the slab
// workspace with vector stores.  No atomics: a fixed input gives a bitwise fixed output.
// polyfit_finish_kernel: the slabs in index order, both triangles of G from one value.
//
// poly_eval_kernel<T>: one workgroup per 64 rows.  The rows are staged once as xt = [x_1 .. x_k, 1] in f64; for every
// right-hand side the workgroup walks the symmetric coefficient matrix C in blocks of 32 columns, forms T = Xt C on the
// MFMAs and adds rowdot(T, Xt) -- V(x) c = xt^T C xt -- and, asked for the gradient, writes 2 T[:, :k].  Rows are
// independent and every sum has a fixed order: bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "colvar_kernels.hpp"  // cv_load
#include "hip_kernels.hpp"     // MT<double>
#include "polyfit_plan.hpp"

namespace corrla {
namespace k {

template <class T>
struct PolyGramArgs {
  const T* x;       // m x kf row-major, ldx
  int64_t m, ldx;
  const T* y;       // m x r row-major, ldy (r == 0: unused)
  int64_t ldy;
  int kf, r;
  int aligned;      // 16-byte loads are legal for x ...
  int y_aligned;    // ... and for y
  const double* mu; // NORM: kf column means and scales (1 for a constant column)
  const double* sd;
  const int32_t* table;  // poly_pair_table: nb * 128 packed pairs
  int64_t slab_rows, npairs;
  int aug_ld;
  double* ws;       // [slab][pair][128][128] partial tiles
};

// cols columns of `src` (row-major, ld) for the chunk's rows into the augmented rows at column offset `at`: load, widen,
// normalise and store in one go.  The evaluation stages its row tile once with this; the Gram kernel, which stages a chunk
// per 128 MFMAs, uses the two halves below.
template <class T, bool NORM>
__device__ __forceinline__ void poly_stage_block(const T* __restrict__ src, int64_t ld, int cols, int aligned, int64_t row0, int64_t r_end,
                                                 int nrows, double* __restrict__ xt, int xld, int at, const double* mu_s,
                                                 const double* sd_s, int tid) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int nu = (cols + VEC - 1) / VEC;
  for (int u = tid; u < nrows * nu; u += kPolyThreads) {
    const int lr = u / nu, col = (u - lr * nu) * VEC;
    const int nv = min(VEC, cols - col);
    const int64_t row = row0 + lr;
    const bool live = row < r_end;
    T e[VEC];
    if (live) {
      cv_load<T, VEC>(src + row * ld + col, aligned && nv == VEC, nv, e);
    } else {
#pragma unroll
      for (int v = 0; v < VEC; ++v) e[v] = (T)0;
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v)
      if (v < nv) {
        double d = (double)e[v];
        if (NORM && live) d = (d - mu_s[col + v]) * sd_s[col + v];
        xt[lr * xld + at + col + v] = d;
      }
  }
}

// The same staging in two halves, so that the loads of the next chunk are in flight while the MFMAs of this one run:
// poly_fetch reads a thread's units (16 bytes each; unit tid + 256 q is the same (row, columns) of every chunk) into
// registers, poly_store widens, normalises and writes them to the augmented rows.  MAXU: units per thread at the widest block.
template <class T, int MAXU>
__device__ __forceinline__ void poly_fetch(const T* __restrict__ src, int64_t ld, int cols, int aligned, int64_t row0, int64_t r_end,
                                           int nrows, int tid, T (&e)[MAXU][16 / (int)sizeof(T)]) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int nu = (cols + VEC - 1) / VEC;
#pragma unroll
  for (int q = 0; q < MAXU; ++q) {
    const int u = tid + q * kPolyThreads;
    if (u < nrows * nu) {
      const int lr = u / nu, col = (u - lr * nu) * VEC;
      const int nv = min(VEC, cols - col);
      const int64_t row = row0 + lr;
      if (row < r_end) {
        cv_load<T, VEC>(src + row * ld + col, aligned && nv == VEC, nv, e[q]);
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) e[q][v] = (T)0;
      }
    }
  }
}
template <class T, bool NORM, int MAXU>
__device__ __forceinline__ void poly_store(const T (&e)[MAXU][16 / (int)sizeof(T)], int cols, int64_t row0, int64_t r_end, int nrows,
                                           double* __restrict__ xt, int xld, int at, const double* mu_s, const double* sd_s, int tid) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int nu = (cols + VEC - 1) / VEC;
#pragma unroll
  for (int q = 0; q < MAXU; ++q) {
    const int u = tid + q * kPolyThreads;
    if (u < nrows * nu) {
      const int lr = u / nu, col = (u - lr * nu) * VEC;
      const int nv = min(VEC, cols - col);
      const bool live = row0 + lr < r_end;
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        if (v < nv) {
          double d = (double)e[q][v];
          if (NORM && live) d = (d - mu_s[col + v]) * sd_s[col + v];
          xt[lr * xld + at + col + v] = d;
        }
    }
  }
}

template <class T, bool NORM>
__global__ __launch_bounds__(kPolyThreads) void polyfit_gram_kernel(PolyGramArgs<T> g) {
  constexpr int BT = kPolyBT, KT = kPolyKT;
  typedef MT<double>::acc_t acc_t;
  extern __shared__ uint4 poly_smem[];
  double* xt = reinterpret_cast<double*>(poly_smem);
  const int ld = g.aug_ld, one = g.kf, zero = g.kf + 1 + g.r;
  double* mu_s = xt + KT * ld;
  double* sd_s = mu_s + g.kf;
  int bi, bj;
  syrk_pair((int64_t)blockIdx.x, &bi, &bj);
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1, fc = lane & 15, kq = lane >> 4;

  // the two entries of the augmented row behind each of this lane's four I columns and four J columns
  int ia[4], ja[4], ib[4], jb[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int32_t ei = g.table[bi * BT + 64 * wi + 4 * fc + t], ej = g.table[bj * BT + 64 * wj + 4 * fc + t];
    ia[t] = ei & 0xffff, ja[t] = ei >> 16;
    ib[t] = ej & 0xffff, jb[t] = ej >> 16;
  }
  if (NORM)
    for (int c = tid; c < g.kf; c += kPolyThreads) {
      mu_s[c] = g.mu[c];
      sd_s[c] = 1.0 / g.sd[c];  // z = (x - mu) * fl(1 / sigma): one correctly rounded division per column, none per sample
    }
  if (tid < KT) xt[tid * ld + zero] = 0.0;  // what the columns of a ragged last tile multiply: written once
  __syncthreads();

  const int64_t r_begin = (int64_t)blockIdx.y * g.slab_rows;
  const int64_t r_end = min(g.m, r_begin + g.slab_rows);
  const int64_t nchunks = r_end > r_begin ? (r_end - r_begin + KT - 1) / KT : 0;

  acc_t acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = acc_t{0, 0, 0, 0};

  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int UX = KT * (kPolyMaxK / VEC) / kPolyThreads, UY = KT * (kPolyMaxRhs / VEC) / kPolyThreads;
  static_assert(UX * kPolyThreads == KT * (kPolyMaxK / VEC) && UY * kPolyThreads == KT * (kPolyMaxRhs / VEC),
                "the units of the widest chunk split evenly over the threads");
  T ex[UX][VEC], ey[UY][VEC];
  auto fetch = [&](int64_t c) {
    const int64_t row0 = r_begin + c * KT;
    poly_fetch<T, UX>(g.x, g.ldx, g.kf, g.aligned, row0, r_end, KT, tid, ex);
    if (g.r > 0) poly_fetch<T, UY>(g.y, g.ldy, g.r, g.y_aligned, row0, r_end, KT, tid, ey);
  };
  if (nchunks > 0) fetch(0);
  for (int64_t c = 0; c < nchunks; ++c) {
    const int64_t row0 = r_begin + c * KT;
    poly_store<T, NORM, UX>(ex, g.kf, row0, r_end, KT, xt, ld, 0, mu_s, sd_s, tid);
    if (g.r > 0) poly_store<T, false, UY>(ey, g.r, row0, r_end, KT, xt, ld, g.kf + 1, nullptr, nullptr, tid);
    if (tid < KT) xt[tid * ld + one] = row0 + tid < r_end ? 1.0 : 0.0;
    __syncthreads();
    if (c + 1 < nchunks) fetch(c + 1);  // in flight while the MFMAs below run
    const double* xr = xt + kq * ld;
#pragma unroll
    for (int kk = 0; kk < KT / 4; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        a[t] = xr[ia[t]] * xr[ja[t]];
        b[t] = xr[ib[t]] * xr[jb[t]];
      }
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = MT<double>::mma(a[ti], b[tj], acc[ti][tj]);
      xr += 4 * ld;
    }
    __syncthreads();
  }

  // D of MFMA tile (ti, tj): row = drow(lane, r) <-> I column 64 wi + 4 row + ti; col = fc <-> J column 64 wj + 4 fc + tj.
  // The four tj of a lane are four consecutive J columns: two 16-byte stores.
  double* out = g.ws + ((int64_t)blockIdx.y * g.npairs + (int64_t)blockIdx.x) * (BT * BT);
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 64 * wi + 4 * MT<double>::drow(lane, r) + ti;
      double v[4] = {acc[ti][0][r], acc[ti][1][r], acc[ti][2][r], acc[ti][3][r]};
      double* dst = out + row * BT + 64 * wj + 4 * fc;
      uint4 raw[2];
      __builtin_memcpy(raw, v, sizeof(raw));
      reinterpret_cast<uint4*>(dst)[0] = raw[0];
      reinterpret_cast<uint4*>(dst)[1] = raw[1];
    }
}

// One workgroup per (pair, 32 x 32 sub-tile): G(i, j) = the slabs' partial sums in index order; G(i, j) and G(j, i) are
// written from the same value (the mirror goes through LDS so that both writes are coalesced).  On a diagonal pair only
// the sub-tiles on and above the diagonal are taken, and inside a diagonal sub-tile every entry reads the partial sums of
// its upper-triangle twin.
struct PolyFinishArgs {
  const double* ws;
  int64_t nsplit, npairs, n;
  double* g;
  int64_t ldg;
};

__global__ __launch_bounds__(256) void polyfit_finish_kernel(PolyFinishArgs g) {
  constexpr int BT = kPolyBT;
  __shared__ double tile[32][33];
  int bi, bj;
  syrk_pair((int64_t)blockIdx.x, &bi, &bj);
  const int si = (int)blockIdx.y >> 2, sj = (int)blockIdx.y & 3;
  const bool diag_pair = bi == bj;
  if (diag_pair && si > sj) return;
  const bool diag_sub = diag_pair && si == sj;
  const int tx = (int)threadIdx.x & 31, ty = (int)threadIdx.x >> 5;
  const int64_t i0 = (int64_t)bi * BT + si * 32, j0 = (int64_t)bj * BT + sj * 32;
  const double* base = g.ws + (int64_t)blockIdx.x * (BT * BT);
  const int64_t slab_stride = g.npairs * (BT * BT);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int li = ty + 8 * q, lj = tx;
    const int64_t i = i0 + li, j = j0 + lj;
    double s = 0.0;
    if (i < g.n && j < g.n) {
      const int ui = (diag_sub && li > lj) ? lj : li, uj = (diag_sub && li > lj) ? li : lj;
      const double* p = base + (si * 32 + ui) * BT + sj * 32 + uj;
#pragma unroll 4
      for (int64_t b = 0; b < g.nsplit; ++b) s += p[b * slab_stride];
      g.g[i * g.ldg + j] = s;
    }
    tile[li][lj] = s;
  }
  if (diag_sub) return;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int lj = ty + 8 * q, li = tx;  // G(j, i), coalesced along i
    const int64_t i = i0 + li, j = j0 + lj;
    if (i < g.n && j < g.n) g.g[j * g.ldg + i] = tile[li][lj];
  }
}

// ---- evaluation ------------------------------------------------------------------------------------------------------------
// The r images of C, [j][k4 rows][ncols columns] zero padded, from the coefficients in the reference's layout
// ([x, x_a x_b (a <= b, a outer), 1] or [x, 1]; coeffs is p x r, row stride ldc):
//   C(a, a) = c_aa, C(a, b) = C(b, a) = c_ab / 2, C(a, k) = C(k, a) = c_a / 2, C(k, k) = c_0 -- the halves are exact.
__global__ void poly_c_assemble_kernel(const double* __restrict__ coeffs, int64_t ldc, int64_t p, int kf, int degree, int r, int k4,
                                       int ncols, double* __restrict__ cimg) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t per = (int64_t)k4 * ncols;
  if (e >= per * r) return;
  const int j = (int)(e / per);
  const int rr = (int)((e - j * per) / ncols), cc = (int)((e - j * per) % ncols);
  double v = 0.0;
  if (rr <= kf && cc <= kf) {
    const int a = min(rr, cc), b = max(rr, cc);
    if (b == kf) {
      v = a == kf ? coeffs[(p - 1) * ldc + j] : 0.5 * coeffs[(int64_t)a * ldc + j];
    } else if (degree >= 2) {
      const int64_t idx = kf + (int64_t)a * kf - (int64_t)a * (a - 1) / 2 + (b - a);
      v = coeffs[idx * ldc + j];
      if (a != b) v *= 0.5;
    }
  }
  cimg[e] = v;
}

template <class T>
struct PolyEvalArgs {
  const T* x;     // m x kf row-major, ldx
  int64_t m, ldx;
  int kf, r;
  int aligned;
  const double* cimg;  // poly_c_assemble_kernel
  int k4, xld, ncb;
  T* out;         // m x r row-major, ld_out
  int64_t ld_out;
  T* jac;         // nullable: r slabs of m x kf, row stride ld_jac, slab stride m * ld_jac
  int64_t ld_jac;
};

template <class T>
__global__ __launch_bounds__(kPolyThreads) void poly_eval_kernel(PolyEvalArgs<T> g) {
  constexpr int BM = kPolyEvalBM, CB = kPolyEvalCB, CLD = kPolyEvalCLd;
  typedef MT<double>::acc_t acc_t;
  extern __shared__ uint4 poly_smem[];
  double* xs = reinterpret_cast<double*>(poly_smem);
  const int xld = g.xld, kf = g.kf, k1 = g.kf + 1;
  double* cs = xs + BM * xld;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, fc = lane & 15, kq = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * BM;

  // the row tile, once: x widened, then the one and zeros up to the row stride; rows beyond m are zeros
  poly_stage_block<T, false>(g.x, g.ldx, kf, g.aligned, row0, g.m, BM, xs, xld, 0, nullptr, nullptr, tid);
  for (int e = tid; e < BM * (xld - kf); e += kPolyThreads) {
    const int lr = e / (xld - kf), c = kf + e % (xld - kf);
    xs[lr * xld + c] = (c == kf && row0 + lr < g.m) ? 1.0 : 0.0;
  }
  const int ncols = g.ncb * CB;
  const int lrow = 16 * wave + fc;  // the row this lane feeds to the MFMAs
  for (int j = 0; j < g.r; ++j) {
    double val[4] = {0.0, 0.0, 0.0, 0.0};
    const double* cj = g.cimg + (int64_t)j * g.k4 * ncols;
    for (int cb = 0; cb < g.ncb; ++cb) {
      __syncthreads();  // the row tile is staged / the previous block of C is done with
      for (int e = tid; e < g.k4 * CB; e += kPolyThreads) {
        const int rr = e / CB, cc = e % CB;
        cs[rr * CLD + cc] = cj[(int64_t)rr * ncols + cb * CB + cc];
      }
      __syncthreads();
      acc_t acc[2] = {acc_t{0, 0, 0, 0}, acc_t{0, 0, 0, 0}};
      const double* pa = xs + lrow * xld + kq;
      const double* pb = cs + kq * CLD + fc;
      for (int kk = 0; kk < g.k4 / 4; ++kk) {
        const double a = pa[4 * kk];
        const double b0 = pb[4 * kk * CLD], b1 = pb[4 * kk * CLD + 16];
        acc[0] = MT<double>::mma(a, b0, acc[0]);
        acc[1] = MT<double>::mma(a, b1, acc[1]);
      }
      // D: row = drow(lane, q) of the wave's 16 rows, col = fc of the 16-wide column tile
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int col = cb * CB + 16 * t + fc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int lr = 16 * wave + MT<double>::drow(lane, q);
          const double tij = acc[t][q];
          if (col < k1) val[q] += tij * xs[lr * xld + col];
          if (g.jac && col < kf && row0 + lr < g.m)
            g.jac[((int64_t)j * g.m + row0 + lr) * g.ld_jac + col] = (T)(2.0 * tij);
        }
      }
    }
    // the 16 lanes of a row hold the columns fc, fc + 16, ...: a butterfly of fixed shape adds them
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) val[q] += __shfl_xor(val[q], off);
      const int64_t row = row0 + 16 * wave + MT<double>::drow(lane, q);
      if (fc == 0 && row < g.m) g.out[row * g.ld_out + j] = (T)val[q];
    }
  }
}

}  // namespace k
}  // namespace corrla
