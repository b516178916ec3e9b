// The Cholesky-QR kernels of the thin-Q (gfx950): factor-and-invert of the l x l Gram in one workgroup, plain and robust
// (chol_inv_kernel), the inspection and the pass verdict of the 2 x 2 blocked form (gram_inspect_kernel,
// combine_need_kernel), the re-seeding of null columns (refill_null_kernel) and the (I + E)^(-1/2) series of the
// host-controlled polishing pass.  thinq_plan.hpp sizes and routes every launch, thinq_stage.hpp launches them; the status
// record and the need_next bits they share with the core SVD and the driver are in thinq_plan.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_kernels.hpp"  // normal_from_index
#include "thinq_plan.hpp"   // CholStatus, kNeed*, chol_inv_threads / chol_inv_lds_bytes / chol_inv_max_threads

namespace corrla {
namespace k {

// ---- device Cholesky + triangular inverse for the Cholesky-QR passes --------------------------------
// One workgroup: G (r x r, symmetric, column-major) -> M = R^-1 with G = R^T R (upper R), written into the
// zero-padded skinny operand of the following apply GEMM.  G and M live in LDS.  status: fail = 0 ok / 1 =
// pivot failure (M is then the identity: the apply becomes a no-op copy) / 2 = zero matrix / 3 = non-finite; [1] = min pivot
// ratio d_j / g_jj, [2] = max |G - I| (both as float bits).  Lets the two passes of a CholeskyQR2 be enqueued
// without any host round trip; the host inspects the status words once at the end.
__device__ inline float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ inline double fast_rcp(double x) {
  double y = __builtin_amdgcn_rcp(x);
  return y * (2.0 - x * y);
}
__device__ inline float fast_rsqrt(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ inline double fast_rsqrt(double x) {
  double y = __builtin_amdgcn_rsq(x);
  return y * (1.5 - 0.5 * x * y * y);
}
// Robust form (rq.need_next != nullptr), used by the device-side Cholesky-QR that never asks the host:
//  * the factorisation is that of G + shift_rel * max_i g_ii * I whenever the Gram is further than 0.25 from I (or
//    always: shift_mode 1; never: shift_mode 2).  A shifted factor stays non-singular however ill-conditioned the
//    sketch is, the product Y R_s^-1 keeps the span of Y and AMPLIFIES its weak directions by up to 1 / sqrt(shift_rel)
//    relative to the strong ones -- they come from Y itself, not from the (squared) Gram -- so a few shifted passes
//    unfold condition numbers up to 1 / eps like a Householder QR does (shifted CholeskyQR3, Fukaya et al. 2020);
//  * a pivot that fails the test all the same (an exactly zero column, or a shift below the Gram's rounding error)
//    is a NULL column instead of a failure: it is skipped, column j of R^-1 is zero (the applied product leaves a zero
//    column that refill_null_kernel replaces by a random one) and null_mask[j] = 1;
//  * need_next <- 1 when the product of this pass cannot be orthonormal to working precision yet (it was shifted, has
//    null columns, or its Gram was further than 0.25 from I), else 0: the kernels of the next pass carry it as their
//    run_if word;
//  * run_if: the whole launch does nothing when *run_if == 0.
struct CholRobust {
  float shift_rel;
  int shift_mode;  // 0: shift iff ||G - I||_max > 0.25, 1: always, 2: never
  float null_excess;  // > 0 (shifted passes only): a column whose pivot exceeds the shift by less than null_excess * shift
                      // -- it lies below the level one shifted pass can lift -- is a null column as well (in-loop
                      // re-orthonormalisations: such directions are re-seeded at random rather than kept as noise)
  int* need_next;
  int* null_mask;  // r words
  const int* run_if;
  float need_ratio;  // > 0 (the single pass of an in-loop thin-Q): need_next <- null columns or a pivot ratio d_j / g_jj below
                     // this, i.e. the sketch was too ill-conditioned for one shifted pass to tame; 0: the standard rule
  const void* abs_shift;  // optional (2 x 2 blocked factorisation): device scalar T = the shift gram_inspect_kernel has
                          // ALREADY added to the diagonal of the whole Gram; decides `shifted` and feeds the null test
};
// what gram_inspect_kernel leaves for the blocked factorisation of one pass
template <class T>
struct GramInspect {
  T shift;      // absolute shift added to the diagonal (0: none)
  int shifted;
  int bad;      // non-finite entries
  float d2;     // ||G - I||_max before the shift
  float gmax;
};
// One workgroup: inspects the l x l Gram (column-major, ld), decides the shift like the robust chol_inv_kernel does
// (mode 0: iff ||G - I||_max > 0.25, 1: always, 2: never), adds it to the diagonal and leaves the record.
template <class T>
__global__ __launch_bounds__(1024) void gram_inspect_kernel(T* g, int64_t ld, int l, float shift_rel, int shift_mode,
                                                            GramInspect<T>* out, const int* run_if) {
  if (run_if && *run_if == 0) return;
  __shared__ float rd[16];
  __shared__ T rg[16];
  __shared__ int sbad;
  const int tid = threadIdx.x;
  if (tid == 0) sbad = 0;
  // (the largest diagonal entry and the finiteness test in the element type: an f64 Gram of 2^800 or 2^-800 is inf / 0 as a
  //  float, which made a finite sketch "non-finite" and a tiny one "zero")
  float dv = 0.f;
  T gm = (T)0;
  int bad = 0;
  for (int idx = tid; idx < l * l; idx += 1024) {
    const int j = idx / l, i = idx - j * l;
    const T x = g[(int64_t)j * ld + i];
    if (!(fabs(x) < (sizeof(T) == 4 ? (T)3.0e38f : (T)1.0e300))) bad = 1;
    dv = fmaxf(dv, (float)fabs(x - (i == j ? (T)1 : (T)0)));
    if (i == j) gm = fmax(gm, x);
  }
  for (int off = 32; off > 0; off >>= 1) {
    dv = fmaxf(dv, __shfl_down(dv, off, 64));
    gm = fmax(gm, __shfl_down(gm, off, 64));
  }
  __syncthreads();
  if ((tid & 63) == 0) {
    rd[tid >> 6] = dv;
    rg[tid >> 6] = gm;
  }
  if (bad) sbad = 1;
  __syncthreads();
  dv = 0.f;
  gm = (T)0;
  for (int i = 0; i < 16; ++i) {
    dv = fmaxf(dv, rd[i]);
    gm = fmax(gm, rg[i]);
  }
  const bool shifted = !sbad && gm > (T)0 && shift_rel > 0.f && (shift_mode == 1 || (shift_mode == 0 && dv > 0.25f));
  // (within float range the shift is taken from the float value, as it always was)
  const T sh = shifted ? (T)shift_rel * ((gm < (T)3.0e38f && gm > (T)1.0e-37f) ? (T)(float)gm : gm) : (T)0;
  if (shifted)
    for (int i = tid; i < l; i += 1024) g[(int64_t)i * ld + i] += sh;
  if (tid == 0) {
    out->shift = sh;
    out->shifted = shifted ? 1 : 0;
    out->bad = sbad;
    out->d2 = dv;
    out->gmax = (float)gm;
  }
}
template <class T>
__global__ void combine_need_kernel(int* need, const GramInspect<T>* insp, const int* na, const int* nb, const int* run_if) {
  if (run_if && *run_if == 0) return;
  // insp == nullptr (the single pass of an in-loop thin-Q): the verdict is that of the two block factorisations alone
  // bit 0: another pass is needed; bit 1 (kNeedNonFinite): a non-finite Gram; bit 2 (kNeedNullCols): null columns were
  // re-seeded -- the host reads the words once at the end of the call (driver.hpp: attempt_verdict)
  const int sub = *na | *nb;
  const int bad = (insp && insp->bad) ? kNeedNonFinite : 0;
  const int need1 = ((insp && (insp->shifted || insp->bad || insp->d2 > 0.05f)) || sub) ? 1 : 0;
  *need = need1 | bad | (sub & (kNeedNonFinite | kNeedNullCols));
}
template <class T>
__global__ __launch_bounds__(chol_inv_max_threads<T>()) void chol_inv_kernel(const T* __restrict__ g, int64_t ldg, int r, T piv_rel, T* m,
                                                        int64_t ldm, CholStatus* st, CholRobust rq = CholRobust{0.f, 0, 0.f, nullptr, nullptr, nullptr, 0.f, nullptr}) {
  if (rq.run_if && *rq.run_if == 0) return;
  const bool robust = rq.need_next != nullptr;
  // Register-resident Gaussian elimination of [G | I] in one sweep of r steps, one barrier per step.
  // Thread t owns the 4x4 tile (ti <= tk) of the upper triangle of G (v) and the same tile of W (w), where
  // W(x, y) = L^-1(y, x) for the unit-lower factor G = L U.  Step j: the owners of row j of the reduced G
  // publish it (rb), the owners of column j of W publish it (cb); then
  //     G(i, k) -= rb[i] rb[k] / d_j           (i > j),
  //     W(x, y) -= cb[x]  rb[y] / d_j          (x <= j < y).
  // With d_j the pivots, R = D^-1/2 U and R^-1(i, c) = W(i, c) / sqrt(d_c).  Buffers are double-buffered by
  // the parity of j so one barrier per step is enough.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nt = (r + 3) >> 2, r4 = nt * 4;
  T* rowbuf = (T*)smem;          // [2][r4]
  T* colbuf = rowbuf + 2 * r4;   // [2][r4]
  T* diag0 = colbuf + 2 * r4;    // [r4] original diagonal
  T* dis = diag0 + r4;           // [r4] 1 / sqrt(d_j)
  float* red = (float*)(dis + r4);  // [32]
  const int tid = threadIdx.x, nwave = blockDim.x >> 6;
  const int ntri = nt * (nt + 1) / 2;
  const bool own = tid < ntri;
  int ti = 0, tk = 0;
  if (own) {
    // row-major over the upper triangle of tiles (ti ascending), so that whole waves retire from the
    // G-update once tj passes their rows
    const int e = ntri - 1 - tid;
    int c = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
    while (c * (c + 1) / 2 > e) --c;
    while ((c + 1) * (c + 2) / 2 <= e) ++c;
    ti = nt - 1 - c;
    tk = nt - 1 - (e - c * (c + 1) / 2);
  }
  const int i0 = 4 * ti, k0 = 4 * tk;
  T v[4][4], w[4][4];
  float dv = 0.f, gm = 0.f;
  int bad = 0;
  // the tile's 16 loads are unconditional (clamped indices) and issued together: one branch per element put an
  // s_waitcnt vmcnt(0) behind every load -- 16 dependent L2 round trips in front of the elimination
#pragma unroll
  for (int aa = 0; aa < 4; ++aa)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = min(i0 + aa, r - 1), k = min(k0 + b, r - 1);
      v[aa][b] = g[(int64_t)k * ldg + i];
    }
  // Scale invariance.  The inspection below works in float and the elimination takes hardware reciprocals of its pivots: a
  // Gram far from unit scale (an f64 sketch beyond 1e19 or below 1e-22, whose Gram is inf or 0 as a float; an f32 sketch
  // whose small pivots are subnormal) is multiplied by the exact power of four that brings its largest diagonal entry
  // into [1/2, 2), and R^-1 is scaled back on output.  Grams within 2^-40 .. 2^40 are left as they are.
  int h = 0;
  {
    T gt = (T)0;
    if (own && ti == tk) {
#pragma unroll
      for (int aa = 0; aa < 4; ++aa)
        if (i0 + aa < r) gt = fmax(gt, v[aa][aa]);
    }
    for (int off = 32; off > 0; off >>= 1) gt = fmax(gt, __shfl_down(gt, off, 64));
    // (one word per wave, at most 16 waves, in the 32-float scratch that thinq_plan.hpp: chol_inv_lds_bytes reserves)
    static_assert(16 * sizeof(T) <= 32 * sizeof(float), "the wave maxima in the element type must fit the float scratch");
    T* redt = (T*)red;
    if ((tid & 63) == 0) redt[tid >> 6] = gt;
    __syncthreads();
    gt = (T)0;
    for (int i = 0; i < nwave; ++i) gt = fmax(gt, redt[i]);
    __syncthreads();
    if (gt <= std::numeric_limits<T>::max() && (gt > (T)1099511627776.0 || (gt > (T)0 && gt < (T)9.094947017729282e-13))) {
      int e;
      (void)frexp((double)gt, &e);
      h = e >> 1;
#pragma unroll
      for (int aa = 0; aa < 4; ++aa)
#pragma unroll
        for (int b = 0; b < 4; ++b) v[aa][b] = (T)ldexp((double)v[aa][b], -2 * h);
    }
  }
#pragma unroll
  for (int aa = 0; aa < 4; ++aa)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = i0 + aa, k = k0 + b;
      const bool in = own && i < r && k < r;
      const T x = in ? v[aa][b] : (T)0;
      if (in) {
        if (!((float)fabs(x) < 3.0e38f)) bad = 1;
        dv = fmaxf(dv, (float)fabs(x - (i == k ? (T)1 : (T)0)));
        if (i == k) gm = fmaxf(gm, (float)x);
      }
      v[aa][b] = x;
      w[aa][b] = (own && i == k && i < r) ? (T)1 : (T)0;
    }
  for (int idx = tid; idx < 4 * r4; idx += blockDim.x) rowbuf[idx] = (T)0;  // rowbuf and colbuf
  if (own && ti == tk) {
#pragma unroll
    for (int aa = 0; aa < 4; ++aa) diag0[i0 + aa] = v[aa][aa];
  }
  for (int off = 32; off > 0; off >>= 1) {
    dv = fmaxf(dv, __shfl_down(dv, off, 64));
    gm = fmaxf(gm, __shfl_down(gm, off, 64));
  }
  if ((tid & 63) == 0) {
    red[tid >> 6] = dv;
    red[16 + (tid >> 6)] = gm;
  }
  bad = __syncthreads_or(bad);
  float d2 = 0.f, g2 = 0.f;
  for (int i = 0; i < nwave; ++i) {
    d2 = fmaxf(d2, red[i]);
    g2 = fmaxf(g2, red[16 + i]);
  }
  int fl = bad ? 3 : (!(g2 > 0.f) ? 2 : 0);
  float min_ratio = 1.f;
  int nnull = 0;
  if (robust && fl == 2) {
    // the zero matrix: every column is null (M = 0, all of them are refilled)
    for (int j = tid; j < r; j += blockDim.x) rq.null_mask[j] = 1;
    if (own) {
#pragma unroll
      for (int aa = 0; aa < 4; ++aa)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int i = i0 + aa, k = k0 + b;
          if (i <= k && k < r) m[(int64_t)k * ldm + i] = (T)0;
        }
    }
    if (tid == 0) {
      *rq.need_next = 1 | kNeedNullCols;
      st->fail = 0;
      st->min_ratio = 0.f;
      st->dev_i = d2;
      st->gmax = 0.f;
      st->clk = 0;
      st->wall = 0;
    }
    return;
  }
  const long long clk0 = clock64(), wall0 = wall_clock64();
  // G = I + E with a tiny E (the polishing pass of CholeskyQR2): (I + E)^(-1/2) = I - E/2 + 3E^2/8 - ..., and
  // 3 ||E||^2 / 8 is below eps / 4, so the symmetric first-order factor replaces the elimination (uniform branch).
  const float series_tol = sizeof(T) == 4 ? 2.0e-4f : 1.0e-8f;
  // (h == 0 only: d2 of a prescaled Gram is that of the SCALED one -- 4^h (I + E) would pass for I + E and the factor written
  //  here would lack its 2^-h; such a Gram goes through the elimination, whose output is scaled back)
  if (fl == 0 && h == 0 && d2 <= series_tol) {
    if (own) {
#pragma unroll
      for (int aa = 0; aa < 4; ++aa)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int i = i0 + aa, k = k0 + b;
          if (i < r && k < r) {
            const T val = (i == k ? (T)1 : (T)0) - (T)0.5 * (v[aa][b] - (i == k ? (T)1 : (T)0));
            m[(int64_t)k * ldm + i] = val;
            m[(int64_t)i * ldm + k] = val;
          }
        }
    }
    if (robust)
      for (int j = tid; j < r; j += blockDim.x) rq.null_mask[j] = 0;
    if (tid == 0) {
      if (robust) *rq.need_next = 0;
      st->fail = 0;
      st->min_ratio = 1.f;
      st->dev_i = d2;
      st->gmax = g2;
      st->clk = 0;
      st->wall = 0;
    }
    return;
  }
  // blocked form: the shift is in the diagonal already (and was scaled with it)
  const T pre_sh = rq.abs_shift ? (h ? (T)ldexp((double)*(const T*)rq.abs_shift, -2 * h) : *(const T*)rq.abs_shift) : (T)0;
  const bool shifted = rq.abs_shift ? pre_sh > (T)0
                                    : (robust && rq.shift_rel > 0.f && (rq.shift_mode == 1 || (rq.shift_mode == 0 && d2 > 0.25f)));
  const T sh = rq.abs_shift ? pre_sh : (shifted ? (T)rq.shift_rel * (T)g2 : (T)0);
  if (fl == 0 && shifted && !rq.abs_shift) {
    // shifted factorisation: G + s I, s relative to the largest diagonal entry (the diagonal tiles own the diagonal)
    if (own && ti == tk) {
#pragma unroll
      for (int aa = 0; aa < 4; ++aa)
        if (i0 + aa < r) v[aa][aa] += sh;
    }
  }
  if (fl == 0) {
    typedef T V4 __attribute__((ext_vector_type(4)));
    for (int tj = 0; tj < nt && fl == 0; ++tj) {
#pragma unroll
      for (int aj = 0; aj < 4; ++aj) {  // unrolled: the published register row / column is static
        const int j = 4 * tj + aj;
        if (j >= r) break;
        T* rb = rowbuf + (j & 1) * r4;
        T* cb = colbuf + (j & 1) * r4;
        if (own && ti == tj) *(V4*)&rb[k0] = V4{v[aj][0], v[aj][1], v[aj][2], v[aj][3]};
        if (own && tk == tj) *(V4*)&cb[i0] = V4{w[0][aj], w[1][aj], w[2][aj], w[3][aj]};
        __syncthreads();
        // every LDS read of the step is issued before the pivot test (one LDS round trip per step)
        const T d = rb[j];
        const T g0 = diag0[j];
        const V4 rk4 = *(const V4*)&rb[k0];
        const V4 ri4 = *(const V4*)&rb[i0];
        const V4 ci4 = *(const V4*)&cb[i0];
        if (!(d > piv_rel * g0) || !(g0 > (T)0) ||
            (shifted && rq.null_excess > 0.f && !(d - sh > (T)rq.null_excess * sh))) {  // uniform: every thread reads the same d
          if (!robust) {
            fl = 1;
            break;
          }
          // null column: no elimination step; its column of R^-1 is zero (dis = 0) and, the step being skipped, no
          // other column of R^-1 receives a contribution from it
          // (dis[j] = 0 marks it: the mask goes to global memory after the loop -- a global store inside it would be
          // waited for at every barrier)
          ++nnull;
          if (tid == 0) dis[j] = (T)0;
          continue;
        }
        if (tid < 64) {
          min_ratio = fminf(min_ratio, (float)d * fast_rcp((float)g0));
          if (tid == 0) {
            T rs = fast_rsqrt(d);
            rs = rs * ((T)1.5 - (T)0.5 * d * rs * rs);
            dis[j] = rs;
          }
        }
        if (own && tk >= tj) {  // tiles left of the pivot column are finished
          T rinv = fast_rcp(d);
          rinv = rinv * ((T)2 - d * rinv);
          T rk[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) rk[q] = rk4[q] * rinv;
          if (ti >= tj) {
            T ri[4] = {ri4[0], ri4[1], ri4[2], ri4[3]};
            if (ti == tj) {
#pragma unroll
              for (int q = 0; q < 4; ++q) ri[q] = (q > aj) ? ri[q] : (T)0;  // rows at or above the pivot stay
            }
#pragma unroll
            for (int aa = 0; aa < 4; ++aa)
#pragma unroll
              for (int b = 0; b < 4; ++b) v[aa][b] -= ri[aa] * rk[b];
          }
          if (ti <= tj) {
            T ci[4] = {ci4[0], ci4[1], ci4[2], ci4[3]};
            if (ti == tj) {
#pragma unroll
              for (int q = 0; q < 4; ++q) ci[q] = (q <= aj) ? ci[q] : (T)0;  // W(x, y): x <= j
            }
            if (tk == tj) {
#pragma unroll
              for (int q = 0; q < 4; ++q) rk[q] = (q > aj) ? rk[q] : (T)0;  // W(x, y): y > j
            }
#pragma unroll
            for (int aa = 0; aa < 4; ++aa)
#pragma unroll
              for (int b = 0; b < 4; ++b) w[aa][b] -= ci[aa] * rk[b];
          }
        }
      }
    }
  }
  const long long clk1 = clock64(), wall1 = wall_clock64();
  __syncthreads();
  if (robust && fl == 0)
    for (int j = tid; j < r; j += blockDim.x) rq.null_mask[j] = dis[j] == (T)0 ? 1 : 0;
  if (own) {
#pragma unroll
    for (int aa = 0; aa < 4; ++aa)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i = i0 + aa, k = k0 + b;
        if (i <= k && k < r) {
          const T val = (fl == 0) ? w[aa][b] * dis[k] : ((i == k && fl == 1) ? (T)1 : (T)0);
          m[(int64_t)k * ldm + i] = (h && fl == 0) ? (T)ldexp((double)val, -h) : val;  // R^-1 of the unscaled Gram
        }
      }
  }
  if (tid == 0) {
    // a plain pass on a Gram within 0.05 of I leaves the product orthonormal to a few eps * sqrt(m)
    if (robust) {
      int need;
      if (rq.need_ratio > 0.f)
        need = (nnull > 0 || min_ratio < rq.need_ratio || fl != 0) ? 1 : 0;
      else
        need = (nnull > 0 || d2 > 0.05f || (shifted && !rq.abs_shift) || fl != 0) ? 1 : 0;
      *rq.need_next = need | (fl == 3 ? kNeedNonFinite : 0) | (nnull > 0 ? kNeedNullCols : 0);
    }
    st->fail = fl;
    st->min_ratio = nnull > 0 ? 0.f : min_ratio;
    st->dev_i = d2;
    st->gmax = g2;
    st->clk = clk1 - clk0;
    st->wall = wall1 - wall0;
  }
}
// columns of y (m x l, column-major) marked in null_mask <- N(0, 1) / sqrt(m): the replacement of the null columns of
// a device Cholesky-QR pass (any orthonormal completion serves, random_svd.rs:38,57 -- a Householder thin-Q returns
// an arbitrary one as well); the following pass orthonormalises them against the rest.  grid = (blocks, l)
template <class T>
__global__ void refill_null_kernel(T* y, int64_t ld, int64_t m, int l, const int* null_mask, uint64_t seed, const int* run_if) {
  if (run_if && *run_if == 0) return;
  const int j = blockIdx.y;
  if (j >= l || null_mask[j] == 0) return;
  const T sc = (T)rsqrt((double)m);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
    y[(int64_t)j * ld + i] = sc * normal_from_index<T>((uint64_t)(i * l + j), seed);
}

// ---- (I + E)^(-1/2) by its Taylor series, for the polishing pass of the Cholesky-QR ---------------
// g (r x r, column-major, ld) holds G = I + E on entry, E on exit
template <class T>
__global__ void series_prep_kernel(T* g, int64_t ld, int r) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i < r && j < r && i == j) g[(int64_t)j * ld + i] -= (T)1;
}
// m = I - E/2 + 3 E^2 / 8 - 5 E^3 / 16
template <class T>
__global__ void series_combine_kernel(const T* e1, const T* e2, const T* e3, int64_t ld, int r, T* m, int64_t ldm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i >= r || j >= r) return;
  const int64_t o = (int64_t)j * ld + i;
  m[(int64_t)j * ldm + i] = (i == j ? (T)1 : (T)0) - (T)0.5 * e1[o] + (T)0.375 * e2[o] - (T)0.3125 * e3[o];
}

}  // namespace k
}  // namespace corrla
