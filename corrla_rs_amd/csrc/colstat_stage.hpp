// The column passes' launchers: each takes the plan of colstat_plan.hpp, the partial sums from the arena, launches the pass
// and its finishing kernel and computes no launch parameter of its own.  The members of HipDev that the generic entry layer
// calls (col_ss, col_ss_csr, sd_from_ss, weighted_colsum) are defined here: shape -> plan -> throw on its error -> launcher.
// Everything enqueues on the context's stream; nothing synchronises.
#pragma once
#include "colstat_plan.hpp"
#include "colvar_kernels.hpp"
#include "hip_backend.hpp"
#include "syrk_kernels.hpp"  // colmom_down_kernel, colmom_final_kernel

namespace corrla {
namespace colstat_stage {

// ss[j] (f64) = sum_i (x_ij - mu_j)^2 per data column j of the staged operand `a` (f32, f64 or bf16 bit patterns, read in
// place), in the orientation the plan was made for
template <class TI, class T>
void col_ss(HipDev& dev, const ColstatPlan& p, const Big<TI>& a, const T* mu, double* ss) {
  const int aligned = ((uintptr_t)a.p % 16 == 0 && a.ld % k::CvIn<TI>::kVec == 0) ? 1 : 0;
  const bool down = p.branch == ColstatBranch::kDown;
  double* partial = (double*)dev.alloc_bytes(p.ws_bytes);
  if (down)
    hipLaunchKernelGGL((k::colss_down_kernel<TI, T>), dim3(p.grid_x, p.grid_y), dim3(p.block), 0, dev.stream, a.p, a.rows, a.cols, a.ld,
                       a.cols_readable, aligned, mu, p.groups, p.rows_per_slab, partial);
  else
    hipLaunchKernelGGL((k::colss_along_kernel<TI, T>), dim3(p.grid_x), dim3(p.block), 0, dev.stream, a.p, a.rows, a.cols, a.ld,
                       a.cols_readable, aligned, mu, (int)p.nslab, p.seg_len, partial);
  hipLaunchKernelGGL(k::colss_final_kernel, dim3(p.final_grid_x), dim3(p.final_block), 0, dev.stream, (const double*)partial, p.nslab,
                     down ? a.cols : a.rows, ss);
  CORRLA_HIP(hipGetLastError());
}

// the same over a CSR whose ROWS are the data columns (a transpose built by csr_transpose: entries ordered by sample), the
// implicit zeros of the n_samples long columns included
template <class T>
void col_ss_csr(HipDev& dev, const ColstatPlan& p, const CsrView<T>& s, const T* mu, int64_t n_samples, double* ss) {
  double* psum = (double*)dev.alloc_bytes(p.ws_bytes / 2);
  double* pcnt = (double*)dev.alloc_bytes(p.ws_bytes / 2);
  hipLaunchKernelGGL((k::csr_colss_kernel<T>), dim3(p.grid_x), dim3(p.block), 0, dev.stream, s.val, s.ci, s.rp, s.rows, mu, (int)p.nslab,
                     psum, pcnt);
  hipLaunchKernelGGL((k::csr_colss_final_kernel<T>), dim3(p.final_grid_x), dim3(p.final_block), 0, dev.stream, (const double*)psum,
                     (const double*)pcnt, p.nslab, s.rows, mu, (double)n_samples, ss);
  CORRLA_HIP(hipGetLastError());
}

// v[c] = sum_r w[r] x(r, c) over the plan's columns of the skinny x (w == nullptr: ones)
template <class T>
void weighted_colsum(HipDev& dev, const ColstatPlan& p, const Skinny<T>& x, int64_t rows, const T* w, T* v) {
  double* partial = (double*)dev.alloc_bytes(p.ws_bytes);
  hipLaunchKernelGGL((k::wcolsum_partial_kernel<T>), dim3(p.grid_x, p.grid_y), dim3(p.block), 0, dev.stream, (const T*)x.p, x.ld, rows, w,
                     partial, (int)p.grid_y);
  hipLaunchKernelGGL((k::wcolsum_final_kernel<T>), dim3(p.final_grid_x), dim3(p.final_block), 0, dev.stream, (const double*)partial,
                     (int)p.nslab, (int)p.grid_y, v);
  CORRLA_HIP(hipGetLastError());
}

// The column moments of x (m x n row-major, ld) in one pass with f64 accumulation (colmom_down_kernel, colmom_final_kernel):
// the f64 means and standard deviations (divisor denom; 1 for a constant column), both rounded to T, and the verdict.
// Workspace of the arena; enqueues only.
template <class T>
struct ColMoments {
  double *mu64, *sd64;
  T *mu_t, *sd_t;
  int* is_const;
};
template <class T>
ColMoments<T> col_moments(HipDev& dev, const T* x, int64_t m, int64_t n, int64_t ld, int aligned, double denom) {
  const ColstatPlan p = colss_plan(m, n, k::CvIn<T>::kVec, /*along_cols=*/true, dev.num_cus);
  if (p.error) throw Error(ST_EINVAL, p.error);
  double* psum = (double*)dev.alloc_bytes(p.ws_bytes);
  double* psq = (double*)dev.alloc_bytes(p.ws_bytes);
  ColMoments<T> cm;
  cm.mu64 = (double*)dev.alloc_bytes(sizeof(double) * (size_t)n);
  cm.sd64 = (double*)dev.alloc_bytes(sizeof(double) * (size_t)n);
  cm.mu_t = (T*)dev.alloc_bytes(sizeof(T) * (size_t)n);
  cm.sd_t = (T*)dev.alloc_bytes(sizeof(T) * (size_t)n);
  cm.is_const = (int*)dev.alloc_bytes(sizeof(int) * (size_t)n);
  hipLaunchKernelGGL((k::colmom_down_kernel<T>), dim3(p.grid_x, p.grid_y), dim3(p.block), 0, dev.stream, x, m, n, ld, aligned, p.groups,
                     p.rows_per_slab, psum, psq);
  hipLaunchKernelGGL((k::colmom_final_kernel<T>), dim3(p.final_grid_x), dim3(p.final_block), 0, dev.stream, (const double*)psum,
                     (const double*)psq, p.nslab, n, x, (double)m, denom, cm.mu64, cm.mu_t, cm.sd64, cm.sd_t, cm.is_const);
  CORRLA_HIP(hipGetLastError());
  return cm;
}

}  // namespace colstat_stage

template <class TI, class T>
void HipDev::col_ss(const Big<TI>& a, bool along_cols, const T* mu, double* ss) {
  const ColstatPlan p = colss_plan(a.rows, a.cols, k::CvIn<TI>::kVec, along_cols, num_cus);
  if (p.error) throw Error(ST_EINVAL, p.error);
  colstat_stage::col_ss(*this, p, a, mu, ss);
}
template <class T>
void HipDev::col_ss_csr(const CsrView<T>& s, const T* mu, int64_t n_samples, double* ss) {
  colstat_stage::col_ss_csr(*this, csr_colss_plan(s.rows, num_cus), s, mu, n_samples, ss);
}
template <class T>
void HipDev::sd_from_ss(const double* ss, const T* mu, int64_t n, int64_t m_samples, T* sd, T* inv_sd) {
  hipLaunchKernelGGL((k::sd_from_ss_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ss, mu, n, (double)m_samples, sd,
                     inv_sd);
  CORRLA_HIP(hipGetLastError());
}
template <class T>
void HipDev::weighted_colsum(const Skinny<T>& x, int64_t rows, const T* w, T* v) {
  colstat_stage::weighted_colsum(*this, wcolsum_plan(rows, (int)x.cols_alloc), x, rows, w, v);
}

}  // namespace corrla
