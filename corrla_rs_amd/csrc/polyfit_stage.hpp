// The polynomial response-surface stage of the C ABI (corrla_polyfit_gram_* / corrla_poly_eval_*; linear_fit, quad_fit,
// quad_eval and jac_from_quad, stats_corr.rs:146-249): the kernels of polyfit_kernels.hpp by the plans of polyfit_plan.hpp,
// and for host pointers the copies around them.  The arguments were checked by polyfit_gram_entry / poly_eval_entry
// (capi_impl.hpp).
// The device path enqueues and returns, as rbf_stage does: begin_call has no end_call there, and a throw after begin_call is
// drained by the entry's locked_call.  What can still synchronise: hipMalloc inside alloc_bytes the first time a call needs
// more workspace than the arena holds, and the upload of the pair table the first time a context sees a (k, r, degree).
// The host path (HostIo, host_io.hpp) copies the strided spans of x, y and the coefficients to the device as they lie (the
// same row strides, the same offset from a 16-byte boundary, so the route is the one a device pointer of this layout takes)
// and the results back; padding columns of the outputs are never written.
#pragma once
#include "capi_impl.hpp"
#include "colstat_stage.hpp"
#include "hip_backend.hpp"
#include "host_io.hpp"

namespace corrla {
namespace polyfit_stage {

// how the last call ran (corrla_ctx_last_polyfit)
struct Ran {
  int route = 0;  // PolyRoute
};

inline void set_lds_limits() {
  constexpr size_t kGram = (size_t)k::poly_gram_lds_bytes(k::kPolyMaxK, k::kPolyMaxRhs);
  constexpr size_t kEval = (size_t)k::poly_eval_lds_bytes(k::kPolyMaxK);
  static_assert(kGram <= k::kLdsMaxBytes && kEval <= k::kLdsMaxBytes, "the images of the largest shape fit in LDS");
  lds_limit((const void*)k::polyfit_gram_kernel<float, true>, kGram);
  lds_limit((const void*)k::polyfit_gram_kernel<float, false>, kGram);
  lds_limit((const void*)k::polyfit_gram_kernel<double, true>, kGram);
  lds_limit((const void*)k::polyfit_gram_kernel<double, false>, kGram);
  lds_limit((const void*)k::poly_eval_kernel<float>, kEval);
  lds_limit((const void*)k::poly_eval_kernel<double>, kEval);
}

template <class T>
void run_gram(HipDev& dev, bool host_ptrs, const PolyGramCall<T>& c, Ran* ran) {
  PolyGramShape s;
  s.m = c.m, s.kf = c.kf, s.r = c.r, s.ldx = c.ldx, s.ldy = c.ldy, s.degree = c.degree, s.esz = (int)sizeof(T);
  s.x_aligned = (uintptr_t)c.x % 16 == 0;
  s.y_aligned = c.r == 0 || (uintptr_t)c.y % 16 == 0;
  s.num_cus = dev.num_cus;
  const PolyGramPlan p = poly_gram_plan(s, dev.poly_knobs());
  if (p.route == PolyRoute::kReject) throw Error(ST_EINVAL, p.error);
  dev.begin_call();
  const int32_t* table = dev.poly_table(c.kf, c.r, c.degree);
  HostIo<HipDev> io(dev, host_ptrs);
  const T* xd = io.in_as_lies<T>(c.x_span());
  const T* yd = io.in_as_lies<T>(c.y_span());  // null when r == 0
  int64_t ldg;
  double* gd = io.out_packed<double>(c.g_span(), &ldg);
  const bool norm = c.normalize != 0;
  const int aligned = p.route == PolyRoute::kInPlace ? 1 : 0;
  const double *mu = nullptr, *sg = nullptr;
  if (norm) {
    // the column pass of cov; the population standard deviation, 1 for a constant column
    const auto cm = colstat_stage::col_moments<T>(dev, xd, c.m, c.kf, c.ldx, aligned, (double)c.m);
    mu = cm.mu64, sg = cm.sd64;
  }
  double* ws = (double*)dev.alloc_bytes(p.ws_bytes);
  k::PolyGramArgs<T> a{xd, c.m, c.ldx, yd, c.ldy, (int)c.kf, (int)c.r, aligned, p.y_vec ? 1 : 0, mu, sg, table, p.slab_rows, p.npairs, p.aug_ld, ws};
  const dim3 grid(p.grid_x, p.grid_y);
  if (norm)
    hipLaunchKernelGGL((k::polyfit_gram_kernel<T, true>), grid, dim3(p.block), p.lds_bytes, dev.stream, a);
  else
    hipLaunchKernelGGL((k::polyfit_gram_kernel<T, false>), grid, dim3(p.block), p.lds_bytes, dev.stream, a);
  CORRLA_HIP(hipGetLastError());
  k::PolyFinishArgs f{ws, p.nsplit, p.npairs, p.order, gd, ldg};
  hipLaunchKernelGGL(k::polyfit_finish_kernel, dim3(p.finish_grid_x, p.finish_grid_y), dim3(p.finish_block), 0, dev.stream, f);
  CORRLA_HIP(hipGetLastError());
  if (ran) ran->route = (int)p.route;
  // the moments of the column pass to the caller's vectors (empty spans without normalize): host pointers take them from
  // where they are, device pointers by a copy on the stream
  const size_t vb = (size_t)c.kf * sizeof(double);
  if (double* md = io.out_from<double>(c.means_span(), mu)) CORRLA_HIP(hipMemcpyAsync(md, mu, vb, hipMemcpyDeviceToDevice, dev.stream));
  if (double* sd = io.out_from<double>(c.scales_span(), sg)) CORRLA_HIP(hipMemcpyAsync(sd, sg, vb, hipMemcpyDeviceToDevice, dev.stream));
  io.finish();
}

template <class T>
void run_eval(HipDev& dev, bool host_ptrs, const PolyEvalCall<T>& c, Ran* ran) {
  const PolyEvalPlan p = poly_eval_plan(c.m, c.kf, c.r, c.degree, c.ldx, (int)sizeof(T), (uintptr_t)c.x % 16 == 0);
  if (!p.ok) throw Error(ST_EINVAL, p.error);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  const T* xd = io.in_as_lies<T>(c.x_span());
  const double* cd = io.in_as_lies<double>(c.coeffs_span());
  int64_t ld_out, ld_jac = c.ld_jac;
  T* od = io.out_packed<T>(c.out_span(), &ld_out);
  T* jd = io.out_packed<T>(c.jac_span(), &ld_jac);
  double* cimg = (double*)dev.alloc_bytes(p.c_bytes);
  hipLaunchKernelGGL(k::poly_c_assemble_kernel, dim3(p.assemble_grid_x), dim3(256), 0, dev.stream, cd, c.ldc, p.p, (int)c.kf, c.degree,
                     (int)c.r, p.k4, p.ncb * p.cb, cimg);
  CORRLA_HIP(hipGetLastError());
  const int aligned = p.route == PolyRoute::kInPlace ? 1 : 0;
  k::PolyEvalArgs<T> a{xd, c.m, c.ldx, (int)c.kf, (int)c.r, aligned, cimg, p.k4, p.xld, p.ncb, od, ld_out, jd, ld_jac};
  hipLaunchKernelGGL((k::poly_eval_kernel<T>), dim3(p.grid_x), dim3(p.block), p.lds_bytes, dev.stream, a);
  CORRLA_HIP(hipGetLastError());
  if (ran) ran->route = (int)p.route;
  io.finish();
}

}  // namespace polyfit_stage
}  // namespace corrla
