// The kernel-density stage of the C ABI (corrla_kde_eval_* / corrla_kde_nll_*; KdeRv::pdf / cdf and UniRv::nll,
// univariate_rv.rs:165-170, 423-444): the kernels of kde_kernels.hpp by the plan of kde_plan.hpp, and for host pointers the
// copies around them.  The arguments were checked by kde_eval_entry / kde_nll_entry (capi_impl.hpp).
// The device path enqueues and returns, as rbf_stage does: begin_call has no end_call there, every constant -- the
// bandwidths among them, which always arrive through a host pointer -- travels in the kernel arguments, never through a
// synchronising copy, and a throw after begin_call is drained by the entry's locked_call.  What can still synchronise:
// hipMalloc inside alloc_bytes the first time a call needs more workspace than the arena holds.  The host path (HostIo,
// host_io.hpp) copies the strided spans of x and s to the device as they lie (the same strides, the same offset from a
// 16-byte boundary) and the n_q elements of the result back; the elements between them are never written.
#pragma once
#include <cmath>

#include "capi_impl.hpp"
#include "hip_backend.hpp"
#include "host_io.hpp"

namespace corrla {
namespace kde_stage {

// what corrla_ctx_last_kde reports of the context's last call
struct Ran {
  int route = 0;  // KdeRoute
};

inline KdePlan plan_of(int64_t n_q, int64_t n_s, int64_t n_h, int esz, KdeMode mode) {
  KdeShape s;
  s.n_q = n_q, s.n_s = n_s, s.n_h = n_h, s.esz = esz, s.mode = mode;
  const KdePlan p = kde_plan(s);
  if (!p.ok) throw Error(ST_EINVAL, p.error);
  return p;
}

struct Workspace {
  void* ws_min;
  void* ws_sum;
  double* ws_red;
};
inline Workspace workspace(HipDev& dev, const KdePlan& p) {
  Workspace w;
  w.ws_min = dev.alloc_bytes(p.ws_min_bytes);
  w.ws_sum = dev.alloc_bytes(p.ws_sum_bytes);
  w.ws_red = (double*)dev.alloc_bytes(p.ws_red_bytes);
  return w;
}

template <class T>
void launch_nearest(HipDev& dev, const KdePlan& p, const Workspace& w, const T* x, int64_t n_q, int64_t incx, const T* s, int64_t n_s,
                    int64_t incs) {
  if (!p.nearest) return;
  k::KdeNearArgs<T> a{x, incx, s, incs, n_q, n_s, p.nqt, p.split_len, (T*)w.ws_min};
  hipLaunchKernelGGL((k::kde_nearest_kernel<T>), dim3(p.near_grid_x), dim3(p.block), 0, dev.stream, a);
  CORRLA_HIP(hipGetLastError());
}

constexpr double kLog2e = 1.4426950408889634074, kLn2 = 0.69314718055994530942, kSqrt2 = 1.4142135623730950488;

// the exponent scale of a bandwidth as the sum kernel takes it (kde_kernels.hpp)
template <class T>
T exponent_scale(double h, bool cdf) {
  if (cdf) return (T)(1.0 / (h * kSqrt2));
  return (T)((sizeof(T) == 4 ? kLog2e : 1.0) / (2.0 * h * h));
}

template <class T>
void run_eval(HipDev& dev, bool host_ptrs, const KdeEvalCall<T>& c, Ran* ran) {
  const KdeMode mode = c.what == 0 ? KdeMode::kPdf : (c.what == 1 ? KdeMode::kCdf : KdeMode::kLogpdf);
  const KdePlan p = plan_of(c.n_q, c.n_s, 1, (int)sizeof(T), mode);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  const T* x = io.in_as_lies<T>(c.x_span());
  const T* s = io.in_as_lies<T>(c.s_span());
  T* out = io.out_as_lies<T>(c.out_span());
  const Workspace w = workspace(dev, p);
  launch_nearest<T>(dev, p, w, x, c.n_q, c.incx, s, c.n_s, c.incs);
  k::KdeSumArgs<T> a{x, c.incx, s, c.incs, c.n_q, c.n_s, p.nqt, p.split_len, p.nsplit, 1, 1, (const T*)w.ws_min, (T*)w.ws_sum, {}};
  a.c[0] = exponent_scale<T>(c.h, mode == KdeMode::kCdf);
  if (mode == KdeMode::kCdf)
    hipLaunchKernelGGL((k::kde_sum_kernel<T, k::kKdeCdf>), dim3(p.sum_grid_full), dim3(p.block), 0, dev.stream, a);
  else
    hipLaunchKernelGGL((k::kde_sum_kernel<T, k::kKdeSum>), dim3(p.sum_grid_full), dim3(p.block), 0, dev.stream, a);
  CORRLA_HIP(hipGetLastError());
  k::KdeFinishArgs<T> f{(const T*)w.ws_min, (const T*)w.ws_sum, p.nsplit, c.n_q, c.n_s, c.what, c.h, out, c.inco};
  hipLaunchKernelGGL((k::kde_finish_kernel<T>), dim3(p.finish_grid_x), dim3(p.finish_block), 0, dev.stream, f);
  CORRLA_HIP(hipGetLastError());
  ran->route = (int)p.route;
  io.finish();
}

template <class T>
void run_nll(HipDev& dev, bool host_ptrs, const KdeNllCall<T>& c, Ran* ran) {
  const KdePlan p = plan_of(c.n_t, c.n_s, c.n_h, (int)sizeof(T), KdeMode::kNll);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  const T* x = io.in_as_lies<T>(c.x_span());
  const T* s = io.in_as_lies<T>(c.s_span());
  double* nll = io.out_packed<double>(c.nll_span());
  double* dnll = io.out_packed<double>(c.dnll_span());
  const Workspace w = workspace(dev, p);
  launch_nearest<T>(dev, p, w, x, c.n_t, c.incx, s, c.n_s, c.incs);
  for (int64_t l = 0; l < p.nlaunch; ++l) {  // the launches share the workspace of the sums, in stream order
    const int b_first = (int)(l * p.hl), nb = l + 1 < p.nlaunch ? p.nb_full : p.nb_last;
    const int ngroups = (nb + p.hg - 1) / p.hg;
    k::KdeSumArgs<T> a{x, c.incx, s, c.incs, c.n_t, c.n_s, p.nqt, p.split_len, p.nsplit, ngroups, nb, (const T*)w.ws_min, (T*)w.ws_sum, {}};
    k::KdeNllArgs<T> f{(const T*)w.ws_min, (const T*)w.ws_sum, p.nsplit, c.n_t, c.n_s, p.red_len, nb, b_first, p.red_blocks,
                       sizeof(T) == 4 ? -kLn2 : -1.0, {}, w.ws_red};
    for (int b = 0; b < nb; ++b) {
      a.c[b] = exponent_scale<T>(c.h[b_first + b], false);
      f.h[b] = c.h[b_first + b];
    }
    hipLaunchKernelGGL((k::kde_sum_kernel<T, k::kKdeNll>), dim3(l + 1 < p.nlaunch ? p.sum_grid_full : p.sum_grid_last), dim3(p.block), 0,
                       dev.stream, a);
    CORRLA_HIP(hipGetLastError());
    hipLaunchKernelGGL((k::kde_nll_points_kernel<T>), dim3(p.red_blocks, (unsigned)nb), dim3(256), 0, dev.stream, f);
    CORRLA_HIP(hipGetLastError());
  }
  k::KdeReduceArgs r{w.ws_red, p.red_blocks, nll, dnll};
  hipLaunchKernelGGL(k::kde_nll_reduce_kernel, dim3((unsigned)c.n_h), dim3(256), 0, dev.stream, r);
  CORRLA_HIP(hipGetLastError());
  ran->route = (int)p.route;
  io.finish();
}

}  // namespace kde_stage
}  // namespace corrla
