// The radial-basis-function stage of the C ABI (corrla_rbf_matrix_* / corrla_rbf_apply_*; RbfInterp::fit's kernel block
// and RbfInterp::predict, interp_utils.rs:96-129 and :146-153): the kernels of rbf_kernels.hpp by the plan of rbf_plan.hpp,
// and for host pointers the copies around them.  The arguments were checked by rbf_entry (capi_impl.hpp).
// The device path enqueues and returns, as pca_apply_stage does: begin_call has no end_call there, every constant travels
// in the kernel arguments, never through a synchronising copy, and a throw after begin_call is drained by the entry's
// locked_call.  What can still synchronise: hipMalloc inside alloc_bytes the first time a call needs more workspace than the
// arena holds.  The host path (HostIo, host_io.hpp) copies the strided spans of xq, xs and the coefficients to the device as
// they lie (the same row strides, the same offset from a 16-byte boundary) and the n_q x n_rhs (or n_q x n_s) block of the
// result back; the padding columns of out are never written.
#pragma once
#include "capi_impl.hpp"
#include "hip_backend.hpp"
#include "host_io.hpp"

namespace corrla {
namespace rbf_stage {

template <class T>
void set_lds_limits() {
  constexpr size_t kApply = (size_t)k::rbf_apply_lds_bytes(k::kRbfMaxDim, (int)sizeof(T));
  constexpr size_t kMatrix = (size_t)k::rbf_matrix_lds_bytes(k::kRbfMaxDim, (int)sizeof(T));
  static_assert(kApply <= k::kLdsMaxBytes && kMatrix <= k::kLdsMaxBytes, "the images of the largest dim fit in LDS");
  for_each_nt<4>([](auto kn) {
    constexpr int K = decltype(kn)::value;
    lds_limit((const void*)k::rbf_apply_kernel<T, K>, kApply);
    lds_limit((const void*)k::rbf_matrix_kernel<T, K>, kMatrix);
  });
}

inline RbfPlan plan_of(int64_t n_q, int64_t n_s, int64_t dim, int64_t n_rhs, int64_t n_poly, int esz, RbfMode mode) {
  RbfShape s;
  s.n_q = n_q, s.n_s = n_s, s.dim = dim, s.n_rhs = n_rhs, s.n_poly = n_poly, s.esz = esz, s.mode = mode;
  const RbfPlan p = rbf_plan(s);
  if (!p.ok) throw Error(ST_EINVAL, p.error);
  return p;
}

// the call with every array on the device, all of them as they lie
template <class T>
RbfCall<T> on_device(HostIo<HipDev>& io, const RbfCall<T>& call, bool apply) {
  RbfCall<T> c = call;
  c.xq = io.in_as_lies<T>(call.xq_span());
  c.xs = io.in_as_lies<T>(call.xs_span());
  c.coeffs = io.in_as_lies<T>(call.coeffs_span(apply));
  c.out = io.out_as_lies<T>(call.out_span(apply));
  return c;
}

template <class T>
void run_matrix(HipDev& dev, bool host_ptrs, const RbfCall<T>& call) {
  const RbfPlan p = plan_of(call.n_q, call.n_s, call.dim, 1, 0, (int)sizeof(T), RbfMode::kMatrix);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  const RbfCall<T> c = on_device<T>(io, call, false);
  k::RbfMatrixArgs<T> a{c.xq, c.ldq, c.xs, c.ldxs, c.n_q, c.n_s, (int)c.dim, (T)c.eps, p.nrg, c.out, c.ld_out};
  with_nt<4>(c.kernel, [&](auto kn) {  // the kernel id is a template argument: one switch per launch, outside every loop
    hipLaunchKernelGGL((k::rbf_matrix_kernel<T, decltype(kn)::value>), dim3(p.grid_x), dim3(p.block), p.lds_bytes, dev.stream, a);
  });
  CORRLA_HIP(hipGetLastError());
  io.finish();
}

template <class T>
void run_apply(HipDev& dev, bool host_ptrs, const RbfCall<T>& call) {
  const int64_t n_poly = call.n_poly();
  const RbfPlan p = plan_of(call.n_q, call.n_s, call.dim, call.n_rhs, n_poly, (int)sizeof(T), RbfMode::kApply);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  const RbfCall<T> c = on_device<T>(io, call, true);
  T* ws = (T*)dev.alloc_bytes(p.ws_bytes);
  k::RbfApplyArgs<T> a{c.xq, c.ldq, c.xs, c.ldxs, c.coeffs, c.ldw, c.n_q, c.n_s, c.n_rhs, (int)c.dim, (T)c.eps, p.nbm, p.nrg, p.split_len, ws};
  with_nt<4>(c.kernel, [&](auto kn) {  // the kernel id is a template argument: one switch per launch, outside every loop
    hipLaunchKernelGGL((k::rbf_apply_kernel<T, decltype(kn)::value>), dim3(p.grid_x), dim3(p.block), p.lds_bytes, dev.stream, a);
  });
  CORRLA_HIP(hipGetLastError());
  const int tail = n_poly == 0 ? 0 : (c.poly_degree >= 2 ? 2 : 1);
  k::RbfFinishArgs<T> f{ws, p.nsplit, c.n_q, c.n_rhs, c.xq, c.ldq, (int)c.dim, tail, tail ? c.coeffs + c.n_s * c.ldw : nullptr, c.ldw, c.out, c.ld_out};
  hipLaunchKernelGGL((k::rbf_finish_kernel<T>), dim3(p.finish_grid_x), dim3(p.finish_block), 0, dev.stream, f);
  CORRLA_HIP(hipGetLastError());
  io.finish();
}

}  // namespace rbf_stage
}  // namespace corrla
