// The covariance / correlation stage of the C ABI (corrla_cov_*): staging of x by the route syrk_plan gives, the launcher of
// that plan (syrk) behind the column moments of colstat_stage.hpp, and for host pointers the copies around it (HostIo,
// host_io.hpp).  The arguments were checked by cov_entry (capi_impl.hpp).
// The device path enqueues and returns: begin_call has no end_call there (end_call is the synchronise), the workspace of
// the arena is reused by later calls in stream order, and a throw after begin_call is drained by the entry's locked_call
// like every other entry's.  The one synchronisation that can still happen is hipMalloc inside alloc_bytes, the first time a
// call needs more workspace than the arena holds.  The host path copies the whole strided SPAN of x -- first to last
// element, gaps included -- so a narrow column view of a wide array stages the wide array's rows.
#pragma once
#include "capi_impl.hpp"
#include "colstat_stage.hpp"
#include "hip_backend.hpp"
#include "host_io.hpp"

namespace corrla {
namespace cov_stage {

// C (n x n, ldc) = covariance (or, corr, Pearson correlation) of the columns of x: m x n row-major with leading dimension
// p.ld on the device, read in place.  center: the column moments first (one pass, f64 accumulation), means_out / scales_out
// (device, optional) receive the means and -- corr only -- the standard deviations.  Enqueues only: no synchronisation.
// The plan keeps both grids within the launch limits (nsplit <= 65535).
template <class T>
void syrk(HipDev& dev, const SyrkPlan& p, const T* x, int64_t m, int64_t n, bool center, bool corr, int ddof, T* means_out,
          T* scales_out, T* c, int64_t ldc) {
  const int aligned = p.route == SyrkRoute::kInPlaceChecked ? 0 : 1;
  const double denom = (double)(m - ddof);
  colstat_stage::ColMoments<T> cm{};
  if (center) {
    cm = colstat_stage::col_moments<T>(dev, x, m, n, p.ld, aligned, denom);
    if (means_out) CORRLA_HIP(hipMemcpyAsync(means_out, cm.mu_t, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, dev.stream));
    if (corr && scales_out) CORRLA_HIP(hipMemcpyAsync(scales_out, cm.sd_t, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, dev.stream));
  }
  T* ws = (T*)dev.alloc_bytes(p.ws_bytes);
  k::SyrkArgs<T> a{x, m, n, p.ld, aligned, cm.mu_t, p.slab_rows, p.npairs, ws};
  const dim3 grid(p.grid_x, p.grid_y);
  if (center)
    hipLaunchKernelGGL((k::syrk_kernel<T, true>), grid, dim3(p.block), p.lds_bytes, dev.stream, a);
  else
    hipLaunchKernelGGL((k::syrk_kernel<T, false>), grid, dim3(p.block), p.lds_bytes, dev.stream, a);
  CORRLA_HIP(hipGetLastError());
  k::SyrkFinishArgs<T> f{ws, p.nsplit, p.npairs, n, (double)m, denom, cm.mu64, cm.mu_t, corr ? cm.sd64 : nullptr, cm.is_const, c, ldc};
  hipLaunchKernelGGL((k::syrk_finish_kernel<T>), dim3(p.finish_grid_x, p.finish_grid_y), dim3(p.finish_block), 0, dev.stream, f);
  CORRLA_HIP(hipGetLastError());
}

template <class T>
void run(HipDev& dev, bool host_ptrs, const CovCall<T>& c) {
  const int64_t m = c.m, n = c.n;
  const bool corr = (c.flags & CORRLA_COV_CORRELATION) != 0, center = (c.flags & CORRLA_COV_NO_CENTER) == 0;
  SyrkShape s;
  s.m = m;
  s.n = n;
  s.row_stride = c.rs;
  s.col_stride = c.cs;
  s.esz = (int)sizeof(T);
  s.base_aligned = (uintptr_t)c.x % 16 == 0;
  s.num_cus = dev.num_cus;
  const SyrkPlan p = syrk_plan(s, dev.syrk_knobs());
  if (p.route == SyrkRoute::kReject) throw Error(ST_EINVAL, p.error);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  const T* xd = io.in_as_lies<T>(c.x_span());  // so the route is the one a device pointer of this layout takes
  if (p.route == SyrkRoute::kRepacked) {
    T* packed = (T*)dev.alloc_bytes(p.repack_bytes);
    dev.pack_strided(xd, m, n, c.rs, c.cs, packed, p.ld);
    xd = packed;
  }
  int64_t ldcd;
  T* cd = io.out_packed<T>(c.c_span(), &ldcd);
  T* md = center ? io.out_packed<T>(c.means_span()) : nullptr;
  T* sd = corr ? io.out_packed<T>(c.scales_span()) : nullptr;
  syrk<T>(dev, p, xd, m, n, center, corr, c.ddof, md, sd, cd, ldcd);
  if (c.route_out) *c.route_out = (int)p.route;
  io.finish();
}

}  // namespace cov_stage
}  // namespace corrla
