// The covariance / correlation stage of the C ABI (corrla_cov_*): staging of x by the route syrk_plan gives, the launcher of
// that plan (syrk) behind the column moments of colstat_stage.hpp, and for host pointers the copies around it.  The arguments were checked by cov_entry (capi_impl.hpp).
// The device path enqueues and returns: begin_call has no end_call there (end_call is the synchronise), the workspace of
// the arena is reused by later calls in stream order, and a throw after begin_call is drained by the entry's locked_call
// like every other entry's.  The one synchronisation that can still happen is hipMalloc inside alloc_bytes, the first time a
// call needs more workspace than the arena holds.  The host path copies the whole strided SPAN of x -- first to last
// element, gaps included -- so a narrow column view of a wide array stages the wide array's rows.
#pragma once
#include "capi_impl.hpp"
#include "colstat_stage.hpp"
#include "hip_backend.hpp"

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
void run(HipDev& dev, bool host_ptrs, const T* x, int64_t m, int64_t n, int64_t rs, int64_t cs, uint64_t flags, int ddof,
         T* means_out, T* scales_out, T* c, int64_t ldc, int* route_out) {
  const bool corr = (flags & CORRLA_COV_CORRELATION) != 0, center = (flags & CORRLA_COV_NO_CENTER) == 0;
  SyrkShape s;
  s.m = m;
  s.n = n;
  s.row_stride = rs;
  s.col_stride = cs;
  s.esz = (int)sizeof(T);
  s.base_aligned = (uintptr_t)x % 16 == 0;
  s.num_cus = dev.num_cus;
  const SyrkPlan p = syrk_plan(s, dev.syrk_knobs());
  if (p.route == SyrkRoute::kReject) throw Error(ST_EINVAL, p.error);
  dev.begin_call();
  const T* xd = x;
  if (host_ptrs) {
    // x to the device as it lies: the same strides and the same offset from a 16-byte boundary, so the route is the one a
    // device pointer of this layout takes
    const size_t span = (size_t)((m - 1) * rs + (n - 1) * cs + 1);
    char* buf = (char*)dev.alloc_bytes(span * sizeof(T) + 16);
    T* xs = (T*)(buf + (uintptr_t)x % 16);
    dev.h2d_bytes(xs, x, span * sizeof(T));
    xd = xs;
  }
  if (p.route == SyrkRoute::kRepacked) {
    T* packed = (T*)dev.alloc_bytes(p.repack_bytes);
    dev.pack_strided(xd, m, n, rs, cs, packed, p.ld);
    xd = packed;
  }
  T* cd = c;
  int64_t ldcd = ldc;
  T *md = means_out, *sd = scales_out;
  if (host_ptrs) {
    cd = (T*)dev.alloc_bytes((size_t)n * (size_t)n * sizeof(T));
    ldcd = n;
    if (means_out && center) md = (T*)dev.alloc_bytes((size_t)n * sizeof(T));
    if (scales_out && corr) sd = (T*)dev.alloc_bytes((size_t)n * sizeof(T));
  }
  syrk<T>(dev, p, xd, m, n, center, corr, ddof, center ? md : nullptr, corr ? sd : nullptr, cd, ldcd);
  if (route_out) *route_out = (int)p.route;
  if (!host_ptrs) return;  // enqueued on the context's stream; the workspace is reused by later calls in stream order
  CORRLA_HIP(hipMemcpy2DAsync(c, (size_t)ldc * sizeof(T), cd, (size_t)n * sizeof(T), (size_t)n * sizeof(T), (size_t)n,
                              hipMemcpyDeviceToHost, dev.stream));
  if (means_out && center) CORRLA_HIP(hipMemcpyAsync(means_out, md, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, dev.stream));
  if (scales_out && corr) CORRLA_HIP(hipMemcpyAsync(scales_out, sd, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, dev.stream));
  dev.end_call();
}

}  // namespace cov_stage
}  // namespace corrla
