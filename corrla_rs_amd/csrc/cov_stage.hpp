// The covariance / correlation stage of the C ABI (corrla_cov_*): staging of x by the route syrk_plan gives, HipDev::syrk,
// and for host pointers the copies around it.  The arguments were checked by cov_entry (capi_impl.hpp).
// The device path enqueues and returns: begin_call has no end_call there (end_call is the synchronise), the workspace of
// the arena is reused by later calls in stream order, and a throw after begin_call is drained by the entry's locked_call
// like every other entry's.  The one synchronisation that can still happen is hipMalloc inside alloc_bytes, the first time a
// call needs more workspace than the arena holds.  The host path copies the whole strided SPAN of x -- first to last
// element, gaps included -- so a narrow column view of a wide array stages the wide array's rows.
#pragma once
#include "capi_impl.hpp"
#include "hip_backend.hpp"

namespace corrla {
namespace cov_stage {

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
  dev.template syrk<T>(p, xd, m, n, center, corr, ddof, center ? md : nullptr, corr ? sd : nullptr, cd, ldcd);
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
