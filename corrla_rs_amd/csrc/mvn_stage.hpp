// The multivariate normal stage of the C ABI (corrla_mvn_sample_* / corrla_sandwich_diag_*; sample_mv_normal and the diagonal
// of sandwich_prop, stats_corr.rs:46-68): the kernels of mvn_kernels.hpp by the plans of mvn_plan.hpp, and for host pointers
// the copies around them.  The arguments were checked by mvn_sample_entry / sandwich_diag_entry (capi_impl.hpp), which also
// hand over the plan they checked them with.
// The device path enqueues and returns, as kde_stage does: begin_call has no end_call there, seed and first travel in the
// kernel arguments, and nothing is read back.  What can still synchronise: hipMalloc inside alloc_bytes the first time a call
// needs more workspace than the arena holds.  The host path (HostIo, host_io.hpp) builds out where a device array of the same
// offset and row stride would lie, so it takes the same stores; the factor, the mean and cov go in at arena alignment, jac as
// it lies.
#pragma once
#include "capi_impl.hpp"
#include "hip_backend.hpp"
#include "host_io.hpp"
#include "pca_apply_stage.hpp"  // back: the staged route's multiply

namespace corrla {
namespace mvn_stage {

// what corrla_ctx_last_mvn reports of the context's last corrla_mvn_sample_* call
struct Ran {
  int route = 0;  // MvnRoute
};

template <class T>
void set_lds_limits() {
  constexpr size_t kMax = k::kLdsMaxBytes;
  lds_limit((const void*)k::mvn_fused_kernel<T, k::kMvnBmWide, false>, kMax / 2);
  lds_limit((const void*)k::mvn_fused_kernel<T, k::kMvnBmWide, true>, kMax / 2);
  lds_limit((const void*)k::sandwich_kernel<T, k::kMvnBmWide>, kMax / 2);
  lds_limit((const void*)k::sandwich_kernel<T, k::kMvnBmNarrow>, kMax);
}

template <class T>
void run_sample(HipDev& dev, bool host_ptrs, const MvnSampleCall<T>& c, const MvnPlan& p, Ran* ran) {
  ran->route = (int)p.route;
  if (p.route == MvnRoute::kEmpty) return;  // no rows: no launch
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  const T* fd = io.in_aligned<T>(c.factor_span());
  const T* md = io.in_aligned<T>(c.mean_span());
  T* od = io.out_as_lies<T>(c.out_span());  // so the stores are those a device pointer of this layout takes
  // F^T with unit stride along the features (r rows, padded row stride), the zeros of a triangular factor written here
  T* ft = (T*)dev.alloc_bytes(p.factor_bytes);
  const int64_t cells = c.r * p.ldft;
  hipLaunchKernelGGL((k::mvn_pack_factor_kernel<T>), dim3((unsigned)std::min<int64_t>(4096, (cells + 255) / 256)), dim3(256), 0, dev.stream, fd,
                     c.d, c.r, c.ldf, c.lower, ft, p.ldft);
  CORRLA_HIP(hipGetLastError());
  if (p.route == MvnRoute::kFused) {
    const k::MvnArgs<T> a{ft, p.ldft, md, c.n, c.d, (int)c.r, c.seed, c.first, od, c.ldo, p.wide};
    const dim3 grid(p.grid_x), block(p.block);
    if (c.lower)
      hipLaunchKernelGGL((k::mvn_fused_kernel<T, k::kMvnBmWide, true>), grid, block, p.lds_bytes, dev.stream, a);
    else
      hipLaunchKernelGGL((k::mvn_fused_kernel<T, k::kMvnBmWide, false>), grid, block, p.lds_bytes, dev.stream, a);
    CORRLA_HIP(hipGetLastError());
  } else {
    // z of a row chunk, column-major as pca_back_kernel reads its scores, then out = z F^T + mu on that kernel; the chunks
    // share the workspace in stream order
    T* z = (T*)dev.alloc_bytes(p.ws_bytes);
    for (int64_t i0 = 0; i0 < c.n; i0 += p.chunk_rows) {
      const int64_t rows = std::min(p.chunk_rows, c.n - i0);
      dev.fill_normal<T>(z, rows, c.r, (int64_t)1, p.chunk_rows, c.seed, c.first + i0, c.r);
      T* oc = od + i0 * c.ldo;
      PcaApplyShape s;
      s.m = rows, s.n = c.d, s.k = c.r;
      s.row_stride = c.ldo, s.col_stride = 1;
      s.esz = (int)sizeof(T);
      s.base_aligned = (uintptr_t)oc % 16 == 0;
      s.mode = PcaApplyMode::kStore;
      const PcaApplyPlan bp = pca_apply_plan(s);
      if (bp.route == PcaApplyRoute::kReject) throw Error(ST_EINVAL, bp.error);
      pca_apply_stage::back<T>(dev, bp, PcaApplyMode::kStore, (const T*)z, p.chunk_rows, (const T*)ft, p.ldft, md, (const T*)nullptr, rows, c.d,
                               c.r, oc, (T*)nullptr);
    }
  }
  io.finish();
}

template <class T>
void run_sandwich(HipDev& dev, bool host_ptrs, const SandwichDiagCall<T>& c, const SandwichPlan& p) {
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  const T* jd = io.in_as_lies<T>(c.jac_span());
  const T* cd = io.in_aligned<T>(c.cov_span());
  T* vd = io.out_packed<T>(c.v_span());
  const k::SandwichArgs<T> a{jd, c.ldj, cd, c.ldc, c.m, (int)c.d, vd};
  if (p.bm == k::kMvnBmWide)
    hipLaunchKernelGGL((k::sandwich_kernel<T, k::kMvnBmWide>), dim3(p.grid_x), dim3(p.block), p.lds_bytes, dev.stream, a);
  else
    hipLaunchKernelGGL((k::sandwich_kernel<T, k::kMvnBmNarrow>), dim3(p.grid_x), dim3(p.block), p.lds_bytes, dev.stream, a);
  CORRLA_HIP(hipGetLastError());
  io.finish();
}

}  // namespace mvn_stage
}  // namespace corrla
