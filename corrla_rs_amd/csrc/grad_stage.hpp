// The active-subspace gradient stage on the device (corrla_grad_mat_*): one launcher per kernel family.  grad_plan.hpp
// has decided every grid, workgroup size, LDS and workspace size; a launcher allocates what the plan sized, fills the
// kernel's arguments and launches.  Events 0 - 1 enclose the scan (corrla_timings.knn_ms), 1 - 2 the fit (fit_ms).
#pragma once
#include <vector>

#include "capi_impl.hpp"
#include "grad_plan.hpp"
#include "hip_backend.hpp"
#include "host_io.hpp"

namespace corrla {

struct GradCall {               // one call, every array on the device
  const double *x, *y, *xq;     // n_pts x k support points, their n_pts values, n_q x k queries (row-major)
  double* g;                    // out: n_q x k gradients, rows ldg apart
  int64_t ldg, n_pts, k, n_q, n_nbrs;
  int order;
  double out_scale;
  int* nbr;                     // n_q x n_nbrs neighbour lists: written by the scan, read by the fit
  int* status;                  // n_q: non-zero where the fit needed the ridge or failed
  bool prof;                    // CORRLA_KNN2_PROF: the bf16 scan and the order-1 fit count ticks and print them (synchronises)
};

namespace grad_stage {

template <class T>
inline T* ws(HipDev& dev, size_t bytes) { return (T*)dev.alloc_bytes(bytes); }

inline unsigned long long* prof_counters(HipDev& dev, const GradCall& c) {
  if (!c.prof) return nullptr;
  unsigned long long* p = ws<unsigned long long>(dev, 4 * sizeof(unsigned long long));
  CORRLA_HIP(hipMemsetAsync(p, 0, 4 * sizeof(unsigned long long), dev.stream));
  return p;
}
inline void prof_read(HipDev& dev, const unsigned long long* p, unsigned long long (&h)[4]) {
  CORRLA_HIP(hipMemcpyAsync(h, p, sizeof(h), hipMemcpyDeviceToHost, dev.stream));
  CORRLA_HIP(hipStreamSynchronize(dev.stream));
}

// Start of a limited scan: the cloud transposed (k x ldt), then event 0.  The VALU and MFMA scans read x^T.
inline const double* transposed(HipDev& dev, const GradCall& c, const GradPlan& p) {
  double* xt = ws<double>(dev, sizeof(double) * (size_t)p.ldt * c.k);
  hipLaunchKernelGGL(k::grad_transpose_kernel, dim3((unsigned)p.pts_wgs), dim3(256), 0, dev.stream, c.x, c.n_pts, (int)c.k, xt, p.ldt);
  dev.event_mark(0);
  return xt;
}

// ---- nearest-neighbour scans: c.nbr ----
inline void scan_wide(HipDev& dev, const GradCall& c, const GradPlan& p) {  // grad_wide_kernels.hpp: any k, any n_nbrs
  const size_t lists = (size_t)p.scan_wgs * k::kWsQ;
  const k::WideScanArgs a{c.x, c.xq, c.n_pts, c.n_q, c.n_nbrs, p.scan_tiles, (int)c.k,
                          ws<double>(dev, lists * (size_t)c.n_nbrs * sizeof(double)), ws<double>(dev, lists * k::kWsCap * sizeof(double)),
                          ws<int>(dev, lists * k::kWsCap * sizeof(int)), c.nbr};
  dev.event_mark(0);
  hipLaunchKernelGGL(k::knn_wide_kernel, dim3((unsigned)p.scan_wgs), dim3(p.scan_block), p.scan_lds, dev.stream, a);
  CORRLA_HIP(hipGetLastError());
}

// knn2_kernels.hpp: bf16x3 MFMA filter + batched bitonic list merges over the centred cloud; n_nbrs <= 128
inline void scan_knn2(HipDev& dev, const GradCall& c, const GradPlan& p) {
  transposed(dev, c, p);  // not read by this scan
  const GradPlan::Knn2& g = p.k2;
  const int kk = (int)c.k;
  __bf16* pb = ws<__bf16>(dev, g.pb);
  float* pn = ws<float>(dev, g.pn);
  double* mean = ws<double>(dev, 64 * sizeof(double) + p.scale_ws);  // the centre, then the filter's scale (Knn2Args::mean)
  double* partial = ws<double>(dev, (size_t)g.nb * 64 * sizeof(double));
  CORRLA_HIP(hipMemsetAsync(mean + 64, 0, p.scale_ws, dev.stream));
  hipLaunchKernelGGL(k::knn2_colsum_kernel, dim3((unsigned)g.nb), dim3(256), 0, dev.stream, c.x, c.n_pts, kk, g.rpb, partial,
                     (unsigned long long*)(mean + 66));
  hipLaunchKernelGGL(k::knn2_mean_kernel, dim3(1), dim3(64), 0, dev.stream, (const double*)partial, g.nb, c.n_pts, kk, mean);
  hipLaunchKernelGGL(k::knn2_prep_kernel, dim3((unsigned)g.nchunks), dim3(256), 0, dev.stream, c.x, c.n_pts, kk, (const double*)mean,
                     p.scan_s, pb, pn);
  const k::Knn2Args a{pb, pn, c.x, c.xq, mean, c.n_pts, c.n_q, g.nchunks, p.scan_tiles, kk, (int)c.n_nbrs,
                      ws<int>(dev, g.cand), ws<double>(dev, g.list_d), ws<int>(dev, g.list_i), c.nbr, prof_counters(dev, c)};
  with_nt<2>(p.scan_s, [&](auto s) {
    hipLaunchKernelGGL((k::knn2_kernel<decltype(s)::value>), dim3((unsigned)p.scan_wgs), dim3(p.scan_block), p.scan_lds, dev.stream, a);
  });
  CORRLA_HIP(hipGetLastError());
  if (a.prof) {  // diagnostic only
    unsigned long long h[4];
    prof_read(dev, a.prof, h);
    std::fprintf(stderr, "knn2 prof (wave 0 of %lld workgroups, 100 MHz ticks): total %llu, flushes %llu (%.1f %%), chunk waits %llu (%.1f %%), "
                 "%llu merge batches\n", (long long)p.scan_wgs, h[2], h[0], 100.0 * h[0] / (double)h[2], h[1], 100.0 * h[1] / (double)h[2], h[3]);
  }
}

inline void scan_valu(HipDev& dev, const GradCall& c, const GradPlan& p) {  // grad_kernels.hpp: lists in LDS, VALU distances
  const double* xt = transposed(dev, c, p);
  hipLaunchKernelGGL(k::knn_kernel, dim3((unsigned)p.scan_wgs), dim3(p.scan_block), p.scan_lds, dev.stream, xt, p.ldt, c.n_pts, (int)c.k,
                     c.xq, c.n_q, (int)c.n_nbrs, c.nbr);
  CORRLA_HIP(hipGetLastError());
}

inline void scan_mfma(HipDev& dev, const GradCall& c, const GradPlan& p) {  // grad_kernels.hpp: f32-MFMA distance tiles
  const double* xt = transposed(dev, c, p);
  double* pnorm = ws<double>(dev, sizeof(double) * (size_t)c.n_pts + p.scale_ws);  // + the largest of them (the filter's scale)
  CORRLA_HIP(hipMemsetAsync(pnorm + c.n_pts, 0, p.scale_ws, dev.stream));
  hipLaunchKernelGGL(k::point_norms_kernel, dim3((unsigned)p.pts_wgs), dim3(256), 0, dev.stream, xt, p.ldt, c.n_pts, (int)c.k, pnorm);
  with_one_of<4, 2>(p.scan_w, [&](auto w) {
    with_one_of<4, 8, 16>(p.scan_nks, [&](auto s) {
      hipLaunchKernelGGL((k::knn_mfma_kernel<decltype(w)::value, decltype(s)::value>), dim3((unsigned)p.scan_wgs), dim3(p.scan_block),
                         p.scan_lds, dev.stream, xt, p.ldt, (const double*)pnorm, c.n_pts, (int)c.k, c.xq, c.n_q, (int)c.n_nbrs, c.nbr);
    });
  });
  CORRLA_HIP(hipGetLastError());
}

// ---- local fits: c.g, c.status ----
inline void fit_wide(HipDev& dev, const GradCall& c, const GradPlan& p) {  // grad_wide_kernels.hpp: normal equations in global memory
  const k::WideFitArgs a{c.x, c.y, c.xq, c.nbr, c.n_q, c.n_nbrs, k::grad_design_cols(c.k, c.order), (int)c.k, c.order, c.out_scale,
                         c.g, c.ldg, c.status, ws<double>(dev, p.fit_ws)};
  hipLaunchKernelGGL(k::grad_fit_wide_kernel, dim3((unsigned)p.fit_wgs), dim3(256), p.fit_lds, dev.stream, a);
  CORRLA_HIP(hipGetLastError());
}

inline void fit_lin(HipDev& dev, const GradCall& c, const GradPlan& p) {  // order 1: the MFMA-built normal equations
  const k::FitRowTab rtab = k::grad_fit_lin_row_table((int)c.k + 1);
  unsigned long long* prof = prof_counters(dev, c);
  with_nt<5>(p.fit_ntt, [&](auto ntt) {
    hipLaunchKernelGGL((k::grad_fit_lin_kernel<decltype(ntt)::value>), dim3((unsigned)p.fit_wgs), dim3(64), p.fit_lds, dev.stream, c.x, c.y,
                       (int)c.k, c.xq, c.n_q, (const int*)c.nbr, (int)c.n_nbrs, c.out_scale, c.g, c.ldg, c.status, prof, rtab);
  });
  CORRLA_HIP(hipGetLastError());
  if (prof) {  // diagnostic only
    unsigned long long h[4];
    prof_read(dev, prof, h);
    const double tot = (double)(h[0] + h[1] + h[2]);
    std::fprintf(stderr, "fit prof (%llu queries, 100 MHz ticks per query): gather + normal equations %.0f (%.0f %%), Cholesky %.0f (%.0f %%), "
                 "solves %.0f (%.0f %%)\n", h[3], h[0] / (double)h[3], 100.0 * h[0] / tot, h[1] / (double)h[3], 100.0 * h[1] / tot,
                 h[2] / (double)h[3], 100.0 * h[2] / tot);
  }
}

// grad_fit_kernel, either order.  kLds: one workgroup per query, the normal equations in LDS; kGlobal: persistent
// workgroups, each with its slice of global memory for them
inline void fit_general(HipDev& dev, const GradCall& c, const GradPlan& p) {
  const bool glob = p.fit == GradFit::kGlobal;
  hipLaunchKernelGGL(k::grad_fit_kernel, dim3((unsigned)p.fit_wgs), dim3(64), p.fit_lds, dev.stream, c.x, c.y, (int)c.k, c.xq, c.n_q,
                     (const int*)c.nbr, (int)c.n_nbrs, c.order, c.out_scale, c.g, c.ldg, c.status,
                     glob ? ws<double>(dev, p.fit_ws) : (double*)nullptr, glob ? (int64_t)k::grad_fit_m_elems((int)c.k, c.order) : (int64_t)0);
  CORRLA_HIP(hipGetLastError());
}

// scan, event 1, fit
inline void run(HipDev& dev, const GradCall& c, const GradPlan& p) {
  switch (p.scan) {
    case GradScan::kWide: scan_wide(dev, c, p); break;
    case GradScan::kKnn2: scan_knn2(dev, c, p); break;
    case GradScan::kValu: scan_valu(dev, c, p); break;
    case GradScan::kMfma: scan_mfma(dev, c, p); break;
  }
  dev.event_mark(1);
  switch (p.fit) {
    case GradFit::kWide: fit_wide(dev, c, p); break;
    case GradFit::kLin: fit_lin(dev, c, p); break;
    case GradFit::kLds:
    case GradFit::kGlobal: fit_general(dev, c, p); break;
  }
}

// One corrla_grad_mat_* call, its arguments checked by grad_entry (capi_impl.hpp): the plan, the copies around the stage
// (HostIo: every host array at arena alignment, g packed), run, and what the call reports -- its device times in *last and
// the number of queries that needed the ridge or failed, a short reduction on the host (n_q ints).  That count is a host
// value, so a device-pointer call synchronises too.
inline void run_entry(HipDev& dev, bool host_ptrs, const GradMatCall& c, Timings* last) {
  // which scan and which fit, every grid and workspace (grad_plan.hpp)
  const GradPlan plan = grad_plan(c.n_pts, c.k, c.n_q, c.est_order, c.n_nbrs, env_int("CORRLA_KNN", 0), env_int("CORRLA_FIT", 0),
                                  dev.num_cus, kGradWideBudgetBytes, env_int("CORRLA_KNN2_WGS_PER_CU", 1));
  if (plan.error) throw Error(ST_EINVAL, plan.error);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  const double *x = io.in_aligned<double>(c.x_span()), *y = io.in_aligned<double>(c.y_span()), *xq = io.in_aligned<double>(c.xq_span());
  int64_t ldg;
  double* g = io.out_packed<double>(c.g_span(), &ldg);
  const GradCall call{x, y, xq, g, ldg, c.n_pts, c.k, c.n_q, c.n_nbrs, c.est_order, c.out_scale,
                      ws<int>(dev, sizeof(int) * (size_t)(c.n_q * c.n_nbrs)), ws<int>(dev, sizeof(int) * (size_t)c.n_q),
                      env_int("CORRLA_KNN2_PROF", 0) != 0};
  run(dev, call, plan);
  std::vector<int> hs((size_t)c.n_q);
  CORRLA_HIP(hipMemcpyAsync(hs.data(), call.status, sizeof(int) * (size_t)c.n_q, hipMemcpyDeviceToHost, dev.stream));
  io.enqueue_back();  // g, behind the status; event 2 behind both, then the one synchronise of either kind of call
  dev.event_mark(2);
  dev.end_call();
  *last = Timings();
  last->knn_ms = dev.event_elapsed_ms(0, 1);
  last->fit_ms = dev.event_elapsed_ms(1, 2);
  last->total_ms = last->knn_ms + last->fit_ms;
  int bad = 0;
  for (int v : hs) bad += v != 0;
  if (c.n_regularised) *c.n_regularised = bad;
}

}  // namespace grad_stage
}  // namespace corrla
