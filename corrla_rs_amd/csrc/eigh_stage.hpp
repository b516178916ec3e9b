// The eigensolver stage of the C ABI (corrla_eigh_*): the kernels of eigh_kernels.hpp by the plan of eigh_plan.hpp, the
// Cholesky launchers of chol_stage.hpp for B = L L^T, and for host pointers the copies around them (eigh_staging.hpp).  The
// arguments were checked by eigh_entry (capi_impl.hpp).
// The whole workspace is allocated before the first launch.  SMALL makes one launch and reads the header back.  BLOCKED reads
// the header after the two norm launches (a non-finite entry and the zero matrix end there), enqueues the shift, the Cholesky
// factorisation and the repack, and then the first sweep on its own and groups of kEighGroup sweeps after it; after each group
// it reads that group's sweep records (and, the first time, the Cholesky status).  The first sweep whose largest measure is <= tol rotated nothing and ends the
// iteration: `sweeps` counts the sweeps before it.  More than kEighMaxSweeps of them end the call with CORRLA_ENUMERIC.  The
// stage counts its launches and holds the count against the plan's.
#pragma once
#include <string>

#include "capi_impl.hpp"
#include "chol_stage.hpp"
#include "eigh_kernels.hpp"
#include "eigh_staging.hpp"
#include "hip_backend.hpp"
#include "host_io.hpp"

namespace corrla {
namespace eigh_stage {

// what corrla_ctx_last_eigh reports of the context's last call
struct Ran {
  int route = 0;     // EighRoute
  int sweeps = 0;    // the sweeps that rotated
  double off = 0.0;  // the largest measure of the last sweep
  double shift = 0.0;
  int64_t info = 0;  // 0; 1 a non-finite entry; 2 the Cholesky factorisation reported a pivot; 3 the sweep cap
};

inline void set_lds_limits() {
  lds_limit((const void*)k::eigh_small_kernel, k::kEighSmallLdsBytes);
  lds_limit((const void*)k::eigh_rayleigh_kernel, k::kEighRayLdsBytes);
  lds_limit((const void*)k::eigh_rot_kernel, k::kEighJacLdsBytes);
  lds_limit((const void*)k::eigh_apply_kernel, k::kEighApplyLdsBytes);
}

inline EighPlan plan_of(int64_t n, int num_cus) {
  EighShape s;
  s.n = n, s.num_cus = num_cus;
  const EighPlan p = eigh_plan(s);
  if (!p.ok) throw Error(ST_EINVAL, p.error);
  return p;
}

struct Work {
  EighHeader* hdr = nullptr;
  double *norms = nullptr, *b = nullptr, *w = nullptr, *gram = nullptr, *rot = nullptr, *meas = nullptr, *cols = nullptr, *ray = nullptr;
  EighSweepRecord* rec = nullptr;
  chol_stage::Work chol{};
};
inline Work workspace(HipDev& dev, const EighPlan& p, const CholPlan* cp) {
  Work w;
  w.hdr = (EighHeader*)dev.alloc_bytes(p.ws_header);
  if (p.route == EighRoute::kSmall) return w;
  w.norms = (double*)dev.alloc_bytes(p.ws_norms);
  w.b = (double*)dev.alloc_bytes(p.ws_b);
  w.w = (double*)dev.alloc_bytes(p.ws_w);
  w.gram = (double*)dev.alloc_bytes(p.ws_gram);
  w.rot = (double*)dev.alloc_bytes(p.ws_r);
  w.meas = (double*)dev.alloc_bytes(p.ws_meas);
  w.rec = (EighSweepRecord*)dev.alloc_bytes(p.ws_records);
  w.cols = (double*)dev.alloc_bytes(p.ws_cols);
  w.ray = (double*)dev.alloc_bytes(p.ws_ray);
  w.chol = chol_stage::workspace(dev, *cp);
  return w;
}

inline EighHeader read_header(HipDev& dev, const Work& w) {
  EighHeader h{};
  CORRLA_HIP(hipMemcpyAsync(&h, w.hdr, sizeof(h), hipMemcpyDeviceToHost, dev.stream));
  dev.sync();
  return h;
}

[[noreturn]] inline void fail(Ran* ran, int64_t info, const char* what) {
  ran->info = info;
  throw Error(ST_ENUMERIC, std::string("eigh: ") + what);
}

// one sweep of the tournament; returns the launches made
inline int64_t sweep(HipDev& dev, const EighPlan& p, const Work& w, int64_t n, int64_t index) {
  int64_t launches = 0;
  for (int64_t r = 0; r < p.rounds; ++r) {
    const k::EighRoundArgs a{w.w, n, p.nb, r, p.slabs, p.slab_rows, w.gram, w.rot, w.meas + 2 * r * p.pairs, p.tol, 0.5 * p.tol};
    hipLaunchKernelGGL(k::eigh_gram_kernel, dim3((unsigned)(p.pairs * p.slabs)), dim3(k::kEighThreads), 0, dev.stream, a);
    hipLaunchKernelGGL(k::eigh_rot_kernel, dim3((unsigned)p.pairs), dim3(k::kEighThreads), k::kEighJacLdsBytes, dev.stream, a);
    hipLaunchKernelGGL(k::eigh_apply_kernel, dim3((unsigned)(p.pairs * p.slabs)), dim3(k::kEighThreads), k::kEighApplyLdsBytes, dev.stream, a);
    CORRLA_HIP(hipGetLastError());
    launches += 3;
  }
  const k::EighSweepArgs f{w.meas, p.rounds * p.pairs, w.rec + index};
  hipLaunchKernelGGL(k::eigh_sweep_kernel, dim3(1), dim3(k::kEighThreads), 0, dev.stream, f);
  CORRLA_HIP(hipGetLastError());
  return launches + 1;
}

inline void run_small(HipDev& dev, const EighPlan& p, const Work& w, const Arrays& on, int64_t n, Ran* ran) {
  const k::EighSmallArgs s{on.a, on.lda, (int)n, on.w, on.v, on.ldv, w.hdr, p.tol, 0.5 * p.tol};
  hipLaunchKernelGGL(k::eigh_small_kernel, dim3(1), dim3(k::kEighThreads), k::kEighSmallLdsBytes, dev.stream, s);
  CORRLA_HIP(hipGetLastError());
  const EighHeader h = read_header(dev, w);
  ran->shift = h.sigma;
  ran->sweeps = (int)h.sweeps;
  ran->off = h.off;
  if (h.bad == 1.0) fail(ran, 1, "the lower triangle of a holds a non-finite entry");
  if (h.bad != 0.0) fail(ran, 2, "the Cholesky factorisation of the shifted matrix reported a pivot");
  if (h.capped != 0.0) fail(ran, 3, "the Jacobi iteration did not converge within the sweep cap");
}

inline void run_blocked(HipDev& dev, const EighPlan& p, const CholPlan& cp, const Work& w, const Arrays& on, int64_t n, Ran* ran) {
  const unsigned tiles = (unsigned)p.norm_groups;
  int64_t launches = 0;
  const k::EighNormArgs na{on.a, on.lda, n, w.norms};
  hipLaunchKernelGGL(k::eigh_norm_kernel, dim3(tiles), dim3(k::kEighThreads), 0, dev.stream, na);
  const k::EighSigmaArgs sa{w.norms, p.norm_groups, w.hdr};
  hipLaunchKernelGGL(k::eigh_sigma_kernel, dim3(1), dim3(k::kEighThreads), 0, dev.stream, sa);
  CORRLA_HIP(hipGetLastError());
  launches += 2;
  const EighHeader h = read_header(dev, w);
  ran->shift = h.sigma;
  if (h.bad != 0.0) fail(ran, 1, "the lower triangle of a holds a non-finite entry");
  if (h.sigma == 0.0) {  // the zero matrix
    const k::EighIdentityArgs ia{on.w, on.v, on.ldv, n};
    hipLaunchKernelGGL(k::eigh_identity_kernel, dim3(tiles, tiles), dim3(k::kEighThreads), 0, dev.stream, ia);
    CORRLA_HIP(hipGetLastError());
    return;
  }
  const k::EighShiftArgs sh{on.a, on.lda, n, w.b, w.hdr};
  hipLaunchKernelGGL(k::eigh_shift_kernel, dim3(tiles, tiles), dim3(k::kEighThreads), 0, dev.stream, sh);
  CORRLA_HIP(hipGetLastError());
  launches += 1 + chol_stage::factor(dev, cp, w.chol, w.b, n, n);
  const k::EighRepackArgs rp{w.b, n, w.w};
  hipLaunchKernelGGL(k::eigh_repack_kernel, dim3((unsigned)p.nb, tiles), dim3(k::kEighThreads), 0, dev.stream, rp);
  CORRLA_HIP(hipGetLastError());
  launches += 1;

  int64_t enqueued = 0;
  bool converged = false;
  EighSweepRecord rec[k::kEighGroup];
  while (!converged && enqueued <= k::kEighMaxSweeps) {
    const int64_t first = enqueued;
    const int count = first == 0 ? 1 : k::kEighGroup;  // the first sweep alone: a diagonal or converged matrix ends there
    for (int g = 0; g < count; ++g) launches += sweep(dev, p, w, n, enqueued++);
    CholFactorStatus cst{};
    if (first == 0) CORRLA_HIP(hipMemcpyAsync(&cst, w.chol.st, sizeof(cst), hipMemcpyDeviceToHost, dev.stream));
    CORRLA_HIP(hipMemcpyAsync(rec, w.rec + first, (size_t)count * sizeof(EighSweepRecord), hipMemcpyDeviceToHost, dev.stream));
    dev.sync();
    if (cst.info != 0) fail(ran, 2, "the Cholesky factorisation of the shifted matrix reported a pivot");
    for (int g = 0; g < count && !converged; ++g) {
      ran->off = rec[g].max_measure;
      if (rec[g].max_measure <= p.tol)
        converged = true;
      else
        ++ran->sweeps;
    }
  }
  if (!converged || ran->sweeps > k::kEighMaxSweeps) fail(ran, 3, "the Jacobi iteration did not converge within the sweep cap");

  const k::EighFinishArgs fa{w.w, n, p.nb, on.a, on.lda, w.cols, w.ray, on.w, on.v, on.ldv};
  const dim3 cols_grid((unsigned)eigh_ceil_div(n, k::kEighThreads));
  hipLaunchKernelGGL(k::eigh_colnorm_kernel, dim3((unsigned)p.nb), dim3(k::kEighThreads), 0, dev.stream, fa);
  hipLaunchKernelGGL(k::eigh_unit_kernel, dim3((unsigned)p.nb, tiles), dim3(k::kEighThreads), 0, dev.stream, fa);
  hipLaunchKernelGGL(k::eigh_rayleigh_kernel, dim3((unsigned)p.nb, tiles), dim3(k::kEighThreads), k::kEighRayLdsBytes, dev.stream, fa);
  hipLaunchKernelGGL(k::eigh_lambda_kernel, cols_grid, dim3(k::kEighThreads), 0, dev.stream, fa);
  hipLaunchKernelGGL(k::eigh_rank_kernel, dim3((unsigned)eigh_ceil_div(n, k::kEighThreads)), dim3(k::kEighThreads), 0, dev.stream, fa);
  hipLaunchKernelGGL(k::eigh_scatter_kernel, dim3((unsigned)p.nb, tiles), dim3(k::kEighThreads), 0, dev.stream, fa);
  CORRLA_HIP(hipGetLastError());
  launches += 6;
  if (launches != p.launches(enqueued)) throw Error(ST_EINVAL, "internal: eigh launch count differs from the plan");
}

inline void run(HipDev& dev, bool host_ptrs, const EighCall& c, Ran* ran) {
  const EighPlan p = plan_of(c.n, dev.num_cus);
  CholPlan cp;
  if (p.route == EighRoute::kBlocked) cp = chol_stage::plan_of(c.n, 0);
  dev.begin_call();
  const Work w = workspace(dev, p, &cp);  // every allocation of the call that can be large, before any launch
  HostIo<HipDev> io(dev, host_ptrs);
  const Arrays on = stage(io, c);
  ran->route = (int)p.route;
  if (p.route == EighRoute::kSmall)
    run_small(dev, p, w, on, c.n, ran);
  else
    run_blocked(dev, p, cp, w, on, c.n, ran);
  io.finish();
  if (!host_ptrs) dev.sync();  // the entry leaves a status record: its outputs are complete when it returns
}

}  // namespace eigh_stage
}  // namespace corrla
