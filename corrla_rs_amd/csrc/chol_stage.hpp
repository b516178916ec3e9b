// The Cholesky stage of the C ABI (corrla_chol_factor_*, corrla_chol_solve_*): the kernels of chol_kernels.hpp by the plan of
// chol_plan.hpp, and for host pointers the copies around them (chol_staging.hpp).  The arguments were checked by
// chol_factor_entry / chol_solve_entry (capi_impl.hpp).
// A call enqueues every launch of the factorisation and of the substitutions without waiting for the device, then makes the
// one read-back of the call: the 32-byte status record (info, smallest and largest l_jj, log det A).  So the device entries
// synchronise once.  info != 0 ends the call with CORRLA_ENUMERIC after the record is kept for corrla_ctx_last_chol; no kernel
// looks at the record, the arrays hold a partial factor whose columns before the failed one are final.  The host path copies
// the strided spans to the device as they lie and the elements of the result back; the padding columns are never written, and
// after a failed column nothing is.
#pragma once
#include <string>

#include "capi_impl.hpp"
#include "chol_kernels.hpp"
#include "chol_staging.hpp"
#include "hip_backend.hpp"
#include "host_io.hpp"

namespace corrla {
namespace chol_stage {

// what corrla_ctx_last_chol reports of the context's last call
struct Ran {
  int route = 0;  // CholRoute
  int64_t info = 0;
  double min_diag = 0.0, max_diag = 0.0, logdet = 0.0;
};

inline void set_lds_limits() {
  lds_limit((const void*)k::chol_small_kernel, k::kCholSmallLdsBytes);
  lds_limit((const void*)k::chol_panel_kernel, k::kCholPanelLdsBytes);
  lds_limit((const void*)k::chol_update_kernel, k::kCholUpdateLdsBytes);
  lds_limit((const void*)k::chol_gemm_kernel<false>, k::kCholGemmLdsBytes);
  lds_limit((const void*)k::chol_gemm_kernel<true>, k::kCholGemmLdsBytes);
}

inline CholPlan plan_of(int64_t n, int64_t n_rhs) {
  CholShape s;
  s.n = n, s.n_rhs = n_rhs;
  const CholPlan p = chol_plan(s);
  if (!p.ok) throw Error(ST_EINVAL, p.error);
  return p;
}

struct Work {
  CholFactorStatus* st;
  CholPanelRecord* rec;
};
inline Work workspace(HipDev& dev, const CholPlan& p) {
  Work w;
  w.st = (CholFactorStatus*)dev.alloc_bytes(p.ws_status);
  w.rec = (CholPanelRecord*)dev.alloc_bytes(p.ws_panels);
  return w;
}

// A = L L^T over the lower triangle of a (device, row-major); returns the launches made
inline int64_t factor(HipDev& dev, const CholPlan& p, const Work& w, double* a, int64_t n, int64_t lda) {
  if (p.route == CholRoute::kSmall) {
    const k::CholSmallArgs s{a, lda, (int)n, w.st};
    hipLaunchKernelGGL(k::chol_small_kernel, dim3(1), dim3(k::kCholThreads), k::kCholSmallLdsBytes, dev.stream, s);
    CORRLA_HIP(hipGetLastError());
    return 1;
  }
  int64_t launches = 0;
  for (int64_t pi = 0; pi < p.npanels; ++pi) {
    const int64_t j0 = pi * p.nb, j1 = std::min(n, j0 + p.nb);
    const k::CholDiagArgs dg{a, lda, j0, (int)(j1 - j0), w.rec + pi};
    hipLaunchKernelGGL(k::chol_diag_kernel, dim3(1), dim3(k::kCholThreads), 0, dev.stream, dg);
    ++launches;
    if (j1 < n) {
      const k::CholPanelArgs pa{a, lda, n, j0, j1};
      hipLaunchKernelGGL(k::chol_panel_kernel, dim3((unsigned)chol_chunks(n, j1)), dim3(64), k::kCholPanelLdsBytes, dev.stream, pa);
      const k::CholUpdateArgs up{a, lda, n, j0, j1};
      hipLaunchKernelGGL(k::chol_update_kernel, dim3((unsigned)chol_tile_pairs(chol_trail_tiles(n, j1))), dim3(k::kCholThreads),
                         k::kCholUpdateLdsBytes, dev.stream, up);
      launches += 2;
    }
    CORRLA_HIP(hipGetLastError());
  }
  const k::CholFinishArgs fin{w.rec, p.npanels, w.st};
  hipLaunchKernelGGL(k::chol_finish_kernel, dim3(1), dim3(k::kCholThreads), 0, dev.stream, fin);
  CORRLA_HIP(hipGetLastError());
  return launches + 1;
}

template <bool TRANS>
inline void launch_tri(HipDev& dev, const double* t, int64_t ldt, int kv, double* x, int64_t ldx, int64_t n_rhs) {
  const k::CholTriArgs a{t, ldt, kv, x, ldx, n_rhs};
  hipLaunchKernelGGL((k::chol_tri_kernel<TRANS>), dim3((unsigned)chol_ceil_div(n_rhs, k::kCholTile)), dim3(64), 0, dev.stream, a);
}
template <bool TRANS>
inline void launch_gemm(HipDev& dev, const double* l, int64_t ldl, const double* x, int64_t ldx, double* c, int64_t ldc, int64_t m, int64_t n,
                        int kv) {
  const int64_t ntm = chol_ceil_div(m, k::kCholTile), ntn = chol_ceil_div(n, k::kCholTile);
  const k::CholGemmArgs a{l, ldl, x, ldx, c, ldc, m, n, kv, ntn};
  hipLaunchKernelGGL((k::chol_gemm_kernel<TRANS>), dim3((unsigned)(ntm * ntn)), dim3(k::kCholThreads), k::kCholGemmLdsBytes, dev.stream, a);
}

// B <- L^-T L^-1 B; returns the launches made
inline int64_t substitute(HipDev& dev, const CholPlan& p, const double* a, int64_t n, int64_t lda, double* b, int64_t n_rhs, int64_t ldb) {
  int64_t launches = 0;
  for (int64_t k0 = 0; k0 < n; k0 += p.nb) {  // forward, L
    const int64_t k1 = std::min(n, k0 + p.nb);
    launch_tri<false>(dev, a + k0 * lda + k0, lda, (int)(k1 - k0), b + k0 * ldb, ldb, n_rhs);
    ++launches;
    if (k1 < n) {
      launch_gemm<false>(dev, a + k1 * lda + k0, lda, b + k0 * ldb, ldb, b + k1 * ldb, ldb, n - k1, n_rhs, (int)(k1 - k0));
      ++launches;
    }
  }
  CORRLA_HIP(hipGetLastError());
  for (int64_t k0 = (p.nblocks - 1) * p.nb; k0 >= 0; k0 -= p.nb) {  // backward, L^T: block row k0 of L holds column block k0 of L^T
    const int64_t k1 = std::min(n, k0 + p.nb);
    launch_tri<true>(dev, a + k0 * lda + k0, lda, (int)(k1 - k0), b + k0 * ldb, ldb, n_rhs);
    ++launches;
    if (k0 > 0) {
      launch_gemm<true>(dev, a + k0 * lda, lda, b + k0 * ldb, ldb, b, ldb, k0, n_rhs, (int)(k1 - k0));
      ++launches;
    }
  }
  CORRLA_HIP(hipGetLastError());
  return launches;
}

// the read-back of the call; throws ENUMERIC on a failed column
inline void read_status(HipDev& dev, const CholPlan& p, const Work& w, const char* who, Ran* ran) {
  CholFactorStatus st{};
  CORRLA_HIP(hipMemcpyAsync(&st, w.st, sizeof(st), hipMemcpyDeviceToHost, dev.stream));
  dev.sync();
  ran->route = (int)p.route;
  ran->info = st.info;
  ran->min_diag = st.min_diag;
  ran->max_diag = st.max_diag;
  ran->logdet = st.logdet;
  if (st.info != 0)
    throw Error(ST_ENUMERIC, std::string(who) + ": the pivot of column " + std::to_string(st.info) +
                                 " (1-based) is not positive or not finite: the matrix is not positive definite or holds a non-finite entry");
}

inline void check_launches(const CholPlan& p, int64_t made_factor, int64_t made_solve) {
  if (made_factor != p.factor_launches || made_solve != p.solve_launches)
    throw Error(ST_EINVAL, "internal: chol launch count differs from the plan");
}

inline void run_factor(HipDev& dev, bool host_ptrs, const CholFactorCall& c, Ran* ran) {
  const CholPlan p = plan_of(c.n, 0);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  const FactorArrays on = stage_factor(dev, io, host_ptrs, c);
  const Work w = workspace(dev, p);
  check_launches(p, factor(dev, p, w, on.l, c.n, on.ldl), 0);
  read_status(dev, p, w, "chol_factor", ran);
  finish_factor(io, host_ptrs, c);
}

inline void run_solve(HipDev& dev, bool host_ptrs, const LuSolveCall& c, Ran* ran) {
  const CholPlan p = plan_of(c.n, c.n_rhs);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  const lu_stage::SolveArrays on = lu_stage::stage_solve(dev, io, host_ptrs, c);
  const Work w = workspace(dev, p);
  const int64_t nf = factor(dev, p, w, on.a, c.n, c.lda);
  const int64_t ns = substitute(dev, p, on.a, c.n, c.lda, on.b, c.n_rhs, on.ldb);
  check_launches(p, nf, ns);
  read_status(dev, p, w, "chol_solve", ran);
  io.finish();
}

}  // namespace chol_stage
}  // namespace corrla
