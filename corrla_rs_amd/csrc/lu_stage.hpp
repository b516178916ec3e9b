// The dense-solve stage of the C ABI (corrla_lu_solve_*, corrla_rbffit_system_*, corrla_rbffit_*): the kernels of
// lu_kernels.hpp by the plan of lu_plan.hpp, and for host pointers the copies around them.  The arguments were checked by
// lu_solve_entry / rbf_system_entry / rbf_fit_entry (capi_impl.hpp).
// A solve enqueues every launch of the factorisation and of the substitutions without waiting for the device, then makes the
// one read-back of the call: the 24-byte status record (info, smallest |pivot|, largest |u_ij|).  So the device entries of a
// solve synchronise once, unlike rbf_stage's; corrla_rbffit_system_dev_* only enqueues.  info != 0 ends the call with
// CORRLA_ENUMERIC after the record is kept for corrla_ctx_last_solve; the kernels behind the failed column have returned at
// once, the arrays hold a partial factorisation.  The host path (HostIo, host_io.hpp) copies the strided spans to the device
// as they lie and the n x n_rhs block of the result back; the padding columns are never written.
#pragma once
#include <string>

#include "capi_impl.hpp"
#include "hip_backend.hpp"
#include "host_io.hpp"
#include "lu_kernels.hpp"
#include "lu_staging.hpp"
#include "rbf_stage.hpp"

namespace corrla {
namespace lu_stage {

// what corrla_ctx_last_solve reports of the context's last call
struct Ran {
  int route = 0;  // LuRoute
  int64_t info = 0;
  double min_pivot = 0.0, max_u = 0.0;
};

inline void set_lds_limits() {
  lds_limit((const void*)k::lu_small_kernel, k::kLuSmallLdsBytes);
  lds_limit((const void*)k::lu_update_kernel, k::kLuUpdateLdsBytes);
}

inline LuPlan plan_of(int64_t n, int64_t n_rhs) {
  LuShape s;
  s.n = n, s.n_rhs = n_rhs;
  const LuPlan p = lu_plan(s);
  if (!p.ok) throw Error(ST_EINVAL, p.error);
  return p;
}

struct Work {
  LuStatus* st;
  k::LuBest* part;
  double* maxu;
  int64_t* ipiv;
};
inline Work workspace(HipDev& dev, const LuPlan& p, int64_t* ipiv) {
  Work w;
  w.st = (LuStatus*)dev.alloc_bytes(p.ws_status);
  w.part = (k::LuBest*)dev.alloc_bytes(p.ws_partials);
  w.maxu = (double*)dev.alloc_bytes(p.ws_maxu);
  w.ipiv = ipiv ? ipiv : (int64_t*)dev.alloc_bytes(p.ws_ipiv);
  return w;
}

inline unsigned blocks_of(int64_t threads) { return (unsigned)((threads + k::kLuThreads - 1) / k::kLuThreads); }

inline void launch_update(HipDev& dev, const double* l, int64_t ldl, const double* u, int64_t ldu, double* c, int64_t ldc, int64_t m, int64_t n,
                          int kv, const LuStatus* st) {
  const int64_t ntm = lu_ceil_div(m, k::kLuTile), ntn = lu_ceil_div(n, k::kLuTile);
  const k::LuUpdateArgs a{l, ldl, u, ldu, c, ldc, m, n, kv, ntn, st};
  hipLaunchKernelGGL(k::lu_update_kernel, dim3((unsigned)(ntm * ntn)), dim3(k::kLuThreads), k::kLuUpdateLdsBytes, dev.stream, a);
}
template <bool UPPER>
inline void launch_tri(HipDev& dev, const double* t, int64_t ldt, int kv, double* x, int64_t ldx, int64_t c0, int64_t c1, const LuStatus* st) {
  const k::LuTriArgs a{t, ldt, kv, x, ldx, c0, c1, st};
  hipLaunchKernelGGL((k::lu_tri_kernel<UPPER>), dim3((unsigned)lu_ceil_div(c1 - c0, k::kLuTile)), dim3(64), 0, dev.stream, a);
}

// P A = L U over a (device, row-major); returns the launches made
inline int64_t factor(HipDev& dev, const LuPlan& p, const Work& w, double* a, int64_t n, int64_t lda) {
  int64_t launches = 0;
  if (p.route == LuRoute::kSmall) {
    const k::LuSmallArgs s{a, lda, (int)n, w.ipiv, w.st};
    hipLaunchKernelGGL(k::lu_small_kernel, dim3(1), dim3(k::kLuThreads), k::kLuSmallLdsBytes, dev.stream, s);
    CORRLA_HIP(hipGetLastError());
    return 1;
  }
  for (int64_t j0 = 0; j0 < n; j0 += p.nb) {
    const int64_t j1 = std::min(n, j0 + p.nb);
    for (int64_t j = j0; j < j1; ++j) {
      // the partial maxima of column j were left by step j - 1 of the same panel
      const k::LuPivotArgs pv{a, lda, n, j, j0, j1, w.part, j == j0 ? 0 : lu_step_chunks(n, j - 1), w.ipiv, w.st};
      hipLaunchKernelGGL(k::lu_pivot_kernel, dim3(1), dim3(k::kLuThreads), 0, dev.stream, pv);
      const k::LuPanelArgs pa{a, lda, n, j, j0, j1, w.part, w.st};
      hipLaunchKernelGGL(k::lu_panel_kernel, dim3((unsigned)lu_step_chunks(n, j)), dim3(k::kLuThreads), 0, dev.stream, pa);
      launches += 2;
    }
    const k::LuSwapArgs sw{a, lda, 0, j0, j1, n, w.ipiv, j0, j1, n, w.st};
    hipLaunchKernelGGL(k::lu_swap_kernel, dim3(blocks_of(j0 + (n - j1))), dim3(k::kLuThreads), 0, dev.stream, sw);
    ++launches;
    if (j1 < n) {
      launch_tri<false>(dev, a + j0 * lda + j0, lda, (int)(j1 - j0), a + j0 * lda, lda, j1, n, w.st);
      launch_update(dev, a + j1 * lda + j0, lda, a + j0 * lda + j1, lda, a + j1 * lda + j1, lda, n - j1, n - j1, (int)(j1 - j0), w.st);
      launches += 2;
    }
    CORRLA_HIP(hipGetLastError());
  }
  const k::LuMaxUArgs mu{a, lda, n, w.maxu, p.maxu_blocks, w.st};
  hipLaunchKernelGGL(k::lu_maxu_kernel, dim3((unsigned)p.maxu_blocks), dim3(k::kLuThreads), 0, dev.stream, mu);
  hipLaunchKernelGGL(k::lu_maxu_finish_kernel, dim3(1), dim3(k::kLuThreads), 0, dev.stream, mu);
  CORRLA_HIP(hipGetLastError());
  return launches + 2;
}

// B <- U^-1 L^-1 P B; returns the launches made
inline int64_t substitute(HipDev& dev, const LuPlan& p, const Work& w, const double* a, int64_t n, int64_t lda, double* b, int64_t n_rhs,
                          int64_t ldb) {
  int64_t launches = 1;
  const k::LuSwapArgs sw{b, ldb, 0, n_rhs, 0, 0, w.ipiv, 0, n, n, w.st};
  hipLaunchKernelGGL(k::lu_swap_kernel, dim3(blocks_of(n_rhs)), dim3(k::kLuThreads), 0, dev.stream, sw);
  for (int64_t k0 = 0; k0 < n; k0 += p.nb) {  // forward, unit lower
    const int64_t k1 = std::min(n, k0 + p.nb);
    launch_tri<false>(dev, a + k0 * lda + k0, lda, (int)(k1 - k0), b + k0 * ldb, ldb, 0, n_rhs, w.st);
    ++launches;
    if (k1 < n) {
      launch_update(dev, a + k1 * lda + k0, lda, b + k0 * ldb, ldb, b + k1 * ldb, ldb, n - k1, n_rhs, (int)(k1 - k0), w.st);
      ++launches;
    }
  }
  CORRLA_HIP(hipGetLastError());
  for (int64_t k0 = (p.nblocks - 1) * p.nb; k0 >= 0; k0 -= p.nb) {  // backward, upper
    const int64_t k1 = std::min(n, k0 + p.nb);
    launch_tri<true>(dev, a + k0 * lda + k0, lda, (int)(k1 - k0), b + k0 * ldb, ldb, 0, n_rhs, w.st);
    ++launches;
    if (k0 > 0) {
      launch_update(dev, a + k0, lda, b + k0 * ldb, ldb, b, ldb, k0, n_rhs, (int)(k1 - k0), w.st);
      ++launches;
    }
  }
  CORRLA_HIP(hipGetLastError());
  return launches;
}

// the read-back of the call; throws ENUMERIC on a failed column
inline void read_status(HipDev& dev, const LuPlan& p, const Work& w, const char* who, Ran* ran) {
  LuStatus st{};
  CORRLA_HIP(hipMemcpyAsync(&st, w.st, sizeof(st), hipMemcpyDeviceToHost, dev.stream));
  dev.sync();
  ran->route = (int)p.route;
  ran->info = st.info;
  ran->min_pivot = st.min_pivot;
  ran->max_u = st.max_u;
  if (st.info != 0)
    throw Error(ST_ENUMERIC, std::string(who) + ": the pivot of column " + std::to_string(st.info) +
                                 " (1-based) is exactly zero or not finite: the matrix is singular or holds a non-finite entry");
}

inline void check_launches(const LuPlan& p, int64_t made_factor, int64_t made_solve) {
  if (made_factor != p.factor_launches || made_solve != p.solve_launches) throw Error(ST_EINVAL, "internal: lu launch count differs from the plan");
}

inline void run_solve(HipDev& dev, bool host_ptrs, const LuSolveCall& c, Ran* ran) {
  const LuPlan p = plan_of(c.n, c.n_rhs);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  const SolveArrays on = stage_solve(dev, io, host_ptrs, c);
  const Work w = workspace(dev, p, host_ptrs ? nullptr : c.ipiv);
  const int64_t nf = factor(dev, p, w, on.a, c.n, c.lda);
  const int64_t ns = substitute(dev, p, w, on.a, c.n, c.lda, on.b, c.n_rhs, on.ldb);
  check_launches(p, nf, ns);
  read_status(dev, p, w, "lu_solve", ran);
  io.finish();
}

// M = [[K, P], [P^T, 0]] into m (device): the K block by rbf_matrix_kernel with the system's row stride, the rest by
// rbf_tail_kernel
inline void build_system(HipDev& dev, const double* xs, int64_t n_s, int64_t ldxs, int64_t dim, int kernel, double eps, int poly_degree,
                         double* m, int64_t ldm) {
  const RbfPlan rp = rbf_stage::plan_of(n_s, n_s, dim, 1, 0, 8, RbfMode::kMatrix);
  k::RbfMatrixArgs<double> a{xs, ldxs, xs, ldxs, n_s, n_s, (int)dim, eps, rp.nrg, m, ldm};
  with_nt<4>(kernel, [&](auto kn) {
    hipLaunchKernelGGL((k::rbf_matrix_kernel<double, decltype(kn)::value>), dim3(rp.grid_x), dim3(rp.block), rp.lds_bytes, dev.stream, a);
  });
  CORRLA_HIP(hipGetLastError());
  const int64_t n_poly = rbf_poly_terms(dim, poly_degree);
  if (n_poly > 0) {
    const k::RbfTailArgs t{xs, ldxs, n_s, (int)dim, poly_degree >= 2 ? 2 : 1, n_poly, m, ldm};
    hipLaunchKernelGGL(k::rbf_tail_kernel, dim3(blocks_of(n_s * n_poly + n_poly * n_poly)), dim3(k::kLuThreads), 0, dev.stream, t);
    CORRLA_HIP(hipGetLastError());
  }
}

inline void run_rbf_system(HipDev& dev, bool host_ptrs, const RbfFitCall& c) {
  (void)plan_of(c.order(), 0);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  const double* xs = io.in_as_lies<double>(c.xs_span());
  double* m = io.out_as_lies<double>(c.system_span());
  build_system(dev, xs, c.n_s, c.ldxs, c.dim, c.kernel, c.eps, c.poly_degree, m, c.ldm);
  io.finish();
}

inline void run_rbf_fit(HipDev& dev, bool host_ptrs, const RbfFitCall& c, Ran* ran) {
  const int64_t n = c.order();
  const LuPlan p = plan_of(n, c.n_rhs);
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  const FitArrays on = stage_fit(io, c);
  double* m = (double*)dev.alloc_bytes((size_t)n * (size_t)n * 8);
  build_system(dev, on.xs, c.n_s, c.ldxs, c.dim, c.kernel, c.eps, c.poly_degree, m, n);
  const k::LuRhsArgs r{on.y, c.ldy, c.n_s, n, c.n_rhs, on.coeffs, c.ldw};
  hipLaunchKernelGGL(k::lu_rhs_kernel, dim3(blocks_of(n * c.n_rhs)), dim3(k::kLuThreads), 0, dev.stream, r);
  CORRLA_HIP(hipGetLastError());
  const Work w = workspace(dev, p, nullptr);
  const int64_t nf = factor(dev, p, w, m, n, n);
  const int64_t ns = substitute(dev, p, w, m, n, n, on.coeffs, c.n_rhs, c.ldw);
  check_launches(p, nf, ns);
  read_status(dev, p, w, "rbf_fit", ran);
  io.finish();
}

}  // namespace lu_stage
}  // namespace corrla
