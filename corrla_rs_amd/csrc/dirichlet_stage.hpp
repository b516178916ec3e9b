// The Dirichlet stage of the C ABI (corrla_dirichlet_draws_* / corrla_dirichlet_sample_*; constr_dirichlet_sample,
// space_samplers.rs:14-126): the kernels of dirichlet_kernels.hpp by the plan of dirichlet_plan.hpp, and for host pointers the
// copies around them.  The arguments were checked by dirichlet_draws_entry / dirichlet_sample_entry (capi_impl.hpp), which
// also hand over the plan they checked them with.
// alphas and bounds always arrive through host pointers: the component table (DirComp) is built on the host and uploaded
// with one synchronising copy.  The draws entry then enqueues and returns on the device path.  The sampling entry has to learn
// when to stop: it queues launches in batches (dir_next_batch) and reads the 24-byte state back once per batch, so it
// synchronises in both kinds of call; the samples do not depend on the batching.
#pragma once
#include <vector>

#include "capi_impl.hpp"
#include "hip_backend.hpp"
#include "host_io.hpp"

namespace corrla {
namespace dirichlet_stage {

// what corrla_ctx_last_dirichlet reports of the context's last call
struct Ran {
  int route = 0;      // DirRoute
  int readbacks = 0;  // of the state, by corrla_dirichlet_sample_*
  int launches = 0;   // TEST launches queued, those that returned at the "enough" word included
};

inline const DirComp* upload_table(HipDev& dev, int64_t d, const double* alphas, const double* bounds) {
  std::vector<DirComp> tab((size_t)d);
  for (int64_t j = 0; j < d; ++j) {
    tab[(size_t)j] = dir_component(alphas[j]);
    if (bounds) tab[(size_t)j].lb = bounds[2 * j], tab[(size_t)j].ub = bounds[2 * j + 1];
  }
  DirComp* t = (DirComp*)dev.alloc_bytes(tab.size() * sizeof(DirComp));
  dev.h2d_bytes(t, tab.data(), tab.size() * sizeof(DirComp));  // complete when it returns: `tab` may go
  return t;
}

template <template <int, bool> class Launch, class Args>
void by_route(const DirPlan& p, HipDev& dev, unsigned grid, const Args& a) {
  if (p.reg_width == 4)
    p.exp_only ? Launch<4, true>::go(dev, grid, a) : Launch<4, false>::go(dev, grid, a);
  else if (p.reg_width == k::kDirRegD)
    p.exp_only ? Launch<k::kDirRegD, true>::go(dev, grid, a) : Launch<k::kDirRegD, false>::go(dev, grid, a);
  else
    p.exp_only ? Launch<0, true>::go(dev, grid, a) : Launch<0, false>::go(dev, grid, a);
}
template <int DP, bool EXP>
struct LaunchDraw {
  static void go(HipDev& dev, unsigned grid, const k::DirDrawArgs& a) {
    hipLaunchKernelGGL((k::dir_draw_kernel<DP, EXP>), dim3(grid), dim3(k::kDirThreads), 0, dev.stream, a);
  }
};
template <int DP, bool EXP>
struct LaunchTest {
  static void go(HipDev& dev, unsigned grid, const k::DirTestArgs& a) {
    hipLaunchKernelGGL((k::dir_test_kernel<DP, EXP>), dim3(grid), dim3(k::kDirThreads), 0, dev.stream, a);
  }
};

inline void run_draws(HipDev& dev, bool host_ptrs, const DirichletDrawsCall& c, const DirPlan& p, Ran* ran) {
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  int64_t ldo = c.ldo;
  double* out = io.out_packed<double>(c.out_span(), &ldo);
  const k::DirStream st{upload_table(dev, c.d, c.alphas, nullptr), (int)c.d, c.seed, c.c_scale};
  const k::DirDrawArgs a{st, c.first, c.n, out, ldo};
  by_route<LaunchDraw>(p, dev, p.draw_grid_x, a);
  CORRLA_HIP(hipGetLastError());
  ran->route = (int)p.route;
  io.finish();
}

inline void run_sample(HipDev& dev, bool host_ptrs, const DirichletSampleCall& c, const DirPlan& p, Ran* ran) {
  dev.begin_call();
  HostIo<HipDev> io(dev, host_ptrs);
  int64_t ldo = c.ldo;
  double* out = io.out_packed<double>(c.out_span(), &ldo);
  const k::DirStream st{upload_table(dev, c.d, c.alphas, c.bounds), (int)c.d, c.seed, c.c_scale};
  unsigned long long* mask = (unsigned long long*)dev.alloc_bytes(p.ws_mask_bytes);
  unsigned int* count = (unsigned int*)dev.alloc_bytes(p.ws_count_bytes);
  unsigned long long* prefix = (unsigned long long*)dev.alloc_bytes(p.ws_prefix_bytes);
  k::DirState* state = (k::DirState*)dev.alloc_bytes(sizeof(k::DirState));
  dev.memset_zero(state, sizeof(k::DirState));
  // the rows nobody finds stay zero, as the reference leaves them: the d columns of every row, never the gap up to ldo
  CORRLA_HIP(hipMemset2DAsync(out, (size_t)ldo * sizeof(double), 0, (size_t)c.d * sizeof(double), (size_t)c.n_samples, dev.stream));
  k::DirState seen{};
  int64_t done = 0, prev = 0;
  while (done < p.total_wgs && seen.total < (unsigned long long)c.n_samples) {
    const int64_t batch = dir_next_batch(p.total_wgs, done, (int64_t)seen.total, c.n_samples, prev);
    for (int64_t q = 0; q < batch; q += p.launch_wgs) {
      const int64_t n_wgs = std::min(p.launch_wgs, batch - q), gw0 = done + q;
      const k::DirTestArgs t{st, gw0, n_wgs, p.wps, c.chunk_size, state, mask, count};
      by_route<LaunchTest>(p, dev, (unsigned)n_wgs, t);
      const k::DirScanArgs s{count, prefix, gw0, n_wgs, c.n_samples, state};
      hipLaunchKernelGGL(k::dir_scan_kernel, dim3(1), dim3(k::kDirScanThreads), 0, dev.stream, s);
      const k::DirEmitArgs e{st, gw0, n_wgs, p.wps, c.chunk_size, mask, count, prefix, c.n_samples, out, ldo};
      const unsigned emit_grid = (unsigned)((n_wgs * k::kDirWords + k::kDirThreads - 1) / k::kDirThreads);
      if (p.exp_only)
        hipLaunchKernelGGL((k::dir_emit_kernel<true>), dim3(emit_grid), dim3(k::kDirThreads), 0, dev.stream, e);
      else
        hipLaunchKernelGGL((k::dir_emit_kernel<false>), dim3(emit_grid), dim3(k::kDirThreads), 0, dev.stream, e);
      CORRLA_HIP(hipGetLastError());
      ++ran->launches;
    }
    CORRLA_HIP(hipMemcpyAsync(&seen, state, sizeof(seen), hipMemcpyDeviceToHost, dev.stream));
    dev.sync();
    ++ran->readbacks;
    done += batch;
    prev = batch;
  }
  const bool all = seen.total >= (unsigned long long)c.n_samples;
  *c.n_found = all ? c.n_samples : (int64_t)seen.total;
  *c.n_drawn = (all ? seen.cross_gw / p.wps + 1 : c.max_zshots) * c.chunk_size;
  ran->route = (int)p.route;
  io.finish();
}

}  // namespace dirichlet_stage
}  // namespace corrla
