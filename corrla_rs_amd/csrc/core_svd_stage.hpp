// The SVD of the l x l core on the device (random_svd.rs:89): one launcher per kernel family.  core_svd_plan.hpp has
// decided the family, every grid, workgroup size, LDS and workspace size, the tolerances and the sweep counts; a launcher
// allocates what the plan sized, fills the kernel's arguments and launches.  HipDev::small_svd, the Dev entry, is defined
// at the end: knobs from the environment, plan, switch.
#pragma once
#include "core_svd_plan.hpp"
#include "hip_backend.hpp"

namespace corrla {

template <class T>
struct CoreSvdCall {
  const Skinny<T>& c;  // the l x l core
  int64_t l, k;
  Skinny<T>&m1, &m2;   // out: the first k columns of the two factors
  T* s_dev;            // out: k singular values
  // device CholStatus record that receives the convergence verdict of the fixed number of sweeps enqueued without any
  // synchronisation (the caller checks it later); nullptr: sweeps are enqueued in groups and the host waits for each
  // group until the iteration has converged
  void* conv_status;
};

namespace core_svd_stage {

// The instantiations the launchers dispatch on; set_lds_limits walks the same lists.
template <class T>
using RingEs = std::integer_sequence<int, 8, 12, 16, sizeof(T) == 4 ? 20 : 18>;  // jacobi_ring_w_kernel<T, E, 8>
constexpr int kMaxNc = 9;                                                          // jmc_step_kernel<T, 1 .. 9, 16>

// every kernel of the stage launched with more dynamic LDS than the default (HipDev::set_lds_limits)
template <class T>
inline void set_lds_limits() {
  for_each_of(RingEs<T>{}, [](auto e) { lds_limit((const void*)k::jacobi_ring_w_kernel<T, decltype(e)::value, 8>, k::kLdsMaxBytes); });
  lds_limit((const void*)k::jacobi_block_round_kernel<T>, k::kLdsMaxBytes);
  for_each_nt<kMaxNc>([](auto nc) { lds_limit((const void*)k::jmc_step_kernel<T, decltype(nc)::value, k::kJmcLanes>, k::kLdsMaxBytes); });
}

// ---- multi-workgroup block Jacobi (jacobi_mc_kernels.hpp) ----
template <class T>
inline void multi_wg(HipDev& dev, const CoreSvdCall<T>& a, const CoreSvdPlan& plan) {
  const CoreSvdPlan::MultiWg& p = plan.mc;
  const int l = (int)a.l;
  T* wj = (T*)dev.alloc_bytes(p.ws_bytes);
  T* vj = (T*)dev.alloc_bytes(p.ws_bytes);
  k::JmcCtl* ctl = (k::JmcCtl*)dev.alloc_bytes(sizeof(k::JmcCtl));
  k::CholStatus* st = a.conv_status ? (k::CholStatus*)a.conv_status : (k::CholStatus*)dev.alloc_bytes(sizeof(k::CholStatus));
  hipLaunchKernelGGL((k::jmc_init_kernel<T>), dim3(1), dim3(1024), 0, dev.stream, (const T*)a.c.p, a.c.ld, l, wj, vj, p.rp,
                     p.ncols_pad, p.force_v, ctl);
  const T tol = (T)plan.tol, tol_early = (T)plan.tol_early, floor2 = (T)plan.floor2;
  auto enqueue_sweeps = [&](int s0, int s1) {
    for (int sw = s0; sw < s1; ++sw)
      for (int step = 0; step < p.nblocks - 1; ++step)
        with_nt<kMaxNc>(p.nc, [&](auto nc) {
          hipLaunchKernelGGL((k::jmc_step_kernel<T, decltype(nc)::value, k::kJmcLanes>), dim3((unsigned)p.np), dim3(p.step_threads),
                             p.step_lds, dev.stream, wj, vj, p.b, p.nblocks, step, sw, step == 0 ? 1 : 0, tol, tol_early, floor2,
                             ctl, p.local);
        });
    CORRLA_HIP(hipGetLastError());
  };
  auto finish = [&](int nsw) {
    hipLaunchKernelGGL((k::jmc_finish_kernel<T>), dim3(1), dim3(1024), p.fin_lds, dev.stream, (const T*)wj, (const T*)vj, p.rp, l,
                       nsw, (const k::JmcCtl*)ctl, a.m1.p, a.m1.ld, a.m2.p, a.m2.ld, a.s_dev, (int)a.k, st);
    // W-only mode: the accumulated-rotation factor is recovered from the core itself (no-op otherwise)
    hipLaunchKernelGGL((k::jmc_other_factor_kernel<T>), dim3(p.other_grid), dim3(256), 0, dev.stream, (const T*)a.c.p, a.c.ld, l,
                       (int)a.k, (const T*)a.m2.p, a.m2.ld, (const T*)a.s_dev, (const k::JmcCtl*)ctl, a.m1.p, a.m1.ld);
    CORRLA_HIP(hipGetLastError());
  };
  if (a.conv_status) {
    const int nsw = p.nsw;
    enqueue_sweeps(0, nsw);
    finish(nsw);
    if (env_int("CORRLA_DEBUG", 0)) {
      k::JmcCtl hd;
      CORRLA_HIP(hipMemcpyAsync(&hd, ctl, sizeof(hd), hipMemcpyDeviceToHost, dev.stream));
      dev.sync();
      int used = 0;
      while (used < nsw && hd.rot[used] && hd.big[used]) ++used;
      std::fprintf(stderr, "[corrla] jacobi_svd (multi-workgroup, %d sweeps enqueued, %s) l=%d np=%d b=%d nc=%d sweeps run=%d rounds(wg0)=%llu "
                           "cycles/round=%.0f ns/round=%.0f (%.0f MHz)\n", nsw, hd.with_v ? "V accumulated" : "W only", l, p.np, p.b, p.nc, std::min(used + 1, nsw),
                   hd.rounds, hd.rounds ? (double)hd.clk / hd.rounds : 0.0, hd.rounds ? 10.0 * hd.wall / hd.rounds : 0.0,
                   hd.wall ? 100.0 * hd.clk / hd.wall : 0.0);
      if (hd.steps)
        std::fprintf(stderr, "[corrla]   per step (wg0, us): load %.2f norms %.2f rounds %.2f store %.2f total %.2f over %llu steps\n",
                     0.01 * hd.t_load / hd.steps, 0.01 * hd.t_norm / hd.steps, 0.01 * hd.wall / hd.steps,
                     0.01 * hd.t_store / hd.steps, 0.01 * hd.t_total / hd.steps, hd.steps);
      if (hd.steps > 1)
        std::fprintf(stderr, "[corrla]   span first-start..last-end over all workgroups: %.2f us per step\n",
                     0.01 * hd.t_span / (hd.steps - 1));
    }
    return;
  }
  int done = 0;
  k::JmcCtl h;
  while (done < p.max_sweeps) {
    const int s1 = std::min(p.max_sweeps, done + p.group);
    enqueue_sweeps(done, s1);
    CORRLA_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, dev.stream));
    dev.sync();
    bool conv = false;
    for (int s_ = 0; s_ < s1; ++s_) conv = conv || !(h.rot[s_] && h.big[s_]);
    done = s1;
    if (conv || h.bad) break;
  }
  if (h.bad) throw Error(ST_ENUMERIC, "non-finite core matrix in small SVD");
  finish(done);
  if (env_int("CORRLA_DEBUG", 0)) {
    int used = 0;
    while (used < done && h.rot[used] && h.big[used]) ++used;
    std::fprintf(stderr, "[corrla] jacobi_svd (multi-workgroup) l=%d np=%d b=%d sweeps=%d\n", l, p.np, p.b, used + 1);
  }
}

// The ring and block Jacobi kernels carry no status word: a non-finite core would come back as a triplet of zeros.
// One small launch scans the core first: optimistic runs find fail = 3 in the status record at the end of the call,
// host-controlled ones read the word now.
template <class T>
inline void finite_check(HipDev& dev, const CoreSvdCall<T>& a, int* sexp_out = nullptr) {
  // sexp_out (the block Jacobi): device word that receives the power-of-two prescale of a core far from unit scale
  int* bad = a.conv_status ? nullptr : dev.alloc_flags(1);
  hipLaunchKernelGGL((k::core_finite_check_kernel<T>), dim3(1), dim3(1024), 0, dev.stream, (const T*)a.c.p, a.c.ld, (int)a.l,
                     (k::CholStatus*)a.conv_status, bad, sexp_out);
  CORRLA_HIP(hipGetLastError());
  if (bad) {
    int h = 0;
    dev.read_flags(bad, 1, &h);
    if (h) throw Error(ST_ENUMERIC, "non-finite core matrix in small SVD");
  }
}

// ---- block Jacobi, one launch per round ----
template <class T>
inline void block(HipDev& dev, const CoreSvdCall<T>& a, const CoreSvdPlan& plan, const int* sexp) {
  const CoreSvdPlan::Block& p = plan.blk;
  const int64_t ld = p.rows_pad;
  T* wj = (T*)dev.alloc_bytes(p.ws_bytes);
  T* vj = (T*)dev.alloc_bytes(p.ws_bytes);
  k::JacobiCtl* ctl = (k::JacobiCtl*)dev.alloc_bytes(sizeof(k::JacobiCtl));
  hipLaunchKernelGGL((k::jacobi_init_kernel<T>), dim3(64), dim3(256), 0, dev.stream, (const T*)a.c.p, a.c.ld, (int)a.l, wj, ld, vj,
                     ld, p.cols_pad, p.rows_pad, ctl, sexp);
  for (int sw = 0; sw < p.max_sweeps; ++sw) {
    for (int round = 0; round < p.nb - 1; ++round)
      hipLaunchKernelGGL((k::jacobi_block_round_kernel<T>), dim3(p.nb / 2), dim3(256), p.round_lds, dev.stream, wj, ld, vj, ld,
                         p.rows_pad, p.nb, round, p.inner, ctl);
    hipLaunchKernelGGL(k::jacobi_sweep_end_kernel, dim3(1), dim3(1), 0, dev.stream, ctl, (float)plan.tol_early);
  }
  hipLaunchKernelGGL((k::jacobi_finish_kernel<T>), dim3(1), dim3(1024), p.fin_lds, dev.stream, (const T*)wj, ld, (const T*)vj,
                     ld, (int)a.l, a.m1.p, a.m1.ld, a.m2.p, a.m2.ld, a.s_dev, (int)a.k, sexp);
  CORRLA_HIP(hipGetLastError());
  if (env_int("CORRLA_DEBUG", 0)) {
    k::JacobiCtl h;
    CORRLA_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, dev.stream));
    dev.sync();
    std::fprintf(stderr, "[corrla] block jacobi l=%d nb=%d sweeps=%u done=%u\n", (int)a.l, p.nb, h.sweeps, h.done);
  }
}

// ---- single-workgroup ring Jacobi: W in registers, 8 lanes x E rows per column (jacobi_ring_w_kernel), then V from the
// recorded rotations (jacobi_replay_v_kernel) ----
template <class T>
inline void ring(HipDev& dev, const CoreSvdCall<T>& a, const CoreSvdPlan& plan) {
  static_assert(sizeof(k::RotEntry<T>) == 2 * sizeof(T), "CoreSvdPlan::Ring::rot_bytes");
  const CoreSvdPlan::Ring& p = plan.ring;
  int* info = (int*)dev.alloc_bytes(sizeof(int) * 4);
  k::RotEntry<T>* rot = (k::RotEntry<T>*)dev.alloc_bytes(p.rot_bytes);
  int* rank_g = (int*)dev.alloc_bytes(p.rank_bytes);
  const T tol = (T)plan.tol, tol_early = (T)plan.tol_early;
  with_one_of(RingEs<T>{}, plan.ring_e, [&](auto e) {
    hipLaunchKernelGGL((k::jacobi_ring_w_kernel<T, decltype(e)::value, 8>), dim3(1), dim3(p.block), p.lds, dev.stream, (const T*)a.c.p,
                       a.c.ld, (int)a.l, a.m2.p, a.m2.ld, a.s_dev, (int)a.k, tol, tol_early, p.max_sw, rot, rank_g, info);
  });
  CORRLA_HIP(hipGetLastError());
  hipLaunchKernelGGL((k::jacobi_replay_v_kernel<T>), dim3(p.replay_grid), dim3(256), 0, dev.stream, (const k::RotEntry<T>*)rot,
                     (const int*)info, (const int*)rank_g, (int)a.l, (int)a.k, a.m1.p, a.m1.ld);
  CORRLA_HIP(hipGetLastError());
  if (env_int("CORRLA_DEBUG", 0)) {
    int h[4] = {0, 0, 0, 0};
    CORRLA_HIP(hipMemcpyAsync(h, info, sizeof(int), hipMemcpyDeviceToHost, dev.stream));
    dev.sync();
    std::fprintf(stderr, "[corrla] jacobi_svd (ring) l=%d sweeps=%d\n", (int)a.l, h[0]);
  }
}

// every knob of the stage, read at the start of each call
inline CoreSvdKnobs knobs_from_env() {
  CoreSvdKnobs kn;
  kn.mode = std::getenv("CORRLA_SVD");
  kn.host_svd = env_int("CORRLA_HOST_SVD", 0) != 0;
  kn.jmc_min_l = env_int("CORRLA_JMC_MIN_L", kn.jmc_min_l);
  kn.jmc_max_b = std::min(32, std::max(2, env_int("CORRLA_JMC_MAX_B", kn.jmc_max_b)));
  kn.jmc_local = env_int("CORRLA_JMC_LOCAL", kn.jmc_local);
  kn.jmc_np = env_int("CORRLA_JMC_NP", kn.jmc_np);
  kn.jmc_sweeps_f32 = env_int("CORRLA_JMC_SWEEPS", kn.jmc_sweeps_f32);
  kn.jmc_sweeps_f64 = env_int("CORRLA_JMC_SWEEPS", kn.jmc_sweeps_f64);
  kn.jmc_force_v = env_int("CORRLA_JMC_FORCE_V", 0) != 0;
  kn.strict = env_int("CORRLA_JACOBI_STRICT", 0) != 0;
  kn.block_sweeps = env_int("CORRLA_JACOBI_SWEEPS", kn.block_sweeps);
  kn.ring_sweeps = env_int("CORRLA_JACOBI_SWEEPS", kn.ring_sweeps);
  kn.block_inner = env_int("CORRLA_JACOBI_INNER", kn.block_inner);
  return kn;
}

}  // namespace core_svd_stage

// SVD of the l x l core: the launcher of the family core_svd_plan picks for l and the knobs.
template <class T>
void HipDev::small_svd(const Skinny<T>& c, int64_t l, int64_t k, Skinny<T>& m1, Skinny<T>& m2, T* s_dev, void* conv_status) {
  // conv_status (optional): kernels that run a FIXED number of sweeps report there whether they converged, the others
  // (loop to convergence inside one launch) leave it cleared = converged
  if (conv_status) memset_zero(conv_status, sizeof(k::CholStatus));
  const CoreSvdCall<T> a{c, l, k, m1, m2, s_dev, conv_status};
  const CoreSvdPlan plan = core_svd_plan((int)sizeof(T), l, k, core_svd_stage::knobs_from_env(), svd_state_, conv_status != nullptr);
  switch (plan.family) {
    case CoreSvd::kMultiWg:
      core_svd_stage::multi_wg(*this, a, plan);
      return;
    case CoreSvd::kHost:
      small_svd_host(*this, c, l, k, m1, m2, s_dev);
      return;
    case CoreSvd::kBlock: {
      int* sexp = (int*)alloc_bytes(sizeof(int));  // written by the check, read by the kernels behind it in stream order
      core_svd_stage::finite_check(*this, a, sexp);
      core_svd_stage::block(*this, a, plan, sexp);
      return;
    }
    case CoreSvd::kRing:
      core_svd_stage::finite_check(*this, a);
      core_svd_stage::ring(*this, a, plan);
      return;
  }
}

}  // namespace corrla
