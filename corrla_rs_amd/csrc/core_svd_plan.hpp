// The plan of the SVD of the l x l core (random_svd.rs:89): which kernel family takes it, and everything its launches need
// -- geometry, grids, workgroup sizes, LDS, workspaces, tolerances, sweep counts -- with the LDS arithmetic that rests on.
// core_svd_stage.hpp launches what the plan says and computes none of it again.
// Host code only, no HIP call: tests/test_core_svd_plan.py compiles this header with the host compiler and pins the
// choice at every l and every field.  The kernels that use the size helpers on the device include it through
// jacobi_mc_kernels.hpp and hip_kernels.hpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CORRLA_HD __host__ __device__
#else
#define CORRLA_HD
#endif

namespace corrla {
namespace k {

constexpr size_t kLdsMaxBytes = (size_t)160 * 1024;  // dynamic LDS of one workgroup on gfx950

// ---- multi-workgroup block Jacobi (jacobi_mc_kernels.hpp) ----
constexpr int kJmcMaxSweeps = 40;
// lanes per Jacobi processor.  (8-lane processors -- half the waves for the same block pair, twice the column per
// lane -- measured 6 % slower at l = 138 f32: the rounds are bound by the per-lane column traffic, not by the
// rotation arithmetic they would amortise; the kernel keeps the template parameter, nothing instantiates 8.)
constexpr int kJmcLanes = 16;
// rows per column image: NC chunk rows of `lanes` lanes x 2 elements
CORRLA_HD constexpr int jmc_rows(int nc, int lanes) { return nc * 2 * lanes; }
// LDS column pitch (elements).  16 lanes per processor: b64 reads (f32) are serviced per 32-lane half = two
// processors, whose 128-byte segments must fall in different halves of the 256-byte bank row -> pitch = 32 (mod 64);
// b128 reads (f64) are serviced in interleaved 16-lane groups that mix two processors -> their columns must be
// bank-aligned, pitch = 0 (mod 32).  8 lanes per processor (f32 only): a 32-lane half is four processors reading 64
// bytes each from four (mostly consecutive) columns -> pitch = 16 or 48 (mod 64).
CORRLA_HD constexpr int jmc_pitch(int nc, int esz, int lanes) {
  return lanes == 8 ? (jmc_rows(nc, 8) + ((nc % 2 == 0) ? 16 : 0))
                    : (esz == 4 ? (jmc_rows(nc, 16) + ((nc % 2 == 0) ? 32 : 0)) : jmc_rows(nc, 16));
}
CORRLA_HD constexpr size_t jmc_lds_bytes(int nc, int b, int esz, int lanes) {
  return (size_t)2 * (2 * b) * jmc_pitch(nc, esz, lanes) * esz + (size_t)2 * b * esz + 64;
}

// ---- single-workgroup ring Jacobi (jacobi_ring_w_kernel, jacobi_replay_v_kernel, hip_kernels.hpp) ----
constexpr int kRingProcPad = 72;  // processors per stream row (padded)
constexpr int kReplayLanes = 16;  // lanes per row of V (one DPP row): 10 line positions per lane (32 lanes: 6)
// rs = G * E: rows per column slot
CORRLA_HD inline size_t jacobi_ring_w_lds_bytes(int l, int rs, size_t esz) {
  const int n2 = (l + 1) & ~1;
  const int nproc = n2 / 2;  // launched with exactly G * np threads
  return (size_t)2 * nproc * rs * esz + (size_t)n2 * (esz + sizeof(int)) + (size_t)2 * nproc * esz + 64;
}
// rows per lane of the ring kernel's column slots (8 lanes per processor); l <= 144
inline int jacobi_ring_e(int64_t l, int esz) { return l <= 64 ? 8 : (l <= 96 ? 12 : (l <= 128 ? 16 : (esz == 4 ? 20 : 18))); }

// ---- block Jacobi, one launch per round (jacobi_block_round_kernel, hip_kernels.hpp) ----
inline size_t jacobi_block_round_lds_bytes(int rows_pad, size_t esz) {
  return (size_t)(2 * 16 * (rows_pad + 1) + 7 * 16 * 17 + 32) * esz + 16 * sizeof(int) + 64;
}
// jmc_finish_kernel and jacobi_finish_kernel: l + 2 norms and as many ranks
inline size_t jacobi_finish_lds_bytes(int l, size_t esz) { return (size_t)(l + 2) * esz + (size_t)(l + 2) * sizeof(int) + 64; }

}  // namespace k

// Geometry of the multi-workgroup block Jacobi for an l x l core, 16 lanes per processor: chunk rows NC, workgroups NP,
// block width b (a multiple of four, <= 32); false when it does not fit.  local: CORRLA_JMC_LOCAL (0 keeps the round-2
// rule: even widths), np_force: CORRLA_JMC_NP (0: the fewest workgroups whose block pair fits one CU and jmc_max_b).
inline bool jmc_geometry(int64_t l, int esz, int jmc_max_b, int local, int np_force, int* nc_out, int* np_out, int* b_out) {
  if (l < 2 || l > 288) return false;
  const int nc = (int)((l + 2 * k::kJmcLanes - 1) / (2 * k::kJmcLanes));
  // block width: a multiple of four columns (= whole waves of four 16-lane processors, whole sub-blocks of the
  // wave-local schedule)
  auto width = [&](int np_) {
    int bb = (int)((l + 2 * np_ - 1) / (2 * np_));
    return local ? (bb + 3) / 4 * 4 : bb + (bb & 1);
  };
  int np = np_force;
  if (np <= 0) {
    // fewest workgroups whose block pair fits one CU (<= 32 processors, LDS): fewer, larger steps per sweep
    np = 2;
    while (np < 128 && (width(np) > jmc_max_b || k::jmc_lds_bytes(nc, width(np), esz, k::kJmcLanes) > k::kLdsMaxBytes)) ++np;
  }
  const int b = width(np);
  if (np < 1 || b < 2 || b > 32 || k::jmc_lds_bytes(nc, b, esz, k::kJmcLanes) > k::kLdsMaxBytes) return false;
  *nc_out = nc;
  *np_out = np;
  *b_out = b;
  return true;
}

enum class CoreSvd {
  kRing,     // single workgroup, W in registers (jacobi_ring_w_kernel) + V replayed from the rotations (one launch each)
  kMultiWg,  // multi-workgroup block Jacobi (jacobi_mc_kernels.hpp)
  kBlock,    // block Jacobi, one launch per round (jacobi_block_round_kernel), any l <= 1024
  kHost,     // f64 Jacobi on the host (small_linalg.hpp)
};
// Every knob of the stage.  The backend fills one from the environment at the start of each small_svd
// (core_svd_stage.hpp: knobs_from_env); the defaults here are what an empty environment gives.
struct CoreSvdKnobs {
  const char* mode = nullptr;  // CORRLA_SVD: mc | lds (= the single-workgroup kernel) | block | host; nullptr = by size
  bool host_svd = false;       // CORRLA_HOST_SVD
  int jmc_min_l = 96;          // CORRLA_JMC_MIN_L: smallest l the default gives to the multi-workgroup kernel (below, the
                               // ring kernel + replay is as fast: one launch)
  int jmc_max_b = 24;          // CORRLA_JMC_MAX_B, clamped to [2, 32]
  int jmc_local = 1;           // CORRLA_JMC_LOCAL: 1: wave-local sub-block schedule (jacobi_mc_kernels.hpp), 0: ring schedule
  int jmc_np = 0;              // CORRLA_JMC_NP
  int jmc_sweeps_f32 = 10, jmc_sweeps_f64 = 13;  // CORRLA_JMC_SWEEPS (one value sets both): sweeps of an optimistic call
  bool jmc_force_v = false;    // CORRLA_JMC_FORCE_V
  bool strict = false;         // CORRLA_JACOBI_STRICT: run to a sweep below tol (multi-workgroup and ring kernels)
  int block_sweeps = 12, ring_sweeps = 40;  // CORRLA_JACOBI_SWEEPS (one value sets both)
  int block_inner = 1;         // CORRLA_JACOBI_INNER
};
// What a context has learnt from its earlier calls (HipDev owns one; sharded calls agree on it in their handshake).
struct CoreSvdState {
  int sweeps_hint = 0;   // sweeps the last converged multi-workgroup SVD used; 0: none yet
  int extra_sweeps = 0;  // enqueued on top of the default after a call that did not converge
  bool force_v = false;  // the W-only shortcut failed its verification once: accumulate V
};

// The whole launch.  tol / tol_early / floor2 are doubles; the launchers cast them to the element type.
struct CoreSvdPlan {
  CoreSvd family = CoreSvd::kHost;
  int ring_e = 0;  // kRing: rows per lane (the E of jacobi_ring_w_kernel<T, E, 8>); 0 otherwise
  double tol = 0;        // sqrt(l) eps: a pair below it is orthogonal
  // The iteration ends with the sweep in which no pair exceeded sqrt(eps) (quadratic convergence).  Clustered
  // singular values do not converge quadratically: the W / sigma factor of a 1.25e6 x 512 Gaussian sketch came out
  // orthonormal to 6e-5 only.  Running to a sweep without any rotation (strict: tol_early = tol) costs two more
  // sweeps; the driver instead re-orthonormalises that factor with one Cholesky-QR pass (a first-order
  // (I + E)^-1/2 here), which is cheaper.  The block kernel has no strict mode.
  double tol_early = 0;
  double floor2 = 0;     // l eps^2: squared norm of a numerically zero column (see jmc_step_kernel)
  struct MultiWg {
    int nc, np, b;       // jmc_geometry
    int local;           // schedule (CoreSvdKnobs::jmc_local)
    int rp;              // column pitch, global = LDS: a block of b columns is one contiguous byte range in both
    int nblocks, ncols_pad;
    unsigned step_threads;
    size_t step_lds;
    size_t ws_bytes;     // W, and as much again for V
    size_t fin_lds;
    unsigned other_grid; // jmc_other_factor_kernel: 16 lanes per entry of the l x k factor, 256 threads
    // optimistic calls may use the W-only mode when the core is well conditioned; the host-controlled repeat always
    // accumulates V
    int force_v;
    int nsw;             // sweeps an optimistic call enqueues
    int group, max_sweeps;  // host-controlled: sweeps between two looks at the convergence words, and their cap
  } mc = {};
  struct Block {
    int nb;              // even number of 8-column blocks
    int cols_pad, rows_pad;
    size_t ws_bytes;     // W, and as much again for V
    size_t round_lds;
    int max_sweeps, inner;
    size_t fin_lds;
  } blk = {};
  struct Ring {
    unsigned block;      // 8 lanes per processor; a partial last wave: no idle processors, no LDS slots for them
    size_t lds;
    int max_sw;
    size_t rot_bytes, rank_bytes;
    unsigned replay_grid;
  } ring = {};
};

// Default: the ring kernel below jmc_min_l (one launch, as fast there), the multi-workgroup kernel up to l = 288, the
// block kernel up to 1024, the host beyond.  The ring kernel needs a column pair per processor (l >= 2) and its W in
// LDS (l <= 144 f32, 138 f64); l = 1 and the widths it cannot take go to the block kernel.  Any CORRLA_SVD value other
// than mc / block / host selects the single-workgroup kernel.
// k: columns of the factors wanted.  optimistic: the call enqueues a fixed number of sweeps and reads a status record at
// its end; otherwise the host waits for groups of sweeps until the iteration has converged.
inline CoreSvdPlan core_svd_plan(int esz, int64_t l, int64_t k, const CoreSvdKnobs& kn, const CoreSvdState& st, bool optimistic) {
  auto is = [&](const char* m) { return kn.mode && std::strcmp(kn.mode, m) == 0; };
  CoreSvdPlan p;
  CoreSvdPlan::MultiWg& g = p.mc;
  const int e = k::jacobi_ring_e(l, esz);
  if ((!kn.mode || is("mc")) && !kn.host_svd && (is("mc") || l >= kn.jmc_min_l) &&
      jmc_geometry(l, esz, kn.jmc_max_b, kn.jmc_local, kn.jmc_np, &g.nc, &g.np, &g.b))
    p.family = CoreSvd::kMultiWg;
  else if (kn.host_svd || is("host") || l > 1024)
    return p;
  else if (!is("block") && l >= 2 && l <= 144 && k::jacobi_ring_w_lds_bytes((int)l, 8 * e, (size_t)esz) <= k::kLdsMaxBytes)
    p.family = CoreSvd::kRing;
  else
    p.family = CoreSvd::kBlock;

  const double eps = esz == 4 ? (double)std::numeric_limits<float>::epsilon() : std::numeric_limits<double>::epsilon();
  p.tol = std::sqrt((double)l) * eps;
  p.tol_early = kn.strict && p.family != CoreSvd::kBlock ? p.tol : std::sqrt(eps);
  p.floor2 = (double)l * eps * eps;
  switch (p.family) {
    case CoreSvd::kMultiWg: {
      g.local = kn.jmc_local;
      g.rp = k::jmc_pitch(g.nc, esz, k::kJmcLanes);
      g.nblocks = 2 * g.np;
      g.ncols_pad = g.nblocks * g.b;
      g.step_threads = (unsigned)((g.b * k::kJmcLanes + 63) / 64 * 64);
      g.step_lds = k::jmc_lds_bytes(g.nc, g.b, esz, k::kJmcLanes);
      g.ws_bytes = (size_t)g.rp * g.ncols_pad * esz;
      g.fin_lds = k::jacobi_finish_lds_bytes((int)l, (size_t)esz);
      g.other_grid = ((unsigned)(l * k) * 16 + 255) / 256;
      g.force_v = (!optimistic || st.force_v || kn.jmc_force_v) ? 1 : 0;
      // two more than the last converged call used instead of the default (the sweeps enqueued beyond convergence are
      // launches that only test a flag: 15 x 4.6 us at C2)
      const int nsw_default = std::max(1, esz == 4 ? kn.jmc_sweeps_f32 : kn.jmc_sweeps_f64);
      g.nsw = std::min(k::kJmcMaxSweeps, (st.sweeps_hint > 0 ? std::min(nsw_default, st.sweeps_hint + 2) : nsw_default) + st.extra_sweeps);
      g.group = 8;
      g.max_sweeps = k::kJmcMaxSweeps;
      break;
    }
    case CoreSvd::kBlock: {
      CoreSvdPlan::Block& b = p.blk;
      b.nb = (int)(2 * ((l + 15) / 16));
      b.cols_pad = b.nb * 8;
      b.rows_pad = (int)((l + 15) / 16 * 16);
      b.ws_bytes = (size_t)b.rows_pad * b.cols_pad * esz;
      b.round_lds = k::jacobi_block_round_lds_bytes(b.rows_pad, (size_t)esz);
      b.max_sweeps = kn.block_sweeps;
      b.inner = kn.block_inner;
      b.fin_lds = k::jacobi_finish_lds_bytes((int)l, (size_t)esz);
      break;
    }
    case CoreSvd::kRing: {
      CoreSvdPlan::Ring& r = p.ring;
      const int np = (int)((l + 1) / 2), n2 = 2 * np;
      p.ring_e = e;
      r.block = (unsigned)(np * 8);
      r.lds = k::jacobi_ring_w_lds_bytes((int)l, 8 * e, (size_t)esz);
      r.max_sw = kn.ring_sweeps;
      r.rot_bytes = (size_t)r.max_sw * n2 * k::kRingProcPad * (2 * (size_t)esz);  // RotEntry<T>: cs, sn
      r.rank_bytes = sizeof(int) * (size_t)n2;
      r.replay_grid = (unsigned)((l + 256 / k::kReplayLanes - 1) / (256 / k::kReplayLanes));
      break;
    }
    case CoreSvd::kHost: break;
  }
  return p;
}
// The choice alone (family, ring E), which depends on neither k, the context's state nor the kind of call.
inline CoreSvdPlan core_svd_plan(int esz, int64_t l, const CoreSvdKnobs& kn) { return core_svd_plan(esz, l, l, kn, CoreSvdState{}, true); }

}  // namespace corrla
