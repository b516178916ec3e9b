// Constrained Dirichlet sampling on the device (constr_dirichlet_sample, space_samplers.rs:14-126): a counter-based stream of
// Dirichlet draws, the box test as a bitmask, and the regeneration of the accepted draws.  All f64.  The geometry is
// dirichlet_plan.hpp's; this comment defines the stream, and tests/dirichlet_reference.py restates it from this text.
//
// THE STREAM.  Draw t (0 <= t < 2^62) of a call (seed, alpha[0..d), c_scale) is the row x[0..d).
//   Random numbers.  U(t, j, a, p) = (u1, u2) are the two uniforms of ONE Philox4x32-10 block (philox_uniform_pair,
//   hip_kernels.hpp) with key (seed mod 2^32, seed >> 32) and counter
//       c0 = t mod 2^32,  c1 = t >> 32,  c2 = j + 65536 p,  c3 = a
//   for component j (< 128), attempt a, purpose p: 0 = the normal of an attempt, 1 = the uniform of its acceptance test,
//   2 = the component's own uniform (a = 0).  u1 = (((w0 << 32 | w1) >> 11) + 0.5) 2^-53 from the output words w0, w1 and
//   u2 likewise from w2, w3: both are > 0, and < 1 but for the one pattern of 53 ones, whose sum rounds to 2^53 (u = 1;
//   every formula below is finite there).
//   Gamma g_j ~ Gamma(alpha_j, 1), the method chosen by alpha_j alone (DirComp, dirichlet_plan.hpp):
//     alpha_j = 1   g = -log(u1),  (u1, .) = U(t, j, 0, 2).
//     alpha_j > 1   Marsaglia-Tsang at shape s = alpha_j:  D = s - 1/3,  C = 1 / sqrt(9 D)  (host, IEEE double).
//                   For attempt a = 0, 1, ...:
//                     (u1, u2) = U(t, j, a, 0);  z = sqrt(-2 log(u1)) * cospi(2 u2)
//                     w = 1 + C z;  if w <= 0 the attempt is rejected
//                     v = (w w) w;  (q, .) = U(t, j, a, 1);  z2 = z z
//                     accept if  q < 1 - 0.0331 (z2 z2)                                 (the squeeze)
//                     else accept if  log(q) < 0.5 z2 + D ((1 - v) + log(v))
//                   g = D v of the first accepted attempt.  After kDirMaxAttempts = 64 rejected attempts (an attempt is
//                   rejected with probability below 0.05, so this has probability below 1e-83) g = D.
//     alpha_j < 1   the same at shape s = alpha_j + 1, then g = (D v) * pow(u1, 1 / alpha_j),  (u1, .) = U(t, j, 0, 2).
//   Row.  S = ((g_0 + g_1) + g_2) + ... in index order;  x_j = (c_scale g_j) / S.
//   Every operation above is one IEEE double operation rounded once, in the order written (contraction is off in this file:
//   no FMA is formed); log, sqrt, cospi and pow are the device library's.  A draw depends on nothing else -- not on the launch
//   geometry, the chunk size, or which other draws the call makes -- and the register and the regenerate routes run the same
//   operations, so they give the same bits.
//
// THE KERNELS.
//   dir_draw_kernel<DP, EXP>   thread i writes draw first + i to row i.
//   dir_test_kernel<DP, EXP>   workgroup w of a launch is workgroup gw = gw0 + w of the call: range k = gw mod wps of shot
//                              s = gw / wps, the draws s chunk + k R + [0, min(R, chunk - k R)).  Thread `tid` takes the
//                              draws i 256 + tid (i < 4) of the range, so the ballot of wave `wv` in round i is word 4 i + wv
//                              of the workgroup's 16.  The comparison lb_j <= x_j <= ub_j (closed, space_samplers.rs:42) is
//                              made on the very value EMIT stores.  Lane 0 of a wave writes the word; thread 0 the count.
//                              When the "enough" word is set the workgroup writes count 0 and returns.
//   dir_scan_kernel            one block: prefix[w] = total + the counts before w, total += the counts of the launch; once
//                              total >= n_samples it sets "enough" and records the gw whose count completed n_samples.
//   dir_emit_kernel<EXP>       thread per word; rank of a set bit = prefix[w] + the set bits before it in the workgroup; a bit
//                              of rank < n_samples has its draw regenerated (regenerate route: at most n_samples draws) into
//                              row `rank`.  So the rows are the first n_samples accepted draws in increasing draw index.
//   DP is the padded width of the register route (the gammas of a row in DP registers), DP = 0 the regenerate route: a first
//   sweep forms S, a second regenerates each g_j from its counter -- in TEST only up to the first component outside its bounds.  EXP: every alpha is 1, the Marsaglia-Tsang code is not
//   compiled in.  No atomics; every global access is guarded by the draw count, the workgroup count or n_samples.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dirichlet_plan.hpp"

namespace corrla {
namespace k {

constexpr uint32_t kDirNormal = 0u, kDirAccept = 1u, kDirOwn = 2u;  // the purposes of a Philox block

__device__ __forceinline__ void dir_uniforms(uint64_t t, int j, uint32_t attempt, uint32_t purpose, uint64_t seed, double& u1, double& u2) {
  philox_uniform_pair((uint32_t)t, (uint32_t)(t >> 32), (uint32_t)j + 65536u * purpose, attempt, seed, u1, u2);
}

template <bool EXP>
__device__ __forceinline__ double dir_gamma(uint64_t t, int j, uint64_t seed, const DirComp* __restrict__ tab) {
#pragma clang fp contract(off)
  double u1, u2;
  if (EXP || tab[j].method == (int)DirMethod::kExp) {
    dir_uniforms(t, j, 0u, kDirOwn, seed, u1, u2);
    return -log(u1);
  }
  const double D = tab[j].d_mt, C = tab[j].c_mt;
  double g = D;
  for (uint32_t a = 0; a < (uint32_t)kDirMaxAttempts; ++a) {
    dir_uniforms(t, j, a, kDirNormal, seed, u1, u2);
    const double z = box_muller_f64(u1, u2);
    const double w = 1.0 + C * z;
    if (w <= 0.0) continue;
    const double v = (w * w) * w;
    double q, unused;
    dir_uniforms(t, j, a, kDirAccept, seed, q, unused);
    const double z2 = z * z;
    bool acc = q < 1.0 - 0.0331 * (z2 * z2);
    if (!acc) acc = log(q) < 0.5 * z2 + D * ((1.0 - v) + log(v));
    if (acc) {
      g = D * v;
      break;
    }
  }
  if (tab[j].method == (int)DirMethod::kBoost) {
    dir_uniforms(t, j, 0u, kDirOwn, seed, u1, u2);
    g = g * pow(u1, tab[j].inv_alpha);
  }
  return g;
}

// the row of draw t: f(j, x_j) for j = 0 .. d - 1 in order, until f returns false (TEST stops at the first component outside
// its bounds: on the regenerate route the gammas behind it are then not drawn a second time)
template <int DP, bool EXP, class F>
__device__ __forceinline__ void dir_row(uint64_t t, int d, uint64_t seed, double c_scale, const DirComp* __restrict__ tab, F&& f) {
#pragma clang fp contract(off)
  if constexpr (DP > 0) {
    double g[DP];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < DP; ++j)
      if (j < d) {
        g[j] = dir_gamma<EXP>(t, j, seed, tab);
        s = j == 0 ? g[j] : s + g[j];
      }
#pragma unroll
    for (int j = 0; j < DP; ++j)
      if (j < d)
        if (!f(j, (c_scale * g[j]) / s)) return;
  } else {
    double s = dir_gamma<EXP>(t, 0, seed, tab);
    for (int j = 1; j < d; ++j) s = s + dir_gamma<EXP>(t, j, seed, tab);
    for (int j = 0; j < d; ++j)
      if (!f(j, (c_scale * dir_gamma<EXP>(t, j, seed, tab)) / s)) return;
  }
}

struct DirStream {
  const DirComp* tab;  // d records on the device
  int d;
  uint64_t seed;
  double c_scale;
};

struct DirDrawArgs {
  DirStream st;
  int64_t first, n;
  double* out;  // n x d, row stride ldo
  int64_t ldo;
};

template <int DP, bool EXP>
__global__ __launch_bounds__(kDirThreads) void dir_draw_kernel(DirDrawArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kDirThreads + threadIdx.x;
  if (i >= a.n) return;
  double* row = a.out + i * a.ldo;
  dir_row<DP, EXP>((uint64_t)(a.first + i), a.st.d, a.st.seed, a.st.c_scale, a.st.tab, [&](int j, double x) {
    row[j] = x;
    return true;
  });
}

// the running state of a sampling call, zeroed at its start
struct DirState {
  unsigned long long total;  // accepted draws of the launches scanned so far
  long long cross_gw;        // the workgroup whose count completed n_samples (valid once enough != 0)
  unsigned int enough;
  unsigned int pad;
};

struct DirTestArgs {
  DirStream st;
  int64_t gw0, n_wgs;   // the launch serves the workgroups [gw0, gw0 + n_wgs) of the call
  int64_t wps, chunk;
  const DirState* state;
  unsigned long long* mask;  // [n_wgs][kDirWords]
  unsigned int* count;       // [n_wgs]
};

template <int DP, bool EXP>
__global__ __launch_bounds__(kDirThreads) void dir_test_kernel(DirTestArgs a) {
  __shared__ unsigned int wave_count[kDirThreads / 64];
  const int64_t w = blockIdx.x;  // the grid is exactly n_wgs
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  if (a.state->enough) {  // uniform over the grid's later launches: nothing of this workgroup is read when its count is 0
    if (tid == 0) a.count[w] = 0u;
    return;
  }
  const int64_t gw = a.gw0 + w;
  const int64_t shot = gw / a.wps, kr = gw - shot * a.wps;
  const int64_t in_shot = kr * kDirRange;  // < chunk: the range is not empty
  const int64_t live = a.chunk - in_shot < (int64_t)kDirRange ? a.chunk - in_shot : (int64_t)kDirRange;
  const uint64_t t0 = (uint64_t)(shot * a.chunk + in_shot);
  unsigned int mine = 0u;
#pragma unroll 1
  for (int i = 0; i < kDirDPT; ++i) {
    const int e = i * kDirThreads + tid;
    bool ok = e < live;
    if (ok)
      dir_row<DP, EXP>(t0 + (uint64_t)e, a.st.d, a.st.seed, a.st.c_scale, a.st.tab,
                       [&](int j, double x) { return ok = (a.st.tab[j].lb <= x) && (x <= a.st.tab[j].ub); });
    const unsigned long long word = __ballot(ok);
    if (lane == 0) {
      a.mask[w * kDirWords + i * (kDirThreads / 64) + wv] = word;
      mine += (unsigned int)__popcll(word);
    }
  }
  if (lane == 0) wave_count[wv] = mine;
  __syncthreads();
  if (tid == 0) a.count[w] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
}

struct DirScanArgs {
  const unsigned int* count;   // [n_wgs]
  unsigned long long* prefix;  // [n_wgs]
  int64_t gw0, n_wgs;
  int64_t n_samples;
  DirState* state;
};

// One block of kDirScanThreads: thread q owns the counts [q per, (q + 1) per), per = ceil(n_wgs / 256); the thread sums, the
// block scans the 256 sums in LDS, the thread writes its prefixes.
__global__ __launch_bounds__(kDirScanThreads) void dir_scan_kernel(DirScanArgs a) {
  __shared__ unsigned long long sums[kDirScanThreads];
  const int tid = threadIdx.x;
  const unsigned long long base = a.state->total;
  const int64_t per = (a.n_wgs + kDirScanThreads - 1) / kDirScanThreads;
  const int64_t lo = tid * per < a.n_wgs ? tid * per : a.n_wgs, hi = lo + per < a.n_wgs ? lo + per : a.n_wgs;
  unsigned long long s = 0ull;
  for (int64_t w = lo; w < hi; ++w) s += a.count[w];
  sums[tid] = s;
  __syncthreads();
  if (tid == 0) {
    unsigned long long run = 0ull;
    for (int q = 0; q < kDirScanThreads; ++q) {
      const unsigned long long v = sums[q];
      sums[q] = run;
      run += v;
    }
    // every thread has read `base` before the barrier above; the new total is visible to the next launch in stream order
    a.state->total = base + run;
    if (base < (unsigned long long)a.n_samples && base + run >= (unsigned long long)a.n_samples) a.state->enough = 1u;
  }
  __syncthreads();
  unsigned long long run = base + sums[tid];
  for (int64_t w = lo; w < hi; ++w) {
    const unsigned long long c = a.count[w];
    a.prefix[w] = run;
    if (run < (unsigned long long)a.n_samples && run + c >= (unsigned long long)a.n_samples) a.state->cross_gw = a.gw0 + w;
    run += c;
  }
}

struct DirEmitArgs {
  DirStream st;
  int64_t gw0, n_wgs, wps, chunk;
  const unsigned long long* mask;
  const unsigned int* count;
  const unsigned long long* prefix;
  int64_t n_samples;
  double* out;  // n_samples x d, row stride ldo
  int64_t ldo;
};

template <bool EXP>
__global__ __launch_bounds__(kDirThreads) void dir_emit_kernel(DirEmitArgs a) {
  const int64_t wi = (int64_t)blockIdx.x * kDirThreads + threadIdx.x;  // word of the launch
  const int64_t w = wi / kDirWords;
  const int q = (int)(wi - w * kDirWords);
  if (w >= a.n_wgs) return;
  if (a.count[w] == 0u) return;  // also: a workgroup that returned at the "enough" word wrote no bits
  unsigned long long rank = a.prefix[w];
  if (rank >= (unsigned long long)a.n_samples) return;
  const unsigned long long* words = a.mask + w * kDirWords;
  for (int p = 0; p < q; ++p) rank += (unsigned long long)__popcll(words[p]);
  unsigned long long m = words[q];
  const int64_t gw = a.gw0 + w;
  const int64_t shot = gw / a.wps, kr = gw - shot * a.wps;
  const uint64_t t0 = (uint64_t)(shot * a.chunk + kr * kDirRange + q * 64);
  while (m != 0ull && rank < (unsigned long long)a.n_samples) {
    const int b = __ffsll((long long)m) - 1;
    m &= m - 1ull;
    double* row = a.out + (int64_t)rank * a.ldo;
    dir_row<0, EXP>(t0 + (uint64_t)b, a.st.d, a.st.seed, a.st.c_scale, a.st.tab, [&](int j, double x) {
    row[j] = x;
    return true;
  });
    ++rank;
  }
}

}  // namespace k
}  // namespace corrla
