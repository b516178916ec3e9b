// Which kernel family takes the SVD of the l x l core (random_svd.rs:89), and the LDS arithmetic that choice rests on.
// Host code only, no HIP call: tests/test_core_svd_plan.py compiles this header with the host compiler and pins the
// choice at every l.  The kernels that use the size helpers on the device include it through jacobi_mc_kernels.hpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

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

// ---- single-workgroup ring Jacobi (jacobi_ring_w_kernel, hip_kernels.hpp) ----
// rs = G * E: rows per column slot
CORRLA_HD inline size_t jacobi_ring_w_lds_bytes(int l, int rs, size_t esz) {
  const int n2 = (l + 1) & ~1;
  const int nproc = n2 / 2;  // launched with exactly G * np threads
  return (size_t)2 * nproc * rs * esz + (size_t)n2 * (esz + sizeof(int)) + (size_t)2 * nproc * esz + 64;
}
// rows per lane of the ring kernel's column slots (8 lanes per processor); l <= 144
inline int jacobi_ring_e(int64_t l, int esz) { return l <= 64 ? 8 : (l <= 96 ? 12 : (l <= 128 ? 16 : (esz == 4 ? 20 : 18))); }

}  // namespace k

// Geometry of the multi-workgroup block Jacobi for an l x l core: chunk rows NC, workgroups NP, block width b (a
// multiple of four, <= 32); false when it does not fit.  local: CORRLA_JMC_LOCAL (0 keeps the round-2 rule: even
// widths), np_force: CORRLA_JMC_NP (0: the fewest workgroups whose block pair fits one CU and jmc_max_b).
inline bool jmc_geometry(int64_t l, int esz, int lanes, int jmc_max_b, int local, int np_force, int* nc_out, int* np_out,
                         int* b_out) {
  if (l < 2 || l > 288) return false;
  const int nc = (int)((l + 2 * lanes - 1) / (2 * lanes));
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
    while (np < 128 && (width(np) > jmc_max_b || k::jmc_lds_bytes(nc, width(np), esz, lanes) > k::kLdsMaxBytes)) ++np;
  }
  const int b = width(np);
  if (np < 1 || b < 2 || b > 32 || k::jmc_lds_bytes(nc, b, esz, lanes) > k::kLdsMaxBytes) return false;
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
struct CoreSvdPlan {
  CoreSvd family;
  int ring_e;  // kRing: rows per lane (the E of jacobi_ring_w_kernel<T, E, 8>); 0 otherwise
};
struct CoreSvdKnobs {
  const char* mode = nullptr;  // CORRLA_SVD: mc | lds (= the single-workgroup kernel) | block | host; nullptr = by size
  bool host_svd = false;       // CORRLA_HOST_SVD
  int jmc_min_l = 96;          // CORRLA_JMC_MIN_L: smallest l the default gives to the multi-workgroup kernel
  int jmc_max_b = 24;          // CORRLA_JMC_MAX_B
  int jmc_local = 1;           // CORRLA_JMC_LOCAL
  int jmc_np = 0;              // CORRLA_JMC_NP
};

// Default: the ring kernel below jmc_min_l (one launch, as fast there), the multi-workgroup kernel up to l = 288, the
// block kernel up to 1024, the host beyond.  The ring kernel needs a column pair per processor (l >= 2) and its W in
// LDS (l <= 144 f32, 138 f64); l = 1 and the widths it cannot take go to the block kernel.  Any CORRLA_SVD value other
// than mc / block / host selects the single-workgroup kernel.
inline CoreSvdPlan core_svd_plan(int esz, int64_t l, const CoreSvdKnobs& kn) {
  auto is = [&](const char* m) { return kn.mode && std::strcmp(kn.mode, m) == 0; };
  int nc, np, b;
  if ((!kn.mode || is("mc")) && !kn.host_svd && (is("mc") || l >= kn.jmc_min_l) &&
      jmc_geometry(l, esz, 16, kn.jmc_max_b, kn.jmc_local, kn.jmc_np, &nc, &np, &b))
    return {CoreSvd::kMultiWg, 0};
  if (kn.host_svd || is("host") || l > 1024) return {CoreSvd::kHost, 0};
  if (is("block")) return {CoreSvd::kBlock, 0};
  const int e = k::jacobi_ring_e(l, esz);
  if (l >= 2 && l <= 144 && k::jacobi_ring_w_lds_bytes((int)l, 8 * e, (size_t)esz) <= k::kLdsMaxBytes)
    return {CoreSvd::kRing, e};
  return {CoreSvd::kBlock, 0};
}

}  // namespace corrla
