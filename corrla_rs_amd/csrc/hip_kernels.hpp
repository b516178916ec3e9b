// gfx950 (MI355X / CDNA4) kernels of the RSVD hot path.  Written for wave64 + MFMA directly; no
// portability layer.
//
// Two GEMM kernels carry every m- or n-sized product of random_svd.rs:15-110:
//
//   gemm_nn :  Out (M x L, col-major) = R (M x K, row-major, streamed once) * X (K x L, col-major)
//   gemm_tn :  Out (K x L, col-major) = R^T * X,  R (M x K row-major, streamed once), X (M x L col-major)
//
// R is the big operand (A, or A^T's memory when A is column-major); X/Out are "skinny" matrices
// (L = rank + oversamples, padded to 16-column MFMA tiles) kept column-major with zero padding.
// With those two, A*Omega / A*Z (random_svd.rs:31,47-51), A^T*Y (:42-46), B^T = A^T*Q (:80), the
// Gram matrices of the orthonormalisation (:38,57) and U = Q*U~ (:92) are all covered for both
// memory layouts of A (see driver.hpp).
//
// MFMA: v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64.  Each workgroup = 4 waves (one per
// SIMD); wave w owns 16 consecutive "outer" indices (rows of R for nn, columns of R for tn) and
// ALL NT 16-column tiles of the skinny operand, so R is read from HBM exactly once per column
// block.  The accumulator tile is D[l-index][outer-index] (skinny operand on the MFMA A side),
// which makes the epilogue stores contiguous along the column-major output.
//
// LDS: both operands are staged by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction)
// into double-buffered images of 256-byte rows (64 f32 / 32 f64 along the reduction index), so
// every fragment read is one ds_read_b128 feeding 4 (f32) / 2 (f64) MFMA k-steps.  The DMA writes
// LDS linearly, so the bank-conflict swizzle (16-byte slot ^= row & 15) is applied to the per-lane
// SOURCE address and again on the read (cdna_hip_programming.md rule 21).  Out-of-range lanes of
// the big operand read a 16-byte zero page instead of being masked, which gives exact zero fill
// on both the reduction tail and the outer tail.  The k index inside an MFMA is a dummy
// summation index, so lane group kq of k-step j is fed element 16g+4kq+j (f32) / 8g+2kq+j (f64)
// of the tile row for BOTH operands.
#pragma once
#include <hip/hip_runtime.h>

#include <limits>
#include <stdint.h>

#include <type_traits>

#include "gemm_plan.hpp"   // kLoaders, kRowBytes, the tile and LDS sizes
#include "thinq_plan.hpp"  // CholStatus (core_finite_check_kernel)

namespace corrla {
namespace k {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

#ifndef CORRLA_F32_BIG_IS_A
#define CORRLA_F32_BIG_IS_A true  // see MT<float>::kBigIsA
#endif
template <class T>
struct MT;
template <>
struct MT<float> {
  typedef f32x4 acc_t;
  typedef f32x4 vec_t;
  static constexpr int VEC = gemm_vec(4);  // elements per 16 bytes
  static constexpr int KT = gemm_kt(4);    // reduction elements per 256-byte LDS row
  // The tall GEMMs feed the BIG operand as MFMA A and the skinny one as B: a lane's four D registers are then four
  // consecutive OUTER indices of one result column, i.e. one 16-byte store (a quarter of the store instructions of
  // the other order; 10^7 x 80 results made the stores 10 % of the product's time).
  static constexpr bool kBigIsA = CORRLA_F32_BIG_IS_A;
  static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  // C/D layout of v_mfma_f32_16x16x4_f32: col = lane & 15, row = 4 * (lane >> 4) + reg
  static __device__ __forceinline__ int drow(int lane, int j) { return 4 * (lane >> 4) + j; }
  // tn-kernel big-operand tile: 64 reduction rows x 256 B; fragment rows of one 32-lane half are
  // 4 apart -> flip the 64-byte chunk bit
  static __device__ __forceinline__ int tswz(int row) { return ((row >> 2) & 1) << 2; }
};
template <>
struct MT<double> {
  typedef f64x4 acc_t;
  typedef f64x2 vec_t;
  static constexpr int VEC = gemm_vec(8);
  static constexpr int KT = gemm_kt(8);
  // f64 D registers are 4 rows apart: the skinny operand stays MFMA A, so that 16 lanes store 128 contiguous bytes
  static constexpr bool kBigIsA = false;
  static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
  static __device__ __forceinline__ int drow(int lane, int j) { return (lane >> 4) + 4 * j; }
  // tn-kernel big-operand tile: 32 reduction rows x 512 B; fragment rows of one half are 2 apart
  // -> flip the 128-byte chunk bit
  static __device__ __forceinline__ int tswz(int row) { return ((row >> 1) & 1) << 3; }
};

#ifndef CORRLA_PD
#define CORRLA_PD 4
#endif
#ifndef CORRLA_GEMM_DEFER
#define CORRLA_GEMM_DEFER 2  // pipeline steps whose MFMAs are issued after the next tile's barrier (0 = off)
#endif
constexpr int kPrefetchSteps = CORRLA_PD;  // LDS fragment reads run this many MFMA steps ahead
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit counter");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wg_barrier() { asm volatile("s_barrier" ::: "memory"); }

template <class T>
struct GemmArgs {
  const T* r;         // big operand, row-major
  int64_t r_rows, r_cols, r_ld, r_cols_readable;
  const T* x;         // skinny operand, column-major, zero padded
  int64_t x_ld;
  T* out;             // skinny result, column-major
  int64_t out_ld;
  int64_t out_cols;   // columns of `out` that may be written (the padded column count, or fewer for a caller's buffer)
  int64_t col_base;   // first column of this launch's column blocks (uneven column blockings take two launches)
  T* slab;            // partial results when nsplit > 1: slab[z][col][outer]
  int64_t slab_stride;
  const T* scale;     // optional device scalar applied to the result (nsplit == 1 only)
  const T* zero;      // >= 16 bytes of zeros
  int tiles_total;    // reduction tiles (of KT elements)
  int tiles_per_split;
  int nsplit;
  int debug_flags;    // timing-only ablation (wrong results): 1 = no DMA after the first tile
  const int* run_if;  // optional device word: the launch does nothing when it is 0 (conditional passes of the
                      // device-side Cholesky-QR, driver.hpp: orthonormalize_device)
  int vec_store;      // out (and the slabs) are 16-byte aligned with out_ld % 4 == 0
  int rotate;         // gemm_nn: workgroup x walks the reduction tiles from tile x mod (tiles per split), wrapping
  int outer_blocks;   // outer tiles in all; workgroup x of gridDim.x takes x, x + gridDim.x, ... (persistent launches of
                      // short reductions: the DMA ring runs on across the tile boundary, so only the first outer tile
                      // of a workgroup pays the fill latency)
  int xcd_remap;      // gemm_tn, gridDim.y == 1: the gridDim.x outer tiles of one reduction slab run on ONE XCD (see the
                      // kernel): they stream the same slab of the skinny operand, which then crosses the fabric once
};

__device__ __forceinline__ void glds16(const void* gsrc, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}


template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// A lean LDS-DMA stream for the loader wave: NVAR per-lane source pointers (one per variant of the
// repeating swizzle pattern), issued NQ times each with a uniform byte stride between repeats; per DMA
// the wave spends one 64-bit pointer add.  Chunk i = p + NVAR*q lands at lds + i KiB.
template <int NVAR, int NQ, int CS>
struct DmaStream {
  const char* ptr[NVAR];
  int64_t step;  // bytes between repeat q and q+1 of a variant
  int64_t adv;   // bytes per reduction tile
  // lds = address of this loader's first chunk; its chunks are CS KiB apart (CS = number of loader waves)
  __device__ __forceinline__ void issue(char* lds) {
    static_for<0, NQ>([&](auto iq) {
      static_for<0, NVAR>([&](auto ip) {
        constexpr int q = decltype(iq)::value, pv = decltype(ip)::value;
        glds16(ptr[pv], lds + CS * (pv + NVAR * q) * 1024);
        ptr[pv] += step;
      });
    });
    const int64_t back = adv - (int64_t)NQ * step;
#pragma unroll
    for (int pv = 0; pv < NVAR; ++pv) ptr[pv] += back;
  }
};

// ---- explicit LDS fragment pipeline (cdna_hip_programming.md 5.7) --------------------------------
// hipcc (ROCm 7.2) brackets every LDS fragment read of this loop with s_waitcnt lgkmcnt(0), which
// exposes the full LDS latency to the single wave per SIMD.  The fragment reads are therefore
// issued as inline-asm ds_read_* PD steps ahead of their MFMAs, and retired by hand-counted
// s_waitcnt lgkmcnt(N) statements that take the fragment as a "+v" operand: the data dependence
// keeps every consumer below its wait, and volatile asm keeps reads and waits in program order.
template <int OFF, class V>
__device__ __forceinline__ void lds_read_b128(V& d, unsigned addr) {
  static_assert(sizeof(V) == 16 && OFF >= 0 && OFF < 65536, "ds_read_b128 operand");
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_read_elem(float& d, unsigned addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds_read_b32 offset");
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_read_elem(double& d, unsigned addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds_read_b64 offset");
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF) : "memory");
}
template <int N, class V>
__device__ __forceinline__ void lds_wait(V& frag) {
  static_assert(N >= 0 && N <= 15, "lgkmcnt is a 4-bit counter");
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(frag) : "n"(N) : "memory");
}
template <class V>
__device__ __forceinline__ void lds_tie(V& frag) {  // frag was retired by an earlier (in-order) wait
  asm volatile("" : "+v"(frag));
}
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(uintptr_t)((const __attribute__((address_space(3))) char*)p);
}

// skinny-operand element x, big-operand element r of one k index -> acc (see MT<T>::kBigIsA)
template <class T>
__device__ __forceinline__ typename MT<T>::acc_t gemm_mma(T x, T r, typename MT<T>::acc_t c) {
  if constexpr (MT<T>::kBigIsA)
    return MT<T>::mma(r, x, c);
  else
    return MT<T>::mma(x, r, c);
}

template <class T, int NT>
__device__ __forceinline__ void store_tile(const GemmArgs<T>& g, const typename MT<T>::acc_t (&acc)[NT], int64_t outer0,
                                           int64_t outer_limit, int64_t col0, int lane, int slab_z = (int)blockIdx.z) {
  if (g.debug_flags & 8) return;  // timing-only ablation: no result stores
  T* dst;
  T sc = (T)1;
  if (g.nsplit > 1) {
    dst = g.slab + (int64_t)slab_z * g.slab_stride;
  } else {
    dst = g.out;
    if (g.scale) {
      sc = *g.scale;
      // retire the load HERE: the stores below sit in branches of their own, and hipcc, not knowing across blocks whether
      // `sc` has landed, put an s_waitcnt vmcnt(0) in front of every one of them -- which also waits for the store before
      asm volatile("" : "+v"(sc));
    }
  }
  if constexpr (MT<T>::kBigIsA) {
    // D: column = lane & 15 (result column), rows 4 (lane >> 4) + j (outer indices)
    const int64_t outer = outer0 + 4 * (lane >> 4);
    if (outer >= outer_limit) return;
    const bool whole = g.vec_store && outer + 3 < outer_limit;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int64_t col = col0 + 16 * t + (lane & 15);
      if (g.nsplit > 1 || col < g.out_cols) {
        T* p = dst + col * g.out_ld + outer;
        if (whole) {
          *(typename MT<T>::acc_t*)p = acc[t] * sc;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (outer + j < outer_limit) p[j] = acc[t][j] * sc;
        }
      }
    }
  } else {
    const int64_t outer = outer0 + (lane & 15);
    if (outer >= outer_limit) return;
    // f64: D register j of column tile t is result column col0 + 16 t + 4 j + (lane >> 4), i.e. the 4 NT stores of a lane are
    // 4 out_ld elements apart: ONE running pointer.  (With `dst[col * out_ld + outer]` hipcc computed the 36 addresses
    // ahead of the reduction loop and parked them in scratch; every store then sat behind a scratch reload and an
    // s_waitcnt vmcnt(0) that also waited for the STORE before it -- ~50 us per outer tile, a third of the short-reduction
    // products of the f64 thin-Q.)
    static_assert(sizeof(T) == 8, "the scalar-store epilogue is the f64 layout (drow = (lane >> 4) + 4 j)");
    const int64_t colb = col0 + (lane >> 4);
    T* p = dst + colb * g.out_ld + outer;
    const int64_t step = 4 * g.out_ld;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t col = colb + 16 * t + 4 * j;
        if (g.nsplit > 1 || col < g.out_cols) *p = acc[t][j] * sc;
        p += step;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// gemm_nn: grid = (ceil(R_rows/64), column blocks, nsplit)
// ---------------------------------------------------------------------------------------------
// ALIAS (Gram matrices, G = Y^T Y: the big operand's memory IS the skinny operand's, and the single outer tile
// holds every column): the skinny fragments are read from the big tile's LDS image -- same rows, same swizzle -- so
// the operand is staged ONCE per tile instead of twice (the Gram of a 10^7 x 80 sketch read Y twice: 6.4 GB).
// NW = MFMA waves per workgroup: 4 (one per SIMD) or 8 (two per SIMD, each with MW row tiles; the tile geometry is that of
// GW = MW * NW / 4 row tiles per SIMD).  Two f64 MFMA waves per SIMD reach 77.8 TF where one reaches 60.5
// (tools/microbench/mfma_chain.hip): the f64 products run <double, 1, NT, false, 8> on the 128-row tile of <double, 2, NT>.
template <class T, int MW, int NT, bool ALIAS = false, int NW = 4>
__global__ __launch_bounds__(64 * (NW + kLoaders)) void gemm_nn_kernel(GemmArgs<T> g) {
  constexpr int GW = MW * NW / 4;
  static_assert(NW == 4 || (NW == 8 && !ALIAS), "4 or 8 MFMA waves");
  typedef typename MT<T>::acc_t acc_t;
  typedef typename MT<T>::vec_t vec_t;
  constexpr int VEC = MT<T>::VEC;
  constexpr int KT = MT<T>::KT;
  constexpr int STAGE = ALIAS ? big_tile_bytes(GW) : stage_bytes(GW, NT);
  constexpr int BIG = big_tile_bytes(GW);
  static_assert(!ALIAS || 16 * NT <= 64 * GW, "alias: the outer tile must hold every column");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if (g.run_if && *g.run_if == 0) return;  // uniform over the grid
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row_first = (int64_t)blockIdx.x * outer_tile(GW);
  const int64_t col0 = g.col_base + (int64_t)blockIdx.y * (NT * 16);
  const int t_begin = blockIdx.z * g.tiles_per_split;
  const int t_end = min(t_begin + g.tiles_per_split, g.tiles_total);
  const int nk = t_end - t_begin;
  // outer tiles of this workgroup: blockIdx.x, blockIdx.x + gridDim.x, ... (one when the grid covers them all)
  const int nob = (g.outer_blocks - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  const int64_t ob_rows = (int64_t)gridDim.x * outer_tile(GW);

  // Waves 0..3 are MFMA waves; waves 4.. (kLoaders of them) are LOADER waves that only issue the LDS-DMA of the next tile
  // (a global_load_lds costs its issuing wave ~100 cycles, which an in-order MFMA wave cannot hide: with
  // the DMA issued from the MFMA waves this kernel lost 14 %).  Chunk c (1 KiB = 4 tile rows): lane
  // (r = lane >> 4, s = lane & 15) fills physical 16-byte slot s of row 4c + r with logical slot
  // s ^ (row & 15).
  if (wave >= NW) {
    __builtin_amdgcn_s_setprio(3);  // few instructions, but they gate everyone: win the issue arbitration
    // generic (bounds-checked) issue of one tile: used for edge tiles only
    int64_t row0 = row_first;  // outer tile being STAGED (runs ahead of the one being multiplied)
    auto stage_checked = [&](int buf, int kt) {
      char* rt = smem + buf * STAGE;
      const int64_t k0 = (int64_t)kt * KT;
      for (int c = wave - NW; c < (ALIAS ? 4 * NT : 16 * GW); c += kLoaders) {
        const int row = 4 * c + (lane >> 4);
        const int ls = (lane & 15) ^ (row & 15);
        const int64_t grow = row0 + row;
        const int64_t kk = k0 + ls * VEC;
        const T* src = (grow < g.r_rows && kk < g.r_cols_readable) ? g.r + grow * g.r_ld + kk : g.zero;
        glds16(src, rt + c * 1024);
      }
      if constexpr (!ALIAS)
        for (int c = wave - NW; c < 4 * NT; c += kLoaders) {
          const int row = 4 * c + (lane >> 4);
          const int ls = (lane & 15) ^ (row & 15);
          glds16(g.x + (col0 + row) * g.x_ld + k0 + ls * VEC, rt + BIG + c * 1024);
        }
    };
    // pattern streams: chunk c covers tile rows 4c..4c+3 and (row & 15) repeats every 4 chunks; loader lw
    // of NL owns chunks c = lw + NL*i, i.e. NV = 4/NL pattern variants, each repeating every 16 rows
    constexpr int NL = kLoaders, NV = 4 / NL;
    const int lw = wave - NW;
    // alias: only the 16 * NT rows that exist as (zero padded) columns of the sketch are staged; the rows above them
    // feed accumulators whose outer index is >= r_rows and is never stored
    DmaStream<NV, ALIAS ? NT : 4 * GW, NL> big;
    DmaStream<NV, NT, NL> sk;
    // rotated reduction order (g.rotate): workgroup x starts at tile x mod nk and wraps.  With a short row (n = 512:
    // 2 KB) every workgroup of a launch would otherwise sit on the same 256-byte phase of its rows at the same time,
    // i.e. on one eighth of the memory channels.
    const int rot = g.rotate ? (int)(blockIdx.x % (unsigned)nk) : 0;
#pragma unroll
    for (int pv = 0; pv < NV; ++pv) {
      const int row = 4 * (lw + NL * pv) + (lane >> 4);
      const int ls = (lane & 15) ^ (row & 15);
      big.ptr[pv] = (const char*)(g.r + (row0 + row) * g.r_ld + (int64_t)(t_begin + rot) * KT + ls * VEC);
      sk.ptr[pv] = (const char*)(g.x + (col0 + row) * g.x_ld + (int64_t)(t_begin + rot) * KT + ls * VEC);
    }
    big.step = 16 * g.r_ld * (int64_t)sizeof(T);
    big.adv = KT * (int64_t)sizeof(T);
    sk.step = 16 * g.x_ld * (int64_t)sizeof(T);
    sk.adv = KT * (int64_t)sizeof(T);
    // alias: the host guarantees 16 * NT allocated columns (x.cols_alloc), all of them readable
    bool rows_inside = ALIAS ? true : (row0 + outer_tile(GW) <= g.r_rows);
    auto stage_tile = [&](int buf, int kt) {
      char* rt = smem + buf * STAGE;
      if (rows_inside && (int64_t)(kt + 1) * KT <= g.r_cols_readable) {
        if (g.debug_flags & 6) {  // timing-only ablations: 2 = no skinny-operand DMA, 4 = no big-operand DMA
          if (!(g.debug_flags & 4)) big.issue(rt + lw * 1024);
          if constexpr (!ALIAS)
            if (!(g.debug_flags & 2)) sk.issue(rt + BIG + lw * 1024);
          return;
        }
        big.issue(rt + lw * 1024);
        if constexpr (!ALIAS) sk.issue(rt + BIG + lw * 1024);
      } else {
        stage_checked(buf, kt);
#pragma unroll
        for (int pv = 0; pv < NV; ++pv) {  // keep the streams in step with the tile counter
          big.ptr[pv] += big.adv;
          sk.ptr[pv] += sk.adv;
        }
      }
    };
    // ring of NSTAGE buffers: tiles i+1 .. i+NSTAGE-1 are in flight while the MFMA waves work on tile i
    constexpr int NSTAGE = ALIAS ? 3 : gemm_stages(GW, NT);
    static_assert((16 * GW) % kLoaders == 0 && (4 * NT) % kLoaders == 0, "chunks must split evenly over the loaders");
    constexpr int DPL = ALIAS ? NT : (16 * GW + 4 * NT) / kLoaders;  // DMA instructions per loader wave per tile
    // the tiles of all outer tiles of this workgroup form ONE sequence through the ring
    const int nflat = nob * nk;
    const int64_t wrap = -(int64_t)nk * KT * (int64_t)sizeof(T);  // back to the first tile of the reduction range
    const int64_t big_jump = ob_rows * g.r_ld * (int64_t)sizeof(T);
    int s_k = rot, s_n = 0;
    auto stage_next = [&](int buf) {
      stage_tile(buf, t_begin + s_k);
      if (++s_k == nk) {
        s_k = 0;
#pragma unroll
        for (int pv = 0; pv < NV; ++pv) {
          big.ptr[pv] += wrap;
          sk.ptr[pv] += wrap;
        }
      }
      if (++s_n == nk) {  // on to the next outer tile (the streams are back at tile `rot`)
        s_n = 0;
        row0 += ob_rows;
#pragma unroll
        for (int pv = 0; pv < NV; ++pv) big.ptr[pv] += big_jump;
        if constexpr (!ALIAS) rows_inside = row0 + outer_tile(GW) <= g.r_rows;
      }
    };
    for (int t = 0; t < NSTAGE - 1 && t < nflat; ++t) stage_next(t % NSTAGE);
    for (int i = 0; i < nflat; ++i) {
      // tile i must have landed; the (NSTAGE-2) younger tiles may stay in flight (vmcnt counts in issue order)
      if (NSTAGE > 2 && i + NSTAGE - 2 < nflat) {
        if (g.debug_flags & 2)
          wait_vmcnt<(NSTAGE - 2) * (16 * GW / kLoaders)>();
        else if (g.debug_flags & 4)
          wait_vmcnt<(NSTAGE - 2) * (4 * NT / kLoaders)>();
        else
          wait_vmcnt<(NSTAGE - 2) * DPL>();
      } else {
        wait_vmcnt<0>();
      }
      wg_barrier();  // tile i visible to the MFMA waves; they are done reading buffer (i-1) % NSTAGE
      if (i + NSTAGE - 1 < nflat && !(g.debug_flags & 1)) stage_next((i + NSTAGE - 1) % NSTAGE);
    }
    return;
  }

  acc_t acc[MW][NT];
  // Fragment read addresses (bytes inside a stage), lane-invariant across tiles: for fragment group
  // gq this lane reads 16-byte slot (4*gq + kq) ^ c of its row in both images.
  const int fc = lane & 15, fkq = lane >> 4;
  const unsigned lds0 = lds_addr(smem);
  unsigned a_off[4], b_off[4];
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) {
    const unsigned so = (unsigned)(((4 * gq + fkq) ^ fc) << 4);
    a_off[gq] = lds0 + (ALIAS ? 0 : BIG) + fc * kRowBytes + so;  // alias: column c of the sketch = row c of the big tile
    b_off[gq] = lds0 + (16 * MW * wave + fc) * kRowBytes + so;
  }

  // Step st = gq*NT + t consumes one skinny fragment a(st) and the MW big-operand fragments b(gq) in
  // MW*VEC MFMAs.  Reads for step st+PD are issued before the MFMAs of step st; the wait for step
  // st leaves exactly the younger reads (steps st+1..st+PD) in flight.
  // The MFMAs of the last kDefer steps of a tile are issued AFTER the next tile's barrier and first fragment reads:
  // their operands are already in registers, so they fill the bubble (barrier -> LDS latency -> first MFMA) that
  // every tile otherwise pays.
  constexpr int NS = 4 * NT;
  constexpr int PD = kPrefetchSteps;
  constexpr int kDefer = (NT >= 2 && NS - CORRLA_GEMM_DEFER >= PD) ? (CORRLA_GEMM_DEFER < NT ? CORRLA_GEMM_DEFER : NT) : 0;
  vec_t afr[NS];
  vec_t bfr[4][MW];
  auto mfma_step = [&](auto ic) {
    constexpr int st = decltype(ic)::value;
    constexpr int gq = st / NT, t = st % NT;
#pragma unroll
    for (int mw = 0; mw < MW; ++mw)
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[mw][t] = gemm_mma<T>(afr[st][j], bfr[gq][mw][j], acc[mw][t]);
  };
  auto compute = [&](int buf, bool have_prev) {
    const unsigned sb = (unsigned)(buf * STAGE);
    // fragments of the previous tile's deferred steps: copied so that this tile's reads may reuse the arrays
    vec_t da[kDefer > 0 ? kDefer : 1];
    vec_t db[MW];
    if constexpr (kDefer > 0) {
#pragma unroll
      for (int d = 0; d < kDefer; ++d) da[d] = afr[NS - kDefer + d];
#pragma unroll
      for (int mw = 0; mw < MW; ++mw) db[mw] = bfr[3][mw];
    }
    auto read_step = [&](auto ic) {  // all reads that step `st` needs and that are not issued yet
      constexpr int st = decltype(ic)::value;
      constexpr int gq = st / NT, t = st % NT;
      if constexpr (t == 0) {
        static_for<0, MW>([&](auto im) {
          constexpr int mw = decltype(im)::value;
          lds_read_b128<mw * 16 * kRowBytes>(bfr[gq][mw], b_off[gq] + sb);
        });
      }
      lds_read_b128<t * 16 * kRowBytes>(afr[st], a_off[gq] + sb);
    };
    static_for<0, (PD < NS ? PD : NS)>(read_step);
    if constexpr (kDefer > 0) {
      if (have_prev) {
        static_for<0, kDefer>([&](auto id) {
          constexpr int d = decltype(id)::value;
          constexpr int t = (NS - kDefer + d) % NT;
          lds_tie(da[d]);  // pins these MFMAs after the barrier and the reads above
#pragma unroll
          for (int mw = 0; mw < MW; ++mw)
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[mw][t] = gemm_mma<T>(da[d][j], db[mw][j], acc[mw][t]);
        });
      }
    }
    static_for<0, NS>([&](auto ic) {
      constexpr int st = decltype(ic)::value;
      constexpr int gq = st / NT, t = st % NT;
      if constexpr (st + PD < NS) read_step(std::integral_constant<int, st + PD>{});
      // reads younger than a(st): steps st+1 .. min(st+PD, NS-1), each 1 read (+MW when it opens a group)
      constexpr int last = (st + PD < NS) ? st + PD : NS - 1;
      constexpr int groups = last / NT - gq;  // fragment groups opened by the younger steps
      constexpr int younger = (last - st) + groups * MW;
      lds_wait<(younger < 15 ? younger : 15)>(afr[st]);  // a smaller count only waits for more
      if constexpr (t == 0) {
        static_for<0, MW>([&](auto im) { lds_tie(bfr[gq][decltype(im)::value]); });
      }
      if constexpr (st < NS - kDefer) mfma_step(ic);
    });
  };

  constexpr int NSTAGE_C = ALIAS ? 3 : gemm_stages(GW, NT);
  int buf = 0;
  int64_t row0 = row_first;
  for (int ob = 0; ob < nob; ++ob, row0 += ob_rows) {
#pragma unroll
    for (int mw = 0; mw < MW; ++mw)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[mw][t] = (acc_t){0, 0, 0, 0};
    for (int i = 0; i < nk; ++i) {
      wg_barrier();  // matches the loaders' barrier: tile i is in LDS (all of this wave's LDS reads are retired)
      compute(buf, i > 0);
      buf = buf + 1 == NSTAGE_C ? 0 : buf + 1;
    }
    if constexpr (kDefer > 0) {
      if (nk > 0) static_for<NS - kDefer, NS>(mfma_step);
    }
#pragma unroll
    for (int mw = 0; mw < MW; ++mw)
      store_tile<T, NT>(g, acc[mw], row0 + 16 * MW * wave + 16 * mw, g.r_rows, col0, lane);
  }
}

// ---------------------------------------------------------------------------------------------
// gemm_tn: grid = (ceil(R_cols/64), column blocks, nsplit); reduction over the rows of R
// ---------------------------------------------------------------------------------------------
template <class T, int MW, int NT, int NW = 4>
__global__ __launch_bounds__(64 * (NW + kLoaders)) void gemm_tn_kernel(GemmArgs<T> g) {
  constexpr int GW = MW * NW / 4;  // see gemm_nn_kernel
  static_assert(NW == 4 || NW == 8, "4 or 8 MFMA waves");
  typedef typename MT<T>::acc_t acc_t;
  typedef typename MT<T>::vec_t vec_t;
  constexpr int VEC = MT<T>::VEC;
  constexpr int KT = MT<T>::KT;
  constexpr int STAGE = stage_bytes(GW, NT);
  constexpr int BIG = big_tile_bytes(GW);
  constexpr int RBT = 64 * GW * (int)sizeof(T);  // bytes per row of the big tile (64*GW outer columns)
  constexpr int LPR = RBT / 16;                  // lanes per row in one DMA instruction (16..128)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if (g.run_if && *g.run_if == 0) return;  // uniform over the grid
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // Which (outer tile, reduction slab) this workgroup takes.  Workgroups go to the eight XCDs round-robin in linear
  // block order (x fastest), so with the plain mapping the few outer tiles of ONE slab land on different XCDs and each
  // pulls that slab of the skinny operand through its own L2: at 1.25M x 512 (C4) Y crossed the fabric four times
  // (FETCH 4.16 GB for 2.96 GB algorithmic, 4.7 TB/s).  xcd_remap: of every 8 * gridDim.x consecutive workgroups, the
  // gridDim.x that share an XCD (ids congruent mod 8) take the outer tiles of one slab.
  int bx = (int)blockIdx.x, bz = (int)blockIdx.z;
  if (g.xcd_remap) {
    const int gx = (int)gridDim.x, per = 8 * gx;
    const int lin = bx + gx * bz, grp = lin / per, r = lin - grp * per;
    if ((grp + 1) * 8 <= (int)gridDim.z) {  // (a last, partial group of slabs keeps the plain mapping)
      bx = r >> 3;
      bz = grp * 8 + (r & 7);
    }
  }
  const int64_t n_first = (int64_t)bx * outer_tile(GW);
  const int64_t col0 = g.col_base + (int64_t)blockIdx.y * (NT * 16);
  const int t_begin = bz * g.tiles_per_split;
  const int t_end = min(t_begin + g.tiles_per_split, g.tiles_total);
  const int nk = t_end - t_begin;
  // outer tiles of this workgroup: bx, bx + gridDim.x, ... (see gemm_nn_kernel)
  const int nob = (g.outer_blocks - bx + (int)gridDim.x - 1) / (int)gridDim.x;
  const int64_t ob_cols = (int64_t)gridDim.x * outer_tile(GW);

  // The loader wave (4) issues the LDS-DMA, waves 0..3 run the MFMAs (see gemm_nn).  The big tile is a
  // row-linear LDS image of KT reduction rows x (64*MW outer columns); 16-byte slot lin = 64c + lane of
  // chunk c holds logical slot (lin % LPR) ^ tswz(row) of row lin / LPR.
  if (wave >= NW) {
    __builtin_amdgcn_s_setprio(3);
    int64_t n0 = n_first;  // outer tile being STAGED
    auto stage_checked = [&](int buf, int mt) {
      char* rt = smem + buf * STAGE;
      const int64_t m0 = (int64_t)mt * KT;
      for (int c = wave - NW; c < 16 * GW; c += kLoaders) {
        const int lin = c * 64 + lane;
        const int row = lin / LPR;
        const int lsb = (lin % LPR) ^ MT<T>::tswz(row);
        const int64_t grow = m0 + row;
        const int64_t nn = n0 + (int64_t)lsb * VEC;
        const T* src = (grow < g.r_rows && nn < g.r_cols_readable) ? g.r + grow * g.r_ld + nn : g.zero;
        glds16(src, rt + c * 1024);
      }
      for (int c = wave - NW; c < 4 * NT; c += kLoaders) {
        const int row = 4 * c + (lane >> 4);
        const int ls = (lane & 15) ^ (row & 15);
        glds16(g.x + (col0 + row) * g.x_ld + m0 + ls * VEC, rt + BIG + c * 1024);
      }
    };
    // big tile: the (row, swizzle) pattern of chunk c repeats every 8 chunks = 8*64/LPR tile rows; loader lw
    // of NL owns chunks c = lw + NL*i
    constexpr int NL = kLoaders, NVB = 8 / NL, NV = 4 / NL;
    const int lw = wave - NW;
    DmaStream<NVB, 2 * GW, NL> big;
    DmaStream<NV, NT, NL> sk;
#pragma unroll
    for (int pv = 0; pv < NVB; ++pv) {
      const int lin = (lw + NL * pv) * 64 + lane;
      const int row = lin / LPR;
      const int lsb = (lin % LPR) ^ MT<T>::tswz(row);
      big.ptr[pv] = (const char*)(g.r + ((int64_t)t_begin * KT + row) * g.r_ld + n0 + (int64_t)lsb * VEC);
    }
#pragma unroll
    for (int pv = 0; pv < NV; ++pv) {
      const int row = 4 * (lw + NL * pv) + (lane >> 4);
      const int ls = (lane & 15) ^ (row & 15);
      sk.ptr[pv] = (const char*)(g.x + (col0 + row) * g.x_ld + (int64_t)t_begin * KT + ls * VEC);
    }
    big.step = (int64_t)(8 * 64 / LPR) * g.r_ld * (int64_t)sizeof(T);
    big.adv = (int64_t)KT * g.r_ld * (int64_t)sizeof(T);
    sk.step = 16 * g.x_ld * (int64_t)sizeof(T);
    sk.adv = KT * (int64_t)sizeof(T);
    bool cols_inside = n0 + outer_tile(GW) <= g.r_cols_readable;
    auto stage_tile = [&](int buf, int mt) {
      char* rt = smem + buf * STAGE;
      if (cols_inside && (int64_t)(mt + 1) * KT <= g.r_rows) {
        big.issue(rt + lw * 1024);
        sk.issue(rt + BIG + lw * 1024);
      } else {
        stage_checked(buf, mt);
#pragma unroll
        for (int pv = 0; pv < NVB; ++pv) big.ptr[pv] += big.adv;
#pragma unroll
        for (int pv = 0; pv < NV; ++pv) sk.ptr[pv] += sk.adv;
      }
    };
    // ring of NSTAGE buffers: tiles i+1 .. i+NSTAGE-1 are in flight while the MFMA waves work on tile i
    constexpr int NSTAGE = gemm_stages(GW, NT);
    static_assert((16 * GW) % kLoaders == 0 && (4 * NT) % kLoaders == 0, "chunks must split evenly over the loaders");
    constexpr int DPL = (16 * GW + 4 * NT) / kLoaders;  // DMA instructions per loader wave per tile
    const int nflat = nob * nk;
    const int64_t big_jump = (ob_cols - (int64_t)nk * KT * g.r_ld) * (int64_t)sizeof(T);
    const int64_t sk_jump = -(int64_t)nk * KT * (int64_t)sizeof(T);
    int s_k = 0;
    auto stage_next = [&](int buf) {
      stage_tile(buf, t_begin + s_k);
      if (++s_k == nk) {  // on to the next outer tile
        s_k = 0;
        n0 += ob_cols;
#pragma unroll
        for (int pv = 0; pv < NVB; ++pv) big.ptr[pv] += big_jump;
#pragma unroll
        for (int pv = 0; pv < NV; ++pv) sk.ptr[pv] += sk_jump;
        cols_inside = n0 + outer_tile(GW) <= g.r_cols_readable;
      }
    };
    for (int t = 0; t < NSTAGE - 1 && t < nflat; ++t) stage_next(t % NSTAGE);
    for (int i = 0; i < nflat; ++i) {
      // tile i must have landed; the (NSTAGE-2) younger tiles may stay in flight (vmcnt counts in issue order)
      if (NSTAGE > 2 && i + NSTAGE - 2 < nflat)
        wait_vmcnt<(NSTAGE - 2) * DPL>();
      else
        wait_vmcnt<0>();
      wg_barrier();  // tile i visible to the MFMA waves; they are done reading buffer (i-1) % NSTAGE
      if (i + NSTAGE - 1 < nflat && !(g.debug_flags & 1)) stage_next((i + NSTAGE - 1) % NSTAGE);
    }
    return;
  }
  acc_t acc[MW][NT];

  // Fragment read addresses (bytes inside a stage), lane-invariant across tiles.  Skinny image: as in
  // gemm_nn.  Big image: element (reduction row mloc, outer column ncol) sits at
  // mloc*RBT + ((ncol/VEC) ^ tswz(mloc))*16 + (ncol%VEC)*sizeof(T); for this lane mloc =
  // (4*gq + kq)*VEC + j, and tswz(mloc) only depends on kq, so one base per mw plus immediates.
  const int fc = lane & 15, fkq = lane >> 4;
  const unsigned lds0 = lds_addr(smem);
  unsigned a_off[4], b_off[MW];
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) a_off[gq] = lds0 + BIG + fc * kRowBytes + (unsigned)(((4 * gq + fkq) ^ fc) << 4);
#pragma unroll
  for (int mw = 0; mw < MW; ++mw) {
    const int ncol = 16 * MW * wave + 16 * mw + fc;
    b_off[mw] = lds0 + (unsigned)(fkq * VEC * RBT + (((ncol / VEC) ^ MT<T>::tswz(fkq * VEC)) << 4) +
                                  (ncol % VEC) * (int)sizeof(T));
  }

  // same deferral of the last steps' MFMAs across the tile barrier as in gemm_nn_kernel
  constexpr int NS = 4 * NT;
  constexpr int PD = kPrefetchSteps;
  constexpr int kDefer = (NT >= 2 && NS - CORRLA_GEMM_DEFER >= PD) ? (CORRLA_GEMM_DEFER < NT ? CORRLA_GEMM_DEFER : NT) : 0;
  vec_t afr[NS];
  T bfr[4][MW][VEC];
  auto mfma_step = [&](auto ic) {
    constexpr int st = decltype(ic)::value;
    constexpr int gq = st / NT, t = st % NT;
#pragma unroll
    for (int mw = 0; mw < MW; ++mw)
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[mw][t] = gemm_mma<T>(afr[st][j], bfr[gq][mw][j], acc[mw][t]);
  };
  auto compute = [&](int buf, bool have_prev) {
    const unsigned sb = (unsigned)(buf * STAGE);
    vec_t da[kDefer > 0 ? kDefer : 1];
    T db[MW][VEC];
    if constexpr (kDefer > 0) {
#pragma unroll
      for (int d = 0; d < kDefer; ++d) da[d] = afr[NS - kDefer + d];
#pragma unroll
      for (int mw = 0; mw < MW; ++mw)
#pragma unroll
        for (int j = 0; j < VEC; ++j) db[mw][j] = bfr[3][mw][j];
    }
    auto read_step = [&](auto ic) {
      constexpr int st = decltype(ic)::value;
      constexpr int gq = st / NT, t = st % NT;
      if constexpr (t == 0) {
        static_for<0, MW * VEC>([&](auto iq) {
          constexpr int mw = decltype(iq)::value / VEC, j = decltype(iq)::value % VEC;
          lds_read_elem<(4 * gq * VEC + j) * RBT>(bfr[gq][mw][j], b_off[mw] + sb);
        });
      }
      lds_read_b128<t * 16 * kRowBytes>(afr[st], a_off[gq] + sb);
    };
    static_for<0, (PD < NS ? PD : NS)>(read_step);
    if constexpr (kDefer > 0) {
      if (have_prev) {
        static_for<0, kDefer>([&](auto id) {
          constexpr int d = decltype(id)::value;
          constexpr int t = (NS - kDefer + d) % NT;
          lds_tie(da[d]);
#pragma unroll
          for (int mw = 0; mw < MW; ++mw)
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[mw][t] = gemm_mma<T>(da[d][j], db[mw][j], acc[mw][t]);
        });
      }
    }
    static_for<0, NS>([&](auto ic) {
      constexpr int st = decltype(ic)::value;
      constexpr int gq = st / NT, t = st % NT;
      if constexpr (st + PD < NS) read_step(std::integral_constant<int, st + PD>{});
      constexpr int last = (st + PD < NS) ? st + PD : NS - 1;
      constexpr int groups = last / NT - gq;
      constexpr int younger = (last - st) + groups * MW * VEC;
      lds_wait<(younger < 15 ? younger : 15)>(afr[st]);  // a smaller count only waits for more
      if constexpr (t == 0) {
        static_for<0, MW * VEC>([&](auto iq) { lds_tie(bfr[gq][decltype(iq)::value / VEC][decltype(iq)::value % VEC]); });
      }
      if constexpr (st < NS - kDefer) mfma_step(ic);
    });
  };

  int buf = 0;
  int64_t n0 = n_first;
  for (int ob = 0; ob < nob; ++ob, n0 += ob_cols) {
#pragma unroll
    for (int mw = 0; mw < MW; ++mw)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[mw][t] = (acc_t){0, 0, 0, 0};
    for (int i = 0; i < nk; ++i) {
      wg_barrier();
      compute(buf, i > 0);
      buf = buf + 1 == gemm_stages(GW, NT) ? 0 : buf + 1;
    }
    if constexpr (kDefer > 0) {
      if (nk > 0) static_for<NS - kDefer, NS>(mfma_step);
    }
#pragma unroll
    for (int mw = 0; mw < MW; ++mw)
      store_tile<T, NT>(g, acc[mw], n0 + 16 * MW * wave + 16 * mw, g.r_cols, col0, lane, bz);
  }
}

// out[col][i] = scale * sum_z slab[z][col][i], i < limit, col < ncols; fixed summation tree (deterministic)
template <class T>
__global__ void slab_reduce_kernel(const T* slab, int64_t slab_stride, int nsplit, T* out, int64_t ld, int64_t limit,
                                   int64_t ncols, const T* scale, const int* run_if = nullptr) {
  if (run_if && *run_if == 0) return;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t col = blockIdx.y;
  if (i >= limit || col >= ncols) return;
  const int64_t off = col * ld + i;
  T s = 0;
  for (int z = 0; z < nsplit; ++z) s += slab[(int64_t)z * slab_stride + off];
  if (scale) s *= *scale;
  out[off] = s;
}
// many slabs, small output (the Gram matrices): 64 outputs x 4 slab groups per block, four loads in flight each
template <class T>
__global__ __launch_bounds__(256) void slab_reduce_deep_kernel(const T* slab, int64_t slab_stride, int nsplit, T* out,
                                                               int64_t ld, int64_t limit, int64_t ncols, const T* scale,
                                                               const int* run_if = nullptr) {
  if (run_if && *run_if == 0) return;
  __shared__ T part[4][64];
  const int li = threadIdx.x & 63, zg = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 64 + li;
  const int64_t col = blockIdx.y;
  const int per = (nsplit + 3) / 4;
  const int z0 = zg * per, z1 = min(nsplit, z0 + per);
  T s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  if (i < limit && col < ncols) {
    const T* src = slab + col * ld + i;
    int z = z0;
    for (; z + 3 < z1; z += 4) {
      s0 += src[(int64_t)z * slab_stride];
      s1 += src[(int64_t)(z + 1) * slab_stride];
      s2 += src[(int64_t)(z + 2) * slab_stride];
      s3 += src[(int64_t)(z + 3) * slab_stride];
    }
    for (; z < z1; ++z) s0 += src[(int64_t)z * slab_stride];
  }
  part[zg][li] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (zg == 0 && i < limit && col < ncols) {
    T s = (part[0][li] + part[1][li]) + (part[2][li] + part[3][li]);
    if (scale) s *= *scale;
    out[col * ld + i] = s;
  }
}

// ---- Frobenius norm pieces (random_svd.rs:53-55) ----------------------------------------------
template <class T>
__global__ void sumsq_partial_kernel(const T* y, int64_t n, double* partial) {
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = (double)y[i];
    s += v * v;
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  __shared__ double ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
__global__ void sum_partials_kernel(const double* partial, int n, double* out) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) s += partial[i];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (threadIdx.x == 0) *out = s;
}
// sum of the block partials and 1 / sqrt of it in one launch (the Z-side rescale of every power iteration)
template <class T>
__global__ void sum_partials_rsqrt_kernel(const double* partial, int n, double* ss_out, T* inv_out) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) s += partial[i];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (threadIdx.x == 0) {
    *ss_out = s;
    *inv_out = (T)(s > 0.0 ? 1.0 / sqrt(s) : 0.0);
  }
}
template <class T>
__global__ void rsqrt_scalar_kernel(const double* ss, T* out) {
  const double v = *ss;
  *out = (T)(v > 0.0 ? 1.0 / sqrt(v) : 0.0);
}
template <class T>
__global__ void sub_kernel(T* y, const T* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) y[i] -= p[i];
}
template <class T>
__global__ void scale_kernel(T* y, int64_t n, const T* scale) {
  const T sc = *scale;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] *= sc;
}

// ---- random_mat_normal (mat_utils.rs:161-175): Philox4x32-10 + Box-Muller -------------------
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0;
    c[1] = n1;
    c[2] = n2;
    c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
template <class T>
__device__ __forceinline__ T normal_from_index(uint64_t idx, uint64_t seed);
template <>
__device__ __forceinline__ float normal_from_index<float>(uint64_t idx, uint64_t seed) {
  uint32_t c[4] = {(uint32_t)idx, (uint32_t)(idx >> 32), 0u, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const float u1 = ((float)(c[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = ((float)(c[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}
// The two f64 uniforms of one Philox block: the top 53 bits of words (0, 1) and of words (2, 3), plus one half, times 2^-53.
// Never 0; below 1 but for the one pattern of 53 ones, where the sum rounds up to 2^53.  Counter (c0, c1, c2, c3), key = the two halves of seed.  Shared by the Gaussian generator
// (counter (idx, 0, 0)) and the Dirichlet stream (dirichlet_kernels.hpp).
__device__ __forceinline__ void philox_uniform_pair(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint64_t seed, double& u1, double& u2) {
  uint32_t c[4] = {c0, c1, c2, c3};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint64_t a = (((uint64_t)c[0] << 32) | c[1]) >> 11;
  const uint64_t b = (((uint64_t)c[2] << 32) | c[3]) >> 11;
  u1 = ((double)a + 0.5) * (1.0 / 9007199254740992.0);
  u2 = ((double)b + 0.5) * (1.0 / 9007199254740992.0);
}
// Box-Muller, the cosine branch
__device__ __forceinline__ double box_muller_f64(double u1, double u2) { return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2); }
template <>
__device__ __forceinline__ double normal_from_index<double>(uint64_t idx, uint64_t seed) {
  double u1, u2;
  philox_uniform_pair((uint32_t)idx, (uint32_t)(idx >> 32), 0u, 0u, seed, u1, u2);
  return box_muller_f64(u1, u2);
}
// element (i, j) -> p[i * rs + j * cs] = N(0,1) keyed by (seed, (row0 + i) * global_cols + j);
// consecutive threads walk the unit-stride direction
template <class T>
__global__ void fill_normal_kernel(T* p, int64_t rows, int64_t cols, int64_t rs, int64_t cs, uint64_t seed, int64_t row0,
                                   int64_t global_cols, int cols_fast) {
  const int64_t total = rows * cols;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    int64_t i, j;
    if (cols_fast) {
      i = t / cols;
      j = t - i * cols;
    } else {
      j = t / rows;
      i = t - j * rows;
    }
    p[i * rs + j * cs] = normal_from_index<T>((uint64_t)((row0 + i) * global_cols + j), seed);
  }
}

// ---- SVD of the l x l core (random_svd.rs:89) on the device -------------------------------------
// One-sided (Hestenes) Jacobi, in three kernel families: the single-workgroup ring kernel below (l <= 144), the
// multi-workgroup block Jacobi (jacobi_mc_kernels.hpp) and the block Jacobi with one launch per round (any l);
// core_svd_plan.hpp chooses between them.  Convergence is quadratic, so the sweep in which every
// |w_p.w_q| / (|w_p||w_q|) was already below sqrt(tol) is the last one.  On exit the columns of W are U_c * sigma
// and V = V_c with C = U_c diag(sigma) V_c^T.  sigma[:k], V_c[:, :k] (-> m1) and U_c[:, :k] (-> m2), sorted by
// sigma descending, go directly into the zero-padded skinny operands of the GEMMs that follow (U = Q * m1,
// V = Qb * m2), so the final stage needs no host round trip.
// Sum over a G-lane group (G = 8 or 16, groups aligned to G lanes), result in every lane.  f32 uses DPP
// (quad_perm xor-1 / xor-2, row_half_mirror, row_mirror) on the VALU; __shfl_xor would go through the LDS
// crossbar (ds_bpermute), which the Jacobi kernels cannot afford.  f64 keeps the shuffles.
template <int G>
__device__ __forceinline__ float group_sum(float x) {
  static_assert(G == 8 || G == 16, "group size");
  auto dpp = [](float v, auto ctrl) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value, 0xf, 0xf, true));
  };
  x += dpp(x, std::integral_constant<int, 0xB1>{});   // quad_perm [1,0,3,2]
  x += dpp(x, std::integral_constant<int, 0x4E>{});   // quad_perm [2,3,0,1]
  x += dpp(x, std::integral_constant<int, 0x141>{});  // row_half_mirror: lane i <-> 7 - i
  if constexpr (G == 16) x += dpp(x, std::integral_constant<int, 0x140>{});  // row_mirror: lane i <-> 15 - i
  return x;
}
template <int G>
__device__ __forceinline__ double group_sum(double x) {
#pragma unroll
  for (int msk = 1; msk < G; msk <<= 1) x += __shfl_xor(x, msk, G);
  return x;
}
// sqrt of a squared column norm for the final ranking of the Jacobi kernels: a non-finite value (non-finite input, reported
// through the status word) becomes 0, because comparisons with NaN are all false -- ranks would collide and the order
// table would keep uninitialised entries, i.e. wild column indices in the output loop
template <class T>
__device__ __forceinline__ T jacobi_safe_sigma(T a) {
  return (a >= (T)0 && a < (T)3.0e38) ? (T)sqrt(a) : (T)0;
}
// Jacobi rotation (cos, sin) that annihilates the off-diagonal g of [[a, g], [g, b]]; `rel` receives
// |g| / sqrt(a b).  f32 uses the single-instruction reciprocal / rsqrt (~1 ulp; the Jacobi kernels are
// VALU-issue bound and the IEEE sqrt/div sequences were ~1/4 of their instruction stream); f64 stays IEEE.
__device__ __forceinline__ bool jacobi_rotation(float a, float b, float g, float tol, float& cs, float& sn, float& rel,
                                                float& t) {
  // |g| / sqrt(a b) without forming a * b (two tiny columns would underflow it and never be rotated)
  const float rs = (a > 0.f && b > 0.f) ? __builtin_amdgcn_rsqf(a) * __builtin_amdgcn_rsqf(b) : 0.f;
  rel = fabsf(g) * rs;
  if (!(rel > tol)) return false;
  const float zeta = (b - a) * 0.5f * __builtin_amdgcn_rcpf(g);
  const float den = fabsf(zeta) + __builtin_amdgcn_sqrtf(1.f + zeta * zeta);
  t = copysignf(__builtin_amdgcn_rcpf(den), zeta);
  cs = __builtin_amdgcn_rsqf(1.f + t * t);
  sn = cs * t;
  // two columns of subnormal size (exact-arithmetic null directions of an integer-valued core): rcp(g) overflows
  // and (b - a) * inf is NaN or inf.  Such a pair carries no information; leave it alone rather than poison W.
  if (!(fabsf(sn) <= 1.f && cs <= 1.f)) return false;
  return true;
}
__device__ __forceinline__ bool jacobi_rotation(float a, float b, float g, float tol, float& cs, float& sn, float& rel) {
  float t;
  return jacobi_rotation(a, b, g, tol, cs, sn, rel, t);
}
// f64: the hardware reciprocal / reciprocal square root (~26 bits) refined by one Newton step each instead of the IEEE
// division / square-root sequences (3 + 3 of them per rotation, ~2/3 of the dependent chain of a Jacobi round in f64).
// The rotation only has to be orthogonal to rounding -- cs^2 + sn^2 = cs^2 (1 + t^2) is, whatever the last bits of t.
__device__ __forceinline__ double jr_rcp(double x) {
  double y = __builtin_amdgcn_rcp(x);
  return y * (2.0 - x * y);
}
__device__ __forceinline__ double jr_rsq(double x) {
  double y = __builtin_amdgcn_rsq(x);
  return y * (1.5 - 0.5 * x * y * y);
}
__device__ __forceinline__ bool jacobi_rotation(double a, double b, double g, double tol, double& cs, double& sn,
                                                double& rel, double& t) {
  // |g| / sqrt(a b) without forming a * b (as in f32)
  const double rs = (a > 0.0 && b > 0.0) ? jr_rsq(a) * jr_rsq(b) : 0.0;
  rel = fabs(g) * rs;
  if (!(rel > tol)) return false;
  const double zeta = (b - a) * 0.5 * jr_rcp(g);
  const double w = 1.0 + zeta * zeta;
  const double den = fabs(zeta) + w * jr_rsq(w);  // sqrt(w)
  t = copysign(jr_rcp(den), zeta);
  cs = jr_rsq(1.0 + t * t);
  sn = cs * t;
  if (!(fabs(sn) <= 1.0 && cs <= 1.0)) return false;  // subnormal-size columns / overflow of zeta: leave the pair alone
  return true;
}
__device__ __forceinline__ bool jacobi_rotation(double a, double b, double g, double tol, double& cs, double& sn,
                                                double& rel) {
  double t;
  return jacobi_rotation(a, b, g, tol, cs, sn, rel, t);
}
// pair (p < q) of slot `pr` in round `step` of the round-robin tournament on n players (no integer division)
__device__ __forceinline__ void tournament_pair(int n, int step, int pr, int& p, int& q) {
  if (pr == 0) {
    p = n - 1;
    q = step;
  } else {
    p = step + pr;
    if (p >= n - 1) p -= n - 1;
    q = step - pr;
    if (q < 0) q += n - 1;
  }
  if (p > q) {
    const int t_ = p;
    p = q;
    q = t_;
  }
}
// ---- ring Jacobi: columns resident in registers --------------------------------------------------
// One-sided Jacobi on one workgroup.  The column a processor (8 lanes) works on stays in REGISTERS (lane g
// owning the 16-byte row chunks g, g + 8, ...), and the pairs follow the odd-even transposition ordering:
// processor i holds the columns at line positions (2i, 2i + 1); after every rotation the two columns swap
// positions, and the window of every processor slides by one position back and forth, so only ONE column per
// processor crosses LDS per round (no address arithmetic or predication in the loop).  n rounds make every pair
// of columns meet exactly once.  Even round: rotate (P, Q), send Q to processor i - 1, receive Q from i + 1.  Odd
// round: rotate (P, Q), send P to i + 1, receive P from i - 1; the last processor then holds (position n - 1,
// wrapped position 0), which are not a pair of the line ordering: it applies (cs, sn) = (0, 1), i.e. P <- -Q,
// Q <- P, a swap that flips the sign of one singular-vector pair.
// The rows of V are independent and need nothing but the (cs, sn) of every round, so V is not accumulated here
// (that was ~45 % of the instructions of a ring kernel that did): jacobi_ring_w_kernel keeps only W in
// registers, records every round's rotations in a global stream (rot[round][processor] = (cs, sn), identity for
// skipped pairs) and double-buffers the W exchange: ONE barrier per round.  jacobi_replay_v_kernel then applies
// the recorded stream to V = I with 8 lanes per ROW of V (18 positions per lane in registers), 32 rows per
// workgroup, on as many CUs as there are row groups.  Line positions after S sweeps are known in closed form
// (always-swap odd-even transposition reverses the order every sweep), so the W kernel only has to publish
// rank[position] for the replay to scatter V_c[:, :k].
template <int G>
__device__ __forceinline__ float ring_sum(float x) {
  static_assert(G == 8, "lanes per processor");
  auto dpp = [](float v, auto ctrl) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value, 0xf, 0xf, true));
  };
  x += dpp(x, std::integral_constant<int, 0xB1>{});  // quad_perm [1,0,3,2]
  x += dpp(x, std::integral_constant<int, 0x4E>{});  // quad_perm [2,3,0,1]
  x += dpp(x, std::integral_constant<int, 0x141>{});  // row_half_mirror
  return x;
}
template <int G>
__device__ __forceinline__ double ring_sum(double x) {
  static_assert(G == 8, "lanes per processor");
  auto dpp = [](double v, auto ctrl) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, decltype(ctrl)::value, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, decltype(ctrl)::value, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
  };
  x += dpp(x, std::integral_constant<int, 0xB1>{});
  x += dpp(x, std::integral_constant<int, 0x4E>{});
  x += dpp(x, std::integral_constant<int, 0x141>{});
  return x;
}
template <class T>
struct RotEntry {
  T cs, sn;
};
template <class T, int E, int G>
__global__ __launch_bounds__(kRingProcPad * G) void jacobi_ring_w_kernel(const T* __restrict__ c, int64_t ldc, int l, T* m2,
                                                                        int64_t ld2, T* s_out, int k, T tol, T tol_early,
                                                                        int max_sweeps, RotEntry<T>* rot, int* rank_g,
                                                                        int* info) {
  typedef typename MT<T>::vec_t vec_t;
  constexpr int VW = MT<T>::VEC;
  static_assert(E % VW == 0, "whole 16-byte chunks per lane");
  constexpr int NC = E / VW;
  constexpr int RS = G * E;  // padded column length
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int n2 = (l + 1) & ~1, np = n2 >> 1;
  const int nproc = blockDim.x / G;      // processors incl. the idle ones of the last wave: all own LDS slots, so
                                         // the round body needs no "active" guards
  T* xw = (T*)smem;                      // [2][nproc][RS] W column in flight (double-buffered)
  T* sigma = xw + (size_t)2 * nproc * RS;  // [n2]
  T* xn = sigma + n2;                    // [2][nproc] squared norm of the column in flight
  int* rank = (int*)(xn + 2 * nproc);    // [n2]
  int* flag = rank + n2;                 // [4]
  const int tid = threadIdx.x, proc = tid / G, g = tid % G;
  const bool act = proc < np;
  const bool last = proc == np - 1;
  vec_t pw[NC], qw[NC];
  {
    const int colp = 2 * proc, colq = 2 * proc + 1;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
#pragma unroll
      for (int z = 0; z < VW; ++z) {
        const int row = (cc * G + g) * VW + z;
        const bool ok = act && row < l;
        pw[cc][z] = (ok && colp < l) ? c[(int64_t)colp * ldc + row] : (T)0;
        qw[cc][z] = (ok && colq < l) ? c[(int64_t)colq * ldc + row] : (T)0;
      }
  }
  // Scale invariance: the core is multiplied by an exact power of two that brings its largest entry into [1, 2)
  // (squared column norms of a tiny or huge core would under- / overflow); sigma is scaled back on output.
  int sexp = 0;
  {
    T mx = (T)0;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
#pragma unroll
      for (int z = 0; z < VW; ++z) mx = fmax(mx, fmax(fabs(pw[cc][z]), fabs(qw[cc][z])));
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    if ((tid & 63) == 0) sigma[tid >> 6] = mx;   // sigma is scratch until the end
    __syncthreads();
    mx = (T)0;
    for (int wv = 0; wv < (int)((blockDim.x + 63) >> 6); ++wv) mx = fmax(mx, sigma[wv]);
    __syncthreads();
    if (mx > (T)0 && mx <= std::numeric_limits<T>::max()) {  // finite, non-zero
      (void)frexp((double)mx, &sexp);
      sexp = 1 - sexp;  // mx * 2^sexp in [1, 2)
#pragma unroll
      for (int cc = 0; cc < NC; ++cc)
#pragma unroll
        for (int z = 0; z < VW; ++z) {
          pw[cc][z] = (T)ldexp((double)pw[cc][z], sexp);
          qw[cc][z] = (T)ldexp((double)qw[cc][z], sexp);
        }
    }
  }
  const int my_off = proc * RS + g * VW;
  // idle processors (proc >= np) form their own harmless ring of zero columns
  const int up_proc = act ? (proc + 1 >= np ? 0 : proc + 1) : proc, dn_proc = act ? (proc == 0 ? np - 1 : proc - 1) : proc;
  const int up_off = up_proc * RS + g * VW, dn_off = dn_proc * RS + g * VW;
  T na = (T)0, nb = (T)0;
  auto recompute_norms = [&]() {
    vec_t va, vb;
#pragma unroll
    for (int z = 0; z < VW; ++z) va[z] = vb[z] = (T)0;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
      va += pw[cc] * pw[cc];
      vb += qw[cc] * qw[cc];
    }
    T a = va[0], b = vb[0];
#pragma unroll
    for (int z = 1; z < VW; ++z) {
      a += va[z];
      b += vb[z];
    }
    na = ring_sum<G>(a);
    nb = ring_sum<G>(b);
  };
  // one round: rotate (P, Q), record the rotation, send `snd` (with its norm) and receive it from `src`
  auto round = [&](bool forced, RotEntry<T>* rot_row, T* xwb, T* xnb, vec_t (&snd)[NC], T& nsnd, int src_off, int src_proc) {
    vec_t vg;
#pragma unroll
    for (int z = 0; z < VW; ++z) vg[z] = (T)0;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) vg += pw[cc] * qw[cc];
    T gg = vg[0];
#pragma unroll
    for (int z = 1; z < VW; ++z) gg += vg[z];
    gg = ring_sum<G>(gg);
    T rel = (T)0, t = (T)0, cs = (T)1, sn = (T)0;
    const bool rot_now = !forced && jacobi_rotation(na, nb, gg, tol, cs, sn, rel, t);
    if (rot_now) {
      if (g == 0) {
        flag[0] = 1;
        if (rel > tol_early) flag[1] = 1;
      }
      na -= t * gg;
      nb += t * gg;
    } else {
      cs = (T)1;
      sn = (T)0;
    }
    if (g == 0) rot_row[proc] = RotEntry<T>{cs, sn};  // the pseudo pair is recorded as the identity
    if (forced) {  // P <- -Q, Q <- P
      cs = (T)0;
      sn = (T)1;
      const T tmp = na;
      na = nb;
      nb = tmp;
    }
    // unconditional: (cs, sn) = (1, 0) is exact, and a branch would only pay off when all 8 processors of a wave skip
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
      const vec_t x = pw[cc], y = qw[cc];
      pw[cc] = cs * x - sn * y;
      qw[cc] = sn * x + cs * y;
    }
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) *(vec_t*)(xwb + my_off + cc * G * VW) = snd[cc];
    if (g == 0) xnb[proc] = nsnd;
    // LDS-only barrier: the rotation-stream store above must stay in flight (__syncthreads waits on vmcnt too)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) snd[cc] = *(const vec_t*)(xwb + src_off + cc * G * VW);
    nsnd = xnb[src_proc];
  };
  int sweep = 0;
  int rounds = 0;
  for (; sweep < max_sweeps; ++sweep) {
    if (tid < 2) flag[tid] = 0;
    recompute_norms();
    __syncthreads();
    for (int r2 = 0; r2 < np; ++r2, rounds += 2) {
      // even round: send Q to processor i - 1, receive Q from i + 1
      round(false, rot + (size_t)rounds * kRingProcPad, xw, xn, qw, nb, up_off, up_proc);
      // odd round: send P to i + 1, receive P from i - 1 (other buffer: one barrier per round is enough)
      round(last, rot + (size_t)(rounds + 1) * kRingProcPad, xw + (size_t)nproc * RS, xn + nproc, pw, na, dn_off, dn_proc);
    }
    __syncthreads();
    const int rotated = flag[0], big = flag[1];
    __syncthreads();
    if (!rotated || !big) {
      ++sweep;  // this sweep's rounds are in the stream whether or not it rotated anything
      break;
    }
  }
  // Column ids by position: every completed sweep reverses the line order.  The zero padding column of an odd l
  // (id l) must sort last even against exact-zero singular values.
  {
    T a = 0, b = 0;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
#pragma unroll
      for (int z = 0; z < VW; ++z) {
        a += pw[cc][z] * pw[cc][z];
        b += qw[cc][z] * qw[cc][z];
      }
    a = ring_sum<G>(a);
    b = ring_sum<G>(b);
    const int nsw = rounds / n2;
    const int idp = (nsw & 1) ? n2 - 1 - 2 * proc : 2 * proc;
    const int idq = (nsw & 1) ? n2 - 2 - 2 * proc : 2 * proc + 1;
    if (act && g == 0) {
      sigma[2 * proc] = idp < l ? jacobi_safe_sigma(a) : (T)-1;
      sigma[2 * proc + 1] = idq < l ? jacobi_safe_sigma(b) : (T)-1;
    }
  }
  __syncthreads();
  for (int j = tid; j < n2; j += blockDim.x) {
    const T sj = sigma[j];
    int r = 0;
    for (int i = 0; i < n2; ++i) {
      const T si = sigma[i];
      r += (si > sj || (si == sj && i < j)) ? 1 : 0;
    }
    rank[j] = r;
    rank_g[j] = r;
  }
  __syncthreads();
  if (act) {
    const int rp = rank[2 * proc], rq = rank[2 * proc + 1];
    const T sp = sigma[2 * proc], sq = sigma[2 * proc + 1];
    const T ip = sp > (T)0 ? (T)1 / sp : (T)0, iq = sq > (T)0 ? (T)1 / sq : (T)0;
#pragma unroll
    for (int cc = 0; cc < NC; ++cc)
#pragma unroll
      for (int z = 0; z < VW; ++z) {
        const int row = (cc * G + g) * VW + z;
        if (row < l) {
          if (rp < k) m2[(int64_t)rp * ld2 + row] = pw[cc][z] * ip;
          if (rq < k) m2[(int64_t)rq * ld2 + row] = qw[cc][z] * iq;
        }
      }
    if (g == 0) {
      if (rp < k) s_out[rp] = sp > (T)0 ? (T)ldexp((double)sp, -sexp) : (T)0;
      if (rq < k) s_out[rq] = sq > (T)0 ? (T)ldexp((double)sq, -sexp) : (T)0;
    }
  }
  if (tid == 0) {
    info[0] = sweep;
    info[1] = rounds;
  }
}

// V_c[:, :k] from the recorded rotation stream: 8 lanes per row of V, 18 line positions per lane, 32 rows per
// workgroup.  Round semantics (identical to the ring kernel): pair (first, second) = positions (2i, 2i + 1) in
// even rounds, (2i + 1, 2i + 2) in odd rounds; first <- sn x + cs y, second <- cs x - sn y (rotation, then the two
// columns swap positions); in odd rounds positions n - 1 and 0 are idle and position 0 changes sign (the pseudo
// pair of the last processor).
constexpr int kReplayChunk = 16;  // rounds staged in LDS at a time
// value of the previous / next lane inside the 16-lane DPP row (the 8-lane groups are row-aligned)
__device__ __forceinline__ float dpp_from_prev(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x111, 0xf, 0xf, true));
}
__device__ __forceinline__ float dpp_from_next(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x101, 0xf, 0xf, true));
}
__device__ __forceinline__ double dpp_from_prev(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x111, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), 0x111, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double dpp_from_next(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x101, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), 0x101, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
template <class T>
__global__ __launch_bounds__(256) void jacobi_replay_v_kernel(const RotEntry<T>* __restrict__ rot, const int* __restrict__ info,
                                                              const int* __restrict__ rank_g, int l, int k, T* m1,
                                                              int64_t ld1) {
  constexpr int GL = kReplayLanes, NPL = GL == 16 ? 10 : 6, NPR = NPL / 2;  // GL * NPL >= 144 positions
  static_assert(GL * NPL >= 2 * kRingProcPad, "positions");
  constexpr int ROWS = 256 / GL;                             // rows of V per workgroup
  constexpr int kReplayRow = GL * (NPR + 1);                 // staged entries per round (one pad entry per lane)
  typedef typename MT<T>::vec_t vec_t;
  constexpr int VW = MT<T>::VEC;
  constexpr int EV = (2 * (NPR + 1)) / VW;  // 16-byte vectors holding one lane's staged entries
  static_assert((2 * (NPR + 1)) % VW == 0, "lane entries must fill whole 16-byte vectors");
  __shared__ __attribute__((aligned(16))) RotEntry<T> stage[2][kReplayChunk][kReplayRow];
  const int n2 = (l + 1) & ~1, np = n2 >> 1;
  const int nrounds = info[1];
  const int tid = threadIdx.x, ln = tid % GL, row = blockIdx.x * ROWS + tid / GL;
  T v[NPL];
#pragma unroll
  for (int j = 0; j < NPL; ++j) v[j] = (ln * NPL + j == row && row < l) ? (T)1 : (T)0;
  const int nchunks = (nrounds + kReplayChunk - 1) / kReplayChunk;
  constexpr int PER_THREAD = (kReplayChunk * kRingProcPad + 255) / 256;
  RotEntry<T> pre[PER_THREAD];
  auto fetch = [&](int chunk) {
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) {
      const int idx = tid + 256 * q;
      const int64_t gidx = (int64_t)chunk * kReplayChunk * kRingProcPad + idx;
      const bool ok = idx < kReplayChunk * kRingProcPad && gidx < (int64_t)nrounds * kRingProcPad;
      pre[q] = ok ? rot[gidx] : RotEntry<T>{(T)1, (T)0};
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) {
      const int idx = tid + 256 * q;
      if (idx < kReplayChunk * kRingProcPad) {
        const int rr = idx / kRingProcPad, i = idx - rr * kRingProcPad;
        stage[buf][rr][(i / NPR) * (NPR + 1) + i % NPR] = pre[q];
      }
    }
  };
  // validity of this lane's pairs (even rounds: i < np; odd rounds: i < np - 1)
  const int i0 = ln * NPR;
  if (nchunks > 0) {
    fetch(0);
    stash(0);
  }
  __syncthreads();
  for (int ch = 0; ch < nchunks; ++ch) {
    const int buf = ch & 1;
    if (ch + 1 < nchunks) fetch(ch + 1);
    const int r_hi = min(kReplayChunk, nrounds - ch * kReplayChunk);
    // Rounds come in (even, odd) pairs (chunks start on an even round); the entries of the next round are
    // loaded into the other register set while this one is applied, so no LDS latency sits between rounds.
    vec_t ea[EV], eb[EV];
    T acs = (T)1, asn = (T)0, bcs = (T)1, bsn = (T)0;  // boundary pair of the previous lane
    auto load_round = [&](int rr, vec_t (&dst)[EV], T& pc, T& ps) {
      const vec_t* src = (const vec_t*)&stage[buf][rr][ln * (NPR + 1)];
#pragma unroll
      for (int q = 0; q < EV; ++q) dst[q] = src[q];
      const RotEntry<T> pb = stage[buf][rr][ln > 0 ? (ln - 1) * (NPR + 1) + NPR - 1 : 0];
      pc = pb.cs;
      ps = pb.sn;
    };
    auto even_round = [&](const vec_t (&e)[EV]) {
#pragma unroll
      for (int j = 0; j < NPR; ++j) {
        const T cs = e[(2 * j) / VW][(2 * j) % VW], sn = e[(2 * j + 1) / VW][(2 * j + 1) % VW];
        const bool ok = i0 + j < np;
        const T x = v[2 * j], y = v[2 * j + 1];
        const T nx = sn * x + cs * y, ny = cs * x - sn * y;
        v[2 * j] = ok ? nx : x;
        v[2 * j + 1] = ok ? ny : y;
      }
    };
    auto odd_round = [&](const vec_t (&e)[EV], T pc, T ps) {
      const T my_last = v[NPL - 1], my_first = v[0];
      // neighbours' boundary values: DPP inside a 16-lane row, the LDS crossbar for 32-lane groups (issued
      // first, consumed after the in-lane pairs)
      const T y_next = GL <= 16 ? dpp_from_next(my_first) : __shfl_down(my_first, 1, GL);
      const T x_prev = GL <= 16 ? dpp_from_prev(my_last) : __shfl_up(my_last, 1, GL);
#pragma unroll
      for (int j = 0; j < NPR - 1; ++j) {
        const T cs = e[(2 * j) / VW][(2 * j) % VW], sn = e[(2 * j + 1) / VW][(2 * j + 1) % VW];
        const bool ok = i0 + j < np - 1;
        const T x = v[2 * j + 1], y = v[2 * j + 2];
        const T nx = sn * x + cs * y, ny = cs * x - sn * y;
        v[2 * j + 1] = ok ? nx : x;
        v[2 * j + 2] = ok ? ny : y;
      }
      const T lcs = e[(2 * (NPR - 1)) / VW][(2 * (NPR - 1)) % VW], lsn = e[(2 * NPR - 1) / VW][(2 * NPR - 1) % VW];
      const T nl = lsn * my_last + lcs * y_next;
      v[NPL - 1] = (ln < GL - 1 && i0 + NPR - 1 < np - 1) ? nl : my_last;
      const T nf = pc * x_prev - ps * my_first;
      v[0] = ln == 0 ? -my_first : ((i0 - 1 < np - 1) ? nf : my_first);
    };
    if (r_hi > 0) load_round(0, ea, acs, asn);
    for (int rr = 0; rr < r_hi; rr += 2) {
      if (rr + 1 < r_hi) load_round(rr + 1, eb, bcs, bsn);
      even_round(ea);
      if (rr + 1 < r_hi) {
        if (rr + 2 < r_hi) load_round(rr + 2, ea, acs, asn);
        odd_round(eb, bcs, bsn);
      }
    }
    if (ch + 1 < nchunks) stash(buf ^ 1);
    __syncthreads();
  }
  if (row < l) {
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const int pos = ln * NPL + j;
      if (pos < n2) {
        const int r = rank_g[pos];
        if (r < k) m1[(int64_t)r * ld1 + row] = v[j];
      }
    }
  }
}

// ---- block Jacobi SVD of the l x l core for any l (random_svd.rs:89) -----------------------------
// W (= C on entry) and V (= I) live in global memory (L2-resident, a few hundred KiB).  The columns are
// cut into nb blocks of 8; a round-robin tournament over the blocks gives nb/2 disjoint block pairs per
// round, one kernel launch per round, ONE WAVE per block pair:
//   1. stage the 16 columns of W and V into LDS,
//   2. G = W_S^T W_S (16 x 16) with MFMAs (the same LDS element feeds both operands),
//   3. two-sided Jacobi on G in LDS (tournament of 8 disjoint rotations per step, all 64 lanes apply
//      them) accumulating the 16 x 16 rotation J -- in exact arithmetic this is one-sided Jacobi on the
//      16 columns without touching the long columns,
//   4. W_S <- W_S J and V_S <- V_S J with MFMAs, stored straight from the accumulators.
// Every element of W and V is read and written once per ROUND (2*nb/8 times fewer than per column-pair
// step).  Convergence: each wave publishes max |g_pq| / sqrt(g_pp g_qq) of its block pair (before
// rotating) with atomicMax; a one-thread kernel per sweep raises `done` when the whole sweep stayed
// below tol_early (quadratic convergence), and every later launch returns immediately.
struct JacobiCtl {
  unsigned done;
  unsigned max_bits;  // float bits of the sweep's max relative off-diagonal (non-negative floats order as uints)
  unsigned sweeps;
  unsigned pad;
};

template <class T>
__global__ __launch_bounds__(256) void jacobi_block_round_kernel(T* w, int64_t ldw, T* v, int64_t ldv, int rows_pad, int nb,
                                                                 int round, int inner_sweeps, JacobiCtl* ctl) {
  typedef typename MT<T>::acc_t acc_t;
  if (ctl->done) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int LP = rows_pad + 1;
  T* wt = (T*)smem;          // [16][LP]
  T* vt = wt + 16 * LP;      // [16][LP]
  T* gm = vt + 16 * LP;      // [16][17]
  T* g2 = gm + 16 * 17;      // [16][17]
  T* jm = g2 + 16 * 17;      // [16][17]
  T* gpart = jm + 16 * 17;   // [4][16][17] partial Grams of the 4 waves
  T* alpha = gpart + 4 * 16 * 17;  // [16]
  T* beta = alpha + 16;            // [16]
  int* part = (int*)(beta + 16);
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int x = lane & 15, kq = lane >> 4;
  // block pair of this workgroup
  int bi, bj;
  tournament_pair(nb, round, blockIdx.x, bi, bj);
  auto gcol = [&](int c) { return (c < 8) ? bi * 8 + c : bj * 8 + (c - 8); };
  // 1. stage the 16 columns of W and V (all 4 waves)
  for (int e = tid; e < 16 * rows_pad; e += 256) {
    const int c = e / rows_pad, r = e - c * rows_pad;
    const int64_t gc = gcol(c);
    wt[c * LP + r] = w[gc * ldw + r];
    vt[c * LP + r] = v[gc * ldv + r];
  }
  __syncthreads();
  // 2. Gram: wave `wave` sums the 16-row groups it = wave, wave + 4, ... (independent MFMA chains per wave)
  const int nit = rows_pad / 16;
  {
    acc_t acc = (acc_t){0, 0, 0, 0};
    for (int it = wave; it < nit; it += 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const T a = wt[x * LP + 16 * it + 4 * kq + j];
        acc = MT<T>::mma(a, a, acc);
      }
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) gpart[(wave * 16 + MT<T>::drow(lane, jj)) * 17 + x] = acc[jj];
  }
  __syncthreads();
  {
    const int r = tid >> 4, cx = tid & 15;  // 256 threads = 16 x 16 entries
    const T gsum = gpart[(0 * 16 + r) * 17 + cx] + gpart[(1 * 16 + r) * 17 + cx] + gpart[(2 * 16 + r) * 17 + cx] +
                   gpart[(3 * 16 + r) * 17 + cx];
    gm[r * 17 + cx] = gsum;
    jm[r * 17 + cx] = (r == cx) ? (T)1 : (T)0;
  }
  __syncthreads();
  // 3. inner two-sided Jacobi on the 16 x 16 Gram, wave 0 only (the others wait at the barrier below)
  if (wave == 0) {
    {  // convergence measure of this block pair (before rotating)
      float mx = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int idx = lane + 64 * e, r = idx >> 4, cx = idx & 15;
        if (r != cx) {
          const T d = gm[r * 17 + r] * gm[cx * 17 + cx];
          if (d > (T)0) mx = fmaxf(mx, (float)(fabs(gm[r * 17 + cx]) / sqrt(d)));
        }
      }
      for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_down(mx, off, 64));
      if (lane == 0) atomicMax(&ctl->max_bits, __float_as_uint(mx));
    }
    const T tiny = (T)4 * (T)(sizeof(T) == 4 ? 1.1920929e-07 : 2.220446049250313e-16);
    for (int sw = 0; sw < inner_sweeps; ++sw) {
      for (int step = 0; step < 15; ++step) {
        if (lane < 8) {
          int p, q;
          tournament_pair(16, step, lane, p, q);
          T cs = (T)1, sn = (T)0, rel;
          if (!jacobi_rotation(gm[p * 17 + p], gm[q * 17 + q], gm[p * 17 + q], tiny, cs, sn, rel)) {
            cs = (T)1;
            sn = (T)0;
          }
          alpha[p] = cs;
          beta[p] = -sn;
          part[p] = q;
          alpha[q] = cs;
          beta[q] = sn;
          part[q] = p;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // G <- R^T G R in one pass through g2, J <- J R
        T gn[4], jn[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int idx = lane + 64 * e, r = idx >> 4, cx = idx & 15, pc = part[cx], pr_ = part[r];
          const T ar = alpha[r], br = beta[r], ac = alpha[cx], bc = beta[cx];
          gn[e] = ar * (ac * gm[r * 17 + cx] + bc * gm[r * 17 + pc]) + br * (ac * gm[pr_ * 17 + cx] + bc * gm[pr_ * 17 + pc]);
          jn[e] = ac * jm[r * 17 + cx] + bc * jm[r * 17 + pc];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int idx = lane + 64 * e, r = idx >> 4, cx = idx & 15;
          gm[r * 17 + cx] = gn[e];
          jm[r * 17 + cx] = jn[e];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  __syncthreads();
  // 4. apply J to the W and V column blocks: wave `wave` owns the row groups it = wave, wave + 4, ...
  T jb[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) jb[ks] = jm[(4 * ks + kq) * 17 + x];
  const int64_t gx = gcol(x);
  for (int it = wave; it < nit; it += 4) {
    acc_t aw = (acc_t){0, 0, 0, 0}, av = (acc_t){0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      aw = MT<T>::mma(wt[(4 * ks + kq) * LP + 16 * it + x], jb[ks], aw);
      av = MT<T>::mma(vt[(4 * ks + kq) * LP + 16 * it + x], jb[ks], av);
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int r = 16 * it + MT<T>::drow(lane, jj);
      w[gx * ldw + r] = aw[jj];
      v[gx * ldv + r] = av[jj];
    }
  }
}

__global__ void jacobi_sweep_end_kernel(JacobiCtl* ctl, float tol_early) {
  if (ctl->done) return;
  ctl->sweeps += 1;
  if (__uint_as_float(ctl->max_bits) <= tol_early) ctl->done = 1;
  ctl->max_bits = 0;
}

template <class T>
__global__ void jacobi_init_kernel(const T* c, int64_t ldc, int l, T* w, int64_t ldw, T* v, int64_t ldv, int cols_pad,
                                   int rows_pad, JacobiCtl* ctl, const int* sexp_p) {
  // W <- 2^sexp * C: the prescale core_finite_check_kernel chose (0 for a core near unit scale), undone by the finish kernel
  const int sexp = *sexp_p;
  const int64_t total = (int64_t)cols_pad * rows_pad;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(e / rows_pad), i = (int)(e - (int64_t)j * rows_pad);
    const bool in = i < l && j < l;
    const T x = in ? c[(int64_t)j * ldc + i] : (T)0;
    w[(int64_t)j * ldw + i] = sexp ? (T)ldexp((double)x, sexp) : x;
    v[(int64_t)j * ldv + i] = (in && i == j) ? (T)1 : (T)0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctl->done = 0;
    ctl->max_bits = 0;
    ctl->sweeps = 0;
    ctl->pad = 0;
  }
}

// sigma_j = ||w_j||, descending order, outputs (see the top of the core-SVD section)
template <class T>
__global__ __launch_bounds__(1024) void jacobi_finish_kernel(const T* w, int64_t ldw, const T* v, int64_t ldv, int l, T* m1,
                                                             int64_t ld1, T* m2, int64_t ld2, T* s_out, int k, const int* sexp_p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* sigma = (T*)smem;
  int* order = (int*)(sigma + l + 2);
  const int sexp = *sexp_p;
  const int tid = threadIdx.x, group = tid >> 4, gl = tid & 15;
  for (int j = group; j < l; j += 64) {
    T a = 0;
    for (int i = gl; i < l; i += 16) {
      const T xx = w[(int64_t)j * ldw + i];
      a += xx * xx;
    }
#pragma unroll
    for (int msk = 1; msk < 16; msk <<= 1) a += __shfl_xor(a, msk, 16);
    if (gl == 0) sigma[j] = jacobi_safe_sigma(a);  // NaN-safe: the ranking below must stay a permutation
  }
  __syncthreads();
  for (int j = tid; j < l; j += 1024) {
    const T sj = sigma[j];
    int r = 0;
    for (int i = 0; i < l; ++i) {
      const T si = sigma[i];
      r += (si > sj || (si == sj && i < j)) ? 1 : 0;
    }
    order[r] = j;
  }
  __syncthreads();
  for (int r = group; r < k; r += 64) {
    const int j = order[r];
    const T sj = sigma[j];
    const T inv = sj > (T)0 ? (T)1 / sj : (T)0;
    for (int i = gl; i < l; i += 16) {
      m2[(int64_t)r * ld2 + i] = w[(int64_t)j * ldw + i] * inv;
      m1[(int64_t)r * ld1 + i] = v[(int64_t)j * ldv + i];
    }
    if (gl == 0) s_out[r] = sexp ? (T)ldexp((double)sj, -sexp) : sj;
  }
}

// ---- non-finite cores -------------------------------------------------------------------------------
// One workgroup scans the l x l core of the small SVD (random_svd.rs:89) before a kernel family that has no status
// word of its own (ring / block Jacobi): *bad <- 1 and, when a status record is given, st->fail <- 3,
// so that a non-finite core ends the call with CORRLA_ENUMERIC instead of a triplet of zeros.  (The multi-workgroup
// Jacobi reports the same through jmc_init_kernel / jmc_finish_kernel.)
template <class T>
__global__ __launch_bounds__(1024) void core_finite_check_kernel(const T* __restrict__ c, int64_t ld, int l, CholStatus* st, int* bad_out,
                                                                  int* sexp_out) {
  // (in the element type: an f64 core of 2^400 is finite, and inf as a float)
  const T finite_below = sizeof(T) == 4 ? (T)3.0e38f : (T)1.0e300;
  __shared__ T red[16];
  int bad = 0;
  T mx = (T)0;
  for (int idx = threadIdx.x; idx < l * l; idx += 1024) {
    const int j = idx / l, i = idx - j * l;
    const T x = fabs(c[(int64_t)j * ld + i]);
    if (!(x < finite_below)) bad = 1;
    mx = fmax(mx, x);
  }
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    if (bad) {
      if (st) st->fail = 3;
      if (bad_out) *bad_out = 1;
    }
    // sexp_out (the block Jacobi, which has no prescale of its own): the exponent that brings the largest entry of a core
    // far from unit scale into [1, 2); 0 for a core within 2^-30 .. 2^30, whose kernels run on it as it is
    if (sexp_out) {
      for (int i = 0; i < 16; ++i) mx = fmax(mx, red[i]);
      int e = 0;
      if (!bad && mx > (T)0 && (mx > (T)1073741824.0 || mx < (T)9.313225746154785e-10)) {
        (void)frexp((double)mx, &e);
        e = 1 - e;
      }
      *sexp_out = e;
    }
  }
}
// TEST HOOK (CORRLA_TEST_POISON_CORE, tests/test_gpu_parity.py): one entry of a device matrix <- NaN (kind 1) / +inf (2)
template <class T>
__global__ void poison_entry_kernel(T* p, int kind) {
  *p = kind == 2 ? std::numeric_limits<T>::infinity() : std::numeric_limits<T>::quiet_NaN();
}

// ---- PCA caller: centring (center_mat_col, mat_utils.rs:482-502) -----------------------------------
template <class T>
__global__ void fill_const_kernel(T* p, int64_t n, T v) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}
// out[r][c] = in[r][c] - (along_cols ? mu[c] : mu[r]); row-major in/out with leading dimensions ldi / ldo.
// inv_sd (optional, indexed like mu): the centred value is scaled by it (the centred AND standardised copy)
template <class T>
__global__ void center_kernel(const T* in, int64_t rows, int64_t cols, int64_t ldi, const T* mu, int along_cols, T* out,
                              int64_t ldo, const T* inv_sd) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  const T mc = along_cols ? mu[c] : (T)0;
  const T ic = (inv_sd && along_cols) ? inv_sd[c] : (T)1;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const T m_ = along_cols ? mc : mu[r];
    const T d = in[r * ldi + c] - m_;
    out[r * ldo + c] = inv_sd ? d * (along_cols ? ic : inv_sd[r]) : d;
  }
}

// ---- implicit centring: rank-1 corrections of the products with A - 1 mu^T ----------------
// partial[b][c] = sum over this block's rows of (w ? w[r] : 1) * x(r, c), f64 accumulation, fixed order
template <class T>
__global__ __launch_bounds__(256) void wcolsum_partial_kernel(const T* __restrict__ x, int64_t ld, int64_t rows,
                                                              const T* __restrict__ w, double* partial, int ncols) {
  __shared__ double red[256];
  const int c = blockIdx.y;
  const int64_t per = (rows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = min(rows, r0 + per);
  double s = 0.0;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) s += (w ? (double)w[r] : 1.0) * (double)x[(int64_t)c * ld + r];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * ncols + c] = red[0];
}
template <class T>
__global__ void wcolsum_final_kernel(const double* partial, int nblk, int ncols, T* v) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncols) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partial[(int64_t)b * ncols + c];
  v[c] = (T)s;
}
// out(i, c) -= scale * (u ? u[i] : 1) * v[c]
template <class T>
__global__ void rank1_sub_kernel(T* out, int64_t ld, int64_t rows, const T* __restrict__ u, const T* __restrict__ v,
                                 const T* __restrict__ scale) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  const T sc = scale ? *scale : (T)1;
  out[(int64_t)blockIdx.y * ld + i] -= sc * (u ? u[i] : (T)1) * v[blockIdx.y];
}
// out(i, c) = d[i] * in(i, c): the diagonal of the standardised operator on the skinny side (in and out share ld; out may
// be in)
template <class T>
__global__ void row_scale_kernel(const T* in, T* out, int64_t ld, int64_t rows, const T* __restrict__ d) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  const int64_t o = (int64_t)blockIdx.y * ld + i;
  out[o] = d[i] * in[o];
}

// ---- sign convention of the singular triplets ---------------------------------------------------
// The reference leaves the signs of (u_i, v_i) to faer's SVD.  Here triplet i is normalised so that the
// largest-magnitude component (first one on ties) of column i of the SHORT-side factor V_tall (n_t rows,
// replicated on every rank of a sharded run) is positive.  One workgroup per column finds the sign, then
// both factors are flipped.
// One workgroup per column finds the sign and flips its column of both factors (one launch: round 2 used a sign kernel
// and two apply kernels, 27 us of the C2 step's tail).
template <class T>
__global__ __launch_bounds__(256) void column_sign_apply_kernel(T* v, int64_t ld, int64_t rows, T* other, int64_t ld_o, int64_t rows_o) {
  const int j = blockIdx.x;
  T* col = v + (int64_t)j * ld;
  T best = (T)-1;
  int64_t best_i = 0;
  for (int64_t i0 = threadIdx.x; i0 < rows; i0 += 8 * (int64_t)blockDim.x) {  // eight loads in flight
    // (clamped, unconditional loads: behind a branch each one gets an s_waitcnt vmcnt(0) of its own)
    T a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t i = i0 + u * (int64_t)blockDim.x;
      a[u] = col[i < rows ? i : rows - 1];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = i0 + u * (int64_t)blockDim.x < rows ? (T)fabs(a[u]) : (T)-1;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (a[u] > best) {  // increasing i: the first maximum wins
        best = a[u];
        best_i = i0 + u * (int64_t)blockDim.x;
      }
  }
  __shared__ T sb[256];
  __shared__ int64_t si[256];
  __shared__ int flip;
  sb[threadIdx.x] = best;
  si[threadIdx.x] = best_i;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      const T ob = sb[threadIdx.x + off];
      const int64_t oi = si[threadIdx.x + off];
      if (ob > sb[threadIdx.x] || (ob == sb[threadIdx.x] && oi < si[threadIdx.x])) {
        sb[threadIdx.x] = ob;
        si[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) flip = (sb[0] > (T)0 && col[si[0]] < (T)0) ? 1 : 0;
  __syncthreads();
  if (!flip) return;
  for (int64_t i = threadIdx.x; i < rows; i += blockDim.x) col[i] = -col[i];
  T* oc = other + (int64_t)j * ld_o;
  for (int64_t i = threadIdx.x; i < rows_o; i += blockDim.x) oc[i] = -oc[i];
}

// ---- layout helpers --------------------------------------------------------------------------
// dst[r * ldd + c] = src[r * rs + c * cs]   (repack any strided matrix to padded row-major)
template <class T>
__global__ void pack_strided_kernel(const T* src, int64_t rows, int64_t cols, int64_t rs, int64_t cs, T* dst, int64_t ldd,
                                    int64_t tiles_c) {
  __shared__ T tile[32][33];
  // 32x32 tiles through LDS so both sides stay coalesced whichever stride is the unit one
  const int64_t r0 = ((int64_t)blockIdx.x / tiles_c) * 32, c0 = ((int64_t)blockIdx.x % tiles_c) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: ty = 0..7
  const bool col_fast = cs <= rs;
  for (int q = ty; q < 32; q += 8) {
    // read with the fast source direction on tx
    const int64_t r = col_fast ? r0 + q : r0 + tx;
    const int64_t c = col_fast ? c0 + tx : c0 + q;
    if (r < rows && c < cols) tile[r - r0][c - c0] = src[r * rs + c * cs];
  }
  __syncthreads();
  for (int q = ty; q < 32; q += 8) {
    const int64_t r = r0 + q, c = c0 + tx;
    if (r < rows && c < cols) dst[r * ldd + c] = tile[q][tx];
  }
}
// dst (col-major, ldd) <- src (col-major skinny, lds): plain copy or transpose
template <class T>
__global__ void copy_out_kernel(const T* src, int64_t lds_, int64_t rows, int64_t cols, T* dst, int64_t ldd, int transpose,
                                int64_t tiles_c) {
  __shared__ T tile[32][33];
  const int64_t r0 = ((int64_t)blockIdx.x / tiles_c) * 32, c0 = ((int64_t)blockIdx.x % tiles_c) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  if (!transpose) {
    for (int q = ty; q < 32; q += 8) {
      const int64_t r = r0 + tx, c = c0 + q;
      if (r < rows && c < cols) dst[c * ldd + r] = src[c * lds_ + r];
    }
    return;
  }
  for (int q = ty; q < 32; q += 8) {
    const int64_t r = r0 + tx, c = c0 + q;
    if (r < rows && c < cols) tile[q][tx] = src[c * lds_ + r];
  }
  __syncthreads();
  // dst is cols x rows column-major: dst[r * ldd + c]
  for (int q = ty; q < 32; q += 8) {
    const int64_t r = r0 + q, c = c0 + tx;
    if (r < rows && c < cols) dst[r * ldd + c] = tile[tx][q];
  }
}

}  // namespace k
}  // namespace corrla
