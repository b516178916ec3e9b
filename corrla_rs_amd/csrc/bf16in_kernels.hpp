// Dense bfloat16 INPUT: the tall products of the range finder (random_svd.rs:31, 42-51, 80) for a matrix A that is STORED in
// bf16.  A is read from HBM at 2 bytes per element, once per product, and is never widened or copied.
//
// gemm_bf16a_kernel<NT, false>:  Out (M x L, col-major f32) = R (M x K, row-major bf16) * X (K x L)
// gemm_bf16a_kernel<NT, true >:  Out (K x L, col-major f32) = R^T * X (M x L)
//
// Why three products.  mixed_kernels.hpp splits BOTH f32 operands into bf16 pieces (hi, mid, lo) and needs six MFMAs per
// step.  A value stored in bf16 IS one piece: there is nothing to split, and
//     r x  =  r lo' + r mid' + r hi'  + O(2^-27 |r x|)
// with every product of two 8-bit significands exact in the f32 accumulator -- the f32 product to f32 rounding from three
// v_mfma_f32_16x16x32_bf16 per step and no VALU work on R at all.  The terms are added smallest first, as in mx_products.
//
// What is kept from gemm_bf16s_kernel: the workgroup (8 MFMA waves of two 16-wide outer tiles each + 4 loader waves, 256
// outer indices, all NT <= 9 column tiles), the planes of X written once per product by split_planes_kernel, LDS-DMA
// staging with counted vmcnt waits, the slab output (slab_reduce) of a split reduction, run_if, the scale epilogue and
// mx_store.  What differs:
//   * a 32-deep tile of R is 16 KiB; the big ring has 4 slots (three tiles ahead) and the plane ring 3 (two ahead), so the
//     counted wait of a tile leaves TWO big tiles = 32 KiB per CU in flight, what the f32 kernel has with one;
//   * the reduction index of a fragment is in MEMORY order (k = 8 g + j), so the planes use the identity map
//     (split_planes_kernel<3, false>), not mx_kmap;
//   * nn: a lane's 8 reduction indices are 8 consecutive bf16 of one row of R = ONE ds_read_b128.  The image is 256 rows of
//     64 bytes -- the geometry of a plane image, and it takes the plane image's swizzle (mx_plane_swz);
//   * tn: the reduction index runs DOWN the rows of the image (32 rows of 512 bytes = 256 outer columns).  Two
//     ds_read_b64_tr_b16 per fragment: the 16 lanes of group g fetch the 4 x 16 block of rows 8 g .. 8 g + 3 (then + 4) of
//     the tile's 16 outer columns and each lane receives ITS column (cdna_hip_programming.md 5.5 T10).  Every lane of an
//     MFMA wave is active at these reads (the wave-uniform branches above them are the only ones) and every address is a
//     multiple of 8 bytes.  A 32-lane half reads rows {8 g + q} of two groups g: eight rows 512 bytes apart, i.e. on the
//     same banks; the swizzle  physical 32-byte block = logical ^ ba_tn_swz(row)  spreads them over the eight 32-byte
//     blocks of a 256-byte bank line (tools/lds_layout_check.py replays both images).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mixed_kernels.hpp"

namespace corrla {
namespace k {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef MxArgsT<uint16_t> BaArgs;  // r: bf16 bit patterns; r_ld, r_cols_readable in 2-byte elements

// tn image: 32-byte block index (16 outer columns) of reduction row kr is XORed with this
__host__ __device__ constexpr int ba_tn_swz(int kr) { return (kr & 3) | ((kr >> 1) & 4); }

__device__ __forceinline__ s16x4 ba_read_tr(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}

// the three products of one (row tile, column tile, 32-deep step): smallest terms first (b: hi, mid, lo)
__device__ __forceinline__ f32x4 ba_products(const bf16x8& a, const bf16x8 (&b)[kBaPlanes], f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[0], c, 0, 0, 0);
  return c;
}

// ---------------------------------------------------------------------------------------------------------------------
// TN = false:  grid = (ceil(R_rows / 256), 1, nsplit), reduction over the columns of R
// TN = true :  grid = (ceil(R_cols / 256), 1, nsplit), reduction over the rows of R
// Big image of a stage (16 KiB, 1-KiB DMA chunks):
//   nn: 256 outer rows x 64 bytes (32 reduction indices);  chunk c = rows 16 c .. 16 c + 15, lane -> (row 16 c + lane / 4,
//       physical 16-byte slot lane & 3 = logical ^ mx_plane_swz(row))
//   tn: 32 reduction rows x 512 bytes (256 outer columns);  chunk c = rows 2 c, 2 c + 1, lane -> (row 2 c + lane / 32,
//       physical 16-byte slot lane & 31; its 32-byte block (lane & 31) / 2 = logical ^ ba_tn_swz(row))
// Plane images: as in gemm_bf16s_kernel.
// ---------------------------------------------------------------------------------------------------------------------
template <int NT, bool TN>
__global__ __launch_bounds__(64 * (kMxWaves + kMxLoaders), 3) void gemm_bf16a_kernel(BaArgs g) {
  constexpr int NP = kBaPlanes;
  constexpr int PLANE = mx_plane_bytes(NT);
  constexpr int BSLOT = ba_bslot_bytes(NT);
  constexpr int BRING = kBaASlots * kBaBigBytes;  // byte offset of the plane ring
  static_assert(ba_lds_bytes(kMaxColTiles) <= 160 * 1024, "LDS budget");
  static_assert(kMxKT == 32 && kMxOuter == 256, "the images below are laid out for 32 x 256 tiles");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if (g.run_if && *g.run_if == 0) return;  // uniform over the grid
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t outer_first = (int64_t)blockIdx.x * kMxOuter;
  const int t_begin = blockIdx.z * g.tiles_per_split;
  const int t_end = min(t_begin + g.tiles_per_split, g.tiles_total);
  const int nk = t_end - t_begin;

  if (wave >= kMxWaves) {
    // ---- loader waves: chunks of 1 KiB dealt round-robin; every loader issues the same number of DMA instructions per
    // tile and ring (the short ones add a dummy into the scratch KiB), so the counted waits are uniform.
    __builtin_amdgcn_s_setprio(3);
    const int lw = wave - kMxWaves;
    constexpr int NBIG = kBaBigBytes / 1024;                        // 16 chunks of the big operand per tile
    constexpr int DA = NBIG / kMxLoaders;                           // 4 per loader
    constexpr int NSK = NP * NT;                                    // plane chunks per tile
    constexpr int DB = (NSK + kMxLoaders - 1) / kMxLoaders;         // per loader (padded)
    static_assert(2 * DA + DB <= 63, "vmcnt is a 6-bit counter");
    char* scratch = smem + BRING + kBaBSlots * BSLOT;
    auto stage_big = [&](int i) {
      char* st = smem + (i % kBaASlots) * kBaBigBytes;
      const int64_t k0 = (int64_t)(t_begin + i) * kMxKT;
#pragma unroll
      for (int q = 0; q < DA; ++q) {
        const int c = lw + kMxLoaders * q;
        const uint16_t* src;
        if constexpr (!TN) {
          const int row = 16 * c + (lane >> 2);
          const int ls = (lane & 3) ^ mx_plane_swz(row);
          const int64_t grow = outer_first + row, kk = k0 + 8 * ls;
          src = (grow < g.r_rows && kk < g.r_cols_readable) ? g.r + grow * g.r_ld + kk : (const uint16_t*)g.zero;
        } else {
          const int kr = 2 * c + (lane >> 5);  // reduction row of the tile
          const int sp = lane & 31;
          const int lb = (sp >> 1) ^ ba_tn_swz(kr);
          const int64_t grow = k0 + kr, oc = outer_first + 16 * lb + 8 * (sp & 1);
          src = (grow < g.r_rows && oc < g.r_cols_readable) ? g.r + grow * g.r_ld + oc : (const uint16_t*)g.zero;
        }
        glds16(src, st + c * 1024);
      }
    };
    auto stage_planes = [&](int i) {
      char* st = smem + BRING + (i % kBaBSlots) * BSLOT;
      const int64_t k0 = (int64_t)(t_begin + i) * kMxKT;
#pragma unroll
      for (int q = 0; q < DB; ++q) {
        const int cc = lw + kMxLoaders * q;
        if (cc >= NSK) {
          glds16(g.zero, scratch);  // keeps the per-tile DMA count uniform over the loaders
          continue;
        }
        const int p = cc / NT, ct = cc - p * NT;
        const int row = 16 * ct + (lane >> 2);
        const int ls = (lane & 3) ^ mx_plane_swz(row);
        glds16(g.planes + p * g.plane_stride + (int64_t)row * g.x_ld + k0 + 8 * ls, st + p * PLANE + ct * 1024);
      }
    };
    // issue order (vmcnt retires in order):  A(0) B(0) A(1) B(1) A(2) | then per tile i, after its barrier:  B(i+2) A(i+3).
    // Before barrier i the planes B(i) and the big tile A(i) (older than B(i)) must have landed; what was issued after
    // B(i) -- A(i+1), B(i+1), A(i+2), as far as those tiles exist -- may stay in flight.
    if (nk > 0) {
      stage_big(0);
      stage_planes(0);
      if (nk > 1) {
        stage_big(1);
        stage_planes(1);
      }
      if (nk > 2) stage_big(2);
    }
    for (int i = 0; i < nk; ++i) {
      if (i + 2 < nk)
        wait_vmcnt<2 * DA + DB>();
      else if (i + 1 < nk)
        wait_vmcnt<DA + DB>();
      else
        wait_vmcnt<0>();
      wg_barrier();  // tile i visible to the MFMA waves; they are done with tile i - 1 (its slots are free)
      if (i + 2 < nk) stage_planes(i + 2);  // slot of B(i - 1)
      if (i + 3 < nk) stage_big(i + 3);     // slot of A(i - 1)
    }
    return;
  }

  // ---- MFMA waves -------------------------------------------------------------------------------------------------
  const int fr = lane & 15, fg = lane >> 4;
  f32x4 acc[kMxRowTiles][NT];
#pragma unroll
  for (int mw = 0; mw < kMxRowTiles; ++mw)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[mw][t] = (f32x4){0, 0, 0, 0};
  // byte offsets inside a stage.  Row tile mw of wave w holds outer indices 32 w + 16 mw + (0 .. 15).
  //   nn: row 32 w + 16 mw + fr, logical slot fg (reduction indices 8 fg .. 8 fg + 7); the swizzle only depends on fr
  //   tn: lane 4 q + p of group fg addresses row 8 fg + q (then + 4: same swizzle, + 2048 bytes), columns 4 p .. 4 p + 3
  //       of the tile's 32-byte block 2 w + mw, and receives column fr of the four rows
  unsigned a_off[kMxRowTiles];
#pragma unroll
  for (int mw = 0; mw < kMxRowTiles; ++mw) {
    if constexpr (!TN) {
      a_off[mw] = (unsigned)((32 * wave + 16 * mw + fr) * 64 + ((fg ^ mx_plane_swz(fr)) << 4));
    } else {
      const int kr = 8 * fg + (fr >> 2);
      a_off[mw] = (unsigned)(kr * 512 + (((2 * wave + mw) ^ ba_tn_swz(kr)) << 5) + ((fr & 3) << 3));
    }
  }
  const unsigned b_base = (unsigned)(fr * 64 + ((fg ^ mx_plane_swz(fr)) << 4));  // inside a slot of the plane ring
  int abuf = 0, bbuf = 0;
  for (int i = 0; i < nk; ++i) {
    wg_barrier();  // matches the loaders' barrier: tile i is in LDS
    const char* st = smem + abuf * kBaBigBytes;    // big-operand slot
    const char* sb = smem + BRING + bbuf * BSLOT;  // plane slot
    bf16x8 af[kMxRowTiles];
#pragma unroll
    for (int mw = 0; mw < kMxRowTiles; ++mw) {
      if constexpr (!TN) {
        af[mw] = *(const bf16x8*)(st + a_off[mw]);
      } else {
        const s16x4 lo = ba_read_tr(st + a_off[mw]);
        const s16x4 hi = ba_read_tr(st + a_off[mw] + 4 * 512);
        af[mw] = __builtin_bit_cast(bf16x8, (s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
      }
    }
    // the plane fragments of a column tile are read one tile ahead of their six MFMAs
    bf16x8 bn[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) bn[p] = *(const bf16x8*)(sb + b_base + p * PLANE);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      bf16x8 bc[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) bc[p] = bn[p];
      if (t + 1 < NT) {
#pragma unroll
        for (int p = 0; p < NP; ++p) bn[p] = *(const bf16x8*)(sb + b_base + (t + 1) * 1024 + p * PLANE);
      }
#pragma unroll
      for (int mw = 0; mw < kMxRowTiles; ++mw) acc[mw][t] = ba_products(af[mw], bc, acc[mw][t]);
    }
    abuf = abuf + 1 == kBaASlots ? 0 : abuf + 1;
    bbuf = bbuf + 1 == kBaBSlots ? 0 : bbuf + 1;
  }
  const int64_t limit = TN ? g.r_cols : g.r_rows;
#pragma unroll
  for (int mw = 0; mw < kMxRowTiles; ++mw) mx_store<NT, NP>(g, acc[mw], outer_first + 32 * wave + 16 * mw, limit, lane);
}

// ---- fallback: a strided bf16 view -> zero-padded row-major f32 (the bf16 twin of pack_strided_kernel) ---------------------
// dst[r * ldd + c] = widen(src[r * rs + c * cs]); bf16 -> f32 is exact (the bit pattern moves to the upper half)
__global__ void widen_bf16_kernel(const uint16_t* src, int64_t rows, int64_t cols, int64_t rs, int64_t cs, float* dst, int64_t ldd,
                                  int64_t tiles_c) {
  __shared__ uint16_t tile[32][33];
  // 32x32 tiles through LDS so both sides stay coalesced whichever stride is the unit one
  const int64_t r0 = ((int64_t)blockIdx.x / tiles_c) * 32, c0 = ((int64_t)blockIdx.x % tiles_c) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: ty = 0..7
  const bool col_fast = cs <= rs;
  for (int q = ty; q < 32; q += 8) {
    const int64_t r = col_fast ? r0 + q : r0 + tx;
    const int64_t c = col_fast ? c0 + tx : c0 + q;
    if (r < rows && c < cols) tile[r - r0][c - c0] = src[r * rs + c * cs];
  }
  __syncthreads();
  for (int q = ty; q < 32; q += 8) {
    const int64_t r = r0 + q, c = c0 + tx;
    if (r < rows && c < cols) dst[r * ldd + c] = __builtin_bit_cast(float, (unsigned)tile[q][tx] << 16);
  }
}

}  // namespace k
}  // namespace corrla
