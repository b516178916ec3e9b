// The tall products' plans (tall_stage.hpp launches what they say and computes none of it again).  gemm_plan: which
// kernel family and instantiation serves a product (gemm_nn / gemm_tn / gemm_mixed / gemm_bf16a), its launches (grid, column
// base, XCD remap, dynamic LDS), the reduction split and the slab reduction that sums it -- or why the call is rejected.
// ata_plan: the one-sweep A^T (A Z).  spmm_plan: the CSR product.  With them the LDS and geometry arithmetic those choices
// rest on, the layout of a padded skinny matrix, and the list of instantiations each kernel family has.
// Host code only, no HIP call: tests/test_gemm_plan.py, tests/test_gemm_plan_bf16.py and tests/test_tall_stage_plan.py
// compile this header with the host compiler and pin the plans.  The kernels that use the size helpers on the device include
// it through hip_kernels.hpp (which tall_kernels.hpp, mixed_kernels.hpp and ata_kernels.hpp include) or directly
// (spmm_kernels.hpp); driver.hpp takes the column blocking and kLdPad from it.
//
// Families.  GENERAL: gemm_nn_kernel / gemm_tn_kernel<T, MW, NT, NW> (hip_kernels.hpp), any shape.  GRAM ALIAS: the
// aliased gemm_nn_kernel<T, 2, NT, true> for G = Y^T Y with l <= 128.  TALL APPLY / TALL GRAM: the register-resident
// kernels of tall_kernels.hpp for Y M and Y^T Y of a very tall sketch with l <= 96 (f32) / 64 (f64).  BF16 SPLIT:
// gemm_bf16s_kernel<NT, NP, TN> (mixed_kernels.hpp), only when the caller asks for NP = 2 / 3 planes.  BF16 STORED:
// gemm_bf16a_kernel<NT, TN> (bf16in_kernels.hpp), whenever the big operand is stored in bfloat16 (no size threshold).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>

#include "core_svd_plan.hpp"  // kLdsMaxBytes, CORRLA_HD

namespace corrla {

// Skinny operands are padded to the column blocking: `tiles` 16-column MFMA tiles in `nblk` workgroup column blocks of
// at most kMaxColTiles tiles (144 columns), `nt` tiles in the widest block.
constexpr int kMaxColTiles = 9;

struct ColBlocking {
  int tiles, nblk, nt;
  int64_t cols_alloc;
};
inline ColBlocking col_blocking(int64_t cols) {
  ColBlocking b;
  b.tiles = (int)std::max<int64_t>(1, (cols + 15) / 16);
  b.nblk = (b.tiles + kMaxColTiles - 1) / kMaxColTiles;
  b.nt = (b.tiles + b.nblk - 1) / b.nblk;
  b.cols_alloc = (int64_t)b.nblk * b.nt * 16;
  return b;
}

// A skinny matrix (driver.hpp: Skinny) of rows x cols as the backend allocates it: the leading dimension padded to kLdPad
// elements, the column count to the column blocking.
constexpr int kLdPad = 64;
struct SkinnyLayout {
  int64_t ld, cols_alloc;
};
inline SkinnyLayout skinny_layout(int64_t rows, int64_t cols) {
  return {(std::max<int64_t>(rows, 1) + kLdPad - 1) / kLdPad * kLdPad, col_blocking(cols).cols_alloc};
}

// ---- the instantiations of each kernel family.  tall_stage.hpp dispatches on these and registers the dynamic LDS of every
// kernel from these: a kernel that can be launched is one whose limit was set. ----
// gemm_nn_kernel<T, MW, NT, false, NW> / gemm_tn_kernel<T, MW, NT, NW>: four MFMA waves, or the f64 MW = 2 tile on eight
constexpr bool gemm_general_exists(int esz, int mw, int nt, int nw) {
  return (mw == 1 || mw == 2) && nt >= 1 && nt <= kMaxColTiles && (nw == 4 || (nw == 8 && mw == 1 && esz == 8));
}
using GeneralNWs = std::integer_sequence<int, 4, 8>;
constexpr int kAliasMaxTiles = 8;                    // gemm_nn_kernel<T, 2, NT, true>: NT 1 .. 8
constexpr int tall_max_tiles(int esz) { return esz == 4 ? 6 : 4; }  // tall_apply_kernel<T, K, K>, tall_gram_kernel<T, NCT>
constexpr int kMxMinPlanes = 2, kMxMaxPlanes = 3;    // gemm_bf16s_kernel<NT, NP, TN>: NT 1 .. kMaxColTiles, NP 2 .. 3
using AtaNKs = std::integer_sequence<int, 2, 4, 8>;  // ata_fused_kernel<NK, NCT>: NK of the list, NCT 1 .. 5
constexpr int kAtaMaxColTiles = 5;                   // (gemm_bf16a_kernel<NT, TN>: NT 1 .. kMaxColTiles)

namespace k {

// ---- general kernels (hip_kernels.hpp) ----
constexpr int kRowBytes = 256;  // LDS row of the k-contiguous images
constexpr int kLoaders = 4;     // LDS-DMA loader waves per workgroup (besides the 4 MFMA waves); must divide 4
CORRLA_HD constexpr int gemm_vec(int esz) { return 16 / esz; }        // elements per 16 bytes
CORRLA_HD constexpr int gemm_kt(int esz) { return kRowBytes / esz; }  // reduction elements per 256-byte LDS row
// A workgroup owns 64*MW outer indices (4 waves x MW 16-wide MFMA tiles each).  MW = 2 halves the
// skinny-operand bytes staged per MFMA (the per-CU global->LDS fill rate, ~11 B/clk, is what bounds
// the MW = 1 shape at 144 columns: 52 KiB per 4608 MFMA cycles); MW = 1 keeps small problems spread
// over more workgroups.
CORRLA_HD constexpr int outer_tile(int mw) { return 64 * mw; }
CORRLA_HD constexpr int big_tile_bytes(int mw) { return 64 * 256 * mw; }
CORRLA_HD constexpr int stage_bytes(int mw, int nt) { return big_tile_bytes(mw) + nt * 16 * kRowBytes; }
// LDS ring depth: 3 stages (the loaders run two tiles ahead, which hides the higher memory latency of the
// chip's low-clock state between bursts) whenever they fit in 160 KiB, else 2.
CORRLA_HD constexpr int gemm_stages(int mw, int nt) { return 3 * stage_bytes(mw, nt) <= 160 * 1024 ? 3 : 2; }
CORRLA_HD constexpr int gemm_lds_bytes(int mw, int nt) { return gemm_stages(mw, nt) * stage_bytes(mw, nt); }

// ---- tall Gram kernel (tall_kernels.hpp): rows per LDS tile, 512 bytes per column ----
template <class T>
CORRLA_HD constexpr int gram_rows() { return 512 / (int)sizeof(T); }
CORRLA_HD constexpr int gram_tile_bytes(int nct) { return 16 * nct * 512; }
CORRLA_HD constexpr int gram_stages(int nct) {
  const int s = (160 * 1024 - 4096) / gram_tile_bytes(nct);
  return s > 4 ? 4 : s;
}
CORRLA_HD constexpr int gram_lds_bytes(int nct, int esz) {
  const int ring = gram_stages(nct) * gram_tile_bytes(nct);
  const int red = 3 * (nct * (nct + 1) / 2) * 256 * esz;  // cross-wave sum of the partial tiles (waves 1..3)
  return ring > red ? ring : red;
}

// ---- bf16-split kernels (mixed_kernels.hpp) ----
constexpr int kMxWaves = 8;                  // MFMA waves per workgroup
constexpr int kMxLoaders = 4;                // LDS-DMA loader waves
constexpr int kMxRowTiles = 2;               // 16-wide outer tiles per MFMA wave
constexpr int kMxOuter = kMxWaves * kMxRowTiles * 16;  // 256 outer indices per workgroup
constexpr int kMxKT = 32;                    // reduction indices per tile (one 16x16x32 step)
constexpr int kMxBigBytes = kMxOuter * kMxKT * 4;       // 32 KiB
CORRLA_HD constexpr int mx_plane_bytes(int nt) { return nt * 16 * kMxKT * 2; }  // one plane of one tile
// Two LDS rings: the big operand comes from HBM and is prefetched TWO tiles ahead (3 slots of 32 KiB); the planes of the
// skinny operand are re-read by every workgroup, i.e. served by L2, and run one tile ahead (2 slots).  (Round 3's first
// version had one ring of whole tiles: only 2 fit for three planes, and the DMA cost 30 % on top of the DMA-free time.)
constexpr int kMxASlots = 3, kMxBSlots = 2;
CORRLA_HD constexpr int mx_bslot_bytes(int nt, int np) { return np * mx_plane_bytes(nt); }
CORRLA_HD constexpr int mx_lds_bytes(int nt, int np) { return kMxASlots * kMxBigBytes + kMxBSlots * mx_bslot_bytes(nt, np) + 1024; }

// ---- bf16-stored kernels (bf16in_kernels.hpp): the workgroup shape of the bf16-split kernels, R in 2-byte elements ----
constexpr int kBaPlanes = 3;                            // the skinny operand is always split into three bf16 pieces
constexpr int kBaBigBytes = kMxOuter * kMxKT * 2;       // 16 KiB: one 32-deep tile of R
// The big operand runs THREE tiles ahead (4 slots of 16 KiB: as many bytes of HBM latency in flight as the f32 kernel's two
// tiles of 32 KiB), the planes two ahead (3 slots), so that the counted wait of a tile leaves two big tiles in flight.
constexpr int kBaASlots = 4, kBaBSlots = 3;
CORRLA_HD constexpr int ba_bslot_bytes(int nt) { return kBaPlanes * mx_plane_bytes(nt); }
CORRLA_HD constexpr int ba_lds_bytes(int nt) { return kBaASlots * kBaBigBytes + kBaBSlots * ba_bslot_bytes(nt) + 1024; }

// ---- one-sweep A^T (A Z) (ata_kernels.hpp): a ring of up to 4 tiles of kAtaRows rows of A, then the partial T tiles ----
constexpr int kAtaRows = 16;  // rows of A per LDS tile
CORRLA_HD constexpr int ata_tile_bytes(int nk) { return kAtaRows * nk * 256; }
CORRLA_HD constexpr int ata_tpart_bytes(int nct) { return 2 * 4 * nct * 1024; }  // [parity][wave][ct][16 x 16]
CORRLA_HD constexpr int ata_stages(int nk, int nct) {
  const int s = (160 * 1024 - ata_tpart_bytes(nct)) / ata_tile_bytes(nk);
  return s > 4 ? 4 : s;
}
CORRLA_HD constexpr int ata_lds_bytes(int nk, int nct) { return ata_stages(nk, nct) * ata_tile_bytes(nk) + ata_tpart_bytes(nct); }

// ---- CSR product (spmm_kernels.hpp) ----
constexpr int kSpTile = 64;  // rows and sketch columns of one output tile

}  // namespace k

// Geometry knobs of the tall products, read once when a device context is created (hip_backend.hpp).
struct GemmKnobs {
  int split_nn = 0, split_tn = 0;      // CORRLA_SPLIT_NN / _TN: reduction split (0: by shape)
  int mw = 0;                          // CORRLA_MW: outer tile width in 64-index units (0: by shape)
  int xcd_remap = 1;                   // CORRLA_GEMM_XCD=0: plain block mapping in gemm_tn
  int64_t tall_min_rows = 65536;       // CORRLA_TALL_MIN_ROWS: rows from which the tall kernels serve (0: never)
  int persist_max_tiles = 16;          // CORRLA_GEMM_PERSIST_TILES: persistent launches up to this many tiles per split
  int f64_waves = 8;                   // CORRLA_F64_WAVES=4: f64 MW = 2 tiles on four MFMA waves
  double mixed_min_work = 16777216.0;  // CORRLA_MIXED_MIN_WORK: outer x reduction from which the bf16 split serves
  bool even_blocks = false;            // CORRLA_EVEN_BLOCKS=1: no uneven column blocking
  bool no_gram_alias = false;          // CORRLA_NO_GRAM_ALIAS=1: Gram matrices on the general kernels
  bool no_rotate = false;              // CORRLA_GEMM_NO_ROTATE=1: gemm_nn workgroups all start at the split's first tile
  int mixed_split = 0;                 // CORRLA_MIXED_SPLIT: reduction split of the bf16-split kernels (0: by shape)
};

// One product out = scale * op(R) * X without its pointers: op(R) = R (tn false) or R^T, outer_n x red_n.  R is row-major
// with cols_readable columns readable per row; X and out are column-major with cols_alloc columns allocated (zero padded
// unless external: a caller's buffer with exactly `cols` columns).
struct GemmOperand {
  int64_t rows = 0, cols = 0, ld = 0, cols_readable = 0, cols_alloc = 0;
  bool external = false, aligned = true;  // aligned: 16 bytes
};
struct GemmShape {
  bool tn = false;
  int esz = 4;  // 4: f32, 8: f64
  GemmOperand r, x, out;
  bool same = false;  // R and X are the same memory (Gram matrices)
  int np = 0;         // bf16 planes: 0 = exact products, 2 / 3 = the bf16-split kernels
  int num_cus = 256;
  bool r_bf16 = false;  // R is stored in bfloat16 (r.ld, r.cols_readable in 2-byte elements); X and out stay f32
};

enum class GemmFamily { general, gram_alias, tall_apply, tall_gram, bf16_split, bf16_stored };
enum class SlabReduce { none, plain, deep };  // slab_reduce_kernel / slab_reduce_deep_kernel

// Sum of `slabs` partial results (stride apart) into rows x cols of the output.
struct SlabReducePlan {
  SlabReduce kind = SlabReduce::none;
  unsigned grid[2] = {0, 0};
  int slabs = 0;
  int64_t rows = 0, cols = 0;
};

struct GemmLaunch {
  unsigned grid[3] = {1, 1, 1};
  int nt = 0;            // NT (general, alias, bf16 split), K (tall apply), NCT (tall Gram)
  int64_t col_base = 0;  // first column of this launch's column blocks
  int xcd_remap = 0;
  int lds = 0;           // dynamic LDS bytes
};

struct GemmPlan {
  const char* error = nullptr;  // the call is rejected (thrown as ST_EINVAL)
  GemmFamily family = GemmFamily::general;
  int mw = 1, nw = 4, np = 0;   // instantiation: MW / NW (general, alias), NP (bf16 split)
  int block = 256;              // threads per workgroup
  int nlaunch = 0;
  GemmLaunch launch[2];
  int tiles_total = 0, nsplit = 1, tiles_per_split = 0, outer_blocks = 0, rotate = 0, vec_store = 0;
  int64_t out_cols = 0;         // columns of the output the product may write
  int64_t slab_stride = 0;      // elements between partial results
  size_t slab_bytes = 0;        // workspace of the partial results (none when reduce.kind == none)
  SlabReducePlan reduce;
  int64_t rows_per_group = 0, groups = 0;  // tall Gram: row groups, one partial Gram each
  int64_t plane_stride = 0, plane_cols = 0;  // bf16 split: plane_cols columns of X in np planes of plane_stride bf16 ...
  size_t plane_bytes = 0;
  unsigned split_grid = 0;      // ... written by split_planes_kernel<NP> on this many workgroups
};

// The bf16-split kernels' domain: row-major f32 R, one column block (<= 144 columns), vector-aligned operands, a product
// of at least mixed_min_work outer x reduction elements, and no Gram product (those stay exact).
inline bool gemm_mixed_domain(const GemmShape& s, const GemmKnobs& kn) {
  const int64_t outer_n = s.tn ? s.r.cols : s.r.rows, red_n = s.tn ? s.r.rows : s.r.cols;
  if (s.esz != 4 || s.x.external || col_blocking(s.x.cols).nblk != 1) return false;
  if (!s.r.aligned || (s.r.ld % 4) || (s.r.cols_readable % 4) || !s.x.aligned || (s.x.ld % 64)) return false;
  if (s.x.ld < (red_n + k::kMxKT - 1) / k::kMxKT * k::kMxKT || s.out.ld < outer_n || s.out.rows != outer_n) return false;
  if (s.same) return false;
  return outer_n >= 1 && red_n >= 1 && (double)outer_n * (double)red_n >= kn.mixed_min_work;
}

// The bf16-stored kernels' domain: row-major bf16 R (unit stride along its memory rows) with a 16-byte aligned base, a
// leading dimension and a readable row length that are multiples of 8 elements, f32 X and out in the padded layout, one
// column block (<= 144 columns).  No size threshold: every product in the domain takes the kernel.
inline bool gemm_bf16a_domain(const GemmShape& s) {
  const int64_t outer_n = s.tn ? s.r.cols : s.r.rows, red_n = s.tn ? s.r.rows : s.r.cols;
  if (!s.r_bf16 || s.esz != 4 || s.x.external || col_blocking(s.x.cols).nblk != 1) return false;
  if (!s.r.aligned || (s.r.ld % 8) || (s.r.cols_readable % 8) || !s.x.aligned || (s.x.ld % 64)) return false;
  if (s.x.ld < (red_n + k::kMxKT - 1) / k::kMxKT * k::kMxKT || s.out.ld < outer_n || s.out.rows != outer_n) return false;
  if (s.same) return false;
  return outer_n >= 1 && red_n >= 1;
}

namespace gemm_plan_detail {

inline bool grid_fits(unsigned y, unsigned z) { return y <= 65535u && z <= 65535u; }
inline bool padding_fits(const GemmShape& s, const ColBlocking& cb) {
  return cb.cols_alloc <= s.x.cols_alloc && (s.out.external ? s.out.cols >= s.x.cols : cb.cols_alloc <= s.out.cols_alloc);
}
inline GemmPlan rejected(GemmPlan p, const char* why) {
  p.error = why;
  return p;
}

// nsplit >= 8 slabs: the deep reduction (64 rows per workgroup), else the plain one (256)
inline bool plan_reduce(GemmPlan& p, int64_t outer_n, int64_t cols_alloc) {
  if (p.nsplit <= 1) return true;
  const bool deep = p.nsplit >= 8;
  const unsigned rows_per_wg = deep ? 64 : 256;
  p.reduce = {deep ? SlabReduce::deep : SlabReduce::plain,
              {(unsigned)((outer_n + rows_per_wg - 1) / rows_per_wg), (unsigned)cols_alloc}, p.nsplit, outer_n, p.out_cols};
  return grid_fits(p.reduce.grid[1], 1);
}

// Y M (tn) and Y^T Y (nn) of a very tall sketch on the register-resident kernels; false: not theirs
inline bool plan_tall(const GemmShape& s, const GemmKnobs& kn, int64_t outer_n, int64_t red_n, GemmPlan& p) {
  const int kMaxL = 16 * tall_max_tiles(s.esz);  // 96 / 64: register budget of the B fragments
  const int vec = k::gemm_vec(s.esz);
  if (kn.tall_min_rows <= 0) return false;
  if (s.tn) {
    // out (m x n2) = R^T X with R = Y^T stored row-major kdim x m: the columns of Y are contiguous
    const int64_t m = outer_n, kdim = red_n, n2 = s.x.cols;
    if (kdim > kMaxL || n2 > kMaxL || m < kn.tall_min_rows || s.r.ld < (m + 63) / 64 * 64 || s.x.ld < kdim) return false;
    if (s.out.cols < n2) {
      p.error = "internal: gemm output shape mismatch";
      return true;
    }
    const int kt = (int)std::max((kdim + 15) / 16, (n2 + 15) / 16);
    p.family = GemmFamily::tall_apply;
    p.out_cols = s.out.external ? s.out.cols : std::min<int64_t>(s.out.cols_alloc, 16 * kt);
    p.vec_store = ((s.out.ld % vec) == 0 && s.out.aligned) ? 1 : 0;
    const int64_t nblocks = (m + 16 * vec - 1) / (16 * vec);
    p.nlaunch = 1;
    p.launch[0] = {{(unsigned)std::min<int64_t>((nblocks + 3) / 4, s.num_cus), 1, 1}, kt, 0, 0, 0};
    return true;
  }
  // G (l x l) = Y^T Y: both operands are the same column-major m x l memory
  const int64_t l = outer_n;
  const int nct = (int)((l + 15) / 16);
  if (!s.same || s.r.ld != s.x.ld || l != s.x.cols || l > kMaxL || red_n < kn.tall_min_rows || s.out.external) return false;
  if (s.out.ld < 16 * nct || s.out.cols_alloc < 16 * nct) return false;
  const int rows_tile = s.esz == 4 ? k::gram_rows<float>() : k::gram_rows<double>();
  const int64_t rows = s.x.ld;  // the padding rows are zero and may be read
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>(s.num_cus, rows / (4 * rows_tile)));
  p.family = GemmFamily::tall_gram;
  p.rows_per_group = ((rows + want - 1) / want + rows_tile - 1) / rows_tile * rows_tile;
  p.groups = (rows + p.rows_per_group - 1) / p.rows_per_group;
  p.slab_stride = s.out.ld * s.out.cols_alloc;
  p.slab_bytes = (size_t)p.groups * (size_t)p.slab_stride * s.esz;
  p.nlaunch = 1;
  p.launch[0] = {{(unsigned)p.groups, 1, 1}, nct, 0, 0, k::gram_lds_bytes(nct, s.esz)};
  p.reduce = {SlabReduce::deep, {(unsigned)((l + 63) / 64), (unsigned)(16 * nct)}, (int)p.groups, l, 16 * nct};
  return true;
}

// What the bf16-split and the bf16-stored kernels share: the np planes of the skinny operand, 32-deep reduction tiles,
// one workgroup per 256 outer indices and CU (`lds` bytes of LDS), the reduction split that fills the chip
inline GemmPlan plan_mx_launch(GemmPlan p, const GemmShape& s, int64_t outer_n, int64_t red_n, const ColBlocking& cb, int lds,
                               int split_override) {
  if (!padding_fits(s, cb)) return rejected(p, "internal: skinny column padding too small for the column blocking");
  // the skinny operand in np bf16 planes
  p.plane_cols = cb.cols_alloc;
  p.plane_stride = s.x.ld * cb.cols_alloc;
  p.plane_bytes = (size_t)p.np * (size_t)p.plane_stride * 2;
  p.split_grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (p.plane_stride / 8 + 255) / 256));
  const int64_t tiles64 = (red_n + k::kMxKT - 1) / k::kMxKT;
  if (tiles64 > 0x7fffffff) return rejected(p, "reduction dimension too large");
  p.tiles_total = (int)tiles64;
  const int64_t outer_tiles = (outer_n + k::kMxOuter - 1) / k::kMxOuter;
  if (outer_tiles > 0x7fffffff) return rejected(p, "outer dimension too large");
  // one workgroup per CU (120-155 KB of LDS): split the reduction until the grid fills the chip
  int nsplit = 1;
  if (outer_tiles < s.num_cus)
    nsplit = (int)std::min<int64_t>((s.num_cus + outer_tiles / 2) / outer_tiles, std::max(1, p.tiles_total / 16));
  if (split_override) nsplit = split_override;
  p.nsplit = std::max(1, std::min(std::min(nsplit, p.tiles_total), 65535));
  p.tiles_per_split = (p.tiles_total + p.nsplit - 1) / p.nsplit;
  p.outer_blocks = (int)outer_tiles;
  p.out_cols = s.out.external ? s.out.cols : cb.cols_alloc;
  p.vec_store = ((s.out.ld % 4) == 0 && s.out.aligned) ? 1 : 0;
  p.slab_stride = s.out.ld * cb.cols_alloc;
  if (p.nsplit > 1) p.slab_bytes = (size_t)p.nsplit * (size_t)p.slab_stride * 4;
  p.nlaunch = 1;
  p.launch[0] = {{(unsigned)outer_tiles, 1, (unsigned)p.nsplit}, cb.nt, 0, 0, lds};
  if (!plan_reduce(p, outer_n, cb.cols_alloc)) p.error = "problem too large for the launch grid";
  return p;
}

inline GemmPlan plan_bf16_split(const GemmShape& s, const GemmKnobs& kn, int64_t outer_n, int64_t red_n,
                                const ColBlocking& cb) {
  GemmPlan p;
  p.family = GemmFamily::bf16_split;
  p.np = s.np;
  p.block = 64 * (k::kMxWaves + k::kMxLoaders);
  if (s.np != 2 && s.np != 3) return rejected(p, "internal: bf16 split takes 2 or 3 planes");
  if (!gemm_mixed_domain(s, kn)) return rejected(p, "internal: operands outside the bf16-split kernels' domain");
  return plan_mx_launch(p, s, outer_n, red_n, cb, k::mx_lds_bytes(cb.nt, s.np), kn.mixed_split);
}

// R stored in bfloat16: gemm_bf16a_kernel<NT, TN>, X in three planes whose reduction index is in memory order
inline GemmPlan plan_bf16_stored(const GemmShape& s, int64_t outer_n, int64_t red_n, const ColBlocking& cb) {
  GemmPlan p;
  p.family = GemmFamily::bf16_stored;
  p.np = k::kBaPlanes;
  p.block = 64 * (k::kMxWaves + k::kMxLoaders);
  if (!gemm_bf16a_domain(s)) return rejected(p, "internal: operands outside the bf16-stored kernels' domain");
  return plan_mx_launch(p, s, outer_n, red_n, cb, k::ba_lds_bytes(cb.nt), 0);
}

}  // namespace gemm_plan_detail

inline GemmPlan gemm_plan(const GemmShape& s, const GemmKnobs& kn) {
  using namespace gemm_plan_detail;
  const int64_t outer_n = s.tn ? s.r.cols : s.r.rows, red_n = s.tn ? s.r.rows : s.r.cols;
  const ColBlocking cb = col_blocking(s.x.cols);
  if (s.r_bf16) return plan_bf16_stored(s, outer_n, red_n, cb);
  if (s.np) return plan_bf16_split(s, kn, outer_n, red_n, cb);
  GemmPlan p;
  const int vec = k::gemm_vec(s.esz), kt = k::gemm_kt(s.esz);
  if (s.x.external) return rejected(p, "internal: an external buffer cannot be a padded operand");
  if (!padding_fits(s, cb)) return rejected(p, "internal: skinny column padding too small for the column blocking");
  if (s.out.rows != outer_n || s.out.ld < outer_n) return rejected(p, "internal: gemm output shape mismatch");
  if (!s.r.aligned || (s.r.ld % vec) || (s.r.cols_readable % vec) || !s.x.aligned)
    return rejected(p, "internal: operand not 16-byte vector aligned");
  if (plan_tall(s, kn, outer_n, red_n, p)) return p;
  const int64_t tiles64 = (red_n + kt - 1) / kt;
  if (tiles64 > 0x7fffffff) return rejected(p, "reduction dimension too large");
  p.tiles_total = (int)tiles64;
  if (s.x.ld < (int64_t)p.tiles_total * kt) return rejected(p, "internal: skinny leading dimension too small");

  // Uneven column blocking: `tiles` 16-column tiles over nblk blocks need not all be cb.nt wide -- 17 tiles (l = 266)
  // are 9 + 8, not 9 + 9: the narrower blocks run the next-smaller instantiation in a second launch and skip the
  // all-zero padding tile (5.5 % of the MFMA work of every tall product at l = 266).  Only where it pays: the second
  // launch costs ~10 us, the skipped tile 1/18 of a product's time.
  const int n_wide = cb.tiles - cb.nblk * (cb.nt - 1);  // column blocks that really have cb.nt tiles
  const bool uneven = cb.nblk > 1 && n_wide < cb.nblk && cb.nt >= 2 && !kn.even_blocks &&
                      (double)outer_n * (double)red_n * (double)cb.cols_alloc >= 1.0e10;
  // Gram matrix G = Y^T Y: both operands are the same memory and one outer tile (MW = 2: 128 indices) holds every
  // column -> the aliased instantiation stages Y once per tile
  const bool alias = !s.tn && s.same && s.r.ld == s.x.ld && cb.nblk == 1 && outer_n <= 128 && cb.nt <= kAliasMaxTiles &&
                     outer_n == s.x.cols && !kn.no_gram_alias;

  // MW (16-wide outer tiles per wave) and nsplit (split of the reduction into slabs).  One workgroup is resident per CU
  // at the large column blockings, so aim for >= num_cus workgroups; prefer the MW = 2 shape (fewer skinny-operand bytes
  // per MFMA) whenever the reduction is long enough to make up the workgroup count by splitting it.  The two launches
  // of an uneven blocking must each fill the chip: the split is sized for the blocks of ONE launch.
  int mw = 2, nsplit;
  if (alias) {
    nsplit = (int)std::min<int64_t>(std::max(1, p.tiles_total / 4), 2 * (int64_t)s.num_cus);
    if (kn.split_nn > 0) nsplit = std::min(kn.split_nn, p.tiles_total);
  } else {
    const int ov = s.tn ? kn.split_tn : kn.split_nn;
    mw = (outer_n >= 256 && p.tiles_total >= 8) ? 2 : 1;  // small outputs (Gram, core) use the MW = 1 instantiation
    if (kn.mw > 0) mw = kn.mw;
    const int nblk = uneven ? std::max(1, std::min(n_wide, cb.nblk - n_wide)) : cb.nblk;
    const int64_t wgs = (outer_n + 64 * mw - 1) / (64 * mw) * nblk;
    nsplit = 1;
    if (ov > 0) {
      nsplit = ov;
    } else if (wgs < s.num_cus) {
      nsplit = (int)((s.num_cus + wgs - 1) / wgs);
      if (wgs * nsplit < 2 * (int64_t)s.num_cus && wgs < s.num_cus / 4) nsplit *= 2;  // small grids: two waves of WGs
      nsplit = std::min(nsplit, std::max(1, p.tiles_total / 4));
    }
    nsplit = std::min(std::max(1, std::min(nsplit, p.tiles_total)), 65535);
  }
  const int64_t outer_tiles = (outer_n + 64 * mw - 1) / (64 * mw);
  if (outer_tiles > 0x7fffffff) return rejected(p, "outer dimension too large");

  // the instantiation: f64 MW = 2 tiles run on EIGHT MFMA waves of one row tile each (two waves per SIMD keep the f64
  // matrix pipe busier than one can: 77.8 vs 60.5 TF register-only)
  p.family = alias ? GemmFamily::gram_alias : GemmFamily::general;
  p.mw = mw == 2 ? 2 : 1;
  if (!alias && mw == 2 && s.esz == 8 && kn.f64_waves == 8) {
    p.mw = 1;
    p.nw = 8;
  }
  p.block = 64 * (p.nw + k::kLoaders);
  p.nsplit = nsplit;
  p.tiles_per_split = (p.tiles_total + nsplit - 1) / nsplit;
  p.outer_blocks = (int)outer_tiles;
  // columns this product may write: a caller's buffer has exactly `cols`; an uneven column blocking never computes the
  // all-zero tail tile, which therefore stays as allocated (zero)
  p.out_cols = s.out.external ? s.out.cols : (uneven ? (int64_t)cb.tiles * 16 : cb.cols_alloc);
  p.vec_store = ((s.out.ld % 4) == 0 && s.out.aligned) ? 1 : 0;
  p.rotate = (!s.tn && !alias && p.tiles_per_split <= 32 && p.tiles_per_split > 1 && !kn.no_rotate) ? 1 : 0;
  p.slab_stride = s.out.ld * cb.cols_alloc;
  if (nsplit > 1) p.slab_bytes = (size_t)nsplit * (size_t)p.slab_stride * s.esz;

  // Short reductions (A Z with n = 512: 8 tiles; Y R^-1: 2): a workgroup per outer tile spends a fifth of its life
  // waiting for its first tile.  A persistent launch -- as many workgroups as fit the chip at once, each walking its
  // outer tiles with the DMA ring running on across the boundaries -- pays that latency once.
  int64_t gx = outer_tiles;
  if (!alias && p.tiles_per_split <= kn.persist_max_tiles) {
    const int64_t lds_full = (int64_t)k::gemm_lds_bytes(mw, cb.nt);
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(4, (160 * 1024) / lds_full));
    const int64_t slots = per_cu * s.num_cus / ((int64_t)cb.nblk * nsplit);
    if (slots >= 1 && outer_tiles >= 3 * slots) gx = slots;
  }
  if (!grid_fits((unsigned)cb.nblk, (unsigned)nsplit)) return rejected(p, "problem too large for the launch grid");

  // one launch, or the wide and the narrow blocks of an uneven blocking.  gemm_tn with a few outer tiles and a long,
  // split reduction (A^T Y at n = 512): the outer tiles of one slab on one XCD (per launch: the kernel's remap assumes
  // gridDim.y == 1)
  const int gw = p.mw * p.nw / 4;  // row tiles per SIMD
  p.nlaunch = uneven ? 2 : 1;
  for (int i = 0; i < p.nlaunch; ++i) {
    GemmLaunch& L = p.launch[i];
    L.grid[0] = (unsigned)gx;
    L.grid[1] = (unsigned)(uneven ? (i == 0 ? n_wide : cb.nblk - n_wide) : cb.nblk);
    L.grid[2] = (unsigned)nsplit;
    L.nt = cb.nt - i;
    L.col_base = (int64_t)i * n_wide * cb.nt * 16;
    L.xcd_remap = (s.tn && kn.xcd_remap && L.grid[1] == 1 && gx == outer_tiles && outer_tiles >= 2 && outer_tiles <= 32 &&
                   nsplit >= 8) ? 1 : 0;
    if (alias) {
      L.lds = 3 * k::big_tile_bytes(2);
    } else {
      // the kernels only touch ring buffers [0, min(tiles per workgroup, stages)): a short reduction (the l-deep
      // products Y * R^-1 and U = Q * U~ have 2-3 tiles) asks for less LDS, so several workgroups share a CU and one's
      // load latency hides behind another's MFMAs and stores
      const int64_t per_wg = (int64_t)std::max(1, p.tiles_per_split) * ((outer_tiles + gx - 1) / gx);
      L.lds = (int)std::min<int64_t>(k::gemm_stages(gw, L.nt), per_wg) * k::stage_bytes(gw, L.nt);
    }
  }
  if (!plan_reduce(p, outer_n, cb.cols_alloc)) p.error = "problem too large for the launch grid";
  return p;
}

// Both tall products of a call on the bf16-stored operand r with an l-column sketch, the skinny operands as the backend
// allocates them, are in the bf16-stored kernels' domain.
inline bool gemm_bf16a_call_domain(const GemmOperand& r, int64_t l, int num_cus) {
  for (int tn = 0; tn < 2; ++tn) {
    const int64_t xr = tn ? r.rows : r.cols, outr = tn ? r.cols : r.rows;
    const SkinnyLayout lx = skinny_layout(xr, l), lo = skinny_layout(outr, l);
    GemmShape s;
    s.tn = tn != 0;
    s.r = r;
    s.x = {xr, l, lx.ld, 0, lx.cols_alloc, false, true};
    s.out = {outr, l, lo.ld, 0, lo.cols_alloc, false, true};
    s.r_bf16 = true;
    s.num_cus = num_cus;
    if (!gemm_bf16a_domain(s)) return false;
  }
  return true;
}

// ---- one-sweep Z' = A^T (A Z) (ata_kernels.hpp): row-major f32 A (rows x n), Z and Z' n x l in the padded layout ----------
struct AtaPlan {
  bool in_domain = false;       // what the driver asks before it takes this route: f32, 16 <= n <= 512, l <= 80, rows >= 4096
  const char* error = nullptr;  // the call is rejected (thrown as ST_EINVAL)
  int nk = 0, nct = 0;          // ata_fused_kernel<NK, NCT>: n padded to 64 NK, 16 NCT columns
  int nrg = 0;                  // row groups = workgroups, one partial Z' each
  int block = 256, lds = 0;
  int64_t rows_per_group = 0, slab_stride = 0;
  size_t slab_bytes = 0;        // zero-filled: empty groups contribute zeros
  SlabReducePlan reduce;
};
inline bool ata_domain(int esz, int64_t rows, int64_t n, int64_t l) {
  return esz == 4 && n <= 512 && n >= 16 && l <= 16 * kAtaMaxColTiles && rows >= 4096;
}
// a: the big operand; x, z: the skinny operand and the result
inline AtaPlan ata_plan(int esz, const GemmOperand& a, const GemmOperand& x, const GemmOperand& z, int num_cus) {
  AtaPlan p;
  auto rejected = [&p](const char* why) {
    p.error = why;
    return p;
  };
  p.in_domain = ata_domain(esz, a.rows, a.cols, x.cols);
  if (esz != 4) return rejected("internal: the one-sweep power iteration is f32 only");
  if (x.rows != a.cols || z.rows != a.cols) return rejected("ata_fused: shapes");
  const ColBlocking cb = col_blocking(x.cols);
  if (cb.cols_alloc > x.cols_alloc || cb.cols_alloc > z.cols_alloc || x.ld != z.ld || cb.cols_alloc > 16 * kAtaMaxColTiles)
    return rejected("internal: ata_fused operands must share the padded layout (<= 80 columns)");
  if (!a.aligned || (a.ld % 4) || (a.cols_readable % 4)) return rejected("internal: operand not vector aligned");
  // reduction segments: n padded to 128 / 256 / 512 (three instantiation families)
  p.nk = a.cols <= 128 ? 2 : (a.cols <= 256 ? 4 : 8);
  p.nct = (int)(cb.cols_alloc / 16);
  // one workgroup per CU; every workgroup gets at least a few tiles
  const int64_t blocks = (a.rows + k::kAtaRows - 1) / k::kAtaRows;
  p.nrg = (int)std::max<int64_t>(1, std::min<int64_t>(num_cus, blocks / 8));
  p.rows_per_group = ((blocks + p.nrg - 1) / p.nrg) * k::kAtaRows;
  p.lds = k::ata_lds_bytes(p.nk, p.nct);
  p.slab_stride = z.ld * cb.cols_alloc;
  p.slab_bytes = (size_t)p.nrg * (size_t)p.slab_stride * 4;
  p.reduce = {SlabReduce::deep, {(unsigned)((a.cols + 63) / 64), (unsigned)cb.cols_alloc}, p.nrg, a.cols, cb.cols_alloc};
  if (!gemm_plan_detail::grid_fits(p.reduce.grid[1], 1)) return rejected("problem too large for the launch grid");
  return p;
}

// ---- CSR product Y (rows x L) = S X (spmm_kernels.hpp): X goes through a row-major scratch XT (cols x Lp), the long rows
// (n_long of them, in n_chunks chunks) through partial sums of Lpart values per chunk ----
struct SpmmPlan {
  const char* error = nullptr;  // the call is rejected (thrown as ST_EINVAL)
  int64_t Lp = 0, jt = 0, Lpart = 0;
  size_t xt_bytes = 0, scratch_bytes = 0;  // XT, and XT + the partial sums
  unsigned grid_xt[2] = {0, 0}, grid_rows[2] = {0, 0};
  unsigned grid_long_partial[2] = {0, 0}, grid_long_reduce[2] = {0, 0};  // launched when n_long > 0
};
inline SpmmPlan spmm_plan(int esz, int64_t rows, int64_t cols, int64_t L, int64_t n_long, int64_t n_chunks) {
  SpmmPlan p;
  const int64_t tile = k::kSpTile;
  p.Lp = (L + 15) / 16 * 16;
  p.jt = (L + tile - 1) / tile;
  p.Lpart = p.jt * 64;
  p.xt_bytes = ((size_t)cols * (size_t)p.Lp * (size_t)esz + 255) / 256 * 256;
  p.scratch_bytes = p.xt_bytes + (size_t)n_chunks * (size_t)p.Lpart * (size_t)esz;
  p.grid_xt[0] = (unsigned)((cols + tile - 1) / tile), p.grid_xt[1] = (unsigned)((p.Lp + tile - 1) / tile);
  p.grid_rows[0] = (unsigned)((rows + tile - 1) / tile), p.grid_rows[1] = (unsigned)p.jt;
  p.grid_long_partial[0] = (unsigned)n_chunks, p.grid_long_partial[1] = (unsigned)p.jt;
  p.grid_long_reduce[0] = (unsigned)n_long, p.grid_long_reduce[1] = (unsigned)p.jt;
  if (!gemm_plan_detail::grid_fits(p.grid_xt[1], p.grid_rows[1])) p.error = "problem too large for the launch grid";
  return p;
}

}  // namespace corrla
