// The plans of the column passes (colstat_stage.hpp launches what they say): the bandwidth-bound reductions over A that give
// per-column statistics -- the column sums of squares of the standardised PCA (colvar_kernels.hpp), dense in both
// orientations and CSR, the column moments of cov and polyfit (colmom_*_kernel in syrk_kernels.hpp), which take the "down"
// plan, and the weighted column sums of the implicit centring (wcolsum_*_kernel in hip_kernels.hpp).  Every pass writes
// per-slab partial sums and a finishing launch adds them in index order; a plan gives the slabs, both grids and block
// sizes and the bytes of partial sums, or a rejection with its reason.
// Host code only, no HIP call: tests/test_colstat_plan.py compiles this header with the host compiler and pins the plans.
// The kernels take their block size and the elements of a 16-byte load from it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace corrla {
namespace k {

constexpr int kCvThreads = 256;                     // threads of a workgroup of the column-variance and moment kernels
constexpr int cv_vec(int esz) { return 16 / esz; }  // elements of one 16-byte load: 4 (f32), 2 (f64), 8 (bf16)

}  // namespace k

// workgroups that fill the device: what a pass cuts its reduced dimension for
inline int64_t colstat_fill_target(int num_cus) { return (int64_t)num_cus * 8; }

// kDown: the data columns run along the memory columns, reduce down the memory rows in slabs of rows.  kAlong: the data
// columns are the memory rows, reduce along them in segments of columns.
enum class ColstatBranch : int { kReject = 0, kDown = 1, kAlong = 2, kCsr = 3, kWcolsum = 4 };

struct ColstatPlan {
  ColstatBranch branch = ColstatBranch::kReject;
  const char* error = nullptr;
  int groups = 0;             // down: 16-byte column groups per workgroup, a power of two <= 256 (256 / groups row lanes)
  int64_t rows_per_slab = 0;  // down: slab s covers rows [s * rows_per_slab, min(rows, (s + 1) * rows_per_slab))
  int64_t seg_len = 0;        // along: columns per segment, a multiple of 64 * vec (what one wave reads per step)
  int64_t nslab = 0;          // partial sums per result: slabs (down, weighted sums) or segments (along, CSR)
  unsigned grid_x = 0, grid_y = 1, block = k::kCvThreads;  // down: (column block, slab); weighted sums: (slab, column)
  unsigned final_grid_x = 0, final_block = 256;            // one thread per result
  size_t ws_bytes = 0;        // the partial sums: nslab doubles per result (the moments take two such arrays), CSR: twice that
};

// x: rows x cols in memory (row-major), vec elements per 16-byte load; along_cols: the data columns run along the memory
// columns.  The moments of cov and polyfit are the down plan of their row-major x.
inline ColstatPlan colss_plan(int64_t rows, int64_t cols, int vec, bool along_cols, int num_cus) {
  ColstatPlan p;
  const int64_t target = colstat_fill_target(num_cus), n = along_cols ? cols : rows;
  if (along_cols) {
    const int64_t ngroups = (cols + vec - 1) / vec;
    p.groups = 1;
    while (p.groups < k::kCvThreads && p.groups < ngroups) p.groups *= 2;
    const int ny = k::kCvThreads / p.groups;
    const int64_t col_blocks = (ngroups + p.groups - 1) / p.groups;
    // every row lane gets at least eight rows
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>((target + col_blocks - 1) / col_blocks, (rows + 8 * ny - 1) / (8 * ny)));
    p.rows_per_slab = (rows + want - 1) / want;
    p.nslab = (rows + p.rows_per_slab - 1) / p.rows_per_slab;
    p.grid_x = (unsigned)col_blocks;
    p.grid_y = (unsigned)p.nslab;
    if (p.nslab > 65535) p.error = "problem too large for the launch grid";
  } else {
    const int64_t quantum = 64 * (int64_t)vec;  // what one wave reads per step
    const int64_t max_segs = (cols + 4 * quantum - 1) / (4 * quantum);
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>((4 * target + rows - 1) / rows, max_segs));
    p.seg_len = ((cols + want - 1) / want + quantum - 1) / quantum * quantum;
    p.nslab = (cols + p.seg_len - 1) / p.seg_len;
    // one wave per (row, segment) unit, four waves per workgroup
    p.grid_x = (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows * p.nslab + 3) / 4, 2 * target));
  }
  if (!p.error) p.branch = along_cols ? ColstatBranch::kDown : ColstatBranch::kAlong;
  p.final_grid_x = (unsigned)((n + 255) / 256);
  p.ws_bytes = sizeof(double) * (size_t)p.nslab * (size_t)n;
  return p;
}

// The same over a CSR whose `rows` ROWS are the data columns: one wave per (row, segment) unit, a row cut into nslab
// segments of equal entry counts; the partial sums and the entry counts are one array of rows * nslab doubles each.
inline ColstatPlan csr_colss_plan(int64_t rows, int num_cus) {
  ColstatPlan p;
  const int64_t target = colstat_fill_target(num_cus);
  p.branch = ColstatBranch::kCsr;
  p.nslab = std::max<int64_t>(1, std::min<int64_t>((4 * target + rows - 1) / rows, 64));
  p.grid_x = (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows * p.nslab + 3) / 4, 2 * target));
  p.final_grid_x = (unsigned)((rows + 255) / 256);
  p.ws_bytes = 2 * sizeof(double) * (size_t)(rows * p.nslab);
  return p;
}

// v[c] = sum over the rows of w[r] * x(r, c) for the ncols columns of a skinny operand: nslab slabs of rows per column.
inline ColstatPlan wcolsum_plan(int64_t rows, int ncols) {
  ColstatPlan p;
  p.branch = ColstatBranch::kWcolsum;
  p.nslab = std::max<int64_t>(1, std::min<int64_t>(64, (rows + 4095) / 4096));
  p.grid_x = (unsigned)p.nslab;
  p.grid_y = (unsigned)ncols;
  p.block = 256;
  p.final_grid_x = (unsigned)((ncols + 63) / 64);
  p.final_block = 64;
  p.ws_bytes = sizeof(double) * (size_t)p.nslab * (size_t)ncols;
  return p;
}

}  // namespace corrla
