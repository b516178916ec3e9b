"""The plan of the bf16-stored tall products (gemm_plan.hpp: gemm_bf16a_domain, plan_bf16_stored), pinned on the CPU: the
header is host code, compiled here with the host compiler as tests/test_gemm_plan.py does.  The expected values are
restated independently below: domain, grid, column tiles, dynamic LDS, reduction split, slab workspace and planes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include <cstdio>
#include "gemm_plan.hpp"
int main() {
  const char* red[] = {"none", "plain", "deep"};
  long long v[12];
  while (true) {
    for (int i = 0; i < 12; ++i)
      if (std::scanf("%lld", &v[i]) != 1) return 0;
    corrla::GemmShape s;
    s.tn = v[0] != 0;
    s.r_bf16 = v[10] != 0;
    s.num_cus = (int)v[11];
    const long long outer_n = s.tn ? v[2] : v[1], red_n = s.tn ? v[1] : v[2];
    const long long ldx = (red_n + 63) / 64 * 64, ldo = (outer_n + 63) / 64 * 64;
    const long long ca = corrla::col_blocking(v[7]).cols_alloc;
    s.r = {v[1], v[2], v[3], v[4], 0, false, v[5] != 0};
    s.x = {red_n, v[7], ldx, 0, ca, v[8] != 0, true};
    s.out = {outer_n, v[7], ldo, 0, ca, false, true};
    s.same = v[9] != 0;
    (void)v[6];
    const bool dom = corrla::gemm_bf16a_domain(s);
    const corrla::GemmPlan p = corrla::gemm_plan(s, corrla::GemmKnobs{});
    if (p.error) {
      std::printf("%d reject %s\n", dom ? 1 : 0, p.error);
      continue;
    }
    const corrla::GemmLaunch& L = p.launch[0];
    std::printf("%d %d %d %d %d %u %u %u %d %d %d %d %d %lld %lld %zu %s %u %u %d %lld %zu %u\n", dom ? 1 : 0, (int)p.family, p.np, p.block,
                p.nlaunch, L.grid[0], L.grid[1], L.grid[2], L.nt, L.lds, p.tiles_total, p.nsplit, p.tiles_per_split,
                (long long)p.out_cols, (long long)p.slab_stride, p.slab_bytes, red[(int)p.reduce.kind], p.reduce.grid[0],
                p.reduce.grid[1], p.reduce.slabs, (long long)p.plane_stride, p.plane_bytes, p.split_grid);
  }
}
"""
FAMILY_BF16_STORED = 5  # position in enum class GemmFamily


def cdiv(a, b):
    return (a + b - 1) // b


def round_up(a, b):
    return cdiv(a, b) * b


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gemm_plan_bf16")
    src = tmp / "plan.cpp"
    src.write_text(MAIN)
    exe = tmp / "plan"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "corrla_rs_amd", "csrc"),
                           str(src), "-o", str(exe)])

    def run(tn, rows, cols, l, ld=None, readable=None, aligned=True, x_external=False, same=False, bf16=True, cus=256):
        ld = cols if ld is None else ld
        readable = cols if readable is None else readable
        line = " ".join(str(int(v)) for v in (tn, rows, cols, ld, readable, aligned, 0, l, x_external, same, bf16, cus))
        return subprocess.run([str(exe)], input=line + "\n", capture_output=True, text=True, check=True).stdout.split()
    return run


def expected(tn, rows, cols, l, cus=256):
    """plan_bf16_stored restated: 256 outer indices and all column tiles per workgroup, 32-deep tiles, three planes, a big
    ring of four 16-KiB slots and a plane ring of three, one workgroup per CU -> the reduction is split to fill the chip"""
    outer_n, red_n = (cols, rows) if tn else (rows, cols)
    nt = cdiv(l, 16)
    assert nt <= 9
    cols_alloc = 16 * nt
    lds = 4 * 256 * 32 * 2 + 3 * 3 * nt * 16 * 32 * 2 + 1024
    assert lds <= 160 * 1024
    tiles = cdiv(red_n, 32)
    outer_tiles = cdiv(outer_n, 256)
    nsplit = 1
    if outer_tiles < cus:
        nsplit = min((cus + outer_tiles // 2) // outer_tiles, max(1, tiles // 16))
    nsplit = max(1, min(nsplit, tiles))
    ldx, ldo = round_up(red_n, 64), round_up(outer_n, 64)
    stride = ldo * cols_alloc
    if nsplit >= 8:
        red = ["deep", cdiv(outer_n, 64), cols_alloc, nsplit]
    elif nsplit > 1:
        red = ["plain", cdiv(outer_n, 256), cols_alloc, nsplit]
    else:
        red = ["none", 0, 0, 0]
    plane_stride = ldx * cols_alloc
    return [str(v) for v in [1, FAMILY_BF16_STORED, 3, 768, 1, outer_tiles, 1, nsplit, nt, lds, tiles, nsplit, cdiv(tiles, nsplit),
                             cols_alloc, stride, nsplit * stride * 4 if nsplit > 1 else 0] + red +
            [plane_stride, 3 * plane_stride * 2, max(1, min(4096, cdiv(plane_stride // 8, 256)))]]


@pytest.mark.parametrize("shape", [
    (False, 16384, 16384, 138),   # square, nn: 64 outer tiles, the reduction split four ways
    (True, 16384, 16384, 138),
    (False, 1250000, 512, 74),    # the config-4 shard: more outer tiles than CUs, no split
    (True, 1250000, 512, 74),     # its transposed product: TWO outer tiles, a 39063-tile reduction split 128 ways (deep)
    (True, 100000, 200, 16),      # ONE outer tile with a long reduction
    (False, 200, 100000, 1),      # ... and its nn twin (column means of a fat matrix): NT = 1
    (False, 4096, 1024, 138),     # the parity shape: 16 outer tiles, 32 tiles -> split 2 (plain)
    (False, 33, 8, 144),          # one tile, nine column tiles, the LDS maximum
])
def test_plan_of_in_domain_products(plan, shape):
    tn, rows, cols, l = shape
    assert plan(tn, rows, cols, l) == expected(tn, rows, cols, l), shape


def test_plan_pins_a_few_values_by_hand(plan):
    """so that `expected` itself cannot drift with the header: 16384^2, l = 138 by hand"""
    got = plan(False, 16384, 16384, 138)
    assert got[5:8] == ["64", "1", "4"]             # grid
    assert got[8] == "9" and got[9] == str(65536 + 3 * 27648 + 1024) == "149504"  # NT, LDS
    assert got[10:13] == ["512", "4", "128"]        # tiles, split, tiles per split
    assert got[15] == str(4 * 16384 * 144 * 4)      # slab workspace
    assert got[16] == "plain"
    got = plan(True, 100000, 200, 16)
    assert got[5:8] == ["1", "1", "195"] and got[16] == "deep" and got[8] == "1"
    assert got[9] == str(65536 + 3 * 3072 + 1024)


def test_domain_accepts_and_rejects(plan):
    ok = plan(False, 4096, 1024, 138)
    assert ok[0] == "1"
    # leading dimension not a multiple of 8 elements (rows would start off 16-byte boundaries)
    assert plan(False, 4096, 1024, 138, ld=1028)[:2] == ["0", "reject"]
    assert plan(False, 4096, 1024, 138, ld=1032)[0] == "1"
    # readable row length not a multiple of 8
    assert plan(False, 4096, 1021, 138, ld=1024)[:2] == ["0", "reject"]
    assert plan(True, 4096, 1021, 138, ld=1024)[:2] == ["0", "reject"]
    # base not 16-byte aligned
    assert plan(False, 4096, 1024, 138, aligned=False)[:2] == ["0", "reject"]
    # two column blocks
    assert plan(False, 4096, 1024, 144)[0] == "1"
    assert plan(False, 4096, 1024, 145)[:2] == ["0", "reject"]
    # Gram-like aliasing and a caller's buffer as the skinny operand
    assert plan(False, 4096, 1024, 138, same=True)[:2] == ["0", "reject"]
    assert plan(False, 4096, 1024, 138, x_external=True)[:2] == ["0", "reject"]
    # no size threshold: the smallest product is in the domain
    assert plan(False, 1, 8, 1)[0] == "1" and plan(True, 1, 8, 1)[0] == "1"
    # an f32 operand never takes this family
    f32 = plan(False, 4096, 1024, 138, bf16=False)
    assert f32[0] == "0" and f32[1] != str(FAMILY_BF16_STORED)
