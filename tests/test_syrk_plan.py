"""The plan of the symmetric rank-k product behind corrla_cov_* (corrla_rs_amd/csrc/syrk_plan.hpp), pinned on the CPU: the
header is host code, compiled here with the host compiler in a temporary directory.

For every row of SHAPES the driver prints the plan and the pair enumeration; pinned here: every (bi, bj) with bi <= bj
occurs exactly once and none with bi > bj, the slabs cover [0, m) exactly once in multiples of the tile depth, the
workspace stays within the plan's stated bound, the dynamic LDS within 160 KiB, and the route is the expected one for
aligned, unaligned and feature-strided input.  The table ends with the calls of tests/test_gpu_cov.py (GPU_CALLS), built from
the shape tables below, which that file imports -- as tests/test_gpu_gemm_routes.py imports ROUTES from test_gemm_plan.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corrla_rs_amd", "csrc")
REJECT, INPLACE, CHECKED, REPACKED = 0, 1, 2, 3

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "syrk_plan.hpp"
using namespace corrla;
int main(int argc, char** argv) {
  // m n rs cs esz base_aligned num_cus knob_slab_rows
  if (argc != 9) return 2;
  SyrkShape s;
  s.m = atoll(argv[1]); s.n = atoll(argv[2]); s.row_stride = atoll(argv[3]); s.col_stride = atoll(argv[4]);
  s.esz = atoi(argv[5]); s.base_aligned = atoi(argv[6]) != 0; s.num_cus = atoi(argv[7]);
  SyrkKnobs kn; kn.slab_rows = atoll(argv[8]);
  const SyrkPlan p = syrk_plan(s, kn);
  printf("route %d\n", (int)p.route);
  if (p.route == SyrkRoute::kReject) { printf("error %s\n", p.error); return 0; }
  printf("bt %d\nkt %d\nnb %d\nnpairs %lld\nktiles %lld\nnsplit %lld\nslab_rows %lld\n", p.bt, p.kt, p.nb, (long long)p.npairs,
         (long long)p.ktiles, (long long)p.nsplit, (long long)p.slab_rows);
  printf("grid %u %u %u\nlds %zu\nld %lld\nrepack %zu\nws %zu\nws_bound %zu\nfinish %u %u %u\n", p.grid_x, p.grid_y, p.block,
         p.lds_bytes, (long long)p.ld, p.repack_bytes, p.ws_bytes, p.ws_bound, p.finish_grid_x, p.finish_grid_y, p.finish_block);
  printf("pairs");
  for (long long q = 0; q < (long long)p.npairs; ++q) { int bi, bj; k::syrk_pair(q, &bi, &bj); printf(" %d:%d", bi, bj); }
  printf("\n");
  return 0;
}
"""


def build_driver(tmp, csrc=CSRC):
    src = os.path.join(tmp, "syrk_plan_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "syrk_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + csrc, src, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("syrk_plan")))


def plan(exe, m, n, rs, cs, esz, base_aligned=1, num_cus=256, slab_rows=0):
    out = subprocess.check_output([exe] + [str(v) for v in (m, n, rs, cs, esz, base_aligned, num_cus, slab_rows)], text=True)
    d = {}
    for line in out.splitlines():
        key, _, rest = line.partition(" ")
        d[key] = rest
    p = {"route": int(d["route"])}
    if p["route"] == REJECT:
        p["error"] = d["error"]
        return p
    for key in ("bt", "kt", "nb", "npairs", "ktiles", "nsplit", "slab_rows", "lds", "ld", "repack", "ws", "ws_bound"):
        p[key] = int(d[key])
    p["grid"] = tuple(int(v) for v in d["grid"].split())
    p["finish"] = tuple(int(v) for v in d["finish"].split())
    p["pairs"] = [tuple(int(v) for v in t.split(":")) for t in d["pairs"].split()]
    return p


# The shapes, layouts and forced slab of tests/test_gpu_cov.py, which imports them from here: one table for both files.
EXACT_SHAPES = ((1031, 200), (130, 129), (64, 128), (7, 5))        # integer second moments, center=False
CENTRED_SHAPES = ((1031, 77), (61, 300))                            # Gaussian, every layout of LAYOUTS
LAYOUTS = ("contiguous", "ld_n_plus_3", "base_plus_1", "column_major")
EDGE_CASES = {"ddof0": (1031, 77, 0), "n1": (1031, 1, 1), "m2": (2, 77, 1)}   # name -> (m, n, ddof)
REFERENCE_SHAPE = (10000, 5)                                        # stats_corr.rs:259-298
SLAB_ROWS = 96   # CORRLA_SYRK_SLAB_ROWS of the forced-slab context: several slabs, a short last one at m = 1031 and 130


# (m, n, row stride, column stride, element size, base aligned, forced slab rows, route) of every call above -- row stride n:
# contiguous; n + 3: padded rows; base aligned 0: a view one element past a 16-byte boundary; column-major: strides (1, m).
def _gpu_calls():
    calls = []
    for esz in (4, 8):
        vec = 16 // esz

        def rowmajor(ld, base=1):
            return INPLACE if base and ld % vec == 0 else CHECKED
        for (m, n) in EXACT_SHAPES:
            calls.append((m, n, n, 1, esz, 1, 0, rowmajor(n)))
            calls.append((m, n, n, 1, esz, 1, SLAB_ROWS, rowmajor(n)))
        for (m, n) in CENTRED_SHAPES:
            for layout in LAYOUTS:
                calls.append({"contiguous": (m, n, n, 1, esz, 1, 0, rowmajor(n)),
                              "ld_n_plus_3": (m, n, n + 3, 1, esz, 1, 0, rowmajor(n + 3)),
                              "base_plus_1": (m, n, n, 1, esz, 0, 0, CHECKED),
                              "column_major": (m, n, 1, m, esz, 1, 0, REPACKED)}[layout])
        for (m, n, _ddof) in EDGE_CASES.values():
            rs = 1 if n == 1 else n
            calls.append((m, n, rs, 1, esz, 1, 0, rowmajor(rs)))
        m, n = REFERENCE_SHAPE
        calls.append((m, n, n, 1, esz, 1, 0, rowmajor(n)))
    return calls


GPU_CALLS = _gpu_calls()

SHAPES = [
    # (m, n, rs, cs, esz, base_aligned, slab_rows, route)
    (1000000, 256, 256, 1, 4, 1, 0, INPLACE),
    (100000, 1024, 1024, 1, 8, 1, 0, INPLACE),
    (16384, 4096, 4096, 1, 4, 1, 0, INPLACE),
    (16384, 16384, 16384, 1, 4, 1, 0, INPLACE),
    (16384, 16384, 16384, 1, 8, 1, 0, INPLACE),
    (5000, 300, 300, 1, 8, 1, 0, INPLACE),
    (5000, 301, 301, 1, 8, 1, 0, CHECKED),
    (5000, 300, 302, 1, 4, 1, 0, CHECKED),
    (5000, 300, 304, 1, 4, 0, 0, CHECKED),
    (5000, 300, 1, 5000, 4, 1, 0, REPACKED),
    (5000, 300, 1, 5008, 8, 0, 0, REPACKED),
    (5000, 300, 600, 2, 4, 1, 0, REPACKED),
    (1, 9, 9, 1, 8, 1, 0, CHECKED),
    (3, 1, 7, 5, 8, 1, 0, CHECKED),
    (33, 129, 129, 1, 4, 1, 32, CHECKED),
] + GPU_CALLS


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "-".join(str(v) for v in c))
def test_plan_properties(driver, case):
    m, n, rs, cs, esz, base, slab, route = case
    p = plan(driver, m, n, rs, cs, esz, base, 256, slab)
    assert p["route"] == route, p
    assert p["bt"] == 128 and p["kt"] == (32 if esz == 4 else 16)
    nb = (n + 127) // 128
    assert p["nb"] == nb and p["npairs"] == nb * (nb + 1) // 2 == len(p["pairs"])
    # every (bi, bj) with bi <= bj exactly once, none below the diagonal
    assert all(0 <= bi <= bj < nb for bi, bj in p["pairs"]), [q for q in p["pairs"] if not 0 <= q[0] <= q[1] < nb][:3]
    assert sorted(p["pairs"]) == [(bi, bj) for bi in range(nb) for bj in range(bi, nb)]
    # the slabs cover [0, m) exactly once, in multiples of the tile depth
    assert p["slab_rows"] % p["kt"] == 0 and p["slab_rows"] >= p["kt"]
    covered = 0
    for s_ in range(p["nsplit"]):
        lo, hi = s_ * p["slab_rows"], min(m, (s_ + 1) * p["slab_rows"])
        assert lo == covered and hi > lo, (s_, lo, hi)      # no gap, no overlap, no empty slab
        covered = hi
    assert covered == m
    assert p["ktiles"] == (m + p["kt"] - 1) // p["kt"]
    if slab:
        assert p["slab_rows"] == (slab + p["kt"] - 1) // p["kt"] * p["kt"] or p["nsplit"] == 1
    # grid, LDS, workspace
    assert p["grid"] == (p["npairs"], p["nsplit"], 256) and p["nsplit"] <= 65535
    assert p["finish"] == (p["npairs"], 16, 256)
    assert p["lds"] == 2 * p["kt"] * 128 * esz == 32768 <= 160 * 1024
    assert p["ws"] == p["nsplit"] * p["npairs"] * 128 * 128 * esz <= p["ws_bound"]
    if not slab:
        assert p["ws_bound"] == (p["npairs"] + 4 * 256) * 128 * 128 * esz
    # the leading dimension the kernel reads with, and the repacked copy
    if route == REPACKED:
        assert p["ld"] == (n + 63) // 64 * 64 and p["repack"] == m * p["ld"] * esz
    else:
        assert p["repack"] == 0 and p["ld"] == (rs if (m > 1 or n == 1) else max(rs, n))
        vec = 16 // esz
        assert (route == INPLACE) == (bool(base) and p["ld"] % vec == 0)


def test_the_split_fills_the_chip_when_pairs_are_few_and_is_one_when_they_are_many(driver):
    tall = plan(driver, 10 ** 6, 256, 256, 1, 4)
    assert tall["npairs"] == 3 and tall["nsplit"] > 1
    assert 2 * 256 <= tall["nsplit"] * tall["npairs"] <= 4 * 256 + tall["npairs"]      # two to four workgroups per CU
    assert plan(driver, 16384, 16384, 16384, 1, 4)["nsplit"] == 1
    assert plan(driver, 100000, 1024, 1024, 1, 8)["nsplit"] > 1
    # a short matrix is not cut into slabs of fewer than 8 tiles
    short = plan(driver, 1000, 256, 256, 1, 4)
    assert short["slab_rows"] >= 8 * 32 and short["nsplit"] == 4


def test_rejections_carry_their_reason(driver):
    for args, word in (((0, 5, 5, 1, 4), "empty"), ((5, 0, 5, 1, 4), "empty"), ((5, 5, 5, 1, 2), "element size"),
                       ((5, 5, 0, 0, 4), "stride"), ((5, 5, -5, 1, 4), "negative"), ((5, 128 * 40000, 1, 5, 4), "tiles")):
        p = plan(driver, *args)
        assert p["route"] == REJECT and word in p["error"], (args, p)


def test_a_shifted_pair_index_is_caught(tmp_path):
    """A scratch copy of the header whose pair enumeration is off by one must fail the pair check above."""
    import shutil
    scratch = tmp_path / "csrc"
    shutil.copytree(CSRC, scratch)
    hdr = scratch / "syrk_plan.hpp"
    txt = hdr.read_text()
    good = "  *bi = (int)p;\n"
    assert txt.count(good) == 1
    hdr.write_text(txt.replace(good, "  *bi = (int)p + 1;\n"))
    exe = build_driver(str(tmp_path), str(scratch))
    p = plan(exe, 1031, 200, 200, 1, 4)
    nb = 2
    assert not (all(0 <= bi <= bj < nb for bi, bj in p["pairs"]) and
                sorted(p["pairs"]) == [(bi, bj) for bi in range(nb) for bj in range(bi, nb)])


def test_the_gpu_files_calls_reach_every_route_and_several_slabs(driver):
    assert {c[-1] for c in GPU_CALLS} == {INPLACE, CHECKED, REPACKED}
    forced = [plan(driver, *c[:6], 256, c[6]) for c in GPU_CALLS if c[6]]
    assert any(p["nsplit"] > 2 and c[0] % p["slab_rows"] for p, c in zip(forced, [c for c in GPU_CALLS if c[6]]))   # a short last slab
    assert any(p["npairs"] == 3 for p in forced)      # a diagonal and an off-diagonal pair, a ragged second tile
