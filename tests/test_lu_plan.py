"""The plan of the dense LU solve behind corrla_lu_solve_* and corrla_rbffit_* (corrla_rs_amd/csrc/lu_plan.hpp), pinned on
the CPU: the header is host code, compiled here with the host compiler in a temporary directory.

Pinned: the row chunks of a panel step cover [j, n) exactly once; the tiles of the trailing update cover A22 exactly once for
n at NB k - 1, NB k and NB k + 1; the route boundary sits at kLuSmallN / kLuSmallN + 1; the LDS images stay within 160 KiB;
the workspace stays within the plan's stated bound; the launch counts are the documented ones (2 per column, 3 per panel but
1 for the last, 2 for max |u|; the solve's 1 + 2 (2 blocks - 1)); every rejection names its argument.  The module ends with
the calls of tests/test_gpu_lu.py (GPU_CALLS), which that file imports -- as tests/test_gpu_rbf.py imports its table from
test_rbf_plan.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corrla_rs_amd", "csrc")
NB, TILE, CHUNK, THREADS, SMALL_N = 64, 64, 64, 256, 128
MAX_N, MAX_RHS = 1 << 17, 1 << 20
LDS_MAX = 160 * 1024
SMALL, BLOCKED = 1, 2

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "lu_plan.hpp"
using namespace corrla;
int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "chunks")) {  // chunks n j
    const long long n = atoll(argv[2]), j = atoll(argv[3]);
    for (long long c = 0; c < lu_step_chunks(n, j); ++c)
      printf("%lld %lld\n", (long long)lu_piece_begin(j, c, k::kLuChunk), (long long)lu_piece_end(j, c, k::kLuChunk, n));
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "tiles")) {  // tiles n j1
    const long long n = atoll(argv[2]), j1 = atoll(argv[3]);
    for (long long t = 0; t < lu_trail_tiles(n, j1); ++t)
      printf("%lld %lld\n", (long long)lu_piece_begin(j1, t, k::kLuTile), (long long)lu_piece_end(j1, t, k::kLuTile, n));
    return 0;
  }
  if (argc != 3) return 2;
  LuShape s;
  s.n = atoll(argv[1]); s.n_rhs = atoll(argv[2]);
  const LuPlan p = lu_plan(s);
  printf("ok %d\n", (int)p.ok);
  if (!p.ok) { printf("error %s\n", p.error); return 0; }
  printf("route %d\nnb %d\nnpanels %lld\nnblocks %lld\nmax_chunks %lld\nmaxu_blocks %lld\nrhs_tiles %lld\n", (int)p.route, p.nb,
         (long long)p.npanels, (long long)p.nblocks, (long long)p.max_chunks, (long long)p.maxu_blocks, (long long)p.rhs_tiles);
  printf("factor_launches %lld\nsolve_launches %lld\n", (long long)p.factor_launches, (long long)p.solve_launches);
  printf("lds_small %zu\nlds_update %zu\nlds_tri %zu\nws %zu\nws_bound %zu\n", p.lds_small, p.lds_update, p.lds_tri, p.ws_bytes, p.ws_bound);
  printf("consts %d %d %d %d %d %lld %lld %zu %zu\n", k::kLuNB, k::kLuTile, k::kLuChunk, k::kLuThreads, k::kLuSmallN, (long long)k::kLuMaxN,
         (long long)k::kLuMaxRhs, k::kLdsMaxBytes, sizeof(LuStatus));
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("lu_plan"))
    src = os.path.join(tmp, "lu_plan_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "lu_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, src, "-o", exe])
    return exe


def plan(exe, n, n_rhs=1):
    out = subprocess.check_output([exe, str(n), str(n_rhs)], text=True)
    d = dict(line.partition(" ")[::2] for line in out.splitlines())
    p = {"ok": int(d["ok"])}
    if not p["ok"]:
        p["error"] = d["error"]
        return p
    for key, v in d.items():
        if key not in ("ok", "consts"):
            p[key] = int(v)
    p["consts"] = tuple(int(v) for v in d["consts"].split())
    return p


def pieces(exe, what, n, base):
    out = subprocess.check_output([exe, what, str(n), str(base)], text=True)
    return [tuple(int(v) for v in line.split()) for line in out.splitlines()]


def covers_once(ranges, lo, hi):
    at = lo
    for a, b in ranges:
        if a != at or b <= a:
            return False
        at = b
    return at == hi


PLAN_N = (1, 2, 5, 100, SMALL_N, SMALL_N + 1, 3 * NB - 1, 3 * NB, 3 * NB + 1, 704, 2048, 16384, MAX_N)


def test_constants(driver):
    p = plan(driver, 100)
    assert p["consts"] == (NB, TILE, CHUNK, THREADS, SMALL_N, MAX_N, MAX_RHS, LDS_MAX, 24)


def test_chunks_cover_the_rows_of_a_panel_step_once(driver):
    for n in (SMALL_N + 1, 3 * NB - 1, 3 * NB, 3 * NB + 1, 704):
        for j in (0, 1, NB - 1, NB, n - CHUNK - 1, n - CHUNK, n - 2, n - 1):
            r = pieces(driver, "chunks", n, j)
            assert covers_once(r, j, n), (n, j, r)
            assert all(b - a <= CHUNK for a, b in r)
            assert len(r) == -(-(n - j) // CHUNK)


@pytest.mark.parametrize("k", (3, 4, 11))
def test_tiles_cover_the_trailing_matrix_once(driver, k):
    for n in (NB * k - 1, NB * k, NB * k + 1):
        for j1 in range(NB, n, NB):  # the end of every panel but the last
            t = pieces(driver, "tiles", n, j1)
            assert covers_once(t, j1, n), (n, j1, t)  # rows and columns alike: the tile grid is the product
            assert all(b - a <= TILE for a, b in t)


def test_route_boundary(driver):
    assert plan(driver, SMALL_N)["route"] == SMALL
    assert plan(driver, SMALL_N + 1)["route"] == BLOCKED
    assert plan(driver, 1)["route"] == SMALL


@pytest.mark.parametrize("n", PLAN_N)
def test_lds_workspace_and_launches(driver, n):
    for n_rhs in (0, 1, 3, 65):
        p = plan(driver, n, n_rhs)
        assert p["ok"]
        assert max(p["lds_small"], p["lds_update"], p["lds_tri"]) <= LDS_MAX
        assert p["lds_small"] == (SMALL_N * (SMALL_N + 1) + 2 * THREADS) * 8
        assert p["lds_update"] == (TILE * (NB + 1) + NB * (TILE + 1)) * 8
        assert p["ws"] <= p["ws_bound"] == 9 * n + 2048
        # the pieces: status, partial maxima (16 bytes each), partial max |u|, ipiv; each rounded up to 256
        r256 = lambda b: -(-b // 256) * 256  # noqa: E731
        chunks0 = -(-n // CHUNK)
        assert p["max_chunks"] == chunks0
        assert p["ws"] == 256 + r256(16 * chunks0) + r256(8 * -(-n // TILE)) + r256(8 * n)
        npanels = -(-n // NB)
        assert p["npanels"] == p["nblocks"] == npanels
        if n <= SMALL_N:
            assert p["factor_launches"] == 1
        else:
            assert p["factor_launches"] == 2 * n + 3 * (npanels - 1) + 1 + 2
        assert p["solve_launches"] == (0 if n_rhs == 0 else 1 + 2 * (2 * npanels - 1))
        assert p["rhs_tiles"] == -(-n_rhs // TILE)


def test_grids_stay_inside_int32(driver):
    p = plan(driver, MAX_N, MAX_RHS)
    assert p["ok"]
    tiles = -(-MAX_N // TILE)
    assert tiles * tiles < 2 ** 31 and tiles * p["rhs_tiles"] < 2 ** 31
    assert MAX_N * MAX_N * 8 < 2 ** 63


@pytest.mark.parametrize("n,n_rhs,text", [
    (0, 1, "lu: n must be >= 1"),
    (-3, 1, "lu: n must be >= 1"),
    (MAX_N + 1, 1, "lu: n must be <= 131072"),
    (5, -1, "lu: n_rhs must be >= 0"),
    (5, MAX_RHS + 1, "lu: n_rhs must be <= 1048576"),
])
def test_rejections_name_their_argument(driver, n, n_rhs, text):
    p = plan(driver, n, n_rhs)
    assert not p["ok"] and p["error"] == text


# ---- the calls of tests/test_gpu_lu.py, which imports them from here ------------------------------------------------------------
# (n, n_rhs, lda - n, ldb - n_rhs, matrix): the small route at 1, 2, 5, 100 and kLuSmallN; the blocked route at kLuSmallN + 1,
# around a panel boundary with three panels, and 704 = 11 panels; n_rhs 1, 3 and 65 (two column tiles); padded strides
SMALL_NS = (1, 2, 5, 100, SMALL_N)
BLOCKED_NS = (SMALL_N + 1, 3 * NB - 1, 3 * NB, 3 * NB + 1, 704)


def _gpu_calls():
    calls = [(n, 3, 0, 0, "gauss") for n in SMALL_NS + BLOCKED_NS]
    calls += [(n, 1, 0, 0, "shift") for n in (5, 100, SMALL_N + 1, 3 * NB + 1, 704)]
    calls += [(100, 65, 0, 0, "gauss"), (3 * NB + 1, 65, 0, 0, "gauss"), (3 * NB - 1, 1, 0, 0, "gauss")]
    calls += [(100, 3, 5, 2, "gauss"), (3 * NB + 1, 3, 7, 1, "shift"), (3 * NB, 65, 1, 3, "gauss")]
    calls += [(40, 3, 0, 0, "wilkinson")]
    return calls


GPU_CALLS = _gpu_calls()


def test_gpu_calls_take_both_routes(driver):
    routes = {plan(driver, c[0], c[1])["route"] for c in GPU_CALLS}
    assert routes == {SMALL, BLOCKED}
    assert {c[1] for c in GPU_CALLS} >= {1, 3, 65}
    assert any(c[2] > 0 and c[3] > 0 for c in GPU_CALLS)
