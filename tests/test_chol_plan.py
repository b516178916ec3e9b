"""The plan of the dense Cholesky factor and SPD solve behind corrla_chol_factor_* and corrla_chol_solve_*
(corrla_rs_amd/csrc/chol_plan.hpp), pinned on the CPU: the header is host code, compiled here with the host compiler in a
temporary directory.

Pinned: the route boundary sits at kCholSmallN / kCholSmallN + 1; the launch counts are the documented ones (3 per panel but
1 for the last, 1 to reduce the panel records -- against the LU plan's 2 n + 3 npanels; the solve's 2 (2 blocks - 1)); for n
around 64, 128, 192, 193 and 704 the chunks of every panel solve cover each row below the block exactly once and the tile
pairs of every trailing update cover each tile with bi >= bj exactly once and none above the diagonal; the LDS images stay
within 160 KiB (the static ones within 64 KiB); the workspace stays within the plan's stated bound; every rejection names its
argument.  The module ends with the calls of tests/test_gpu_chol.py (GPU_CALLS), which that file imports."""
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
#include "chol_plan.hpp"
using namespace corrla;
int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "chunks")) {  // chunks n j1
    const long long n = atoll(argv[2]), j1 = atoll(argv[3]);
    for (long long c = 0; c < chol_chunks(n, j1); ++c)
      printf("%lld %lld\n", (long long)chol_piece_begin(j1, c, k::kCholChunk), (long long)chol_piece_end(j1, c, k::kCholChunk, n));
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "pairs")) {  // pairs n j1: the row and column ranges of every workgroup's tile
    const long long n = atoll(argv[2]), j1 = atoll(argv[3]);
    const long long nt = chol_trail_tiles(n, j1);
    for (long long p = 0; p < chol_tile_pairs(nt); ++p) {
      int64_t bi, bj;
      chol_tile_pair(p, &bi, &bj);
      printf("%lld %lld %lld %lld %lld %lld\n", (long long)bi, (long long)bj, (long long)chol_piece_begin(j1, bi, k::kCholTile),
             (long long)chol_piece_end(j1, bi, k::kCholTile, n), (long long)chol_piece_begin(j1, bj, k::kCholTile),
             (long long)chol_piece_end(j1, bj, k::kCholTile, n));
    }
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "pair")) {  // pair p
    int64_t bi, bj;
    chol_tile_pair(atoll(argv[2]), &bi, &bj);
    printf("%lld %lld\n", (long long)bi, (long long)bj);
    return 0;
  }
  if (argc != 3) return 2;
  CholShape s;
  s.n = atoll(argv[1]); s.n_rhs = atoll(argv[2]);
  const CholPlan p = chol_plan(s);
  printf("ok %d\n", (int)p.ok);
  if (!p.ok) { printf("error %s\n", p.error); return 0; }
  printf("route %d\nnb %d\nnpanels %lld\nnblocks %lld\nrhs_tiles %lld\n", (int)p.route, p.nb, (long long)p.npanels, (long long)p.nblocks,
         (long long)p.rhs_tiles);
  printf("factor_launches %lld\nsolve_launches %lld\n", (long long)p.factor_launches, (long long)p.solve_launches);
  printf("lds_small %zu\nlds_update %zu\nlds_gemm %zu\nlds_diag %zu\nlds_panel %zu\nlds_tri %zu\nws %zu\nws_bound %zu\n", p.lds_small,
         p.lds_update, p.lds_gemm, p.lds_diag, p.lds_panel, p.lds_tri, p.ws_bytes, p.ws_bound);
  printf("consts %d %d %d %d %d %lld %lld %zu %zu\n", k::kCholNB, k::kCholTile, k::kCholChunk, k::kCholThreads, k::kCholSmallN,
         (long long)k::kCholMaxN, (long long)k::kCholMaxRhs, k::kLdsMaxBytes, sizeof(CholFactorStatus));
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("chol_plan"))
    src = os.path.join(tmp, "chol_plan_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "chol_plan_driver")
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


def rows_of(exe, what, *args):
    out = subprocess.check_output([exe, what, *(str(a) for a in args)], text=True)
    return [tuple(int(v) for v in line.split()) for line in out.splitlines()]


def covers_once(ranges, lo, hi):
    at = lo
    for a, b in ranges:
        if a != at or b <= a:
            return False
        at = b
    return at == hi


PLAN_N = (1, 2, 5, 100, SMALL_N, SMALL_N + 1, 3 * NB - 1, 3 * NB, 3 * NB + 1, 704, 2048, 16384, MAX_N)
COVER_N = (NB - 1, NB, NB + 1, 2 * NB - 1, 2 * NB, 2 * NB + 1, 3 * NB - 1, 3 * NB, 3 * NB + 1, 704)


def test_constants(driver):
    p = plan(driver, 100)
    assert p["consts"] == (NB, TILE, CHUNK, THREADS, SMALL_N, MAX_N, MAX_RHS, LDS_MAX, 32)


def test_route_boundary(driver):
    assert plan(driver, SMALL_N)["route"] == SMALL
    assert plan(driver, SMALL_N + 1)["route"] == BLOCKED
    assert plan(driver, 1)["route"] == SMALL


@pytest.mark.parametrize("n", COVER_N)
def test_chunks_cover_the_rows_below_every_panel_once(driver, n):
    for j1 in range(NB, n, NB):  # the end of every panel but the last
        r = rows_of(driver, "chunks", n, j1)
        assert covers_once(r, j1, n), (n, j1, r)
        assert all(b - a <= CHUNK for a, b in r)
        assert len(r) == -(-(n - j1) // CHUNK)


@pytest.mark.parametrize("n", COVER_N)
def test_tile_pairs_cover_the_lower_triangle_once_and_nothing_above(driver, n):
    for j1 in range(NB, n, NB):
        nt = -(-(n - j1) // TILE)
        pairs = rows_of(driver, "pairs", n, j1)
        assert len(pairs) == nt * (nt + 1) // 2
        assert sorted((bi, bj) for bi, bj, *_ in pairs) == [(bi, bj) for bi in range(nt) for bj in range(bi + 1)]  # each once
        for bi, bj, r0, r1, c0, c1 in pairs:
            assert bj <= bi and (r0, c0) == (j1 + bi * TILE, j1 + bj * TILE)
            assert (r1, c1) == (min(n, r0 + TILE), min(n, c0 + TILE)) and r1 > r0 and c1 > c0
        # the row ranges of the diagonal tiles cut [j1, n) exactly once; so do the column ranges
        diag = sorted((r0, r1) for bi, bj, r0, r1, _, _ in pairs if bi == bj)
        assert covers_once(diag, j1, n)


def test_tile_pair_map_at_the_largest_grid(driver):
    nt = MAX_N // TILE
    last = nt * (nt + 1) // 2 - 1
    assert rows_of(driver, "pair", last) == [(nt - 1, nt - 1)]
    assert rows_of(driver, "pair", last - nt + 1) == [(nt - 1, 0)]
    assert rows_of(driver, "pair", last - nt) == [(nt - 2, nt - 2)]
    for bi in (1, 2, 3, 1000, 2047):  # the first and last pair of a row: where the square root may round either way
        assert rows_of(driver, "pair", bi * (bi + 1) // 2) == [(bi, 0)]
        assert rows_of(driver, "pair", bi * (bi + 1) // 2 + bi) == [(bi, bi)]
    assert last + 1 < 2 ** 31


@pytest.mark.parametrize("n", PLAN_N)
def test_lds_workspace_and_launches(driver, n):
    for n_rhs in (0, 1, 3, 65):
        p = plan(driver, n, n_rhs)
        assert p["ok"]
        assert max(p["lds_small"], p["lds_update"], p["lds_gemm"], p["lds_panel"]) <= LDS_MAX
        assert max(p["lds_diag"], p["lds_tri"]) <= 65536  # static
        assert p["lds_small"] == (SMALL_N * (SMALL_N + 1) + 2 * THREADS) * 8
        assert p["lds_update"] == 2 * TILE * (NB + 2) * 8
        assert p["lds_gemm"] == 2 * NB * (TILE + 16) * 8
        assert p["lds_diag"] == (NB * (NB + 1) + 2 * THREADS) * 8
        assert p["lds_panel"] == (NB * NB + CHUNK * (NB + 1)) * 8
        assert p["lds_tri"] == (NB * NB + NB * TILE) * 8
        npanels = -(-n // NB)
        assert p["npanels"] == p["nblocks"] == npanels
        # the pieces: the status record and one 32-byte record per panel; each rounded up to 256
        r256 = lambda b: -(-b // 256) * 256  # noqa: E731
        assert p["ws"] == 256 + r256(32 * npanels)
        assert p["ws"] <= p["ws_bound"] == n // 2 + 1024
        if n <= SMALL_N:
            assert p["factor_launches"] == 1
        else:
            assert p["factor_launches"] == 3 * npanels - 2 + 1
            assert p["factor_launches"] < 2 * n + 3 * npanels  # the LU plan's
        assert p["solve_launches"] == (0 if n_rhs == 0 else 2 * (2 * npanels - 1))
        assert p["rhs_tiles"] == -(-n_rhs // TILE)


def test_grids_stay_inside_int32(driver):
    p = plan(driver, MAX_N, MAX_RHS)
    assert p["ok"]
    tiles = -(-MAX_N // TILE)
    assert tiles * (tiles + 1) // 2 < 2 ** 31 and tiles * p["rhs_tiles"] < 2 ** 31
    assert MAX_N * MAX_N * 8 < 2 ** 63


@pytest.mark.parametrize("n,n_rhs,text", [
    (0, 1, "chol: n must be >= 1"),
    (-3, 1, "chol: n must be >= 1"),
    (MAX_N + 1, 1, "chol: n must be <= 131072"),
    (5, -1, "chol: n_rhs must be >= 0"),
    (5, MAX_RHS + 1, "chol: n_rhs must be <= 1048576"),
])
def test_rejections_name_their_argument(driver, n, n_rhs, text):
    p = plan(driver, n, n_rhs)
    assert not p["ok"] and p["error"] == text


# ---- the calls of tests/test_gpu_chol.py, which imports them from here ----------------------------------------------------------
# (n, n_rhs, lda - n, ldb - n_rhs, matrix): the small route at 1, 2, 5, 100 and kCholSmallN; the blocked route at
# kCholSmallN + 1, around a panel boundary with three panels, and 704 = 11 panels; n_rhs 1, 3 and 65 (two column tiles); padded
# strides; every kind of matrix at least once per route
SMALL_NS = (1, 2, 5, 100, SMALL_N)
BLOCKED_NS = (SMALL_N + 1, 3 * NB - 1, 3 * NB, 3 * NB + 1, 704)


def _gpu_calls():
    calls = [(n, 3, 0, 0, "gram") for n in SMALL_NS + BLOCKED_NS]
    calls += [(n, 1, 0, 0, kind) for n in (5, 100, SMALL_N + 1, 3 * NB + 1) for kind in ("lehmer", "kms", "scaled")]
    calls += [(704, 1, 0, 0, "kms"), (704, 3, 0, 0, "scaled")]
    calls += [(100, 65, 0, 0, "gram"), (3 * NB + 1, 65, 0, 0, "gram"), (3 * NB - 1, 1, 0, 0, "lehmer")]
    calls += [(100, 3, 5, 2, "gram"), (3 * NB + 1, 3, 7, 1, "scaled"), (3 * NB, 65, 1, 3, "kms")]
    return calls


GPU_CALLS = _gpu_calls()


def test_gpu_calls_take_both_routes_with_every_kind(driver):
    seen = {(plan(driver, c[0], c[1])["route"], c[4]) for c in GPU_CALLS}
    assert seen == {(r, kind) for r in (SMALL, BLOCKED) for kind in ("gram", "lehmer", "kms", "scaled")}
    assert {c[0] for c in GPU_CALLS} >= set(SMALL_NS + BLOCKED_NS)
    assert {c[1] for c in GPU_CALLS} >= {1, 3, 65}
    assert any(c[2] > 0 and c[3] > 0 for c in GPU_CALLS)
