"""The plan of the symmetric eigensolver behind corrla_eigh_* (corrla_rs_amd/csrc/eigh_plan.hpp), pinned on the CPU: the header
is host code, compiled here with the host compiler in a temporary directory.

Pinned: the route at every n (the boundary sits at 64 / 65); the tournament for 2, 3, 4, 5 and 9 blocks -- every unordered
pair exactly once per sweep, the pairs of a round disjoint, the smaller block first -- and for the 64 indices of the LDS
Jacobi; slabs that are whole chunks of 64 rows and cover every row; grids; LDS images within 160 KiB; the workspace as the sum
of its stated pieces; the launch counts; every rejection names its argument.  The numpy restatement of the algorithm
(tests/eigh_reference.py) is run on the small cases and held against LAPACK within a quarter of the fixed caps.  The module
ends with the shapes of tests/test_gpu_eigh.py (GPU_CALLS), which that file imports."""
import os
import subprocess

import numpy as np
import pytest

from tests import eigh_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corrla_rs_amd", "csrc")
B, PAIR, SMALL_N, THREADS, CHUNK, MAX_SWEEPS, INNER, GROUP, MAX_N = 32, 64, 64, 256, 64, 40, 1, 2, 32768
LDS_MAX = 160 * 1024
SMALL, BLOCKED = 1, 2

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "eigh_plan.hpp"
using namespace corrla;
int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "schedule")) {  // schedule nb: round, i, j per pair
    const long long nb = atoll(argv[2]);
    for (long long r = 0; r < eigh_rounds(nb); ++r)
      for (long long p = 0; p < eigh_pairs(nb); ++p) {
        int64_t i, j;
        eigh_pair(nb, r, p, &i, &j);
        printf("%lld %lld %lld\n", r, (long long)i, (long long)j);
      }
    return 0;
  }
  if (argc != 3) return 2;
  EighShape s;
  s.n = atoll(argv[1]); s.num_cus = atoi(argv[2]);
  const EighPlan p = eigh_plan(s);
  printf("ok %d\n", (int)p.ok);
  if (!p.ok) { printf("error %s\n", p.error); return 0; }
  printf("route %d\nnb %lld\nrounds %lld\npairs %lld\nslabs %lld\nslab_rows %lld\nnorm_groups %lld\n", (int)p.route, (long long)p.nb,
         (long long)p.rounds, (long long)p.pairs, (long long)p.slabs, (long long)p.slab_rows, (long long)p.norm_groups);
  printf("chol_launches %lld\nprologue_launches %lld\nsweep_launches %lld\nfinish_launches %lld\nlaunches10 %lld\n", (long long)p.chol_launches,
         (long long)p.prologue_launches, (long long)p.sweep_launches, (long long)p.finish_launches, (long long)p.launches(10));
  printf("lds_gram %zu\nlds_apply %zu\nlds_jac %zu\nlds_small %zu\nlds_ray %zu\n", p.lds_gram, p.lds_apply, p.lds_jac, p.lds_small, p.lds_ray);
  printf("ws_header %zu\nws_norms %zu\nws_b %zu\nws_w %zu\nws_gram %zu\nws_r %zu\nws_meas %zu\nws_records %zu\nws_cols %zu\nws_ray %zu\nws_chol %zu\nws_bytes %zu\n",
         p.ws_header, p.ws_norms, p.ws_b, p.ws_w, p.ws_gram, p.ws_r, p.ws_meas, p.ws_records, p.ws_cols, p.ws_ray, p.ws_chol, p.ws_bytes);
  printf("tol %.17g\n", p.tol);
  printf("consts %d %d %d %d %d %d %d %d %lld %zu %zu %zu\n", k::kEighB, k::kEighPair, k::kEighSmallN, k::kEighThreads, k::kEighChunk,
         k::kEighMaxSweeps, k::kEighInnerSweeps, k::kEighGroup, (long long)k::kEighMaxN, k::kLdsMaxBytes, sizeof(EighHeader),
         sizeof(EighSweepRecord));
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("eigh_plan"))
    src = os.path.join(tmp, "eigh_plan_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "eigh_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, src, "-o", exe])
    return exe


def plan(exe, n, cus=256):
    out = subprocess.check_output([exe, str(n), str(cus)], text=True)
    d = dict(line.partition(" ")[::2] for line in out.splitlines())
    p = {"ok": int(d["ok"])}
    if not p["ok"]:
        p["error"] = d["error"]
        return p
    for key, v in d.items():
        if key == "tol":
            p[key] = float(v)
        elif key not in ("ok", "consts"):
            p[key] = int(v)
    p["consts"] = tuple(int(v) for v in d["consts"].split())
    return p


def schedule(exe, nb):
    out = subprocess.check_output([exe, "schedule", str(nb)], text=True)
    return [tuple(int(v) for v in line.split()) for line in out.splitlines()]


def chol_launches(n):
    return 1 if n <= 128 else 3 * -(-n // 64) - 2 + 1   # tests/test_chol_plan.py pins these


PLAN_N = (1, 2, 5, 63, 64, 65, 96, 129, 200, 257, 2048, 8192, MAX_N)


def test_constants(driver):
    assert plan(driver, 100)["consts"] == (B, PAIR, SMALL_N, THREADS, CHUNK, MAX_SWEEPS, INNER, GROUP, MAX_N, LDS_MAX, 64, 16)


@pytest.mark.parametrize("n", PLAN_N)
def test_route_geometry_and_counts(driver, n):
    p = plan(driver, n)
    assert p["ok"] and p["route"] == (SMALL if n <= SMALL_N else BLOCKED)
    assert p["tol"] == 2.0 * np.sqrt(n) * 2.0 ** -53
    assert p["lds_gram"] <= 65536 and p["lds_apply"] <= LDS_MAX and p["lds_jac"] <= LDS_MAX
    assert p["lds_gram"] == CHUNK * 80 * 8 and p["lds_apply"] == (CHUNK * 66 + PAIR * 80) * 8
    assert p["lds_jac"] == (2 * PAIR * (PAIR + 1) + 2 * B + 2 * THREADS) * 8 and p["lds_small"] == p["lds_jac"] + PAIR * (PAIR + 1) * 8 <= LDS_MAX
    assert p["lds_ray"] == (64 * 80 + 64 * 48) * 8 <= LDS_MAX
    if n <= SMALL_N:
        assert p["prologue_launches"] == 1 and p["ws_bytes"] == 256 and p["launches10"] == 1
        return
    nb = -(-n // B)
    assert p["nb"] == nb and p["rounds"] == nb + (nb & 1) - 1 and p["pairs"] == nb // 2
    chunks = -(-n // CHUNK)
    assert p["norm_groups"] == chunks
    # the slabs: whole chunks, every row covered, none empty, two workgroups per CU where the rows allow
    assert p["slab_rows"] % CHUNK == 0 and (p["slabs"] - 1) * p["slab_rows"] < n <= p["slabs"] * p["slab_rows"]
    assert p["slabs"] <= max(1, -(-512 // p["pairs"])) and (p["slabs"] == chunks or p["pairs"] * p["slabs"] >= min(512, p["pairs"] * chunks) // 2)
    assert p["pairs"] * p["slabs"] < 2 ** 31
    assert p["chol_launches"] == chol_launches(n)
    assert p["prologue_launches"] == 2 + 1 + chol_launches(n) + 1
    assert p["sweep_launches"] == 3 * p["rounds"] + 1 and p["finish_launches"] == 6
    assert p["launches10"] == p["prologue_launches"] + 10 * p["sweep_launches"] + 6

    def r256(b):
        return (b + 255) // 256 * 256
    assert p["ws_b"] == r256(n * n * 8) and p["ws_w"] == r256(nb * n * B * 8)
    assert p["ws_gram"] == r256(p["pairs"] * p["slabs"] * PAIR * PAIR * 8) and p["ws_r"] == r256(p["pairs"] * PAIR * PAIR * 8)
    assert p["ws_meas"] == r256(p["rounds"] * p["pairs"] * 16) and p["ws_records"] == r256((MAX_SWEEPS + GROUP) * 16)
    assert p["ws_norms"] == r256(chunks * 32) and p["ws_cols"] == r256(nb * B * 24) and p["ws_ray"] == r256(nb * chunks * B * 8)
    assert p["ws_bytes"] == sum(p[k] for k in ("ws_header", "ws_norms", "ws_b", "ws_w", "ws_gram", "ws_r", "ws_meas", "ws_records", "ws_cols", "ws_ray", "ws_chol"))
    # B and W (16 n^2), the partial quotients (n^2 / 8), at most 512 + pairs Gram tiles and pairs rotations of 32 KiB, the rest
    assert p["ws_bytes"] <= 16 * n * n + n * n // 8 + 1100 * n + 18 * 2 ** 20


def test_slabs_follow_the_cu_count(driver):
    few, many = plan(driver, 2048, 64), plan(driver, 2048, 256)
    assert few["slabs"] == 4 and many["slabs"] == 16 and few["pairs"] == many["pairs"] == 32
    assert few["slab_rows"] == 512 and many["slab_rows"] == 128


@pytest.mark.parametrize("nb", (2, 3, 4, 5, 9, PAIR))
def test_tournament(driver, nb):
    rows = schedule(driver, nb)
    rounds = nb + (nb & 1) - 1
    assert len(rows) == rounds * (nb // 2)
    assert sorted((i, j) for _, i, j in rows) == [(i, j) for i in range(nb) for j in range(i + 1, nb)]   # each pair once
    for r in range(rounds):
        blocks = [b for rr, i, j in rows if rr == r for b in (i, j)]
        assert len(blocks) == 2 * (nb // 2) == len(set(blocks))                                        # disjoint
        assert [(i, j) for rr, i, j in rows if rr == r] == R.tournament(nb, r)                          # the restatement's


def test_rejections_name_the_argument(driver):
    assert plan(driver, 0) == {"ok": 0, "error": "eigh: n must be >= 1"}
    assert plan(driver, MAX_N + 1) == {"ok": 0, "error": "eigh: n must be <= 32768"}


# the restatement against LAPACK on the small cases: it has to stay under a quarter of every cap
SMALL_CASES = [(f, n) for f in R.FAMILIES for n in (1, 2, 5, 33, 64)] + [("gauss", 65), ("pm", 65)]


@pytest.mark.parametrize("name,n", SMALL_CASES)
def test_restatement_against_lapack(name, n):
    a = R.family(name, n)
    poisoned = a + np.triu(np.full((n, n), np.nan), 1)   # the strict upper triangle is never read
    w, v, sweeps = R.restatement(poisoned)
    got = R.ratios(a, w, v)
    print(name, n, sweeps, got)
    assert np.all(np.diff(w) >= 0) and R.sign_convention_holds(v)
    assert R.within_restatement_limits(got)
    assert sweeps <= 20 and (sweeps == 0) == (name in ("diag", "zero") or n == 1 or not np.any(np.tril(a, -1)))


def test_golden_covers_the_gpu_calls():
    gold = R.load_golden()
    assert sorted(gold) == sorted(R.case_id(f, n) for f, n in GPU_CALLS)
    for key, rec in gold.items():
        assert set(rec) == {"sweeps", "residual", "orth", "eig", "lapack_residual", "lapack_orth"}, key
        assert R.within_restatement_limits(rec), key
        assert 0 <= rec["sweeps"] <= 30, key   # the device may take 3 more and stays clear of the cap of 40


# The shapes of tests/test_gpu_eigh.py: every family on both routes.  1, 2, 5, 63, 64: the small route and its edge; 65: the
# first blocked size, three blocks, the last one column wide, a bye; 96: three full blocks; 129: five blocks; 200: a partial last
# block; 257: nine blocks.
GPU_N = (1, 2, 5, 63, 64, 65, 96, 129, 200, 257)
GPU_CALLS = [(f, n) for n in GPU_N for f in R.FAMILIES]


def test_gpu_calls_cover_both_routes_and_every_block_count(driver):
    assert len(GPU_CALLS) == len(set(GPU_CALLS)) == len(GPU_N) * len(R.FAMILIES)
    plans = {n: plan(driver, n) for n in GPU_N}
    assert [plans[n]["route"] for n in GPU_N] == [SMALL] * 5 + [BLOCKED] * 5
    assert [plans[n]["nb"] for n in GPU_N[5:]] == [3, 3, 5, 7, 9]
    assert 65 % B == 1 and 200 % B != 0 and 96 % B == 0
