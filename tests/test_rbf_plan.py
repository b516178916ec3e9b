"""The plan of the radial-basis-function kernels behind corrla_rbf_apply_* and corrla_rbf_matrix_*
(corrla_rs_amd/csrc/rbf_plan.hpp), pinned on the CPU: the header is host code, compiled here with the host compiler in a
temporary directory.

For every row of SHAPES the driver prints the plan; pinned here: the query tiles and the column groups cover [0, n_q) and
[0, n_rhs) exactly once, the splits cover the supports [0, n_s) exactly once in whole chunks with no empty split, there is one
split when the queries alone fill the device and several when few queries meet many supports, the dynamic LDS stays within
160 KiB, the workspace within the plan's stated bound, and every rejection carries the name of its argument.  The table
ends with the calls of tests/test_gpu_rbf.py (GPU_CALLS), built from the shape tables below, which that file imports -- as
tests/test_gpu_pca_apply.py imports its tables from test_pca_apply_plan.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corrla_rs_amd", "csrc")
APPLY, MATRIX = 0, 1
BM, KC, RG, MN, MAX_DIM, THREADS = 64, 32, 64, 64, 128, 256
TARGET = 4 * 256

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "rbf_plan.hpp"
using namespace corrla;
int main(int argc, char** argv) {
  // n_q n_s dim n_rhs n_poly esz mode
  if (argc == 3) { printf("terms %lld\n", (long long)rbf_poly_terms(atoll(argv[1]), atoi(argv[2]))); return 0; }
  if (argc != 8) return 2;
  RbfShape s;
  s.n_q = atoll(argv[1]); s.n_s = atoll(argv[2]); s.dim = atoll(argv[3]); s.n_rhs = atoll(argv[4]); s.n_poly = atoll(argv[5]);
  s.esz = atoi(argv[6]); s.mode = atoi(argv[7]) ? RbfMode::kMatrix : RbfMode::kApply;
  const RbfPlan p = rbf_plan(s);
  printf("ok %d\n", (int)p.ok);
  if (!p.ok) { printf("error %s\n", p.error); return 0; }
  printf("bm %d\nkc %d\nrg %d\nnbm %lld\nnrg %lld\nnchunks %lld\nnsplit %lld\nsplit_len %lld\n", p.bm, p.kc, p.rg, (long long)p.nbm,
         (long long)p.nrg, (long long)p.nchunks, (long long)p.nsplit, (long long)p.split_len);
  printf("grid %u\nblock %u\nlds %zu\nws %zu\nws_bound %zu\nfinish %u %u\n", p.grid_x, p.block, p.lds_bytes, p.ws_bytes, p.ws_bound,
         p.finish_grid_x, p.finish_block);
  printf("consts %d %d %d %d %d %d %d %lld %zu\n", k::kRbfBM, k::kRbfKC, k::kRbfRG, k::kRbfMN, k::kRbfMaxDim, k::kRbfThreads, k::kRbfWLd,
         (long long)k::kRbfTargetWgs, k::kLdsMaxBytes);
  return 0;
}
"""


def build_driver(tmp, csrc=CSRC):
    src = os.path.join(tmp, "rbf_plan_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "rbf_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + csrc, src, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("rbf_plan")))


def plan(exe, n_q, n_s, dim, n_rhs=1, n_poly=0, esz=8, mode=APPLY):
    out = subprocess.check_output([exe] + [str(v) for v in (n_q, n_s, dim, n_rhs, n_poly, esz, mode)], text=True)
    d = {}
    for line in out.splitlines():
        key, _, rest = line.partition(" ")
        d[key] = rest
    p = {"ok": int(d["ok"])}
    if not p["ok"]:
        p["error"] = d["error"]
        return p
    for key in ("bm", "kc", "rg", "nbm", "nrg", "nchunks", "nsplit", "split_len", "grid", "block", "lds", "ws", "ws_bound"):
        p[key] = int(d[key])
    p["finish"] = tuple(int(v) for v in d["finish"].split())
    p["consts"] = tuple(int(v) for v in d["consts"].split())
    return p


def poly_terms(dim, degree):
    """rbf_poly_terms restated: degree None or < 0 no tail, 0 or 1 [x, 1], >= 2 [x, x_a x_b (a <= b), 1]"""
    if degree is None or degree < 0:
        return 0
    return dim + 1 if degree < 2 else dim + dim * (dim + 1) // 2 + 1


# ---- the shapes of tests/test_gpu_rbf.py, which imports them from here: one table for both files ---------------------------
# (n_q, n_s, dim, n_rhs, poly_degree)
BASE = (2 * BM + 3, 2 * KC + 7, 3, 17, 1)
SPLIT_CASE = (5, 3 * KC + 5, 3, 17, 1)      # one query tile, four chunks: four splits, the last of 5 supports
NQ_VALUES = (1, BM - 1, BM, BM + 1)
NS_VALUES = (1, 3, 4, 5, KC - 1, KC, KC + 1)
NRHS_VALUES = (1, 15, 16, RG, RG + 1)
DIM_VALUES = (1, 2, 17, 128)
DEGREES = (None, 1, 2)
DEGREE2_MAX_DIM = 17
EXACT_NS = (KC - 1, KC + 1, SPLIT_CASE[1])   # phi == 1: every support counted once ...
EXACT_NRHS = (1, RG + 1)                    # ... across chunk, split and column-group boundaries


def _replace(case, **kw):
    d = dict(zip(("n_q", "n_s", "dim", "n_rhs", "degree"), case))
    d.update(kw)
    return (d["n_q"], d["n_s"], d["dim"], d["n_rhs"], d["degree"])


def _gpu_calls():
    """one axis at a time from the base case, then the split case"""
    calls = [BASE]
    calls += [_replace(BASE, n_q=v) for v in NQ_VALUES]
    calls += [_replace(BASE, n_s=v) for v in NS_VALUES]
    calls += [_replace(BASE, n_rhs=v) for v in NRHS_VALUES]
    calls += [_replace(BASE, dim=v) for v in DIM_VALUES]
    calls += [_replace(BASE, degree=v) for v in DEGREES if v != BASE[4]]
    calls += [_replace(BASE, dim=DEGREE2_MAX_DIM, degree=2)]
    calls += [SPLIT_CASE]
    out = []
    for c in calls:
        if c not in out:
            out.append(c)
    return out


GPU_CALLS = _gpu_calls()
EXACT_CALLS = [(BM + 1 if n_s != SPLIT_CASE[1] else SPLIT_CASE[0], n_s, 3, n_rhs, None) for n_s in EXACT_NS for n_rhs in EXACT_NRHS]

SHAPES = [
    # the shapes of tools/bench_rbf.py first
    (10 ** 6, 4096, 3, 1, None), (10 ** 6, 4096, 3, 32, None), (10 ** 5, 16384, 16, 32, None),
    (10 ** 5, 10 ** 4, 3, 1, 1), (20, 20, 1, 8, 1), (7, 10 ** 6, 2, 3, 2), (1, 1, 1, 1, None), (300, 5000, 128, 130, 1),
    (BM * TARGET, 100 * KC, 3, 1, None), (BM * TARGET - 1, 100 * KC, 3, 1, None),
] + GPU_CALLS + EXACT_CALLS


@pytest.mark.parametrize("esz", (4, 8))
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "-".join(str(v) for v in c))
def test_apply_plan_properties(driver, case, esz):
    n_q, n_s, dim, n_rhs, degree = case
    n_poly = poly_terms(dim, degree)
    p = plan(driver, n_q, n_s, dim, n_rhs, n_poly, esz, APPLY)
    assert p["ok"], p
    assert (p["bm"], p["kc"], p["rg"]) == (BM, KC, RG) and p["consts"][:6] == (BM, KC, RG, MN, MAX_DIM, THREADS)
    assert KC % 4 == 0 and p["consts"][7] == TARGET and p["consts"][8] == 160 * 1024
    nbm, nrg, nchunks, nsplit, split_len = p["nbm"], p["nrg"], p["nchunks"], p["nsplit"], p["split_len"]
    # tiles, column groups and chunks: each covers its range once, the last one may be short
    assert (nbm - 1) * BM < n_q <= nbm * BM
    assert (nrg - 1) * RG < n_rhs <= nrg * RG
    assert (nchunks - 1) * KC < n_s <= nchunks * KC
    # the splits: whole chunks, contiguous, none empty, together exactly [0, n_s)
    assert split_len % KC == 0 and 1 <= nsplit <= nchunks
    covered = 0
    for s in range(nsplit):
        lo, hi = s * split_len, min(n_s, (s + 1) * split_len)
        assert lo == covered and hi > lo
        covered = hi
    assert covered == n_s
    # chosen from the shape alone: one split when the tiles alone reach the target, else the target is reached whenever the
    # supports allow it
    tiles = nbm * nrg
    if tiles >= TARGET:
        assert nsplit == 1
    else:
        assert tiles * nsplit >= TARGET or nsplit == nchunks
        assert tiles * nsplit < 4 * TARGET
    assert p["grid"] == tiles * nsplit < 2 ** 31 and p["block"] == THREADS
    wld = p["consts"][6]
    assert wld == RG + 2
    assert p["lds"] == (dim * (BM + KC) + KC * wld) * esz <= 160 * 1024
    assert p["ws"] == nsplit * n_q * n_rhs * esz <= p["ws_bound"] == max(n_q * n_rhs, 4 * TARGET * BM * RG) * esz
    assert p["finish"] == ((n_q * n_rhs + 255) // 256, 256)


def test_tile_chunk_and_group_counts_at_their_edges(driver):
    assert [plan(driver, n_q, 10, 3)["nbm"] for n_q in (1, 63, 64, 65)] == [1, 1, 1, 2]
    assert [plan(driver, 10, n_s, 3)["nchunks"] for n_s in (KC - 1, KC, KC + 1, 2 * KC, 2 * KC + 1)] == [1, 1, 2, 2, 3]
    assert [plan(driver, 10, 10, 3, n_rhs)["nrg"] for n_rhs in (1, 64, 65, 128, 129)] == [1, 1, 2, 2, 3]
    # the largest dim in f64 is the largest LDS image, and it stays well under the limit
    assert plan(driver, 10, 10, 128, esz=8)["lds"] == 115200 < 120 * 1024
    assert plan(driver, 10, 10, 3, esz=8)["lds"] == 19200


def test_one_split_for_many_queries_and_several_for_few(driver):
    assert plan(driver, 10 ** 6, 4096, 3)["nsplit"] == 1
    assert plan(driver, BM * TARGET, 100 * KC, 3)["nsplit"] == 1
    assert plan(driver, BM * TARGET // 2, 100 * KC, 3)["nsplit"] == 2
    p = plan(driver, 5, 10 ** 5, 3)
    assert p["nsplit"] > 1 and p["nsplit"] * p["nbm"] * p["nrg"] >= TARGET
    # never more splits than chunks
    p = plan(driver, 5, 3 * KC + 5, 3)
    assert (p["nchunks"], p["nsplit"], p["split_len"]) == (4, 4, KC)
    # the split case of the GPU file: at least three splits, the last one shorter
    p = plan(driver, *SPLIT_CASE[:4], poly_terms(SPLIT_CASE[2], SPLIT_CASE[4]))
    assert p["nsplit"] >= 3 and SPLIT_CASE[1] - (p["nsplit"] - 1) * p["split_len"] < p["split_len"]


@pytest.mark.parametrize("esz", (4, 8))
def test_matrix_plan(driver, esz):
    for n_q, n_s, dim in ((1, 1, 1), (2 * BM + 3, 2 * KC + 7, 3), (BM, MN, 128), (BM + 1, MN + 1, 17), (10 ** 5, 10 ** 4, 3)):
        p = plan(driver, n_q, n_s, dim, esz=esz, mode=MATRIX)
        assert p["ok"], p
        assert (p["nbm"] - 1) * BM < n_q <= p["nbm"] * BM and (p["nrg"] - 1) * MN < n_s <= p["nrg"] * MN
        assert p["grid"] == p["nbm"] * p["nrg"] and p["block"] == THREADS
        assert p["lds"] == dim * (BM + MN) * esz <= 160 * 1024
        assert p["ws"] == 0 == p["ws_bound"] and p["finish"][0] == 0


def test_poly_terms(driver):
    def terms(dim, degree):
        return int(subprocess.check_output([driver, str(dim), str(degree)], text=True).split()[1])
    for dim in (1, 2, 3, 17, 128):
        assert terms(dim, -1) == 0 and terms(dim, -5) == 0
        assert terms(dim, 0) == terms(dim, 1) == dim + 1
        assert terms(dim, 2) == terms(dim, 3) == dim + dim * (dim + 1) // 2 + 1
        for degree in (None, -1, 0, 1, 2):
            assert terms(dim, -1 if degree is None else degree) == poly_terms(dim, degree)
    assert terms(3, 2) == 10        # x1 x2 x3, x1x1 x1x2 x1x3 x2x2 x2x3 x3x3, 1


def test_rejections_carry_their_reason(driver):
    # (n_q, n_s, dim, n_rhs, n_poly, esz, mode)
    for args, word in (((5, 5, 3, 1, 0, 2), "esz"), ((5, 5, 3, 1, 0, 16), "esz"), ((0, 5, 3, 1, 0, 8), "n_q"), ((5, 0, 3, 1, 0, 8), "n_s"),
                       ((5, 5, 3, 0, 0, 8), "n_rhs"), ((5, 5, 0, 1, 0, 8), "dim"), ((5, 5, 129, 1, 0, 8), "dim"),
                       ((5, 5, 3, 1, -1, 8), "n_poly"), ((0, 5, 3, 1, 0, 8, MATRIX), "n_q"), ((5, 5, 129, 1, 0, 8, MATRIX), "dim"),
                       ((2 ** 40, 5, 3, 2 ** 20, 0, 8), "tiles"), ((2 ** 36, 2 ** 36, 3, 1, 0, 8, MATRIX), "tiles"),
                       ((2 ** 36, 5, 3, 64, 0, 8), "finishing")):
        p = plan(driver, *args)
        assert not p["ok"] and word in p["error"], (args, p)


def test_the_gpu_files_calls_reach_every_edge(driver):
    """what tests/test_gpu_rbf.py runs: every listed value of every axis, more than one tile, chunk, column group and split"""
    assert BASE in GPU_CALLS and SPLIT_CASE in GPU_CALLS and len(GPU_CALLS) == len(set(GPU_CALLS)) <= 30
    for v in NQ_VALUES:
        assert _replace(BASE, n_q=v) in GPU_CALLS
    for v in NS_VALUES:
        assert _replace(BASE, n_s=v) in GPU_CALLS
    for v in NRHS_VALUES:
        assert _replace(BASE, n_rhs=v) in GPU_CALLS
    for v in DIM_VALUES:
        assert _replace(BASE, dim=v) in GPU_CALLS
    assert {c[4] for c in GPU_CALLS} == set(DEGREES)
    assert all(c[2] <= DEGREE2_MAX_DIM for c in GPU_CALLS if c[4] == 2)
    plans = [plan(driver, *c[:4], poly_terms(c[2], c[4])) for c in GPU_CALLS]
    assert any(p["nbm"] > 1 for p in plans) and any(p["nrg"] > 1 for p in plans) and any(p["nchunks"] > 2 for p in plans)
    assert any(p["nsplit"] >= 3 for p in plans)
    for c in EXACT_CALLS:
        p = plan(driver, *c[:4], 0)
        assert p["nsplit"] > 1 or c[1] < KC
