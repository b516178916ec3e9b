"""The plan of the kernel-density kernels behind corrla_kde_eval_* and corrla_kde_nll_* (corrla_rs_amd/csrc/kde_plan.hpp),
pinned on the CPU: the header is host code, compiled here with the host compiler in a temporary directory.

For every row of SHAPES the driver prints the plan; pinned here: the point tiles cover [0, n_q) exactly once, the splits cover
the supports [0, n_s) exactly once in whole chunks with no empty split, the splits depend on n_q and n_s alone (never on the
number of bandwidths: a bandwidth's sums must not depend on its neighbours), there is one split when the points alone fill the
device and several when few points meet many supports, the launches cover the bandwidths in groups, the workspace stays
within the plan's stated bound, the reduction of the likelihood is a fixed tree of at most 256 ranges, and every rejection
carries the name of its argument.  The table ends with the calls of tests/test_gpu_kde.py (GPU_CALLS), built from the shape
tables below, which that file and tests/golden/kde/make_kde_golden.py import -- as tests/test_gpu_rbf.py imports its tables
from test_rbf_plan.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corrla_rs_amd", "csrc")
PDF, CDF, LOGPDF, NLL = 0, 1, 2, 3
THREADS, PP, QT, SC, HG, HL, MAX_H, RED_MAX = 256, 2, 512, 1024, 4, 8, 64, 256
TARGET = 4 * 256

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "kde_plan.hpp"
using namespace corrla;
int main(int argc, char** argv) {
  // n_q n_s n_h esz mode
  if (argc != 6) return 2;
  KdeShape s;
  s.n_q = atoll(argv[1]); s.n_s = atoll(argv[2]); s.n_h = atoll(argv[3]); s.esz = atoi(argv[4]); s.mode = (KdeMode)atoi(argv[5]);
  const KdePlan p = kde_plan(s);
  printf("ok %d\n", (int)p.ok);
  if (!p.ok) { printf("error %s\n", p.error); return 0; }
  printf("qt %d\nsc %d\nhg %d\nhl %d\nnacc %d\nnearest %d\nnqt %lld\nnchunks %lld\nnsplit %lld\nsplit_len %lld\nnlaunch %lld\n", p.qt, p.sc, p.hg,
         p.hl, p.nacc, (int)p.nearest, (long long)p.nqt, (long long)p.nchunks, (long long)p.nsplit, (long long)p.split_len, (long long)p.nlaunch);
  printf("nb_full %d\nnb_last %d\nblock %u\nnear_grid %u\nsum_full %u\nsum_last %u\nfinish %u %u\nred_blocks %u\nred_len %lld\n", p.nb_full,
         p.nb_last, p.block, p.near_grid_x, p.sum_grid_full, p.sum_grid_last, p.finish_grid_x, p.finish_block, p.red_blocks, (long long)p.red_len);
  printf("lds %zu\nws_min %zu\nws_sum %zu\nws_red %zu\nws %zu\nws_bound %zu\nroute %d\n", p.lds_bytes, p.ws_min_bytes, p.ws_sum_bytes,
         p.ws_red_bytes, p.ws_bytes, p.ws_bound, (int)p.route);
  printf("consts %d %d %d %d %d %d %d %d %lld\n", k::kKdeThreads, k::kKdePP, k::kKdeQT, k::kKdeSC, k::kKdeHG, k::kKdeHL, k::kKdeMaxH,
         k::kKdeRedMax, (long long)k::kKdeTargetWgs);
  return 0;
}
"""


def build_driver(tmp, csrc=CSRC):
    src = os.path.join(tmp, "kde_plan_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "kde_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + csrc, src, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("kde_plan")))


def plan(exe, n_q, n_s, n_h=1, esz=8, mode=PDF):
    out = subprocess.check_output([exe] + [str(v) for v in (n_q, n_s, n_h, esz, mode)], text=True)
    d = {}
    for line in out.splitlines():
        key, _, rest = line.partition(" ")
        d[key] = rest
    p = {"ok": int(d["ok"])}
    if not p["ok"]:
        p["error"] = d["error"]
        return p
    for key in d:
        if key in ("ok", "finish", "consts"):
            continue
        p[key] = int(d[key])
    p["finish"] = tuple(int(v) for v in d["finish"].split())
    p["consts"] = tuple(int(v) for v in d["consts"].split())
    return p


# ---- the shapes of tests/test_gpu_kde.py, which imports them from here: one table for both files -----------------------------
# (n_q, n_s, n_h); pdf, cdf and logpdf use the first bandwidth only
BASE = (2 * QT + 3, 2 * SC + 7, 3)
SPLIT_CASE = (5, 3 * SC + 5, 3)            # one point tile, four chunks: four splits, the last of 5 supports
NQ_VALUES = (1, QT)
NS_VALUES = (1, SC, SC + 1)
NH_VALUES = (1, HG, HG + 1, HL + 1, MAX_H)  # one group, a full group, a ragged group, a ragged launch, every launch full


def _replace(case, **kw):
    d = dict(zip(("n_q", "n_s", "n_h"), case))
    d.update(kw)
    return (d["n_q"], d["n_s"], d["n_h"])


def _gpu_calls():
    """one axis at a time from the base case, then the split case"""
    calls = [BASE]
    calls += [_replace(BASE, n_q=v) for v in NQ_VALUES]
    calls += [_replace(BASE, n_s=v) for v in NS_VALUES]
    calls += [_replace(BASE, n_h=v) for v in NH_VALUES]
    calls += [SPLIT_CASE]
    out = []
    for c in calls:
        if c not in out:
            out.append(c)
    return out


GPU_CALLS = _gpu_calls()
EXACT_CDF = (1, 128, 1)                    # a point equal to all of 128 coincident supports

SHAPES = [
    # the shapes of tools/bench_kde.py first
    (10 ** 6, 10 ** 5, 1), (10 ** 5, 10 ** 5, 1), (10 ** 5, 10 ** 5, 64), (60000, 140000, 64),
    (1, 1, 1), (7, 10 ** 6, 5), (QT * TARGET, 100 * SC, 3), (QT * TARGET - 1, 100 * SC, 3), (QT * TARGET // 2, 100 * SC, 64),
    (131, 71, 64), (3, 10 ** 7, 64),
] + GPU_CALLS + [EXACT_CDF]


@pytest.mark.parametrize("esz", (4, 8))
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "-".join(str(v) for v in c))
def test_plan_properties(driver, case, esz):
    n_q, n_s, n_h = case
    for mode in (PDF, CDF, LOGPDF, NLL):
        nh = n_h if mode == NLL else 1
        p = plan(driver, n_q, n_s, nh, esz, mode)
        assert p["ok"], p
        assert p["consts"] == (THREADS, PP, QT, SC, HG, HL, MAX_H, RED_MAX, TARGET) and QT == THREADS * PP and HL % HG == 0
        assert (p["qt"], p["sc"], p["hg"], p["hl"]) == (QT, SC, HG, HL) and p["block"] == THREADS
        nqt, nchunks, nsplit, split_len = p["nqt"], p["nchunks"], p["nsplit"], p["split_len"]
        assert (nqt - 1) * QT < n_q <= nqt * QT
        assert (nchunks - 1) * SC < n_s <= nchunks * SC
        # the splits: whole chunks, contiguous, none empty, together exactly [0, n_s)
        assert split_len % SC == 0 and 1 <= nsplit <= nchunks
        covered = 0
        for s in range(nsplit):
            lo, hi = s * split_len, min(n_s, (s + 1) * split_len)
            assert lo == covered and hi > lo
            covered = hi
        assert covered == n_s
        # chosen from n_q and n_s alone: one split when the tiles alone reach the target, else the target is reached whenever
        # the supports allow it
        if nqt >= TARGET:
            assert nsplit == 1
        else:
            assert nqt * nsplit >= TARGET or nsplit == nchunks
            assert nqt * nsplit < 4 * TARGET
        assert p["route"] == (2 if nsplit > 1 else 1)
        # the launches cover the bandwidths, the groups of a launch its bandwidths
        assert p["nlaunch"] == -(-nh // HL) and p["nb_full"] == min(nh, HL)
        assert (p["nlaunch"] - 1) * HL + p["nb_last"] == nh and 1 <= p["nb_last"] <= HL
        assert p["sum_full"] == nqt * nsplit * -(-p["nb_full"] // HG) < 2 ** 31
        assert p["sum_last"] == nqt * nsplit * -(-p["nb_last"] // HG)
        assert p["nearest"] == (mode != CDF) and p["near_grid"] == (0 if mode == CDF else nqt * nsplit)
        assert p["nacc"] == (2 if mode == NLL else 1)
        assert p["lds"] == SC * esz <= 64 * 1024
        # the workspace: the three arrays, each rounded up to 256 bytes, within the stated bound
        assert p["ws_min"] == (0 if mode == CDF else nsplit * n_q * esz)
        assert p["ws_sum"] == nsplit * p["nacc"] * p["nb_full"] * n_q * esz
        r256 = lambda b: -(-b // 256) * 256  # noqa: E731
        assert p["ws"] == r256(p["ws_min"]) + r256(p["ws_sum"]) + r256(p["ws_red"])
        bound = max(n_q, 4 * TARGET * QT) * (p["nacc"] * min(nh, HL) + 1) * esz + nh * RED_MAX * 16 + 768
        assert p["ws"] <= p["ws_bound"] == bound
        if mode == NLL:
            rb, rl = p["red_blocks"], p["red_len"]
            assert 1 <= rb <= RED_MAX and rl % 256 == 0 and (rb - 1) * rl < n_q <= rb * rl
            assert p["ws_red"] == nh * rb * 16 and p["finish"][0] == 0
        else:
            assert p["finish"] == (-(-n_q // 256), 256) and p["red_blocks"] == 0 and p["ws_red"] == 0


def test_splits_do_not_depend_on_the_bandwidths(driver):
    for n_q, n_s in ((BASE[0], BASE[1]), SPLIT_CASE[:2], (10 ** 5, 10 ** 5), (7, 10 ** 6)):
        plans = [plan(driver, n_q, n_s, n_h, 4, NLL) for n_h in (1, HG, HG + 1, HL, HL + 1, MAX_H)]
        assert len({(p["nsplit"], p["split_len"], p["red_blocks"], p["red_len"]) for p in plans}) == 1
        # ... and the evaluation entries split as the likelihood does
        assert plan(driver, n_q, n_s, 1, 4, LOGPDF)["nsplit"] == plans[0]["nsplit"]


def test_tile_chunk_and_group_counts_at_their_edges(driver):
    assert [plan(driver, n_q, 10)["nqt"] for n_q in (1, QT - 1, QT, QT + 1)] == [1, 1, 1, 2]
    assert [plan(driver, 10, n_s)["nchunks"] for n_s in (SC - 1, SC, SC + 1, 2 * SC, 2 * SC + 1)] == [1, 1, 2, 2, 3]
    assert [plan(driver, 10, 10, n_h, 8, NLL)["nlaunch"] for n_h in (1, HL, HL + 1, MAX_H)] == [1, 1, 2, MAX_H // HL]
    assert [plan(driver, 10, 10, n_h, 8, NLL)["sum_last"] for n_h in (1, HG, HG + 1, HL, HL + 1)] == [1, 1, 2, 2, 1]
    assert [plan(driver, n_q, 10, 1, 8, NLL)["red_blocks"] for n_q in (1, 256, 257, 256 * 256, 256 * 256 + 1, 10 ** 7)] == [1, 1, 2, 256, 129, 256]


def test_one_split_for_many_points_and_several_for_few(driver):
    assert plan(driver, 10 ** 6, 10 ** 5)["nsplit"] == 1
    assert plan(driver, QT * TARGET, 100 * SC)["nsplit"] == 1
    assert plan(driver, QT * TARGET // 2, 100 * SC)["nsplit"] == 2
    p = plan(driver, 5, 10 ** 7)
    assert p["nsplit"] > 1 and p["nsplit"] * p["nqt"] >= TARGET
    p = plan(driver, 5, 10 ** 6)                       # fewer chunks than the target: a split per chunk
    assert p["nsplit"] == p["nchunks"] == 977
    # never more splits than chunks; the split case of the GPU file: at least three splits, the last one shorter
    p = plan(driver, *SPLIT_CASE[:2], SPLIT_CASE[2], 8, NLL)
    assert (p["nchunks"], p["nsplit"], p["split_len"]) == (4, 4, SC)
    assert p["nsplit"] >= 3 and SPLIT_CASE[1] - (p["nsplit"] - 1) * p["split_len"] == 5 < p["split_len"]


def test_rejections_carry_their_reason(driver):
    # (n_q, n_s, n_h, esz, mode)
    for args, word in (((5, 5, 1, 2, PDF), "esz"), ((5, 5, 1, 16, NLL), "esz"), ((0, 5, 1, 8, PDF), "n_q"), ((5, 0, 1, 8, CDF), "n_s"),
                       ((-1, 5, 1, 8, NLL), "n_q"), ((5, 5, 0, 8, NLL), "n_h must be in [1, 64]"), ((5, 5, 65, 8, NLL), "n_h must be in [1, 64]"),
                       ((5, 5, 2, 8, LOGPDF), "n_h must be 1"), ((2 ** 42, 5, 1, 8, PDF), "workgroups"),
                       ((2 ** 40 - 1, 5, 64, 8, NLL), "workgroups")):
        p = plan(driver, *args)
        assert not p["ok"] and word in p["error"], (args, p)


def test_the_gpu_files_calls_reach_every_edge(driver):
    """what tests/test_gpu_kde.py runs: every listed value of every axis, more than one tile, chunk, group, launch and split"""
    assert BASE in GPU_CALLS and SPLIT_CASE in GPU_CALLS and len(GPU_CALLS) == len(set(GPU_CALLS)) <= 16
    for v in NQ_VALUES:
        assert _replace(BASE, n_q=v) in GPU_CALLS
    for v in NS_VALUES:
        assert _replace(BASE, n_s=v) in GPU_CALLS
    for v in NH_VALUES:
        assert _replace(BASE, n_h=v) in GPU_CALLS
    plans = [plan(driver, *c, 4, NLL) for c in GPU_CALLS]
    assert any(p["nqt"] > 2 for p in plans) and any(p["nchunks"] > 2 for p in plans)
    assert any(p["nlaunch"] > 1 and p["nb_last"] < HL for p in plans) and any(p["nlaunch"] == MAX_H // HL for p in plans)
    assert any(p["nb_last"] % HG for p in plans) and any(p["nsplit"] >= 3 for p in plans)
    # the base case itself splits its three chunks: every accuracy case but n_s <= SC adds partial sums
    assert plan(driver, *BASE, 4, NLL)["nsplit"] == 3
