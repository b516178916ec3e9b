"""The gradient stage's plan (corrla_rs_amd/csrc/grad_plan.hpp), pinned on the CPU: grad_plan is host code, compiled here
with the host compiler in a temporary directory.

Every call the stage accepted before the wide kernels existed must keep its kernels: EXPECTED_* below is that routing and
those LDS sizes, written from the former body of corrla_grad_mat_* in corrla_rsvd.hip (today grad_entry and grad_stage::run_entry) as it was (the validation, then the scan and fit choices and
the LDS helpers of grad_kernels.hpp / knn2_kernels.hpp), independent of grad_plan.  old_launches further down restates in
the same way the grids, workgroup sizes and workspaces that function computed beside the plan before the plan carried them."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMAX = 160 * 1024
NUM_CUS = 256
BUDGET = 4 << 30


# ---- the limited kernels' LDS, as grad_kernels.hpp / knn2_kernels.hpp compute it ----
def knn_lds(k, n):
    return k * 64 * 8 + 16 * k * 8 + 16 * n * 12 + 64


def mfma_slices(k):
    return 4 if k <= 16 else (8 if k <= 32 else 16)


def knn_mfma_lds(k, n, w):
    k4, qt, kd = (k + 3) & ~3, 16 * w, 4 * mfma_slices(k)
    return (qt * k4 + qt + kd * 80 + 64 + qt * n + qt) * 8 + (kd * 80 + qt * n + 1 + qt) * 4 + 64


def k2_lds(s):
    return 4 * (s * 8192 + 1024) + 12 * 512 + 1024


def lin_row_total(P):
    placed, end = [False] * 68, 0
    for _ in range(P + 1):
        pick, pad = -1, 0
        while pad < 16:
            res = (end + pad) & 15
            for r in range(P, -1, -1):
                if not placed[r] and (r & 15) == res:
                    pick = r
                    break
            if pick >= 0:
                break
            pad += 1
        placed[pick] = True
        end += pad + ((pick + 2) >> 1)
    return 2 * end


def fit_lin_lds(k, n):
    P = k + 1
    return (lin_row_total(P) + 2 * P) * 8 + (((n + 15) & ~15) + 16) * 4 + 128 * 2 + 64


def fit_lds(k, n, order, m_in_lds):
    P = k + 1 if order == 1 else k + k * (k + 1) // 2 + 1
    LM = (P + 1) | 1
    return (n * k + n + (P * LM if m_in_lds else 0) + k + 2 * P) * 8 + (2 * P + 4 + n) * 4 + 64


def old_routing(n_pts, k, n_q, order, n, knn_mode, fit_mode):
    """the entry of corrla_grad_mat_* (today grad_entry / grad_stage::run_entry) before the wide kernels: None when it rejected the call, else (scan, fit) descriptions"""
    need = k + 1 if order == 1 else k * (k + 3) // 2
    if k > 64 or not (n_pts > need and n > need) or n > n_pts or n > 512 or fit_lds(k, n, order, False) > KMAX:
        return None
    if (knn_mode == 3 or (knn_mode == 0 and n_pts >= 8192)) and n <= 128:
        s = 1 if k <= 32 else 2
        scan = ("knn2", 0, 0, s, k2_lds(s))
    elif knn_mode == 1 or (knn_mode == 0 and n_pts < 131072) or knn_mfma_lds(k, n, 2) > KMAX:
        scan = ("valu", 0, 0, 0, knn_lds(k, n))
    else:
        w = 4 if knn_mfma_lds(k, n, 4) <= KMAX else 2
        scan = ("mfma", w, mfma_slices(k), 0, knn_mfma_lds(k, n, w))
    if order == 1 and fit_mode != 1:
        fit = ("lin", min(5, (k + 2 + 15) // 16), fit_lin_lds(k, n))
    elif fit_lds(k, n, order, True) <= KMAX:
        fit = ("lds", 0, fit_lds(k, n, order, True))
    else:
        fit = ("global", 0, fit_lds(k, n, order, False))
    return scan, fit


MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "grad_plan.hpp"
int main(int argc, char** argv) {
  const char* scans[] = {"valu", "mfma", "knn2", "wide"};
  const char* fits[] = {"lin", "lds", "global", "wide"};
  long long np, kf, nq, n, budget;
  int order, km, fm;
  const int wgs_per_cu = argc > 1 ? std::atoi(argv[1]) : 1;   // CORRLA_KNN2_WGS_PER_CU
  while (std::scanf("%lld %lld %lld %d %lld %d %d %lld", &np, &kf, &nq, &order, &n, &km, &fm, &budget) == 8) {
    const corrla::GradPlan p = corrla::grad_plan(np, kf, nq, order, n, km, fm, 256, (size_t)budget, wgs_per_cu);
    if (p.error) {
      std::printf("reject %s\n", p.error);
      continue;
    }
    std::printf("%s %d %d %d %zu %s %d %zu %lld %zu %lld %zu", scans[(int)p.scan], p.scan_w, p.scan_nks, p.scan_s, p.scan_lds,
                fits[(int)p.fit], p.fit_ntt, p.fit_lds, (long long)p.scan_wgs, p.scan_ws, (long long)p.fit_wgs, p.fit_ws);
    std::printf(" %d %lld %lld %lld %lld %d %lld %zu %zu %zu %zu %zu\n", p.scan_block, (long long)p.scan_tiles, (long long)p.ldt,
                (long long)p.pts_wgs, (long long)p.k2.nchunks, p.k2.nb, (long long)p.k2.rpb, p.k2.pb, p.k2.pn, p.k2.cand,
                p.k2.list_d, p.k2.list_i);
  }
  return 0;
}
"""


GEOMETRY = ("block", "tiles", "ldt", "pts_wgs", "nchunks", "nb", "rpb", "pb", "pn", "cand", "list_d", "list_i")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("grad_plan")
    src = tmp / "plan.cpp"
    src.write_text(MAIN)
    exe = tmp / "plan"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "corrla_rs_amd", "csrc"),
                           str(src), "-o", str(exe)])

    def run(cases, budget=BUDGET, wgs_per_cu=None):
        inp = "".join("%d %d %d %d %d %d %d %d\n" % (*c, budget) for c in cases)
        argv = [str(exe)] + ([] if wgs_per_cu is None else [str(wgs_per_cu)])
        out = subprocess.run(argv, input=inp, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        res = []
        for line in out:
            if line.startswith("reject "):
                res.append(("reject", line[7:]))
            else:
                f = line.split()
                res.append(((f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4])), (f[5], int(f[6]), int(f[7])),
                            (int(f[8]), int(f[9]), int(f[10]), int(f[11])), dict(zip(GEOMETRY, map(int, f[12:])))))
        return res
    return run


def _accepted_grid():
    cases = []
    for k, order, knn_mode, fit_mode in itertools.product([1, 5, 17, 32, 33, 64], [1, 2], [0, 1, 2, 3], [0, 1]):
        need = k + 1 if order == 1 else k * (k + 3) // 2
        for n in sorted({need + 1, need + 7, 80, 128, 129, 200, 300, 400, 480, 512}):
            if n <= need or n > 512:
                continue
            for n_pts in (max(n, need + 1, 600), 8191, 8192, 131071, 131072, 400000):
                if n_pts < n:
                    continue
                cases.append((n_pts, k, 37, order, n, knn_mode, fit_mode))
    return [c for c in cases if old_routing(*c) is not None]


def test_accepted_calls_keep_their_kernels(plan):
    cases = _accepted_grid()
    assert len(cases) > 1500
    got = plan(cases)
    bad = []
    for c, g in zip(cases, got):
        exp = old_routing(*c)
        if g[0] == "reject" or (g[0], g[1]) != exp:
            bad.append((c, g, exp))
    assert not bad, bad[:5]
    kinds = {(g[0][0], g[1][0]) for g in got}
    assert {s for s, _ in kinds} == {"valu", "mfma", "knn2"} and {f for _, f in kinds} == {"lin", "lds", "global"}


# a few of the above as literal rows: (n_pts, k, n_q, order, n_nbrs, CORRLA_KNN, CORRLA_FIT) -> scan, fit
LITERAL = [
    ((1000000, 64, 1000000, 1, 80, 0, 0), ("knn2", 0, 0, 2, 76800), ("lin", 5, 19696)),        # BASELINE config 5
    ((5000, 64, 256, 1, 80, 0, 0), ("valu", 0, 0, 0, 56384), ("lin", 5, 19696)),
    ((200000, 64, 100, 1, 130, 0, 0), ("mfma", 2, 16, 0, 128964), ("lin", 5, 19952)),
    ((200000, 16, 100, 1, 150, 0, 0), ("mfma", 4, 4, 0, 140612), ("lin", 2, 2944)),
    ((200000, 32, 100, 1, 140, 2, 0), ("mfma", 4, 8, 0, 156484), ("lin", 3, 6384)),
    ((200000, 64, 100, 1, 300, 0, 0), ("valu", 0, 0, 0, 98624), ("lin", 5, 20592)),    # MFMA lists outgrow LDS
    ((3000, 64, 100, 1, 100, 2, 1), ("mfma", 2, 16, 0, 117444), ("lds", 0, 89392)),
    ((4000, 14, 50, 2, 120, 0, 0), ("valu", 0, 0, 0, 32064), ("lds", 0, 134112)),
    ((4000, 20, 50, 2, 300, 1, 0), ("valu", 0, 0, 0, 70464), ("global", 0, 57384)),
    ((9000, 5, 50, 1, 12, 0, 1), ("knn2", 0, 0, 1, 44032), ("lds", 0, 1224)),
]


def test_literal_rows(plan):
    got = plan([r[0] for r in LITERAL])
    for (c, scan, fit), g in zip(LITERAL, got):
        assert (g[0], g[1]) == (scan, fit), (c, g)


def test_beyond_the_limits_goes_wide(plan):
    cases, expect = [], []
    for k in list(range(65, 130)) + [255, 256, 300, 1024, 2048, 4096]:   # k > 64: both stages wide
        cases.append((max(6000, k + 10), k, 10, 1, k + 5, 0, 0))
        expect.append(("wide", "wide"))
    for n in (513, 600, 1024, 2048, 5000):                                # n_nbrs > 512: both wide
        for k in (1, 5, 64):
            cases.append((20000, k, 10, 1, n, 0, 0))
            expect.append(("wide", "wide"))
    for k in range(31, 65):                                               # order 2 beyond k = 30
        need = k * (k + 3) // 2
        cases.append((need + 100, k, 3, 2, need + 1, 0, 0))
        expect.append(("wide", "wide"))
    # within the scans' limits, beyond the limited fits': the scan is unchanged, only the fit is wide
    # (the MFMA and bf16 scans' lists outgrow LDS before the neighbours outgrow the limited fits: only the VALU scan meets it)
    cases += [(5000, 64, 10, 1, 400, 0, 0), (200000, 64, 10, 1, 400, 0, 0), (20000, 50, 10, 1, 512, 0, 0)]
    expect += [("valu", "wide"), ("valu", "wide"), ("valu", "wide")]
    # the switches force the wide kernels on any call
    cases += [(20000, 64, 10, 1, 80, 4, 0), (20000, 64, 10, 1, 80, 0, 2), (300, 5, 10, 2, 30, 4, 2)]
    expect += [("wide", "lin"), ("knn2", "wide"), ("wide", "wide")]
    got = plan(cases)
    for c, g, e in zip(cases, got, expect):
        assert g[0] != "reject", (c, g)
        assert (g[0][0], g[1][0]) == e, (c, g)
        if e[0] == "wide":
            wgs, ws = g[2][0], g[2][1]
            assert 1 <= wgs <= min(2 * NUM_CUS, (c[2] + 63) // 64) and ws == wgs * 64 * (c[4] * 8 + 512 * 12)
            assert g[0][4] <= KMAX // 2   # two scanning workgroups per CU
        if e[1] == "wide":
            P = c[1] + 1 if c[3] == 1 else c[1] + c[1] * (c[1] + 1) // 2 + 1
            assert g[2][2] == min(c[2], NUM_CUS) and g[2][3] == g[2][2] * ((P + 1) ** 2 + 2 * (P + 1)) * 8
            assert g[1][2] <= KMAX


def test_argument_rejections_remain(plan):
    cases = [
        (1000, 5, 10, 3, 20, 0, 0),        # order not in {1, 2}
        (1000, 5, 10, 0, 20, 0, 0),
        (1000, 5, 10, 1, 6, 0, 0),         # n_nbrs not above k + 1
        (6, 5, 10, 1, 6, 0, 0),            # n_pts not above k + 1
        (1000, 5, 10, 2, 20, 0, 0),        # order 2: n_nbrs not above k (k + 3) / 2 = 20
        (1000, 100, 10, 2, 5150, 0, 0),    # ... n_nbrs above, n_pts not
        (1000, 5, 10, 1, 1001, 0, 0),      # n_nbrs > n_pts
        (1 << 31, 5, 10, 1, 20, 0, 0),     # n_pts > 2^31 - 1
        (100000, 5, (1 << 40) // 50 + 1, 1, 50, 0, 0),   # n_q n_nbrs > 2^40
        (1000, 5, 0, 1, 20, 0, 0),         # empty
        (1000, 0, 10, 1, 20, 0, 0),
    ]
    got = plan(cases)
    for c, g in zip(cases, got):
        assert g[0] == "reject", (c, g)
    assert "est_order" in got[0][1] and "exceed k + 1" in got[2][1] and "n_nbrs exceeds" in got[6][1]
    assert got[7][1] == "point set too large" and got[8][1] == "point set too large"


def test_memory_rejection_starts_at_the_budget(plan):
    # order 1: P = k + 1, slice (P + 1)^2 + 2 (P + 1) doubles <= 4 GiB  <=>  P + 1 <= 23169 (23170^2 + 2 * 23170 > 2^29)
    def slice_bytes(P):
        return ((P + 1) ** 2 + 2 * (P + 1)) * 8
    kmax = max(k for k in range(23000, 23200) if slice_bytes(k + 1) <= BUDGET)
    got = plan([(kmax + 3, kmax, 1, 1, kmax + 2, 0, 0), (kmax + 4, kmax + 1, 1, 1, kmax + 3, 0, 0)])
    assert got[0][0] != "reject" and got[0][1][0] == "wide"
    assert got[1][0] == "reject" and "4 GiB" in got[1][1]
    # order 2: P = k + k (k + 1) / 2 + 1 -- k = 213 fits, 214 does not
    p2 = lambda k: k + k * (k + 1) // 2 + 1
    k2 = max(k for k in range(150, 260) if slice_bytes(p2(k)) <= BUDGET)
    assert k2 == 213
    n2 = k2 * (k2 + 3) // 2 + 1
    got = plan([(n2 + 10, k2, 1, 2, n2, 0, 0), (n2 + 300, k2 + 1, 1, 2, n2 + 220, 0, 0)])
    assert got[0][0] != "reject" and got[1][0] == "reject"
    # a smaller budget: fewer workgroups first, then the rejection
    P = 1025
    got = plan([(3000, 1024, 1000, 1, 1100, 0, 0)], budget=3 * slice_bytes(P))
    assert got[0][2][2] == 3
    got = plan([(3000, 1024, 1000, 1, 1100, 0, 0)], budget=slice_bytes(P) - 1)
    assert got[0][0] == "reject"


# ---- every launch: grids, workgroup sizes, the bf16 scan's geometry, workspaces ----------------------------------------
def old_launches(c, scan, fit, wgs_per_cu=1):
    """What the entry of corrla_grad_mat_* (today grad_stage::run_entry) computed beside the plan when it launched (scan, fit) for the call c, written from that function as
    it was: (scan grid, scan workspace, fit grid, fit workspace) and the GEOMETRY fields."""
    n_pts, k, n_q, order, n = c[:5]
    P = k + 1 if order == 1 else k + k * (k + 1) // 2 + 1
    geo = dict.fromkeys(GEOMETRY, 0)
    if scan == "wide":                                    # three arrays per workgroup: list_d, cand_d, cand_i
        geo.update(block=64 * 4, tiles=(n_q + 63) // 64)
        scan_wgs = min(geo["tiles"], 2 * NUM_CUS)
        scan_ws = scan_wgs * 64 * n * 8 + scan_wgs * 64 * 512 * 8 + scan_wgs * 64 * 512 * 4
    else:                                                 # xt, by grad_transpose_kernel on (n_pts + 255) / 256 blocks
        geo.update(ldt=(n_pts + 63) // 64 * 64, pts_wgs=(n_pts + 255) // 256)
        scan_ws = geo["ldt"] * k * 8
    if scan == "valu":
        geo.update(block=64 * 4)
        scan_wgs = (n_q + 16 - 1) // 16
    elif scan == "mfma":
        waves = 4 if knn_mfma_lds(k, n, 4) <= KMAX else 2
        geo.update(block=64 * waves)
        scan_wgs = (n_q + 16 * waves - 1) // (16 * waves)
        scan_ws += n_pts * 8                              # pnorm
    elif scan == "knn2":
        s = 1 if k <= 32 else 2
        nchunks = (n_pts + 63) // 64
        nb = max(1, min(1024, (n_pts + 4095) // 4096))
        geo.update(block=64 * 12, tiles=(n_q + 384 - 1) // 384, nchunks=nchunks, nb=nb, rpb=(n_pts + nb - 1) // nb)
        scan_wgs = min(geo["tiles"], NUM_CUS * max(1, wgs_per_cu))
        geo.update(pb=nchunks * s * 8192, pn=nchunks * 64 * 4 * 4, cand=scan_wgs * 384 * 256 * 4,
                   list_d=scan_wgs * 384 * 128 * 8, list_i=scan_wgs * 384 * 128 * 4)
        scan_ws += geo["pb"] + geo["pn"] + 64 * 8 + nb * 64 * 8 + geo["cand"] + geo["list_d"] + geo["list_i"]   # + mean, partial
    if fit in ("lin", "lds"):
        fit_wgs, fit_ws = n_q, 0
    elif fit == "global":
        fit_wgs = min(n_q, 2 * NUM_CUS)
        fit_ws = fit_wgs * P * ((P + 1) | 1) * 8
    else:
        fit_wgs = min(n_q, NUM_CUS)
        fit_ws = fit_wgs * ((P + 1) ** 2 + 2 * (P + 1)) * 8
    return (scan_wgs, scan_ws, fit_wgs, fit_ws), geo


# beyond the limits and forced (scan and fit wide, each alone, many query tiles), and the accepted grid's kernels with enough
# queries that the persistent grids bind (1e6 / 384 = 2605 and 150000 / 384 = 391 bf16-scan tiles against 256 and 512)
WIDE_ROWS = [(6000, 96, 10, 1, 101, 0, 0), (20000, 64, 1000, 1, 600, 0, 0), (300, 5, 10, 2, 30, 4, 2),
             (20000, 64, 100000, 1, 80, 4, 0), (20000, 64, 10, 1, 80, 0, 2), (3000, 1024, 1000, 1, 1100, 0, 0)]
MANY_QUERIES = [(1000000, 64, 1000000, 1, 80, 0, 0), (150000, 20, 150000, 1, 30, 0, 1), (9000, 5, 385, 1, 12, 3, 0),
                (200000, 16, 1001, 1, 150, 0, 0), (200000, 64, 1001, 1, 130, 2, 0), (5000, 64, 1001, 1, 80, 1, 0),
                (4000, 20, 1000, 2, 300, 1, 0), (4000, 20, 511, 2, 300, 1, 0), (400000, 33, 100000, 2, 600, 3, 0)]


@pytest.mark.parametrize("wgs_per_cu", [None, 0, 1, 2])
def test_every_launch_is_sized_by_the_plan(plan, wgs_per_cu):
    cases = _accepted_grid() + WIDE_ROWS + MANY_QUERIES
    got = plan(cases, wgs_per_cu=wgs_per_cu)
    bad = []
    for c, g in zip(cases, got):
        assert g[0] != "reject", (c, g)
        exp = old_launches(c, g[0][0], g[1][0], 1 if wgs_per_cu is None else wgs_per_cu)
        if (g[2], g[3]) != exp:
            bad.append((c, g, exp))
    assert not bad, bad[:3]
    kinds = {g[0][0] for g in got} | {g[1][0] for g in got}
    assert kinds == {"valu", "mfma", "knn2", "wide", "lin", "lds", "global"}
    # the knob binds: 2605 tiles on 256 or 512 workgroups, 391 tiles on 256 or all
    big = {c: g[2][0] for c, g in zip(cases, got) if c in MANY_QUERIES[:2]}
    assert list(big.values()) == ([512, 391] if wgs_per_cu == 2 else [256, 256])


# The smallest call that reaches each instantiation the dispatch can select: (features k, neighbours, order, CORRLA_KNN,
# CORRLA_FIT) on a 3000-point cloud with 64 queries -> (scan, waves, slices, steps, fit, tiles).  tests/test_gpu_grad_routes.py
# runs every row on the device.
ROUTES = [
    ((6, 12, 1, 0, 0), ("valu", 0, 0, 0, "lin", 1)),
    ((20, 30, 1, 0, 0), ("valu", 0, 0, 0, "lin", 2)),
    ((40, 60, 1, 0, 0), ("valu", 0, 0, 0, "lin", 3)),
    ((50, 60, 1, 0, 0), ("valu", 0, 0, 0, "lin", 4)),
    ((64, 80, 1, 0, 0), ("valu", 0, 0, 0, "lin", 5)),
    ((16, 150, 1, 2, 0), ("mfma", 4, 4, 0, "lin", 2)),
    ((32, 140, 1, 2, 0), ("mfma", 4, 8, 0, "lin", 3)),
    ((40, 60, 1, 2, 0), ("mfma", 4, 16, 0, "lin", 3)),
    ((16, 200, 1, 2, 0), ("mfma", 2, 4, 0, "lin", 2)),
    ((32, 200, 1, 2, 0), ("mfma", 2, 8, 0, "lin", 3)),
    ((64, 130, 1, 2, 0), ("mfma", 2, 16, 0, "lin", 5)),
    ((5, 12, 1, 3, 0), ("knn2", 0, 0, 1, "lin", 1)),
    ((40, 50, 1, 3, 0), ("knn2", 0, 0, 2, "lin", 3)),
    ((3, 14, 2, 0, 0), ("valu", 0, 0, 0, "lds", 0)),
    ((5, 12, 1, 0, 1), ("valu", 0, 0, 0, "lds", 0)),
    ((20, 300, 2, 1, 0), ("valu", 0, 0, 0, "global", 0)),
    ((5, 30, 2, 4, 2), ("wide", 0, 0, 0, "wide", 0)),
]


def route_points(k, order):
    return max(3000, k * (k + 3) // 2 + 100 if order == 2 else 0)


def test_route_table_reaches_what_it_names(plan):
    got = plan([(route_points(k, order), k, 64, order, n, km, fm) for (k, n, order, km, fm), _ in ROUTES])
    for (c, exp), g in zip(ROUTES, got):
        assert g[0] != "reject" and (g[0][0], g[0][1], g[0][2], g[0][3], g[1][0], g[1][1]) == exp, (c, g)
    reached = {e[:4] for _, e in ROUTES} | {e[4:] for _, e in ROUTES}
    assert reached >= {("mfma", w, s, 0) for w in (4, 2) for s in (4, 8, 16)} | {("knn2", 0, 0, 1), ("knn2", 0, 0, 2)}
    assert reached >= {("lin", t) for t in range(1, 6)} | {("lds", 0), ("global", 0), ("wide", 0), ("valu", 0, 0, 0), ("wide", 0, 0, 0)}
