"""The plan of the PCA back-projection kernel behind corrla_pca_inverse_* and the Q-residuals of corrla_pca_transform_*
(corrla_rs_amd/csrc/pca_apply_plan.hpp), pinned on the CPU: the header is host code, compiled here with the host compiler in
a temporary directory.

For every row of SHAPES the driver prints the plan; pinned here: the workgroups' tiles cover [0, m) x [0, n) exactly once,
the k-chunks cover [0, k) exactly once, the dynamic LDS stays within 160 KiB, the workspace within the plan's stated bound,
and the route is the expected one for aligned, misaligned and feature-strided operands.  The table ends with the calls of
tests/test_gpu_pca_apply.py (GPU_CALLS), built from the shape tables below, which that file imports -- as tests/test_gpu_cov.py
imports its tables from test_syrk_plan.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corrla_rs_amd", "csrc")
REJECT, INPLACE, CHECKED, REPACKED = 0, 1, 2, 3
STORE, RESID = 0, 1
BM, BN = 64, 128


def KC(esz):
    return 128 // esz


DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "pca_apply_plan.hpp"
using namespace corrla;
int main(int argc, char** argv) {
  // m n k rs cs esz base_aligned mode
  if (argc != 9) return 2;
  PcaApplyShape s;
  s.m = atoll(argv[1]); s.n = atoll(argv[2]); s.k = atoll(argv[3]); s.row_stride = atoll(argv[4]); s.col_stride = atoll(argv[5]);
  s.esz = atoi(argv[6]); s.base_aligned = atoi(argv[7]) != 0; s.mode = atoi(argv[8]) ? PcaApplyMode::kResid : PcaApplyMode::kStore;
  const PcaApplyPlan p = pca_apply_plan(s);
  printf("route %d\n", (int)p.route);
  if (p.route == PcaApplyRoute::kReject) { printf("error %s\n", p.error); return 0; }
  printf("bm %d\nbn %d\nkc %d\nnbm %lld\nnbn %lld\nnchunks %lld\n", p.bm, p.bn, p.kc, (long long)p.nbm, (long long)p.nbn,
         (long long)p.nchunks);
  printf("grid %u\nblock %u\nlds %zu\nwide %d\nld %lld\nrepack %zu\nws %zu\nws_bound %zu\nfinish %u %u\n", p.grid_x, p.block,
         p.lds_bytes, p.wide, (long long)p.ld, p.repack_bytes, p.ws_bytes, p.ws_bound, p.finish_grid_x, p.finish_block);
  printf("consts %d %d %d %d\n", k::kPcaBackBM, k::kPcaBackBN, k::pca_back_kc(s.esz), k::pca_back_lds_bytes(s.esz));
  return 0;
}
"""


def build_driver(tmp, csrc=CSRC):
    src = os.path.join(tmp, "pca_apply_plan_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "pca_apply_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + csrc, src, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("pca_apply_plan")))


def plan(exe, m, n, k, rs, cs, esz, base_aligned=1, mode=STORE):
    out = subprocess.check_output([exe] + [str(v) for v in (m, n, k, rs, cs, esz, base_aligned, mode)], text=True)
    d = {}
    for line in out.splitlines():
        key, _, rest = line.partition(" ")
        d[key] = rest
    p = {"route": int(d["route"])}
    if p["route"] == REJECT:
        p["error"] = d["error"]
        return p
    for key in ("bm", "bn", "kc", "nbm", "nbn", "nchunks", "grid", "block", "lds", "wide", "ld", "repack", "ws", "ws_bound"):
        p[key] = int(d[key])
    p["finish"] = tuple(int(v) for v in d["finish"].split())
    p["consts"] = tuple(int(v) for v in d["consts"].split())
    return p


# ---- the shapes of tests/test_gpu_pca_apply.py, which imports them from here: one table for both files ----------------------
M_VALUES = (1, BM - 1, BM + 1, 2 * BM + 3)
N_VALUES = (1, BN - 1, BN + 1, 2 * BN + 5)


def k_values(esz):
    return (1, 3, 4, 5, KC(esz), KC(esz) + 1)


def shapes(esz):
    """The cross product of M_VALUES, N_VALUES and k_values thinned to the cases in which one of the three runs through all its
    values while the two others sit at a corner of their extremes; k is capped at n."""
    ks = k_values(esz)
    out = []

    def add(m, n, k):
        c = (m, n, min(k, n))
        if c not in out:
            out.append(c)
    ext_m, ext_n, ext_k = (M_VALUES[0], M_VALUES[-1]), (N_VALUES[0], N_VALUES[-1]), (ks[0], ks[-1])
    for m in M_VALUES:
        for n in ext_n:
            for k in ext_k:
                add(m, n, k)
    for n in N_VALUES:
        for m in ext_m:
            for k in ext_k:
                add(m, n, k)
    for k in ks:
        for m in ext_m:
            for n in ext_n:
                add(m, n, k)
    return out


LAYOUTS = ("contiguous", "row_stride_n_plus_1", "base_plus_1", "column_major")


def layout_shapes(esz):
    """two shapes that take every layout: between them n, n + 1 reach an aligned and a misaligned row stride for both types"""
    return ((2 * BM + 3, BN - 1, 5), (BM + 1, 2 * BN + 5, KC(esz) + 1))


def layout_call(m, n, k, esz, layout, mode):
    """(m, n, k, row stride, column stride, element size, base aligned, mode, route) of the m x n operand in `layout`"""
    vec = 16 // esz

    def rowmajor(ld, base=1):
        return INPLACE if base and ld % vec == 0 else CHECKED
    return {"contiguous": (m, n, k, n, 1, esz, 1, mode, rowmajor(n)),
            "row_stride_n_plus_1": (m, n, k, n + 1, 1, esz, 1, mode, rowmajor(n + 1)),
            "base_plus_1": (m, n, k, n, 1, esz, 0, mode, CHECKED),
            "column_major": (m, n, k, 1, m, esz, 1, mode, REPACKED)}[layout]


LOWRANK_SHAPE = (300, 200, 8)   # the low-rank-plus-noise case of the Q-residuals
CSR_SHAPE = (257, 131, 7)


def _gpu_calls():
    calls = []
    for esz in (4, 8):
        for (m, n, k) in shapes(esz):
            for mode in (STORE, RESID):
                calls.append(layout_call(m, n, k, esz, "contiguous", mode))
        for (m, n, k) in layout_shapes(esz):
            for layout in LAYOUTS:
                calls.append(layout_call(m, n, k, esz, layout, RESID))
                if layout != "column_major":     # the output of the inverse always has unit stride along the features
                    calls.append(layout_call(m, n, k, esz, layout, STORE))
        calls.append(layout_call(*LOWRANK_SHAPE, esz, "contiguous", RESID))
    return calls


GPU_CALLS = _gpu_calls()

SHAPES = [
    # (m, n, k, rs, cs, esz, base_aligned, mode, route): the shapes of tools/bench_pca_transform.py first
    (1000000, 512, 64, 512, 1, 4, 1, STORE, INPLACE),
    (1000000, 512, 64, 512, 1, 4, 1, RESID, INPLACE),
    (16384, 16384, 32, 16384, 1, 4, 1, STORE, INPLACE),
    (16384, 16384, 32, 16384, 1, 4, 1, RESID, INPLACE),
    (65536, 4096, 256, 4096, 1, 8, 1, STORE, INPLACE),
    (65536, 4096, 256, 4096, 1, 8, 1, RESID, INPLACE),
    (5000, 301, 9, 301, 1, 8, 1, RESID, CHECKED),
    (5000, 300, 9, 302, 1, 4, 1, STORE, CHECKED),
    (5000, 300, 9, 304, 1, 4, 0, STORE, CHECKED),
    (5000, 300, 300, 1, 5000, 4, 1, RESID, REPACKED),
    (5000, 300, 9, 600, 2, 8, 0, RESID, REPACKED),
    (1, 9, 2, 9, 1, 8, 1, STORE, CHECKED),
    (1, 8, 2, 0, 1, 8, 1, STORE, INPLACE),
    (3, 1, 1, 7, 5, 8, 1, RESID, CHECKED),
    (10000000, 16, 3, 16, 1, 4, 1, STORE, INPLACE),
] + GPU_CALLS


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "-".join(str(v) for v in c))
def test_plan_properties(driver, case):
    m, n, k, rs, cs, esz, base, mode, route = case
    p = plan(driver, m, n, k, rs, cs, esz, base, mode)
    assert p["route"] == route, p
    assert (p["bm"], p["bn"], p["kc"]) == (BM, BN, KC(esz)) == p["consts"][:3]
    # workgroup w owns tile (w // nbn, w % nbn): every tile once, each non-empty, together exactly [0, m) x [0, n)
    nbm, nbn = p["nbm"], p["nbn"]
    assert p["grid"] == nbm * nbn < 2 ** 31 and p["block"] == 256
    assert (nbm - 1) * BM < m <= nbm * BM and (nbn - 1) * BN < n <= nbn * BN
    if nbm * nbn <= 4096:
        tiles = [(w // nbn, w % nbn) for w in range(p["grid"])]
        assert sorted(tiles) == [(i, j) for i in range(nbm) for j in range(nbn)]
        area = sum((min(m, (i + 1) * BM) - i * BM) * (min(n, (j + 1) * BN) - j * BN) for i, j in tiles)
        assert area == m * n
    # the chunks cover [0, k) once; the last one may be short and is padded in LDS, never read past k
    assert (p["nchunks"] - 1) * p["kc"] < k <= p["nchunks"] * p["kc"]
    covered = 0
    for c in range(p["nchunks"]):
        lo, hi = c * p["kc"], min(k, (c + 1) * p["kc"])
        assert lo == covered and hi > lo
        covered = hi
    assert covered == k
    # LDS and workspace
    assert p["lds"] == p["kc"] * (BM + BN) * esz == p["consts"][3] <= 160 * 1024
    if mode == RESID:
        assert p["ws"] == nbn * m * esz <= p["ws_bound"] == m * (n // BN + 1) * esz
        assert p["finish"] == ((m + 255) // 256, 256)
    else:
        assert p["ws"] == 0 == p["ws_bound"]
    # the row stride the kernel uses, the width of its accesses, and the repacked copy
    vec = 16 // esz
    if route == REPACKED:
        assert p["ld"] == (n + 63) // 64 * 64 and p["repack"] == m * p["ld"] * esz and p["wide"] == 1
    else:
        assert p["repack"] == 0 and p["ld"] == (rs if m > 1 else max(rs, n))
        assert (route == INPLACE) == (bool(base) and p["ld"] % vec == 0) == bool(p["wide"])


def test_rejections_carry_their_reason(driver):
    for args, word in (((0, 5, 1, 5, 1, 4), "empty"), ((5, 0, 1, 5, 1, 4), "empty"), ((5, 5, 0, 5, 1, 4), "k must"),
                       ((5, 5, 1, 5, 1, 2), "element size"), ((5, 5, 1, -5, 1, 4), "negative"),
                       ((5, 5, 1, 1, 5, 4, 1, STORE), "unit stride"), ((5, 5, 1, 0, 0, 4, 1, RESID), "stride"),
                       ((2 ** 40, 2 ** 20, 1, 2 ** 20, 1, 4), "tiles")):
        p = plan(driver, *args)
        assert p["route"] == REJECT and word in p["error"], (args, p)


def test_the_thinned_cross_product_keeps_every_value_with_every_extreme():
    for esz in (4, 8):
        cases = shapes(esz)
        assert len(cases) <= 40 and len(set(cases)) == len(cases)
        ks = k_values(esz)
        for m in M_VALUES:
            for n in (N_VALUES[0], N_VALUES[-1]):
                for k in (ks[0], ks[-1]):
                    assert (m, n, min(k, n)) in cases
        for n in N_VALUES:
            for m in (M_VALUES[0], M_VALUES[-1]):
                for k in (ks[0], ks[-1]):
                    assert (m, n, min(k, n)) in cases
        for k in ks:
            for m in (M_VALUES[0], M_VALUES[-1]):
                for n in (N_VALUES[0], N_VALUES[-1]):
                    assert (m, n, min(k, n)) in cases


def test_the_gpu_files_calls_reach_every_route_in_both_modes(driver):
    for mode in (STORE, RESID):
        want = {INPLACE, CHECKED} | ({REPACKED} if mode == RESID else set())
        for esz in (4, 8):
            assert {c[-1] for c in GPU_CALLS if c[7] == mode and c[5] == esz} == want, (mode, esz)
    # more than one tile in both directions, a short last chunk and more than one chunk
    assert any(plan(driver, *c[:8])["nbm"] > 1 and plan(driver, *c[:8])["nbn"] > 1 and plan(driver, *c[:8])["nchunks"] > 1
               for c in GPU_CALLS[:60])
