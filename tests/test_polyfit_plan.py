"""The plan of the polynomial response-surface kernels behind corrla_polyfit_gram_* and corrla_poly_eval_*
(corrla_rs_amd/csrc/polyfit_plan.hpp), pinned on the CPU: the header is host code, compiled here with the host compiler in a
temporary directory.

Pinned here: the pair table names the columns of W = [V, y] in the reference's order (against the golden
``test_col_interact`` values and tests/polyfit_reference.py), the tiles cover every column and the slabs every sample exactly
once with no empty slab, the dynamic LDS stays within 160 KiB and the workspace within the plan's stated bound, the route
follows the alignment of x, and every rejection carries the name of its argument.  The shape tables of
tests/test_gpu_polyfit.py live here and are imported there, as tests/test_gpu_rbf.py imports its tables from test_rbf_plan.py."""
import os
import subprocess

import numpy as np
import pytest

from tests import polyfit_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# in a folder of its own: the suite's older tests take every .npz directly under tests/golden for an RSVD case
KNOWN = os.path.join(ROOT, "tests", "golden", "polyfit", "polyfit_known.npz")
CSRC = os.path.join(ROOT, "corrla_rs_amd", "csrc")
BT, KT, THREADS, MAX_K, MAX_R = 128, 32, 256, 128, 64
EVAL_BM, EVAL_CB = 64, 32
LDS_MAX = 160 * 1024
INPLACE, CHECKED = 1, 2

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "polyfit_plan.hpp"
using namespace corrla;
int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "table")) {  // table k r degree
    const std::vector<int32_t> t = poly_pair_table(atoll(argv[2]), atoll(argv[3]), atoi(argv[4]));
    for (int32_t e : t) printf("%d %d\n", e & 0xffff, e >> 16);
    return 0;
  }
  if (argc == 9 && !strcmp(argv[1], "eval")) {  // eval m k r degree ldx esz aligned
    const PolyEvalPlan p = poly_eval_plan(atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), atoi(argv[5]), atoll(argv[6]), atoi(argv[7]),
                                          atoi(argv[8]) != 0);
    printf("ok %d\n", (int)p.ok);
    if (!p.ok) { printf("error %s\n", p.error); return 0; }
    printf("route %d\np %lld\nk1 %d\nk4 %d\nxld %d\nncb %d\nntiles %lld\ngrid %u\nblock %u\nlds %zu\nc_bytes %zu\nc_block %d\nassemble %u\n",
           (int)p.route, (long long)p.p, p.k1, p.k4, p.xld, p.ncb, (long long)p.ntiles, p.grid_x, p.block, p.lds_bytes, p.c_bytes,
           k::poly_eval_c_block_bytes(atoi(argv[3])), p.assemble_grid_x);
    return 0;
  }
  if (argc != 13 || strcmp(argv[1], "gram")) return 2;  // gram m k r degree ldx ldy esz x_aligned y_aligned num_cus slab_rows
  PolyGramShape s;
  s.m = atoll(argv[2]); s.kf = atoll(argv[3]); s.r = atoll(argv[4]); s.degree = atoi(argv[5]); s.ldx = atoll(argv[6]);
  s.ldy = atoll(argv[7]); s.esz = atoi(argv[8]); s.x_aligned = atoi(argv[9]) != 0; s.y_aligned = atoi(argv[10]) != 0;
  s.num_cus = atoi(argv[11]);
  PolyKnobs kn;
  kn.slab_rows = atoll(argv[12]);
  const PolyGramPlan p = poly_gram_plan(s, kn);
  printf("route %d\n", (int)p.route);
  if (p.route == PolyRoute::kReject) { printf("error %s\n", p.error); return 0; }
  printf("bt %d\nkt %d\np %lld\norder %lld\ny_vec %d\naug %d\naug_ld %d\nnb %d\nnpairs %lld\nchunks %lld\nnsplit %lld\nslab_rows %lld\n",
         p.bt, p.kt, (long long)p.p, (long long)p.order, (int)p.y_vec, p.aug, p.aug_ld, p.nb, (long long)p.npairs, (long long)p.chunks,
         (long long)p.nsplit, (long long)p.slab_rows);
  printf("grid_x %u\ngrid_y %u\nblock %u\nlds %zu\ntable_bytes %zu\nws %zu\nws_bound %zu\nfinish_x %u\nfinish_y %u\nfinish_block %u\n",
         p.grid_x, p.grid_y, p.block, p.lds_bytes, p.table_bytes, p.ws_bytes, p.ws_bound, p.finish_grid_x, p.finish_grid_y, p.finish_block);
  for (long long q = 0; q < p.npairs && q < 6; ++q) { int bi, bj; k::syrk_pair(q, &bi, &bj); printf("pair%lld %d %d\n", q, bi, bj); }
  return 0;
}
"""


def build_driver(tmp, csrc=CSRC):
    src = os.path.join(tmp, "polyfit_plan_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "polyfit_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + csrc, src, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("polyfit_plan")))


def _parse(out):
    d = {}
    for line in out.splitlines():
        key, _, rest = line.partition(" ")
        d[key] = rest
    return d


def gram_plan(exe, m, k, r=1, degree=2, ldx=None, ldy=None, esz=8, x_aligned=True, y_aligned=True, num_cus=256, slab_rows=0):
    ldx = k if ldx is None else ldx
    ldy = max(r, 1) if ldy is None else ldy
    d = _parse(subprocess.check_output([exe, "gram"] + [str(int(v)) for v in (m, k, r, degree, ldx, ldy, esz, x_aligned, y_aligned, num_cus,
                                                                               slab_rows)], text=True))
    if int(d["route"]) == 0:
        return {"route": 0, "error": d["error"]}
    p = {key: int(v) for key, v in d.items() if not key.startswith("pair")}
    p["pairs"] = [tuple(int(v) for v in d[key].split()) for key in sorted(d) if key.startswith("pair")]
    return p


def eval_plan(exe, m, k, r=1, degree=2, ldx=None, esz=8, aligned=True):
    d = _parse(subprocess.check_output([exe, "eval"] + [str(int(v)) for v in (m, k, r, degree, k if ldx is None else ldx, esz, aligned)],
                                       text=True))
    if not int(d["ok"]):
        return {"ok": 0, "error": d["error"]}
    return {key: int(v) for key, v in d.items()}


def pair_table(exe, k, r, degree):
    out = subprocess.check_output([exe, "table", str(k), str(r), str(degree)], text=True)
    return [tuple(int(v) for v in line.split()) for line in out.splitlines()]


def poly_terms(k, degree):
    return k + 1 if degree < 2 else k + k * (k + 1) // 2 + 1


# ---- the shapes of tests/test_gpu_polyfit.py, which imports them from here: one table for both files -----------------------
# m: 1, 3, 5 (less than one MFMA step, odd), one staged chunk - 1 / exact / + 1, and 300 with the slab knob forcing 5 slabs
M_VALUES = (1, 3, 5, KT - 1, KT, KT + 1)
SLAB_M, SLAB_KNOB, SLAB_COUNT = 300, 64, 5          # 5 slabs of 64 samples, the last of 44
# (k, r, degree): p + r = 2 one ragged tile; (14, 8) fills one tile exactly (p + r = 128), (14, 9) has one column in a second,
# (15, 1) two tiles with a ragged last one, (22, 3) three tiles, (128, 1) the widest row at degree 1, (40, 2) a C of more than
# one LDS block
KR_VALUES = ((1, 0, 2), (1, 1, 2), (3, 1, 2), (14, 8, 2), (14, 9, 2), (15, 1, 2), (22, 3, 2), (128, 1, 1), (40, 2, 2))
BASE_KR = (3, 1, 2)
BASE_M = KT + 1


def gpu_gram_shapes():
    """(m, k, r, degree): every m at the base (k, r), every (k, r) at m = 70 (three chunks, the last ragged)"""
    out = [(m,) + BASE_KR for m in M_VALUES]
    out += [(2 * KT + 6,) + kr for kr in KR_VALUES if kr != BASE_KR]
    return out


def gpu_eval_shapes():
    """(m, k, r, degree) with r >= 1: row tiles of 64 -- one row, a ragged tile, one tile +- 1, two tiles and a ragged third"""
    out = [(m,) + BASE_KR for m in (1, 5, EVAL_BM - 1, EVAL_BM, EVAL_BM + 1)]
    out += [(2 * EVAL_BM + 3,) + kr for kr in KR_VALUES if kr[1] >= 1 and kr != BASE_KR]
    return out


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("r", [0, 3])
def test_pair_table_is_the_reference_column_order(driver, k, degree, r):
    t = pair_table(driver, k, r, degree)
    p = poly_terms(k, degree)
    one, zero = k, k + 1 + r
    assert len(t) % BT == 0 and len(t) - BT < p + r <= len(t)
    assert all(e == (zero, zero) for e in t[p + r:])
    # the augmented row of a sample and the columns the table builds from it against the restated reference
    rng = np.random.default_rng(k * 10 + degree)
    x, y = rng.standard_normal((6, k)), rng.standard_normal((6, r))
    aug = np.hstack([x, np.ones((6, 1)), y, np.zeros((6, 1))])
    w = np.stack([aug[:, a] * aug[:, b] for a, b in t[:p + r]], axis=1)
    assert np.array_equal(w, np.hstack([R.build_full_vandermonde(x, degree), y]))
    assert t[:k] == [(a, one) for a in range(k)] and t[p - 1] == (one, one)
    assert t[p:p + r] == [(k + 1 + j, one) for j in range(r)]


def test_pair_table_against_the_golden_interactions(driver):
    """``test_col_interact`` (stats_corr.rs:374-391): x = [1, 2, 3, 4] -> x1 x1, x1 x2, ..., x4 x4"""
    g = np.load(KNOWN)
    x, want = g["interact_x"], g["interact_expected"]
    k = x.shape[1]
    t = pair_table(driver, k, 0, 2)
    aug = np.hstack([x, np.ones((x.shape[0], 1)), np.zeros((x.shape[0], 1))])
    inter = np.stack([aug[:, a] * aug[:, b] for a, b in t[k:k + k * (k + 1) // 2]], axis=1)
    assert np.max(np.abs(inter - want)) <= float(g["interact_tol"])
    assert np.max(np.abs(R.mat_col_interactions(x, True) - want)) <= float(g["interact_tol"])


def _check_gram_cover(p, m, k, r, degree):
    order = poly_terms(k, degree) + r
    assert (p["bt"], p["kt"], p["block"]) == (BT, KT, THREADS)
    assert p["p"] == poly_terms(k, degree) and p["order"] == order
    # tiles: every column exactly once
    assert (p["nb"] - 1) * BT < order <= p["nb"] * BT and p["table_bytes"] == p["nb"] * BT * 4
    assert p["npairs"] == p["nb"] * (p["nb"] + 1) // 2 and p["grid_x"] == p["npairs"] and p["finish_x"] == p["npairs"]
    assert p["finish_y"] == 16 and p["finish_block"] == 256
    # slabs: every sample exactly once, whole chunks, none empty
    assert p["chunks"] == -(-m // KT) and p["slab_rows"] % KT == 0 and p["slab_rows"] >= KT
    assert p["grid_y"] == p["nsplit"] and 1 <= p["nsplit"] <= 65535
    assert (p["nsplit"] - 1) * p["slab_rows"] < m <= p["nsplit"] * p["slab_rows"]
    # LDS and workspace
    assert p["aug"] == k + r + 2 and p["aug_ld"] >= p["aug"] and p["aug_ld"] % 2 == 1
    assert p["lds"] == (KT * p["aug_ld"] + 2 * k) * 8 <= LDS_MAX
    assert p["ws"] == p["nsplit"] * p["npairs"] * BT * BT * 8 <= p["ws_bound"]


def test_gram_plans_cover_columns_and_samples_once(driver):
    shapes = gpu_gram_shapes() + [(10 ** 6, 16, 1, 2), (10 ** 6, 64, 1, 2), (10 ** 5, 128, 1, 2), (10 ** 6, 128, 64, 2), (1, 128, 64, 2),
                                  (KT * 65535 * 3 + 1, 1, 0, 1)]
    for m, k, r, degree in shapes:
        p = gram_plan(driver, m, k, r, degree)
        assert p["route"] == INPLACE or (k % 2 == 1 and p["route"] == CHECKED), (m, k, r, degree, p)
        _check_gram_cover(p, m, k, r, degree)
        assert p["ws_bound"] == (p["npairs"] + 4 * 256) * BT * BT * 8
    # pairs: the upper triangle, column by column
    p = gram_plan(driver, 100, 22, 3)
    assert p["nb"] == 3 and p["pairs"] == [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2)]
    # the tiles of the GPU cases that are named for them
    assert gram_plan(driver, 70, 14, 8)["order"] == 128 and gram_plan(driver, 70, 14, 8)["nb"] == 1
    assert gram_plan(driver, 70, 14, 9)["order"] == 129 and gram_plan(driver, 70, 14, 9)["nb"] == 2
    assert gram_plan(driver, 70, 15, 1)["nb"] == 2 and gram_plan(driver, 70, 22, 3)["nb"] == 3
    # few pairs and many samples: the slabs carry the parallelism; many pairs: one slab
    assert gram_plan(driver, 10 ** 6, 16)["nsplit"] > 100 and gram_plan(driver, 10 ** 5, 128)["nsplit"] == 1
    # the widest shape
    p = gram_plan(driver, 10 ** 5, MAX_K, MAX_R)
    assert p["lds"] == (KT * 195 + 256) * 8 and p["order"] == 8385 + 64


def test_slab_knob(driver):
    p = gram_plan(driver, SLAB_M, 3, 1, slab_rows=SLAB_KNOB)
    assert p["nsplit"] == SLAB_COUNT and p["slab_rows"] == SLAB_KNOB and p["ws_bound"] == p["ws"]
    _check_gram_cover(p, SLAB_M, 3, 1, 2)
    q = gram_plan(driver, SLAB_M, 3, 1, slab_rows=50)          # rounded up to whole chunks: the same plan, the same bits
    assert (q["nsplit"], q["slab_rows"]) == (p["nsplit"], p["slab_rows"])
    one = gram_plan(driver, SLAB_M, 3, 1, slab_rows=10 ** 9)
    assert one["nsplit"] == 1 and one["slab_rows"] == -(-SLAB_M // KT) * KT


def test_routes(driver):
    assert gram_plan(driver, 50, 4)["route"] == INPLACE
    assert gram_plan(driver, 50, 4, x_aligned=False)["route"] == CHECKED
    assert gram_plan(driver, 50, 4, ldx=5)["route"] == CHECKED                 # f64: rows start off a 16-byte boundary
    assert gram_plan(driver, 50, 4, ldx=6)["route"] == INPLACE
    assert gram_plan(driver, 50, 4, ldx=6, esz=4)["route"] == CHECKED and gram_plan(driver, 50, 4, ldx=8, esz=4)["route"] == INPLACE
    assert gram_plan(driver, 50, 3)["route"] == CHECKED
    # y is the narrow operand: it is read by its own alignment and does not move the route
    p = gram_plan(driver, 50, 4, r=1)
    assert p["route"] == INPLACE and p["y_vec"] == 0
    assert gram_plan(driver, 50, 4, r=2)["y_vec"] == 1 and gram_plan(driver, 50, 4, r=2, y_aligned=False)["y_vec"] == 0
    assert eval_plan(driver, 50, 4)["route"] == INPLACE and eval_plan(driver, 50, 4, aligned=False)["route"] == CHECKED
    assert eval_plan(driver, 50, 3)["route"] == CHECKED


def test_eval_plans(driver):
    for m, k, r, degree in gpu_eval_shapes() + [(10 ** 6, 16, 1, 2), (10 ** 6, 64, 1, 2), (10 ** 5, 128, 64, 2)]:
        p = eval_plan(driver, m, k, r, degree)
        assert p["ok"] and p["p"] == poly_terms(k, degree) and p["k1"] == k + 1 and p["block"] == THREADS
        assert p["k4"] % 4 == 0 and k + 1 <= p["k4"] < k + 5 and p["xld"] % 8 == 4 and p["xld"] > p["k4"]
        assert (p["ncb"] - 1) * EVAL_CB < k + 1 <= p["ncb"] * EVAL_CB
        assert p["ntiles"] == -(-m // EVAL_BM) == p["grid"]
        assert p["lds"] == (EVAL_BM * p["xld"] + p["k4"] * (EVAL_CB + 8)) * 8 <= LDS_MAX
        assert p["c_bytes"] == r * p["k4"] * p["ncb"] * EVAL_CB * 8 and p["assemble"] * 256 >= p["c_bytes"] // 8
        # C is walked in blocks exactly when (k + 1)^2 doubles exceed the one block the plan allows beside the row tile
        assert (p["ncb"] > 1) == (k + 1 > EVAL_CB)
    assert eval_plan(driver, 100, 40)["ncb"] == 2 and eval_plan(driver, 100, 40)["c_block"] == 44 * (EVAL_CB + 8) * 8
    assert eval_plan(driver, 100, 128)["ncb"] == 5 and eval_plan(driver, 100, 22)["ncb"] == 1


def test_every_rejection_names_its_argument(driver):
    bad = ((dict(m=0), "m must be >= 1"), (dict(k=0), "k must be in [1, 128]"), (dict(k=129, ldx=129), "k must be in [1, 128]"),
           (dict(degree=0), "degree must be 1 or 2"), (dict(degree=3), "degree must be 1 or 2"), (dict(r=-1), "r must be in [0, 64]"),
           (dict(r=65, ldy=65), "r must be in [0, 64]"), (dict(ldx=3), "ldx < k"), (dict(r=2, ldy=1), "ldy < r"),
           (dict(esz=2), "element size (esz) must be 4 or 8"))
    for kw, word in bad:
        a = dict(m=10, k=4, r=1, degree=2)
        a.update(kw)
        p = gram_plan(driver, **a)
        assert p["route"] == 0 and p["error"].startswith("polyfit: ") and word in p["error"], (kw, p)
    bad = ((dict(m=0), "m must be >= 1"), (dict(k=0), "k must be in [1, 128]"), (dict(k=129, ldx=129), "k must be in [1, 128]"),
           (dict(degree=0), "degree must be 1 or 2"), (dict(r=0), "r must be in [1, 64]"), (dict(r=65), "r must be in [1, 64]"),
           (dict(ldx=3), "ldx < k"), (dict(esz=16), "element size (esz) must be 4 or 8"))
    for kw, word in bad:
        a = dict(m=10, k=4, r=1, degree=2)
        a.update(kw)
        p = eval_plan(driver, **a)
        assert not p["ok"] and p["error"].startswith("poly_eval: ") and word in p["error"], (kw, p)
