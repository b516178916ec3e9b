"""The plans of the multivariate normal sampler and the sandwich variances (corrla_rs_amd/csrc/mvn_plan.hpp), pinned on the
CPU: the header is host code, compiled here with the host compiler in a temporary directory.

Pinned: the route, the row tile BM, the grid, the dynamic LDS (within 160 KiB, and equal to the z tile plus the staging image)
and the workspace bound for r = 1, 3, 4, 5, 16, 17, 128, the largest fused r and one above it, for both element sizes; 16-byte
stores only for an aligned base and row stride; the rejections; and the shape tables tests/test_gpu_mvn.py imports -- as
tests/test_gpu_pca_apply.py imports its tables from test_pca_apply_plan.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corrla_rs_amd", "csrc")
REJECT, FUSED, STAGED, EMPTY = 0, 1, 2, 3
LDS_MAX = 160 * 1024
WS_BUDGET = 256 << 20

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "mvn_plan.hpp"
using namespace corrla;
int main(int argc, char** argv) {
  if (argc == 6 && !strcmp(argv[1], "sandwich")) {  // m d ldj esz
    SandwichShape s;
    s.m = atoll(argv[2]); s.d = atoll(argv[3]); s.ldj = atoll(argv[4]); s.ldc = s.d; s.esz = atoi(argv[5]);
    const SandwichPlan p = sandwich_plan(s);
    printf("ok %d\n", p.ok ? 1 : 0);
    if (!p.ok) { printf("error %s\n", p.error); return 0; }
    printf("bm %d\nbn %d\nkc %d\ngrid %u\nblock %u\nncoltiles %lld\nlds %zu\n", p.bm, p.bn, p.kc, p.grid_x, p.block,
           (long long)p.ncoltiles, p.lds_bytes);
    return 0;
  }
  // n d r first ldo esz out_aligned lower
  if (argc != 9) return 2;
  MvnShape s;
  s.n = atoll(argv[1]); s.d = atoll(argv[2]); s.r = atoll(argv[3]); s.first = atoll(argv[4]); s.ldo = atoll(argv[5]);
  s.esz = atoi(argv[6]); s.out_aligned = atoi(argv[7]) != 0; s.lower = atoi(argv[8]) != 0;
  const MvnPlan p = mvn_plan(s);
  printf("route %d\n", (int)p.route);
  if (p.route == MvnRoute::kReject) { printf("error %s\n", p.error); return 0; }
  printf("bm %d\nbn %d\nkc %d\ngrid %u\nblock %u\nncoltiles %lld\nlds %zu\nwide %d\nldft %lld\nfactor %zu\n", p.bm, p.bn, p.kc,
         p.grid_x, p.block, (long long)p.ncoltiles, p.lds_bytes, p.wide, (long long)p.ldft, p.factor_bytes);
  printf("chunk_rows %lld\nnchunks %lld\nws %zu\nws_bound %zu\n", (long long)p.chunk_rows, (long long)p.nchunks, p.ws_bytes,
         p.ws_bound);
  printf("maxr %lld\n", (long long)k::mvn_max_fused_r(s.esz));
  return 0;
}
"""


def build_driver(tmp, csrc=CSRC):
    src = os.path.join(tmp, "mvn_plan_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "mvn_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + csrc, src, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("mvn_plan")))


def _parse(out):
    d = {}
    for line in out.splitlines():
        key, _, rest = line.partition(" ")
        d[key] = rest if key == "error" else int(rest)
    return d


def plan(exe, n, d, r, esz, first=0, ldo=None, out_aligned=1, lower=0):
    ldo = d if ldo is None else ldo
    return _parse(subprocess.check_output([exe] + [str(v) for v in (n, d, r, first, ldo, esz, out_aligned, lower)], text=True))


def sandwich(exe, m, d, esz, ldj=None):
    return _parse(subprocess.check_output([exe, "sandwich"] + [str(v) for v in (m, d, d if ldj is None else ldj, esz)], text=True))


# ---- the geometry restated, and the tables of tests/test_gpu_mvn.py, which imports them from here --------------------------
def KC(esz):
    return 128 // esz


def BN(bm):
    return 64 * (64 // bm)


def lds_bytes(r, bm, esz):
    return ((r + 3) // 4 * 4 * bm + KC(esz) * BN(bm)) * esz


def BM(r, esz):
    """the row tile of the fused kernels for a reduction length r: 64 while two workgroups fit 160 KiB, then 32, then none"""
    if lds_bytes(r, 64, esz) <= LDS_MAX // 2:
        return 64
    return 32 if lds_bytes(r, 32, esz) <= LDS_MAX else 0


MAX_FUSED_R = {4: 288, 8: 144}    # the sampler is fused on the 64-row tile only: two workgroups per compute unit
NARROW_MAX_R = {4: 1152, 8: 576}  # what the 32-row tile holds (the sandwich uses it up to d = 512)
R_VALUES = (1, 3, 4, 5, 16, 17, 128)
IDENTITY_D = (1, 3, 16, 17, 128)
FIRSTS = (0, 7, 2 ** 33 + 3)
SANDWICH_D = (1, 5, 16, 17, 129, 512)


def n_values(bm):
    return (1, bm - 1, bm + 1, 3 * bm + 5)


@pytest.mark.parametrize("esz", [4, 8])
def test_fused_boundary_follows_from_lds(driver, esz):
    rmax = MAX_FUSED_R[esz]
    assert BM(NARROW_MAX_R[esz], esz) == 32 and BM(NARROW_MAX_R[esz] + 1, esz) == 0
    assert BM(rmax, esz) == 64 and BM(rmax + 1, esz) == 32
    p = plan(driver, 100, rmax, rmax, esz)
    assert p["maxr"] == rmax and p["route"] == FUSED and p["bm"] == 64 and p["lds"] == LDS_MAX // 2
    p = plan(driver, 100, rmax + 1, rmax + 1, esz)
    assert p["route"] == STAGED


@pytest.mark.parametrize("esz", [4, 8])
@pytest.mark.parametrize("r", R_VALUES + ("max", "max+1"))
def test_plan_of_every_r(driver, esz, r):
    r = {"max": MAX_FUSED_R[esz], "max+1": MAX_FUSED_R[esz] + 1}.get(r, r)
    d = max(r, 130)
    for n in (1, 31, 33, 63, 65, 197, 10 ** 6):
        p = plan(driver, n, d, r, esz)
        assert p["block"] == 256 and p["kc"] == KC(esz)
        assert p["ldft"] % 64 == 0 and p["ldft"] >= d and p["factor"] == r * p["ldft"] * esz
        if r <= MAX_FUSED_R[esz]:
            bm = BM(r, esz)
            assert bm == 64
            assert p["route"] == FUSED and p["bm"] == bm and p["bn"] == BN(bm)
            assert p["grid"] == -(-n // bm) and p["ncoltiles"] == -(-d // BN(bm))
            assert p["lds"] == lds_bytes(r, bm, esz) <= LDS_MAX
            assert p["ws"] == 0 and p["nchunks"] == 0
        else:
            assert p["route"] == STAGED and (p["bm"], p["bn"]) == (64, 128)
            assert p["lds"] == KC(esz) * (64 + 128) * esz
            assert p["chunk_rows"] == min(n, WS_BUDGET // (r * esz) // 64 * 64)
            assert p["nchunks"] == -(-n // p["chunk_rows"])
            assert p["ws"] == p["chunk_rows"] * r * esz <= p["ws_bound"] == WS_BUDGET


@pytest.mark.parametrize("esz", [4, 8])
def test_staged_workspace_bound_at_the_widest_factor(driver, esz):
    p = plan(driver, 10 ** 6, 65536, 65536, esz)
    assert p["route"] == STAGED and p["chunk_rows"] == WS_BUDGET // (65536 * esz) // 64 * 64 >= 64
    assert p["ws"] <= p["ws_bound"] == WS_BUDGET
    assert plan(driver, 10, 65537, 65537, esz)["route"] == REJECT
    # a small r walks any d on the fused route
    assert plan(driver, 10, 10 ** 6, 4, esz)["route"] == FUSED


@pytest.mark.parametrize("esz", [4, 8])
def test_wide_stores_need_an_aligned_base_and_row_stride(driver, esz):
    vec = 16 // esz
    assert plan(driver, 70, 17, 3, esz, ldo=17 + (-17) % vec)["wide"] == 1
    assert plan(driver, 70, 17, 3, esz, ldo=17 + (-17) % vec + 1)["wide"] == 0
    assert plan(driver, 70, 16, 3, esz, ldo=16, out_aligned=0)["wide"] == 0
    assert plan(driver, 1, 16, 3, esz, ldo=0)["wide"] == 1   # one row has no stride


def test_rejections(driver):
    for kw, word in ((dict(n=4, d=3, r=4), "r > d"), (dict(n=4, d=3, r=0), "r >= 1"), (dict(n=-1, d=3, r=3), "n must be >= 0"),
                     (dict(n=4, d=3, r=3, ldo=-3), "negative strides"), (dict(n=4, d=3, r=3, ldo=2), "row stride"),
                     (dict(n=4, d=3, r=3, first=-1), "first"), (dict(n=4, d=3, r=2, lower=1), "square"),
                     (dict(n=4, d=3, r=3, esz=2), "element size"),
                     (dict(n=2 ** 62, d=4, r=4, first=2 ** 62), "63 bits"), (dict(n=1, d=4, r=4, first=2 ** 61), "63 bits")):
        kw.setdefault("esz", 8)
        p = plan(driver, **kw)
        assert p["route"] == REJECT and word in p["error"], (kw, p)
    assert plan(driver, 1, 4, 4, 8, first=2 ** 61 - 2)["route"] == FUSED   # (first + n) r = 2^63 - 4
    assert plan(driver, 0, 4, 4, 8)["route"] == EMPTY
    for args, word in (((0, 4, 8), "at least one row"), ((4, 0, 8), "d must be >= 1"), ((4, 513, 8), "<= 512"),
                       ((4, 4, 2), "element size")):
        p = sandwich(driver, *args)
        assert p["ok"] == 0 and word in p["error"], (args, p)
    p = sandwich(driver, 4, 8, 8, ldj=-8)
    assert p["ok"] == 0 and "negative strides" in p["error"]
    p = sandwich(driver, 4, 8, 8, ldj=7)
    assert p["ok"] == 0 and "below d" in p["error"]


@pytest.mark.parametrize("esz", [4, 8])
@pytest.mark.parametrize("d", SANDWICH_D)
def test_sandwich_plan(driver, esz, d):
    bm = BM(d, esz)
    assert bm in (32, 64)
    for m in (1, bm + 1, 10 ** 5):
        p = sandwich(driver, m, d, esz, ldj=d + 3)
        assert p["ok"] == 1 and p["bm"] == bm and p["bn"] == BN(bm) and p["block"] == 256
        assert p["grid"] == -(-m // bm) and p["ncoltiles"] == -(-d // BN(bm))
        assert p["lds"] == lds_bytes(d, bm, esz) <= LDS_MAX


def test_gpu_shape_tables():
    """what tests/test_gpu_mvn.py runs: every identity width on the fused route, the largest fused r and the first staged one
    among the general factors, both tiles among the sandwich widths"""
    for esz in (4, 8):
        assert all(BM(d, esz) == 64 for d in IDENTITY_D)
        assert BM(MAX_FUSED_R[esz], esz) == 64 and BM(MAX_FUSED_R[esz] + 1, esz) == 32
        assert n_values(64) == (1, 63, 65, 197)
        assert {BM(d, esz) for d in SANDWICH_D} == {32, 64}
    assert FIRSTS[-1] * 1 >= 2 ** 32   # the counter's second word is exercised at r = 1 already
