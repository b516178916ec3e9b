"""The plans of the column passes (corrla_rs_amd/csrc/colstat_plan.hpp), pinned on the CPU: the header is host code, compiled
here with the host compiler in a temporary directory.  The driver answers one query per line of its input, so a sweep is
one process.

OLD_* below is the launch arithmetic as hip_backend.hpp computed it inline before the plans existed -- HipDev::col_ss (both
branches), HipDev::col_ss_csr, HipDev::col_moments (which repeated the "down" branch) and HipDev::weighted_colsum -- restated
from that text, not from the header, in the fields of the one plan record (nslab: the slabs, segments, `segs` or `nblk` of
that text).  Every field of a plan must equal it over the sweep; the invariants a launcher relies on are asserted on the same
sweep.  GPU_CALLS is the table of tests/test_gpu_colstat.py, which imports it from here: one public call per branch of the
plans, with the fields that show the branch was reached, pinned at 256 compute units."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corrla_rs_amd", "csrc")
REJECT, DOWN, ALONG, CSR, WCOLSUM = range(5)

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "colstat_plan.hpp"
using namespace corrla;
int main() {
  char pass[16];
  long long a, b, c, d, e;
  static_assert(k::kCvThreads == 256 && k::cv_vec(4) == 4 && k::cv_vec(8) == 2 && k::cv_vec(2) == 8, "constants of the kernels");
  while (scanf("%15s", pass) == 1) {
    ColstatPlan p;
    if (!strcmp(pass, "colss")) {   // rows cols vec along_cols num_cus
      if (scanf("%lld %lld %lld %lld %lld", &a, &b, &c, &d, &e) != 5) return 2;
      p = colss_plan(a, b, (int)c, d != 0, (int)e);
    } else if (!strcmp(pass, "csr")) {   // rows num_cus
      if (scanf("%lld %lld", &a, &b) != 2) return 2;
      p = csr_colss_plan(a, (int)b);
    } else if (!strcmp(pass, "wcolsum")) {   // rows ncols
      if (scanf("%lld %lld", &a, &b) != 2) return 2;
      p = wcolsum_plan(a, (int)b);
    } else {
      return 2;
    }
    if ((p.branch == ColstatBranch::kReject) != (p.error != nullptr)) return 3;
    if (p.error) { printf("0 %s\n", p.error); continue; }
    printf("%d %d %lld %lld %lld %u %u %u %u %u %zu\n", (int)p.branch, p.groups, (long long)p.rows_per_slab, (long long)p.seg_len,
           (long long)p.nslab, p.grid_x, p.grid_y, p.block, p.final_grid_x, p.final_block, p.ws_bytes);
  }
  return 0;
}
"""

FIELDS = ("branch", "groups", "rows_per_slab", "seg_len", "nslab", "grid_x", "grid_y", "block", "final_grid_x", "final_block",
          "ws_bytes")


def build_driver(tmp, csrc=CSRC):
    src = os.path.join(tmp, "colstat_plan_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "colstat_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + csrc, src, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("colstat_plan")))


def plans(exe, queries):
    """queries: tuples (pass, args...) -> one dict per query, in order"""
    text = "".join(" ".join(str(v) for v in q) + "\n" for q in queries)
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    assert len(out) == len(queries)
    res = []
    for line in out:
        if line.startswith("0 "):
            res.append({"branch": REJECT, "error": line[2:]})
            continue
        vals = [int(v) for v in line.split()]
        assert len(vals) == len(FIELDS), line
        res.append(dict(zip(FIELDS, vals)))
    return res


# ---- the arithmetic the plans replaced (hip_backend.hpp at the parent commit) ---------------------------------------------------
def _ceil(a, b):
    return (a + b - 1) // b


def OLD_col_ss(rows, cols, vec, along_cols, num_cus):
    """HipDev::col_ss: a.rows, a.cols of the staged operand; check_grid threw where "error" is set here"""
    n = cols if along_cols else rows
    target = num_cus * 8
    if along_cols:
        ngroups = _ceil(cols, vec)
        groups = 1
        while groups < 256 and groups < ngroups:
            groups *= 2
        ny = 256 // groups
        col_blocks = _ceil(ngroups, groups)
        want = max(1, min(_ceil(target, col_blocks), _ceil(rows, 8 * ny)))
        rows_per_slab = _ceil(rows, want)
        nslab = _ceil(rows, rows_per_slab)
        if nslab > 65535:
            return {"branch": REJECT, "error": "problem too large for the launch grid"}
        return {"branch": DOWN, "groups": groups, "rows_per_slab": rows_per_slab, "seg_len": 0, "nslab": nslab,
                "grid_x": col_blocks, "grid_y": nslab, "block": 256, "final_grid_x": _ceil(n, 256), "final_block": 256,
                "ws_bytes": 8 * nslab * n}
    quantum = 64 * vec
    max_segs = _ceil(cols, 4 * quantum)
    want = max(1, min(_ceil(4 * target, rows), max_segs))
    seg_len = _ceil(_ceil(cols, want), quantum) * quantum
    nslab = _ceil(cols, seg_len)
    units = rows * nslab
    blocks = max(1, min(_ceil(units, 4), 2 * target))
    return {"branch": ALONG, "groups": 0, "rows_per_slab": 0, "seg_len": seg_len, "nslab": nslab, "grid_x": blocks,
            "grid_y": 1, "block": 256, "final_grid_x": _ceil(n, 256), "final_block": 256, "ws_bytes": 8 * nslab * n}


def OLD_col_moments(m, n, vec, num_cus):
    """HipDev::col_moments: x is m x n row-major; psum and psq are one array of ws_bytes each"""
    ngroups = _ceil(n, vec)
    groups = 1
    while groups < 256 and groups < ngroups:
        groups *= 2
    ny = 256 // groups
    col_blocks = _ceil(ngroups, groups)
    target = num_cus * 8
    want = max(1, min(_ceil(target, col_blocks), _ceil(m, 8 * ny)))
    rows_per_slab = _ceil(m, want)
    nslab = _ceil(m, rows_per_slab)
    if nslab > 65535:
        return {"branch": REJECT, "error": "problem too large for the launch grid"}
    return {"branch": DOWN, "groups": groups, "rows_per_slab": rows_per_slab, "seg_len": 0, "nslab": nslab,
            "grid_x": col_blocks, "grid_y": nslab, "block": 256, "final_grid_x": _ceil(n, 256), "final_block": 256,
            "ws_bytes": 8 * nslab * n}


def OLD_col_ss_csr(rows, num_cus):
    """HipDev::col_ss_csr: psum and pcnt are `units` doubles each"""
    target = num_cus * 8
    segs = max(1, min(_ceil(4 * target, rows), 64))
    units = rows * segs
    blocks = max(1, min(_ceil(units, 4), 2 * target))
    return {"branch": CSR, "groups": 0, "rows_per_slab": 0, "seg_len": 0, "nslab": segs, "grid_x": blocks, "grid_y": 1,
            "block": 256, "final_grid_x": _ceil(rows, 256), "final_block": 256, "ws_bytes": 2 * 8 * units}


def OLD_weighted_colsum(rows, ncols):
    nblk = max(1, min(64, _ceil(rows, 4096)))
    return {"branch": WCOLSUM, "groups": 0, "rows_per_slab": 0, "seg_len": 0, "nslab": nblk, "grid_x": nblk, "grid_y": ncols,
            "block": 256, "final_grid_x": _ceil(ncols, 64), "final_block": 64, "ws_bytes": 8 * nblk * ncols}


SIZES = (1, 2, 5, 7, 8, 61, 64, 77, 255, 256, 257, 1024, 1031, 1500, 4096, 65536, 10 ** 6)
VECS = (2, 4, 8)
CUS = (1, 64, 256, 304)
# beyond the sweep: the only way to a grid.y above 65535 is a device of thousands of compute units (want <= 8 num_cus)
TOO_LARGE = ("colss", 10 ** 6, 1024, 4, 1, 10000)
COLSS_SWEEP = [("colss", r, c, v, a, cu) for r, c, v, a, cu in itertools.product(SIZES, SIZES, VECS, (1, 0), CUS)]
CSR_SWEEP = [("csr", r, cu) for r, cu in itertools.product(SIZES, CUS)]
WCOLSUM_SWEEP = [("wcolsum", r, c) for r, c in itertools.product(SIZES + (4097, 262144, 262145), (1, 8, 16, 64, 65, 256))]


def check_restatement(exe):
    """every field of every plan against OLD_* over the sweep; raises AssertionError at the first difference"""
    qs = COLSS_SWEEP + [TOO_LARGE]
    for q, p in zip(qs, plans(exe, qs)):
        assert p == OLD_col_ss(q[1], q[2], q[3], bool(q[4]), q[5]), (q, p)
        if q[4]:
            assert p == OLD_col_moments(q[1], q[2], q[3], q[5]), (q, p)
    for q, p in zip(CSR_SWEEP, plans(exe, CSR_SWEEP)):
        assert p == OLD_col_ss_csr(q[1], q[2]), (q, p)
    for q, p in zip(WCOLSUM_SWEEP, plans(exe, WCOLSUM_SWEEP)):
        assert p == OLD_weighted_colsum(q[1], q[2]), (q, p)


def test_every_field_equals_the_inline_arithmetic_it_replaced(driver):
    check_restatement(driver)


def test_invariants_the_launchers_rely_on(driver):
    for (_, rows, cols, vec, along_cols, _cu), p in zip(COLSS_SWEEP, plans(driver, COLSS_SWEEP)):
        n = cols if along_cols else rows
        assert p["branch"] == (DOWN if along_cols else ALONG)
        assert min(p["grid_x"], p["grid_y"], p["block"], p["final_grid_x"], p["final_block"], p["nslab"]) >= 1, p
        assert p["ws_bytes"] == p["nslab"] * n * 8 and p["final_grid_x"] * p["final_block"] >= n
        if along_cols:
            # the slabs cover the rows exactly once, none empty; the column blocks cover the 16-byte groups
            step, total = p["rows_per_slab"], rows
            g = p["groups"]
            assert g & (g - 1) == 0 and 1 <= g <= 256
            assert p["grid_x"] * g * vec >= cols > (p["grid_x"] - 1) * g * vec
            assert p["grid_y"] == p["nslab"] <= 65535
        else:
            step, total = p["seg_len"], cols
            assert step % (64 * vec) == 0 and p["grid_y"] == 1
        assert step >= 1 and (p["nslab"] - 1) * step < total <= p["nslab"] * step, p
    for (_, rows, _cu), p in zip(CSR_SWEEP, plans(driver, CSR_SWEEP)):
        units = rows * p["nslab"]
        assert p["branch"] == CSR and 1 <= p["nslab"] <= 64 and p["ws_bytes"] == 2 * units * 8
        assert p["grid_x"] >= 1 and p["grid_y"] == 1 and p["final_grid_x"] * p["final_block"] >= rows
    for (_, rows, ncols), p in zip(WCOLSUM_SWEEP, plans(driver, WCOLSUM_SWEEP)):
        # the kernel gives slab b the rows [b * per, (b + 1) * per) with per = ceil(rows / nslab): none of them is empty
        per = _ceil(rows, p["nslab"])
        assert p["branch"] == WCOLSUM and 1 <= p["nslab"] <= 64 and (p["nslab"] - 1) * per < rows
        assert p["ws_bytes"] == p["nslab"] * ncols * 8
        assert p["grid_x"] == p["nslab"] and p["grid_y"] == ncols and p["final_grid_x"] * p["final_block"] >= ncols


def test_the_rejection_carries_check_grids_message(driver):
    assert plans(driver, [TOO_LARGE]) == [{"branch": REJECT, "error": "problem too large for the launch grid"}]


# ---- the calls of tests/test_gpu_colstat.py --------------------------------------------------------------------------------------
# One row per branch of the plans: the public call that reaches it and the fields that show it did.
#   colvar rows   Context.pca(standardize=True) of an m x n matrix of `dtype` in `layout`: row-major memory holds the data
#                 columns along its columns (down, the staged operand is m x n), column-major memory holds them as its rows
#                 (along, the staged operand is n x m); a CSR operand of m x n reduces over the n rows of its transpose
#   moments rows  Context.cov(correlation=True) of a row-major m x n matrix (ld: its row stride): the down plan
#   wcolsum rows  Context.pca(center="fused") of a tall m x n matrix: the correction of A^T Y sums over m rows
# ld is the row stride of a row-major matrix where it is not n.
VEC = {"float32": 4, "float64": 2, "bf16": 8}
GPU_CALLS = [
    dict(id="down-groups2-short-last-slab", kind="colvar", dtype="float32", m=1031, n=5, layout="row",
         expect=dict(branch=DOWN, groups=2, nslab=2, rows_per_slab=516, grid_x=1)),
    dict(id="down-groups32-17-slabs", kind="colvar", dtype="float32", m=1031, n=77, layout="row",
         expect=dict(branch=DOWN, groups=32, nslab=17, rows_per_slab=61, grid_x=1)),
    dict(id="down-groups256-two-column-blocks", kind="colvar", dtype="float32", m=61, n=1500, layout="row",
         expect=dict(branch=DOWN, groups=256, nslab=8, rows_per_slab=8, grid_x=2)),
    dict(id="down-bf16-vec8", kind="colvar", dtype="bf16", m=1024, n=64, layout="row",
         expect=dict(branch=DOWN, groups=8, nslab=4, rows_per_slab=256, grid_x=1)),
    dict(id="down-ld-n-plus-3", kind="colvar", dtype="float32", m=1031, n=76, layout="row", ld=79,
         expect=dict(branch=DOWN, groups=32, nslab=17, rows_per_slab=61, grid_x=1)),
    dict(id="along-one-segment", kind="colvar", dtype="float32", m=61, n=1500, layout="col",
         expect=dict(branch=ALONG, nslab=1, seg_len=256, grid_x=375)),
    dict(id="along-two-segments", kind="colvar", dtype="float32", m=1031, n=77, layout="col",
         expect=dict(branch=ALONG, nslab=2, seg_len=768, grid_x=39)),
    dict(id="along-f64-quantum", kind="colvar", dtype="float64", m=1031, n=77, layout="col",
         expect=dict(branch=ALONG, nslab=3, seg_len=384, grid_x=58)),
    dict(id="csr-64-segments", kind="csr", dtype="float32", m=1031, n=77, expect=dict(branch=CSR, nslab=64, grid_x=1232)),
    dict(id="csr-fewer-segments", kind="csr", dtype="float32", m=1031, n=150, expect=dict(branch=CSR, nslab=55, grid_x=2063)),
    dict(id="moments-groups2-short-last-slab", kind="moments", dtype="float32", m=1031, n=5,
         expect=dict(branch=DOWN, groups=2, nslab=2, rows_per_slab=516, grid_x=1)),
    dict(id="moments-groups32-17-slabs", kind="moments", dtype="float32", m=1031, n=77,
         expect=dict(branch=DOWN, groups=32, nslab=17, rows_per_slab=61, grid_x=1)),
    dict(id="moments-groups256-two-column-blocks", kind="moments", dtype="float32", m=61, n=1500,
         expect=dict(branch=DOWN, groups=256, nslab=8, rows_per_slab=8, grid_x=2)),
    dict(id="moments-ld-n-plus-3-f64", kind="moments", dtype="float64", m=1031, n=76, ld=79,
         expect=dict(branch=DOWN, groups=64, nslab=33, rows_per_slab=32, grid_x=1)),
    dict(id="wcolsum-one-slab", kind="wcolsum", dtype="float32", m=1031, n=77, expect=dict(branch=WCOLSUM, nslab=1)),
    dict(id="wcolsum-two-slabs", kind="wcolsum", dtype="float64", m=4097, n=16, expect=dict(branch=WCOLSUM, nslab=2)),
]
WCOLSUM_NCOLS = 16   # of the table's wcolsum queries: the padded sketch width (the slab count does not depend on it)


def plan_query(call):
    """the plan query of a row of GPU_CALLS at 256 compute units"""
    m, n = call["m"], call["n"]
    if call["kind"] == "colvar":
        rows, cols, along_cols = (m, n, 1) if call["layout"] == "row" else (n, m, 0)
        return ("colss", rows, cols, VEC[call["dtype"]], along_cols, 256)
    if call["kind"] == "moments":
        return ("colss", m, n, VEC[call["dtype"]], 1, 256)
    if call["kind"] == "csr":
        return ("csr", n, 256)
    return ("wcolsum", m, WCOLSUM_NCOLS)


def test_the_gpu_files_calls_reach_every_branch(driver):
    got = plans(driver, [plan_query(c) for c in GPU_CALLS])
    for call, p in zip(GPU_CALLS, got):
        assert {key: p[key] for key in call["expect"]} == call["expect"], (call["id"], p)
    by_id = {c["id"]: p for c, p in zip(GPU_CALLS, got)}
    assert 1031 % by_id["down-groups2-short-last-slab"]["rows_per_slab"] != 0          # a short last slab
    assert 256 // by_id["down-groups256-two-column-blocks"]["groups"] == 1           # ny = 1
    assert {p["branch"] for p in got} == {DOWN, ALONG, CSR, WCOLSUM}
    assert {p["groups"] for c, p in zip(GPU_CALLS, got) if c["kind"] == "moments"} >= {2, 32, 256}
    assert len({c["id"] for c in GPU_CALLS}) == len(GPU_CALLS)


@pytest.mark.parametrize("good,bad", [
    ("(rows + 8 * ny - 1) / (8 * ny)", "(rows + 4 * ny - 1) / (4 * ny)"),                  # the down plan's rows per lane
    ("const int64_t max_segs = (cols + 4 * quantum - 1) / (4 * quantum);", "const int64_t max_segs = (cols + quantum - 1) / quantum;"),
    ("(4 * target + rows - 1) / rows, 64)", "(4 * target + rows - 1) / rows, 32)"),       # the CSR plan's segment cap
    ("(rows + 4095) / 4096", "(rows + 4096) / 4096"),                                     # the weighted sums' slab rule
])
def test_a_perturbed_rule_is_caught(tmp_path, good, bad):
    """A scratch copy of the header with one rule changed must fail the restatement check above."""
    scratch = tmp_path / "csrc"
    scratch.mkdir()
    txt = open(os.path.join(CSRC, "colstat_plan.hpp")).read()
    assert txt.count(good) == 1
    (scratch / "colstat_plan.hpp").write_text(txt.replace(good, bad))
    exe = build_driver(str(tmp_path), str(scratch))
    with pytest.raises(AssertionError):
        check_restatement(exe)
