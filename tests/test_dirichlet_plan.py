"""The plan of the Dirichlet sampling kernels behind corrla_dirichlet_draws_* and corrla_dirichlet_sample_*
(corrla_rs_amd/csrc/dirichlet_plan.hpp), pinned on the CPU: the header is host code, compiled here with the host compiler in a
temporary directory.

Pinned: the workgroups of a shot cover its draws exactly once (ranges of R = 1024, the last one short, none empty) for chunk
sizes of 1, R - 1, R, R + 1 and 10^6; the workspace of a launch (bits, counts, prefixes, table, state) stays within the plan's
stated bound whatever chunk_size and max_zshots are; the register route ends and the regenerate route begins exactly at
kDirRegD; the exponential-only route is taken exactly when every alpha is 1; the method table follows alpha; the batches of a
call at least double and never make more read-backs than the plan states, whatever acceptance they meet; every rejection
names its argument.  The file ends with the shape tables of tests/test_gpu_dirichlet.py (GPU_CALLS)."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corrla_rs_amd", "csrc")
THREADS, DPT, RANGE, WORDS, REG_D, MAX_D, LAUNCH_WGS, FIRST_BATCH, MAX_ATTEMPTS = 256, 4, 1024, 16, 16, 128, 65536, 1024, 64
EXP, MT, BOOST = 0, 1, 2
ROUTES = {(True, True): 1, (True, False): 2, (False, True): 3, (False, False): 4}   # (registers, exponential-only)

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dirichlet_plan.hpp"
using namespace corrla;
int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "batch")) {  // batch total done found n_samples prev
    if (argc != 7) return 2;
    printf("%lld\n", (long long)dir_next_batch(atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), atoll(argv[5]), atoll(argv[6])));
    return 0;
  }
  // plan d c_scale n_samples max_zshots chunk first n null_alphas null_bounds alphas[d] bounds[2 d]
  if (argc < 11) return 2;
  DirShape s;
  s.d = atoll(argv[2]); s.c_scale = atof(argv[3]); s.n_samples = atoll(argv[4]); s.max_zshots = atoll(argv[5]);
  s.chunk_size = atoll(argv[6]); s.first = atoll(argv[7]); s.n = atoll(argv[8]);
  const bool null_alphas = atoi(argv[9]), null_bounds = atoi(argv[10]);
  std::vector<double> al, bo;
  int at = 11;
  for (int64_t j = 0; j < s.d && at < argc; ++j) al.push_back(atof(argv[at++]));
  while (at < argc) bo.push_back(atof(argv[at++]));
  s.alphas = null_alphas ? nullptr : al.data();
  s.bounds = null_bounds ? nullptr : bo.data();
  const DirPlan p = dir_plan(s);
  printf("ok %d\n", (int)p.ok);
  if (!p.ok) { printf("error %s\n", p.error); return 0; }
  printf("reg_width %d\nexp_only %d\nroute %d\ndpt %d\nrange %d\nwords %d\nblock %u\ndraw_grid %u\n", p.reg_width, (int)p.exp_only, (int)p.route,
         p.dpt, p.range, p.words, p.block, p.draw_grid_x);
  printf("wps %lld\ntotal_wgs %lld\nlaunch_wgs %lld\nfirst_batch_wgs %lld\nmax_readbacks %d\n", (long long)p.wps, (long long)p.total_wgs,
         (long long)p.launch_wgs, (long long)p.first_batch_wgs, p.max_readbacks);
  printf("ws_mask %zu\nws_count %zu\nws_prefix %zu\nws_table %zu\nws %zu\nws_bound %zu\n", p.ws_mask_bytes, p.ws_count_bytes, p.ws_prefix_bytes,
         p.ws_table_bytes, p.ws_bytes, p.ws_bound);
  printf("consts %d %d %d %d %d %d %lld %lld %d %zu\n", k::kDirThreads, k::kDirDPT, k::kDirRange, k::kDirWords, k::kDirRegD, k::kDirMaxD,
         (long long)k::kDirLaunchWgs, (long long)k::kDirFirstBatchWgs, k::kDirMaxAttempts, sizeof(DirComp));
  for (int64_t j = 0; j < s.d; ++j) {
    const DirComp m = dir_component(al[j]);
    printf("comp%lld %d %.17g %.17g %.17g\n", (long long)j, m.method, m.d_mt, m.c_mt, m.inv_alpha);
  }
  return 0;
}
"""


def build_driver(tmp, csrc=CSRC):
    src = os.path.join(tmp, "dirichlet_plan_driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "dirichlet_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + csrc, src, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("dirichlet_plan")))


def plan(exe, alphas, *, bounds=None, c_scale=1.0, n_samples=0, max_zshots=1, chunk_size=1, first=0, n=1, d=None, null_alphas=False,
         null_bounds=False):
    d = len(alphas) if d is None else d
    if bounds is None and n_samples:
        bounds = [(0.0, c_scale)] * d
    flat = [v for b in (bounds or []) for v in b]
    args = ["plan", d, repr(float(c_scale)), n_samples, max_zshots, chunk_size, first, n, int(null_alphas), int(null_bounds)]
    out = subprocess.check_output([exe] + [str(v) for v in args] + [repr(float(v)) for v in list(alphas) + flat], text=True)
    lines = dict(line.partition(" ")[::2] for line in out.splitlines())
    p = {"ok": int(lines["ok"])}
    if not p["ok"]:
        p["error"] = lines["error"]
        return p
    for key, v in lines.items():
        if key == "consts":
            p[key] = tuple(int(x) for x in v.split())
        elif key.startswith("comp"):
            f = v.split()
            p.setdefault("comps", []).append((int(f[0]),) + tuple(float(x) for x in f[1:]))
        elif key != "ok":
            p[key] = int(v)
    return p


def next_batch(exe, total, done, found, n_samples, prev):
    return int(subprocess.check_output([exe, "batch"] + [str(v) for v in (total, done, found, n_samples, prev)], text=True))


def test_the_constants_are_the_ones_this_file_and_the_gpu_test_assume(driver):
    p = plan(driver, [1.0, 1.0, 1.0])
    assert p["consts"][:9] == (THREADS, DPT, RANGE, WORDS, REG_D, MAX_D, LAUNCH_WGS, FIRST_BATCH, MAX_ATTEMPTS)
    assert p["consts"][9] == 48                       # DirComp: five doubles and two ints, no padding the kernels do not know of
    assert RANGE == THREADS * DPT and WORDS * 64 == RANGE
    assert (p["dpt"], p["range"], p["words"], p["block"]) == (DPT, RANGE, WORDS, THREADS)


@pytest.mark.parametrize("chunk", [1, RANGE - 1, RANGE, RANGE + 1, 10 ** 6])
@pytest.mark.parametrize("max_zshots", [1, 7, 500])
def test_the_workgroups_of_a_shot_cover_its_draws_exactly_once(driver, chunk, max_zshots):
    p = plan(driver, [1.0] * 3, n_samples=10, max_zshots=max_zshots, chunk_size=chunk)
    assert p["ok"]
    wps = p["wps"]
    assert wps == -(-chunk // RANGE)
    # range k of a shot is [k R, min(chunk, (k + 1) R)): the first wps - 1 are full, the last is not empty and ends at chunk
    ends = [min(chunk, (k + 1) * RANGE) for k in range(wps)]
    starts = [k * RANGE for k in range(wps)]
    assert starts[0] == 0 and ends[-1] == chunk and all(s < e for s, e in zip(starts, ends))
    assert all(e == s for e, s in zip(ends[:-1], starts[1:]))
    assert p["total_wgs"] == max_zshots * wps
    assert p["launch_wgs"] == min(p["total_wgs"], LAUNCH_WGS)
    assert p["first_batch_wgs"] == min(p["total_wgs"], FIRST_BATCH)


@pytest.mark.parametrize("chunk,max_zshots", [(1, 1), (1, 500), (10 ** 6, 500), (2 ** 40, 2 ** 21), (2 ** 61, 1), (1, 2 ** 61)])
def test_the_workspace_stays_within_the_stated_bound(driver, chunk, max_zshots):
    for d in (2, REG_D + 1, MAX_D):
        p = plan(driver, [0.5] * d, n_samples=3000, max_zshots=max_zshots, chunk_size=chunk)
        assert p["ok"], p
        assert p["launch_wgs"] <= LAUNCH_WGS
        assert p["ws_mask"] == p["launch_wgs"] * WORDS * 8            # one bit per draw: an eighth of a byte
        assert p["ws_count"] == p["launch_wgs"] * 4 and p["ws_prefix"] == p["launch_wgs"] * 8
        assert p["ws_table"] == 48 * d
        assert p["ws"] <= p["ws_bound"] == LAUNCH_WGS * (WORDS * 8 + 12) + MAX_D * 48 + 5 * 256
    assert p["ws_bound"] < 10 << 20


@pytest.mark.parametrize("d", [2, 3, 4, 5, REG_D - 1, REG_D, REG_D + 1, 40, MAX_D])
@pytest.mark.parametrize("exp_only", [True, False])
def test_the_register_route_ends_exactly_at_kDirRegD(driver, d, exp_only):
    alphas = [1.0] * d if exp_only else [1.0] * (d - 1) + [0.6]
    for kw in ({}, {"n_samples": 5, "max_zshots": 2, "chunk_size": 100}):
        p = plan(driver, alphas, **kw)
        assert p["ok"]
        assert p["reg_width"] == (4 if d <= 4 else REG_D if d <= REG_D else 0)
        assert p["exp_only"] == int(exp_only)
        assert p["route"] == ROUTES[(d <= REG_D, exp_only)]


def test_the_method_table_follows_alpha(driver):
    alphas = [1.0, 0.3, 2.5, 7.0, 0.6, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, 50.0]
    p = plan(driver, alphas)
    for a, (method, d_mt, c_mt, inv) in zip(alphas, p["comps"]):
        assert inv == 1.0 / a
        if a == 1.0:
            assert (method, d_mt, c_mt) == (EXP, 0.0, 0.0)
        else:
            s = a if a > 1.0 else a + 1.0
            assert method == (MT if a > 1.0 else BOOST)
            assert d_mt == s - 1.0 / 3.0 and c_mt == 1.0 / math.sqrt(9.0 * d_mt)    # the same IEEE operations, bit for bit


def test_draw_plans(driver):
    for n in (1, THREADS, THREADS + 1, 3 * RANGE + 5):
        p = plan(driver, [1.0] * 3, n=n, first=2 ** 33 + 7)
        assert p["ok"] and p["draw_grid"] == -(-n // THREADS) and p["ws"] <= p["ws_bound"]
    assert plan(driver, [1.0] * 3, first=2 ** 62 - 5, n=5)["ok"]


@pytest.mark.parametrize("total", [1, FIRST_BATCH - 1, FIRST_BATCH, FIRST_BATCH + 1, 4 * 500, 977 * 500, 2 ** 40])
@pytest.mark.parametrize("rate", [0.0, 1e-7, 1.8e-5, 0.01, 0.5])
def test_batches_at_least_double_and_respect_the_read_back_bound(driver, total, rate):
    """simulated acceptance `rate` per draw; the found count the plan sees is whatever the batches so far gave"""
    n_samples = 3000
    chunk_plan = plan(driver, [1.0] * 3, n_samples=n_samples, max_zshots=1, chunk_size=min(total, 2 ** 50) * RANGE)
    assert chunk_plan["total_wgs"] == total
    done = found = prev = readbacks = 0
    while done < total and found < n_samples:
        b = next_batch(driver, total, done, found, n_samples, prev)
        assert 1 <= b <= total - done
        if prev == 0:
            assert b == min(total, FIRST_BATCH)
        else:
            assert b >= 2 * prev or b == total - done
        done, prev, readbacks = done + b, b, readbacks + 1
        found = int(done * RANGE * rate)
    assert readbacks <= chunk_plan["max_readbacks"] == 1 + max(0, math.ceil(math.log2(max(1, -(-total // FIRST_BATCH)))))


REJECTIONS = [
    (dict(alphas=[1.0]), "d"),
    (dict(alphas=[1.0] * (MAX_D + 1)), "d"),
    (dict(alphas=[1.0] * 3, null_alphas=True), "alphas"),
    (dict(alphas=[1.0, 0.0, 1.0]), "alphas"),
    (dict(alphas=[1.0, -1.0, 1.0]), "alphas"),
    (dict(alphas=[1.0, float("inf"), 1.0]), "alphas"),
    (dict(alphas=[1.0, float("nan"), 1.0]), "alphas"),
    (dict(alphas=[1.0] * 3, c_scale=0.0), "c_scale"),
    (dict(alphas=[1.0] * 3, c_scale=float("inf")), "c_scale"),
    (dict(alphas=[1.0] * 3, c_scale=float("nan")), "c_scale"),
    (dict(alphas=[1.0] * 3, first=-1), "first"),
    (dict(alphas=[1.0] * 3, n=0), "n "),
    (dict(alphas=[1.0] * 3, first=2 ** 62 - 5, n=6), "first + n"),
    (dict(alphas=[1.0] * 3, n_samples=5, null_bounds=True), "bounds"),
    (dict(alphas=[1.0] * 3, n_samples=-1), "n_samples"),
    (dict(alphas=[1.0] * 3, n_samples=5, max_zshots=0), "max_zshots"),
    (dict(alphas=[1.0] * 3, n_samples=5, chunk_size=0), "chunk_size"),
    (dict(alphas=[1.0] * 3, n_samples=5, max_zshots=2 ** 31, chunk_size=2 ** 31), "max_zshots * chunk_size"),
    (dict(alphas=[1.0] * 3, n_samples=5, bounds=[(0.0, 1.0), (0.5, 0.4), (0.0, 1.0)]), "bounds[j][0]"),
    (dict(alphas=[1.0] * 3, n_samples=5, bounds=[(0.0, 1.0), (0.0, float("inf")), (0.0, 1.0)]), "bounds[j]"),
    (dict(alphas=[1.0] * 3, n_samples=5, bounds=[(0.0, 1.0), (float("nan"), 1.0), (0.0, 1.0)]), "bounds[j]"),
    (dict(alphas=[1.0] * 3, n_samples=5, bounds=[(0.5, 1.0), (0.4, 1.0), (0.2, 1.0)]), "infeasible"),
    (dict(alphas=[1.0] * 3, n_samples=5, bounds=[(0.0, 0.3), (0.0, 0.3), (0.0, 0.3)]), "infeasible"),
    (dict(alphas=[1.0] * 3, n_samples=5, c_scale=2.5, bounds=[(0.0, 0.8)] * 3), "infeasible"),
]


@pytest.mark.parametrize("kw,names", REJECTIONS)
def test_every_rejection_names_its_argument(driver, kw, names):
    kw = dict(kw)
    p = plan(driver, kw.pop("alphas"), **kw)
    assert not p["ok"]
    assert p["error"].startswith("dirichlet: ") and names in p["error"], p["error"]


def test_a_box_that_touches_the_simplex_is_feasible(driver):
    # sum of the upper bounds equal to c_scale up to rounding: 0.1 + 0.2 + 0.7 and ten times 0.1 are not 1 exactly
    assert plan(driver, [1.0] * 3, n_samples=1, bounds=[(0.0, 0.1), (0.0, 0.2), (0.0, 0.7)])["ok"]
    assert plan(driver, [1.0] * 10, n_samples=1, bounds=[(0.1, 1.0)] * 10)["ok"]
    assert plan(driver, [1.0] * 3, n_samples=1, c_scale=2.5, bounds=[(0.0, 2.5)] * 3)["ok"]


# ---- the shapes of tests/test_gpu_dirichlet.py, which imports them from here: one table for both files -----------------------
MIXED5 = (0.3, 1.0, 2.5, 7.0, 0.6)
# draws: (d or alphas, n, first), one axis at a time from the base case
DRAW_BASE = ((0.6,) * 3, RANGE + 1, 0)
DRAW_ALPHAS = ((1.0,) * 2, (1.0,) * 3, (1.0,) * REG_D, (1.0,) * (REG_D + 1), (1.0,) * 40, (0.6,) * 2, (0.6,) * REG_D,
               (0.6,) * (REG_D + 1), (0.6,) * 40, MIXED5, MIXED5 * 4, (1.0, 50.0, 1.0))
DRAW_N = (1, RANGE - 1, RANGE, 3 * RANGE + 5)
DRAW_FIRST = (2 ** 33 + 7,)
# constrained sampling: name -> (bounds, alphas, the acceptance estimated on the CPU with numpy's own Dirichlet)
BOXES = {
    "A": (((0.1, 0.6), (0.05, 0.5), (0.2, 0.7)), (1.0,) * 3, 0.34),
    "B": (((0.0, 0.05), (0.3, 0.4), (0.55, 0.7)), (1.0,) * 3, 0.010),
    "C": (((0.0, 0.5),) * 5, MIXED5, 0.19),
    "D": (((0.0, 0.2),) * 17, (1.0,) * 17, 0.56),
}
SAMPLE_N, SAMPLE_CHUNK = 300, 4096
URANIUM_BOX = ((0.0, 0.0026), (0.1955, 0.1995), (0.80, 0.825))


def _draw_calls():
    calls = [DRAW_BASE]
    calls += [(a, DRAW_BASE[1], DRAW_BASE[2]) for a in DRAW_ALPHAS]
    calls += [(DRAW_BASE[0], n, DRAW_BASE[2]) for n in DRAW_N]
    calls += [(DRAW_BASE[0], DRAW_BASE[1], f) for f in DRAW_FIRST]
    calls += [((1.0,) * (REG_D + 1), 5, DRAW_FIRST[0])]
    out = []
    for c in calls:
        if c not in out:
            out.append(c)
    return out


GPU_CALLS = _draw_calls()


def test_gpu_calls_are_plans_the_header_accepts(driver):
    for alphas, n, first in GPU_CALLS:
        p = plan(driver, list(alphas), n=n, first=first)
        assert p["ok"] and p["route"] == ROUTES[(len(alphas) <= REG_D, all(a == 1.0 for a in alphas))]
    assert {plan(driver, list(a), n=1)["route"] for a, _, _ in GPU_CALLS} == {1, 2, 3, 4}
    for bounds, alphas, _ in BOXES.values():
        p = plan(driver, list(alphas), bounds=bounds, n_samples=SAMPLE_N, max_zshots=500, chunk_size=SAMPLE_CHUNK)
        assert p["ok"] and p["wps"] == 4
