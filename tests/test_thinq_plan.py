"""The plan of the thin-Q orthonormalisation, pinned on the CPU: thinq_plan.hpp (corrla_rs_amd/csrc) is host code, compiled
here with the host compiler in a temporary directory.  The route of every width 1 .. 400 against a table; every field of
thinq_route, hh_tree_plan and hh_column_blocks against OLD_* below -- the arithmetic as hip_backend.hpp and driver.hpp
made it inline (device_chol_fits, device_chol_blocked_fits, device_qr_robust_fits, qr_inplace_fits, chol_inv, block_split,
householder_fits / _up / _down / _max_width, householder_thin_q_any_width) before the plan carried it; robust_schedule
against the loop header of orthonormalize_device as it stood; robust_shift_rel against its line."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_MAX = 400
LDS_MAX = 160 * 1024
NO_CAP = 2 ** 63 - 1
KNOBS = {"default": (0, 1), "host_chol": (1, 1), "robust_off": (0, 0)}  # (CORRLA_HOST_CHOL, CORRLA_DEVICE_ROBUST_QR)
FACTOR = ["single", "blocked", "none"]  # enum ThinQFactor

# One query per line on stdin, one answer per line on stdout (integers; doubles as %.17g).
MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "thinq_plan.hpp"
using namespace corrla;
int main() {
  char cmd[32];
  long long a, b, c, d;
  while (std::scanf("%31s %lld %lld %lld %lld", cmd, &a, &b, &c, &d) == 5) {
    if (!std::strcmp(cmd, "route")) {  // esz l host_chol robust_qr
      ThinQKnobs kn;
      kn.host_chol = c != 0;
      kn.robust_qr = d != 0;
      const ThinQRoute r = thinq_route((size_t)a, b, kn);
      std::printf("%d %lld %lld %d %d %d", (int)r.factor, (long long)r.n1, (long long)r.n2, r.records_per_pass, (int)r.robust, (int)r.inplace);
      for (int i = 0; i < 2; ++i) std::printf(" %d %u %zu", r.blk[i].n, r.blk[i].threads, r.blk[i].lds);
      std::printf("\n");
    } else if (!std::strcmp(cmd, "hhfit")) {  // esz l
      std::printf("%d %d\n", (int)hh_fits((size_t)a, b), hh_max_width((size_t)a));
    } else if (!std::strcmp(cmd, "tree")) {  // esz m l
      const HhTreePlan p = hh_tree_plan((size_t)a, b, c);
      std::printf("%s|%d %d %d %d %zu %zu %zu %zu", p.error ? p.error : "", (int)p.fits, p.nleaf, p.max_rows, p.levels, p.lds_up_leaf,
                  p.lds_up_tree, p.lds_down_tree, p.lds_down_leaf);
      for (int k_ = 0; k_ <= p.levels; ++k_)
        std::printf(" %d %zu %zu %zu %zu %zu", p.n_at[k_], p.r_elems[k_], p.c_elems[k_], p.tau_elems[k_], p.v_elems[k_], p.t_elems[k_]);
      std::printf("\n");
    } else if (!std::strcmp(cmd, "blocks")) {  // l wmax cap
      const HhColumnBlocks cb = hh_column_blocks(a, b, c);
      std::printf("%lld %lld\n", (long long)cb.nb, (long long)cb.w);
    } else if (!std::strcmp(cmd, "sched")) {  // passes mode inplace
      const RobustSchedule s = robust_schedule((int)a, (RobustMode)b, c != 0);
      std::printf("%d %d %d", s.npass, s.always, s.flag_slot);
      for (int p = 0; p < s.npass; ++p)
        std::printf(" %d %d %d %.9g %d", s.pass[p].gate, s.pass[p].shift_mode, (int)s.pass[p].null_excess, (double)s.pass[p].need_ratio,
                    (int)s.pass[p].refill);
      std::printf("\n");
    } else if (!std::strcmp(cmd, "shift")) {  // esz rows l single
      std::printf("%.17g\n", robust_shift_rel((size_t)a, b, c, d != 0));
    } else if (!std::strcmp(cmd, "grids")) {  // rows l r
      const Grid2 g = refill_null_grid(a, b), s = series_grid(c);
      std::printf("%u %u %u %u %u %u\n", g.x, g.y, g.block, s.x, s.y, s.block);
    } else if (!std::strcmp(cmd, "consts")) {
      std::printf("%d %d %d %d %d %zu\n", k::kHhThreads, k::kHhMaxRowsPerLane, k::kWyNb, k::kWyExtra, kRobustMaxPasses, sizeof(k::CholStatus));
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("thinq_plan")
    src = tmp / "plan.cpp"
    src.write_text(MAIN)
    exe = tmp / "plan"
    # plain host compiler, warnings are errors: the header has no HIP call
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "corrla_rs_amd", "csrc"),
                           str(src), "-o", str(exe)])

    def run(queries):
        text = "".join(" ".join(str(x) for x in (list(q) + [0, 0, 0, 0])[:5]) + "\n" for q in queries)
        out = subprocess.check_output([str(exe)], input=text, text=True).splitlines()
        assert len(out) == len(queries)
        return out
    return run


# ---- the arithmetic the plan replaced (hip_kernels.hpp, tsqr_kernels.hpp, hip_backend.hpp, driver.hpp at the parent commit) ----
def OLD_round_up(x, a):
    return (x + a - 1) // a * a


def OLD_chol_inv_threads(r):
    nt = (r + 3) // 4
    return ((nt * (nt + 1) // 2 + 63) // 64) * 64


def OLD_chol_inv_lds_bytes(r, esz):
    return 6 * ((r + 3) // 4 * 4) * esz + 32 * 4 + 64


def OLD_chol_inv_fits(r, esz):
    return r >= 1 and OLD_chol_inv_threads(r) <= (768 if esz == 8 else 1024)


def OLD_device_chol_fits(esz, l, host_chol):
    return l <= 4096 and OLD_chol_inv_fits(l, esz) and not host_chol


def OLD_device_chol_blocked_fits(esz, l, host_chol):
    n1 = OLD_round_up((l + 1) // 2, 4)
    return l > 8 and l <= 4096 and OLD_chol_inv_fits(n1, esz) and not host_chol


def OLD_qr_inplace_fits(l):
    tiles = max(1, (l + 15) // 16)
    return (tiles + 9 - 1) // 9 == 1  # col_blocking(l).nblk == 1


def OLD_route(esz, l, host_chol, robust_qr):
    """what orthonormalize_core / orthonormalize_device / block_split / chol_inv made of the four fit tests"""
    single = OLD_device_chol_fits(esz, l, host_chol)
    blocked = OLD_device_chol_blocked_fits(esz, l, host_chol)
    rpp = 1 if single else (2 if blocked else 0)
    robust = bool(robust_qr) and (single or blocked)
    if rpp == 1:
        n1, n2 = l, 0
    elif rpp == 2:
        n1 = OLD_round_up((l + 1) // 2, 4)
        n2 = l - n1
    else:
        n1 = n2 = 0
    blk = []
    for n in (n1, n2):
        blk += [n, OLD_chol_inv_threads(n), OLD_chol_inv_lds_bytes(n, esz)] if n > 0 else [0, 0, 0]
    return [2 if rpp == 0 else rpp - 1, n1, n2, rpp, int(robust), int(OLD_qr_inplace_fits(l))] + blk


def OLD_hh_pitch(rows):
    return (rows + 3) & ~3


def OLD_hh_lds_bytes(rows, l, esz):
    return OLD_hh_pitch(rows) * l * esz + 64


def OLD_hh_wy_lds_bytes(rows, l, esz):
    return OLD_hh_lds_bytes(rows, l, esz) + (2 * 16 * 16 + 16) * esz


def OLD_householder_fits(esz, l):  # hh_wy_ set (the default): the panel is sized by the WY formula
    return l >= 1 and l <= 4096 and OLD_hh_wy_lds_bytes(2 * l, l, esz) <= LDS_MAX and 2 * l <= 64 * 5


def OLD_householder_max_width(esz):
    w = 1
    while OLD_householder_fits(esz, w + 1):
        w += 1
    return w


def OLD_tree(esz, m, l):
    """householder_up / householder_down: error text, then the launch geometry and the buffer element counts per level"""
    fits = OLD_householder_fits(esz, l)
    if m < l:
        return "householder_thin_q: fewer rows than columns", [int(fits)]
    if not fits:
        return "householder_thin_q: panel does not fit in LDS", [0]
    br = 2 * l
    nleaf = 1 if m <= br else (m + br - 1) // br
    if nleaf > 0x3fffffff:
        return "householder_thin_q: too many panels", [1]
    max_rows = min(m, br)
    n_at = [nleaf]
    while n_at[-1] > 1:
        n_at.append((n_at[-1] + 1) // 2)
    levels = len(n_at) - 1
    ll = l * l
    tsz = ((l + 15) // 16) * 16 * 16
    out = [1, nleaf, max_rows, levels, OLD_hh_wy_lds_bytes(max_rows, l, esz), OLD_hh_wy_lds_bytes(2 * l, l, esz),
           OLD_hh_lds_bytes(2 * l, l, esz), OLD_hh_lds_bytes(max_rows, l, esz)]
    for k, n in enumerate(n_at):
        out += [n, ll * n, ll * n, l * n, 2 * ll * n if k >= 1 else 0, tsz * n]
    return "", out


def OLD_column_blocks(l, wmax, cap):
    """householder_thin_q_any_width: (nb, w); one panel is (1, l)"""
    if cap is not None:
        wmax = max(1, min(wmax, cap))
    if l <= wmax:
        return [1, l]
    nb = (l + wmax - 1) // wmax
    return [nb, (l + nb - 1) // nb]


def OLD_schedule(passes, rough, polish, inplace):
    """the loop header of orthonormalize_device"""
    level = max(2, min(passes, 8))
    inloop = rough and not polish
    npass = (1 if level <= 2 else level - 1) if inloop else ((1 if level <= 2 else 3) if polish else level)
    always = 1 if (polish or inloop) else 2
    out = [npass, always, -1 if (inloop and npass > 1) else 0]
    for p in range(npass):
        gate = -1 if p < always else (p - 1 if inplace else always + ((p - always) // 2) * 2 - 1)
        shift_mode = 2 if polish else (1 if p == 0 else 0)
        nx = (not polish) and p >= 2
        need_ratio = float(np.float32(1e-2)) if (inloop and p == 0) else 0.0
        refill = p + 1 < npass or inloop
        out.append((gate, shift_mode, int(nx), need_ratio, int(refill)))
    return out


# ---- the route table ----
# (first l, last l, factor) per element size under the default knobs; single wins where both fit, so the blocked form's
# floor (l > 8) never shows
ROUTES = {4: [(1, 176, "single"), (177, 352, "blocked"), (353, L_MAX, "none")],
          8: [(1, 152, "single"), (153, 304, "blocked"), (305, L_MAX, "none")]}
INPLACE_MAX = 144
HH_MAX_WIDTH = {4: 142, 8: 99}


@pytest.fixture(scope="module")
def routes(ask):
    keys = [(esz, kn, l) for esz in (4, 8) for kn in KNOBS for l in range(1, L_MAX + 1)]
    ans = ask([("route", esz, l) + KNOBS[kn] for esz, kn, l in keys])
    return {key: [int(x) for x in line.split()] for key, line in zip(keys, ans)}


@pytest.mark.parametrize("esz", [4, 8])
def test_route_table(routes, ask, esz):
    ranges = ROUTES[esz]
    assert ranges[0][0] == 1 and ranges[-1][1] == L_MAX
    assert all(a[1] + 1 == b[0] for a, b in zip(ranges, ranges[1:]))  # the ranges tile 1 .. L_MAX
    for lo, hi, factor in ranges:
        for l in range(lo, hi + 1):
            r = routes[(esz, "default", l)]
            assert FACTOR[r[0]] == factor, l
            assert r[3] == {"single": 1, "blocked": 2, "none": 0}[factor], l
            assert r[4] == (factor != "none"), l                      # device-robust wherever a device factor exists
            assert r[5] == (l <= INPLACE_MAX), l
            # robust off: the same factor, never the robust schedule; CORRLA_HOST_CHOL: nothing on the device
            off, host = routes[(esz, "robust_off", l)], routes[(esz, "host_chol", l)]
            assert off[:4] == r[:4] and off[4] == 0 and off[5:] == r[5:], l
            assert FACTOR[host[0]] == "none" and host[1:5] == [0, 0, 0, 0] and host[5] == r[5] and host[6:] == [0] * 6, l
    # the blocked form itself starts above 8: asked alone (no single factor), 8 does not fit and 9 does
    assert not OLD_device_chol_blocked_fits(esz, 8, False) and OLD_device_chol_blocked_fits(esz, 9, False)
    fits = ask([("hhfit", esz, l) for l in range(1, L_MAX + 1)])
    for l, line in zip(range(1, L_MAX + 1), fits):
        f, wmax = (int(x) for x in line.split())
        assert f == (l <= HH_MAX_WIDTH[esz]) and wmax == HH_MAX_WIDTH[esz], l


def test_route_fields_match_the_inline_arithmetic(routes):
    for (esz, kn, l), got in routes.items():
        assert got == OLD_route(esz, l, *KNOBS[kn]), (esz, kn, l)


def _boundary_ls(esz):
    edges = [8, 9, 144, 145, 176, 177, 152, 153, 352, 353, 304, 305, HH_MAX_WIDTH[esz], HH_MAX_WIDTH[esz] + 1]
    return sorted({l for e in edges for l in (e - 1, e, e + 1) if l >= 1} | {1, 2, 16, 17, 33, 64})


@pytest.mark.parametrize("esz", [4, 8])
def test_tree_plan_matches_the_inline_arithmetic(ask, esz):
    cases = [(l, m) for l in _boundary_ls(esz) for m in (l, 2 * l, 2 * l + 1, 5 * l, 64 * l + 3)]
    cases += [(10, 9), (1, 2 ** 31 + 5), (2, 2 ** 33)]  # fewer rows than columns; many leaves; too many panels
    ans = ask([("tree", esz, m, l) for l, m in cases])
    seen = set()
    for (l, m), line in zip(cases, ans):
        err, _, nums = line.partition("|")
        want_err, want = OLD_tree(esz, m, l)
        assert err == want_err, (l, m)
        got = [int(x) for x in nums.split()]
        if err:
            assert got[0] == want[0], (l, m)
        else:
            assert got == want, (l, m)
            nleaf = got[1]
            seen |= {1 if nleaf == 1 else (2 if nleaf == 2 else ("odd" if nleaf % 2 else "even")), "many" if nleaf > 16 else "few"}
        seen.add(err)
    # one leaf, two, an odd count (pass-through nodes), many; each refusal
    assert {1, 2, "odd", "many", "", "householder_thin_q: fewer rows than columns", "householder_thin_q: panel does not fit in LDS",
            "householder_thin_q: too many panels"} <= seen


@pytest.mark.parametrize("esz", [4, 8])
def test_column_blocks_match_the_inline_arithmetic(ask, esz):
    wmax = OLD_householder_max_width(esz)
    assert wmax == HH_MAX_WIDTH[esz]
    # ... and exact multiples of each width, where a count rounded the wrong way shows
    ls = sorted(set(_boundary_ls(esz)) | {2 * wmax, 3 * wmax, 56, 138, 207, 280})
    cases = [(l, cap) for l in ls for cap in (None, 69, 28)]
    ans = ask([("blocks", l, wmax, NO_CAP if cap is None else cap) for l, cap in cases])
    for (l, cap), line in zip(cases, ans):
        got = [int(x) for x in line.split()]
        assert got == OLD_column_blocks(l, wmax, cap), (l, cap)
        assert got[0] * got[1] >= l and got[1] <= wmax


MODES = {"final": (0, False, False), "inloop": (1, True, False), "polish": (2, False, True)}  # enum RobustMode, rough, polish


def _parse_sched(line):
    t = line.split()
    head = [int(x) for x in t[:3]]
    body = [(int(t[i]), int(t[i + 1]), int(t[i + 2]), float(t[i + 3]), int(t[i + 4])) for i in range(3, len(t), 5)]
    return head + body


@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("passes", [2, 4, 8])
def test_robust_schedule_matches_the_loop_header(ask, passes, mode, inplace):
    code, rough, polish = MODES[mode]
    got = _parse_sched(ask([("sched", passes, code, int(inplace))])[0])
    want = OLD_schedule(passes, rough, polish, inplace)
    assert got[:3] == want[:3]
    assert len(got) == len(want)
    for g, w in zip(got[3:], want[3:]):
        assert g[:3] == w[:3] and g[4] == w[4] and abs(g[3] - w[3]) <= 1e-9 * max(w[3], 1e-30)
    npass, always = got[0], got[1]
    gates = [p[0] for p in got[3:]]
    assert gates[:always] == [-1] * always and all(0 <= g < i for i, g in enumerate(gates) if i >= always)
    if not inplace:
        # conditional passes come in pairs, both gated by the word of the pass before the pair: a skipped pair leaves
        # the data where the host expects it
        assert (npass - always) % 2 == 0
        for i in range(always, npass, 2):
            assert gates[i] == gates[i + 1] == i - 1
    # polish rides with rough or without: orthonormalize_device asks polish first
    if polish:
        assert want == OLD_schedule(passes, True, True, inplace)
    # the context's count outside 2 .. 8 is clamped as the driver clamped it
    assert _parse_sched(ask([("sched", 1, code, int(inplace))])[0]) == _parse_sched(ask([("sched", 2, code, int(inplace))])[0])
    assert _parse_sched(ask([("sched", 16, code, int(inplace))])[0]) == _parse_sched(ask([("sched", 8, code, int(inplace))])[0])


@pytest.mark.parametrize("esz", [4, 8])
def test_robust_shift_rel(ask, esz):
    eps = float(np.finfo(np.float32 if esz == 4 else np.float64).eps)
    cases = [(rows, l, single) for rows in (1, 4096, 10 ** 7) for l, single in ((138, 1), (177, 0), (352, 0))]
    ans = ask([("shift", esz, rows, l, single) for rows, l, single in cases])
    for (rows, l, single), line in zip(cases, ans):
        want = eps * max(16.0, 0.25 * math.sqrt(max(rows, 1)), 0.0 if single else 2.0 * l)
        assert float(line) == want, (rows, l, single)
    # rows 1: the 16 eps floor; 10^7 rows: the Gram's rounding error; blocked: the Schur complement's l eps
    assert float(ans[0]) == 16 * eps and float(ans[6]) == eps * 0.25 * math.sqrt(10 ** 7) and float(ans[2]) == eps * 704


def test_small_grids_and_constants(ask):
    cases = [(rows, l, r) for rows in (1, 255, 256, 257, 16384, 10 ** 7) for l, r in ((1, 1), (64, 64), (65, 65), (352, 352))]
    ans = ask([("grids", rows, l, r) for rows, l, r in cases])
    for (rows, l, r), line in zip(cases, ans):
        want = [max(min(64, (rows + 255) // 256), 1), l, 256, (r + 63) // 64, r, 64]  # refill_null, series_prep / series_combine
        assert [int(x) for x in line.split()] == want, (rows, l, r)
    assert [int(x) for x in ask([("consts",)])[0].split()] == [1024, 5, 16, 528, 8, 32]


def test_the_arithmetic_is_stated_once():
    """The split of the blocked form and the `single or blocked` disjunction live in the plan alone; the backend launches no
    thin-Q kernel itself; the emulation backend carries none of the limits as literals."""
    import re
    csrc = os.path.join(ROOT, "corrla_rs_amd", "csrc")

    def code(path):  # without comments
        return re.sub(r"//[^\n]*", "", open(path).read())
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hpp", ".hip")) and name != "thinq_plan.hpp":
            text = code(os.path.join(csrc, name))
            assert "round_up((l + 1) / 2" not in open(os.path.join(csrc, name)).read(), name
            assert not re.search(r"device_chol_fits<T>\(l\)\s*\|\|", text), name
    backend = code(os.path.join(csrc, "hip_backend.hpp"))
    for kernel in ("chol_inv_kernel", "gram_inspect_kernel", "combine_need_kernel", "refill_null_kernel", "series_prep_kernel",
                   "series_combine_kernel", "hh_leaf_factor_kernel", "hh_tree_factor_kernel", "hh_tree_apply_kernel", "hh_leaf_apply_kernel"):
        assert kernel not in backend, kernel
        assert kernel in code(os.path.join(csrc, "thinq_stage.hpp")), kernel
    for helper in ("chol_inv_threads", "chol_inv_lds_bytes", "hh_lds_bytes", "hh_wy_lds_bytes", "hh_wy_panels", "CORRLA_HH_WY"):
        assert helper not in backend, helper
    emu = code(os.path.join(ROOT, "tests", "emu", "emu_backend.cpp"))
    assert not re.search(r"\b(176|152|276|528|320)\b", emu)
    assert "thinq_route(" in emu and "hh_fits(" in emu and "hh_max_width(" in emu
