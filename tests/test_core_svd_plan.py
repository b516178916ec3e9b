"""The plan of the core SVD (random_svd.rs:89), pinned on the CPU: core_svd_plan (corrla_rs_amd/csrc/core_svd_plan.hpp) is
host code, compiled here with the host compiler in a temporary directory.  Two checks: the kernel family and ring E at
every l against a table, and every field of the plan against OLD_* below -- the launch arithmetic as hip_backend.hpp made
it inline (small_svd_mc, jmc_launch_step, small_svd_block, small_svd_ring) before the plan carried it."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_MAX = 1100

# (first l, last l, family, ring E) per element size and CORRLA_SVD mode; the ranges cover 1 .. L_MAX
EXPECTED = {
    (4, "default"): [(1, 1, "block", 0), (2, 64, "ring", 8), (65, 95, "ring", 12), (96, 288, "mc", 0),
                     (289, 1024, "block", 0), (1025, L_MAX, "host", 0)],
    (8, "default"): [(1, 1, "block", 0), (2, 64, "ring", 8), (65, 95, "ring", 12), (96, 288, "mc", 0),
                     (289, 1024, "block", 0), (1025, L_MAX, "host", 0)],
    (4, "mc"): [(1, 1, "block", 0), (2, 288, "mc", 0), (289, 1024, "block", 0), (1025, L_MAX, "host", 0)],
    (8, "mc"): [(1, 1, "block", 0), (2, 288, "mc", 0), (289, 1024, "block", 0), (1025, L_MAX, "host", 0)],
    (4, "block"): [(1, 1024, "block", 0), (1025, L_MAX, "host", 0)],
    (8, "block"): [(1, 1024, "block", 0), (1025, L_MAX, "host", 0)],
    (4, "host"): [(1, L_MAX, "host", 0)],
    (8, "host"): [(1, L_MAX, "host", 0)],
    # the single-workgroup kernel: the ring while W fits in LDS (f32: E = 20 up to 144, f64: E = 18 up to 138)
    (4, "lds"): [(1, 1, "block", 0), (2, 64, "ring", 8), (65, 96, "ring", 12), (97, 128, "ring", 16),
                 (129, 144, "ring", 20), (145, 1024, "block", 0), (1025, L_MAX, "host", 0)],
    (8, "lds"): [(1, 1, "block", 0), (2, 64, "ring", 8), (65, 96, "ring", 12), (97, 128, "ring", 16),
                 (129, 138, "ring", 18), (139, 1024, "block", 0), (1025, L_MAX, "host", 0)],
}

MAIN = r"""
#include <cstdio>
#include "core_svd_plan.hpp"
int main() {
  const char* modes[] = {nullptr, "mc", "block", "host", "lds"};
  const char* names[] = {"ring", "mc", "block", "host"};
  const int eszs[] = {4, 8};
  for (int esz : eszs)
    for (const char* m : modes)
      for (int l = 1; l <= %d; ++l) {
        corrla::CoreSvdKnobs kn;
        kn.mode = m;
        const corrla::CoreSvdPlan p = corrla::core_svd_plan(esz, l, kn);
        std::printf("%%d %%s %%d %%s %%d\n", esz, m ? m : "default", l, names[(int)p.family], p.ring_e);
      }
  return 0;
}
""" % L_MAX


def _compile(tmp, name, text):
    src = tmp / (name + ".cpp")
    src.write_text(text)
    exe = tmp / name
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "corrla_rs_amd", "csrc"),
                           str(src), "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = _compile(tmp_path_factory.mktemp("core_svd_plan"), "plan", MAIN)
    out = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        esz, mode, l, fam, e = line.split()
        out[(int(esz), mode, int(l))] = (fam, int(e))
    return out


@pytest.mark.parametrize("esz,mode", sorted(EXPECTED))
def test_core_svd_plan_table(plans, esz, mode):
    ranges = EXPECTED[(esz, mode)]
    assert ranges[0][0] == 1 and ranges[-1][1] == L_MAX
    assert all(a[1] + 1 == b[0] for a, b in zip(ranges, ranges[1:]))
    for lo, hi, fam, e in ranges:
        for l in range(lo, hi + 1):
            assert plans[(esz, mode, l)] == (fam, e), (esz, mode, l)


# ---- every field of the plan against the launch arithmetic it replaced --------------------------------------------------
# The knob axes of the comparison; l is thinned to both sides of every width at which OLD_geometry / OLD_family change
# their answer under any of these knobs (_grid_ls), and a few widths in between.
MODES = ["default", "mc", "block", "host", "lds"]
MAX_BS = [8, 16, 24, 32]
LOCALS = [0, 1]
NPS = [0, 3, 5]
SWEEPS = [0, 5]            # CORRLA_JMC_SWEEPS: 0 = absent
STRICTS = [0, 1]
HINTS = [0, 4, 12]
EXTRAS = [0, 8, 24]
FORCE_VS = [0, 1, 2]       # off, the context's state, CORRLA_JMC_FORCE_V
OPTIMISTIC = [1, 0]
FIELDS = ["family", "ring_e", "tol", "tol_early", "floor2",
          "mc.nc", "mc.np", "mc.b", "mc.local", "mc.rp", "mc.nblocks", "mc.ncols_pad", "mc.step_threads", "mc.step_lds",
          "mc.ws_bytes", "mc.fin_lds", "mc.other_grid", "mc.force_v", "mc.nsw", "mc.group", "mc.max_sweeps",
          "blk.nb", "blk.cols_pad", "blk.rows_pad", "blk.ws_bytes", "blk.round_lds", "blk.max_sweeps", "blk.inner", "blk.fin_lds",
          "ring.block", "ring.lds", "ring.max_sw", "ring.rot_bytes", "ring.rank_bytes", "ring.replay_grid"]
RING, MC, BLOCK, HOST = 0, 1, 2, 3  # enum CoreSvd
LDS_MAX = 160 * 1024


def _k_of(l):
    return max(1, l - 8)


def _c_list(v):
    return "{" + ", ".join(str(x) for x in v) + "}"


# argv: esz, mode, then the widths.  One record of int64 per grid point (doubles by their bits), FIELDS order, to stdout.
FIELDS_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "core_svd_plan.hpp"
static long long bits(double x) { long long b; std::memcpy(&b, &x, sizeof(b)); return b; }
int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int esz = std::atoi(argv[1]);
  const char* mode = std::strcmp(argv[2], "default") ? argv[2] : nullptr;
  const int max_bs[] = %s, locals[] = %s, nps[] = %s, sweeps[] = %s, stricts[] = %s, hints[] = %s, extras[] = %s, force_vs[] = %s,
            optimistic[] = %s;
  std::vector<long long> rec;
  for (int i = 3; i < argc; ++i) {
    const int l = std::atoi(argv[i]);
    rec.clear();
    for (int max_b : max_bs) for (int local : locals) for (int np : nps) for (int sw : sweeps) for (int strict : stricts)
    for (int hint : hints) for (int extra : extras) for (int fv : force_vs) for (int opt : optimistic) {
      corrla::CoreSvdKnobs kn;
      kn.mode = mode;
      kn.jmc_max_b = max_b;
      kn.jmc_local = local;
      kn.jmc_np = np;
      if (sw) kn.jmc_sweeps_f32 = kn.jmc_sweeps_f64 = sw;
      kn.strict = strict != 0;
      kn.jmc_force_v = fv == 2;
      corrla::CoreSvdState st;
      st.sweeps_hint = hint;
      st.extra_sweeps = extra;
      st.force_v = fv == 1;
      const corrla::CoreSvdPlan p = corrla::core_svd_plan(esz, l, l > 9 ? l - 8 : 1, kn, st, opt != 0);
      const long long f[] = {(long long)p.family, p.ring_e, bits(p.tol), bits(p.tol_early), bits(p.floor2),
          p.mc.nc, p.mc.np, p.mc.b, p.mc.local, p.mc.rp, p.mc.nblocks, p.mc.ncols_pad, p.mc.step_threads, (long long)p.mc.step_lds,
          (long long)p.mc.ws_bytes, (long long)p.mc.fin_lds, p.mc.other_grid, p.mc.force_v, p.mc.nsw, p.mc.group, p.mc.max_sweeps,
          p.blk.nb, p.blk.cols_pad, p.blk.rows_pad, (long long)p.blk.ws_bytes, (long long)p.blk.round_lds, p.blk.max_sweeps,
          p.blk.inner, (long long)p.blk.fin_lds,
          p.ring.block, (long long)p.ring.lds, p.ring.max_sw, (long long)p.ring.rot_bytes, (long long)p.ring.rank_bytes,
          p.ring.replay_grid};
      static_assert(sizeof(f) / sizeof(f[0]) == %d, "FIELDS");
      rec.insert(rec.end(), f, f + sizeof(f) / sizeof(f[0]));
    }
    if (std::fwrite(rec.data(), sizeof(long long), rec.size(), stdout) != rec.size()) return 1;
  }
  return 0;
}
""" % tuple([_c_list(v) for v in (MAX_BS, LOCALS, NPS, SWEEPS, STRICTS, HINTS, EXTRAS, FORCE_VS, OPTIMISTIC)] + [len(FIELDS)])


# -- core_svd_plan.hpp's size helpers as they were (the kernels still call them with a lanes argument)
def OLD_jmc_pitch(nc, esz, lanes):
    rows = nc * 2 * lanes
    if lanes == 8:
        return rows + (16 if nc % 2 == 0 else 0)
    return rows + (32 if nc % 2 == 0 else 0) if esz == 4 else rows


def OLD_jmc_lds_bytes(nc, b, esz, lanes):
    return 2 * (2 * b) * OLD_jmc_pitch(nc, esz, lanes) * esz + 2 * b * esz + 64


def OLD_ring_w_lds_bytes(l, rs, esz):
    n2 = (l + 1) & ~1
    nproc = n2 // 2
    return 2 * nproc * rs * esz + n2 * (esz + 4) + 2 * nproc * esz + 64


def OLD_ring_e(l, esz):
    return 8 if l <= 64 else 12 if l <= 96 else 16 if l <= 128 else 20 if esz == 4 else 18


def OLD_geometry(l, esz, lanes, max_b, local, np_force):
    """jmc_geometry: (nc, np, b) or None."""
    if l < 2 or l > 288:
        return None
    nc = (l + 2 * lanes - 1) // (2 * lanes)

    def width(np_):
        bb = (l + 2 * np_ - 1) // (2 * np_)
        return (bb + 3) // 4 * 4 if local else bb + (bb & 1)

    np_ = np_force
    if np_ <= 0:
        np_ = 2
        while np_ < 128 and (width(np_) > max_b or OLD_jmc_lds_bytes(nc, width(np_), esz, lanes) > LDS_MAX):
            np_ += 1
    b = width(np_)
    if np_ < 1 or b < 2 or b > 32 or OLD_jmc_lds_bytes(nc, b, esz, lanes) > LDS_MAX:
        return None
    return nc, np_, b


def OLD_family(esz, mode, l, max_b, local, np_force, min_l=96):
    """core_svd_plan + HipDev::jmc_lanes (always 16): (family, ring E, geometry)."""
    geo = OLD_geometry(l, esz, 16, max_b, local, np_force)
    if mode in ("default", "mc") and (mode == "mc" or l >= min_l) and geo:
        return MC, 0, geo
    if mode == "host" or l > 1024:
        return HOST, 0, None
    if mode == "block":
        return BLOCK, 0, None
    e = OLD_ring_e(l, esz)
    if 2 <= l <= 144 and OLD_ring_w_lds_bytes(l, 8 * e, esz) <= LDS_MAX:
        return RING, e, None
    return BLOCK, 0, None


def _geometry_axes():
    return itertools.product(MAX_BS, LOCALS, NPS)


def _grid_ls():
    keep = {1, 2, 3, 17, 50, 138, 200, 266, 600, 1023, L_MAX}
    for esz in (4, 8):
        for mode in MODES:
            for knobs in _geometry_axes():
                prev = None
                for l in range(1, L_MAX + 1):
                    cur = OLD_family(esz, mode, l, *knobs)
                    if cur != prev and prev is not None:
                        keep.update((l - 1, l))
                    prev = cur
    return sorted(keep)


def _f64_bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def OLD_launch(esz, mode, ls):
    """Every FIELDS entry as the launchers computed it: {name: array that broadcasts over ls x the knob axes, in the order
    FIELDS_MAIN loops in}, and that shape."""
    shape = (len(ls), len(MAX_BS), len(LOCALS), len(NPS), len(SWEEPS), len(STRICTS), len(HINTS), len(EXTRAS), len(FORCE_VS),
             len(OPTIMISTIC))

    def axis(values, i):
        sh = [1] * len(shape)
        sh[i] = len(values)
        return np.asarray(values, dtype=np.int64).reshape(sh)

    l = axis(ls, 0)
    local, sweeps, strict = axis(LOCALS, 2), axis(SWEEPS, 4), axis(STRICTS, 5)
    hint, extra, fv, opt = axis(HINTS, 6), axis(EXTRAS, 7), axis(FORCE_VS, 8), axis(OPTIMISTIC, 9)
    k = axis([_k_of(x) for x in ls], 0)
    # family, E and geometry: scalar code over the axes they can depend on
    geo = np.zeros((5,) + shape[:4] + (1,) * 6, dtype=np.int64)
    for (i, lv), (a, max_b), (c, loc), (d, npf) in itertools.product(enumerate(ls), enumerate(MAX_BS), enumerate(LOCALS),
                                                                     enumerate(NPS)):
        fam_, e_, g = OLD_family(esz, mode, lv, max_b, loc, npf)
        geo[(slice(None), i, a, c, d) + (0,) * 6] = (fam_, e_) + (g or (0, 0, 0))
    fam, e, nc, np_, b = geo
    is_mc, is_blk, is_ring = fam == MC, fam == BLOCK, fam == RING
    out = {}
    out["family"], out["ring_e"] = fam, e
    eps = 2.0 ** -23 if esz == 4 else 2.0 ** -52
    lf = l.astype(np.float64)
    tol = np.sqrt(lf) * eps                                        # (T)(sqrt(l) * eps)
    tol_early = np.where((strict != 0) & ~is_blk, tol, math.sqrt(eps))  # STRICT ? tol : (T)sqrt(eps); block: (float)sqrt(eps)
    not_host = fam != HOST
    out["tol"] = np.where(not_host, _f64_bits(tol), 0)
    out["tol_early"] = np.where(not_host, _f64_bits(tol_early), 0)
    out["floor2"] = np.where(not_host, _f64_bits(lf * eps * eps), 0)
    fin_lds = (l + 2) * esz + (l + 2) * 4 + 64
    # small_svd_mc, jmc_launch_step
    lanes = 16
    rows = nc * 2 * lanes
    rp = np.where(esz == 4, rows + np.where(nc % 2 == 0, 32, 0), rows)
    nblocks = 2 * np_
    ncols_pad = nblocks * b
    nsw_default = np.maximum(1, np.where(sweeps != 0, sweeps, 10 if esz == 4 else 13))
    nsw = np.minimum(40, np.where(hint > 0, np.minimum(nsw_default, hint + 2), nsw_default) + extra)
    mc = {"nc": nc, "np": np_, "b": b, "local": local, "rp": rp, "nblocks": nblocks, "ncols_pad": ncols_pad,
          "step_threads": (b * lanes + 63) // 64 * 64,
          "step_lds": 2 * (2 * b) * rp * esz + 2 * b * esz + 64,
          "ws_bytes": rp * ncols_pad * esz, "fin_lds": fin_lds, "other_grid": (l * k * 16 + 255) // 256,
          "force_v": ((opt == 0) | (fv != 0)).astype(np.int64), "nsw": nsw, "group": 8, "max_sweeps": 40}
    for name, v in mc.items():
        out["mc." + name] = np.where(is_mc, v, 0)
    # small_svd_block
    nb = 2 * ((l + 15) // 16)
    rows_pad = (l + 15) // 16 * 16
    blk = {"nb": nb, "cols_pad": nb * 8, "rows_pad": rows_pad, "ws_bytes": rows_pad * nb * 8 * esz,
           "round_lds": (2 * 16 * (rows_pad + 1) + 7 * 16 * 17 + 32) * esz + 16 * 4 + 64, "max_sweeps": 12, "inner": 1,
           "fin_lds": fin_lds}
    for name, v in blk.items():
        out["blk." + name] = np.where(is_blk, v, 0)
    # small_svd_ring
    nproc = (l + 1) // 2
    n2 = 2 * nproc
    ring = {"block": nproc * 8, "lds": 2 * nproc * 8 * e * esz + n2 * (esz + 4) + 2 * nproc * esz + 64, "max_sw": 40,
            "rot_bytes": 40 * n2 * 72 * 2 * esz, "rank_bytes": 4 * n2, "replay_grid": (l + 256 // 16 - 1) // (256 // 16)}
    for name, v in ring.items():
        out["ring." + name] = np.where(is_ring, v, 0)
    return out, shape


@pytest.fixture(scope="module")
def fields_exe(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("core_svd_fields"), "fields", FIELDS_MAIN)


@pytest.fixture(scope="module")
def grid_ls():
    return _grid_ls()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("esz", [4, 8])
def test_core_svd_plan_fields_match_the_inline_arithmetic(fields_exe, grid_ls, esz, mode):
    raw = subprocess.check_output([str(fields_exe), str(esz), mode] + [str(l) for l in grid_ls])
    exp, shape = OLD_launch(esz, mode, grid_ls)
    got = np.frombuffer(raw, dtype=np.int64).reshape(shape + (len(FIELDS),))
    for j, name in enumerate(FIELDS):
        bad = np.argwhere(got[..., j] != exp[name])
        assert bad.size == 0, "%s at l = %d, knob indices %s: plan %d, inline arithmetic %d" % (
            name, grid_ls[bad[0][0]], bad[0][1:].tolist(), got[..., j][tuple(bad[0])], np.broadcast_to(exp[name], shape)[tuple(bad[0])])
    got = got.reshape(-1, len(FIELDS))
    # the instantiations that exist: jmc_step_kernel<T, 1 .. 9, 16>, jacobi_ring_w_kernel<T, E, 8>
    fam, e, nc = got[:, 0], got[:, 1], got[:, FIELDS.index("mc.nc")]
    assert set(np.unique(nc[fam == MC])) <= set(range(1, 10))
    assert set(np.unique(e[fam == RING])) <= {8, 12, 16, 20 if esz == 4 else 18}
    assert not nc[fam != MC].any() and not e[fam != RING].any()


# ---- one row per instantiation the launchers can select, at the smallest l that reaches it -----------------------------
# (esz, CORRLA_SVD mode, l, family, ring E, NC); tests/test_gpu_core_svd_routes.py makes one call per row on the GPU
def _routes():
    rows = []
    for esz in (4, 8):
        big_e, widest = (20, 144) if esz == 4 else (18, 138)
        rows += [(esz, "default", 2, RING, 8, 0), (esz, "default", 64, RING, 8, 0), (esz, "default", 65, RING, 12, 0),
                 (esz, "default", 95, RING, 12, 0), (esz, "lds", 97, RING, 16, 0), (esz, "lds", 129, RING, big_e, 0),
                 (esz, "lds", widest, RING, big_e, 0)]
        rows += [(esz, "mc", 32, MC, 0, 1), (esz, "mc", 64, MC, 0, 2)]
        rows += [(esz, "default", 32 * nc, MC, 0, nc) for nc in range(3, 10)]
        rows += [(esz, "default", 1, BLOCK, 0, 0), (esz, "default", 289, BLOCK, 0, 0), (esz, "lds", 145, BLOCK, 0, 0)]
    return rows


ROUTES = _routes()


@pytest.mark.parametrize("row", ROUTES, ids=lambda r: "f%d-%s-l%d" % (8 * r[0], r[1], r[2]))
def test_every_route_row_reaches_the_instantiation_it_names(fields_exe, row):
    esz, mode, l, fam, e, nc = row
    raw = subprocess.check_output([str(fields_exe), str(esz), mode, str(l)])
    got = np.frombuffer(raw, dtype=np.int64).reshape(-1, len(FIELDS))[0]  # the default knobs come first
    assert (got[0], got[1], got[FIELDS.index("mc.nc")]) == (fam, e, nc)
