"""The tall products' plan (corrla_rs_amd/csrc/gemm_plan.hpp), pinned on the CPU: gemm_plan is host code, compiled here with
the host compiler in a temporary directory.

OLD_* below is the routing of every product as hip_backend.hpp made it before the plan existed -- launch_gemm,
choose_geometry, launch_tall, launch_one / launch_mw and gemm_mixed_f32, knobs read per call included -- restated
independently of gemm_plan.  Each case compares the family, the instantiation, every launch's grid, column base, XCD remap
and dynamic LDS, the reduction split, rotation, written columns, the slab reduction and its workspace, the tall-Gram
grouping and the bf16 planes, or the rejection.  (The retired exact variant of the bf16-split skeleton, np = 0 under
CORRLA_GEMM_WIDE, was off by default and is not part of the table.)

ROUTES / GRAM_ROUTES at the end are the calls of tests/test_gpu_gemm_routes.py, which multiplies each against a reference on
the GPU: one Context.matmul (or, for the aliased Gram kernels, one power_iter) per instantiation launch_gemm (tall_stage.hpp)
can dispatch and per feature of a launch.  PLANE_ROUTES / ATA_ROUTES next to them are the calls of
tests/test_gpu_tall_routes.py for the bf16-split, bf16-stored and one-sweep kernels; tests/test_tall_stage_plan.py pins them.  Pinned here: every row's plan has the properties the row names, all 90 general and 16 aliased
instantiations and every feature of FEATURES occur, the knob names are the ones a context reads, and the integer operands
of the exact check tell neighbouring tiles and columns apart."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB_NAMES = ("split_nn", "split_tn", "mw", "xcd_remap", "tall_min_rows", "persist_max_tiles", "f64_waves", "mixed_min_work",
              "even_blocks", "no_gram_alias", "no_rotate", "mixed_split")
DEFAULT_KNOBS = dict(split_nn=0, split_tn=0, mw=0, xcd_remap=1, tall_min_rows=65536, persist_max_tiles=16, f64_waves=8,
                     mixed_min_work=16777216.0, even_blocks=0, no_gram_alias=0, no_rotate=0, mixed_split=0)
SHAPE_NAMES = ("tn", "esz", "r_rows", "r_cols", "r_ld", "r_cols_readable", "r_aligned", "x_cols", "x_ld", "x_cols_alloc",
               "x_external", "x_aligned", "out_rows", "out_ld", "out_cols", "out_cols_alloc", "out_external", "out_aligned",
               "same", "np", "num_cus")


def cdiv(a, b):
    return (a + b - 1) // b


def round_up(a, b):
    return cdiv(a, b) * b


def col_blocking(cols):
    tiles = max(1, cdiv(cols, 16))
    nblk = cdiv(tiles, 9)
    nt = cdiv(tiles, nblk)
    return tiles, nblk, nt, nblk * nt * 16


# ---- LDS sizes as hip_kernels.hpp / tall_kernels.hpp / mixed_kernels.hpp computed them ----
def stage_bytes(mw, nt):
    return 64 * 256 * mw + nt * 16 * 256


def gemm_stages(mw, nt):
    return 3 if 3 * stage_bytes(mw, nt) <= 160 * 1024 else 2


def gram_lds(nct, esz):
    tile = 16 * nct * 512
    ring = min(4, (160 * 1024 - 4096) // tile) * tile
    return max(ring, 3 * (nct * (nct + 1) // 2) * 256 * esz)


def mx_lds(nt, np_):
    return 3 * 256 * 32 * 4 + 2 * np_ * nt * 16 * 32 * 2 + 1024


def fmt(family, inst, block, launches, tiles_total=0, nsplit=1, tps=0, outer_blocks=0, rotate=0, vec_store=0, out_cols=0,
        slab_stride=0, slab_bytes=0, reduce=("none", 0, 0, 0, 0, 0), rpg=0, groups=0, planes=(0, 0, 0, 0)):
    """one line, in the printer's layout"""
    f = [family] + list(inst) + [block, len(launches)]
    for g in launches:
        f += list(g)
    f += [tiles_total, nsplit, tps, outer_blocks, rotate, vec_store, out_cols, slab_stride, slab_bytes]
    f += list(reduce) + [rpg, groups] + list(planes)
    return " ".join(str(v) for v in f)


def old_reduce(nsplit, outer_n, cols_alloc, out_cols):
    if nsplit >= 8:
        return ("deep", cdiv(outer_n, 64), cols_alloc, nsplit, outer_n, out_cols)
    if nsplit > 1:
        return ("plain", cdiv(outer_n, 256), cols_alloc, nsplit, outer_n, out_cols)
    return ("none", 0, 0, 0, 0, 0)


def old_mixed(s, kn, outer_n, red_n):
    """gemm_mixed_f32 with mixed_fits, np = 2 / 3"""
    tiles, nblk, nt, cols_alloc = col_blocking(s["x_cols"])
    if s["np"] not in (2, 3):
        return "reject internal: bf16 split takes 2 or 3 planes"
    fits = (s["esz"] == 4 and not s["x_external"] and nblk == 1 and s["r_aligned"] and s["r_ld"] % 4 == 0 and
            s["r_cols_readable"] % 4 == 0 and s["x_aligned"] and s["x_ld"] % 64 == 0 and s["x_ld"] >= round_up(red_n, 32) and
            s["out_ld"] >= outer_n and s["out_rows"] == outer_n and not s["same"] and outer_n >= 1 and red_n >= 1 and
            float(outer_n) * float(red_n) >= kn["mixed_min_work"])
    if not fits:
        return "reject internal: operands outside the bf16-split kernels' domain"
    if (cols_alloc > s["x_cols_alloc"] or (not s["out_external"] and cols_alloc > s["out_cols_alloc"]) or
            (s["out_external"] and s["out_cols"] < s["x_cols"])):
        return "reject internal: skinny column padding too small for the column blocking"
    plane_stride = s["x_ld"] * cols_alloc
    planes = (plane_stride, cols_alloc, s["np"] * plane_stride * 2, max(1, min(4096, cdiv(plane_stride // 8, 256))))
    tiles_total = cdiv(red_n, 32)
    outer_tiles = cdiv(outer_n, 256)
    nsplit = 1
    if outer_tiles < s["num_cus"]:
        nsplit = min((s["num_cus"] + outer_tiles // 2) // outer_tiles, max(1, tiles_total // 16))
    if kn["mixed_split"]:
        nsplit = kn["mixed_split"]
    nsplit = max(1, min(nsplit, tiles_total, 65535))
    out_cols = s["out_cols"] if s["out_external"] else cols_alloc
    stride = s["out_ld"] * cols_alloc
    vec = int(s["out_ld"] % 4 == 0 and s["out_aligned"])
    launch = (outer_tiles, 1, nsplit, nt, 0, 0, mx_lds(nt, s["np"]))
    return fmt("bf16_split", [s["np"]], 64 * 12, [launch], tiles_total, nsplit, cdiv(tiles_total, nsplit), outer_tiles, 0, vec,
               out_cols, stride, nsplit * stride * 4 if nsplit > 1 else 0, old_reduce(nsplit, outer_n, cols_alloc, out_cols),
               planes=planes)


def old_tall(s, kn, outer_n, red_n, cb):
    """launch_tall: None when the register-resident kernels do not serve the product"""
    esz = s["esz"]
    kmax, kvec = (96 if esz == 4 else 64), 16 // esz
    if kn["tall_min_rows"] <= 0:
        return None
    if s["tn"]:
        m, kdim, n2 = outer_n, red_n, s["x_cols"]
        if kdim > kmax or n2 > kmax or m < kn["tall_min_rows"] or s["r_rows"] != kdim:
            return None
        if s["r_ld"] < round_up(m, 64) or s["r_ld"] % kvec or not s["r_aligned"]:
            return None
        if s["x_external"] or s["x_ld"] < kdim:
            return None
        if s["out_rows"] != m or s["out_ld"] < m or s["out_cols"] < n2:
            return "reject internal: gemm output shape mismatch"
        kt = max(cdiv(kdim, 16), cdiv(n2, 16))
        out_cols = s["out_cols"] if s["out_external"] else min(s["out_cols_alloc"], 16 * kt)
        vec = int(s["out_ld"] % kvec == 0 and s["out_aligned"])
        grid = min(cdiv(cdiv(m, 16 * kvec), 4), s["num_cus"])
        return fmt("tall_apply", [], 256, [(grid, 1, 1, kt, 0, 0, 0)], vec_store=vec, out_cols=out_cols)
    l, m = outer_n, red_n
    if not s["same"] or s["r_ld"] != s["x_ld"] or l != s["x_cols"] or l > kmax or m < kn["tall_min_rows"]:
        return None
    if s["r_ld"] % kvec or not s["r_aligned"] or s["x_external"] or s["out_external"]:
        return None
    nct = cdiv(l, 16)
    if s["out_ld"] < 16 * nct or s["out_cols_alloc"] < 16 * nct or cb[3] < 16 * nct:
        return None
    if s["out_rows"] != l:
        return "reject internal: gemm output shape mismatch"
    krows = 512 // esz
    rows = s["x_ld"]
    want = max(1, min(s["num_cus"], rows // (4 * krows)))
    rpg = round_up(cdiv(rows, want), krows)
    ngroups = cdiv(rows, rpg)
    stride = s["out_ld"] * s["out_cols_alloc"]
    return fmt("tall_gram", [], 256, [(ngroups, 1, 1, nct, 0, 0, gram_lds(nct, esz))], slab_stride=stride,
               slab_bytes=ngroups * stride * esz, reduce=("deep", cdiv(l, 64), 16 * nct, ngroups, l, 16 * nct), rpg=rpg,
               groups=ngroups)


def old_geometry(s, kn, outer_n, nblk, tiles_total):
    """choose_geometry"""
    ov = kn["split_tn"] if s["tn"] else kn["split_nn"]
    mw = 2 if (outer_n >= 256 and tiles_total >= 8) else 1
    if kn["mw"] > 0:
        mw = kn["mw"]
    wgs = cdiv(outer_n, 64 * mw) * nblk
    ns = 1
    if ov > 0:
        ns = ov
    elif wgs < s["num_cus"]:
        ns = cdiv(s["num_cus"], wgs)
        if wgs * ns < 2 * s["num_cus"] and wgs < s["num_cus"] // 4:
            ns *= 2
        ns = min(ns, max(1, tiles_total // 4))
    ns = max(1, min(ns, tiles_total))
    return mw, min(ns, 65535)


def old_plan(s, kn):
    tn, esz = s["tn"], s["esz"]
    outer_n, red_n = (s["r_cols"], s["r_rows"]) if tn else (s["r_rows"], s["r_cols"])
    if s["np"]:
        return old_mixed(s, kn, outer_n, red_n)
    kt_, vec_ = (64, 4) if esz == 4 else (32, 2)
    cb = col_blocking(s["x_cols"])
    tiles, nblk, nt, cols_alloc = cb
    if s["x_external"]:
        return "reject internal: an external buffer cannot be a padded operand"
    if (cols_alloc > s["x_cols_alloc"] or (not s["out_external"] and cols_alloc > s["out_cols_alloc"]) or
            (s["out_external"] and s["out_cols"] < s["x_cols"])):
        return "reject internal: skinny column padding too small for the column blocking"
    if s["out_rows"] != outer_n or s["out_ld"] < outer_n:
        return "reject internal: gemm output shape mismatch"
    if not s["r_aligned"] or s["r_ld"] % vec_ or s["r_cols_readable"] % vec_ or not s["x_aligned"]:
        return "reject internal: operand not 16-byte vector aligned"
    tall = old_tall(s, kn, outer_n, red_n, cb)
    if tall:
        return tall
    tiles_total = cdiv(red_n, kt_)
    if s["x_ld"] < tiles_total * kt_:
        return "reject internal: skinny leading dimension too small"
    n_wide = tiles - nblk * (nt - 1)
    uneven0 = (nblk > 1 and n_wide < nblk and nt >= 2 and not kn["even_blocks"] and
               float(outer_n) * float(red_n) * float(cols_alloc) >= 1.0e10)
    mw, nsplit = old_geometry(s, kn, outer_n, max(1, min(n_wide, nblk - n_wide)) if uneven0 else nblk, tiles_total)
    alias = (not tn and s["same"] and s["r_ld"] == s["x_ld"] and nblk == 1 and outer_n <= 128 and nt <= 8 and
             outer_n == s["x_cols"] and not kn["no_gram_alias"])
    if alias:
        mw = 2
        nsplit = min(max(1, tiles_total // 4), 2 * s["num_cus"])
        if kn["split_nn"] > 0:
            nsplit = min(kn["split_nn"], tiles_total)
    outer_tiles = cdiv(outer_n, 64 * mw)
    uneven = not alias and uneven0
    out_cols = s["out_cols"] if s["out_external"] else (tiles * 16 if uneven else cols_alloc)
    tps = cdiv(tiles_total, nsplit)
    stride = s["out_ld"] * cols_alloc
    vec = int(s["out_ld"] % 4 == 0 and s["out_aligned"])
    rotate = int(not tn and not alias and 1 < tps <= 32 and not kn["no_rotate"])
    gx = outer_tiles
    if not alias and tps <= kn["persist_max_tiles"]:
        lds_full = gemm_stages(mw, nt) * stage_bytes(mw, nt)
        per_cu = max(1, min(4, (160 * 1024) // lds_full))
        slots = per_cu * s["num_cus"] // (nblk * nsplit)
        if slots >= 1 and outer_tiles >= 3 * slots:
            gx = slots
    if nblk > 65535 or nsplit > 65535:
        return "reject problem too large for the launch grid"

    def xcd_ok(gy):
        return int(tn and kn["xcd_remap"] != 0 and gy == 1 and gx == outer_tiles and 2 <= outer_tiles <= 32 and nsplit >= 8)

    # launch_mw / launch_one / launch_alias
    if alias:
        kmw, knw = 2, 4
    elif mw == 2:
        kmw, knw = (1, 8) if (esz == 8 and kn["f64_waves"] == 8) else (2, 4)
    else:
        kmw, knw = 1, 4

    def lds(ntl):
        if alias:
            return 3 * 64 * 256 * 2
        gw = kmw * knw // 4
        per_wg = max(1, tps) * cdiv(outer_tiles, gx)
        return min(gemm_stages(gw, ntl), per_wg) * stage_bytes(gw, ntl)

    if uneven:
        launches = [(gx, n_wide, nsplit, nt, 0, xcd_ok(n_wide), lds(nt)),
                    (gx, nblk - n_wide, nsplit, nt - 1, n_wide * nt * 16, xcd_ok(nblk - n_wide), lds(nt - 1))]
    else:
        launches = [(gx, nblk, nsplit, nt, 0, xcd_ok(nblk), lds(nt))]
    red = old_reduce(nsplit, outer_n, cols_alloc, out_cols)
    if red[2] > 65535:
        return "reject problem too large for the launch grid"
    return fmt("gram_alias" if alias else "general", [kmw, knw], 64 * (knw + 4), launches, tiles_total, nsplit, tps,
               outer_tiles, rotate, vec, out_cols, stride, nsplit * stride * esz if nsplit > 1 else 0, red)


MAIN = r"""
#include <cstdio>
#include "gemm_plan.hpp"
int main() {
  const char* fam[] = {"general", "gram_alias", "tall_apply", "tall_gram", "bf16_split"};
  const char* red[] = {"none", "plain", "deep"};
  long long v[21];
  corrla::GemmKnobs kn;
  long long ki[11];
  while (true) {
    for (int i = 0; i < 21; ++i)
      if (std::scanf("%lld", &v[i]) != 1) return 0;
    for (int i = 0; i < 7; ++i) std::scanf("%lld", &ki[i]);
    std::scanf("%lf", &kn.mixed_min_work);
    for (int i = 7; i < 11; ++i) std::scanf("%lld", &ki[i]);
    kn.split_nn = (int)ki[0], kn.split_tn = (int)ki[1], kn.mw = (int)ki[2], kn.xcd_remap = (int)ki[3];
    kn.tall_min_rows = ki[4], kn.persist_max_tiles = (int)ki[5], kn.f64_waves = (int)ki[6];
    kn.even_blocks = ki[7] != 0, kn.no_gram_alias = ki[8] != 0, kn.no_rotate = ki[9] != 0, kn.mixed_split = (int)ki[10];
    corrla::GemmShape s;
    s.tn = v[0] != 0, s.esz = (int)v[1], s.np = (int)v[19], s.num_cus = (int)v[20], s.same = v[18] != 0;
    s.r = {v[2], v[3], v[4], v[5], 0, false, v[6] != 0};
    s.x = {0, v[7], v[8], 0, v[9], v[10] != 0, v[11] != 0};
    s.out = {v[12], v[14], v[13], 0, v[15], v[16] != 0, v[17] != 0};
    const corrla::GemmPlan p = corrla::gemm_plan(s, kn);
    if (p.error) {
      std::printf("reject %s\n", p.error);
      continue;
    }
    std::printf("%s", fam[(int)p.family]);
    if (p.family == corrla::GemmFamily::general || p.family == corrla::GemmFamily::gram_alias) std::printf(" %d %d", p.mw, p.nw);
    if (p.family == corrla::GemmFamily::bf16_split) std::printf(" %d", p.np);
    std::printf(" %d %d", p.block, p.nlaunch);
    for (int i = 0; i < p.nlaunch; ++i) {
      const corrla::GemmLaunch& L = p.launch[i];
      std::printf(" %u %u %u %d %lld %d %d", L.grid[0], L.grid[1], L.grid[2], L.nt, (long long)L.col_base, L.xcd_remap, L.lds);
    }
    std::printf(" %d %d %d %d %d %d %lld %lld %zu", p.tiles_total, p.nsplit, p.tiles_per_split, p.outer_blocks, p.rotate,
                p.vec_store, (long long)p.out_cols, (long long)p.slab_stride, p.slab_bytes);
    std::printf(" %s %u %u %d %lld %lld", red[(int)p.reduce.kind], p.reduce.grid[0], p.reduce.grid[1], p.reduce.slabs,
                (long long)p.reduce.rows, (long long)p.reduce.cols);
    std::printf(" %lld %lld %lld %lld %zu %u\n", (long long)p.rows_per_group, (long long)p.groups, (long long)p.plane_stride,
                (long long)p.plane_cols, p.plane_bytes, p.split_grid);
  }
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gemm_plan")
    src = tmp / "plan.cpp"
    src.write_text(MAIN)
    exe = tmp / "plan"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "corrla_rs_amd", "csrc"),
                           str(src), "-o", str(exe)])

    def run(cases):
        inp = "".join(" ".join(str(int(s[n])) for n in SHAPE_NAMES) + " " +
                      " ".join(repr(float(k[n])) if n == "mixed_min_work" else str(int(k[n])) for n in KNOB_NAMES) + "\n"
                      for s, k in cases)
        out = subprocess.run([str(exe)], input=inp, capture_output=True, text=True, check=True).stdout
        return out.splitlines()
    return run


# ---- operands as the backend builds them (gemm_plan.hpp: skinny_layout, driver.hpp: as_rowmajor_transposed) ----
def skinny(rows, cols, external=False, aligned=True, ld=None):
    return dict(rows=rows, cols=cols, ld=ld if ld is not None else round_up(max(rows, 1), 64),
                cols_alloc=cols if external else col_blocking(cols)[3], external=external, aligned=aligned)


def big(rows, cols, ld=None, aligned=True):
    ld = ld if ld is not None else round_up(cols, 4)
    return dict(rows=rows, cols=cols, ld=ld, cols_readable=ld, aligned=aligned)


def transposed(y, ncols):
    return dict(rows=ncols, cols=y["rows"], ld=y["ld"], cols_readable=y["ld"], aligned=y["aligned"])


def shape(tn, esz, r, x, out, same=False, np_=0, num_cus=256):
    return dict(tn=int(tn), esz=esz, r_rows=r["rows"], r_cols=r["cols"], r_ld=r["ld"], r_cols_readable=r["cols_readable"],
                r_aligned=int(r["aligned"]), x_cols=x["cols"], x_ld=x["ld"], x_cols_alloc=x["cols_alloc"],
                x_external=int(x["external"]), x_aligned=int(x["aligned"]), out_rows=out["rows"], out_ld=out["ld"],
                out_cols=out["cols"], out_cols_alloc=out["cols_alloc"], out_external=int(out["external"]),
                out_aligned=int(out["aligned"]), same=int(same), np=np_, num_cus=num_cus)


def products(esz, m, n, l, num_cus, np_=0):
    """the products of one range-finder step on an m x n row-major A with l sketch columns"""
    a, om, y, z = big(m, n), skinny(n, l), skinny(m, l), skinny(n, l)
    mm = skinny(l, l)
    g = skinny(l, l)
    yt = transposed(y, l)
    return [
        shape(False, esz, a, om, y, np_=np_, num_cus=num_cus),    # Y = A Omega
        shape(True, esz, a, y, z, np_=np_, num_cus=num_cus),      # Z = A^T Y
        shape(False, esz, yt, y, g, same=True, num_cus=num_cus),  # G = Y^T Y
        shape(True, esz, yt, mm, dict(y, cols=l), num_cus=num_cus),  # Y <- Y M (apply_inplace)
    ]


def shapes(esz, num_cus):
    out = []
    # the bench configurations: C2 16384^2 f32 l = 138, C3 65536 x 4096 f64 l = 266, a C4 shard 1.25M x 512 f32 l = 74,
    # C5's RSVD of the 64 x 10^6 f64 gradient matrix with l = 42 (as its transpose)
    for m, n, l in ((16384, 16384, 138), (65536, 4096, 266), (1250000, 512, 74), (1000000, 64, 42)):
        out += products(esz, m, n, l, num_cus)
        if esz == 4:
            out += products(esz, m, n, l, num_cus, np_=3) + products(esz, m, n, l, num_cus, np_=2)
    # tall rows 65535 / 65536; l at the tall kernels' edge (96 / 97 f32, 64 / 65 f64); alias outer 128 / 129;
    # cols 144 / 145 / 266
    for m in (4096, 65535, 65536):
        for l in (16, 63, 64, 65, 96, 97, 128, 129, 144, 145, 266):
            out += products(esz, m, 512, l, num_cus)
    # an aliased operand whose leading dimension differs, and a Gram product of two different operands
    y = skinny(4096, 64)
    out.append(shape(False, esz, dict(transposed(y, 64), ld=y["ld"] + 64), y, skinny(64, 64), same=True, num_cus=num_cus))
    out.append(shape(False, esz, transposed(y, 64), y, skinny(64, 64), same=False, num_cus=num_cus))
    # the uneven blocking's threshold outer x red x cols_alloc = 1e10: exactly at l = 240 (15 tiles = 8 + 7, 256 columns),
    # between 34722222 and 34722223 at l = 266 (17 tiles = 9 + 8, 288 columns)
    for outer, red, l in ((39062499, 1, 240), (39062500, 1, 240), (17361111, 2, 266), (17361112, 2, 266), (34722222, 1, 266),
                          (34722223, 1, 266)):
        for tn in (False, True):
            r = big(red, outer) if tn else big(outer, red)
            out.append(shape(tn, esz, r, skinny(red, l), skinny(outer, l), num_cus=num_cus))
    # tiles per split around 16 / 17 (persistent) and 32 / 33 (rotate), long outer dimension
    kt = 64 if esz == 4 else 32
    for tiles in (2, 3, 8, 16, 17, 32, 33):
        for outer in (1 << 16, 1 << 20):
            for l in (64, 138):
                for tn in (False, True):
                    r = big(tiles * kt, outer) if tn else big(outer, tiles * kt)
                    out.append(shape(tn, esz, r, skinny(tiles * kt, l), skinny(outer, l), num_cus=num_cus))
    # XCD remap: 1 / 2 / 32 / 33 outer tiles with a long reduction
    for outer in (64, 128, 4096, 4224, 8192):
        for tn in (False, True):
            r = big(1 << 16, outer) if tn else big(outer, 1 << 16)
            out.append(shape(tn, esz, r, skinny(1 << 16, 80), skinny(outer, 80), num_cus=num_cus))
    # the bf16 split's domain: outer x red around 2^24, x.ld not a multiple of 64, unaligned, external, > 144 columns
    if esz == 4:
        for outer, red in ((4096, 4096), (4096, 4095), (100000, 64), (256, 1 << 20)):
            for tn in (False, True):
                for np_ in (2, 3):
                    r = big(red, outer) if tn else big(outer, red)
                    out.append(shape(tn, esz, r, skinny(red, 138), skinny(outer, 138), np_=np_, num_cus=num_cus))
                    out.append(shape(tn, esz, r, skinny(red, 138, ld=round_up(red, 32) + 32), skinny(outer, 138), np_=np_,
                                     num_cus=num_cus))
                    out.append(shape(tn, esz, r, skinny(red, 145), skinny(outer, 145), np_=np_, num_cus=num_cus))
                    out.append(shape(tn, esz, r, skinny(red, 74), skinny(outer, 74, external=True, ld=outer), np_=np_,
                                     num_cus=num_cus))
        out.append(shape(False, esz, big(4096, 4096), skinny(4096, 64), skinny(4096, 64), np_=1, num_cus=num_cus))
    # unaligned and external operands, short padding, wrong output shapes
    a = big(65536, 512)
    out += [
        shape(False, esz, dict(a, aligned=False), skinny(512, 64), skinny(65536, 64), num_cus=num_cus),
        shape(False, esz, dict(a, ld=514, cols_readable=514), skinny(512, 64), skinny(65536, 64), num_cus=num_cus),
        shape(False, esz, a, skinny(512, 64, aligned=False), skinny(65536, 64), num_cus=num_cus),
        shape(False, esz, a, skinny(512, 64), skinny(65536, 64, aligned=False), num_cus=num_cus),
        shape(False, esz, a, skinny(512, 64), skinny(65536, 64, ld=65538), num_cus=num_cus),
        shape(False, esz, a, skinny(512, 64, external=True), skinny(65536, 64), num_cus=num_cus),
        shape(False, esz, a, skinny(512, 70), skinny(65536, 64, external=True, ld=65536), num_cus=num_cus),
        shape(False, esz, a, skinny(512, 70), dict(skinny(65536, 70), cols_alloc=64), num_cus=num_cus),
        shape(False, esz, a, skinny(512, 64), skinny(65535, 64), num_cus=num_cus),
        shape(False, esz, a, skinny(256, 64), skinny(65536, 64), num_cus=num_cus),
        shape(True, esz, a, skinny(65536, 40), skinny(512, 40, external=True, ld=512), num_cus=num_cus),
    ]
    y = skinny(1 << 17, 40)
    out.append(shape(True, esz, transposed(y, 40), skinny(40, 40), dict(y, cols=40, external=True, cols_alloc=40), num_cus=num_cus))
    out.append(shape(True, esz, transposed(y, 40), skinny(40, 48), dict(y, cols=40, external=True, cols_alloc=40), num_cus=num_cus))
    out.append(shape(True, esz, dict(transposed(y, 40), aligned=False), skinny(40, 40), dict(y, cols=40), num_cus=num_cus))
    return out


KNOB_SETS = [{}, {"split_nn": 5}, {"split_tn": 9}, {"mw": 1}, {"mw": 2}, {"xcd_remap": 0}, {"tall_min_rows": 0},
             {"tall_min_rows": 1 << 20}, {"persist_max_tiles": 0}, {"persist_max_tiles": 40}, {"f64_waves": 4},
             {"mixed_min_work": 1.0}, {"even_blocks": 1}, {"no_gram_alias": 1}, {"no_rotate": 1}, {"mixed_split": 3},
             {"split_tn": 7}, {"split_tn": 8}]


@pytest.mark.parametrize("esz", [4, 8])
@pytest.mark.parametrize("num_cus", [256, 80])
def test_plan_matches_the_old_routing(plan, esz, num_cus):
    cases = [(s, dict(DEFAULT_KNOBS, **k)) for s, k in itertools.product(shapes(esz, num_cus), KNOB_SETS)]
    got = plan(cases)
    assert len(got) == len(cases)
    bad = [(s, k, g, e) for (s, k), g in zip(cases, got) for e in [old_plan(s, k)] if g != e]
    assert not bad, "%d of %d cases differ, first: %r" % (len(bad), len(cases), bad[0])


def test_every_family_and_boundary_is_reached(plan):
    """the table is not vacuous: every family, both reductions, an uneven blocking, XCD remap, rotation, persistence and
    rejections all occur under the default knobs"""
    cases = [(s, dict(DEFAULT_KNOBS)) for esz in (4, 8) for s in shapes(esz, 256)]
    got = plan(cases)
    fams = {g.split()[0] for g in got}
    assert fams == {"general", "gram_alias", "tall_apply", "tall_gram", "bf16_split", "reject"}
    general = [g.split() for g in got if g.startswith("general")]
    assert any(f[4] == "2" for f in general)                       # uneven blocking: two launches
    assert any(" deep " in g for g in got) and any(" plain " in g for g in got)
    assert any(f[10] == "1" for f in general)                      # XCD remap of the first launch
    assert any(f[5 + 7 * int(f[4]) + 4] == "1" for f in general)  # rotate
    assert any(int(f[5]) < int(f[5 + 7 * int(f[4]) + 3]) for f in general)  # persistent: fewer workgroups than tiles


# ---- the routes the GPU test runs (tests/test_gpu_gemm_routes.py) ------------------------------------------------------
# environment variable of each knob (hip_backend.hpp reads them when a context is created)
KNOB_ENV = {"CORRLA_SPLIT_NN": "split_nn", "CORRLA_SPLIT_TN": "split_tn", "CORRLA_MW": "mw", "CORRLA_GEMM_XCD": "xcd_remap",
            "CORRLA_TALL_MIN_ROWS": "tall_min_rows", "CORRLA_GEMM_PERSIST_TILES": "persist_max_tiles",
            "CORRLA_F64_WAVES": "f64_waves", "CORRLA_MIXED_MIN_WORK": "mixed_min_work", "CORRLA_EVEN_BLOCKS": "even_blocks",
            "CORRLA_NO_GRAM_ALIAS": "no_gram_alias", "CORRLA_GEMM_NO_ROTATE": "no_rotate", "CORRLA_MIXED_SPLIT": "mixed_split"}


def matmul_shape(esz, m, n, l, trans, num_cus=256):
    """The product of Context.matmul(a, x, trans) on a row-major m x n device matrix with l columns (capi_impl.hpp:
    stage_input, product_body): A is read in place when its rows are whole 16-byte vectors, else from a copy with a
    64-element leading dimension; the skinny operand and the result are padded work matrices."""
    a = big(m, n, ld=n if n % (16 // esz) == 0 else round_up(n, 64))
    xin, xout = (m, n) if trans else (n, m)
    return shape(trans, esz, a, skinny(xin, l), skinny(xout, l), num_cus=num_cus)


def parse(line):
    """a line of the printer (general / gram_alias) as a dict"""
    f = line.split()
    assert f[0] in ("general", "gram_alias"), line
    p = dict(family=f[0], mw=int(f[1]), nw=int(f[2]), block=int(f[3]), nlaunch=int(f[4]), launches=[])
    at = 5
    for _ in range(p["nlaunch"]):
        g = [int(v) for v in f[at:at + 7]]
        p["launches"].append(dict(grid=tuple(g[:3]), nt=g[3], col_base=g[4], xcd_remap=g[5], lds=g[6]))
        at += 7
    for name in ("tiles_total", "nsplit", "tiles_per_split", "outer_blocks", "rotate", "vec_store", "out_cols", "slab_stride",
                 "slab_bytes"):
        p[name] = int(f[at])
        at += 1
    p["reduce"] = f[at]
    return p


def reached(p):
    """what a plan reaches, in the words of the `expect` column of ROUTES"""
    gw = p["mw"] * p["nw"] // 4  # row tiles per SIMD: the LDS ring is sized for the 64 * gw outer tile
    ls = p["launches"]
    r = dict(family=p["family"], mw=p["mw"], nw=p["nw"], nt=tuple(g["nt"] for g in ls), nlaunch=p["nlaunch"], reduce=p["reduce"],
             persistent=ls[0]["grid"][0] < p["outer_blocks"], rotate=p["rotate"], xcd_remap=tuple(g["xcd_remap"] for g in ls),
             col_base=tuple(g["col_base"] for g in ls), nsplit=p["nsplit"], tiles_total=p["tiles_total"],
             tiles_per_split=p["tiles_per_split"], outer_blocks=p["outer_blocks"],
             empty_slabs=(p["nsplit"] * p["tiles_per_split"] - p["tiles_total"]) // max(1, p["tiles_per_split"]))
    if p["family"] == "general":
        r["stages"] = tuple(gemm_stages(gw, g["nt"]) for g in ls)
        r["short_ring"] = tuple(g["lds"] < gemm_stages(gw, g["nt"]) * stage_bytes(gw, g["nt"]) for g in ls)
    return r


def _expect(mw, nw, nt, reduce="none", persistent=False, rotate=0, xcd_remap=0, stages=None, short_ring=False, **more):
    """`expect` of a row: the instantiation, the NT / XCD remap / ring depth / shortened ring of each launch, the reduction
    kind, persistence and rotation; `more` names what a feature row is there for (nsplit, tiles_total, ...)"""
    nt = nt if isinstance(nt, tuple) else (nt,)
    per = lambda v: v if isinstance(v, tuple) else (v,) * len(nt)
    gw = mw * nw // 4
    return dict(more, family="general", mw=mw, nw=nw, nt=nt, nlaunch=len(nt), reduce=reduce, persistent=persistent, rotate=rotate,
                xcd_remap=per(xcd_remap), stages=per(stages) if stages else tuple(gemm_stages(gw, t) for t in nt),
                short_ring=per(short_ring))


EXPECT_KEYS = ("family", "mw", "nw", "nt", "nlaunch", "reduce", "persistent", "rotate", "xcd_remap", "stages", "short_ring")
F64_W4 = {"CORRLA_F64_WAVES": 4}


def _routes():
    """(name, esz, m, n, l, trans, knobs, expect): Context.matmul(a, x, trans) on a row-major m x n matrix, x with l columns.
    Ragged on purpose: l = 16 NT - 3 leaves 13 of 16 columns in the last column tile, and neither the outer nor the
    reduction dimension is a multiple of its tile."""
    rows = []
    for esz in (4, 8):
        for trans in (False, True):
            tag = "f%d-%s" % (8 * esz, "tn" if trans else "nn")
            for nt in range(1, 10):
                l = 16 * nt - 3
                # small: the 64-index tile on four waves, 3 / 4 outer tiles, 3 .. 7 reduction tiles, one slab
                rows.append(("small-%s-nt%d" % (tag, nt), esz, 150, 200, l, trans, {},
                             _expect(1, 4, nt, rotate=int(not trans), stages=3)))
                # mid: the 128-index tile (f32 MW 2; f64 eight waves, or MW 2 under CORRLA_F64_WAVES=4), 5 outer tiles,
                # the 3-stage ring up to NT = 5 and the 2-stage ring beyond, the plain reduction of 2 (f32) / 4 (f64) slabs
                wide = dict(reduce="plain", rotate=int(not trans), stages=3 if nt <= 5 else 2, nsplit=2 if esz == 4 else 4)
                rows.append(("mid-%s-nt%d" % (tag, nt), esz, 520, 520, l, trans, {},
                             _expect(2 if esz == 4 else 1, 4 if esz == 4 else 8, nt, **wide)))
                if esz == 8:
                    rows.append(("mid-w4-%s-nt%d" % (tag, nt), esz, 520, 520, l, trans, F64_W4, _expect(2, 4, nt, **wide)))
    for trans in (False, True):
        tag, rot = "tn" if trans else "nn", int(not trans)
        # uneven column blocking (outer x red x cols_alloc >= 1e10): the second launch runs NT - 1 from column n_wide * NT * 16
        rows += [
            ("uneven-f32-%s-9+8" % tag, 4, 6100, 6000, 266, trans, {},
             _expect(2, 4, (9, 8), reduce="deep", persistent=True, rotate=rot, stages=2, col_base=(0, 144), nsplit=12)),
            ("uneven-f64-%s-9+8" % tag, 8, 6100, 6000, 266, trans, {},
             _expect(1, 8, (9, 8), reduce="deep", persistent=True, rotate=rot, stages=2, col_base=(0, 144), nsplit=12)),
            # one product on a 2-stage and a 3-stage ring
            ("uneven-f32-%s-6+5" % tag, 4, 8000, 8000, 170, trans, {},
             _expect(2, 4, (6, 5), reduce="deep", persistent=True, rotate=rot, stages=(2, 3), col_base=(0, 96), nsplit=10)),
            ("uneven-f64-%s-7+6" % tag, 8, 7000, 7100, 200, trans, {},
             _expect(1, 8, (7, 6), reduce="deep", persistent=False, rotate=rot, stages=2, col_base=(0, 112), nsplit=10)),
        ]
    rows += [
        # persistent launches: fewer workgroups than outer tiles, the ring runs on across the tile boundaries
        ("persist-f32-nn", 4, 100037, 72, 13, False, {}, _expect(1, 4, 1, persistent=True, rotate=1, outer_blocks=1564)),
        ("persist-f64-nn", 8, 100037, 72, 141, False, {}, _expect(1, 4, 9, persistent=True, rotate=1, outer_blocks=1564)),
        ("persist-f32-nn-wide", 4, 99000, 520, 141, False, {}, _expect(2, 4, 9, persistent=True, rotate=1, outer_blocks=774)),
        # 100 rows, not 72: on 96 or fewer rows A^T Y with 100037 outer indices belongs to the register-resident kernels
        ("persist-f32-tn", 4, 100, 100037, 29, True, {}, _expect(1, 4, 2, persistent=True, outer_blocks=1564)),
        # persistent and deep reduction together: 65 tiles in 64 slabs of 2, so 31 slabs have no tile at all
        ("persist-deep-f32-nn", 4, 1600, 4100, 61, False, {"CORRLA_SPLIT_NN": 64},
         _expect(2, 4, 4, reduce="deep", persistent=True, rotate=1, nsplit=64, tiles_total=65, tiles_per_split=2, empty_slabs=31)),
        # XCD remap: 9 outer tiles x 58 slabs; 3 outer tiles x 11 slabs (neither a multiple of 8)
        ("xcd-f64-tn", 8, 30000, 1100, 141, True, {},
         _expect(1, 8, 9, reduce="deep", xcd_remap=1, nsplit=58, outer_blocks=9, empty_slabs=2)),
        ("xcd-f32-tn", 4, 40000, 190, 77, True, {"CORRLA_SPLIT_TN": 11},
         _expect(1, 4, 5, reduce="deep", xcd_remap=1, nsplit=11, outer_blocks=3)),
        # an nn product that does not rotate although its workgroups walk many tiles (more than 32 per split)
        ("norotate-f32-nn", 4, 300, 2200, 45, False, {"CORRLA_SPLIT_NN": 1}, _expect(2, 4, 3, tiles_per_split=35, nsplit=1)),
        ("norotate-f64-nn", 8, 300, 1100, 45, False, {"CORRLA_SPLIT_NN": 1}, _expect(1, 8, 3, tiles_per_split=35, nsplit=1)),
        # a split whose last slabs are empty: 79 tiles in 19 slabs of 5 (3 empty), 157 in 39 of 5 (7 empty)
        ("emptyslab-f32-tn", 4, 5000, 36, 74, True, {}, _expect(1, 4, 5, reduce="deep", nsplit=19, tiles_per_split=5, empty_slabs=3)),
        ("emptyslab-f64-tn", 8, 5000, 36, 74, True, {}, _expect(1, 4, 5, reduce="deep", nsplit=39, tiles_per_split=5, empty_slabs=7)),
        # one reduction tile, unsplit: the launch asks for one slot of the ring
        ("onetile-f32-nn", 4, 150, 60, 13, False, {}, _expect(1, 4, 1, short_ring=True, tiles_total=1, nsplit=1)),
        ("onetile-f64-nn", 8, 150, 30, 13, False, {}, _expect(1, 4, 1, short_ring=True, tiles_total=1, nsplit=1)),
        ("onetile-f32-tn", 4, 60, 150, 13, True, {}, _expect(1, 4, 1, short_ring=True, tiles_total=1, nsplit=1)),
        ("onetile-f64-tn", 8, 30, 150, 13, True, {}, _expect(1, 4, 1, short_ring=True, tiles_total=1, nsplit=1)),
        # two reduction tiles: two slots of the 3-stage ring, and the rotation starts half the workgroups on the second
        ("twotiles-f32-nn", 4, 150, 100, 29, False, {}, _expect(1, 4, 2, rotate=1, short_ring=True, tiles_total=2)),
        ("twotiles-f64-nn", 8, 150, 50, 29, False, {}, _expect(1, 4, 2, rotate=1, short_ring=True, tiles_total=2)),
    ]
    return rows


ROUTES = _routes()

# (name, esz, rows, l, knobs, expect): G = Y^T Y of the rows x l sketch of power_iter (the third of products()); the aliased
# instantiations gemm_nn_kernel<T, 2, NT, true> by default, the general kernels under CORRLA_NO_GRAM_ALIAS=1
GRAM_ROWS, GRAM_COLS = 700, 150
GRAM_ROUTES = [("gram-f%d-nt%d-%s" % (8 * esz, nt, "general" if knobs else "alias"), esz, GRAM_ROWS, 16 * nt - 3, knobs,
                dict(family="general", mw=1, nw=4, nt=(nt,)) if knobs else dict(family="gram_alias", mw=2, nw=4, nt=(nt,)))
               for esz in (4, 8) for nt in range(1, 9) for knobs in ({}, {"CORRLA_NO_GRAM_ALIAS": 1})]

# (name, family, m, n, l, trans, np, knobs, expect): Context.matmul(a, x, trans) on a row-major m x n matrix -- f32 under
# CORRLA_SKETCH_MIXED=bf16x3 / bf16x6 (np 2 / 3) for the bf16 split, a bfloat16 tensor for the bf16-stored kernel -- x with
# l = 16 NT - 3 columns.  300 x 72: outer and reduction tails in both orientations, and a row of 72 elements is whole 16-byte
# vectors in either type, so both kernels read the matrix in place.
PLANE_M, PLANE_N = 300, 72
PLANE_MODES = {2: "bf16x3", 3: "bf16x6"}
PLANE_ROUTES = (
    [("split-np%d-%s-nt%d" % (np_, "tn" if trans else "nn", nt), "bf16_split", PLANE_M, PLANE_N, 16 * nt - 3, trans, np_,
      {"CORRLA_MIXED_MIN_WORK": 1}, dict(family="bf16_split", nt=nt, np=np_, tn=trans))
     for np_ in (2, 3) for trans in (False, True) for nt in range(1, 10)] +
    [("stored-%s-nt%d" % ("tn" if trans else "nn", nt), "bf16_stored", PLANE_M, PLANE_N, 16 * nt - 3, trans, 0, {},
      dict(family="bf16_stored", nt=nt, np=3, tn=trans))
     for trans in (False, True) for nt in range(1, 10)])

# (name, m, n, k, p, q, expect): rsvd(a, k, q, p, fused=True) on a row-major f32 m x n matrix; the sketch has l = k + p =
# 16 NCT - 3 columns and the one-sweep kernel runs on ata_fused_kernel<NK, NCT>, NK by n: 2 (<= 128), 4 (<= 256), 8
ATA_M = 4100
ATA_ROUTES = [("ata-nk%d-nct%d" % (nk, nct), ATA_M, n, 16 * nct - 3 - 5, 5, 1, dict(nk=nk, nct=nct))
              for nk, n in ((2, 100), (4, 200), (8, 300)) for nct in range(1, 6)]

# what the table must reach besides every instantiation, in the element types named
FEATURES = {
    "3-stage ring of the 128-index tile": ((4, 8), lambda row, r: r["mw"] * r["nw"] == 8 and 3 in r["stages"]),
    "2-stage ring of the 128-index tile": ((4, 8), lambda row, r: r["mw"] * r["nw"] == 8 and 2 in r["stages"]),
    "a 2-stage and a 3-stage launch in one product": ((4,), lambda row, r: r["stages"] == (2, 3)),
    "shortened ring": ((4, 8), lambda row, r: any(r["short_ring"])),
    "uneven blocking, nn": ((4, 8), lambda row, r: not row[5] and r["nlaunch"] == 2 and r["col_base"][1] != 0),
    "uneven blocking, tn": ((4, 8), lambda row, r: row[5] and r["nlaunch"] == 2 and r["col_base"][1] != 0),
    "uneven blocking, not persistent": ((8,), lambda row, r: r["nlaunch"] == 2 and not r["persistent"]),
    "persistent, nn": ((4, 8), lambda row, r: not row[5] and r["persistent"]),
    "persistent, tn": ((4, 8), lambda row, r: row[5] and r["persistent"]),
    "persistent on the 128-index tile, one launch": ((4,), lambda row, r: r["persistent"] and r["mw"] == 2 and r["nlaunch"] == 1),
    "persistent with the deep reduction": ((4, 8), lambda row, r: r["persistent"] and r["reduce"] == "deep"),
    "no reduction": ((4, 8), lambda row, r: r["reduce"] == "none"),
    "plain reduction": ((4, 8), lambda row, r: r["reduce"] == "plain"),
    "deep reduction": ((4, 8), lambda row, r: r["reduce"] == "deep"),
    "XCD remap": ((4, 8), lambda row, r: any(r["xcd_remap"])),
    "XCD remap, outer tiles and slabs no multiples of 8": ((4, 8), lambda row, r: any(r["xcd_remap"]) and r["outer_blocks"] % 8 and r["nsplit"] % 8),
    "rotation": ((4, 8), lambda row, r: r["rotate"] == 1),
    "nn without rotation on more than one tile per split": ((4, 8), lambda row, r: not row[5] and not r["rotate"] and r["tiles_per_split"] > 1),
    "empty last slabs": ((4, 8), lambda row, r: r["empty_slabs"] >= 1),
    "one tile, unsplit": ((4, 8), lambda row, r: r["tiles_total"] == 1 and r["nsplit"] == 1),
}


def route_a(i, j):
    """Integer test operand A[i, j] in [-3, 3] (i and j: integer index arrays that broadcast, numpy or torch): not
    symmetric, and row i differs from rows i + 64 and i + 128 -- and column j from columns j + 64 and j + 128 -- in most
    entries, so a result computed from the neighbouring 64-index tile cannot pass."""
    return (3 * i + j + (i * j) % 1013 + (i // 64) * (j % 5)) % 7 - 3


def route_x(r, c):
    """Integer skinny operand X[r, c] in [-4, 4]: every column differs from every other within the first 16 rows."""
    return ((r + 1) * (c + 1) + (r // 3) * (c // 7) + (r // 5) * (c // 63) + c // 9) % 9 - 4


def _plans(plan, table, shape_of):
    cases = [(shape_of(row), dict(DEFAULT_KNOBS, **{KNOB_ENV[k]: v for k, v in row[-2].items()})) for row in table]
    got = plan(cases)
    assert len(got) == len(table)
    return [reached(parse(g)) for g in got]


def _route_plans(plan):
    return _plans(plan, ROUTES, lambda row: matmul_shape(*row[1:6]))


def _gram_plans(plan):
    return _plans(plan, GRAM_ROUTES, lambda row: products(row[1], row[2], GRAM_COLS, row[3], 256)[2])


def test_every_route_reaches_what_it_names(plan):
    for table, plans in ((ROUTES, _route_plans(plan)), (GRAM_ROUTES, _gram_plans(plan))):
        assert len({row[0] for row in table}) == len(table)
        for row, r in zip(table, plans):
            expect = row[-1]
            if table is ROUTES:
                assert set(EXPECT_KEYS) <= set(expect), row[0]
                assert 12 * max(row[2], row[3]) < 1 << 24, row[0]             # the GPU test's integer sums are exact in f32
                # operand bytes: "about 300 MB", with room for the largest shape first proposed, 7000 x 7100 in f64 (398 MB)
                assert row[1] * row[2] * row[3] <= 400e6, row[0]
            assert {k: r[k] for k in expect} == expect, (row[0], r)


def test_the_route_table_is_complete(plan):
    """every instantiation the `general` launcher can dispatch, alias included (tall_stage.hpp), every feature in FEATURES"""
    plans = _route_plans(plan)
    seen = {(row[1], bool(row[5]), r["mw"], r["nw"], nt) for row, r in zip(ROUTES, plans) for nt in r["nt"]}
    # gemm_general_exists (gemm_plan.hpp): NW == 4 || (NW == 8 && MW == 1 && T is double), NT 1 .. kMaxColTiles, nn and tn;
    # tests/test_tall_stage_plan.py counts the same 90 from the predicate itself
    want = {(esz, tn, mw, nw, nt) for esz in (4, 8) for tn in (False, True) for mw in (1, 2) for nw in (4, 8)
            if nw == 4 or (nw == 8 and mw == 1 and esz == 8) for nt in range(1, 10)}
    assert len(want) == 90
    assert not want - seen, sorted(want - seen)
    assert not seen - want, sorted(seen - want)
    for name, (types, hit) in FEATURES.items():
        for esz in types:
            assert any(row[1] == esz and hit(row, r) for row, r in zip(ROUTES, plans)), (name, esz)
    gram = _gram_plans(plan)
    alias = {(row[1], r["nt"][0]) for row, r in zip(GRAM_ROUTES, gram) if r["family"] == "gram_alias"}
    assert alias == {(esz, nt) for esz in (4, 8) for nt in range(1, 9)}   # gemm_nn_kernel<T, 2, NT, true>, NT 1 .. 8
    # ... and each has its twin on the general kernels, which the route table above covers
    twins = {(row[1], r["mw"], r["nw"], r["nt"][0]) for row, r in zip(GRAM_ROUTES, gram) if r["family"] == "general"}
    assert {(e, nt) for e, _, _, nt in twins} == alias
    assert {(e, False, mw, nw, nt) for e, mw, nw, nt in twins} <= seen


def test_route_knobs_are_the_ones_a_context_reads():
    import re
    src = open(os.path.join(ROOT, "corrla_rs_amd", "csrc", "hip_backend.hpp")).read()
    # a statement that assigns a knob names the variable it reads, before (getenv) or after (env_int) the assignment
    read = {}
    for stmt in src.split(";"):
        knob, env = re.search(r"gemm_knobs_\.(\w+)\s*=[^=]", stmt), re.findall(r'"(CORRLA_\w+)"', stmt)
        if knob and len(env) == 1:
            read[env[0]] = knob.group(1)
    assert read == KNOB_ENV
    assert set(KNOB_ENV.values()) == set(KNOB_NAMES)


def test_route_operands_tell_tiles_and_columns_apart():
    """the integer operands of the GPU test: value ranges, distinct columns of X within the shortest reduction, rows and
    columns of A 64 and 128 apart that differ in most of the entries the shortest reduction of the table reads"""
    import numpy as np
    red = min(row[2] if row[5] else row[3] for row in ROUTES)
    lmax = max(row[4] for row in ROUTES)
    assert red >= 16  # route_x tells its columns apart within 16 rows
    i, j = np.arange(1100)[:, None], np.arange(1100)[None, :]
    a = route_a(i, j)
    assert a.min() == -3 and a.max() == 3 and np.mean(a != a.T) > 0.8
    for d in (64, 128):
        assert np.mean(a[:-d, :red] != a[d:, :red], axis=1).min() > 0.5
        assert np.mean(a[:red, :-d] != a[:red, d:], axis=0).min() > 0.5
    x = route_x(np.arange(16)[:, None], np.arange(lmax)[None, :])
    assert x.min() == -4 and x.max() == 4
    assert len({tuple(col) for col in x.T}) == lmax
