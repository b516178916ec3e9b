"""The rest of the tall products' launch arithmetic (corrla_rs_amd/csrc/gemm_plan.hpp: ata_plan, spmm_plan, skinny_layout,
gemm_bf16a_call_domain and the lists of instantiations), pinned on the CPU: host code, compiled here with the host compiler
as tests/test_gemm_plan.py does.

old_ata / old_spmm / old_bf16a_fits below restate the arithmetic HipDev::ata_fused, ata_fused_fits, HipDev::spmm and
HipDev::bf16a_fits computed inline in hip_backend.hpp before these plans existed; every field of a plan, or its rejection
with its message, must equal them.  PLANE_ROUTES / ATA_ROUTES (tests/test_gemm_plan.py) are the calls of
tests/test_gpu_tall_routes.py: pinned here that every row's plan reaches the instantiation the row names, that the rows cover
every instantiation of the three families, and that the lists the launchers dispatch on are the lists the LDS registration
walks."""
import itertools
import os
import re
import subprocess

import pytest

from tests.test_gemm_plan import ATA_ROUTES, PLANE_ROUTES, cdiv, col_blocking, round_up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "corrla_rs_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <cstring>
#include "gemm_plan.hpp"
using namespace corrla;
static const char* red[] = {"none", "plain", "deep"};
static const char* fam[] = {"general", "gram_alias", "tall_apply", "tall_gram", "bf16_split", "bf16_stored"};
template <int... Vs>
static void print_list(std::integer_sequence<int, Vs...>) {
  ((std::printf(" %d", Vs)), ...);
}
int main() {
  char what[16];
  long long v[16];
  auto read = [&](int n) {
    for (int i = 0; i < n; ++i)
      if (std::scanf("%lld", &v[i]) != 1) return false;
    return true;
  };
  while (std::scanf("%15s", what) == 1) {
    if (!std::strcmp(what, "ata")) {
      // esz rows n ld readable aligned | l x_rows x_ld x_cols_alloc | z_rows z_ld z_cols_alloc | num_cus
      if (!read(14)) return 1;
      const GemmOperand a{v[1], v[2], v[3], v[4], 0, false, v[5] != 0};
      const GemmOperand x{v[7], v[6], v[8], 0, v[9], false, true}, z{v[10], v[6], v[11], 0, v[12], false, true};
      const AtaPlan p = ata_plan((int)v[0], a, x, z, (int)v[13]);
      std::printf("%d ", (p.in_domain ? 1 : 0) + (ata_domain((int)v[0], v[1], v[2], v[6]) ? 2 : 0));
      if (p.error) {
        std::printf("reject %s\n", p.error);
        continue;
      }
      std::printf("%d %d %d %d %d %lld %lld %zu %s %u %u %d %lld %lld\n", p.nk, p.nct, p.nrg, p.block, p.lds, (long long)p.rows_per_group,
                  (long long)p.slab_stride, p.slab_bytes, red[(int)p.reduce.kind], p.reduce.grid[0], p.reduce.grid[1], p.reduce.slabs,
                  (long long)p.reduce.rows, (long long)p.reduce.cols);
    } else if (!std::strcmp(what, "spmm")) {
      // esz rows cols L n_long n_chunks
      if (!read(6)) return 1;
      const SpmmPlan p = spmm_plan((int)v[0], v[1], v[2], v[3], v[4], v[5]);
      if (p.error) {
        std::printf("reject %s\n", p.error);
        continue;
      }
      std::printf("%lld %lld %lld %zu %zu %u %u %u %u %u %u %u %u\n", (long long)p.Lp, (long long)p.jt, (long long)p.Lpart, p.xt_bytes,
                  p.scratch_bytes, p.grid_xt[0], p.grid_xt[1], p.grid_rows[0], p.grid_rows[1], p.grid_long_partial[0],
                  p.grid_long_partial[1], p.grid_long_reduce[0], p.grid_long_reduce[1]);
    } else if (!std::strcmp(what, "layout")) {
      if (!read(2)) return 1;
      const SkinnyLayout l = skinny_layout(v[0], v[1]);
      std::printf("%lld %lld\n", (long long)l.ld, (long long)l.cols_alloc);
    } else if (!std::strcmp(what, "bf16a")) {
      // rows cols ld readable aligned l
      if (!read(6)) return 1;
      std::printf("%d\n", gemm_bf16a_call_domain({v[0], v[1], v[2], v[3], 0, false, v[4] != 0}, v[5], 256) ? 1 : 0);
    } else if (!std::strcmp(what, "route")) {
      // tn m n l np bf16: Context.matmul on a row-major m x n matrix read in place, the skinny operands as allocated
      if (!read(6)) return 1;
      GemmShape s;
      s.tn = v[0] != 0, s.np = (int)v[4], s.r_bf16 = v[5] != 0;
      const long long red_n = s.tn ? v[1] : v[2], outer_n = s.tn ? v[2] : v[1];
      const SkinnyLayout lx = skinny_layout(red_n, v[3]), lo = skinny_layout(outer_n, v[3]);
      s.r = {v[1], v[2], v[2], v[2], 0, false, true};
      s.x = {red_n, v[3], lx.ld, 0, lx.cols_alloc, false, true};
      s.out = {outer_n, v[3], lo.ld, 0, lo.cols_alloc, false, true};
      GemmKnobs kn;
      kn.mixed_min_work = 1.0;
      const GemmPlan p = gemm_plan(s, kn);
      if (p.error) {
        std::printf("reject %s\n", p.error);
        continue;
      }
      std::printf("%s %d %d %d %d\n", fam[(int)p.family], p.launch[0].nt, p.np, p.nlaunch, p.launch[0].lds);
    } else if (!std::strcmp(what, "counts")) {
      for (int esz = 4; esz <= 8; esz += 4) {
        int n = 0;
        for (int mw = 0; mw < 4; ++mw)
          for (int nt = 0; nt < 12; ++nt)
            for (int nw = 0; nw < 17; ++nw) n += gemm_general_exists(esz, mw, nt, nw) ? 2 : 0;  // nn and tn
        std::printf("general%d %d\n", esz, n);
        std::printf("tall%d %d\n", esz, tall_max_tiles(esz));
      }
      std::printf("alias %d\n", kAliasMaxTiles);
      std::printf("col_tiles %d\n", kMaxColTiles);
      std::printf("planes %d %d %d\n", kMxMinPlanes, kMxMaxPlanes, k::kBaPlanes);
      std::printf("ata_nct %d\n", kAtaMaxColTiles);
      std::printf("ata_nk");
      print_list(AtaNKs{});
      std::printf("\ngeneral_nw");
      print_list(GeneralNWs{});
      std::printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tall_stage_plan")
    src = tmp / "plan.cpp"
    src.write_text(MAIN)
    exe = tmp / "plan"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)])

    def run(lines):
        out = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout
        return out.splitlines()
    return run


# ---- the one-sweep A^T (A Z): HipDev::ata_fused and ata_fused_fits as they were ----------------------------------------
def ata_case(rows, n, l, num_cus=256, esz=4, **over):
    """operands as the driver passes them: a row-major rows x n matrix read in place, Omega / Z and Z' as alloc_skinny makes
    them; `over` breaks one property"""
    ld = round_up(n, 4)
    c = dict(esz=esz, rows=rows, n=n, ld=ld, readable=ld, aligned=1, l=l, x_rows=n, x_ld=round_up(max(n, 1), 64),
             x_cols_alloc=col_blocking(l)[3], z_rows=n, z_ld=round_up(max(n, 1), 64), z_cols_alloc=col_blocking(l)[3], num_cus=num_cus)
    c.update(over)
    return c


ATA_FIELDS = ("esz", "rows", "n", "ld", "readable", "aligned", "l", "x_rows", "x_ld", "x_cols_alloc", "z_rows", "z_ld",
              "z_cols_alloc", "num_cus")


def ata_lds(nk, nct):
    tile, tpart = 16 * nk * 256, 2 * 4 * nct * 1024
    return min(4, (160 * 1024 - tpart) // tile) * tile + tpart


def old_ata(c):
    fits = c["esz"] == 4 and c["n"] <= 512 and c["n"] >= 16 and c["l"] <= 80 and c["rows"] >= 4096
    head = "%d " % (3 if fits else 0)  # the plan's in_domain and ata_domain are the one predicate
    if c["esz"] != 4:
        return head + "reject internal: the one-sweep power iteration is f32 only"
    if c["x_rows"] != c["n"] or c["z_rows"] != c["n"]:
        return head + "reject ata_fused: shapes"
    cols_alloc = col_blocking(c["l"])[3]
    if cols_alloc > c["x_cols_alloc"] or cols_alloc > c["z_cols_alloc"] or c["x_ld"] != c["z_ld"] or cols_alloc > 80:
        return head + "reject internal: ata_fused operands must share the padded layout (<= 80 columns)"
    if not c["aligned"] or c["ld"] % 4 or c["readable"] % 4:
        return head + "reject internal: operand not vector aligned"
    nk = 2 if c["n"] <= 128 else (4 if c["n"] <= 256 else 8)
    nct = cols_alloc // 16
    blocks = cdiv(c["rows"], 16)
    nrg = max(1, min(c["num_cus"], blocks // 8))
    rpg = cdiv(blocks, nrg) * 16
    stride = c["z_ld"] * cols_alloc
    return head + " ".join(str(v) for v in (nk, nct, nrg, 256, ata_lds(nk, nct), rpg, stride, nrg * stride * 4, "deep",
                                            cdiv(c["n"], 64), cols_alloc, nrg, c["n"], cols_alloc))


ATA_ROWS = (4095, 4096, 4100, 65536, 10 ** 7)
ATA_NS = (15, 16, 100, 128, 129, 256, 257, 300, 512, 513)


def ata_cases():
    out = [ata_case(rows, n, l, cus) for rows, n, l, cus in itertools.product(ATA_ROWS, ATA_NS, range(1, 82), (256, 80))]
    for rows, n, l in ((4100, 100, 77), (65536, 512, 80), (4096, 16, 1)):
        base = ata_case(rows, n, l)
        out += [
            ata_case(rows, n, l, esz=8),
            ata_case(rows, n, l, ld=base["ld"] + 2, readable=base["ld"] + 4),   # leading dimension
            ata_case(rows, n, l, ld=base["ld"] + 4, readable=base["ld"] + 2),   # readable row length
            ata_case(rows, n, l, ld=base["ld"] + 64, readable=base["ld"] + 64),  # valid: a padded row
            ata_case(rows, n, l, aligned=0),
            ata_case(rows, n, l, x_rows=n + 1),
            ata_case(rows, n, l, z_rows=n - 1),
            ata_case(rows, n, l, z_ld=base["z_ld"] + 64),
            ata_case(rows, n, l, x_cols_alloc=base["x_cols_alloc"] - 16),
            ata_case(rows, n, l, z_cols_alloc=base["z_cols_alloc"] - 16),
            ata_case(rows, n, l, x_cols_alloc=144, z_cols_alloc=144),           # valid: more padding than the blocking needs
        ]
    return out


def test_ata_plan_matches_the_inline_arithmetic(plan):
    cases = ata_cases()
    got = plan(["ata " + " ".join(str(int(c[f])) for f in ATA_FIELDS) for c in cases])
    assert len(got) == len(cases)
    bad = [(c, g, e) for c, g in zip(cases, got) for e in [old_ata(c)] if g != e]
    assert not bad, "%d of %d cases differ, first: %r" % (len(bad), len(cases), bad[0])
    # the table is not vacuous: every instantiation, every rejection, both sides of the domain
    seen = {tuple(g.split()[1:3]) for g in got if "reject" not in g}
    assert seen == {(str(nk), str(nct)) for nk in (2, 4, 8) for nct in range(1, 6)}
    assert len({g.split(" ", 2)[2] for g in got if "reject" in g}) == 4
    assert {g.split()[0] for g in got} == {"0", "3"}


def test_ata_plan_pins_a_few_values_by_hand(plan):
    """so that old_ata cannot drift with the header: a C4 shard (1.25e6 x 512, l = 74) by hand"""
    got = plan(["ata " + " ".join(str(int(ata_case(1250000, 512, 74)[f])) for f in ATA_FIELDS)])[0].split()
    # 78125 blocks of 16 rows on 256 workgroups of 306 blocks; 3 stages of 32 KiB + 40 KiB of partial tiles
    assert got == ["3", "8", "5", "256", "256", str(3 * 32768 + 40960), str(306 * 16), str(512 * 80), str(256 * 512 * 80 * 4), "deep",
                   "8", "80", "256", "512", "80"]


# ---- the CSR product: HipDev::spmm as it was ---------------------------------------------------------------------------
def old_spmm(esz, rows, cols, L, n_long, n_chunks):
    Lp, jt = round_up(L, 16), cdiv(L, 64)
    Lpart = jt * 64
    xt_bytes = round_up(cols * Lp * esz, 256)
    need = xt_bytes + n_chunks * Lpart * esz
    gx, gr = (cdiv(cols, 64), cdiv(Lp, 64)), (cdiv(rows, 64), jt)
    if gx[1] > 65535 or gr[1] > 65535:
        return "reject problem too large for the launch grid"
    return " ".join(str(v) for v in (Lp, jt, Lpart, xt_bytes, need) + gx + gr + (n_chunks, jt, n_long, jt))


def test_spmm_plan_matches_the_inline_arithmetic(plan):
    edge = 65535 * 64  # the widest sketch whose tiles fit the grid's y dimension
    cases = [(esz, rows, cols, L, n_long, n_chunks)
             for esz in (4, 8) for rows, cols in ((1000, 300), (1, 1), (5000000, 64), (65, 4097))
             for L in (1, 16, 17, 64, 65, 138, 300, edge - 1, edge, edge + 1, edge + 64) for n_long, n_chunks in ((0, 0), (3, 7), (1, 2000))]
    got = plan(["spmm " + " ".join(str(v) for v in c) for c in cases])
    assert len(got) == len(cases)
    bad = [(c, g, e) for c, g in zip(cases, got) for e in [old_spmm(*c)] if g != e]
    assert not bad, "%d of %d cases differ, first: %r" % (len(bad), len(cases), bad[0])
    assert any("reject" in g for g in got) and any(g.split()[1] == "65535" for g in got)
    # by hand: 300 columns of X in f32, L = 138 -> 144 floats per row of XT, three tiles of sketch columns
    assert plan(["spmm 4 1000 300 138 3 7"]) == ["144 3 192 %d %d 5 3 16 3 7 3 3 3" % (300 * 144 * 4, 300 * 144 * 4 + 7 * 192 * 4)]


# ---- the padded layout, and the once-per-call question of the bf16-stored route ----------------------------------------------
def test_skinny_layout_is_the_allocation_rule(plan):
    shapes = [(r, c) for r in (0, 1, 63, 64, 65, 4100, 10 ** 7) for c in (1, 16, 17, 144, 145, 266, 300)]
    got = plan(["layout %d %d" % s for s in shapes])
    assert got == ["%d %d" % (round_up(max(r, 1), 64), col_blocking(c)[3]) for r, c in shapes]


def old_bf16a_fits(rows, cols, ld, readable, aligned, l):
    """HipDev::bf16a_fits as it built its two shapes: gemm_bf16a_domain of R X and R^T X on freshly allocated skinny operands"""
    for tn in (False, True):
        xr, outr = (rows, cols) if tn else (cols, rows)
        x_ld, out_ld = round_up(max(xr, 1), 64), round_up(max(outr, 1), 64)
        ok = (col_blocking(l)[1] == 1 and aligned and ld % 8 == 0 and readable % 8 == 0 and x_ld % 64 == 0 and
              x_ld >= round_up(xr, 32) and out_ld >= outr and outr >= 1 and xr >= 1)
        if not ok:
            return 0
    return 1


def test_bf16a_call_domain_matches_the_hand_built_shapes(plan):
    cases = [(rows, cols, ld if ld else cols, rd if rd else cols, al, l)
             for rows, cols in ((300, 72), (4096, 1024), (1, 8), (33, 8), (300, 71), (0, 8))
             for ld, rd in ((0, 0), (1028, 1028), (1032, 1024), (1032, 1028)) for al in (1, 0) for l in (1, 138, 144, 145)]
    got = plan(["bf16a " + " ".join(str(v) for v in c) for c in cases])
    assert got == [str(old_bf16a_fits(*c)) for c in cases]
    assert set(got) == {"0", "1"}


# ---- the routes of tests/test_gpu_tall_routes.py -------------------------------------------------------------------------
def _counts(plan):
    return {f[0]: [int(v) for v in f[1:]] for f in (line.split() for line in plan(["counts"]))}


def test_every_plane_and_ata_route_reaches_what_it_names(plan):
    assert len(PLANE_ROUTES) == 36 + 18 and len({r[0] for r in PLANE_ROUTES}) == len(PLANE_ROUTES)
    got = plan(["route %d %d %d %d %d %d" % (r[5], r[2], r[3], r[4], r[6], r[1] == "bf16_stored") for r in PLANE_ROUTES])
    assert len(got) == len(PLANE_ROUTES)
    for row, g in zip(PLANE_ROUTES, got):
        name, family, m, n, l, trans, np_, knobs, expect = row
        f = g.split()
        assert dict(family=f[0], nt=int(f[1]), np=int(f[2]), tn=trans) == expect, (name, g)
        assert f[3] == "1" and expect["family"] == family
        assert l == 16 * expect["nt"] - 3 and n % 8 == 0 and 64 * max(m, n) < 1 << 24  # ragged; read in place; exact sums
        assert knobs == ({"CORRLA_MIXED_MIN_WORK": 1} if family == "bf16_split" else {})
    assert len(ATA_ROUTES) == 15 and len({r[0] for r in ATA_ROUTES}) == len(ATA_ROUTES)
    cases = [ata_case(m, n, k + p) for _, m, n, k, p, q, _ in ATA_ROUTES]
    got = plan(["ata " + " ".join(str(int(c[f])) for f in ATA_FIELDS) for c in cases])
    for row, c, g in zip(ATA_ROUTES, cases, got):
        name, m, n, k, p, q, expect = row
        f = g.split()
        assert f[0] == "3", (name, g)  # in the domain the driver asks for: the call takes the one-sweep kernel
        assert dict(nk=int(f[1]), nct=int(f[2])) == expect, (name, g)
        assert g == old_ata(c)
        assert (k, p, q) == (16 * expect["nct"] - 8, 5, 1) and k + p <= n and m % 16 and n % 64  # tails in rows and columns


def test_the_plane_and_ata_route_tables_are_complete(plan):
    """every instantiation of the three families occurs, counted from the lists the launchers dispatch on -- which are the
    lists the LDS registration walks"""
    cnt = _counts(plan)
    nts = range(1, cnt["col_tiles"][0] + 1)
    np_min, np_max, np_stored = cnt["planes"]
    want = {("bf16_split", nt, np_, tn) for nt in nts for np_ in range(np_min, np_max + 1) for tn in (False, True)}
    want |= {("bf16_stored", nt, np_stored, tn) for nt in nts for tn in (False, True)}
    assert len(want) == 36 + 18
    seen = {(r[8]["family"], r[8]["nt"], r[8]["np"], r[8]["tn"]) for r in PLANE_ROUTES}
    assert seen == want
    want_ata = {(nk, nct) for nk in cnt["ata_nk"] for nct in range(1, cnt["ata_nct"][0] + 1)}
    assert len(want_ata) == 15 and cnt["ata_nk"] == [2, 4, 8]
    assert {(r[6]["nk"], r[6]["nct"]) for r in ATA_ROUTES} == want_ata
    # the other lists, as tests/test_gemm_plan.py counts them by hand
    assert cnt["general4"] == [36] and cnt["general8"] == [54] and cnt["general_nw"] == [4, 8]
    assert cnt["alias"] == [8] and cnt["tall4"] == [6] and cnt["tall8"] == [4]

    # one list per family: tall_stage.hpp names each kernel of the three families once, in the function both its launcher
    # and set_lds_limits go through, and hip_backend.hpp names none of the stage's kernels any more
    stage = open(os.path.join(CSRC, "tall_stage.hpp")).read()
    strip = lambda text: "\n".join(line.split("//")[0] for line in text.splitlines())
    code, backend = strip(stage), strip(open(os.path.join(CSRC, "hip_backend.hpp")).read())
    for kernel in ("gemm_bf16s_kernel", "gemm_bf16a_kernel"):
        assert len(re.findall(r"k::%s<" % kernel, code)) == 1, kernel
    # the launch and the registration (of nn and tn, for the planes) ...
    assert code.count("k::ata_fused_kernel<") == 2 and code.count("k::gemm_tn_kernel<") == 2 and code.count("P::template kernel<") == 4
    # ... each through the list: once per use (the planes' NP range also picks split_planes_kernel<NP>)
    for name, uses in (("AtaNKs{}", 2), ("kAtaMaxColTiles", 2), ("each_general", 2), ("with_general", 2), ("P::kMaxPlanes, P::kMinPlanes", 3)):
        assert code.count(name) == uses, name
    for name in ("gemm_nn_kernel", "gemm_tn_kernel", "gemm_bf16s_kernel", "gemm_bf16a_kernel", "ata_fused_kernel", "tall_gram_kernel",
                 "tall_apply_kernel", "spmm_rows_kernel", "slab_reduce_kernel"):
        assert name not in backend, name
