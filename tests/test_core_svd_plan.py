"""The choice of the core-SVD kernel family (random_svd.rs:89), pinned at every l on the CPU: core_svd_plan
(corrla_rs_amd/csrc/core_svd_plan.hpp) is host code, compiled here with the host compiler in a temporary directory."""
import os
import subprocess

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


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("core_svd_plan")
    src = tmp / "plan.cpp"
    src.write_text(MAIN)
    exe = tmp / "plan"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "corrla_rs_amd", "csrc"),
                           str(src), "-o", str(exe)])
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
