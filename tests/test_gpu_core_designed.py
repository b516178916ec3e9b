"""GPU test (run with -m gpu on an MI355X): every kernel family of the core SVD on every designed core of
tests/core_cases.py -- an (l - 1)-fold cluster, a graded triangular core whose diagonal hides its conditioning, an
already-diagonal core, two clusters, cores 2^-e / 2^+e away from unit scale, and 2^e I -- with the FACTORS checked, not S alone:
S against numpy's f64 svd(R), U diag(S) V^T = A, and the orthonormality of U and of the square V^T.  With k = l nothing is
truncated, so none of the three depends on how a cluster is split.  tests/test_core_cases_host.py proves on the CPU that
the oracle and the emulated driver are inside every bound used here.

What the scaled cores found (46 of the 212 cases failed before the repair; every unscaled family passed on every row):
  two_level_up   f64 (2^+400), all rows   CORRLA_ENUMERIC "non-finite Gram matrix": the thin-Q inspected its Gram in float
                                          whatever the element type, and 2^800 is inf as a float
  two_level_down f64 (2^-400), all rows   no error and max |S - svd(R)| = 0.59 .. 0.88 sigma_1: 2^-800 is 0 as a float, every
                                          column counted as null and was re-seeded at random
  two_level_down f32 (2^-60),  all rows   CORRLA_ENUMERIC: the pivots of the small cluster, 1e-4 * 2^-120, are subnormal
  two_level_up   f32 (2^+60),  l = 300    max |S - svd(R)| = 4.1e-5 sigma_1 (8.1e-7 unscaled): the block Jacobi had no prescale
Repaired in chol_inv_kernel / gram_inspect_kernel (power-of-four prescale of a Gram outside 2^-40 .. 2^40, inspection in the
element type), jmc_init_kernel and core_finite_check_kernel (element type), and the block Jacobi (prescale chosen by the
finiteness check); small::jacobi_svd on the host had the same overflow (tests/test_core_cases_host.py).

The context is shared and the cases run family-major, `equicorr` last: its refused W-only attempt makes the context
accumulate V for good.  Before it the kernel chooses the mode itself from the diagonal of the core: `equicorr_kept` and the
three `identity` families run W-only on every multi-workgroup row; `scaled_perm_diag`, `two_level` (diagonal ratio of the
core 100) and `kahan` (20 - 31 in f32, thousands in f64: the core is the OTHER triangular factor of R R^T, not R) accumulate
V.  The last test of the file runs every family on a context of its own and pins the mode against the CPU model."""
import re

import numpy as np
import pytest

from tests import core_cases as cc
from tests.test_gpu_round3 import _POISON_CASES

pytestmark = pytest.mark.gpu

# the kernel families of the non-finite-core test without the two rows that only vary the thin-Q, and the ring schedule
# of the multi-workgroup kernel
_THIN_Q_ONLY = ("CORRLA_DEVICE_ROBUST_QR", "CORRLA_HOST_CHOL")
KERNEL_ROWS = [(l, env) for l, env in _POISON_CASES if not any(name in env for name in _THIN_Q_ONLY)]
KERNEL_ROWS.append((138, {"CORRLA_JMC_LOCAL": "0"}))


def _row_id(row):
    l, env = KERNEL_ROWS[row]
    return "l%d" % l + "".join("-%s=%s" % (k.replace("CORRLA_", "").lower(), v) for k, v in sorted(env.items()))


CASES = [(name, row) for name in cc.FAMILIES for row in range(len(KERNEL_ROWS)) if name in cc.families_for(KERNEL_ROWS[row][0])]


def test_the_kernel_rows_are_the_table_of_the_non_finite_core_test():
    assert len(_POISON_CASES) == 17 and len(KERNEL_ROWS) == 16
    assert all(not any(name in env for name in _THIN_Q_ONLY) for _, env in KERNEL_ROWS)
    assert len(CASES) == 15 * len(cc.FAMILIES) + 4     # l = 1: the four diagonal cores only


@pytest.fixture(scope="module")
def ctx():
    import corrla_rs_amd as cr
    return cr.Context(0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name,row", CASES, ids=["%s-%s" % (name, _row_id(row)) for name, row in CASES])
def test_every_kernel_family_factors_every_designed_core(ctx, monkeypatch, name, row, dtype):
    l, env = KERNEL_ROWS[row]
    for var, val in env.items():
        monkeypatch.setenv(var, val)
    c = cc.case(name, l, dtype)
    a, k, q, p = c.args
    u, s, vt = ctx.rsvd(a, k, q, p, omega=c.omega)
    cc.check(c, u, s, vt, _row_id(row))


# ---- the multi-workgroup rows once more, every family on a context of its own --------------------------------------------
# On the shared context above nothing says which mode served a case, and a refused W-only attempt changes it for every case
# behind.  Here every family starts from a fresh context at two multi-workgroup widths, and the debug lines say which mode
# served it.
_SVD_LINE = re.compile(r"jacobi_svd \(multi-workgroup, \d+ sweeps enqueued, (W only|V accumulated)\)")
_REC_LINE = re.compile(r"status record \d+ \(core SVD\): fail (\d+)")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("l", [138, 288])
@pytest.mark.parametrize("name", cc.FAMILIES)
def test_every_family_on_a_fresh_context_takes_the_mode_its_diagonal_and_sigma_dictate(monkeypatch, capfd, name, l, dtype):
    import corrla_rs_amd as cr
    monkeypatch.setenv("CORRLA_DEBUG", "1")
    c = cc.case(name, l, dtype)
    a, k, q, p = c.args
    ctx = cr.Context(0)
    try:
        capfd.readouterr()
        u, s, vt = ctx.rsvd(a, k, q, p, omega=c.omega)
        err = capfd.readouterr().err
    finally:
        ctx.close()
    modes, fails = _SVD_LINE.findall(err), [int(f) for f in _REC_LINE.findall(err)]
    ratio, cond = cc.model_core_diagonal_ratio(c.r), c.s_ref[0] / c.s_ref[-1]
    print("%s l=%d %s: diagonal ratio %.3g cond %.3g -> modes %s, fails %s" % (name, l, np.dtype(dtype).name, ratio, cond, modes, fails))
    cc.check(c, u, s, vt, "fresh")
    assert modes and fails and fails[-1] == 0
    # the CPU model of the core decides what to expect, with a quarter of margin around the kernel's two thresholds
    if ratio <= 0.75 * cc.FAST_COND and cond <= 0.75 * cc.VERIFY_COND:
        assert set(modes) == {"W only"} and fails == [0]
    elif ratio <= 0.75 * cc.FAST_COND and cond >= 1.25 * cc.VERIFY_COND:
        assert modes[0] == "W only" and fails[0] == 4 and modes[-1] == "V accumulated"
    elif ratio >= 1.25 * cc.FAST_COND:
        assert set(modes) == {"V accumulated"} and 4 not in fails
