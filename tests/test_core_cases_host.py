"""The designed cores of tests/core_cases.py on the CPU: every family is what it claims to be at every width the GPU tests
use, and the reference alone -- the oracle, and the real driver on the emulation backend -- is inside every bound those
tests apply (tests/test_gpu_core_designed.py, tests/test_gpu_context_history.py).  No GPU."""
import numpy as np
import pytest

from oracle import rsvd_oracle as orc
from tests import core_cases as cc
from tests.emu_harness import emu_rsvd
from tests.test_gpu_round3 import _POISON_CASES

# every width at which a GPU test hands a designed core to a kernel family
WIDTHS = sorted({l for l, _ in _POISON_CASES})
# the widths of the multi-workgroup block Jacobi among them, and those of the kNeedV test: where the W-only window matters
JMC_WIDTHS = [l for l in WIDTHS if 96 <= l <= 288]
# one width per thin-Q route (thinq_plan.hpp): products in place (<= 144), conditional passes in pairs with one factor
# kernel (145 .. 176 f32 / 152 f64), the 2 x 2 blocked factor beyond
EMU_WIDTHS = [24, 138, 150, 266]
DTYPES = [np.float32, np.float64]


def test_the_widths_are_those_of_the_kernel_family_table():
    assert WIDTHS == [1, 24, 75, 95, 96, 138, 144, 170, 266, 288, 300]
    assert JMC_WIDTHS == [96, 138, 144, 170, 266, 288]
    assert set(EMU_WIDTHS) - {150} <= set(WIDTHS)


@pytest.mark.parametrize("l", WIDTHS)
def test_every_family_is_upper_triangular_with_its_target_gram(l):
    for dtype in DTYPES:
        for name in cc.families_for(l):
            r = cc.build(name, l, dtype)
            assert r.shape == (l, l) and np.all(np.isfinite(r))
            assert np.array_equal(r, np.triu(r)), name
            assert np.all(np.diag(r) != 0), name
    for rho in (cc.EQUICORR_RHO, cc.EQUICORR_RHO_KEPT):
        r = cc.equicorr(l, rho)
        assert np.max(np.abs(r @ r.T - cc.equicorr_gram(l, rho))) <= 1e-13
        if l > 1:  # one large and an (l - 1)-fold singular value
            s = np.linalg.svd(r, compute_uv=False)
            assert abs(s[0] - np.sqrt(1 + (l - 1) * rho)) <= 1e-12 * s[0]
            assert np.max(np.abs(s[1:] - np.sqrt(1 - rho))) <= 1e-12 * s[0]
    for dtype in DTYPES:   # 2^e I: its Gram, 4^e I, lies outside the 2^-40 .. 2^40 in which the thin-Q leaves a Gram unscaled
        for name, e in (("identity_down", -cc.SCALE_EXP[dtype]), ("identity_mid", cc.IDENTITY_MID_EXP), ("identity_up", cc.SCALE_EXP[dtype])):
            assert np.array_equal(cc.build(name, l, dtype), np.ldexp(np.eye(l), e)) and abs(2 * e) > 40
            assert np.array_equal(cc.case(name, l, dtype).a[:l], np.ldexp(np.eye(l), e).astype(dtype))
    d = cc.perm_diag_values(l)
    r = cc.scaled_perm_diag(l)
    assert np.array_equal(r @ r.T, np.diag(d * d))
    assert np.allclose(np.sort(d)[::-1], np.logspace(0, -3, l) if l > 1 else [1.0], rtol=1e-15, atol=0)
    if l > 2:
        assert np.any(np.diff(d) > 0) and np.any(np.diff(d) < 0)   # unsorted: the ordering does the work
        r = cc.two_level(l)
        assert np.max(np.abs(np.linalg.svd(r, compute_uv=False) - cc.two_level_values(l))) <= 1e-13
        for dtype in DTYPES:
            e = cc.SCALE_EXP[dtype]
            assert np.array_equal(cc.build("two_level_up", l, dtype), r * 2.0 ** e)
            assert np.array_equal(cc.build("two_level_down", l, dtype), r * 2.0 ** -e)
            # ... and the element type holds them: nothing overflows, nothing becomes subnormal or zero
            for name in ("two_level_up", "two_level_down"):
                c = cc.case(name, l, dtype)
                nz = np.abs(c.a[c.a != 0])
                assert np.all(np.isfinite(c.a)) and nz.min() >= np.finfo(dtype).tiny and np.count_nonzero(c.a) == np.count_nonzero(r)


@pytest.mark.parametrize("l", [w for w in WIDTHS if w > 1])
def test_kahan_cores_have_the_requested_condition_behind_a_flat_diagonal(l):
    for dtype in DTYPES:
        r = cc.build("kahan", l, dtype)
        s = np.linalg.svd(r, compute_uv=False)
        want = cc.KAHAN_COND[dtype]
        assert abs(s[0] / s[-1] - want) <= 1e-6 * want
        d = np.abs(np.diag(r))
        print("kahan l=%d %s: cond %.6g, diagonal ratio %.3f, r_ll / sigma_min %.1f" % (l, np.dtype(dtype).name, s[0] / s[-1],
                                                                                      d.max() / d.min(), d.min() / s[-1]))
        # the diagonal hides the conditioning: its ratio is far below cond(R) ...
        assert d.max() / d.min() <= want / 8
        if l >= 96:  # ... and near 1 at the widths of the multi-workgroup kernel
            assert d.max() / d.min() <= 2.0


@pytest.mark.parametrize("l", JMC_WIDTHS)
def test_equicorr_sits_in_the_window_where_w_only_is_chosen_and_refused(l):
    """jmc_init_kernel chooses W-only when the diagonal ratio of the core is <= 16; jmc_finish_kernel refuses it when the
    computed sigma_max > 64 sigma_min.  rho = 0.99: chosen and refused.  rho = 0.5: chosen and kept."""
    r = cc.equicorr(l, cc.EQUICORR_RHO)
    ratio, cond = cc.model_core_diagonal_ratio(r), np.linalg.cond(r)
    print("equicorr(%.2f) l=%d: diagonal ratio of the core %.3f, cond %.2f" % (cc.EQUICORR_RHO, l, ratio, cond))
    assert ratio <= cc.FAST_COND * 0.75 and cond > cc.VERIFY_COND * 1.25   # a quarter of margin on either side
    r = cc.equicorr(l, cc.EQUICORR_RHO_KEPT)
    ratio, cond = cc.model_core_diagonal_ratio(r), np.linalg.cond(r)
    assert ratio <= cc.FAST_COND * 0.75 and cond < cc.VERIFY_COND * 0.75
    if l == 138:   # the figures the window was chosen from
        assert abs(np.linalg.cond(cc.equicorr(138, 0.99)) - 116.9) < 0.05 and abs(cond - np.sqrt(139.0)) < 1e-9
        assert abs(cc.model_core_diagonal_ratio(cc.equicorr(138, 0.99)) - 9.96) < 0.01
    if l == 96:
        assert abs(np.linalg.cond(cc.equicorr(96, 0.99)) - 97.5) < 0.05
        assert abs(cc.model_core_diagonal_ratio(cc.equicorr(96, 0.99)) - 9.95) < 0.01


def test_the_other_families_leave_the_w_only_window_on_one_side():
    """Which mode the multi-workgroup kernel takes on each family at l = 138 (documentation of what the GPU cases reach)."""
    for dtype in DTYPES:
        # graded diagonal: V accumulated from the start
        assert cc.model_core_diagonal_ratio(cc.build("scaled_perm_diag", 138, dtype)) > 4 * cc.FAST_COND
        # the two-level cores: cond = 100 exactly, whatever the scale
        for name in ("two_level", "two_level_down", "two_level_up"):
            assert abs(np.linalg.cond(cc.build(name, 138, dtype)) - 100.0) < 1e-6


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("l", WIDTHS)
def test_the_oracle_agrees_with_numpy_on_every_designed_input(l, dtype):
    f64 = dtype == np.float64
    for name in cc.families_for(l):
        c = cc.case(name, l, dtype)
        a, k, q, p = c.args
        assert a.shape == (max(3 * l, 200), l) and a.dtype == dtype and not np.any(a[l:])
        u, s, vt = orc.random_svd(a, k, q, p, omega=c.omega)
        ds = float(np.max(np.abs(s.ravel().astype(np.float64) - c.s_ref)) / c.s_ref[0])
        assert ds <= (1e-12 if f64 else 1e-6), (name, ds)
        cc.check(c, u, s, vt, "oracle")


def test_the_host_jacobi_is_scale_invariant_to_the_bit():
    """small::jacobi_svd (the CORRLA_SVD=host family, and every core of the emulated driver) prescales by a power of two:
    without it the convergence test's product of two squared column norms overflowed for entries beyond 2^256, no pair was
    ever rotated and the column norms of the input came back as its singular values (found by two_level_up in f64)."""
    import ctypes as C
    from tests.emu_harness import emu
    e = emu()
    e.corrla_emu_jacobi_svd.restype = C.c_int
    n = 24
    c0 = cc.two_level(n)

    def run(ex):
        c = np.asfortranarray(np.ldexp(c0, ex))
        u, v, s = np.empty((n, n), order="F"), np.empty((n, n), order="F"), np.empty(n)
        sweeps = e.corrla_emu_jacobi_svd(n, c.ctypes.data_as(C.c_void_p), n, u.ctypes.data_as(C.c_void_p),
                                         s.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), C.c_double(1e-15))
        return sweeps, u, s, v

    sw0, u0, s0, v0 = run(0)
    assert 0 < sw0 < 40 and np.max(np.abs(s0 - cc.two_level_values(n))) <= 1e-13
    assert np.max(np.abs((u0 * s0) @ v0.T - c0)) <= 1e-13
    for ex in (-900, -400, 400, 900):
        sw, u, s, v = run(ex)
        assert sw == sw0 and np.array_equal(u, u0) and np.array_equal(v, v0) and np.array_equal(s, np.ldexp(s0, ex)), ex


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("l", EMU_WIDTHS)
def test_the_emulated_driver_meets_the_gpu_bounds_on_every_designed_input(l, dtype):
    for name in cc.families_for(l):
        c = cc.case(name, l, dtype)
        a, k, q, p = c.args
        u, s, vt = emu_rsvd(a, k, q, p, omega=c.omega)
        cc.check(c, u, s, vt, "emu")
