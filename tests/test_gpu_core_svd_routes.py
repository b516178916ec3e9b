"""GPU test of the core SVD's dispatch (core_svd_stage.hpp; run with -m gpu on an MI355X): one small call per instantiation
the launchers can select -- the four ring kernels per element type, the nine chunk-row counts of the multi-workgroup step
kernel, the block kernel at l = 1, beyond the multi-workgroup geometry and beyond the ring's widths -- each against the
oracle.  tests/test_core_svd_plan.py pins on the CPU that every row reaches what it names."""
import numpy as np
import pytest

from tests.test_core_svd_plan import ROUTES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import corrla_rs_amd as cr
    return cr.Context(0)


def route_case(l, dtype):
    """The shapes of the non-finite-core test (tests/test_gpu_round3.py): the smallest that reach each kernel."""
    rng = np.random.default_rng(l)
    m, n = max(3 * l, 200), l + 25
    p = min(8, l - 1)
    a = rng.standard_normal((m, n)).astype(dtype)
    om = rng.standard_normal((n, l)).astype(dtype)
    return a, l - p, 2, p, om


@pytest.mark.parametrize("row", ROUTES, ids=lambda r: "f%d-%s-l%d" % (8 * r[0], r[1], r[2]))
def test_every_route_matches_the_oracle(ctx, monkeypatch, row):
    """The bounds of the clean half of the non-finite-core test at these shapes: 3e-5 (f32) / 1e-10 (f64) of S[0]."""
    from oracle import rsvd_oracle as orc
    esz, mode, l = row[:3]
    dtype = np.float32 if esz == 4 else np.float64
    a, k, q, p, om = route_case(l, dtype)
    if mode != "default":
        monkeypatch.setenv("CORRLA_SVD", mode)
    u, s, vt = ctx.rsvd(a, k, q, p, omega=om)
    so = orc.random_svd(a, k, q, p, omega=om)[1].ravel()
    s = s.ravel().astype(np.float64)
    err = float(np.max(np.abs(s - so)))
    print("route f%d %s l=%d: max |S - S_oracle| = %.3e of S[0] = %.3e" % (8 * esz, mode, l, err, so[0]))
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(s)) and np.all(np.isfinite(vt))
    assert np.all(s >= 0) and np.all(np.diff(s) <= 0)
    assert err <= (3e-5 if esz == 4 else 1e-10) * so[0]
