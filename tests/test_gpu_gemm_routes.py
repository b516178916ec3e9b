"""GPU test of the tall products' dispatch (gemm_plan.hpp, launch_gemm in tall_stage.hpp; run with -m gpu on an MI355X): one
small Context.matmul per instantiation and per feature of the plan -- every gemm_nn_kernel / gemm_tn_kernel<T, MW, NT, NW>,
both ring depths of the wide tile, the uneven two-launch column blocking, persistent launches, both slab reductions, empty
slabs, the XCD remap, rotation and its absence -- on integer operands whose product is exact in either element type, and on
Gaussian operands against the componentwise rounding bound of a dot product; then the aliased Gram instantiations through
power_iter against the general kernels.  tests/test_gemm_plan.py pins on the CPU that every row reaches what it names."""
import os

import numpy as np
import pytest

from tests.helpers import orth_err
from tests.test_gemm_plan import GRAM_COLS, GRAM_ROUTES, ROUTES, route_a, route_x

pytestmark = pytest.mark.gpu

PINNED_CUS = 256  # the routes of ROUTES were pinned for this many compute units
BETAS = (1.0, 0.25)  # a power of two keeps the integer products exact: applied once is right, twice is not


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def contexts():
    """one context per knob set: the geometry knobs are read when a context is created"""
    import corrla_rs_amd as cr
    made = {}

    def get(knobs):
        key = tuple(sorted(knobs.items()))
        if key not in made:
            with pytest.MonkeyPatch.context() as mp:
                for name, val in key:
                    mp.setenv(name, str(val))
                made[key] = cr.Context(0)
        return made[key]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def device_note(torch):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    note = "" if cus == PINNED_CUS else " (the route names were pinned for %d compute units, this device has %d)" % (PINNED_CUS, cus)
    print("compute units: %d%s" % (cus, note))
    return note


def _index(torch, n):
    return torch.arange(n, device="cuda", dtype=torch.int64)


def first_mismatch(torch, res, ref):
    """(row, column, got, want) of the first entry of res that differs from ref, columns first"""
    bad = (res != ref) | torch.isnan(res)
    col = int(torch.nonzero(bad.any(dim=0))[0])
    row = int(torch.nonzero(bad[:, col])[0])
    return row, col, float(res[row, col]), float(ref[row, col])


@pytest.mark.parametrize("row", ROUTES, ids=lambda r: r[0])
def test_every_route_is_exact_and_within_the_rounding_bound(torch, contexts, device_note, row):
    name, esz, m, n, l, trans, knobs, _ = row
    dt = torch.float32 if esz == 4 else torch.float64
    ctx = contexts(knobs)
    red, outer = (m, n) if trans else (n, m)

    # a. exact: integers in [-3, 3] x [-4, 4], every partial sum below 12 * red < 2^24
    a = route_a(_index(torch, m)[:, None], _index(torch, n)[None, :]).to(dt)
    x = route_x(_index(torch, red)[:, None], _index(torch, l)[None, :]).to(dt)
    ref = ((a.t() if trans else a).double() @ x.double())
    assert float(ref.abs().max()) <= 12 * red < 1 << 24
    for beta in BETAS:
        res = ctx.matmul(a, x, trans=trans, beta=beta)
        assert res.shape == (outer, l)
        want = (beta * ref).to(dt)
        if not torch.equal(res, want):
            r, c, got, exp = first_mismatch(torch, res, want)
            wrong = int((res != want).sum())
            pytest.fail("%s beta=%g: %d of %d entries differ, first at (row %d, column %d): %r instead of %r -- 16-column tile %d, "
                        "64-row tile %d%s" % (name, beta, wrong, res.numel(), r, c, got, exp, c // 16, r // 64, device_note))
    del a, x, ref

    # b. rounding: |res - ref| <= gamma |op(A)| |X| componentwise, gamma = red u / (1 - red u), for any order of an FMA sum;
    # an f64 reference carries the same bound, so gamma is doubled there
    g = torch.Generator(device="cuda").manual_seed(1000 * m + n + l)
    a = torch.randn((m, n), dtype=dt, device="cuda", generator=g)
    x = torch.randn((red, l), dtype=dt, device="cuda", generator=g)
    u = 2.0 ** -24 if esz == 4 else 2.0 ** -53
    gamma = red * u / (1.0 - red * u) * (1 if esz == 4 else 2)
    op = (a.t() if trans else a).double()
    ref = op @ x.double()
    scale = op.abs() @ x.double().abs()
    assert float(scale.min()) > 0
    for beta in BETAS:
        res = ctx.matmul(a, x, trans=trans, beta=beta)
        ratio = float(((res.double() - beta * ref).abs() / (beta * scale)).max())
        print("route %s beta=%g: max |res - ref| / (|op(A)| |X|) = %.3e, gamma = %.3e (%.3f of it)" % (name, beta, ratio, gamma, ratio / gamma))
        assert ratio <= gamma, (name, beta, ratio, gamma, device_note)


# ---- the aliased Gram instantiations gemm_nn_kernel<T, 2, NT, true>: only a thin-Q reaches them ---------------------
@pytest.mark.parametrize("esz,nt", sorted({(r[1], r[5]["nt"][0]) for r in GRAM_ROUTES}), ids=lambda v: str(v))
def test_aliased_gram_kernels_match_the_general_kernels(contexts, esz, nt):
    """power_iter on a 700 x 150 Gaussian matrix, width 16 NT - 3, shared Omega: the default context forms G = Y^T Y on the
    aliased kernel, the context created under CORRLA_NO_GRAM_ALIAS=1 on the general kernel the route test above checks
    exactly.  Bounds of test_tall_thin_q_products_match_the_general_kernels_and_the_oracle (tests/test_gpu_parity.py)."""
    rows = [r for r in GRAM_ROUTES if r[1] == esz and r[5]["nt"] == (nt,)]
    assert sorted(r[5]["family"] for r in rows) == ["general", "gram_alias"]
    dtype = np.float32 if esz == 4 else np.float64
    tol = 2e-5 if esz == 4 else 1e-13
    m, l = rows[0][2], rows[0][3]
    rng = np.random.default_rng(100 * esz + nt)
    a = rng.standard_normal((m, GRAM_COLS)).astype(dtype)
    om = rng.standard_normal((GRAM_COLS, l)).astype(dtype)
    q = {}
    for r in rows:
        q[r[5]["family"]] = contexts(r[4]).power_iter(a, l, 1, omega=om)
    qa, qg = q["gram_alias"], q["general"]
    assert qa.shape == qg.shape == (m, l)
    assert np.all(np.isfinite(qa)) and np.all(np.isfinite(qg))
    ea, eg, diff = orth_err(qa), orth_err(qg), float(np.max(np.abs(qa.astype(np.float64) - qg.astype(np.float64))))
    print("gram f%d NT=%d l=%d: orth_err alias %.3e general %.3e, max |Q_alias - Q_general| = %.3e (bound %.0e)"
          % (8 * esz, nt, l, ea, eg, diff, tol))
    assert ea <= tol and eg <= tol
    assert diff <= tol
