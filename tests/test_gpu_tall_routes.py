"""GPU test of the dispatch of the tall products' other kernel families (gemm_plan.hpp, tall_stage.hpp; run with -m gpu on an
MI355X): one small call per instantiation of gemm_bf16s_kernel<NT, NP, TN> (the bf16 split), gemm_bf16a_kernel<NT, TN> (the
bf16-stored operand) and ata_fused_kernel<NK, NCT> (the one-sweep power iteration).  The rows are PLANE_ROUTES and ATA_ROUTES
of tests/test_gemm_plan.py; tests/test_tall_stage_plan.py pins on the CPU that every row reaches the instantiation it names
and that the rows cover every instantiation.  tests/test_gpu_gemm_routes.py does the same for the general kernels."""
import functools

import numpy as np
import pytest

from oracle import rsvd_oracle as orc
from tests.helpers import orth_err
from tests.test_gemm_plan import ATA_ROUTES, PLANE_M, PLANE_MODES, PLANE_N, PLANE_ROUTES
from tests.test_gpu_gemm_routes import BETAS, first_mismatch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def contexts():
    """one context per knob set: the size threshold of the bf16 split is read when a context is created"""
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
def plane_operands(torch):
    """A (300 x 72) and, per orientation, X with the widest row's columns and the f64 product: integers in [-8, 8], exact in
    bf16, every partial sum at most 64 * 300 < 2^24.  Computed once; a row takes the leading l columns."""
    g = torch.Generator(device="cuda").manual_seed(7)
    lmax = max(r[4] for r in PLANE_ROUTES)
    a = torch.randint(-8, 9, (PLANE_M, PLANE_N), device="cuda", generator=g).float()
    out = {"a": a, "a16": a.to(torch.bfloat16)}
    assert torch.equal(out["a16"].float(), a)
    for trans in (False, True):
        x = torch.randint(-8, 9, (PLANE_M if trans else PLANE_N, lmax), device="cuda", generator=g).float()
        ref = (a.t() if trans else a).double() @ x.double()
        assert float(ref.abs().max()) <= 64 * x.shape[0] < 1 << 24
        out[trans] = (x, ref)
    return out


@pytest.mark.parametrize("row", PLANE_ROUTES, ids=lambda r: r[0])
def test_every_plane_route_is_exact(torch, contexts, plane_operands, monkeypatch, row):
    name, family, m, n, l, trans, np_, knobs, _ = row
    ctx = contexts(knobs)
    a = plane_operands["a16" if family == "bf16_stored" else "a"]
    x_full, ref_full = plane_operands[trans]
    x, ref = x_full[:, :l].contiguous(), ref_full[:, :l]
    if family == "bf16_split":
        monkeypatch.setenv("CORRLA_SKETCH_MIXED", PLANE_MODES[np_])
    else:
        monkeypatch.delenv("CORRLA_SKETCH_MIXED", raising=False)
    for beta in BETAS:
        res = ctx.matmul(a, x, trans=trans, beta=beta)
        t = ctx.timings()
        ran = (t["n_mixed_products"], t["n_bf16_products"])
        assert ran == ((1, 0) if family == "bf16_split" else (0, 1)), (name, beta, ran)
        assert res.dtype == torch.float32 and res.shape == ((n if trans else m), l)
        want = (beta * ref).float()
        if not torch.equal(res, want):
            r, c, got, exp = first_mismatch(torch, res, want)
            wrong = int((res != want).sum())
            pytest.fail("%s beta=%g: %d of %d entries differ, first at (row %d, column %d): %r instead of %r -- 16-column tile %d, "
                        "256-row tile %d" % (name, beta, wrong, res.numel(), r, c, got, exp, c // 16, r // 256))


@functools.lru_cache(maxsize=None)
def _ata_matrix(m, n):
    """the matrix of test_one_sweep_power_iteration_matches_oracle (tests/test_gpu_parity.py): Gaussian, columns scaled by 0.995^j"""
    rng = np.random.default_rng(m + n)
    a = (rng.standard_normal((m, n)) * (0.995 ** np.arange(n))).astype(np.float32)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def ctx(contexts):
    return contexts({})


@pytest.mark.parametrize("row", ATA_ROUTES, ids=lambda r: r[0])
def test_every_one_sweep_route_matches_the_two_products_and_the_oracle(ctx, torch, row):
    """rsvd(a, k, 1, 5, fused=True): the sketch and the one power iteration are ONE launch of ata_fused_kernel<NK, NCT>.
    Bounds of test_one_sweep_power_iteration_matches_oracle: singular values within 3e-5 sigma_1 of the oracle and of the
    two-product schedule, orth_err below 2e-4, |d relerr| <= 1e-5.  The witness that the one-sweep kernel ran (the CPU test
    pins that the shape is in its domain): its U differs from the two-product U in at least one bit -- the two schedules
    round the intermediate Y differently."""
    name, m, n, k, p, q, _ = row
    a = _ata_matrix(m, n)
    om = np.random.default_rng(k + n).standard_normal((n, k + p)).astype(np.float32)
    at = torch.tensor(a, device="cuda")
    u1, s1, vt1 = ctx.rsvd(at, k, q, p, omega=om, fused=True)
    u0, s0, vt0 = ctx.rsvd(at, k, q, p, omega=om)
    uo, so, vto = orc.random_svd(a.astype(np.float64), k, q, p, omega=om.astype(np.float64))
    u1n, s1n, vt1n = u1.cpu().numpy(), s1.cpu().numpy(), vt1.cpu().numpy()
    ds_oracle = float(np.max(np.abs(s1n - so)) / so[0, 0])
    ds_two = float((s1 - s0).abs().max()) / float(so[0, 0])
    dre = abs(orc.relerr(a, u1n, s1n, vt1n) - orc.relerr(a, uo, so, vto))
    print("%s: max|dS|/s1 vs oracle %.2e, vs two products %.2e, |d relerr| %.2e, orth_err U %.2e V %.2e"
          % (name, ds_oracle, ds_two, dre, orth_err(u1n), orth_err(vt1n.T)))
    assert np.max(np.abs(s1n - so)) <= 3e-5 * so[0, 0]
    assert torch.allclose(s1, s0, rtol=0, atol=3e-5 * float(so[0, 0]))
    assert dre <= 1e-5
    assert orth_err(u1n) < 2e-4 and orth_err(vt1n.T) < 2e-4
    assert u1.shape == u0.shape and not torch.equal(u1, u0), name
