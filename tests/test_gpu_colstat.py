"""The column passes (csrc/colstat_plan.hpp, colstat_stage.hpp) on the GPU, one public call per branch of their plans.  Run
with -m gpu on an MI355X.  tests/test_colstat_plan.py pins on the CPU which branch each row of GPU_CALLS reaches.

  colvar, csr   Context.pca(standardize=True): the scales against std(ddof=1) in numpy f64 of the values the GPU sees
                (correctly rounded sums), under 4 x SCALES_ERR_MEASURED of tests/test_gpu_pca_standardize.py, whose data
                these cases use: column scales spread over 1e-3 .. 1e3 and one exactly constant column, which gets scale 1
  moments       Context.cov(correlation=True), its means and scales, and Context.cov, under the bounds of tests/test_gpu_cov.py
  wcolsum       the fused centring against the centred copy, under FUSED_COPY_* of tests/test_gpu_pca_standardize.py
Every call runs twice and must give the same bits."""
import functools

import numpy as np
import pytest

from tests.test_colstat_plan import GPU_CALLS
from tests.test_gpu_cov import _check_corr, _check_cov, _give
from tests.test_gpu_pca_standardize import (FUSED_COPY_PROJ_TOL, FUSED_COPY_S_RTOL, K, SCALES_ERR_MEASURED, _data, _omega,
                                            _proj_err, _standardise)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx():
    import corrla_rs_amd as cr
    c = cr.Context(0)
    yield c
    c.close()


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _calls(kind):
    return [pytest.param(c, id=c["id"]) for c in GPU_CALLS if c["kind"] == kind]


def _twice(call):
    """the outputs of call() as numpy arrays, after a second call has given the same bits"""
    a, b = ([None if t is None else _np(t) for t in call()] for _ in range(2))
    for ta, tb in zip(a, b):
        assert (ta is None and tb is None) or np.array_equal(ta, tb, equal_nan=True), "two runs differ"
    return a


def _check_scales(call, seen64, scales, const_col):
    sd = _standardise(seen64)[2]
    out_dt = np.float64 if call["dtype"] == "float64" else np.float32
    assert scales.shape == sd.shape and scales.dtype == out_dt
    assert scales[0, const_col] == 1.0                                       # the constant column: exactly 1
    err = float(np.max(np.abs(scales.astype(np.float64) - sd) / sd))
    print(f"colstat {call['id']}: scales max rel err {err:.3e} (bound {4.0 * SCALES_ERR_MEASURED[call['dtype']]:.3e})")
    assert err <= 4.0 * SCALES_ERR_MEASURED[call["dtype"]], (call["id"], err)


@pytest.mark.parametrize("call", _calls("colvar"))
def test_column_variances_of_a_dense_operand(ctx, torch, call):
    m, n, seed = call["m"], call["n"], 500 + call["m"] + call["n"]
    x64 = _data(m, n, seed)
    if call["dtype"] == "bf16":
        x = torch.tensor(np.asarray(x64), dtype=torch.float32).to(torch.bfloat16).cuda()
        seen = x.float().cpu().numpy().astype(np.float64)
    else:
        tdt = getattr(torch, call["dtype"])
        if "ld" in call:   # n columns of a wider buffer: nothing behind column n - 1 may be counted
            big = torch.full((m, call["ld"]), 1e6, dtype=tdt, device="cuda")
            big[:, :n] = torch.tensor(np.asarray(x64), dtype=tdt, device="cuda")
            x = big[:, :n]
            assert x.stride() == (call["ld"], 1)
        else:
            x = torch.tensor(np.asarray(x64), dtype=tdt, device="cuda")
            if call["layout"] == "col":
                x = x.t().contiguous().t()                                     # same values, column-major memory
                assert x.stride() == (1, m)
        seen = x.cpu().numpy().astype(np.float64)
    om = _omega(m, n, seed + 1)
    _means, _s, _comps, scales = _twice(lambda: ctx.pca(x, K, omega=om, standardize=True))
    _check_scales(call, seen, scales, n // 2)


@functools.lru_cache(maxsize=None)
def _sparse(m, n):
    """m x n at density 0.05 with column scales 1e-3 .. 1e3; column 10 is all zero: (scipy CSR f32, its dense f64 form)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(31 * m + n)
    mask = rng.random((m, n)) < 0.05
    mask[:, 10] = False
    v = rng.standard_normal((m, n)) * 10.0 ** rng.uniform(-3, 3, n)
    a = sp.csr_matrix(np.where(mask, v, 0.0).astype(np.float32))
    a.sort_indices()
    return a, a.toarray().astype(np.float64)


@pytest.mark.parametrize("call", _calls("csr"))
def test_column_variances_of_a_csr_operand(ctx, call):
    a, dense = _sparse(call["m"], call["n"])
    om = _omega(call["m"], call["n"], 5)
    _means, _s, _comps, scales = _twice(lambda: ctx.pca(a, K, omega=om, standardize=True))
    _check_scales(call, dense, scales, 10)


@pytest.mark.parametrize("call", _calls("moments"))
def test_column_moments_through_cov(ctx, torch, call):
    m, n = call["m"], call["n"]
    dtype = np.dtype(call["dtype"]).type
    x = np.random.default_rng(1000 * m + n + 2).standard_normal((m, n))
    x[:, 1] += 0.8 * x[:, 0]                       # some real correlation, scales over 1e-2 .. 1e2, means within 3 sd
    x = ((x + np.linspace(-3, 3, n)) * np.logspace(-2, 2, n)).astype(dtype)
    if "ld" in call:
        padded = np.zeros((m, call["ld"]), dtype=dtype)
        padded[:, :n] = x
        x = padded[:, :n]
    xd = _give(torch, x, "dev")
    assert xd.stride() == (call.get("ld", n), 1)
    r, means, scales = _twice(lambda: ctx.cov(xd, correlation=True))
    _check_corr(x, r, scales, "colstat corr " + call["id"])
    c, means_c, _none = _twice(lambda: ctx.cov(xd))
    assert np.array_equal(means, means_c)          # the same pass, whatever follows it
    _check_cov(x, c, means_c, 1, "colstat cov " + call["id"])


@pytest.mark.parametrize("call", _calls("wcolsum"))
def test_weighted_column_sums_of_the_fused_centring(ctx, torch, call):
    m, n, dtype, seed = call["m"], call["n"], call["dtype"], 700 + call["m"]
    x = torch.tensor(np.asarray(_data(m, n, seed)), dtype=getattr(torch, dtype), device="cuda")
    om = _omega(m, n, seed + 1)
    mf, sf, cf, df = _twice(lambda: ctx.pca(x, K, omega=om, center="fused", standardize=True))
    mc, sc, cc, dc = _twice(lambda: ctx.pca(x, K, omega=om, center="copy", standardize=True))
    assert np.array_equal(mf, mc) and np.array_equal(df, dc)
    print(f"colstat {call['id']}: fused vs copy max |dS|/S {float(np.max(np.abs(sf - sc) / sc)):.3e}  projector {_proj_err(cf, cc):.3e}")
    assert np.allclose(sf, sc, rtol=FUSED_COPY_S_RTOL[dtype])
    assert _proj_err(cf, cc) < FUSED_COPY_PROJ_TOL[dtype]
