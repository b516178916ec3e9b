"""Host tests of the numpy paths of the statistics entries that the other *_host.py files do not reach: solve, cholesky,
rbf_system, rbf_fit, dirichlet_draws, dirichlet_sample, mvn_sample and sandwich_diag, on a Context without a device
(tests/api_stub.py).  Each pins the symbol called, the whole argument tuple, the outputs, the number of
corrla_ctx_synchronize calls and which last_* accessors moved.  The arrays are views of wider storage, so that a leading
dimension cannot pass for a width."""
import ctypes as C

import numpy as np
import pytest

from corrla_rs_amd import _lib as L
from tests.api_stub import last_records, make_stub, on_gpu

SOLVE = (2, 0, 0.5, 4.0)                 # what the fake corrla_ctx_last_solve reports: route, info, min_pivot, max_u
CHOL = (1, 0, 0.25, 8.0, -1.5)           # ... corrla_ctx_last_chol: route, info, min_diag, max_diag, logdet
SOLVE_INFO = {"info": 0, "min_pivot": 0.5, "max_u": 4.0}
CHOL_INFO = {"info": 0, "min_diag": 0.25, "max_diag": 8.0, "logdet": -1.5}


@pytest.fixture
def stub():
    return make_stub(last={"corrla_ctx_last_solve": SOLVE, "corrla_ctx_last_chol": CHOL, "corrla_ctx_last_dirichlet": (0x0302,),
                           "corrla_ctx_last_mvn": (1,)})


def padded(rows, cols, dtype=np.float64, pad=1):
    """a (rows, cols) view of (rows, cols + pad) storage, filled with distinct values"""
    wide = np.arange(rows * (cols + pad), dtype=dtype).reshape(rows, cols + pad)
    return wide[:, :cols]


def moved(c, before):
    now = last_records(c)
    return {k: v for k, v in now.items() if v != before[k]}


def test_nothing_is_recorded_before_the_first_call(stub):
    assert all(v is None for v in last_records(stub[0]).values())


@pytest.mark.parametrize("assume", ["general", "pos"])
def test_solve_builds_its_call(stub, assume):
    c, rec, names = stub
    a, b = padded(3, 3), padded(3, 2)
    before = last_records(c)
    x = c.solve(a, b, assume=assume)
    assert names == ["corrla_chol_solve_f64" if assume == "pos" else "corrla_lu_solve_f64"]
    # (ctx, a, n, lda, b, n_rhs, ldb, x, ldx)
    assert rec.calls[-1] == (None, a.ctypes.data, 3, 4, b.ctypes.data, 2, 3, x.ctypes.data, 2)
    assert type(x) is np.ndarray and x.shape == (3, 2) and x.dtype == np.float64
    want = {"chol_route": "small", "chol_info": CHOL_INFO} if assume == "pos" else {"solve_route": "blocked", "solve_info": SOLVE_INFO}
    assert moved(c, before) == want
    assert rec.log == ["entry", "corrla_ctx_last_chol" if assume == "pos" else "corrla_ctx_last_solve"]   # no synchronize on the host
    # a vector b is one column, and a vector comes back over the same memory
    x = c.solve(a, np.arange(3.0), assume=assume)
    assert x.shape == (3,) and rec.calls[-1][2:4] == (3, 4) and rec.calls[-1][5:] == (1, 1, x.ctypes.data, 1)
    # anything that is not float64 is converted: a copy, contiguous
    c.solve(a.astype(np.float32), b.astype(np.int64), assume=assume)
    assert rec.calls[-1][1] != a.ctypes.data and rec.calls[-1][2:4] == (3, 3) and rec.calls[-1][5:7] == (2, 2)
    assert rec.log.count("corrla_ctx_synchronize") == 0


@pytest.mark.parametrize("assume", ["general", "pos"])
def test_solve_keeps_the_record_of_a_numeric_failure_and_of_nothing_else(stub, assume, monkeypatch):
    c, rec, _ = stub
    monkeypatch.setattr(L, "load", lambda: c._lib)       # where check() asks for the message
    key, last = ("chol", "corrla_ctx_last_chol") if assume == "pos" else ("solve", "corrla_ctx_last_solve")
    a, b = padded(3, 3), padded(3, 2)
    c.solve(a, b, assume=assume)
    c._lib.last[last] = (1, 2) + c._lib.last[last][2:]
    rec.rc = L.ENUMERIC
    with pytest.raises(L.CorrlaError, match="what the fake library says"):
        c.solve(a, b, assume=assume)
    after = last_records(c)
    assert after[key + "_route"] == "small" and after[key + "_info"]["info"] == 2
    assert rec.log[-2:] == ["entry", last]
    c._lib.last[last] = (2, 3) + c._lib.last[last][2:]
    rec.rc = L.EINVAL
    with pytest.raises(ValueError, match="what the fake library says"):
        c.solve(a, b, assume=assume)
    assert last_records(c) == after and rec.log[-1] == "entry"
    assert rec.log.count("corrla_ctx_synchronize") == 0


def test_cholesky_builds_its_call_and_keeps_the_record_of_a_numeric_failure(stub, monkeypatch):
    c, rec, names = stub
    monkeypatch.setattr(L, "load", lambda: c._lib)
    a = padded(3, 3)
    before = last_records(c)
    out = c.cholesky(a)
    assert names == ["corrla_chol_factor_f64"]
    # (ctx, a, n, lda, l, ldl)
    assert rec.calls[-1] == (None, a.ctypes.data, 3, 4, out.ctypes.data, 3)
    assert type(out) is np.ndarray and out.shape == (3, 3) and out.dtype == np.float64
    assert moved(c, before) == {"chol_route": "small", "chol_info": CHOL_INFO}
    assert rec.log == ["entry", "corrla_ctx_last_chol"]
    c._lib.last["corrla_ctx_last_chol"] = (2, 3, 0.25, 8.0, 0.0)
    rec.rc = L.ENUMERIC
    with pytest.raises(L.CorrlaError):
        c.cholesky(a)
    after = last_records(c)
    assert after["chol_route"] == "blocked" and after["chol_info"] == {"info": 3, "min_diag": 0.25, "max_diag": 8.0, "logdet": 0.0}
    c._lib.last["corrla_ctx_last_chol"] = CHOL
    rec.rc = L.EINVAL
    with pytest.raises(ValueError, match="what the fake library says"):
        c.cholesky(a)
    assert last_records(c) == after and rec.log == ["entry", "corrla_ctx_last_chol"] * 2 + ["entry"]
    with pytest.raises(ValueError, match="overwrite=True needs a CUDA tensor"):
        c.cholesky(a, overwrite=True)
    with pytest.raises(ValueError, match=r"a must be square and non-empty, got \(3, 2\)"):
        c.cholesky(padded(3, 2))


@pytest.mark.parametrize("poly_degree,degree,n_poly", [(None, -1, 0), (-3, -1, 0), (0, 0, 4), (1, 1, 4), (2, 2, 10), (5, 5, 10)])
def test_rbf_system_and_fit_build_their_calls(stub, poly_degree, degree, n_poly):
    c, rec, names = stub
    x, y = padded(4, 3), padded(4, 2)
    before = last_records(c)
    m = c.rbf_system(x, 2, 0.5, poly_degree=poly_degree)
    n = 4 + n_poly
    # (ctx, x, n_s, ldx, dim, kernel, eps, poly_degree, out, ld_out)
    assert rec.calls[-1] == (None, x.ctypes.data, 4, 4, 3, 2, 0.5, degree, m.ctypes.data, n)
    assert type(m) is np.ndarray and m.shape == (n, n) and m.dtype == np.float64
    assert moved(c, before) == {} and rec.log == ["entry"]
    w = c.rbf_fit(x, y, 7, poly_degree=poly_degree)          # an unknown kernel id is the Gaussian, the parameter defaults to 0
    # (ctx, x, n_s, ldx, dim, y, n_rhs, ldy, kernel, eps, poly_degree, out, ld_out)
    assert rec.calls[-1] == (None, x.ctypes.data, 4, 4, 3, y.ctypes.data, 2, 3, 4, 0.0, degree, w.ctypes.data, 2)
    assert type(w) is np.ndarray and w.shape == (n, 2) and w.dtype == np.float64
    assert moved(c, before) == {"solve_route": "blocked", "solve_info": SOLVE_INFO}
    assert rec.log == ["entry", "entry", "corrla_ctx_last_solve"]
    w = c.rbf_fit(x, np.arange(4.0), 1)                       # a vector y is one column; the result stays a matrix
    assert w.shape == (4, 1) and rec.calls[-1][6:8] == (1, 1) and rec.calls[-1][10] == -1
    assert names == ["corrla_rbffit_system_f64", "corrla_rbffit_f64", "corrla_rbffit_f64"]


def test_rbf_fit_keeps_the_record_of_a_numeric_failure_and_of_nothing_else(stub, monkeypatch):
    c, rec, _ = stub
    monkeypatch.setattr(L, "load", lambda: c._lib)
    x, y = padded(4, 3), padded(4, 2)
    c._lib.last["corrla_ctx_last_solve"] = (1, 5, 0.0, 1.0)
    rec.rc = L.ENUMERIC
    with pytest.raises(L.CorrlaError):
        c.rbf_fit(x, y, 1)
    after = last_records(c)
    assert after["solve_route"] == "small" and after["solve_info"] == {"info": 5, "min_pivot": 0.0, "max_u": 1.0}
    c._lib.last["corrla_ctx_last_solve"] = SOLVE
    rec.rc = L.EINVAL
    with pytest.raises(ValueError, match="what the fake library says"):
        c.rbf_fit(x, y, 1)
    assert last_records(c) == after and rec.log == ["entry", "corrla_ctx_last_solve", "entry"]
    rec.rc = L.OK
    for bad in (True, 1.0, "1"):
        with pytest.raises(ValueError, match="poly_degree must be None or an integer"):
            c.rbf_fit(x, y, 1, poly_degree=bad)
        with pytest.raises(ValueError, match="poly_degree must be None or an integer"):
            c.rbf_system(x, 1, poly_degree=bad)
    with pytest.raises(ValueError, match=r"y must have n_s = 4 rows and at least one column, got \(3, 2\)"):
        c.rbf_fit(x, padded(3, 2), 1)
    with pytest.raises(ValueError, match="x must be non-empty"):
        c.rbf_system(np.zeros((0, 3)), 1)
    assert len(rec.calls) == 2


def test_dirichlet_draws_and_sample_build_their_calls(stub):
    c, rec, names = stub
    before = last_records(c)
    rec.peek = {1: (C.c_double, 3)}
    out = c.dirichlet_draws(4, [1.0, 2.0, 3.0], c_scale=2.0, seed=7, first=5)
    a = rec.calls[-1]
    # (ctx, alphas, d, c_scale, seed, first, n, out, ldo)
    assert len(a) == 9 and a[0] is None and a[2:] == (3, 2.0, 7, 5, 4, out.ctypes.data, 3)
    assert np.array_equal(rec.seen[1], [1.0, 2.0, 3.0])
    assert type(out) is np.ndarray and out.shape == (4, 3) and out.dtype == np.float64
    assert moved(c, before) == {"dirichlet_route": "registers/general", "dirichlet_readbacks": 3}
    assert rec.log == ["entry", "corrla_ctx_last_dirichlet"]
    c._lib.last["corrla_ctx_last_dirichlet"] = (0x0003,)
    bounds = np.array([[0.0, 1.0], [0.125, 0.5], [0.25, 0.75]])
    rec.peek = {1: (C.c_double, 6), 2: (C.c_double, 3)}
    out, n_found, n_drawn = c.dirichlet_sample(bounds, 4, seed=9, max_zshots=6, chunk_size=50)
    a = rec.calls[-1]
    # (ctx, bounds, alphas, d, c_scale, seed, n_samples, max_zshots, chunk_size, out, ldo, n_found, n_drawn)
    assert len(a) == 13 and a[0] is None and a[3:11] == (3, 1.0, 9, 4, 6, 50, out.ctypes.data, 3)
    assert np.array_equal(rec.seen[1], bounds.ravel()) and np.array_equal(rec.seen[2], [1.0, 1.0, 1.0])    # alphas None: all ones
    assert isinstance(a[11]._obj, C.c_int64) and isinstance(a[12]._obj, C.c_int64) and (n_found, n_drawn) == (0, 0)
    assert type(out) is np.ndarray and out.shape == (4, 3) and out.dtype == np.float64
    assert c.last_dirichlet_route() == "regenerate/exponential" and c.last_dirichlet_readbacks() == 0
    assert set(moved(c, before)) == {"dirichlet_route", "dirichlet_readbacks"}
    assert rec.log == ["entry", "corrla_ctx_last_dirichlet"] * 2 and names == ["corrla_dirichlet_draws_f64", "corrla_dirichlet_sample_f64"]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mvn_sample_builds_its_call(stub, dtype):
    c, rec, names = stub
    suf = "f32" if dtype == np.float32 else "f64"
    f, mean = padded(3, 2, dtype), np.arange(3, dtype=dtype)
    before = last_records(c)
    out = c.mvn_sample(4, f, mean, seed=7, first=5)
    # (ctx, n, d, r, factor, ldf, mean, seed, first, lower, out, ldo)
    assert rec.calls[-1] == (None, 4, 3, 2, f.ctypes.data, 3, mean.ctypes.data, 7, 5, 0, out.ctypes.data, 3)
    assert type(out) is np.ndarray and out.shape == (4, 3) and out.dtype == dtype
    assert moved(c, before) == {"mvn_route": "fused"} and rec.log == ["entry", "corrla_ctx_last_mvn"]
    # no mean: NULL; lower: the flag, on a square factor; a given out with a padded row stride is filled where it lies
    sq, given = padded(3, 3, dtype, pad=2), padded(4, 3, dtype, pad=2)
    out = c.mvn_sample(4, sq, lower=True, out=given)
    assert out is given and rec.calls[-1] == (None, 4, 3, 3, sq.ctypes.data, 5, None, 0, 0, 1, given.ctypes.data, 5)
    out = c.mvn_sample(1, f)                                  # one row has no stride: its length serves
    assert rec.calls[-1][10:] == (out.ctypes.data, 3)
    assert names == ["corrla_mvn_sample_" + suf] * 3
    # n = 0: an empty array, the route "empty", and the library is not touched
    n_log = len(rec.log)
    out = c.mvn_sample(0, f, mean)
    assert out.shape == (0, 3) and out.dtype == dtype and c.last_mvn_route() == "empty"
    assert len(rec.calls) == 3 and len(rec.log) == n_log and len(names) == 3
    assert rec.log.count("corrla_ctx_synchronize") == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sandwich_diag_builds_its_call(stub, dtype):
    c, rec, names = stub
    jac, cov = padded(4, 3, dtype), padded(3, 3, dtype, pad=2)
    before = last_records(c)
    v = c.sandwich_diag(jac, cov)
    # (ctx, jac, m, d, ldj, cov, ldc, out)
    assert rec.calls[-1] == (None, jac.ctypes.data, 4, 3, 4, cov.ctypes.data, 5, v.ctypes.data)
    assert type(v) is np.ndarray and v.shape == (4,) and v.dtype == dtype
    assert moved(c, before) == {} and rec.log == ["entry"]
    assert names == ["corrla_sandwich_diag_" + ("f32" if dtype == np.float32 else "f64")]
    c.sandwich_diag(np.asfortranarray(jac), cov)              # a column-major jac is copied into rows
    assert rec.calls[-1][1] != jac.ctypes.data and rec.calls[-1][4] == 3
    with pytest.raises(ValueError, match=r"cov must have the dtype of the other arguments"):
        c.sandwich_diag(jac, cov.astype(np.float32 if dtype == np.float64 else np.float64))
    with pytest.raises(ValueError, match=r"jac must be float32 or float64, got int64"):
        c.sandwich_diag(np.zeros((4, 3), dtype=np.int64), cov)
    with pytest.raises(ValueError, match=r"cov must be \(3, 3\), got shape \(3, 2\)"):
        c.sandwich_diag(jac, padded(3, 2, dtype))


def test_a_tensor_on_another_device_is_named_before_the_library_is_touched(stub):
    torch = pytest.importorskip("torch")
    c, rec, _ = stub
    a, b = np.eye(3), np.ones((3, 2))
    for call in (lambda t: c.solve(t, b), lambda t: c.solve(t, b, assume="pos"), lambda t: c.cholesky(t)):
        with pytest.raises(ValueError, match="tensor is on cuda:1, context is on cuda:0"):
            call(on_gpu(torch, 1, (3, 3)))
    for call in (lambda t: c.rbf_system(t, 1), lambda t: c.rbf_fit(t, np.ones(4), 1), lambda t: c.sandwich_diag(t, a)):
        with pytest.raises(ValueError, match="tensor is on cuda:1, context is on cuda:0"):
            call(on_gpu(torch, 1, (4, 3)))
    with pytest.raises(ValueError, match="tensor is on cuda:1, context is on cuda:0"):
        c.mvn_sample(4, on_gpu(torch, 1, (3, 2)))
    assert not rec.calls and not rec.log
