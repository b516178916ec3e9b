"""The symmetric eigensolver on the device (corrla_eigh_*, Context.eigh, Context.eigh_solve) on a real MI355X.
tests/test_eigh_plan.py pins on the CPU what plan each shape of this file gets (GPU_CALLS there): every family of
tests/eigh_reference.py at n = 1, 2, 5, 63, 64 (the small route and its edge), 65 (three blocks, the last one column wide, a
bye), 96 (three full blocks), 129 (five), 200 (a partial last block) and 257 (nine).

Every device call is made with padded lda / ldv whose gaps hold a sentinel, with the sentinel in the strict upper triangle of
a, and a has to come back bitwise unchanged.  Per case: w ascending; the sign convention; residual, orthogonality and the
distance to numpy.linalg.eigh within the working bounds -- 4 x what the numpy restatement of the algorithm recorded for the
case in tests/golden/eigh_cases.json (tools/record_eigh_cases.py), never above the fixed caps 64 n u |A|_F, 32 n u and
4 n u |A|_F; the sweeps within the recorded ones + 3; a second call and the host entry give the same bits; the zero and
diagonal matrices take no sweep."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import eigh_reference as R
from tests.test_eigh_plan import GPU_CALLS, SMALL_N

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e300
ENUMERIC, EINVAL = 5, 1
PAD_A, PAD_V = 3, 2


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


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@functools.lru_cache(maxsize=None)
def _case(name, n):
    a = R.family(name, n)
    return a, np.linalg.eigh(a)[0]   # numpy.linalg.eigh, as recorded: eigvalsh takes another LAPACK path and differs by ulps


def _poisoned(a, pad):
    """a in an array with `pad` more columns: the sentinel in the gaps and in the strict upper triangle"""
    n = a.shape[0]
    whole = np.full((n, n + pad), SENTINEL)
    whole[:, :n] = a
    whole[:, :n][np.triu_indices(n, 1)] = SENTINEL
    return whole


def last_eigh(ctx):
    route, sweeps, info = C.c_int(0), C.c_int(0), C.c_int64(0)
    off, shift = C.c_double(0.0), C.c_double(0.0)
    assert ctx._lib.corrla_ctx_last_eigh(ctx._h, C.byref(route), C.byref(sweeps), C.byref(off), C.byref(shift), C.byref(info)) == 0
    assert ctx._lib.corrla_ctx_last_eigh(ctx._h, None, None, None, None, None) == 0  # any pointer may be NULL
    return route.value, sweeps.value, off.value, shift.value, info.value


def eigh_dev(torch, ctx, a):
    """the raw device entry on the poisoned, padded a -> (status, w, v) as numpy; asserts what must stay untouched"""
    n = a.shape[0]
    src = _poisoned(a, PAD_A)
    wa = torch.from_numpy(src).cuda()
    wv = torch.full((n, n + PAD_V), SENTINEL, dtype=torch.float64, device="cuda")
    w = torch.full((n + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = ctx._lib.corrla_eigh_dev_f64(ctx._h, wa.data_ptr(), n, n + PAD_A, w.data_ptr(), wv.data_ptr(), n + PAD_V)
    torch.cuda.synchronize()
    assert np.array_equal(wa.cpu().numpy(), src), "a was written"
    assert bool((wv[:, n:] == SENTINEL).all()) and bool((w[n:] == SENTINEL).all()), "a padding element of v or w was written"
    return rc, w[:n].cpu().numpy(), wv[:, :n].cpu().numpy()


def eigh_host(ctx, a):
    n = a.shape[0]
    src = _poisoned(a, PAD_A)
    wa = src.copy()
    wv = np.full((n, n + PAD_V), SENTINEL)
    w = np.full(n + 2, SENTINEL)
    rc = ctx._lib.corrla_eigh_f64(ctx._h, wa.ctypes.data, n, n + PAD_A, w.ctypes.data, wv.ctypes.data, n + PAD_V)
    assert np.array_equal(wa, src), "a was written"
    assert np.all(wv[:, n:] == SENTINEL) and np.all(w[n:] == SENTINEL), "a padding element of v or w was written"
    return rc, w[:n].copy(), wv[:, :n].copy()


@pytest.mark.parametrize("name,n", GPU_CALLS)
def test_decomposition_within_the_working_bounds(torch, ctx, golden, name, n):
    a, w_lapack = _case(name, n)
    rec = golden[R.case_id(name, n)]
    rc, w, v = eigh_dev(torch, ctx, a)
    assert rc == 0
    route, sweeps, off, shift, info = last_eigh(ctx)
    got = R.ratios(a, w, v, w_lapack)
    bounds = {key: R.working_bound(rec[key], key) for key in R.CAPS}
    print(f"{name}-{n}: sweeps {sweeps} (recorded {rec['sweeps']}) off {off:.2e} "
          + " ".join(f"{key} {got[key]:.3f} (recorded {rec[key]:.3f}, bound {bounds[key]:.3f})" for key in R.CAPS))
    assert route == (1 if n <= SMALL_N else 2) and info == 0
    assert shift == R.shift_of(a) or abs(shift - R.shift_of(a)) <= 4 * n * R.U * shift   # the sums run in another order
    assert off <= 2.0 * np.sqrt(n) * R.U
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(v))
    assert np.all(np.diff(w) >= 0.0), "w is not ascending"
    assert R.sign_convention_holds(v)
    for key in R.CAPS:
        assert got[key] <= bounds[key] <= R.CAPS[key], (key, got[key], bounds[key])
    assert sweeps <= rec["sweeps"] + 3
    if name in ("zero", "diag"):
        assert sweeps == 0 and np.array_equal(np.sort(np.diag(a)), w)
    # a second call, and the host entry, give the same bits
    rc2, w2, v2 = eigh_dev(torch, ctx, a)
    assert rc2 == 0 and np.array_equal(w2, w) and np.array_equal(v2, v)
    rc3, w3, v3 = eigh_host(ctx, a)
    assert rc3 == 0 and np.array_equal(w3, w) and np.array_equal(v3, v)
    assert last_eigh(ctx) == (route, sweeps, off, shift, 0)


@pytest.mark.parametrize("n", [5, 64, 65, 129])
def test_context_eigh_from_numpy_and_tensors(torch, ctx, n):
    a, _ = _case("gauss", n)
    _, w_raw, v_raw = eigh_dev(torch, ctx, a)
    w, v = ctx.eigh(a)
    assert isinstance(w, np.ndarray) and isinstance(v, np.ndarray) and w.shape == (n,) and v.shape == (n, n)
    assert np.array_equal(w, w_raw) and np.array_equal(v, v_raw)
    wt, vt = ctx.eigh(torch.tensor(a, device="cuda"))
    assert wt.is_cuda and vt.is_cuda and np.array_equal(wt.cpu().numpy(), w) and np.array_equal(vt.cpu().numpy(), v)
    assert ctx.last_eigh_route == ("small" if n <= SMALL_N else "blocked")
    assert set(ctx.last_eigh_info) == {"info", "sweeps", "off", "shift", "dropped"} and ctx.last_eigh_info["info"] == 0
    assert ctx.last_eigh_info["dropped"] is None
    assert ctx.eigh(a.astype(np.float32))[0].dtype == np.float64
    with pytest.raises(ValueError):
        ctx.eigh(a[:, :-1]) if n > 1 else ctx.eigh(np.zeros((0, 0)))


@pytest.mark.parametrize("n", [5, 65])
def test_non_finite_entries(torch, ctx, n):
    a, _ = _case("gauss", n)
    _, w_ok, v_ok = eigh_dev(torch, ctx, a)
    # a NaN above the diagonal changes nothing: the strict upper triangle is never read
    up = a.copy()
    up[0, n - 1] = np.nan
    w, v = ctx.eigh(up)
    assert np.array_equal(w, w_ok) and np.array_equal(v, v_ok)
    # a NaN or an infinity in the lower triangle ends the call, and a host caller's arrays stay as they were
    for bad in (np.nan, np.inf):
        low = a.copy()
        low[n - 1, 0] = bad
        wv, ww = np.full((n, n), SENTINEL), np.full(n, SENTINEL)
        rc = ctx._lib.corrla_eigh_f64(ctx._h, low.ctypes.data, n, n, ww.ctypes.data, wv.ctypes.data, n)
        assert rc == ENUMERIC and np.all(wv == SENTINEL) and np.all(ww == SENTINEL)
        assert last_eigh(ctx)[4] == 1
        with pytest.raises(RuntimeError):
            ctx.eigh(torch.tensor(low, device="cuda"))
        assert ctx.last_eigh_info["info"] == 1
    # the context goes on working
    w, v = ctx.eigh(a)
    assert np.array_equal(w, w_ok) and np.array_equal(v, v_ok)


def test_rejected_arguments(ctx):
    n = 4
    a, w, v = np.eye(n), np.empty(n), np.empty((n, n))
    lib, h = ctx._lib, ctx._h
    for fn in (lib.corrla_eigh_f64, lib.corrla_eigh_dev_f64):
        assert fn(h, a.ctypes.data, 0, n, w.ctypes.data, v.ctypes.data, n) == EINVAL
        assert fn(h, a.ctypes.data, n, n - 1, w.ctypes.data, v.ctypes.data, n) == EINVAL
        assert fn(h, a.ctypes.data, n, n, w.ctypes.data, v.ctypes.data, n - 1) == EINVAL
        assert fn(h, None, n, n, w.ctypes.data, v.ctypes.data, n) == EINVAL
        assert fn(h, a.ctypes.data, n, n, None, v.ctypes.data, n) == EINVAL
        assert fn(h, a.ctypes.data, n, n, w.ctypes.data, None, n) == EINVAL
        assert fn(h, a.ctypes.data, 32769, 32769, w.ctypes.data, v.ctypes.data, 32769) == EINVAL
        assert fn(h, a.ctypes.data, n, n, w.ctypes.data, a.ctypes.data, n) == EINVAL   # v over a


def _solve_reference(a, b, *, rcond=None, reg=None):
    """the rule of eigh_solve in numpy on LAPACK's decomposition -> (x, dropped)"""
    w, v = np.linalg.eigh(a)
    if reg is not None:
        return v @ ((np.where(w < 0, -1.0, 1.0) / (np.abs(w) + reg))[:, None] * (v.T @ b)), 0
    keep = np.abs(w) > (a.shape[0] * 2.0 ** -52 if rcond is None else rcond) * np.abs(w).max()
    f = np.where(keep, 1.0 / np.where(keep, w, 1.0), 0.0)
    return v @ (f[:, None] * (v.T @ b)), int((~keep).sum())


@pytest.mark.parametrize("n", [63, 129])
def test_eigh_solve_both_rules(torch, ctx, n):
    rng = np.random.default_rng(n)
    b = rng.standard_normal((n, 3))
    # the rank n / 3 Gram matrix: the default rule drops the null directions.  The eigenvalues kept are of the order of |a|,
    # so x carries the eigensolver's absolute error n u |a| relative to them: 64 n u |a| |a^+| |x| bounds the difference with
    # the same factor the residual cap has.
    a, w_lapack = _case("gram", n)
    x, dropped = _solve_reference(a, b)
    got = ctx.eigh_solve(a, b)
    assert isinstance(got, np.ndarray) and got.shape == b.shape
    assert dropped == n - n // 3 and ctx.last_eigh_info["dropped"] == dropped
    kept = w_lapack[np.abs(w_lapack) > n * 2.0 ** -52 * np.abs(w_lapack).max()]
    bound = 64 * n * R.U * np.abs(w_lapack).max() / np.abs(kept).min()
    err = np.linalg.norm(got - x) / np.linalg.norm(x)
    print(f"gram-{n}: default rule, relative difference {err:.2e}, bound {bound:.2e}")
    assert err <= bound
    gt = ctx.eigh_solve(torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda"))
    assert gt.is_cuda and np.array_equal(gt.cpu().numpy(), got)
    x0 = ctx.eigh_solve(a, b[:, 0])   # a vector: the products may take another route, the decomposition is the same
    assert x0.shape == (n,) and np.linalg.norm(x0 - got[:, 0]) <= bound * np.linalg.norm(got[:, 0])
    # the regularised rule on the well-conditioned indefinite matrix: every direction is kept
    a, w_lapack = _case("gauss", n)
    x, _ = _solve_reference(a, b, reg=1e-14)
    got = ctx.eigh_solve(a, b, reg=1e-14)
    bound = 64 * n * R.U * np.abs(w_lapack).max() / np.abs(w_lapack).min()
    err = np.linalg.norm(got - x) / np.linalg.norm(x)
    print(f"gauss-{n}: reg rule, relative difference {err:.2e}, bound {bound:.2e}")
    assert err <= bound and ctx.last_eigh_info["dropped"] == 0
    with pytest.raises(ValueError):
        ctx.eigh_solve(a, b, rcond=1e-8, reg=1e-14)
    with pytest.raises(ValueError):
        ctx.eigh_solve(a, b[:-1])
