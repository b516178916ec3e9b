"""Gaussian kernel density estimates on the GPU: Context.kde_eval / kde_nll and KdeRv(device=True) over them
(corrla_kde_eval_*, corrla_kde_nll_*, csrc/kde_kernels.hpp).  Run with -m gpu on an MI355X.

Every case runs in f32 and f64, with host pointers (numpy) and with CUDA tensors.  tests/test_kde_plan.py pins on the CPU
what plan each call of this file gets (GPU_CALLS there); the shapes come from its tables: one axis at a time from the base
case n_q = 2 QT + 3, n_s = 2 SC + 7, n_h = 3, and one case whose few points meet supports in four splits, the last of 5.
The reference is tests/golden/kde/kde_known.npz (make_kde_golden.py: mpmath, 50 digits, rounded once to f64) on values that
are exact in f32, so the same fixture judges both types and contributes only its final rounding.  Neither mpmath nor scipy
is needed here.

Bounds, from the operation order of kde_kernels.hpp.  u = 2^-24 (f32) / 2^-53 (f64), v = 2^-53, L = 1 for v_exp_f32 (f32)
and 2 for the library exp (f64) and erfc (both): a function of L ulp is off by 2 L u relatively.
With d = fl(x - s) (u), d2 = fl(d d) (3 u in all), d* the minimum of the same bit patterns, a = fl(d* - d2), c the rounded
exponent scale (at most 2 u) and e = fl(a c), the exponent -(t - t*) of a pair is off by at most
    delta = u (3 (t + t*) + 4 |t - t*|) <= 7 u (t + t*),
and K = exp(e) by the factor e^delta (1 + 2 L u): relatively rho = delta / (1 - delta) + 2 L u (1 + delta / (1 - delta)).
S = sum_j K_j is summed in index order in the type, n_s u relatively (all terms positive), the splits in f64; v_exp_f32
flushes results below 2^-126, n_s 2^-126 absolutely against S >= 1.  With the weights w_j = K_j / S, which sum to 1:
    E_S    = sum_j w_j rho_j + n_s u + n_s tiny                   (far supports cost nothing: t e^-t is bounded)
    logpdf = -t* + ln S - ln(n_s h sqrt(2 pi))  off by  3 u t* + E_S / (1 - E_S) + 8 v (t* + |ln S| + |ln norm|), + u |logpdf|
             for the store in the type;  pdf relatively by the same without the last term, + u, or a denormal
    cdf    z = fl(-d r), r the rounded 1 / (h sqrt 2): 5 u relatively; |z erfc'(z) / erfc(z)| <= 2 t + 1; so a term is off by
             5 u (2 t + 1) + 4 u relatively, the sum by the weighted mean of that + n_s u, the store by u
    nll    the sum of its points' logpdf bounds (without the store), + n_t v sum_i |logpdf_i| for the f64 tree
    dnll   R_i = 2 (t* + mean_w(t - t*)); the mean sum(e K) / sum(K) is off by
             sum_j w_j (delta_j + |e_j| (rho_j + n_s u)) + |mean| E_S,
           t* by 3 u t*;  dnll = -sum_i (R_i - 1) / h carries the sum of 2 (...) / h, + n_t v sum_i |R_i - 1| / h for the tree.
The accuracy points lie within 4 bandwidths of their nearest support (t* <= 8; the generator asserts it); the far point,
60 h_0 beyond the largest support, is judged by the same formulas with its own t*: its plain f64 density is zero, its
logpdf and its share of nll are finite.  A dropped or doubled support moves a sum by O(1 / n_s) of its scale, orders above
n_s u, so the slack hides nothing.
The exact cases compare bitwise: the cdf of a point equal to all of 128 coincident supports is 0.5; the same call twice gives
the same bits, on the split route and for nll / dnll too; kde_nll with 64 bandwidths equals 64 calls with one."""
import functools
import os

import numpy as np
import pytest

from tests.test_kde_plan import BASE, EXACT_CDF, GPU_CALLS, HG, HL, MAX_H, QT, SC, SPLIT_CASE

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
KINDS = ("host", "dev")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kde", "kde_known.npz")
V = 2.0 ** -53
SEEDED = dict(seed=20241008, mean=5.25, std=10.0, n_s=71, n_t=131)


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


def _u(dtype):
    return 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    assert tuple(int(v) for v in z["consts"]) == (QT, SC, HG, HL, MAX_H), "the fixture was built for other tile sizes: regenerate it"
    return z


@functools.lru_cache(maxsize=None)
def known(n_q, n_s):
    """the fixture of one data set: x, s (float32 values), h (its bandwidths), pdf, cdf, logpdf at h[0], nll, dnll over h"""
    z = golden()
    d = {k: z[f"{n_q}_{n_s}_{k}"] for k in ("x", "s", "h", "pdf", "cdf", "logpdf", "nll", "dnll")}
    for a in d.values():
        a.setflags(write=False)
    return d


def _pair_terms(x, s, h):
    """t (n_q, n_s), t* (n_q), the weights w and S in f64"""
    d = x.astype(np.float64)[:, None] - s.astype(np.float64)[None, :]
    t = d * d / (2.0 * h * h)
    tstar = t.min(axis=1)
    kk = np.exp(tstar[:, None] - t)
    ssum = kk.sum(axis=1)
    return d, t, tstar, kk / ssum[:, None], ssum


def _rho(t, tstar, u, lib):
    delta = u * (3.0 * (t + tstar[:, None]) + 4.0 * (t - tstar[:, None]))
    assert delta.max() < 0.5
    grow = delta / (1.0 - delta)
    return delta, grow + 2.0 * lib * u * (1.0 + grow)


def _sum_bound(w, rho, n_s, dtype):
    return (w * rho).sum(axis=1) + n_s * _u(dtype) + n_s * float(np.finfo(dtype).tiny)


def eval_bounds(x, s, h, dtype, what, ref):
    """the componentwise bound of kde_eval (module docstring)"""
    u, n_s = _u(dtype), s.shape[0]
    d, t, tstar, w, ssum = _pair_terms(x, s, h)
    if what == "cdf":
        z = -d / (h * np.sqrt(2.0))
        import math
        term = np.frompyfunc(math.erfc, 1, 1)(z).astype(np.float64)
        wc = term / term.sum(axis=1)[:, None]
        rel = (wc * (5.0 * u * (2.0 * t + 1.0) + 4.0 * u)).sum(axis=1) + n_s * u + 4.0 * V
        return (rel + u) * np.abs(ref) + float(np.finfo(dtype).smallest_subnormal)
    _, rho = _rho(t, tstar, u, 1 if dtype == np.float32 else 2)
    e_s = _sum_bound(w, rho, n_s, dtype)
    assert e_s.max() < 0.5
    lognorm = np.log(n_s * h * np.sqrt(2.0 * np.pi))
    core = 3.0 * u * tstar + e_s / (1.0 - e_s) + 8.0 * V * (tstar + np.abs(np.log(ssum)) + abs(lognorm))
    if what == "logpdf":
        return core + u * np.abs(ref)
    return (core / (1.0 - core) + u) * np.abs(ref) + float(np.finfo(dtype).smallest_subnormal)


@functools.lru_cache(maxsize=None)
def known_eval_bounds(n_q, n_s, dtype, what):
    """the bound of kde_eval at the first bandwidth of a data set of the fixture: computed once and shared"""
    k = known(n_q, n_s)
    return eval_bounds(k["x"], k["s"], float(k["h"][0]), dtype, what, k[what])


@functools.lru_cache(maxsize=None)
def nll_bounds(n_q, n_s, b, dtype):
    """-> (bound of nll, bound of dnll) for bandwidth b of the data set: computed once and shared"""
    k = known(n_q, n_s)
    x, s, h = k["x"], k["s"], float(k["h"][b])
    u = _u(dtype)
    _, t, tstar, w, ssum = _pair_terms(x, s, h)
    delta, rho = _rho(t, tstar, u, 1 if dtype == np.float32 else 2)
    e_s = _sum_bound(w, rho, n_s, dtype)
    lognorm = np.log(n_s * h * np.sqrt(2.0 * np.pi))
    lp = -tstar + np.log(ssum) - lognorm
    lp_err = 3.0 * u * tstar + e_s / (1.0 - e_s) + 8.0 * V * (tstar + np.abs(np.log(ssum)) + abs(lognorm))
    nll_b = lp_err.sum() + n_q * V * np.abs(lp).sum() + V * abs(float(k["nll"][b]))
    e = t - tstar[:, None]
    mean = (w * e).sum(axis=1)
    mean_err = (w * (delta + e * (rho + n_s * u))).sum(axis=1) + mean * e_s / (1.0 - e_s)
    r = 2.0 * (tstar + mean)
    r_err = 2.0 * (3.0 * u * tstar + mean_err) + 8.0 * V * np.abs(r)
    dnll_b = r_err.sum() / h + n_q * V * np.abs((r - 1.0) / h).sum() + V * abs(float(k["dnll"][b]))
    return float(nll_b), float(dnll_b)


def _give(torch, a, kind):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if kind == "dev" else a


def _strided(torch, a, inc, kind):
    """`a` at element stride inc in a buffer whose base is one element off a 16-byte boundary"""
    per16 = 16 // a.itemsize
    if kind == "dev":
        buf = torch.full((per16 + 1 + a.shape[0] * inc,), float("nan"), dtype=torch.from_numpy(a[:1]).dtype, device="cuda")
        off = next(o for o in range(1, 2 * per16) if (buf.data_ptr() + o * a.itemsize) % 16 == a.itemsize)
        view = buf[off:off + a.shape[0] * inc:inc]
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        assert view.data_ptr() % 16 == a.itemsize and view.stride(0) == inc
        return view
    buf = np.full(2 * per16 + 1 + a.shape[0] * inc, np.nan, dtype=a.dtype)
    off = next(o for o in range(1, 2 * per16) if (buf.ctypes.data + o * a.itemsize) % 16 == a.itemsize)
    view = buf[off:off + a.shape[0] * inc:inc]
    view[:] = a
    assert view.ctypes.data % 16 == a.itemsize and view.strides[0] == inc * a.itemsize
    return view


EVAL_CALLS = sorted({c[:2] for c in GPU_CALLS})


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("what", ("pdf", "cdf", "logpdf"))
@pytest.mark.parametrize("case", EVAL_CALLS, ids=lambda c: "-".join(str(v) for v in c))
def test_eval_against_the_fixture(ctx, torch, case, what, dtype, kind):
    n_q, n_s = case
    k = known(n_q, n_s)
    x, s, h = k["x"].astype(dtype), k["s"].astype(dtype), float(k["h"][0])
    got = ctx.kde_eval(_give(torch, x, kind), _give(torch, s, kind), h, what)
    assert (type(got) is np.ndarray) == (kind == "host") and tuple(got.shape) == (n_q,)
    got = _np(got)
    assert got.dtype == dtype and np.all(np.isfinite(got))
    assert ctx.last_kde_route() == ("split" if n_s > SC else "single")
    ref = k[what]
    bound = known_eval_bounds(n_q, n_s, dtype, what)
    err = np.abs(got.astype(np.float64) - ref)
    worst = int(np.argmax(err / bound))
    print(f"{what} {case} {np.dtype(dtype).name} {kind}: worst err / bound = {err[worst] / bound[worst]:.3g} at point {worst} (err {err[worst]:.3g})")
    assert np.all(err <= bound), (worst, err[worst], bound[worst])
    if n_q > 1 and what == "logpdf":                      # the far point: the plain f64 density is zero, the log-density finite
        assert k["pdf"][-1] == 0.0 and np.isfinite(got[-1]) and got[-1] < -1700.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("case", GPU_CALLS, ids=lambda c: "-".join(str(v) for v in c))
def test_nll_against_the_fixture(ctx, torch, case, dtype, kind):
    n_q, n_s, n_h = case
    k = known(n_q, n_s)
    x, s, h = k["x"].astype(dtype), k["s"].astype(dtype), k["h"][:n_h]
    nll, dnll = ctx.kde_nll(_give(torch, x, kind), _give(torch, s, kind), h)
    assert (type(nll) is np.ndarray) == (kind == "host")
    nll, dnll = _np(nll), _np(dnll)
    assert nll.dtype == dnll.dtype == np.float64 and nll.shape == dnll.shape == (n_h,)
    assert np.all(np.isfinite(nll)) and np.all(np.isfinite(dnll))
    for b in range(n_h):
        nb, db = nll_bounds(n_q, n_s, b, dtype)
        en, ed = abs(nll[b] - k["nll"][b]), abs(dnll[b] - k["dnll"][b])
        print(f"nll {case} {np.dtype(dtype).name} {kind} h = {h[b]:.4g}: err / bound = {en / nb:.3g} (nll), {ed / db:.3g} (dnll)")
        assert en <= nb and ed <= db, (b, en, nb, ed, db)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_strided_inputs_with_bases_off_a_16_byte_boundary(ctx, torch, dtype, kind):
    """strides 3 (points) and 2 (supports), each base one element off a 16-byte boundary: the same bits as the contiguous call"""
    n_q, n_s, n_h = BASE
    k = known(n_q, n_s)
    x, s, h = k["x"].astype(dtype), k["s"].astype(dtype), k["h"][:n_h]
    xs, ss = _strided(torch, x, 3, kind), _strided(torch, s, 2, kind)
    xc, sc = _give(torch, x, kind), _give(torch, s, kind)
    for what in ("pdf", "cdf", "logpdf"):
        assert np.array_equal(_np(ctx.kde_eval(xs, ss, float(h[0]), what)), _np(ctx.kde_eval(xc, sc, float(h[0]), what)))
    a, b = ctx.kde_nll(xs, ss, h), ctx.kde_nll(xc, sc, h)
    assert np.array_equal(_np(a[0]), _np(b[0])) and np.array_equal(_np(a[1]), _np(b[1]))
    err = np.abs(_np(ctx.kde_eval(xs, ss, float(h[0]), "logpdf")).astype(np.float64) - k["logpdf"])
    assert np.all(err <= known_eval_bounds(n_q, n_s, dtype, "logpdf"))
    # an n x 1 column, as the reference's column matrices, comes back as one
    col = ctx.kde_eval(xc.reshape(-1, 1), sc.reshape(-1, 1), float(h[0]), "pdf")
    assert tuple(col.shape) == (n_q, 1) and np.array_equal(_np(col).ravel(), _np(ctx.kde_eval(xc, sc, float(h[0]), "pdf")))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_cdf_of_a_point_on_128_coincident_supports_is_exactly_half(ctx, torch, dtype, kind):
    n_q, n_s, _ = EXACT_CDF
    s = np.full(n_s, 3.25, dtype=dtype)
    got = _np(ctx.kde_eval(_give(torch, s[:n_q].copy(), kind), _give(torch, s, kind), 0.7, "cdf"))
    assert got.dtype == dtype and got.tobytes() == np.array([0.5], dtype=dtype).tobytes()
    # ... and the density there is the kernel's peak: every term is exactly 1
    pdf = _np(ctx.kde_eval(_give(torch, s[:n_q].copy(), kind), _give(torch, s, kind), 0.7, "pdf"))
    assert abs(float(pdf[0]) - 1.0 / (0.7 * np.sqrt(2.0 * np.pi))) <= 4.0 * _u(dtype)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("case", (BASE, SPLIT_CASE), ids=("base", "split"))
def test_the_same_call_twice_gives_the_same_bits(ctx, torch, case, dtype, kind):
    n_q, n_s, n_h = case
    k = known(n_q, n_s)
    x, s, h = _give(torch, k["x"].astype(dtype), kind), _give(torch, k["s"].astype(dtype), kind), k["h"][:n_h]
    for what in ("pdf", "cdf", "logpdf"):
        assert _np(ctx.kde_eval(x, s, float(h[0]), what)).tobytes() == _np(ctx.kde_eval(x, s, float(h[0]), what)).tobytes()
    assert ctx.last_kde_route() == "split"
    a, b = ctx.kde_nll(x, s, h), ctx.kde_nll(x, s, h)
    assert _np(a[0]).tobytes() == _np(b[0]).tobytes() and _np(a[1]).tobytes() == _np(b[1]).tobytes()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_64_bandwidths_equal_64_calls_of_one(ctx, torch, dtype, kind):
    """the grouping must not change a sum"""
    n_q, n_s, _ = BASE
    k = known(n_q, n_s)
    x, s, h = _give(torch, k["x"].astype(dtype), kind), _give(torch, k["s"].astype(dtype), kind), k["h"][:MAX_H]
    nll, dnll = (_np(v) for v in ctx.kde_nll(x, s, h))
    for b in range(MAX_H):
        one = ctx.kde_nll(x, s, h[b:b + 1])
        assert _np(one[0]).tobytes() == nll[b:b + 1].tobytes() and _np(one[1]).tobytes() == dnll[b:b + 1].tobytes(), b


def reference_dnll(x, s, h):
    """d nll / d h of the reference's likelihood in extended precision (longdouble), in the stabilised form so that it exists
    at small h: g(h) = -sum_i (R_i - 1) / h"""
    xl, sl, hl = np.asarray(x, dtype=np.longdouble), np.asarray(s, dtype=np.longdouble), np.longdouble(h)
    d2 = (xl[:, None] - sl[None, :]) ** 2
    kk = np.exp(-(d2 - d2.min(axis=1)[:, None]) / (2 * hl * hl))
    r = (d2 / (hl * hl) * kk).sum(axis=1) / kk.sum(axis=1)
    return float(-((r - 1) / hl).sum())


def seeded_case(dtype):
    rng = np.random.default_rng(SEEDED["seed"])
    s = rng.normal(SEEDED["mean"], SEEDED["std"], SEEDED["n_s"]).astype(dtype)
    x = rng.normal(SEEDED["mean"], SEEDED["std"], SEEDED["n_t"]).astype(dtype)
    return s, x


def assert_brackets_the_minimum(s, x, h, rtol):
    """the precondition on the reference alone -- its derivative changes sign exactly once on a 400-point log grid over
    [0.05, 200] -- then g(h (1 - 2 rtol)) < 0 < g(h (1 + 2 rtol)): no tolerance beyond the caller's own rtol"""
    g = np.array([reference_dnll(x, s, v) for v in np.geomspace(0.05, 200.0, 400)])
    assert np.count_nonzero(np.sign(g[1:]) != np.sign(g[:-1])) == 1 and g[0] < 0.0 < g[-1]
    lo, hi = reference_dnll(x, s, h * (1.0 - 2.0 * rtol)), reference_dnll(x, s, h * (1.0 + 2.0 * rtol))
    assert lo < 0.0 < hi, (h, lo, hi)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_kde_rv_on_the_device(ctx, torch, dtype):
    """KdeRv(device=True) with CUDA tensors returns tensors; est_bandwidth on the seeded case brackets the reference's minimum"""
    from corrla_rs_amd.callers import KdeRv
    s, x = seeded_case(dtype)
    st, xt = torch.from_numpy(s).cuda(), torch.from_numpy(x).cuda()
    rv = KdeRv(1.0, st, device=True, ctx=ctx)
    for f in (rv.pdf, rv.cdf, rv.logpdf):
        out = f(xt)
        assert torch.is_tensor(out) and out.is_cuda and out.dtype == xt.dtype and tuple(out.shape) == (x.shape[0],)
    assert type(rv.nll(xt)) is float and np.isfinite(rv.nll(xt, 1e-3))
    rtol = 1e-6
    h = rv.est_bandwidth(xt, rtol=rtol)
    assert 1e-9 <= h <= 1000.0 and rv.bandwidth == h and rv.n_nll_calls <= 12
    assert_brackets_the_minimum(s, x, h, rtol)
    # numpy input with device=True takes the device too and returns numpy
    rv2 = KdeRv(1.0, s, device=True, ctx=ctx)
    assert type(rv2.pdf(x)) is np.ndarray and rv2.est_bandwidth(x, rtol=rtol) == h       # the same kernels, the same bits
