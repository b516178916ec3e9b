"""Radial-basis-function kernel matrices on the GPU: Context.rbf_matrix / rbf_apply and RbfInterp(device=True) over them
(corrla_rbf_matrix_*, corrla_rbf_apply_*, csrc/rbf_kernels.hpp).  Run with -m gpu on an MI355X.

Every case runs in f32 and f64, with host pointers (numpy) and with CUDA tensors.  tests/test_rbf_plan.py pins on the CPU
what plan each call of this file gets (GPU_CALLS there); the shapes come from its tables: one axis at a time from the base
case n_q = 2 BM + 3, n_s = 2 KC + 7, dim = 3, n_rhs = 17, poly_degree = 1, and one case whose supports are split.

Bounds.  u = 2^-24 (f32) / 2^-53 (f64); the reference is the numpy formula on the same stored values, in f64 for the f32 runs
and in numpy's extended precision (longdouble) for the f64 runs: an f64 reference carries an error of the size of the bound
it is to judge (tests/test_gpu_pca_apply.py, for the same reason).  With t = eps^2 s for the Gaussian and 0 otherwise:
  apply   |out - ref|_ic <= (n_s + n_poly + 2 dim + 12 + t_max (dim + 5)) u (|Phi| |W_rbf| + |P| |W_poly|)_ic
  matrix  |Phi^ - Phi|_ij <= (2 dim + 12 + t_ij (dim + 5)) u |Phi_ij|
-- the length of the dot product, (dim + 2) u for the squared distance, its propagation through sqrt, the cube and exp (a
relative error delta in t gives t delta in exp(-t)), and library functions of 2 ulp.  A dropped or doubled support is
O(1 / n_s) of the scale, so the slack of the bound hides nothing.  The Gaussian eps is chosen so that t <= 12.
The exact cases compare bitwise: phi == 1 (kernels 2 and 4 with eps = 0) with integer W gives the column sums of W_rbf;
rbf_matrix(x, x) equals its transpose, has the diagonal phi(0) and zeros where two rows coincide."""
import functools

import numpy as np
import pytest

from tests.test_rbf_plan import BASE, BM, EXACT_CALLS, GPU_CALLS, KC, MAX_DIM, SPLIT_CASE, poly_terms

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
KINDS = ("host", "dev")
KERNELS = (1, 2, 3, 4)
MQ_EPS = 0.75          # the multiquadric's eps: exactly representable in both types
T_MAX = 12.0           # the Gaussian's largest eps^2 s


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


def _wide(dtype):
    """the type the reference is evaluated in: f64 for the f32 cases, extended precision for the f64 cases"""
    return np.float64 if dtype == np.float32 else np.longdouble


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _sqdist(xq, xs, wide):
    a, b = np.asarray(xq, dtype=wide), np.asarray(xs, dtype=wide)
    s = np.zeros((a.shape[0], b.shape[0]), dtype=wide)
    for d in range(a.shape[1]):
        diff = a[:, d:d + 1] - b[None, :, d]
        s += diff * diff
    return s


def _phi(kernel, s, eps):
    if kernel == 1:
        return np.sqrt(s)
    if kernel == 2:
        return np.sqrt(1 + (eps * eps) * s)
    if kernel == 3:
        r = np.sqrt(s)
        return r * r * r
    return np.exp(-((eps * eps) * s))


def _poly(x, degree):
    """[x, 1] below degree 2, else [x, x_a x_b (a <= b, a outer), 1]; nothing for degree None"""
    if degree is None:
        return np.zeros((x.shape[0], 0), dtype=x.dtype)
    cols = [x]
    if degree >= 2:
        d = x.shape[1]
        cols += [x[:, a:a + 1] * x[:, b:b + 1] for a in range(d) for b in range(a, d)]
    return np.hstack(cols + [np.ones((x.shape[0], 1), dtype=x.dtype)])


def _eps(kernel, xq, xs, dtype):
    """the kernel parameter as the library will hold it (a value of dtype)"""
    if kernel in (1, 3):
        return 0.0
    if kernel == 2:
        return MQ_EPS
    s_max = float(_sqdist(xq, xs, np.float64).max())
    return float(dtype(np.sqrt(T_MAX / max(s_max, 1e-30)) * 0.999))


@functools.lru_cache(maxsize=None)
def _points(n_q, n_s, dim, n_rhs, degree, dtype):
    """queries, supports and coefficients as stored in dtype (read-only)"""
    rng = np.random.default_rng(100000 * n_q + 1000 * n_s + 10 * dim + n_rhs + (7 if degree is None else degree))
    xq = rng.standard_normal((n_q, dim)).astype(dtype)
    xs = rng.standard_normal((n_s, dim)).astype(dtype)
    w = rng.standard_normal((n_s + poly_terms(dim, degree), n_rhs)).astype(dtype)
    for a in (xq, xs, w):
        a.setflags(write=False)
    return xq, xs, w


@functools.lru_cache(maxsize=None)
def _apply_ref(n_q, n_s, dim, n_rhs, degree, dtype, kernel):
    """-> (eps, reference, componentwise bound), computed once per case and shared"""
    xq, xs, w = _points(n_q, n_s, dim, n_rhs, degree, dtype)
    wide = _wide(dtype)
    eps = _eps(kernel, xq, xs, dtype)
    s = _sqdist(xq, xs, wide)
    phi = _phi(kernel, s, wide(eps))
    p = _poly(np.asarray(xq, dtype=wide), degree)
    ww = np.asarray(w, dtype=wide)
    ref = phi @ ww[:n_s] + p @ ww[n_s:]
    scale = np.abs(phi) @ np.abs(ww[:n_s]) + np.abs(p) @ np.abs(ww[n_s:])
    t_max = float((eps * eps) * s.max()) if kernel == 4 else 0.0
    assert t_max <= 16.0
    bound = (n_s + poly_terms(dim, degree) + 2 * dim + 12 + t_max * (dim + 5)) * _u(dtype) * scale
    for a in (ref, bound):
        a.setflags(write=False)
    return eps, ref, bound


def _give(torch, a, kind):
    """a numpy view as the host or device operand with the SAME strides and the same offset of its base from a 16-byte
    boundary"""
    if kind == "host":
        return a
    it = a.itemsize
    span = (a.shape[0] - 1) * a.strides[0] // it + (a.shape[1] - 1) * a.strides[1] // it + 1
    off = (a.ctypes.data % 16) // it
    flat = torch.zeros(span + off, dtype=torch.float32 if a.dtype == np.float32 else torch.float64, device="cuda")
    t = torch.as_strided(flat, a.shape, tuple(s // it for s in a.strides), off)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert t.data_ptr() % 16 == a.ctypes.data % 16
    return t


def _check_apply(got, ref, bound, dtype, what):
    got = _np(got)
    assert got.dtype == dtype and got.shape == ref.shape, what
    err = np.abs(np.asarray(got, dtype=ref.dtype) - ref)
    worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print(f"{what}: worst error / bound = {worst:.3g}")
    assert np.all(err <= bound), (what, worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("case", GPU_CALLS, ids=lambda c: "-".join(str(v) for v in c))
def test_apply_within_its_bound(ctx, torch, case, dtype):
    n_q, n_s, dim, n_rhs, degree = case
    xq, xs, w = _points(*case, dtype)
    for kernel in KERNELS:
        eps, ref, bound = _apply_ref(*case, dtype, kernel)
        outs = {}
        for kind in KINDS:
            got = ctx.rbf_apply(_give(torch, xq, kind), _give(torch, xs, kind), _give(torch, w, kind), kernel, eps, poly_degree=degree)
            assert (type(got) is np.ndarray) == (kind == "host") and (kind == "host" or got.is_cuda)
            _check_apply(got, ref, bound, dtype, f"apply {case} kernel {kernel} {kind}")
            outs[kind] = _np(got)
        assert np.array_equal(outs["host"], outs["dev"])       # the same kernels on the same values


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_apply_on_padded_and_misaligned_operands(ctx, torch, dtype):
    """ldq = dim + 1, xs one element past a 16-byte boundary, ldw and ld_out padded; the padding of out keeps its sentinel.
    The entry is called as a C caller would: Context.rbf_apply always hands over a dense out."""
    from corrla_rs_amd import _lib as L
    n_q, n_s, dim, n_rhs, degree = BASE
    xq, xs, w = _points(*BASE, dtype)
    it = np.dtype(dtype).itemsize

    def flat(count, off):
        raw = np.zeros(count + 16 // it + 2, dtype=dtype)
        start = (-raw.ctypes.data % 16) // it + off
        return raw[start:start + count]
    xq_v = flat(n_q * (dim + 1), 0).reshape(n_q, dim + 1)[:, :dim]
    xs_v = flat(n_s * dim, 1).reshape(n_s, dim)
    w_v = flat(w.shape[0] * (n_rhs + 3), 0).reshape(w.shape[0], n_rhs + 3)[:, :n_rhs]
    xq_v[...], xs_v[...], w_v[...] = xq, xs, w
    assert xs_v.ctypes.data % 16 == it and xq_v.strides[0] == (dim + 1) * it
    ld_out, sentinel = n_rhs + 5, -777.0
    for kernel in KERNELS:
        eps, ref, bound = _apply_ref(*BASE, dtype, kernel)
        for kind in KINDS:
            a, b, c = (_give(torch, v, kind) for v in (xq_v, xs_v, w_v))
            if kind == "host":
                out = np.full((n_q, ld_out), sentinel, dtype=dtype)
                ptr = lambda v: v.ctypes.data  # noqa: E731
            else:
                out = torch.full((n_q, ld_out), sentinel, dtype=a.dtype, device="cuda")
                ptr = lambda v: v.data_ptr()  # noqa: E731
                torch.cuda.synchronize()
            entry = getattr(ctx._lib, "corrla_rbf_apply_" + ("dev_" if kind == "dev" else "") + ("f32" if dtype == np.float32 else "f64"))
            L.check(entry(ctx._h, ptr(a), n_q, dim + 1, ptr(b), n_s, dim, dim, kernel, eps, degree, ptr(c), n_rhs + 3, n_rhs, ptr(out),
                          ld_out))
            L.check(ctx._lib.corrla_ctx_synchronize(ctx._h))
            o = _np(out)
            assert np.all(o[:, n_rhs:] == sentinel), (kernel, kind)
            _check_apply(o[:, :n_rhs], ref, bound, dtype, f"padded apply kernel {kernel} {kind}")
            # the same values in dense arrays give the same bits: the layout changes no arithmetic
            assert np.array_equal(o[:, :n_rhs], ctx.rbf_apply(xq, xs, w, kernel, eps, poly_degree=degree))
        # the public surface takes the strided views as they lie
        assert np.array_equal(ctx.rbf_apply(xq_v, xs_v, w_v, kernel, eps, poly_degree=degree), o[:, :n_rhs])


MATRIX_SHAPES = sorted({(c[0], c[1], c[2]) for c in GPU_CALLS})


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("shape", MATRIX_SHAPES, ids=lambda c: "-".join(str(v) for v in c))
def test_matrix_within_its_bound(ctx, torch, shape, dtype):
    n_q, n_s, dim = shape
    xq, xs, _ = _points(n_q, n_s, dim, 1, None, dtype)
    wide = _wide(dtype)
    s = _sqdist(xq, xs, wide)
    for kernel in KERNELS:
        eps = _eps(kernel, xq, xs, dtype)
        ref = _phi(kernel, s, wide(eps))
        t = (eps * eps) * s if kernel == 4 else 0 * s
        bound = (2 * dim + 12 + t * (dim + 5)) * _u(dtype) * np.abs(ref)
        outs = {}
        for kind in KINDS:
            got = ctx.rbf_matrix(_give(torch, xq, kind), _give(torch, xs, kind), kernel, eps)
            assert (type(got) is np.ndarray) == (kind == "host")
            g = _np(got)
            assert g.dtype == dtype and g.shape == (n_q, n_s)
            err = np.abs(np.asarray(g, dtype=wide) - ref)
            worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
            print(f"matrix {shape} kernel {kernel} {kind}: worst error / bound = {worst:.3g}")
            assert np.all(err <= bound), (shape, kernel, kind, worst)
            outs[kind] = g
        assert np.array_equal(outs["host"], outs["dev"])


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("case", EXACT_CALLS, ids=lambda c: "-".join(str(v) for v in c))
def test_phi_identically_one_gives_the_column_sums_exactly(ctx, torch, case, dtype):
    """kernels 4 and 2 with eps = 0: every support is counted once across chunk, split and column-group boundaries, and the
    padded slots contribute nothing"""
    n_q, n_s, dim, n_rhs, degree = case
    rng = np.random.default_rng(n_s * 100 + n_rhs)
    xq, xs = rng.standard_normal((n_q, dim)).astype(dtype), rng.standard_normal((n_s, dim)).astype(dtype)
    w = rng.integers(-3, 4, (n_s, n_rhs)).astype(dtype)
    want = np.broadcast_to(w.sum(axis=0, dtype=np.float64).astype(dtype), (n_q, n_rhs))
    for kernel in (2, 4):
        for kind in KINDS:
            got = _np(ctx.rbf_apply(_give(torch, xq, kind), _give(torch, xs, kind), _give(torch, w, kind), kernel, 0.0))
            assert np.array_equal(got, want), (case, kernel, kind)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("dim", (3, 17))
def test_matrix_of_a_point_set_with_itself_is_exactly_symmetric(ctx, torch, dim, dtype):
    n = 2 * BM + 3
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((n, dim)).astype(dtype)
    x[17], x[BM + 40] = x[5], x[5]                        # coinciding rows, within a tile and across tiles
    for kernel in KERNELS:
        eps = _eps(kernel, x, x, dtype)
        for kind in KINDS:
            xt = _give(torch, x, kind)
            k = _np(ctx.rbf_matrix(xt, xt, kernel, eps))
            assert np.array_equal(k, k.T), (kernel, kind)
            assert np.all(np.diag(k) == (0.0, 1.0, 0.0, 1.0)[kernel - 1]), (kernel, kind)
            if kernel in (1, 3):
                assert k[5, 17] == 0.0 and k[17, BM + 40] == 0.0 and k[BM + 40, 5] == 0.0
                off = k[~np.eye(n, dtype=bool)]
                assert np.count_nonzero(off == 0.0) == 6


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_repeated_calls_are_bitwise_equal(ctx, torch, dtype):
    for case in (BASE, SPLIT_CASE):
        xq, xs, w = _points(*case, dtype)
        for kernel in KERNELS:
            eps = _eps(kernel, xq, xs, dtype)
            for kind in KINDS:
                a, b, c = (_give(torch, v, kind) for v in (xq, xs, w))
                first = _np(ctx.rbf_apply(a, b, c, kernel, eps, poly_degree=case[4]))
                assert np.array_equal(first, _np(ctx.rbf_apply(a, b, c, kernel, eps, poly_degree=case[4])))
                m = _np(ctx.rbf_matrix(a, b, kernel, eps))
                assert np.array_equal(m, _np(ctx.rbf_matrix(a, b, kernel, eps)))


def test_dim_beyond_the_limit_raises(ctx):
    xq, xs = np.zeros((4, MAX_DIM + 1)), np.zeros((3, MAX_DIM + 1))
    with pytest.raises(ValueError, match=r"dim must be in \[1, 128\]"):
        ctx.rbf_apply(xq, xs, np.zeros((3, 1)), 1)
    with pytest.raises(ValueError, match=r"dim must be in \[1, 128\]"):
        ctx.rbf_matrix(xq, xs, 1)


# ---- end to end: RbfInterp(device=True) against the restatement of the reference -------------------------------------------
# (4, 0.7) of test_rbf_interp_host_helper_matches_the_oracle is left out on purpose: its block system has condition 1e10, and
# 4-ulp noise in K alone moves the oracle's own predictions by 1e-8 to 6e-8; at these four settings by at most 2e-11.
INTERP_KERNELS = ((1, 0.0), (2, 1.0), (3, 0.0), (4, 2.0))


def _interp_fixture(kernel_type, degree):
    rng = np.random.default_rng(kernel_type * 10 + degree)
    x = rng.standard_normal((40, 2))
    y = (np.sin(x[:, 0]) + np.sin(x[:, 1])).reshape(-1, 1)
    xq = rng.standard_normal((10, 2))
    return x, y, xq


@pytest.mark.parametrize("kernel_type,param", INTERP_KERNELS)
@pytest.mark.parametrize("degree", [1, 2])
def test_rbf_interp_on_the_device_matches_the_oracle(ctx, torch, kernel_type, param, degree):
    from corrla_rs_amd.callers import RbfInterp
    from oracle import callers_oracle as co
    x, y, xq = _interp_fixture(kernel_type, degree)
    fo = co.RbfInterpOracle(kernel_type, param, 2, degree)
    fo.fit(x, y)
    ref = fo.predict(xq)
    tol = 1e-7 * max(1.0, np.abs(ref).max())
    f = RbfInterp(kernel_type, param, 2, degree, device=True, ctx=ctx)
    f.fit(x, y)
    got = f.predict(xq)
    assert type(got) is np.ndarray and got.shape == (10, 1) and got.dtype == np.float64
    assert np.max(np.abs(got - ref)) < tol
    if kernel_type in (1, 3):      # conditionally positive definite kernels with a polynomial tail interpolate
        assert np.max(np.abs(f.predict(x) - y)) < 1e-6
    # two right-hand sides at once == one interpolant per column
    y2 = np.hstack([y, np.cos(x[:, :1])])
    f2 = RbfInterp(kernel_type, param, 2, degree, device=True, ctx=ctx)
    f2.fit(x, y2)
    fo2 = co.RbfInterpOracle(kernel_type, param, 2, degree)
    fo2.fit(x, y2[:, 1:])
    ref2 = np.hstack([ref, fo2.predict(xq)])
    got2 = f2.predict(xq)
    assert got2.shape == (10, 2) and np.max(np.abs(got2 - ref2)) < 1e-7 * max(1.0, np.abs(ref2).max())
    # CUDA tensors in, tensors out: fit and predict on the device; a host-fitted model takes a CUDA query as well
    ft = RbfInterp(kernel_type, param, 2, degree, ctx=ctx)
    ft.fit(torch.as_tensor(x, device="cuda"), torch.as_tensor(y, device="cuda"))
    gt = ft.predict(torch.as_tensor(xq, device="cuda"))
    assert torch.is_tensor(gt) and gt.is_cuda and gt.dtype == torch.float64 and ft.x_known.is_cuda and ft.coeffs.is_cuda
    assert np.max(np.abs(gt.cpu().numpy() - ref)) < tol
    assert type(ft.predict(xq)) is np.ndarray and np.max(np.abs(ft.predict(xq) - ref)) < tol
    fh = RbfInterp(kernel_type, param, 2, degree)
    fh.fit(x, y)
    gh = fh.predict(torch.as_tensor(xq, device="cuda"))
    assert torch.is_tensor(gh) and gh.is_cuda and np.max(np.abs(gh.cpu().numpy() - ref)) < tol
