"""GPU tests of dense bfloat16 input (csrc/bf16in_kernels.hpp, corrla_*_bf16): the product kernel bit for bit on small
integers in both orientations on shapes with row and reduction tails (the one-row-per-instantiation check of
gemm_bf16a_kernel<NT, TN> is tests/test_gpu_tall_routes.py), its accuracy against f64, and random_svd / PCA on a bf16
tensor against the f32 oracle on the SAME values (the tensor's .float() widening) with the gates of the exact f32 path.
Run with -m gpu.

A is always built as torch.tensor(a32).to(torch.bfloat16); the references see its .float() widening."""
import functools

import numpy as np
import pytest

from oracle import rsvd_oracle as orc

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


def _bf16(a32):
    """(bf16 CPU tensor, its float32 widening as numpy): both sides of every comparison see identical values"""
    import torch
    t = torch.tensor(np.ascontiguousarray(a32, dtype=np.float32)).to(torch.bfloat16)
    return t, t.float().numpy()


# ---- the product kernel ------------------------------------------------------------------------------------------------
# (rows of A, columns of A, columns of the skinny operand).  First the list of tests/test_gpu_mixed.py; a bf16 row must be a
# multiple of 8 elements (16 bytes) long to be read in place, so those of its shapes with n % 8 != 0 go the widened way --
# each is followed here by a twin with n rounded up to 8, so that the column-tile counts of that list (1 .. 4, 6 .. 9) and
# the row / reduction tails run on the kernel as well, and (520, 136, 70) adds NT = 5 in the nn and the tn orientation
# (tests/test_gpu_tall_routes.py has one row per instantiation); the last shape is the odd row length the widened route is
# asserted on.
_SHAPES = [(256, 32, 16), (300, 70, 5), (1000, 600, 138), (257, 33, 144), (513, 1030, 17), (2048, 96, 40), (700, 257, 49),
           (64, 4100, 64), (4100, 64, 81), (1500, 520, 100), (1024, 1024, 113), (33, 8, 128),
           (300, 72, 5), (257, 40, 144), (513, 1032, 17), (700, 264, 49), (64, 4104, 64), (520, 136, 70),
           (300, 71, 20)]


def _matmul(ctx, torch, a_bf16, x32, trans):
    res = ctx.matmul(a_bf16.cuda(), torch.tensor(x32, device="cuda"), trans=trans)
    n_kernel = ctx.timings()["n_bf16_products"]
    assert res.dtype == torch.float32 and res.is_cuda
    return res.cpu().numpy(), n_kernel


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("shape", _SHAPES)
def test_bf16_input_products_exact_on_small_integers(ctx, torch, shape, trans):
    """Integers in [-8, 8] are exact in bf16 and their dot products exact in the f32 accumulator, so the result must be the
    integer product bit for bit: any slip in the fragment maps, the transposed LDS reads, the swizzles, the tails, the DMA
    ring or the slab reduction shows.  A row length that is a multiple of 8 runs on the kernel (n_bf16_products == 1), any
    other one is widened (0) -- and is bit-exact all the same."""
    m, n, l = shape
    rng = np.random.default_rng(m * 7 + n * 3 + l)
    a, a32 = _bf16(rng.integers(-8, 9, size=(m, n)))
    x = rng.integers(-8, 9, size=((m if trans else n), l)).astype(np.float32)
    got, n_kernel = _matmul(ctx, torch, a, x, trans)
    assert n_kernel == (1 if n % 8 == 0 else 0), (shape, n_kernel)
    if shape == (300, 71, 20):
        assert n_kernel == 0
    want = (a32.T.astype(np.float64) @ x if trans else a32.astype(np.float64) @ x)
    assert got.shape == want.shape
    assert np.array_equal(got.astype(np.float64), want), float(np.max(np.abs(got - want)))


@pytest.mark.parametrize("n", [2100, 2104])
@pytest.mark.parametrize("trans", [False, True])
def test_bf16_input_accuracy_on_gaussian_data(ctx, torch, trans, n):
    """A is one bf16 piece, X keeps 24 bits in three: the product is as accurate as the exact f32 kernel on the widened
    matrix -- the project's gate for the 24-bit split (tests/test_gpu_mixed.py: max(2 x exact-f32 error, 3e-7)).
    3000 x 2100 x 138 is that test's shape; its row length is no multiple of 8, so it is widened -- 2104 runs on the kernel."""
    rng = np.random.default_rng(5)
    m, l = 3000, 138
    a, a32 = _bf16(rng.standard_normal((m, n)))
    x = rng.standard_normal(((m if trans else n), l)).astype(np.float32)
    truth = a32.T.astype(np.float64) @ x if trans else a32.astype(np.float64) @ x
    got, n_kernel = _matmul(ctx, torch, a, x, trans)
    assert n_kernel == (1 if n % 8 == 0 else 0)
    exact = ctx.matmul(torch.tensor(a32, device="cuda"), torch.tensor(x, device="cuda"), trans=trans).cpu().numpy()
    err = float(np.linalg.norm(got - truth) / np.linalg.norm(truth))
    err_f32 = float(np.linalg.norm(exact - truth) / np.linalg.norm(truth))
    print(f"trans={trans}: relative Frobenius error vs f64: bf16 input {err:.3e}, exact f32 kernel {err_f32:.3e}")
    assert err <= max(2.0 * err_f32, 3e-7)


@pytest.mark.parametrize("n", [300, 304])
def test_bf16_input_handles_scales_and_signed_zeros(ctx, torch, n):
    """the scale pairs and the 600 x 300 shape of tests/test_gpu_mixed.py (widened: 300 % 8 != 0) and 304 columns on the kernel"""
    rng = np.random.default_rng(6)
    a0 = rng.standard_normal((600, n)).astype(np.float32)
    x = rng.standard_normal((n, 20)).astype(np.float32)
    a0[::7] = 0.0
    a0[5, :] = -0.0
    for sa, sx in ((1e-12, 1e12), (1e15, 1e-3), (1e-18, 1.0)):
        a, a32 = _bf16(a0 * np.float32(sa))
        xs = x * np.float32(sx)
        got, n_kernel = _matmul(ctx, torch, a, xs, False)
        assert n_kernel == (1 if n % 8 == 0 else 0)
        truth = a32.astype(np.float64) @ xs.astype(np.float64)
        assert np.all(np.isfinite(got))
        assert np.linalg.norm(got - truth) <= 5e-7 * np.linalg.norm(truth)


def test_matmul_rejects_a_bf16_skinny_operand(ctx, torch):
    a = torch.zeros((64, 32), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):
        ctx.matmul(a, torch.zeros((32, 4), dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(ValueError):
        ctx.matmul(torch.zeros((64, 32), dtype=torch.float32, device="cuda"), torch.zeros((32, 4), dtype=torch.bfloat16, device="cuda"))


# ---- random_svd ----------------------------------------------------------------------------------------------------------
def _spectrum_matrix(rng, m, n, decay):
    if decay is None:
        return rng.standard_normal((m, n)).astype(np.float32)
    u, _ = np.linalg.qr(rng.standard_normal((m, n)))
    v, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return ((u * (decay ** np.arange(n))) @ v.T).astype(np.float32)


K, Q, P = 128, 2, 10


@functools.lru_cache(maxsize=None)
def _tall_case(decay):
    """4096 x 1024 bf16-rounded matrix, a shared Omega, and the f32 oracle on the widened matrix (computed once)"""
    rng = np.random.default_rng(17)
    a, a32 = _bf16(_spectrum_matrix(rng, 4096, 1024, decay))
    om = rng.standard_normal((1024, K + P)).astype(np.float32)
    return a, a32, om, orc.random_svd(a32, K, Q, P, omega=om)


@functools.lru_cache(maxsize=None)
def _small_case(m, n, k):
    rng = np.random.default_rng(m + n + k)
    a, a32 = _bf16(rng.standard_normal((m, n)))
    om = rng.standard_normal((min(m, n), k + P)).astype(np.float32)
    return a, a32, om, orc.random_svd(a32, k, Q, P, omega=om)


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _check_parity(a32, usv, ref, k):
    """the gates of the exact f32 path (tests/test_gpu_parity.py: _parity, tests/test_gpu_mixed.py): same A, same Omega"""
    u, s, vt = (_np(t) for t in usv)
    uo, so, vto = ref
    m, n = a32.shape
    assert u.dtype == np.float32 and s.dtype == np.float32 and vt.dtype == np.float32
    assert u.shape == (m, k) and s.shape == (k, 1) and vt.shape == (k, n)
    ds = float(np.max(np.abs(s.ravel().astype(np.float64) - so.ravel())) / so[0, 0])
    dre = abs(orc.relerr(a32, u, s, vt) - orc.relerr(a32, uo, so, vto))
    eps = np.finfo(np.float32).eps
    ou = float(np.max(np.abs(u.T.astype(np.float64) @ u - np.eye(k))))
    ov = float(np.max(np.abs(vt.astype(np.float64) @ vt.T - np.eye(k))))
    print(f"dS/s1 {ds:.2e}, |d relerr| {dre:.2e}, orth U {ou:.2e} V {ov:.2e}")
    assert ou <= 200 * eps * np.sqrt(m)
    assert ov <= 200 * eps * np.sqrt(n)
    assert dre <= 1e-5 and ds <= 2e-5


@pytest.mark.parametrize("decay", [None, 0.995])
def test_random_svd_on_a_bf16_tensor_holds_the_f32_gates(ctx, torch, decay):
    """A bf16 CUDA tensor in, float32 factors on its device out; all 2 + 2 q tall products run on the bf16-input kernel
    (row-major: A X on the nn kernel, A^T Y on the tn kernel).  Before this feature the call widened A to f64, ran the f64
    kernels and returned f64, and there was no such counter."""
    a, a32, om, ref = _tall_case(decay)
    ad = a.cuda()
    u, s, vt = ctx.rsvd(ad, K, Q, P, omega=om)
    assert ctx.timings()["n_bf16_products"] == 2 + 2 * Q
    for t in (u, s, vt):
        assert t.dtype == torch.float32 and t.device == ad.device
    _check_parity(a32, (u, s, vt), ref, K)


def test_random_svd_on_fat_and_column_major_bf16_tensors(ctx, torch):
    """The other kernel for each product: a column-major view of the tall matrix (A X on the tn kernel, A^T Y on the nn one)
    and the fat matrix A^T, row-major, whose tall view is that same column-major memory."""
    a, a32, om, ref = _tall_case(None)
    fat = a.t().contiguous().cuda()                       # 1024 x 4096, row-major
    colmajor = fat.t()                                    # 4096 x 1024 with strides (1, 4096)
    assert colmajor.stride() == (1, 4096)
    usv = ctx.rsvd(colmajor, K, Q, P, omega=om)
    assert ctx.timings()["n_bf16_products"] == 2 + 2 * Q
    _check_parity(a32, usv, ref, K)
    u, s, vt = ctx.rsvd(fat, K, Q, P, omega=om)
    assert ctx.timings()["n_bf16_products"] == 2 + 2 * Q
    assert u.dtype == torch.float32 and tuple(u.shape) == (1024, K) and tuple(vt.shape) == (K, 4096)
    # random_svd.rs:96-109: the fat call returns (V, S, U^T) of the transposed problem
    _check_parity(a32, (vt.t(), s, u.t()), ref, K)


@pytest.mark.parametrize("case", ["wide_sketch", "strided", "odd_columns"])
def test_random_svd_outside_the_kernel_domain_runs_widened(ctx, torch, case):
    """l = 160 (two column blocks), a view with no unit stride and an odd column count: A is widened once and the call is
    the plain f32 call (n_bf16_products == 0) -- same gates."""
    if case == "wide_sketch":
        a, a32, om, ref = _small_case(1024, 512, 150)
        ad, k = a.cuda(), 150
    elif case == "strided":
        rng = np.random.default_rng(8)
        big, big32 = _bf16(rng.standard_normal((2048, 1536)))
        ad, a32, k = big.cuda()[::2, ::3], np.ascontiguousarray(big32[::2, ::3]), 32
        om = rng.standard_normal((512, k + P)).astype(np.float32)
        ref = orc.random_svd(a32, k, Q, P, omega=om)
    else:
        a, a32, om, ref = _small_case(1024, 511, 32)
        ad, k = a.cuda(), 32
    usv = ctx.rsvd(ad, k, Q, P, omega=om)
    assert ctx.timings()["n_bf16_products"] == 0
    assert usv[0].dtype == torch.float32 and usv[0].is_cuda
    _check_parity(a32, usv, ref, k)


def test_host_entry_takes_a_cpu_bf16_tensor(ctx):
    """A CPU bf16 tensor goes through the host-pointer entry: the 2-byte matrix is staged (and is then in the kernel's
    domain whatever its row length: the staged copy is padded), the outputs are float32 numpy arrays."""
    a, a32, om, ref = _small_case(1024, 511, 32)
    u, s, vt = ctx.rsvd(a, 32, Q, P, omega=om)
    assert ctx.timings()["n_bf16_products"] == 2 + 2 * Q
    for t in (u, s, vt):
        assert isinstance(t, np.ndarray) and t.dtype == np.float32
    _check_parity(a32, (u, s, vt), ref, 32)


def test_householder_thin_q_is_honoured(ctx, torch):
    a, a32, om, ref = _small_case(1024, 512, 32)
    usv = ctx.rsvd(a.cuda(), 32, Q, P, omega=om, qr="householder")
    assert ctx.timings()["n_bf16_products"] == 2 + 2 * Q
    _check_parity(a32, usv, ref, 32)


def test_same_seed_twice_is_bitwise_equal(ctx, torch):
    a, _, _, _ = _tall_case(None)
    ad = a.cuda()
    first = ctx.rsvd(ad, 64, Q, P, seed=7)
    again = ctx.rsvd(ad, 64, Q, P, seed=7)
    assert ctx.timings()["n_bf16_products"] == 2 + 2 * Q
    for x, y in zip(first, again):
        assert torch.equal(x, y)


# ---- PCA -----------------------------------------------------------------------------------------------------------------
def test_pca_on_a_bf16_tensor(ctx, torch):
    """4096 x 512, rank 32, shared Omega against orc.pca_rsvd on the widened matrix, with the f32 gates of
    tests/test_gpu_parity.py::test_pca_matches_oracle_and_sklearn (means atol 1e-5, S rtol 1e-4, projector 2e-3).  The
    default is the fused centring on A in place: the means (one product against a ones column) and every product of the
    range finder run on the bf16-input kernel.
    center="copy" runs widened and must agree with the default as
    tests/test_gpu_parity.py::test_pca_fused_centring_equals_centred_copy requires of f32: S rtol 2e-4, projector 5e-3.  That
    test also finds the two means bitwise equal, because both of its routes sum them with one and the same kernel; here the
    default sums them on the bf16-input kernel and the copy route on the f32 kernel -- two summation orders -- so they are
    held to the mean gate above (1e-5) against the oracle and against each other."""
    rng = np.random.default_rng(4096 + 512)
    m, n, k = 4096, 512, 32
    x, x32 = _bf16(rng.standard_normal((m, n)) * (0.97 ** np.arange(n)) + rng.standard_normal((1, n)) * 0.5)
    omega = rng.standard_normal((n, k + 10)).astype(np.float32)
    mo, so, co, _ = orc.pca_rsvd(x32.astype(np.float64), k, omega=omega.astype(np.float64))
    xd = x.cuda()
    means, s, comps = ctx.pca(xd, k, omega=omega)
    q = 20  # pca_rsvd.rs:65
    assert ctx.timings()["n_bf16_products"] == 1 + 2 + 2 * q
    for t in (means, s, comps):
        assert t.dtype == torch.float32 and t.is_cuda
    means, s, comps = _np(means), _np(s), _np(comps)
    assert means.shape == (1, n) and s.shape == (k, 1) and comps.shape == (k, n)
    assert np.allclose(means, mo, atol=1e-5)
    assert np.allclose(s, so, rtol=1e-4)
    assert np.linalg.norm(comps.T.astype(np.float64) @ comps - co.T @ co) < 2e-3
    mc, sc, cc = (_np(t) for t in ctx.pca(xd, k, omega=omega, center="copy"))
    assert ctx.timings()["n_bf16_products"] == 0
    assert np.allclose(mc, mo, atol=1e-5) and np.allclose(mc, means, atol=1e-5)
    assert np.allclose(s, sc, rtol=2e-4)
    assert np.linalg.norm(comps.T.astype(np.float64) @ comps - cc.T.astype(np.float64) @ cc) < 5e-3
    assert np.allclose(sc, so, rtol=2e-4)


def test_pca_on_a_fat_bf16_tensor(ctx, torch):
    """means along the tall side of the tall view (the nn kernel with one column); the f32 gates of the fat shape of
    tests/test_gpu_parity.py::test_pca_fused_centring_equals_centred_copy against the oracle (S rtol 2e-4)"""
    rng = np.random.default_rng(3)
    m, n, k = 64, 1504, 6
    x, x32 = _bf16(rng.standard_normal((m, n)) * (0.97 ** np.arange(n)) + rng.standard_normal((1, n)) * 0.5)
    omega = rng.standard_normal((m, k + 10)).astype(np.float32)
    mo, so, co, _ = orc.pca_rsvd(x32.astype(np.float64), k, omega=omega.astype(np.float64))
    means, s, comps = (_np(t) for t in ctx.pca(x.cuda(), k, omega=omega))
    assert ctx.timings()["n_bf16_products"] == 1 + 2 + 2 * 20
    assert np.allclose(means, mo, atol=1e-5)
    assert np.allclose(s, so, rtol=2e-4)
    assert np.linalg.norm(comps.T.astype(np.float64) @ comps - co.T @ co) < 5e-3
