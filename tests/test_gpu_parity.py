"""GPU parity tests: the HIP path (through the C ABI of libcorrla_rsvd.so) against the CPU oracle on
the same seeded inputs and the same Omega, against the committed golden fixtures, and -- at
BASELINE.json's full sizes -- through size-independent properties.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

from oracle import rsvd_oracle as orc
from tests.conftest import golden_names
from tests.helpers import check_factorization, load_golden, orth_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import corrla_rs_amd as cr
    return cr.Context(0)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def test_native_library_is_the_path(ctx):
    from corrla_rs_amd import _lib
    lib = _lib.load()
    assert b"gfx950" in lib.corrla_version()
    assert lib.corrla_device_count() >= 1


# ---- the GEMM shim (par_matmul_helper, mat_utils.rs:20-33) --------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("layout", ["row", "col"])
@pytest.mark.parametrize("shape_l", [(64, 64, 16), (200, 136, 24), (333, 130, 1), (130, 333, 40), (1000, 72, 138),
                                     (72, 1000, 150), (4, 4, 3), (257, 63, 17), (2048, 1024, 138), (5000, 36, 74)])
def test_matmul_both_ops(ctx, torch, dtype, layout, shape_l):
    m, n, l = shape_l
    dt = getattr(torch, dtype)
    g = torch.Generator(device="cuda").manual_seed(m * 1000 + n)
    a = torch.randn((m, n), dtype=dt, device="cuda", generator=g)
    if layout == "col":
        a = a.t().contiguous().t()  # same values, column-major memory
    tol = 2e-5 if dtype == "float32" else 1e-12
    for trans in (False, True):
        x = torch.randn(((m if trans else n), l), dtype=dt, device="cuda", generator=g)
        res = ctx.matmul(a, x, trans=trans, beta=1.0)
        ref = (a.double().t() if trans else a.double()) @ x.double()
        scale = ref.abs().max().item() + 1e-30
        err = (res.double() - ref).abs().max().item() / scale
        assert err < tol, (trans, err)
    # beta scaling (res = beta * lhs * rhs, alpha=None => overwrite)
    x = torch.randn((n, l), dtype=dt, device="cuda", generator=g)
    res = ctx.matmul(a, x, trans=False, beta=0.25)
    ref = 0.25 * (a.double() @ x.double())
    assert (res.double() - ref).abs().max().item() / (ref.abs().max().item() + 1e-30) < tol


def test_matmul_known_answers(ctx, torch):
    # mat_utils.rs:642-684
    import os
    from tests.helpers import GOLDEN_DIR
    d = np.load(os.path.join(GOLDEN_DIR, "matmul_known.npz"))
    for rhs, out in (("rhs_vec", "out_vec"), ("rhs_mat", "out_mat")):
        a = torch.tensor(d["lhs"], device="cuda")
        x = torch.tensor(d[rhs], device="cuda")
        assert np.allclose(ctx.matmul(a, x).cpu().numpy(), d[out], atol=1e-6)


def test_matmul_exact_integer_layout_check(ctx, torch):
    """Asymmetric exact-integer operands: any wrong MFMA lane map, swizzle or transposed C-write shows
    as an exact mismatch (cdna guide: 'always A=I-check with ASYMMETRIC B')."""
    for dt in (torch.float32, torch.float64):
        m, n, l = 192, 128, 48
        a = (torch.arange(m * n, device="cuda").reshape(m, n) % 7 - 3).to(dt)
        x = (torch.arange(n * l, device="cuda").reshape(n, l) % 5 - 2).to(dt) + torch.arange(l, device="cuda").to(dt)
        assert torch.equal(ctx.matmul(a, x), a @ x)
        y = (torch.arange(m * l, device="cuda").reshape(m, l) % 11 - 5).to(dt)
        assert torch.equal(ctx.matmul(a, y, trans=True), a.t() @ y)
        ac = a.t().contiguous().t()
        assert torch.equal(ctx.matmul(ac, x), a @ x)
        assert torch.equal(ctx.matmul(ac, y, trans=True), a.t() @ y)


# ---- random_mat_normal (mat_utils.rs:161-175) ---------------------------------------------------
def test_fill_normal_matches_host_restatement(ctx, torch):
    from tests.emu_harness import emu_fill_normal
    for dt, npdt, tol in ((torch.float64, np.float64, 1e-12), (torch.float32, np.float32, 2e-5)):
        t = torch.empty((96, 40), dtype=dt, device="cuda")
        ctx.fill_normal(t, seed=20241008)
        ref = emu_fill_normal(96, 40, seed=20241008, dtype=npdt)
        assert np.max(np.abs(t.cpu().numpy() - ref)) < tol
        shard = torch.empty((32, 40), dtype=dt, device="cuda")
        ctx.fill_normal(shard, seed=20241008, row0=64, global_cols=40)
        assert torch.equal(shard, t[64:96])
        tc = torch.empty((40, 96), dtype=dt, device="cuda").t()  # column-major storage, same logical matrix
        ctx.fill_normal(tc, seed=20241008)
        assert torch.equal(tc, t)
    big = torch.empty((2048, 1024), dtype=torch.float32, device="cuda")
    ctx.fill_normal(big, seed=3)
    assert abs(big.mean().item()) < 3e-3 and abs(big.std().item() - 1) < 3e-3


def test_fill_normal_distribution_on_the_gpu(ctx, torch):
    """random_mat_normal draws i.i.d. N(0,1) (mat_utils.rs:161-175, rand_distr StandardNormal).  Kolmogorov-Smirnov
    test of the GPU generator's OUTPUT (not of the host restatement) against the normal CDF, both dtypes, plus
    moments, tail mass and the absence of correlation between neighbouring counters / rows / seeds."""
    from scipy import stats
    for dt in (torch.float32, torch.float64):
        t = torch.empty((4096, 512), dtype=dt, device="cuda")
        ctx.fill_normal(t, seed=12345)
        x = t.cpu().numpy().astype(np.float64)
        ks = stats.kstest(x.ravel()[:: 2], "norm")            # 1M samples
        assert ks.pvalue > 1e-3, (dt, ks)
        assert abs(x.mean()) < 4 / np.sqrt(x.size) and abs(x.var() - 1) < 6 * np.sqrt(2.0 / x.size)
        assert abs(stats.skew(x.ravel())) < 0.01 and abs(stats.kurtosis(x.ravel())) < 0.02
        frac3 = np.mean(np.abs(x) > 3.0)
        assert abs(frac3 - 0.0026998) < 2.5e-4                # two-sided 3-sigma tail mass
        # neighbouring counters (columns), neighbouring rows, and a different seed: uncorrelated
        assert abs(np.mean(x[:, :-1] * x[:, 1:])) < 5 / np.sqrt(x.size)
        assert abs(np.mean(x[:-1] * x[1:])) < 5 / np.sqrt(x.size)
        t2 = torch.empty_like(t)
        ctx.fill_normal(t2, seed=12346)
        assert abs(np.mean(x * t2.cpu().numpy())) < 5 / np.sqrt(x.size)


# ---- random_svd vs the oracle on the golden fixtures ---------------------------------------------
def _parity(ctx, a, k, q, p, omega, dtype, s_rtol, rec_rtol, device_path=False):
    a = np.asarray(a, dtype=dtype)
    om = np.asarray(omega, dtype=dtype)
    if device_path:
        import torch
        u, s, vt = ctx.rsvd(torch.tensor(a, device="cuda"), k, q, p, omega=om)
        u, s, vt = u.cpu().numpy(), s.cpu().numpy(), vt.cpu().numpy()
    else:
        u, s, vt = ctx.rsvd(a, k, q, p, omega=om)
    assert u.dtype == dtype
    uo, so, vto = orc.random_svd(a, k, q, p, omega=om)
    check_factorization(a, u, s, vt, k, 0)
    s1 = max(float(so[0, 0]), 1e-300)
    assert np.max(np.abs(s.ravel().astype(np.float64) - so.ravel())) <= s_rtol * s1
    # north star: ||A - U S Vt||_F / ||A||_F within 1e-5 of the CPU reference (same A, same Omega)
    assert abs(orc.relerr(a, u, s, vt) - orc.relerr(a, uo, so, vto)) <= 1e-5
    rec = (u.astype(np.float64) * s.ravel()) @ vt.astype(np.float64)
    reco = (uo.astype(np.float64) * so.ravel()) @ vto.astype(np.float64)
    assert np.linalg.norm(rec - reco) <= rec_rtol * max(np.linalg.norm(reco), 1e-300)
    nnz = int(np.sum(so.ravel() > 1e-5 * s1))
    eps = np.finfo(dtype).eps
    assert orth_err(u[:, :nnz]) <= 200 * eps * np.sqrt(a.shape[0])
    assert orth_err(vt[:nnz, :].T) <= 200 * eps * np.sqrt(a.shape[1])
    return u, s, vt


@pytest.mark.parametrize("name", golden_names())
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rsvd_golden(ctx, name, dtype):
    g = load_golden(name)
    f64 = dtype == np.float64
    tight = name not in ("lowrank256x96", "fat20x500_pod", "rankdef96x40")
    s_rtol = (1e-10 if f64 else 2e-5) if tight else (1e-7 if f64 else 2e-3)
    rec_rtol = (1e-8 if f64 else 1e-3) if tight else (1e-6 if f64 else 2e-2)
    u, s, vt = _parity(ctx, g["A"], g["k"], g["q"], g["p"], g["omega"], dtype, s_rtol, rec_rtol)
    if "ref_s" in g and f64:
        # reference author's numpy rsvd, same Omega (examples/benchmark_rsvd.py:26-54)
        assert np.max(np.abs(s.ravel() - g["ref_s"])) <= 1e-9 * g["ref_s"][0]
    if name.startswith("known5x5"):
        assert np.allclose(s.ravel(), orc.KNOWN_ANSWER_S[: g["k"]], atol=1e-3)  # random_svd.rs:170-195


@pytest.mark.parametrize("order", ["C", "F", "strided", "device_C", "device_F", "device_strided"])
@pytest.mark.parametrize("shape", [(70, 33), (33, 70), (64, 64), (1, 9), (9, 1), (301, 129)])
def test_rsvd_layouts_and_shapes(ctx, torch, order, shape):
    rng = np.random.default_rng(7)
    m, n = shape
    base = rng.standard_normal((2 * m, 2 * n))
    k = max(1, min(m, n) // 3)
    q, p = 2, 4
    nt = min(m, n)
    l = min(k + p, nt)
    omega = rng.standard_normal((nt, l))
    if order.startswith("device"):
        tb = torch.tensor(base, device="cuda")
        if order == "device_C":
            a = tb[:m, :n].contiguous()
        elif order == "device_F":
            a = tb[:m, :n].t().contiguous().t()
        else:
            a = tb[::2, ::2]
        u, s, vt = ctx.rsvd(a, k, q, p, omega=omega)
        a_np = a.cpu().numpy()
        u, s, vt = u.cpu().numpy(), s.cpu().numpy(), vt.cpu().numpy()
    else:
        a = {"C": np.ascontiguousarray(base[:m, :n]), "F": np.asfortranarray(base[:m, :n]), "strided": base[::2, ::2]}[order]
        u, s, vt = ctx.rsvd(a, k, q, p, omega=omega)
        a_np = np.array(a)
    uo, so, vto = orc.random_svd(a_np, k, q, p, omega=omega)
    assert s.shape == (k, 1) and u.shape == (m, k) and vt.shape == (k, n)
    assert np.allclose(s, so, rtol=0, atol=1e-9 * so[0, 0])
    assert abs(orc.relerr(a_np, u, s, vt) - orc.relerr(a_np, uo, so, vto)) < 1e-9


def test_rsvd_shape_contract_10000x100(ctx):
    # random_svd.rs:119-151 (test_rsvd_shape): 10000 x 100 f64, k=4, q=12, p=10; device RNG for Omega
    rng = np.random.default_rng(1)
    a = rng.standard_normal((10000, 100))
    u, s, vt = ctx.rsvd(a, 4, 12, 10, seed=99)
    rec = (u * s.ravel()) @ vt
    assert rec.shape == a.shape
    ex = np.linalg.svd(a, compute_uv=False)[:4]
    assert np.all(s.ravel() <= ex * (1 + 1e-9)) and np.all(s.ravel() >= 0.9 * ex)
    assert orth_err(u) < 1e-12 and orth_err(vt.T) < 1e-12
    u2, s2, vt2 = ctx.rsvd(a, 4, 12, 10, seed=99)
    assert np.array_equal(s, s2) and np.array_equal(u, u2)  # deterministic for a fixed seed


def test_invalid_arguments_raise(ctx):
    a = np.ones((6, 4))
    with pytest.raises(ValueError):
        ctx.rsvd(a, 5, 1, 2)   # rank > min(m, n): the reference panics (random_svd.rs:98-107)
    with pytest.raises(ValueError):
        ctx.rsvd(a, 0, 1, 2)
    with pytest.raises(ValueError):
        ctx.rsvd(a, 2, -1, 2)
    with pytest.raises(ValueError):
        ctx.rsvd(np.ones((3,)), 1, 1, 1)


def test_power_iter_surface(ctx):
    rng = np.random.default_rng(3)
    a = rng.standard_normal((500, 60))
    om = rng.standard_normal((60, 14))
    for q in (0, 2, 5):
        qe = ctx.power_iter(a, 14, q, omega=om)
        qo = orc.power_iter(a, om, q)
        assert qe.shape == (500, 14) and orth_err(qe) < 1e-12
        assert np.linalg.norm(qe @ qe.T - qo @ qo.T) < 1e-8


def test_drop_in_module_name(ctx):
    # examples/benchmark_rsvd.py:13,101 : import corrla_rs as hrl; hrl.rsvd(test_A, 4, 8, 10)
    import corrla_rs as hrl
    rng = np.random.default_rng(2)
    a = rng.standard_normal((400, 90))
    u, s, vt = hrl.rsvd(a, 4, 8, 10)
    assert u.shape == (400, 4) and s.shape == (4, 1) and vt.shape == (4, 90) and u.dtype == np.float64
    ex = np.linalg.svd(a, compute_uv=False)[:4]
    assert np.allclose(s.ravel(), ex, rtol=2e-2)


# ---- BASELINE.json configs at full size: size-independent properties ----------------------------
def _device_checks(torch, a, u, s, vt, k, dtype_eps):
    """Orthonormality, Rayleigh consistency (s_i = u_i^T A v_i), optimality bound and relerr identity."""
    ud, vd, sd = u.double(), vt.double().t(), s.double().ravel()
    eye = torch.eye(k, dtype=torch.float64, device=a.device)
    assert (ud.t() @ ud - eye).abs().max().item() < 50 * dtype_eps * np.sqrt(k) * 4
    assert (vd.t() @ vd - eye).abs().max().item() < 50 * dtype_eps * np.sqrt(k) * 4
    av = torch.empty((a.shape[0], k), dtype=torch.float64, device=a.device)
    step = 2048
    for r0 in range(0, a.shape[0], step):
        av[r0:r0 + step] = a[r0:r0 + step].double() @ vd
    ray = (ud * av).sum(dim=0)
    assert ((ray - sd).abs().max() / sd[0]).item() < 1e3 * dtype_eps
    assert torch.all(sd[:-1] >= sd[1:] - 1e-6 * sd[0]) and torch.all(sd >= 0)
    fro2 = float(sum((a[r0:r0 + step].double() ** 2).sum().item() for r0 in range(0, a.shape[0], step)))
    # ||A - U S Vt||^2 = ||A||^2 - 2 sum s_i ray_i + sum s_i^2 for orthonormal U, V
    err2 = fro2 - 2 * float((sd * ray).sum().item()) + float((sd ** 2).sum().item())
    return np.sqrt(max(err2, 0.0) / fro2)


def test_c2_full_size_f32_properties(ctx, torch):
    """BASELINE config 2: 16384 x 16384 f32, rank 128, 2 power iterations, p=10."""
    m = n = 16384
    k, q, p = 128, 2, 10
    a = torch.empty((m, n), dtype=torch.float32, device="cuda")
    ctx.fill_normal(a, seed=20241008)
    u, s, vt = ctx.rsvd(a, k, q, p, seed=1)
    re = _device_checks(torch, a, u, s, vt, k, 1.2e-7)
    # Gaussian square matrix: sigma_1 ~ 2 sqrt(n); rank-128 relerr a little under 1
    assert 0.9 < re < 0.999
    assert 1.7 * np.sqrt(n) < s[0, 0].item() < 2.1 * np.sqrt(n)
    # linearity (size-independent): rsvd(2A) has 2x the singular values, same seed
    u2, s2, vt2 = ctx.rsvd(a * 2, k, q, p, seed=1)
    assert torch.allclose(s2, 2 * s, rtol=1e-5)
    # sampled parity of the sketch GEMM against f64 on random rows
    om = torch.empty((n, 138), dtype=torch.float32, device="cuda")
    ctx.fill_normal(om, seed=5)
    y = ctx.matmul(a, om)
    rows = torch.randint(0, m, (64,), device="cuda")
    ref = a[rows].double() @ om.double()
    assert ((y[rows].double() - ref).abs().max() / ref.abs().max()).item() < 2e-5


def test_c3_like_f64_properties(ctx, torch):
    """BASELINE config 3 shape family (tall f64 snapshot matrix, wide sketch l = 266 > one column
    block) at 1/4 of the rows so the CPU side stays small: 16384 x 4096 f64, rank 256, POD defaults."""
    m, n, k, q, p = 16384, 4096, 256, 2, 10
    a = torch.empty((m, n), dtype=torch.float64, device="cuda")
    ctx.fill_normal(a, seed=7)
    u, s, vt = ctx.rsvd(a, k, q, p, seed=2)
    re = _device_checks(torch, a, u, s, vt, k, 2.2e-16)
    assert 0.8 < re < 0.999


def test_c4_like_tall_f32(ctx, torch):
    """BASELINE config 4 shape family: very tall, n = 512, rank 64 (one GPU's 1/8 shard: 1.25M rows)."""
    m, n, k, q, p = 1_250_000, 512, 64, 2, 10
    a = torch.empty((m, n), dtype=torch.float32, device="cuda")
    ctx.fill_normal(a, seed=11)
    u, s, vt = ctx.rsvd(a, k, q, p, seed=3)
    re = _device_checks(torch, a, u, s, vt, k, 1.2e-7)
    assert 0.8 < re < 0.999


# ---- alternate SVD-of-the-core paths and error handling ------------------------------------------
@pytest.mark.parametrize("mode", ["block", "host", "mc"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_small_svd_paths_agree(ctx, mode, dtype, monkeypatch):
    """The l x l SVD (random_svd.rs:89) has three device kernels and a host routine; all must give the same
    factorization as the default path (up to rounding) on a well-separated and on a rank-deficient case."""
    for name in ("gauss512x256", "rankdef96x40", "lowrank256x96"):
        g = load_golden(name)
        a = g["A"].astype(dtype)
        om = g["omega"].astype(dtype)
        u0, s0, vt0 = ctx.rsvd(a, g["k"], g["q"], g["p"], omega=om)
        monkeypatch.setenv("CORRLA_SVD", mode)
        u1, s1, vt1 = ctx.rsvd(a, g["k"], g["q"], g["p"], omega=om)
        monkeypatch.delenv("CORRLA_SVD")
        tol = 1e-10 if dtype == np.float64 else 5e-5
        assert np.max(np.abs(s1 - s0)) <= tol * s0[0, 0]
        rec0 = (u0.astype(np.float64) * s0.ravel()) @ vt0.astype(np.float64)
        rec1 = (u1.astype(np.float64) * s1.ravel()) @ vt1.astype(np.float64)
        assert np.linalg.norm(rec1 - rec0) <= 50 * tol * np.linalg.norm(rec0)


@pytest.mark.parametrize("l_total", [129, 138, 150, 200])
def test_f64_core_sizes_cross_kernel_boundaries(ctx, l_total):
    """f64 sketches around the LDS-capacity boundaries of the Jacobi kernels (128 / 138 / block fallback)."""
    rng = np.random.default_rng(l_total)
    m, n = 700, 260
    a = rng.standard_normal((m, n)) * (0.99 ** np.arange(n))  # kappa(sketch) ~ 1e4: tests the kernels, not the conditioning
    k, p, q = l_total - 10, 10, 2
    om = rng.standard_normal((n, l_total))
    u, s, vt = ctx.rsvd(a, k, q, p, omega=om)
    uo, so, vto = orc.random_svd(a, k, q, p, omega=om)
    assert np.max(np.abs(s - so)) <= 1e-9 * so[0, 0]
    assert abs(orc.relerr(a, u, s, vt) - orc.relerr(a, uo, so, vto)) <= 1e-9
    assert orth_err(u) < 1e-11 and orth_err(vt.T) < 1e-11


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_core_widths_across_every_kernel_boundary(ctx, dtype):
    """l = k + p swept over the selection boundaries of the device kernels: block Jacobi at l = 1, ring Jacobi register
    variants (64 / 96, odd widths carry a zero padding column through the ring), multi-workgroup and block Jacobi beyond,
    device Cholesky + inverse (l <= 176) vs the host-controlled path.  Same Omega as the oracle."""
    rng = np.random.default_rng(7)
    m, n = 420, 230
    # spectrum decays to 0.16 sigma_1: (sigma_l / sigma_1)^(2q+1) stays far above f32 eps, so every triplet is
    # determined by the data and not by rounding in the power iteration
    a = (rng.standard_normal((m, n)) * (0.992 ** np.arange(n))).astype(dtype)
    f64 = dtype == np.float64
    widths = (1, 2, 3, 4, 5, 8, 9, 17, 31, 63, 64, 65, 95, 96, 97, 127, 128, 129, 137, 143, 144, 145, 161, 176, 177, 201, 230)
    for l in widths:
        if l == n and not f64:
            continue  # l = n: cond(Y) = (sigma_1 / sigma_n)^5 exceeds 1 / eps_f32, the f32 tail is rounding noise
        p = min(10, l - 1)
        k = l - p
        om = rng.standard_normal((n, l)).astype(dtype)
        u, s, vt = ctx.rsvd(a, k, 2, p, omega=om)
        uo, so, vto = orc.random_svd(a.astype(np.float64), k, 2, p, omega=om.astype(np.float64))
        assert np.max(np.abs(s.astype(np.float64) - so)) <= (1e-10 if f64 else 1e-4) * so[0, 0], l
        assert abs(orc.relerr(a, u, s, vt) - orc.relerr(a, uo, so, vto)) <= (1e-9 if f64 else 1e-5), l
        assert orth_err(u) < (1e-11 if f64 else 2e-4) and orth_err(vt.T) < (1e-11 if f64 else 2e-4), l
        assert np.all(np.diff(s.ravel()) <= 0) and np.all(s >= 0), l


@pytest.mark.parametrize("env", ["CORRLA_SVD=block", "CORRLA_SVD=mc", "CORRLA_HOST_CHOL"])
def test_alternative_device_paths_agree(ctx, env, monkeypatch):
    """The block Jacobi, the multi-workgroup Jacobi and the host-controlled Cholesky-QR must reproduce the default
    path (W-only ring + replay at l = 75, multi-workgroup Jacobi at 138; device Cholesky)."""
    name, _, val = env.partition("=")
    rng = np.random.default_rng(11)
    a = (rng.standard_normal((600, 150)) * (0.98 ** np.arange(150))).astype(np.float32)
    for l in (75, 138):   # odd pair count / the C2 width
        om = rng.standard_normal((150, l)).astype(np.float32)
        u0, s0, vt0 = ctx.rsvd(a, l - 10, 2, 10, omega=om)
        monkeypatch.setenv(name, val or "1")
        u1, s1, vt1 = ctx.rsvd(a, l - 10, 2, 10, omega=om)
        monkeypatch.delenv(name)
        assert np.max(np.abs(s1 - s0)) <= 3e-5 * s0[0, 0]
        rec0 = (u0.astype(np.float64) * s0.ravel()) @ vt0.astype(np.float64)
        rec1 = (u1.astype(np.float64) * s1.ravel()) @ vt1.astype(np.float64)
        assert np.linalg.norm(rec1 - rec0) <= 2e-3 * np.linalg.norm(rec0)


def test_non_finite_input_is_an_error_not_garbage(ctx):
    from corrla_rs_amd._lib import CorrlaError
    a = np.ones((64, 32))
    a[3, 5] = np.nan
    with pytest.raises(CorrlaError) as e:
        ctx.rsvd(a, 4, 2, 4)
    assert e.value.code == 5  # CORRLA_ENUMERIC


def test_seed_changes_sketch_not_quality(ctx):
    rng = np.random.default_rng(9)
    a = (rng.standard_normal((400, 30)) * (0.5 ** np.arange(30))) @ rng.standard_normal((30, 120))
    ex = np.linalg.svd(a, compute_uv=False)[:8]
    u1, s1, vt1 = ctx.rsvd(a, 8, 3, 8, seed=1)
    u2, s2, vt2 = ctx.rsvd(a, 8, 3, 8, seed=2)
    assert not np.array_equal(u1, u2)
    for s_ in (s1, s2):  # leading values converge fast; the trailing ones carry RSVD's own approximation error
        assert np.allclose(s_.ravel()[:5], ex[:5], rtol=1e-6) and np.allclose(s_.ravel(), ex, rtol=1e-2)
        assert np.all(s_.ravel() <= ex * (1 + 1e-12))  # Rayleigh-Ritz values never exceed the true ones


def test_large_norm_does_not_overflow_f32(ctx):
    """random_svd.rs:53-55 rescales Y every iteration; sigma_1 ~ 1e9 would overflow f32 after two unscaled
    power iterations (sigma^5 ~ 1e45)."""
    rng = np.random.default_rng(4)
    a = (rng.standard_normal((256, 64)) * 1e9 / 24).astype(np.float32)
    u, s, vt = ctx.rsvd(a, 6, 4, 6, seed=5)
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(u)) and np.all(np.isfinite(vt))
    ex = np.linalg.svd(a.astype(np.float64), compute_uv=False)[:6]
    assert np.allclose(s.ravel(), ex, rtol=0.15)


# ---- PCA caller (pca_rsvd.rs:56-82, pyo3 rpca) --------------------------------
@pytest.mark.parametrize("shape", [(100, 10), (2000, 64), (50, 400)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pca_matches_oracle_and_sklearn(ctx, shape, dtype):
    rng = np.random.default_rng(sum(shape))
    m, n = shape
    x = (rng.standard_normal((m, n)) * (0.85 ** np.arange(n)) + rng.standard_normal((1, n)) * 3.0).astype(dtype)
    k = 4
    p = min(n, 10)
    nt = min(m, n)
    omega = rng.standard_normal((nt, min(k + p, nt))).astype(dtype)
    means, s, comps = ctx.pca(x, k, omega=omega)
    mo, so, co, evo = orc.pca_rsvd(x.astype(np.float64), k, omega=omega.astype(np.float64))
    f64 = dtype == np.float64
    assert means.shape == (1, n) and s.shape == (k, 1) and comps.shape == (k, n)
    assert np.allclose(means, mo, atol=1e-12 if f64 else 1e-5)
    assert np.allclose(s, so, rtol=1e-9 if f64 else 1e-4)
    assert np.linalg.norm(comps.T.astype(np.float64) @ comps - co.T @ co) < (1e-7 if f64 else 2e-3)
    from sklearn.decomposition import PCA
    sk = PCA(n_components=k, svd_solver="full").fit(x.astype(np.float64))
    assert np.allclose((s.astype(np.float64) ** 2 / (m - 1.0)).ravel(), sk.explained_variance_, rtol=1e-6 if f64 else 1e-3)


@pytest.mark.parametrize("shape", [(3000, 96), (64, 1500)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pca_fused_centring_equals_centred_copy(ctx, shape, dtype):
    """implicit centring (rank-1 corrections, the matrix is never rewritten) against the centred copy."""
    rng = np.random.default_rng(sum(shape))
    m, n = shape
    x = (rng.standard_normal((m, n)) * (0.97 ** np.arange(n)) + rng.standard_normal((1, n)) * 0.5).astype(dtype)
    k, p = 6, 10
    nt = min(m, n)
    omega = rng.standard_normal((nt, k + p)).astype(dtype)
    mf, sf, cf = ctx.pca(x, k, omega=omega, center="fused")
    mc, sc, cc = ctx.pca(x, k, omega=omega, center="copy")
    f64 = dtype == np.float64
    assert np.array_equal(mf, mc)
    assert np.allclose(sf, sc, rtol=1e-10 if f64 else 2e-4)
    assert np.linalg.norm(cf.T.astype(np.float64) @ cf - cc.T.astype(np.float64) @ cc) < (1e-8 if f64 else 5e-3)
    mo, so, co, _ = orc.pca_rsvd(x.astype(np.float64), k, omega=omega.astype(np.float64))
    assert np.allclose(sf, so, rtol=1e-9 if f64 else 2e-4)


def test_rpca_surface_ignores_iters_and_oversamples_like_the_reference(ctx):
    # lib_math_utils_py.rs:38-55: rpca(a, n_rank, n_iters, n_oversamples) -> (singular_values (k,1), components (k,n))
    import corrla_rs as hrl
    rng = np.random.default_rng(0)
    x = rng.standard_normal((500, 12)) * np.arange(1, 13)
    sv, pc = hrl.rpca(x, 3, 1, 0, seed=7)
    sv2, pc2 = hrl.rpca(x, 3, 99, 5, seed=7)
    assert sv.shape == (3, 1) and pc.shape == (3, 12)
    assert np.array_equal(sv, sv2) and np.array_equal(pc, pc2)
    pca = hrl.PcaRsvd(x, 3, seed=7)
    assert np.allclose(pca.explained_var().ravel(), np.sort(np.linalg.eigvalsh(np.cov(x, rowvar=False)))[::-1][:3], rtol=1e-6)
    red = pca.apply_tr(x)
    assert red.shape == (500, 3)
    back = pca.apply_inv_tr(red)
    # rank-3 reconstruction of 12-d data equals the optimal (exact PCA) rank-3 residual
    xc = x - x.mean(axis=0)
    opt = np.sqrt(np.sum(np.linalg.svd(xc, compute_uv=False)[3:] ** 2))
    assert abs(np.linalg.norm(back - x) - opt) <= 1e-6 * opt


def test_pca_device_tensor_path(ctx, torch):
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((4096, 256), dtype=torch.float32, device="cuda", generator=g) * torch.linspace(3, 0.1, 256, device="cuda")
    means, s, comps = ctx.pca(x, 8, seed=5)
    xs = x.double()
    ev = torch.linalg.eigvalsh(torch.cov(xs.t())).flip(0)[:8]
    assert torch.allclose((s.double() ** 2 / (4096 - 1)).ravel(), ev, rtol=2e-3)
    assert torch.allclose(means.double().ravel(), xs.mean(dim=0), atol=1e-5)


# ---- callers on the path: POD modes, active-subspace fit_svd, DMDc ------
@pytest.mark.parametrize("nx,nt", [(20, 40), (50, 40), (500, 40)])
def test_dmdc_reference_test_on_gpu(ctx, nx, nt):
    """The reference's own test_dmdc (dmd_rom.rs:233-310) through the GPU RSVD: shapes, 14 eigenvalues, and the
    20-step prediction within 5e-2 of the truth."""
    import corrla_rs_amd as cr
    from oracle import callers_oracle as co
    snaps, u = co.dmdc_reference_test_data(nx, nt)
    m = cr.DMDc(snaps, u, 1.0, 14, 40, seed=3, ctx=ctx)
    assert m.est_a_til().shape == (nx, nx) and m.est_b_til().shape[0] == nx
    assert m.lambdas.shape[0] == 14
    pred = m.predict_multiple(snaps[:, 0:1], u)
    assert np.max(np.abs(pred[:, 19] - snaps[:, 20])) < 5e-2
    # and against the oracle's DMDc with shared sketches: the same one-step operators on the data
    rng = np.random.default_rng(nx)
    lx = min(14 + 12, min(nx + 1, nt - 1))
    ly = min(14 + 12, min(nx, nt - 1))
    om_x = rng.standard_normal((min(nx + 1, nt - 1), lx))
    om_y = rng.standard_normal((min(nx, nt - 1), ly))
    mg = cr.DMDc(snaps, u, 1.0, 14, 40, omega_x=om_x, omega_y=om_y, ctx=ctx)
    mo = co.DMDcOracle(snaps, u, 1.0, 14, 40, omega_x=om_x, omega_y=om_y)
    pg, po = mg.predict_multiple(snaps[:, 0:1], u), mo.predict_multiple(snaps[:, 0:1], u)
    assert np.max(np.abs(pg[:, :20] - po[:, :20])) < 5e-2 * np.max(np.abs(po[:, :20]))


def test_drop_in_pydmdc_class(ctx):
    """`from corrla_rs import PyDMDc` (examples/benchmark_dmd.py:12,119-124): constructor (x, u, n_modes, n_iters) with
    dt = 1, predict(x0, u) = predict_multiple (lib_math_utils_py.rs:254-283)."""
    from corrla_rs import PyDMDc
    from oracle import callers_oracle as co
    snaps, u = co.dmdc_reference_test_data(50, 40)
    m = PyDMDc(snaps, u, 14, 40)
    pred = m.predict(snaps[:, 0:1], u)
    assert pred.shape[0] == 50 and np.max(np.abs(pred[:, 19] - snaps[:, 20])) < 5e-2


# ---- Householder TSQR thin-Q (CORRLA_QR_HOUSEHOLDER, csrc/tsqr_kernels.hpp) --------------------------------------
@pytest.mark.parametrize("name", ["tall64x48", "lowrank256x96", "gauss512x256", "fat48x64", "square40_lcap", "rankdef96x40", "known5x5_k5"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_householder_tsqr_rsvd_on_the_golden_fixtures(ctx, name, dtype):
    from oracle import rsvd_oracle as orc
    g = load_golden(name)
    a, om = g["A"].astype(dtype), g["omega"].astype(dtype)
    u, s, vt = ctx.rsvd(a, g["k"], g["q"], g["p"], omega=om, qr="householder")
    uo, so, vo = orc.random_svd(g["A"], g["k"], g["q"], g["p"], omega=g["omega"])
    tol = 1e-9 if dtype == np.float64 else 2e-4
    assert np.max(np.abs(s.ravel() - so.ravel())) < tol * so[0, 0]
    # f32 on the fixtures whose sketch f32 cannot resolve (decaying spectra after un-orthonormalised
    # power iterations, exactly rank-deficient input) is held to the bound the default path's golden test uses for them
    # (round 2 skipped the comparison there)
    well_posed = dtype == np.float64 or name in ("tall64x48", "gauss512x256", "fat48x64")
    rtol = (1e-9 if dtype == np.float64 else 1e-5) if well_posed else 2e-2
    assert abs(orc.relerr(a, u, s, vt) - orc.relerr(g["A"], uo, so, vo)) < rtol
    k = g["k"]
    otol = 1e-12 if dtype == np.float64 else 2e-5
    assert np.max(np.abs(u.T.astype(np.float64) @ u - np.eye(k))) < otol
    assert np.max(np.abs(vt.astype(np.float64) @ vt.T - np.eye(k))) < otol


@pytest.mark.parametrize("m,n,width,dtype", [(5000, 300, 138, np.float32), (20000, 200, 97, np.float64), (277, 150, 138, np.float32),
                                             (100000, 64, 32, np.float64), (1000, 40, 1, np.float32), (3001, 90, 33, np.float64)])
def test_householder_tsqr_power_iter_q(ctx, m, n, width, dtype):
    """Wide panels (l = 138 f32 / 97 f64; the widest that fit are 142 / 99), a single leaf, odd panel counts, many panels: Q orthonormal
    and spanning the oracle's Householder Q of the same sketch."""
    from oracle import rsvd_oracle as orc
    rng = np.random.default_rng(m + width)
    a = rng.standard_normal((m, n)).astype(dtype)
    om = rng.standard_normal((n, width)).astype(dtype)
    q = ctx.power_iter(a, width, 1, omega=om, qr="householder")
    qo = orc.power_iter(a.astype(np.float64), om.astype(np.float64), 1)
    q64 = q.astype(np.float64)
    tol = 1e-12 if dtype == np.float64 else 1e-5
    assert np.max(np.abs(q64.T @ q64 - np.eye(width))) < tol
    assert np.linalg.norm(q64 @ (q64.T @ qo) - qo) < tol * 100


def test_householder_tsqr_rank_deficient_and_fallbacks(ctx, torch, monkeypatch):
    rng = np.random.default_rng(3)
    a = rng.standard_normal((3000, 4)) @ rng.standard_normal((4, 60))          # exact rank 4, sketch width 20
    q = ctx.power_iter(a, 20, 1, omega=rng.standard_normal((60, 20)), qr="householder")
    assert np.max(np.abs(q.T @ q - np.eye(20))) < 1e-12                        # orthonormal whatever the rank
    u, s, vt = ctx.rsvd(a, 10, 2, 10, seed=1, qr="householder")
    assert np.allclose(s[:4, 0], np.linalg.svd(a, compute_uv=False)[:4], rtol=1e-10) and np.all(s[4:, 0] < 1e-9 * s[0, 0])
    assert np.max(np.abs(u.T @ u - np.eye(10))) < 1e-10 and np.max(np.abs(vt @ vt.T - np.eye(10))) < 1e-10
    # a sketch wider than one LDS panel (l = 160 f64) goes through column blocks; CUDA tensors and the environment switch
    b = rng.standard_normal((2000, 400))
    u1, s1, vt1 = ctx.rsvd(b, 150, 1, 10, seed=2, qr="householder")
    u0, s0, vt0 = ctx.rsvd(b, 150, 1, 10, seed=2)
    assert np.allclose(s0, s1, rtol=1e-11) and not np.array_equal(u0, u1)
    assert np.linalg.norm((u0 * s0.ravel()) @ vt0 - (u1 * s1.ravel()) @ vt1) < 1e-10 * np.linalg.norm(b)
    bt = torch.as_tensor(b[:, :100].copy(), device="cuda")
    ud, sd, vtd = ctx.rsvd(bt, 20, 2, 10, seed=4, qr="householder")
    monkeypatch.setenv("CORRLA_QR", "householder")
    ue, se, vte = ctx.rsvd(bt, 20, 2, 10, seed=4)
    monkeypatch.delenv("CORRLA_QR")
    uc, sc, vtc = ctx.rsvd(bt, 20, 2, 10, seed=4)
    assert torch.equal(sd, se) and torch.allclose(sd, sc, rtol=1e-10) and not torch.equal(ud, uc)
    with pytest.raises(ValueError):
        ctx.rsvd(b, 10, 1, 5, qr="givens")


@pytest.mark.parametrize("m,n,width,dtype", [(6000, 400, 142, np.float32), (6000, 400, 143, np.float32), (6000, 400, 352, np.float32),
                                             (20000, 300, 99, np.float64), (20000, 300, 100, np.float64), (8000, 600, 266, np.float64),
                                             (400, 360, 352, np.float64)])
def test_householder_wider_than_one_panel_goes_through_column_blocks(ctx, m, n, width, dtype):
    """l > 142 (f32) / 99 (f64) up to the library's 352: column blocks of at most one LDS panel, each the thin-Q of
    (I - Q Q^T) Y_j repeated around the Householder panels until the overlap the panel saw was small.  Q orthonormal to
    O(eps) and spanning the oracle's Householder Q; orthonormal also for a sketch of rank 5 (random_svd.rs:38,57 has no
    width limit and no rank condition)."""
    from oracle import rsvd_oracle as orc
    rng = np.random.default_rng(m + width)
    eps = np.finfo(dtype).eps
    a = rng.standard_normal((m, n)).astype(dtype)
    om = rng.standard_normal((n, width)).astype(dtype)
    q64 = ctx.power_iter(a, width, 1, omega=om, qr="householder").astype(np.float64)
    qo = orc.power_iter(a.astype(np.float64), om.astype(np.float64), 1)
    assert np.max(np.abs(q64.T @ q64 - np.eye(width))) < 100 * eps
    assert np.linalg.norm(q64 @ (q64.T @ qo) - qo) < (1e-10 if dtype == np.float64 else 2e-3)
    low = (rng.standard_normal((m, 5)) @ rng.standard_normal((5, n))).astype(dtype)
    q64 = ctx.power_iter(low, width, 1, omega=om, qr="householder").astype(np.float64)
    assert np.max(np.abs(q64.T @ q64 - np.eye(width))) < 100 * eps
    u, s, vt = ctx.rsvd(a, width - 10, 4, 10, omega=om, qr="householder")
    uo, so, vo = orc.random_svd(a, width - 10, 4, 10, omega=om)
    assert np.max(np.abs(s.ravel() - so.ravel())) < (1e-9 if dtype == np.float64 else 2e-4) * so[0, 0]
    assert abs(orc.relerr(a, u, s, vt) - orc.relerr(a, uo, so, vo)) < (1e-9 if dtype == np.float64 else 1e-5)


def test_householder_panels_survive_columns_of_denormal_size(ctx):
    """The blocked panels take sqrt / reciprocals from the hardware approximations, which flush denormals: a trailing
    column whose squared norm is denormal (a decaying f32 sketch after three un-orthonormalised power iterations) must
    count as already reduced instead of producing 1 / 0 (found by tools/fuzz_parity.py, seed 62 case 23)."""
    from oracle import rsvd_oracle as orc
    rng = np.random.default_rng(23)
    a = (rng.standard_normal((55, 392)) * (0.93 ** np.arange(392))).astype(np.float32)
    om = rng.standard_normal((55, 8)).astype(np.float32)
    u, s, vt = ctx.rsvd(a, 5, 3, 3, omega=om, qr="householder")
    uo, so, vo = orc.random_svd(a.astype(np.float64), 5, 3, 3, omega=om.astype(np.float64))
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(u)) and np.all(np.isfinite(vt))
    assert np.max(np.abs(s.ravel() - so.ravel())) < 2e-4 * so[0, 0]
    # columns far below the normal range: every reflector of the panel sees a (sub)normal norm
    tiny = (rng.standard_normal((600, 40)) * 1e-30).astype(np.float32)
    tiny[:, 20:] *= 1e-12
    q = ctx.power_iter(tiny, 30, 0, omega=rng.standard_normal((40, 30)).astype(np.float32), qr="householder")
    assert np.all(np.isfinite(q))
    assert np.max(np.abs(q.T.astype(np.float64) @ q - np.eye(30))) < 1e-5


def test_householder_on_the_sharded_entry_point_world_size_1_rccl(torch, monkeypatch):
    """Cross-rank TSQR on a real one-rank RCCL communicator with every all-reduce issued (the stack of root R factors
    is the one R; the N = 2 exchange runs on the CPU through the same driver, tests/test_sharded_gloo.py): one panel
    (l = 26), column blocks (l = 200 f32) and a rank-deficient input; same factorisation as the unsharded Householder
    call and as the default path."""
    import corrla_rs_amd as cr
    c = cr.Context(0)
    c.comm_init(cr.Context.unique_id(), 0, 1)
    monkeypatch.setenv("CORRLA_FORCE_ALLREDUCE", "1")
    g = torch.Generator(device="cuda").manual_seed(1)
    for (m, n, k, dt, tol) in ((3000, 200, 16, torch.float32, 2e-5), (5000, 400, 190, torch.float32, 5e-5), (3000, 200, 16, torch.float64, 1e-11)):
        a = torch.randn((m, n), dtype=dt, device="cuda", generator=g)
        om = np.random.default_rng(2).standard_normal((n, k + 10)).astype(np.float32 if dt == torch.float32 else np.float64)
        u1, s1, vt1 = c.rsvd_sharded(a, k, 4, 10, omega=om, qr="householder")
        u2, s2, vt2 = c.rsvd(a, k, 4, 10, omega=om, qr="householder")
        u0, s0, vt0 = c.rsvd(a, k, 4, 10, omega=om)
        eye = torch.eye(k, dtype=torch.float64, device="cuda")
        assert (u1.double().T @ u1.double() - eye).abs().max().item() < 10 * tol
        for (u, s, vt) in ((u2, s2, vt2), (u0, s0, vt0)):
            assert (s - s1).abs().max().item() <= tol * s1[0].item() * 10
            assert torch.linalg.norm((u * s.ravel()) @ vt - (u1 * s1.ravel()) @ vt1).item() <= 100 * tol * torch.linalg.norm(a).item()
    low = torch.randn((3000, 4), dtype=torch.float64, device="cuda", generator=g) @ torch.randn((4, 60), dtype=torch.float64, device="cuda", generator=g)
    u, s, vt = c.rsvd_sharded(low, 10, 2, 10, seed=3, qr="householder")
    assert (u.T @ u - torch.eye(10, dtype=torch.float64, device="cuda")).abs().max().item() < 1e-10
    assert torch.all(s.ravel()[4:] < 1e-9 * s.ravel()[0])
    monkeypatch.delenv("CORRLA_FORCE_ALLREDUCE")
    c.close()


# ---- DMDc / POD with the n_x- and N-sized factors resident on the device ---------------------------
def _lti_snapshots(n_x, n_t, k, n_u, seed):
    """x_{t+1} = A x_t + B u_t with rank-k dynamics inside an n_x-dimensional state (distinct stable eigenvalues)."""
    rng = np.random.default_rng(seed)
    basis = np.linalg.qr(rng.standard_normal((n_x, k)))[0]
    az = np.diag(np.linspace(0.55, 0.97, k)) + 0.05 * np.triu(rng.standard_normal((k, k)), 1)
    bz = rng.standard_normal((k, n_u))
    u = rng.standard_normal((n_u, n_t))
    z = rng.standard_normal((k, 1))
    xs = []
    for t in range(n_t):
        xs.append((basis @ z)[:, 0])
        z = az @ z + bz @ u[:, t:t + 1]
    return np.array(xs).T, u, basis @ az @ basis.T, basis @ bz


@pytest.mark.parametrize("n_x,n_t,k,n_u", [(300, 60, 6, 2), (2000, 90, 8, 1), (64, 50, 5, 3)])
def test_dmdc_device_resident_matches_oracle_and_truth(ctx, torch, n_x, n_t, k, n_u):
    """CUDA tensors in: factors stay on the device, the predictor is factored (2 n_modes-dimensional recurrence + one
    GEMM).  Same shared sketches as the oracle -> same operators and the same predictions."""
    import corrla_rs_amd as cr
    from oracle import callers_oracle as co
    x, u, a_true, b_true = _lti_snapshots(n_x, n_t, k, n_u, seed=n_x)
    rng = np.random.default_rng(5)
    om_x = rng.standard_normal((min(n_x + n_u, n_t - 1), min(k + 12, min(n_x + n_u, n_t - 1))))
    om_y = rng.standard_normal((min(n_x, n_t - 1), min(k + 12, min(n_x, n_t - 1))))
    xd, ud = torch.as_tensor(x, device="cuda"), torch.as_tensor(u, device="cuda")
    md = cr.DMDc(xd, ud, 1.0, k, 6, omega_x=om_x, omega_y=om_y, ctx=ctx)
    mh = cr.DMDc(x, u, 1.0, k, 6, omega_x=om_x, omega_y=om_y, ctx=ctx)
    mo = co.DMDcOracle(x, u, 1.0, k, 6, omega_x=om_x, omega_y=om_y)
    assert md.on_device and md.est_b_til().is_cuda and md.modes_re.is_cuda and md.modes_re.shape == (n_x, k)
    sc = np.abs(mo.est_a_til()).max()
    ad = md.est_a_til()
    assert ad.is_cuda and ad.shape == (n_x, n_x)
    assert np.max(np.abs(ad.cpu().numpy() - mo.est_a_til())) < 1e-7 * sc
    assert np.max(np.abs(mh.est_a_til() - mo.est_a_til())) < 1e-7 * sc
    assert np.max(np.abs(md.est_b_til().cpu().numpy() - mo.est_b_til())) < 1e-8 * np.abs(mo.est_b_til()).max()
    assert np.allclose(np.sort_complex(md.lambdas.ravel()), np.sort_complex(mo.lambdas.ravel()), atol=1e-8)
    # factored multi-step prediction == the dense recurrence of the reference
    u_seq = u[:, :40]
    pd_ = md.predict_multiple(xd[:, 0:1], u_seq)
    assert pd_.is_cuda and pd_.shape == (n_x, 40)
    po = mo.predict_multiple(x[:, 0:1], u_seq)
    assert np.max(np.abs(pd_.cpu().numpy() - po)) < 1e-7 * np.abs(po).max()
    p1 = md.predict(x[:, 3:4], u[:, 3:4])
    assert p1.shape == (n_x, 1)
    assert np.max(np.abs(p1.cpu().numpy() - (mo.est_a_til() @ x[:, 3:4] + mo.est_b_til() @ u[:, 3:4]))) < 1e-7 * np.abs(x).max()
    with pytest.raises(ValueError):
        md.predict_multiple(x[:5, 0:1], u_seq)


def test_dmdc_device_resident_with_more_modes_than_the_data_has(ctx, torch):
    """n_modes above the rank of the output space: A~ has null eigen-directions whose modes are rounding noise.  The
    factored predictor must ignore them (as the pseudo-inverse of the modes does) and still reproduce the data."""
    import corrla_rs_amd as cr
    from oracle import callers_oracle as co
    x, u, _a, _b = _lti_snapshots(3000, 120, 10, 3, seed=8)
    m = cr.DMDc(torch.as_tensor(x, device="cuda"), torch.as_tensor(u, device="cuda"), 1.0, 13, 4, seed=2, ctx=ctx)
    pred = m.predict_multiple(x[:, 0:1], u[:, :100]).cpu().numpy()
    assert np.max(np.abs(pred - x[:, 1:101])) < 1e-8 * np.abs(x).max()
    mo = co.DMDcOracle(x, u, 1.0, 13, 4)
    assert np.max(np.abs(mo.predict_multiple(x[:, 0:1], u[:, :100]) - x[:, 1:101])) < 1e-8 * np.abs(x).max()


@pytest.mark.parametrize("nx,nt", [(50, 40), (500, 40)])
def test_dmdc_reference_test_device_resident(ctx, torch, nx, nt):
    """test_dmdc (dmd_rom.rs:233-310) with CUDA tensors: 14 modes, the 20-step prediction within 5e-2."""
    import corrla_rs_amd as cr
    from oracle import callers_oracle as co
    snaps, u = co.dmdc_reference_test_data(nx, nt)
    m = cr.DMDc(torch.as_tensor(snaps, device="cuda"), torch.as_tensor(u, device="cuda"), 1.0, 14, 40, seed=3, ctx=ctx)
    assert m.lambdas.shape[0] == 14 and m.est_a_til().shape == (nx, nx) and m.est_b_til().shape == (nx, 1)
    pred = m.predict_multiple(snaps[:, 0:1], u).cpu().numpy()
    assert np.max(np.abs(pred[:, 19] - snaps[:, 20])) < 5e-2


def test_podi_matches_the_oracle(ctx, torch):
    """PodI on the reference's test_pod data (pod_rom.rs:122-160): same sketch -> same modes (up to sign), same mode
    weights (X * modes on the GPU == pinv(modes) x^T), same interpolated prediction; numpy and CUDA inputs."""
    import corrla_rs_amd as cr
    from oracle import callers_oracle as co
    x, t = co.pod_reference_test_data()
    om = np.random.default_rng(4).standard_normal((20, 14))
    mo = co.PodIOracle(x, t, 4, omega=om)
    for xin in (x, torch.as_tensor(x, device="cuda")):
        m = cr.PodI(xin, t, 4, omega=om, ctx=ctx)
        modes = m.modes.cpu().numpy() if m.on_device else m.modes
        assert modes.shape == (100, 4)
        assert np.linalg.norm(modes @ modes.T - mo.modes @ mo.modes.T) < 1e-8
        p = m.predict(np.array([[5.2]]))
        assert (p.is_cuda if m.on_device else isinstance(p, np.ndarray)) and p.shape == (100, 1)
        pn = p.cpu().numpy() if m.on_device else p
        assert np.max(np.abs(pn - mo.predict(np.array([[5.2]])))) < 1e-8 * np.abs(mo.predict(np.array([[5.2]]))).max() + 1e-12
        many = m.predict_many(np.array([[2.0], [5.2], [7.7]]))
        many = many.cpu().numpy() if m.on_device else many
        assert many.shape == (100, 3) and np.max(np.abs(many[:, 1:2] - pn)) < 1e-12
        with pytest.raises(ValueError):
            m.predict(np.array([[1.0], [2.0]]))


def test_drop_in_pypodi_pyrbf_active_ss(ctx):
    """from corrla_rs import PyPodI, PyRbfInterp, active_ss (lib_math_utils_py.rs:57-86, 178-250)."""
    from corrla_rs import PyPodI, PyRbfInterp, active_ss
    from oracle import active_ss_oracle as aso
    from oracle import callers_oracle as co
    x, t = co.pod_reference_test_data()
    pod = PyPodI(x, t, 4)
    p = pod.predict(np.array([[5.2]]))
    assert p.shape == (100, 1)
    # rank-4 reconstruction of a field between two snapshots: close to the projection of the true field on the modes
    truth = (0.5 * 5.2) * np.exp(-((np.linspace(0, 10, 100) - 5.2) ** 2) / 0.25 ** 2)
    modes = pod.pod.modes
    assert np.linalg.norm(p.ravel() - modes @ (modes.T @ truth)) < 0.5 * np.linalg.norm(truth)
    rb = PyRbfInterp(2, 1.0, 2, 1)
    xs = np.random.default_rng(0).standard_normal((40, 2))
    ys = (np.sin(xs[:, 0]) + np.sin(xs[:, 1])).reshape(-1, 1)
    rb.fit(xs, ys)
    assert np.max(np.abs(rb.predict(xs) - ys)) < 1e-6
    # active_ss on the reference's test_active_ss function (active_subspaces.rs:331-394)
    xa = aso.sample_mv_normal([[0.9, 0.5, 0.5], [0.5, 0.9, 0.5], [0.5, 0.5, 0.9]], 100, np.random.default_rng(7))
    ya = (0.2 * xa[:, 0] + 0.5 * xa[:, 1] ** 2 + 0.10 * xa[:, 2] * xa[:, 0]).reshape(-1, 1)
    comps, sv, sensi = active_ss(xa, ya, 2, 14, 2)
    assert comps.shape == (3, 2) and sv.shape == (3, 2) and sensi.shape == (3,)
    assert abs(comps[0, 0]) < abs(comps[1, 0]) and sensi[1] > sensi[0] and sensi[1] > sensi[2]
    go = aso.create_grad_mat(aso.PolyGradientEstimator(xa, ya, 2, 14), xa)
    lam = np.sort(np.linalg.eigvalsh(go @ go.T / 100.0))[::-1]
    assert np.allclose(np.diag(sv[:2, :2]), lam[:2], rtol=1e-4)


def test_pod_modes_and_active_ss_fit_svd(ctx):
    import corrla_rs_amd as cr
    from oracle import callers_oracle as co
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((20, 6)) * [10, 7, 5, 1e-2, 1e-3, 1e-4]) @ rng.standard_normal((6, 5000))
    om = rng.standard_normal((20, 13))
    mg, mo = cr.pod_modes(x, 3, omega=om, ctx=ctx), co.pod_modes(x, 3, omega=om)   # benchmark_pod.py shape: 20 x 5000
    assert mg.shape == (5000, 3) and np.linalg.norm(mg @ mg.T @ mo - mo) < 1e-8
    g = (rng.standard_normal((8, 8)) * [5, 3, 2, 1, .1, .01, .001, .0001]) @ rng.standard_normal((8, 4000))
    om2 = rng.standard_normal((8, 8))
    ug, sg = cr.active_ss_fit_svd(g, 4, omega=om2, ctx=ctx)
    uo, so = co.active_ss_fit_svd(g, 4, omega=om2)
    assert np.allclose(np.diag(sg), np.diag(so), rtol=1e-9)
    assert np.linalg.norm(ug @ ug.T - uo @ uo.T) < 1e-7


def test_sharded_entry_point_with_world_size_1_rccl(torch, monkeypatch):
    """The row-sharded entry point with a real RCCL communicator of one rank equals the plain entry point
    (the N > 1 exchange logic is covered by tests/test_sharded_gloo.py through the same driver)."""
    import corrla_rs_amd as cr
    c = cr.Context(0)
    c.comm_init(cr.Context.unique_id(), 0, 1)
    g = torch.Generator(device="cuda").manual_seed(1)
    a = torch.randn((3000, 200), dtype=torch.float32, device="cuda", generator=g)
    om = np.random.default_rng(2).standard_normal((200, 26)).astype(np.float32)
    u1, s1, vt1 = c.rsvd_sharded(a, 16, 4, 10, omega=om)
    u0, s0, vt0 = c.rsvd(a, 16, 4, 10, omega=om)
    assert torch.equal(s0, s1) and torch.equal(u0, u1) and torch.equal(vt0, vt1)
    # the same with every all-reduce actually issued to RCCL (identity on one rank): the calls the N > 1 ranks make
    monkeypatch.setenv("CORRLA_FORCE_ALLREDUCE", "1")
    u2, s2, vt2 = c.rsvd_sharded(a, 16, 4, 10, omega=om)
    ad = a.double()
    u3, s3, vt3 = c.rsvd_sharded(ad, 16, 4, 10, omega=om.astype(np.float64))
    monkeypatch.delenv("CORRLA_FORCE_ALLREDUCE")
    assert torch.equal(s0, s2) and torch.equal(u0, u2) and torch.equal(vt0, vt2)
    assert torch.allclose(s3.float(), s0, rtol=1e-4)
    c.close()


def test_active_subspace_fit_svd_sharded_world_size_1(torch):
    """BASELINE config 5's multi-GPU shape (queries sharded, cloud replicated, row-sharded RSVD of G^T) rehearsed with
    one rank and a real RCCL communicator: same spectrum and subspace as the single-process fit_svd."""
    import corrla_rs_amd as cr
    c = cr.Context(0)
    c.comm_init(cr.Context.unique_id(), 0, 1)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((4000, 12))
    y = np.sin(x[:, 0] + 0.5 * x[:, 3]) + 0.1 * x[:, 7] ** 2
    est = cr.PolyGradientEstimator(x, y, 1, 30, ctx=c)
    act = cr.ActiveSsRsvd(est, 3, ctx=c)
    f1 = act.fit_svd_sharded(x, 0, 1, seed=5)
    f0 = act.fit_svd(x, seed=5)
    assert np.allclose(np.diag(f1.singular_vals_), np.diag(f0.singular_vals_), rtol=1e-9)
    assert np.linalg.norm(f1.components_ @ f1.components_.T - f0.components_ @ f0.components_.T) < 1e-8
    assert abs(f0.components_[0, 0]) > 0.5      # the active direction is dominated by x0
    c.close()


def test_sign_convention_is_stable_across_svd_paths(ctx, monkeypatch):
    """Largest-magnitude component of the short-side singular vector is positive, so the LDS, block and host
    SVD paths return the same signs (bitwise-different rounding, identical orientation)."""
    g = load_golden("gauss512x256")
    a, om = g["A"], g["omega"]
    u0, s0, vt0 = ctx.rsvd(a, g["k"], g["q"], g["p"], omega=om)
    for i in range(g["k"]):
        assert vt0[i, int(np.argmax(np.abs(vt0[i, :])))] > 0
    for mode in ("block", "host"):
        monkeypatch.setenv("CORRLA_SVD", mode)
        u1, s1, vt1 = ctx.rsvd(a, g["k"], g["q"], g["p"], omega=om)
        monkeypatch.delenv("CORRLA_SVD")
        assert np.max(np.abs(vt1 - vt0)) < 1e-8 and np.max(np.abs(u1 - u0)) < 1e-8
    ua, sa, vta = ctx.rsvd(np.ascontiguousarray(a.T), g["k"], g["q"], g["p"], omega=om)   # fat: roles swap
    for i in range(g["k"]):
        assert ua[int(np.argmax(np.abs(ua[:, i]))), i] > 0
    assert np.max(np.abs(ua - vt0.T)) < 1e-8


# ---- active-subspace gradient stage (active_subspaces.rs:66-141, 215-277) ---------
def _as_samples(cov, n, seed):
    from oracle import active_ss_oracle as aso
    return aso.sample_mv_normal(cov, n, np.random.default_rng(seed))


@pytest.mark.parametrize("case", ["lin_k6", "lin_k64", "quad_k2", "quad_k3", "quad_k9", "quad_k10", "quad_k12", "quad_k14",
                                  "lin_k20"])
def test_grad_mat_matches_the_oracle(ctx, case):
    """Exact nearest neighbours + local least-squares fits on the GPU against the numpy restatement: same neighbour
    sets (ties -> lower index), gradients equal to rounding (order 2: the oracle follows the reference's forward
    differences with eps = 1e-10, the GPU takes the analytic gradient of the same fitted quadratic)."""
    from oracle import active_ss_oracle as aso
    rng = np.random.default_rng(len(case))
    order = 1 if case.startswith("lin") else 2
    k = int(case.split("k")[1])
    n = {"lin_k6": 500, "lin_k64": 900, "quad_k2": 100, "quad_k3": 100, "quad_k9": 700, "quad_k10": 900, "quad_k12": 1200,
         "quad_k14": 1500, "lin_k20": 2000}[case]
    # (quad_k12 / quad_k14: 91 / 120 design columns, lin_k20: 400 neighbours -- beyond the 66 columns / 160 neighbours of
    # round 1; the bound is one query's LDS footprint now)
    n_nbrs = {"lin_k6": 12, "lin_k64": 90, "quad_k2": 14, "quad_k3": 14, "quad_k9": 80, "quad_k10": 100, "quad_k12": 130,
              "quad_k14": 150, "lin_k20": 400}[case]
    x = rng.standard_normal((n, k)) + 1.5
    w = rng.standard_normal(k)
    y = np.sin(x @ w * 0.3) + 0.1 * (x ** 2).sum(axis=1) - 4.0
    nq = 40
    g, nreg = ctx.grad_mat(x, y, order, n_nbrs, x[:nq])
    assert g.shape == (k, nq) and nreg == 0
    est = aso.PolyGradientEstimator(x, y, order, n_nbrs)
    go = aso.create_grad_mat(est, x[:nq])
    scale = np.abs(go).max()
    assert np.max(np.abs(g - go)) <= (1e-9 if order == 1 else 1e-4) * scale
    if order == 2:   # the same fitted quadratics differentiated exactly: the fits agree to rounding
        est.exact_quad_gradient = True
        assert np.max(np.abs(g - aso.create_grad_mat(est, x[:nq]))) <= 1e-8 * scale
    # all queries at once == the support points as queries (create_grad_mat's own use)
    g_all, _ = ctx.grad_mat(x, y, order, n_nbrs)
    assert g_all.shape == (k, n) and np.array_equal(g_all[:, :nq], g)


def test_reference_active_subspace_tests_on_gpu(ctx):
    """test_grad_est and test_active_ss (active_subspaces.rs:286-394) through the GPU gradient stage and the GPU RSVD."""
    import corrla_rs_amd as cr
    from oracle import active_ss_oracle as aso
    x = _as_samples([[0.9, 0.5], [0.5, 0.9]], 100, 20241008)
    y = x[:, 0] ** 2 + x[:, 1] ** 2
    est = cr.PolyGradientEstimator(x, y, 2, 14, ctx=ctx)
    assert np.allclose(est.grad_at([0.0, 0.0]), [[0.0, 0.0]], atol=1e-2)
    g1, g2 = est.grad_at([1.0, 0.0]), est.grad_at([-1.0, 0.0])
    assert g1.shape == (1, 2) and np.allclose(g1, [[2.0, 0.0]], atol=1e-2) and np.allclose(g1, -g2, atol=1e-2)

    x = _as_samples([[0.9, 0.5, 0.5], [0.5, 0.9, 0.5], [0.5, 0.5, 0.9]], 100, 7)
    y = 0.2 * x[:, 0] + 0.5 * x[:, 1] ** 2 + 0.10 * x[:, 2] * x[:, 0]
    est = cr.PolyGradientEstimator(x, y, 2, 14, ctx=ctx)
    act = cr.ActiveSsRsvd(est, 2, ctx=ctx)
    fit = act.fit(x)
    assert abs(fit.components()[0, 0]) < abs(fit.components()[1, 0])
    assert fit.singular_vals()[0, 0] > fit.singular_vals()[1, 1]
    assert np.allclose(est.grad_at([0.0, 1.0, 0.0]), [[0.2, 1.0, 0.0]], atol=1e-1)
    tr = fit.transform(x)
    assert tr.shape == (100, 2) and fit.inv_transform(tr).shape == (100, 3)
    sens = fit.var_diag_evd_sensi()
    assert sens.shape == (3,) and sens[1] > sens[0] and sens[1] > sens[2]
    # fit_svd (no reference test): equals the oracle with the same Omega
    om = np.random.default_rng(1).standard_normal((3, 3))
    fs = act.fit_svd(x, omega=om)
    uo, so = aso.fit_svd(aso.PolyGradientEstimator(x, y, 2, 14), x, 2, omega=om)
    assert np.allclose(np.diag(fs.singular_vals_), np.diag(so), rtol=1e-6)
    assert np.linalg.norm(fs.components_ @ fs.components_.T - uo @ uo.T) < 1e-6


def test_quadratic_fit_carries_the_constant_term(ctx):
    """build_vandermonde appends a ones column (stats_corr.rs:198-207): an exact quadratic WITH an offset, sampled away
    from the origin, is recovered exactly -- a fit without the constant could not."""
    rng = np.random.default_rng(12)
    k = 5
    x = rng.standard_normal((600, k)) + 4.0
    q = rng.standard_normal((k, k))
    q = q + q.T
    b = rng.standard_normal(k)
    y = 0.5 * np.einsum("ni,ij,nj->n", x, q, x) + x @ b + 37.5
    g, nreg = ctx.grad_mat(x, y, 2, 45, x[:64])
    assert nreg == 0
    assert np.max(np.abs(g - (x[:64] @ q + b).T)) < 1e-7 * np.abs(g).max()


def test_knn_kernels_agree(ctx, monkeypatch):
    """The VALU scan and the MFMA-filtered scan (exact re-check of every candidate) return the same neighbour sets,
    hence the same gradients, including a cloud with repeated points (equal distances -> lower index)."""
    rng = np.random.default_rng(21)
    x = rng.standard_normal((3000, 24))
    x[1000:1500] = x[:500]                      # exact duplicates
    y = np.cos(x @ rng.standard_normal(24) * 0.2)
    out = {}
    for mode in ("1", "2"):
        monkeypatch.setenv("CORRLA_KNN", mode)
        out[mode], _ = ctx.grad_mat(x, y, 1, 60, x[:700])
    monkeypatch.delenv("CORRLA_KNN")
    assert np.max(np.abs(out["1"] - out["2"])) <= 1e-10 * np.abs(out["1"]).max()


def test_grad_mat_argument_checks(ctx):
    x = np.random.default_rng(0).standard_normal((50, 4))
    y = x.sum(axis=1)
    for bad in (dict(est_order=3, n_nbrs=10), dict(est_order=1, n_nbrs=5), dict(est_order=2, n_nbrs=14),
                dict(est_order=1, n_nbrs=60), dict(est_order=1, n_nbrs=200)):
        with pytest.raises(ValueError):
            ctx.grad_mat(x, y, bad["est_order"], bad["n_nbrs"])


def test_grad_mat_device_tensors_and_duplicate_points(ctx, torch):
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn((4000, 16), dtype=torch.float64, device="cuda", generator=g)
    w = torch.arange(1.0, 17.0, dtype=torch.float64, device="cuda")
    y = x @ w + 2.0
    gm, nreg = ctx.grad_mat(x, y, 1, 40)
    assert gm.is_cuda and gm.shape == (16, 4000) and nreg == 0
    assert torch.allclose(gm, w.reshape(-1, 1).expand(16, 4000), atol=1e-8)     # affine function: exact slopes
    # a degenerate cloud (every point repeated): the neighbour set of a query collapses onto few distinct points
    xd = x[:40].repeat_interleave(25, dim=0)
    gd, nreg = ctx.grad_mat(xd, xd @ w, 1, 20)
    assert nreg > 0 and torch.isfinite(gd).all()
    # every point twice, y drawn independently of x, 41 neighbours: the query's two copies, 19 pairs and ONE copy of the
    # next pair -- the lower index, as in the reference (with y = f(x) either copy gives the same gradient);
    # tests/test_grad_reference.py asserts that every query's cut separates a pair and that the other copy would show
    from tests import grad_reference as gr
    xp, yp, xqp = (torch.tensor(a, device="cuda") for a in gr.paired_cloud(16))
    g2, nreg = ctx.grad_mat(xp, yp, 1, gr.PAIRED_CLOUDS[16][1], xqp)
    go, _, _ = gr.reference("paired", 16, 1, gr.PAIRED_CLOUDS[16][1], gr.N_QUERIES)
    assert nreg == 0 and gr.feature_unit_error(g2.cpu().numpy(), go) <= 1e-9


def test_randomised_parity_sweep(ctx):
    """tools/fuzz_parity.py: random shapes / dtypes / layouts / ranks / q / p / spectra (flat, decaying, rank-deficient,
    scaled by 1e-6..1e6) against the oracle with a shared Omega, restricted to sketches the arithmetic can resolve."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bad, worst = mod.run(150, seed=3, ctx=ctx, verbose=True)
    assert bad == 0, worst
    assert worst["ds"] < 1e-8 and worst["relerr"] < 1e-8 and worst["orth"] < 1e-10


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rank_deficient_input_still_gets_orthonormal_factors(ctx, dtype):
    """Same contract as a Householder thin-Q: U and V^T are orthonormal for rank-deficient inputs too (arbitrary
    completion, zero singular values) -- the reference's rank-3 5x5 example and low-rank tall / fat matrices."""
    rng = np.random.default_rng(8)
    cases = [(orc.KNOWN_ANSWER_A.astype(dtype), 5, 12, 10),
             ((rng.standard_normal((600, 5)) @ rng.standard_normal((5, 140))).astype(dtype), 24, 2, 6),
             ((rng.standard_normal((90, 7)) @ rng.standard_normal((7, 900))).astype(dtype), 20, 5, 10),
             (np.zeros((30, 20), dtype=dtype), 4, 2, 3)]
    for a, k, q, p in cases:
        u, s, vt = ctx.rsvd(a, k, q, p, seed=3)
        tol = 1e-10 if dtype == np.float64 else 2e-4
        assert np.max(np.abs(u.T.astype(np.float64) @ u - np.eye(k))) < tol, a.shape
        assert np.max(np.abs(vt.astype(np.float64) @ vt.T - np.eye(k))) < tol, a.shape
        ex = np.linalg.svd(a.astype(np.float64), compute_uv=False)[:k]
        assert np.allclose(s.ravel(), ex, atol=(1e-9 if dtype == np.float64 else 2e-4) * max(ex[0], 1.0))


@pytest.mark.parametrize("scale", [1e-9, 1e9])  # beyond ~1e-12 the reference schedule itself underflows f32: A A^T A Omega is formed before the first rescale
def test_f32_scale_invariance(ctx, scale):
    """The core SVD pre-scales by an exact power of two and the rotation test avoids the a*b product, so tiny or huge
    f32 inputs give the scaled singular values and the same orthonormal factors (random_svd.rs:53-55 keeps the power
    iteration itself normalised)."""
    rng = np.random.default_rng(31)
    a = (rng.standard_normal((300, 90)) * (0.97 ** np.arange(90))).astype(np.float32)
    om = rng.standard_normal((90, 40)).astype(np.float32)
    u0, s0, vt0 = ctx.rsvd(a, 30, 2, 10, omega=om)
    u1, s1, vt1 = ctx.rsvd((a * np.float32(scale)).astype(np.float32), 30, 2, 10, omega=om)
    assert np.allclose(s1.ravel() / scale, s0.ravel(), rtol=2e-4)
    assert np.max(np.abs(u1.T.astype(np.float64) @ u1 - np.eye(30))) < 2e-4
    assert np.max(np.abs(vt1.astype(np.float64) @ vt1.T - np.eye(30))) < 2e-4
    rec0 = (u0.astype(np.float64) * s0.ravel()) @ vt0.astype(np.float64)
    rec1 = (u1.astype(np.float64) * (s1.ravel() / scale)) @ vt1.astype(np.float64)
    assert np.linalg.norm(rec1 - rec0) <= 2e-3 * np.linalg.norm(rec0)


# ---- one-sweep power iteration Z = A^T (A X) (CORRLA_POWER_FUSED, csrc/ata_kernels.hpp) -------------------
@pytest.mark.parametrize("shape", [(4096, 512), (5000, 300), (9999, 64), (20011, 448), (4200, 16), (70000, 512)])
@pytest.mark.parametrize("q", [0, 1, 2, 4])
def test_one_sweep_power_iteration_matches_oracle(ctx, torch, shape, q):
    """Row-major f32 A with n <= 512: every column-tile count, row counts that are not multiples of the 32-row tile,
    n that is not a multiple of 64, q on both sides of the in-loop thin-Q boundary; shared Omega, vs the oracle and vs
    the two-product schedule."""
    m, n = shape
    rng = np.random.default_rng(m + n + q)
    # mild decay: (sigma_1 / sigma_l)^(2 q + 1) stays far below 1 / eps_f32, so f32 resolves every triplet for every q
    # here (the reference re-orthonormalises only from its fourth iteration on)
    a = (rng.standard_normal((m, n)) * (0.995 ** np.arange(n))).astype(np.float32)
    k = max(1, min(n // 3, 70))
    p = min(10, n - k)
    om = rng.standard_normal((n, k + p)).astype(np.float32)
    at = torch.tensor(a, device="cuda")
    u1, s1, vt1 = ctx.rsvd(at, k, q, p, omega=om, fused=True)
    u0, s0, vt0 = ctx.rsvd(at, k, q, p, omega=om)
    uo, so, vto = orc.random_svd(a.astype(np.float64), k, q, p, omega=om.astype(np.float64))
    u1n, s1n, vt1n = u1.cpu().numpy(), s1.cpu().numpy(), vt1.cpu().numpy()
    assert np.max(np.abs(s1n - so)) <= 3e-5 * so[0, 0]
    assert torch.allclose(s1, s0, rtol=0, atol=3e-5 * float(so[0, 0]))
    assert abs(orc.relerr(a, u1n, s1n, vt1n) - orc.relerr(a, uo, so, vto)) <= 1e-5
    assert orth_err(u1n) < 2e-4 and orth_err(vt1n.T) < 2e-4


def test_one_sweep_is_ignored_outside_its_domain(ctx, torch, monkeypatch):
    """f64, column-major or wide (n > 512) inputs take the two-product schedule whatever the flag says; the environment
    switch CORRLA_POWER_FUSED=1 is the same as the flag; the sharded entry point accepts it too."""
    g = torch.Generator(device="cuda").manual_seed(4)
    a = torch.randn((6000, 200), dtype=torch.float32, device="cuda", generator=g)
    om = np.random.default_rng(1).standard_normal((200, 30)).astype(np.float32)
    for x in (a.double(), a.t().contiguous().t(), torch.randn((5000, 600), dtype=torch.float32, device="cuda", generator=g)):
        o = om.astype(np.float64) if x.dtype == torch.float64 else om
        if x.shape[1] == 600:
            o = np.random.default_rng(2).standard_normal((600, 30)).astype(np.float32)
        r1 = ctx.rsvd(x, 20, 2, 10, omega=o, fused=True)
        r0 = ctx.rsvd(x, 20, 2, 10, omega=o)
        assert torch.equal(r1[1], r0[1]) and torch.equal(r1[0], r0[0])
    f1 = ctx.rsvd(a, 20, 2, 10, omega=om, fused=True)
    monkeypatch.setenv("CORRLA_POWER_FUSED", "1")
    f2 = ctx.rsvd(a, 20, 2, 10, omega=om)
    monkeypatch.delenv("CORRLA_POWER_FUSED")
    assert torch.equal(f1[1], f2[1]) and torch.equal(f1[0], f2[0])
    import corrla_rs_amd as cr
    c = cr.Context(0)
    c.comm_init(cr.Context.unique_id(), 0, 1)
    monkeypatch.setenv("CORRLA_FORCE_ALLREDUCE", "1")
    f3 = c.rsvd_sharded(a, 20, 2, 10, omega=om, fused=True)
    monkeypatch.delenv("CORRLA_FORCE_ALLREDUCE")
    assert torch.equal(f3[1], f1[1])
    c.close()


def test_sharded_completeness_world_size_1(torch, monkeypatch):
    """Column-sharded fat input (CORRLA_SHARD_COLS) and sample-sharded PCA (corrla_pca_sharded_dev_*) on a one-rank RCCL
    communicator with every all-reduce issued: equal to the unsharded entry points (the N = 2 exchange logic runs on the
    CPU through the same driver: tests/test_sharded_gloo.py)."""
    import corrla_rs_amd as cr
    c = cr.Context(0)
    c.comm_init(cr.Context.unique_id(), 0, 1)
    monkeypatch.setenv("CORRLA_FORCE_ALLREDUCE", "1")
    g = torch.Generator(device="cuda").manual_seed(6)
    for dt, tol in ((torch.float64, 1e-10), (torch.float32, 3e-5)):
        a = torch.randn((120, 5000), dtype=dt, device="cuda", generator=g)             # fat
        om = np.random.default_rng(3).standard_normal((120, 26))
        u1, s1, vt1 = c.rsvd_sharded(a, 16, 3, 10, omega=om, shard="cols")
        u0, s0, vt0 = c.rsvd(a, 16, 3, 10, omega=om)
        assert u1.shape == (120, 16) and vt1.shape == (16, 5000)
        assert torch.allclose(s1, s0, rtol=0, atol=tol * float(s0[0, 0]))
        r1 = (u1.double() * s1.double().ravel()) @ vt1.double()
        r0 = (u0.double() * s0.double().ravel()) @ vt0.double()
        assert float((r1 - r0).norm() / r0.norm()) < 100 * tol
        x = torch.randn((3000, 64), dtype=dt, device="cuda", generator=g) * torch.linspace(2, 0.2, 64, device="cuda", dtype=dt) + 1.5
        omp = np.random.default_rng(4).standard_normal((64, 16))
        for center in ("fused", "copy"):
            m1, sp1, c1 = c.pca_sharded(x, 6, omega=omp, center=center)
            m0, sp0, c0 = c.pca(x, 6, omega=omp, center=center)
            assert torch.allclose(m1, m0, atol=tol * 10) and torch.allclose(sp1, sp0, rtol=0, atol=tol * 10 * float(sp0[0, 0]))
            assert float((c1.double().t() @ c1.double() - c0.double().t() @ c0.double()).norm()) < 1e3 * tol
    with pytest.raises(ValueError):
        c.rsvd_sharded(a, 16, 3, 10, shard="diagonal")
    c.close()


# ---- the register-resident thin-Q products of very tall sketches (tall_kernels.hpp) ----------------------------------
@pytest.mark.parametrize("m,n,l,dtype", [(65536, 40, 8, np.float32), (70001, 64, 17, np.float32), (70002, 96, 40, np.float32),
                                         (81923, 128, 64, np.float32), (99999, 200, 80, np.float32),
                                         (131072, 160, 96, np.float32), (70003, 130, 97, np.float32),
                                         (65537, 40, 9, np.float64), (70001, 80, 30, np.float64), (90002, 100, 42, np.float64),
                                         (70003, 128, 64, np.float64), (65600, 128, 65, np.float64)])
def test_tall_thin_q_products_match_the_general_kernels_and_the_oracle(ctx, torch, monkeypatch, m, n, l, dtype):
    """Y R^-1, U = Q U~ and the Gram Y^T Y at m >= 65536, l <= 96 (f32) / 64 (f64) take their own kernels: every
    16-column tile count, row counts that are not multiples of 4 / 64 (scalar tail stores, in-place U with ldu = m),
    l = 97 / 65 just outside their domain; compared with the general kernels (CORRLA_TALL_MIN_ROWS=0) and the f64
    oracle, shared Omega."""
    import corrla_rs_amd as cr
    f32 = dtype == np.float32
    # orthonormality: a few eps * sqrt(rows) (the rounding level of an f32 Gram over 1.3e5 rows is ~4e-5)
    s_tol, o_tol, r_tol = (2e-5, 2e-5, 1e-5) if f32 else (1e-12, 1e-13, 1e-11)
    rng = np.random.default_rng(m + l)
    p = min(5, l - 1)
    k = l - p
    a = (rng.standard_normal((m, n)) * (0.98 ** np.arange(n))).astype(dtype)
    om = rng.standard_normal((n, l)).astype(dtype)
    at = torch.tensor(a, device="cuda")
    u1, s1, vt1 = ctx.rsvd(at, k, 2, p, omega=om)
    monkeypatch.setenv("CORRLA_TALL_MIN_ROWS", "0")
    ctx2 = cr.Context(0)   # the threshold is read when a context is created
    u0, s0, vt0 = ctx2.rsvd(at, k, 2, p, omega=om)
    monkeypatch.delenv("CORRLA_TALL_MIN_ROWS")
    uo, so, vto = orc.random_svd(a.astype(np.float64), k, 2, p, omega=om.astype(np.float64))
    s1n, u1n, vt1n = s1.cpu().numpy(), u1.cpu().numpy(), vt1.cpu().numpy()
    assert np.max(np.abs(s1n - so)) <= s_tol * so[0, 0]
    assert torch.allclose(s1, s0, rtol=0, atol=s_tol * float(so[0, 0]))
    assert orth_err(u1n) < o_tol and orth_err(vt1n.T) < o_tol
    assert abs(orc.relerr(a, u1n, s1n, vt1n) - orc.relerr(a, uo, so, vto)) <= r_tol
    # the host-pointer surface writes U into the caller's m x k buffer (leading dimension m)
    uh, sh, vth = ctx.rsvd(a, k, 2, p, omega=om)
    assert np.max(np.abs(sh - so)) <= s_tol * so[0, 0] and orth_err(uh) < o_tol


# ---- decaying spectra: the thin-Q never leaves the device and stays orthonormal -------------------------------------
@pytest.mark.parametrize("m,n,k,d,dtype", [(4096, 1024, 128, 0.97, np.float32), (4096, 1024, 128, 0.8, np.float32),
                                          (4096, 1024, 128, 0.7, np.float64), (4096, 1024, 190, 0.9, np.float64),
                                          (8192, 1024, 256, 0.7, np.float64), (3000, 600, 256, 0.95, np.float32)])
def test_decaying_spectra_take_the_device_robust_thin_q(ctx, m, n, k, d, dtype):
    """sigma_i = d^i: the sketch's condition number (sigma_1 / sigma_l)^5 is far beyond 1 / sqrt(eps), the case that
    used to repeat the whole call on the host-controlled path (and at l = 266 returned a non-orthonormal U).  One and
    two column blocks, single and 2 x 2 blocked factorisations; shared Omega, against the f64 oracle."""
    rng = np.random.default_rng(m + k)
    a = (rng.standard_normal((m, n)) * (d ** np.arange(n))).astype(dtype)
    p = 10
    om = rng.standard_normal((n, k + p)).astype(dtype)
    u, s, vt = ctx.rsvd(a, k, 2, p, omega=om)
    uo, so, vto = orc.random_svd(a.astype(np.float64), k, 2, p, omega=om.astype(np.float64))
    f32 = dtype == np.float32
    assert orth_err(u) < (2e-5 if f32 else 1e-12) and orth_err(vt.T) < (2e-5 if f32 else 1e-12)
    # the leading singular values: those the arithmetic resolves (sigma_i / sigma_1 above ~eps^(1/5) of the sketch)
    lead = int(np.sum(so.ravel() > (0.2 if f32 else 0.02) * so[0, 0]))
    assert lead >= 2
    assert np.max(np.abs(s.ravel()[:lead] - so.ravel()[:lead])) <= (2e-5 if f32 else 1e-10) * so[0, 0]
    # with q = 2 and no re-orthonormalisation before the fourth iteration the schedule itself resolves only
    # sigma_i / sigma_1 > eps^(1/5): the residual of both implementations is the energy of the unresolved tail (3.5e-4 at
    # d = 0.7 in f64) and they differ in its noise, not in what they resolve
    ro = orc.relerr(a, uo, so, vto)
    assert abs(orc.relerr(a, u, s, vt) - ro) <= (5e-2 if f32 else max(1e-5, 0.25 * ro))
    assert np.all(np.diff(s.ravel()) <= 1e-6 * s[0, 0])  # sorted
