"""PCA on standardised columns (CORRLA_PCA_STANDARDIZE, csrc/colvar_kernels.hpp) on the GPU.  Run with -m gpu on an MI355X.

The oracle of every case: the matrix standardised explicitly in numpy f64 (std with ddof=1; exactly constant columns get
scale 1), then oracle.rsvd_oracle.pca_rsvd on it with the SAME Omega the GPU call gets.  Inputs come from fixed numpy
seeds: column scales spread over 1e-3 .. 1e3, |mean| <= 10 sd, a low-rank-plus-noise correlation structure (so the
leading components are separated) and one exactly constant non-zero column.  The shapes are the smallest that reach both
reduction directions of the variance pass, more than one slab / segment, their tails and the 16-byte-load remainders.

Tolerances are those of the existing PCA parity tests, per dtype:
  against the oracle   tests/test_gpu_parity.py::test_pca_matches_oracle_and_sklearn   S rtol 1e-9 / 1e-4, projector 1e-7 / 2e-3
  fused against copy   tests/test_gpu_parity.py::test_pca_fused_centring_equals_centred_copy   S rtol 1e-10 / 2e-4, projector 1e-8 / 5e-3
  bf16 input           tests/test_gpu_bf16_input.py::test_pca_on_a_bf16_tensor against its f32 oracle   S rtol 1e-4, projector 2e-3
The bound on the scales is 4 x the largest relative error measured on the MI355X per output dtype (profiles/pca_standardize.jsonl)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import rsvd_oracle as orc

pytestmark = pytest.mark.gpu

K = 4
S_RTOL = {"float64": 1e-9, "float32": 1e-4, "bf16": 1e-4}
PROJ_TOL = {"float64": 1e-7, "float32": 2e-3, "bf16": 2e-3}
FUSED_COPY_S_RTOL = {"float64": 1e-10, "float32": 2e-4}
FUSED_COPY_PROJ_TOL = {"float64": 1e-8, "float32": 5e-3}
# largest relative error of `scales` against f64 std(ddof=1) (correctly rounded sums, _standardise) measured on the MI355X
# over the cases of this file: the "scales_max_rel_err" row of profiles/pca_standardize.jsonl (4.275e-16 / 5.749e-8 /
# 4.910e-8, rounded up here); the assertion allows 4 x that (input-dependent rounding)
SCALES_ERR_MEASURED = {"float64": 4.3e-16, "float32": 5.8e-8, "bf16": 5.0e-8}


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


@functools.lru_cache(maxsize=None)
def _data(m, n, seed):
    """m x n, f64 (read-only): unit-spread columns with 8 latent factors of decreasing weight plus noise, then column j
    scaled by sd_j in [1e-3, 1e3] and shifted by a mean with |mean_j| <= 10 sd_j; column n // 2 is the constant 3.25"""
    rng = np.random.default_rng(seed)
    r = 8
    w = rng.standard_normal((r, n)) * (np.arange(r, 0, -1)[:, None] / r)
    z = rng.standard_normal((m, r)) @ w + 0.3 * rng.standard_normal((m, n))
    z = (z - z.mean(axis=0)) / z.std(axis=0)
    sd = 10.0 ** rng.uniform(-3, 3, n)
    sd[1], sd[2] = 1e-3, 1e3
    x = z * sd + sd * rng.uniform(-10, 10, n)
    x[:, n // 2] = 3.25
    x.setflags(write=False)
    return x


def _standardise(x64):
    """explicit standardisation in f64 -> (z, means (1, n), scales (1, n)); exactly constant columns get scale 1.
    The scales are std(ddof=1) with correctly rounded sums (math.fsum): numpy's own std adds the m squares of a column one
    after the other down axis 0, and on a column of 1900 equal small terms (the implicit zeros of a sparse column) every
    addition rounds the same way -- 3.6e-14 relative against the exact value where the GPU's sum is within 1e-16 of it."""
    import math
    m, n = x64.shape
    mu = np.array([[math.fsum(x64[:, j]) / m for j in range(n)]])
    sd = np.array([[math.sqrt(math.fsum((x64[:, j] - mu[0, j]) ** 2) / (m - 1)) for j in range(n)]])
    assert np.allclose(sd, x64.std(axis=0, ddof=1, keepdims=True), rtol=1e-12, atol=0)
    sd[:, (x64 == x64[:1]).all(axis=0)] = 1.0
    return (x64 - mu) / sd, mu, sd


def _omega(m, n, seed):
    nt = min(m, n)
    return np.random.default_rng(seed).standard_normal((nt, min(K + min(n, 10), nt)))


@functools.lru_cache(maxsize=None)
def _oracle(m, n, seed, kind):
    """(values the GPU sees as f64, f64 scales, oracle S, oracle components) of the dense case (m, n, seed) in `kind`"""
    x = _data(m, n, seed)
    if kind == "bf16":
        import torch
        seen = torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).float().numpy().astype(np.float64)
    else:
        seen = x.astype(kind).astype(np.float64)
    z, _mu, sd = _standardise(seen)
    _m, so, co, _ev = orc.pca_rsvd(z, K, omega=_omega(m, n, seed + 1))
    return seen, sd, so, co


def _proj_err(c1, c2):
    c1, c2 = np.asarray(c1, dtype=np.float64), np.asarray(c2, dtype=np.float64)
    return float(np.linalg.norm(c1.T @ c1 - c2.T @ c2))


def _check(kind, case, m, n, seed, out, *, const_col=True):
    """assertions 1 and 2 of a dense case: scales against numpy, S and the components (up to sign) against the oracle"""
    means, s, comps, scales = (_np(t) for t in out)
    _seen, sd, so, co = _oracle(m, n, seed, kind)
    out_dt = np.float64 if kind == "float64" else np.float32
    assert means.shape == (1, n) and scales.shape == (1, n) and s.shape == (K, 1) and comps.shape == (K, n), case
    assert scales.dtype == out_dt and means.dtype == out_dt, case
    if const_col:
        assert scales[0, n // 2] == 1.0, case                               # the constant column: exactly 1
    err = float(np.max(np.abs(scales.astype(np.float64) - sd) / sd))
    ds = float(np.max(np.abs(s.astype(np.float64) - so) / so))
    dp = _proj_err(comps, co)
    print(f"standardize {case} {kind} {m}x{n}: scales max rel err {err:.3e}  max |dS|/S {ds:.3e}  projector {dp:.3e}")
    assert err <= 4.0 * SCALES_ERR_MEASURED[kind], (case, err)
    assert np.allclose(s, so, rtol=S_RTOL[kind]), (case, ds)
    assert dp < PROJ_TOL[kind], (case, dp)


def _device(torch, x64, dtype, layout):
    t = torch.tensor(np.asarray(x64), dtype=getattr(torch, dtype), device="cuda")
    return t.t().contiguous().t() if layout == "col" else t    # same values, column-major memory


# ---- 1, 2: scales, S and components against the oracle ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("layout", ["row", "col"])
@pytest.mark.parametrize("shape", [(1031, 77), (61, 1500)])
def test_dense_tall_and_fat_in_both_layouts(ctx, torch, shape, layout, dtype):
    m, n = shape
    seed = 100 + m
    x = _device(torch, _data(m, n, seed), dtype, layout)
    out = ctx.pca(x, K, omega=_omega(m, n, seed + 1), standardize=True)
    assert all(t.is_cuda and t.dtype == x.dtype for t in out)
    _check(dtype, f"{'tall' if m >= n else 'fat'}/{layout}", m, n, seed, out)
    # the means are those of the plain call, bit for bit (the same product, before anything is scaled)
    assert torch.equal(out[0], ctx.pca(x, K, omega=_omega(m, n, seed + 1))[0])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_row_major_view_with_a_leading_dimension_beyond_n(ctx, torch, dtype):
    """76 of the 96 columns of a wider buffer: read in place (ld = 96 > n), nothing behind column 75 may be counted"""
    m, n, seed = 1031, 76, 7
    big = torch.full((m, 96), 1e6, dtype=getattr(torch, dtype), device="cuda")
    big[:, :n] = torch.tensor(_data(m, n, seed), dtype=big.dtype, device="cuda")
    x = big[:, :n]
    assert x.stride() == (96, 1)
    _check(dtype, "ld>n", m, n, seed, ctx.pca(x, K, omega=_omega(m, n, seed + 1), standardize=True))


def test_host_pointers_take_the_scales_back_to_the_host(ctx):
    m, n, seed = 1031, 77, 100 + 1031
    x = np.array(_data(m, n, seed))
    out = ctx.pca(x, K, omega=_omega(m, n, seed + 1), standardize=True)
    assert all(isinstance(t, np.ndarray) for t in out)
    _check("float64", "host", m, n, seed, out)


@pytest.mark.parametrize("shape,in_place", [((1024, 64), True), ((1031, 77), False)])
def test_bf16_input_in_place_and_widened(ctx, torch, shape, in_place):
    """1024 x 64 is read in place at 2 bytes (every product of the call on the bf16-input kernel, as without the flag: the
    variance pass is not a product and widens nothing); 1031 x 77 is outside that kernel's domain and runs widened"""
    m, n = shape
    seed = 300 + m
    x = torch.tensor(np.asarray(_data(m, n, seed)), dtype=torch.float32).to(torch.bfloat16).cuda()
    out = ctx.pca(x, K, omega=_omega(m, n, seed + 1), standardize=True)
    nprod = ctx.timings()["n_bf16_products"]
    assert all(t.is_cuda and t.dtype == torch.float32 for t in out)
    ctx.pca(x, K, omega=_omega(m, n, seed + 1))
    assert nprod == ctx.timings()["n_bf16_products"]                         # unchanged by the flag
    assert (nprod == 1 + 2 + 2 * 20) if in_place else (nprod == 0)          # means, sketch + projection, 20 iterations
    _check("bf16", "in place" if in_place else "widened", m, n, seed, out)


@functools.lru_cache(maxsize=None)
def _sparse_case(dtype_name):
    """2000 x 150 at density 0.05: latent structure on a random pattern, column scales 1e-3 .. 1e3, column 10 all zero,
    column 20 with a single stored value; (scipy CSR, its dense f64 form)"""
    import scipy.sparse as sp
    m, n = 2000, 150
    rng = np.random.default_rng(2150)
    mask = rng.random((m, n)) < 0.05
    mask[:, 10] = False
    mask[:, 20] = False
    mask[777, 20] = True
    w = rng.standard_normal((8, n)) * (np.arange(8, 0, -1)[:, None] / 8)
    v = (rng.standard_normal((m, 8)) @ w + 0.3 * rng.standard_normal((m, n))) * 10.0 ** rng.uniform(-3, 3, n)
    a = sp.csr_matrix(np.where(mask, v, 0.0).astype(dtype_name))
    a.sort_indices()
    return a, a.toarray().astype(np.float64)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_csr_input_counts_the_implicit_zeros(ctx, dtype):
    a, dense = _sparse_case(dtype)
    m, n = dense.shape
    z, _mu, sd = _standardise(dense)
    omega = _omega(m, n, 5)
    _m, so, co, _ev = orc.pca_rsvd(z, K, omega=omega)
    means, s, comps, scales = ctx.pca(a, K, omega=omega, standardize=True)
    assert scales.dtype == np.dtype(dtype) and scales.shape == (1, n)
    assert scales[0, 10] == 1.0                                              # the all-zero column is a constant column
    err = float(np.max(np.abs(scales.astype(np.float64) - sd) / sd))
    dp = _proj_err(comps, co)
    print(f"standardize csr {dtype}: scales max rel err {err:.3e}  max |dS|/S {float(np.max(np.abs(s - so) / so)):.3e}  projector {dp:.3e}")
    assert err <= 4.0 * SCALES_ERR_MEASURED[dtype], err
    assert np.allclose(s, so, rtol=S_RTOL[dtype]) and dp < PROJ_TOL[dtype]
    # duplicate entries add, in the variance pass as in every product: one entry given as two halves changes nothing
    r = int(np.flatnonzero(np.diff(a.indptr) > 0)[0])
    p0 = int(a.indptr[r])
    data = np.insert(a.data, p0 + 1, a.data[p0] / 2)
    data[p0] = a.data[p0] / 2
    idx = np.insert(a.indices, p0 + 1, a.indices[p0])
    ptr = a.indptr.copy()
    ptr[r + 1:] += 1
    dup = ctx.pca((data, idx, ptr, (m, n)), K, omega=omega, standardize=True)
    assert np.allclose(dup[3], scales, rtol=4 * np.finfo(dtype).eps, atol=0) and np.allclose(dup[1], s, rtol=S_RTOL[dtype])


def test_sample_sharded_on_a_one_rank_communicator(torch, monkeypatch):
    """corrla_pca_sharded_dev_* with every all-reduce issued on a one-rank communicator: equal to the unsharded call, and
    the all-reduce of the n_dim sums of squares is counted (one more collective of 8 n bytes than without the flag)"""
    import corrla_rs_amd as cr
    c = cr.Context(0)
    try:
        c.comm_init(cr.Context.unique_id(), 0, 1)
        monkeypatch.setenv("CORRLA_FORCE_ALLREDUCE", "1")
        m, n, seed = 1031, 77, 100 + 1031
        for dtype in ("float32", "float64"):
            x = _device(torch, _data(m, n, seed), dtype, "row")
            om = _omega(m, n, seed + 1)
            for center in ("fused", "copy"):
                # (a context enqueues more thin-Q passes, for good, once a call has asked for them: let that happen before
                # the collectives of two calls are compared)
                c.pca_sharded(x, K, omega=om, center=center, standardize=True)
                c.pca_sharded(x, K, omega=om, center=center)
                sh = c.pca_sharded(x, K, omega=om, center=center, standardize=True)
                t_std = c.timings()
                c.pca_sharded(x, K, omega=om, center=center)
                t_plain = c.timings()
                assert t_std["n_collectives"] == t_plain["n_collectives"] + 1
                assert t_std["collective_bytes"] == t_plain["collective_bytes"] + 8.0 * n
                un = c.pca(x, K, omega=om, center=center, standardize=True)
                assert np.allclose(_np(sh[0]), _np(un[0]), rtol=S_RTOL[dtype], atol=0)
                assert np.allclose(_np(sh[3]), _np(un[3]), rtol=4 * SCALES_ERR_MEASURED[dtype], atol=0)
                assert np.allclose(_np(sh[1]), _np(un[1]), rtol=S_RTOL[dtype])
                assert _proj_err(_np(sh[2]), _np(un[2])) < PROJ_TOL[dtype]
            _check(dtype, "sharded", m, n, seed, sh)
    finally:
        c.close()


# ---- 3: fused against copy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("layout", ["row", "col"])
@pytest.mark.parametrize("shape", [(1031, 77), (61, 1500)])
def test_fused_equals_the_centred_and_scaled_copy(ctx, torch, shape, layout, dtype):
    m, n = shape
    seed = 100 + m
    x = _device(torch, _data(m, n, seed), dtype, layout)
    om = _omega(m, n, seed + 1)
    mf, sf, cf, df = (_np(t) for t in ctx.pca(x, K, omega=om, center="fused", standardize=True))
    mc, sc, cc, dc = (_np(t) for t in ctx.pca(x, K, omega=om, center="copy", standardize=True))
    assert np.array_equal(mf, mc) and np.array_equal(df, dc)
    print(f"fused vs copy {m}x{n} {layout} {dtype}: max |dS|/S {float(np.max(np.abs(sf - sc) / sc)):.3e}  projector {_proj_err(cf, cc):.3e}")
    assert np.allclose(sf, sc, rtol=FUSED_COPY_S_RTOL[dtype])
    assert _proj_err(cf, cc) < FUSED_COPY_PROJ_TOL[dtype]


# ---- 4: invariants that do not depend on the oracle -----------------------------------------------------------------------
def test_full_rank_call_has_the_trace_of_the_correlation_matrix(ctx, torch):
    """rank = n_dim: sum s^2 / (m - 1) is the trace of the correlation matrix = the number of non-constant columns"""
    m, n, seed = 1031, 77, 100 + 1031
    x = _device(torch, _data(m, n, seed), "float64", "row")
    _means, s, _comps, scales = ctx.pca(x, n, seed=3, standardize=True)
    tr = float((s.double() ** 2).sum() / (m - 1.0))
    print(f"trace of the correlation matrix: {tr!r} (non-constant columns: {n - 1})")
    assert int((scales == 1.0).sum()) == 1
    assert abs(tr - (n - 1)) <= 1e-10


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_rescaling_one_column_leaves_s_unchanged(ctx, torch, dtype):
    m, n, seed = 1031, 77, 100 + 1031
    x64 = np.array(_data(m, n, seed))
    y64 = x64.copy()
    y64[:, 2] *= 1000.0          # the column with the largest spread (1e3): unstandardised, it then dominates everything
    x, y = _device(torch, x64, dtype, "row"), _device(torch, y64, dtype, "row")
    om = _omega(m, n, seed + 1)
    sx, sy = _np(ctx.pca(x, K, omega=om, standardize=True)[1]), _np(ctx.pca(y, K, omega=om, standardize=True)[1])
    print(f"column x 1000, standardised, {dtype}: max |dS|/S {float(np.max(np.abs(sx - sy) / sx)):.3e}")
    assert np.allclose(sx, sy, rtol=S_RTOL[dtype])
    # ... and the same rescaling does move S without the flag: the case can fail
    px, py = _np(ctx.pca(x, K, omega=om)[1]), _np(ctx.pca(y, K, omega=om)[1])
    assert not np.allclose(px, py, rtol=S_RTOL[dtype])


# ---- 5: reproducibility ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tall", "fat", "bf16", "csr"])
def test_same_seed_twice_is_bitwise_equal(ctx, torch, case):
    if case == "csr":
        x = _sparse_case("float32")[0]
    elif case == "bf16":
        x = torch.tensor(np.asarray(_data(1024, 64, 1324)), dtype=torch.float32).to(torch.bfloat16).cuda()
    else:
        m, n = (1031, 77) if case == "tall" else (61, 1500)
        x = _device(torch, _data(m, n, 100 + m), "float32", "row")
    a = ctx.pca(x, K, seed=11, standardize=True)
    b = ctx.pca(x, K, seed=11, standardize=True)
    for ta, tb in zip(a, b):
        assert np.array_equal(_np(ta), _np(tb))


# ---- 6: ABI --------------------------------------------------------------------------------------------------------------
def _raw_pca_f64(ctx, x, opts, scales=None):
    from corrla_rs_amd import _lib as L
    m, n = x.shape
    means, s, comps = np.empty((1, n)), np.empty((K, 1)), np.empty((K, n), order="F")
    # (cast: the options block may be the 32-byte layout, which the ctypes prototype does not name)
    po = None if opts is None else C.cast(C.pointer(opts), C.POINTER(L.Opts))
    rc = L.load().corrla_pca_f64(ctx._h, x.ctypes.data, m, n, n, 1, K, 3, 6, po, means.ctypes.data, s.ctypes.data,
                                 comps.ctypes.data, K)
    return rc, means, s, comps


def test_the_first_layout_of_corrla_opts_is_still_accepted(ctx):
    """struct_size = 32 (the layout through omega_ld) with no new flag is accepted and gives, bit for bit, what today's
    layout gives with the same seed.  (NULL opts -- no seed at all, a fresh sketch per call -- succeeds alongside; a seed
    is what makes two calls comparable, so the comparison is between the two layouts.)  Any other size stays EINVAL."""
    from corrla_rs_amd import _lib as L
    x = np.ascontiguousarray(_data(1031, 77, 100 + 1031))

    class OptsV1(C.Structure):
        _fields_ = L.Opts._fields_[:5]
    assert C.sizeof(OptsV1) == 32
    old = OptsV1(struct_size=32, flags=L.SEED_EXPLICIT, seed=9)
    new = L.Opts(struct_size=C.sizeof(L.Opts), flags=L.SEED_EXPLICIT, seed=9)
    rc_old, *r_old = _raw_pca_f64(ctx, x, old)
    rc_new, *r_new = _raw_pca_f64(ctx, x, new)
    assert rc_old == L.OK and rc_new == L.OK
    assert all(np.array_equal(a, b) for a, b in zip(r_old, r_new))
    assert _raw_pca_f64(ctx, x, None)[0] == L.OK
    for bad in (0, 24, 36, 48):
        new.struct_size = bad
        assert _raw_pca_f64(ctx, x, new)[0] == L.EINVAL
    # the old layout has no scales_out to write to: with the flag the call still succeeds, standardised
    old.flags |= L.PCA_STANDARDIZE
    rc, _m, s_std, _c = _raw_pca_f64(ctx, x, old)
    assert rc == L.OK and not np.allclose(s_std, r_old[1], rtol=1e-3)


def test_the_flag_is_refused_outside_pca_and_needs_no_scales_out(ctx, torch):
    from corrla_rs_amd import _lib as L
    lib = L.load()
    o = L.Opts(struct_size=C.sizeof(L.Opts), flags=L.PCA_STANDARDIZE | L.SEED_EXPLICIT, seed=4)
    a = torch.randn((256, 32), dtype=torch.float32, device="cuda")
    u, s, vt = torch.empty((4, 256), device="cuda"), torch.empty(4, device="cuda"), torch.empty((32, 4), device="cuda")
    torch.cuda.synchronize()
    rc = lib.corrla_rsvd_dev_f32(ctx._h, a.data_ptr(), 256, 32, 32, 1, 4, 2, 4, C.byref(o), u.data_ptr(), 256, s.data_ptr(),
                                 vt.data_ptr(), 4)
    assert rc == L.EINVAL and b"corrla_pca_" in lib.corrla_last_error()
    # scales_out == NULL with the flag: the call succeeds, and S is that of the call that asks for the scales
    x = np.ascontiguousarray(_data(1031, 77, 100 + 1031))
    o = L.Opts(struct_size=C.sizeof(L.Opts), flags=L.PCA_STANDARDIZE | L.SEED_EXPLICIT, seed=9)
    rc, _m, s0, _c = _raw_pca_f64(ctx, x, o)
    assert rc == L.OK
    scales = np.empty((1, 77))
    o.scales_out = scales.ctypes.data
    rc, _m, s1, _c = _raw_pca_f64(ctx, x, o)
    assert rc == L.OK and np.array_equal(s0, s1)
    assert np.allclose(scales, _standardise(x)[2], rtol=4 * SCALES_ERR_MEASURED["float64"], atol=0)


# ---- 7: unchanged behaviour ------------------------------------------------------------------------------------------------
def test_standardize_false_is_the_plain_call(ctx, torch):
    x = _device(torch, _data(1031, 77, 100 + 1031), "float32", "row")
    a = ctx.pca(x, K, seed=11)
    b = ctx.pca(x, K, seed=11, standardize=False)
    assert len(a) == len(b) == 3 and all(torch.equal(p, q) for p, q in zip(a, b))
