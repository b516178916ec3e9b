"""CSR sparse input on the GPU: the SpMM kernels against dense f64 products, rsvd / PCA on sparse matrices against the
CPU oracle on the densified matrix (same Omega) and against the dense path of the same build, bitwise repeatability,
rejection of malformed CSR arrays, and a matrix too large to exist densely.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

from oracle import rsvd_oracle as orc
from tests.helpers import check_factorization, orth_err

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


@pytest.fixture(scope="module")
def sp():
    import scipy.sparse as sp
    return sp


def _uniform_sparse(sp, m, n, density, seed, dtype=np.float64, values="normal"):
    """seeded uniform-random pattern; Gaussian (or small-integer) values"""
    rng = np.random.default_rng(seed)
    nnz = max(1, int(round(density * m * n)))
    flat = rng.choice(m * n, size=nnz, replace=False)
    r, c = np.divmod(flat, n)
    v = rng.standard_normal(nnz) if values == "normal" else rng.integers(-4, 5, size=nnz).astype(np.float64)
    a = sp.csr_matrix((v.astype(dtype), (r, c)), shape=(m, n))
    a.sort_indices()
    return a


def _tuple(a):
    return (a.data, a.indices, a.indptr, a.shape)


def _spmm_check(ctx, torch, a_form, dense64, l, dt, tol, seed, beta=1.0, transes=(False, True)):
    m, n = dense64.shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    ad = torch.tensor(dense64, device="cuda")
    for trans in transes:
        x = torch.randn(((m if trans else n), l), dtype=dt, device="cuda", generator=g)
        res = ctx.spmm(a_form, x, trans=trans, beta=beta)
        assert tuple(res.shape) == ((n if trans else m), l) and res.dtype == dt
        ref = beta * ((ad.t() if trans else ad) @ x.double())
        scale = ref.abs().max().item() + 1e-30
        err = (res.double() - ref).abs().max().item() / scale
        print(f"spmm {m}x{n} l={l} trans={trans} {dt}: rel max err {err:.3e}")
        assert err < tol, (trans, err)


# ---- SpMM against a dense f64 product -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("density", [0.005, 0.05, 0.6])
@pytest.mark.parametrize("l", [1, 17, 138, 300])
@pytest.mark.parametrize("shape", [(64, 64), (333, 130), (130, 333), (5000, 36), (2048, 1024)])
def test_spmm_both_ops(ctx, torch, sp, dtype, density, l, shape):
    m, n = shape
    dt = getattr(torch, dtype)
    a = _uniform_sparse(sp, m, n, density, m * 1000 + n + l, np.float32 if dtype == "float32" else np.float64)
    tol = 2e-5 if dtype == "float32" else 1e-12     # the bounds of test_matmul_both_ops
    dense = a.toarray().astype(np.float64)
    _spmm_check(ctx, torch, a, dense, l, dt, tol, m + n + l)
    _spmm_check(ctx, torch, a, dense, l, dt, tol, m + n + l + 1, beta=0.25, transes=(False,))
    _spmm_check(ctx, torch, a, dense, l, dt, tol, m + n + l + 2, beta=-1.5, transes=(True,))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_spmm_row_length_distributions(ctx, torch, sp, dtype):
    """Empty rows and columns; one row holding half of all nonzeros (split over workgroups); unsorted column indices;
    duplicate entries, which add (scipy semantics)."""
    dt = getattr(torch, dtype)
    npdt = np.float32 if dtype == "float32" else np.float64
    tol = 2e-5 if dtype == "float32" else 1e-12
    rng = np.random.default_rng(11)
    # empty rows and columns
    a = _uniform_sparse(sp, 700, 300, 0.03, 5, npdt).tolil()
    a[::7, :] = 0
    a[:, ::5] = 0
    a = a.tocsr()
    a.eliminate_zeros()
    assert (np.diff(a.indptr) == 0).sum() >= 100
    for l in (1, 17, 138):
        _spmm_check(ctx, torch, a, a.toarray().astype(np.float64), l, dt, tol, 100 + l)
    # one row with half of all nonzeros: 9000 columns, row 17 is dense, the other rows share as many entries again
    m, n = 600, 9000
    base = _uniform_sparse(sp, m, n, n / float(m * n), 6, npdt).tolil()
    base[17, :] = rng.standard_normal(n).astype(npdt)
    h = base.tocsr()
    h.sort_indices()
    lens = np.diff(h.indptr)
    assert lens[17] == n and lens[17] >= 0.45 * h.nnz
    for l in (1, 17, 138, 300):
        _spmm_check(ctx, torch, h, h.toarray().astype(np.float64), l, dt, tol, 200 + l)
    # the transpose of that matrix has one dense COLUMN and is what trans=True gathers; also a fat orientation
    _spmm_check(ctx, torch, h.T.tocsr(), h.T.toarray().astype(np.float64), 17, dt, tol, 300)
    # unsorted indices within every row (legal), explicit tuple so that nothing re-sorts them
    u = _uniform_sparse(sp, 333, 130, 0.2, 7, npdt)
    data, idx = u.data.copy(), u.indices.copy()
    for r in range(333):
        s, e = u.indptr[r], u.indptr[r + 1]
        perm = rng.permutation(e - s)
        data[s:e], idx[s:e] = data[s:e][perm], idx[s:e][perm]
    assert any(np.any(np.diff(idx[u.indptr[r]:u.indptr[r + 1]]) < 0) for r in range(333))
    _spmm_check(ctx, torch, (data, idx, u.indptr, u.shape), u.toarray().astype(np.float64), 17, dt, tol, 400)
    # duplicates add: every entry stored twice with halves that differ, against scipy's summed matrix
    rows = np.repeat(np.arange(333), np.diff(u.indptr))
    d2 = np.concatenate([0.25 * u.data, 0.75 * u.data]).astype(npdt)
    r2, c2 = np.concatenate([rows, rows]), np.concatenate([u.indices, u.indices])
    order = np.argsort(r2, kind="stable")
    d2, r2, c2 = d2[order], r2[order], c2[order]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=333))])
    summed = sp.coo_matrix((d2.astype(np.float64), (r2, c2)), shape=u.shape).tocsr()   # scipy sums duplicates
    assert summed.nnz == u.nnz and len(d2) == 2 * u.nnz
    _spmm_check(ctx, torch, (d2, c2, ptr, u.shape), summed.toarray(), 17, dt, tol, 500)


def test_spmm_exact_integers_and_padding(ctx, torch, sp):
    """Small-integer values and an asymmetric integer X: every product and sum is exact, so a wrong tile transpose,
    index or row split shows as an exact mismatch.  Sketch widths around the tile and padding boundaries.  (What the
    product leaves OUTSIDE its destination is test_spmm_writes_nothing_outside_the_destination's subject.)"""
    for dt, npdt in ((torch.float32, np.float32), (torch.float64, np.float64)):
        for (m, n) in ((130, 333), (333, 130), (70, 6000)):
            a = _uniform_sparse(sp, m, n, 0.08, m + n, npdt, values="int")
            if n == 6000:
                lil = a.tolil()
                lil[3, :] = np.arange(n) % 7 - 3     # a long row (split into chunks)
                a = lil.tocsr()
            ad = torch.tensor(a.toarray(), device="cuda", dtype=dt)
            for l in (1, 15, 16, 63, 64, 65, 138):
                for trans in (False, True):
                    xin = m if trans else n
                    x = ((torch.arange(xin * l, device="cuda").reshape(xin, l) * 7 + 3) % 11 - 5).to(dt)
                    res = ctx.spmm(a, x, trans=trans)
                    ref = (ad.t() if trans else ad) @ x
                    assert torch.equal(res, ref), (dt, m, n, l, trans)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_spmm_writes_nothing_outside_the_destination(ctx, torch, sp, dtype):
    """Destination padding after the call.  corrla_spmm_csr_dev_* makes the caller's buffer the destination of the SpMM
    kernels themselves (an `external` Skinny: ld = ldres, l columns).  The buffer here has padding rows below every column
    (ldres > rows), extra columns behind the last one and guard elements in front, all zero (and, in a second run, a
    sentinel) before the call: afterwards rows [0, rows) x columns [0, l) hold the product and every other element is
    what it was.  Widths around the 64-column tile, row counts off the 64-row tile, short and long (chunked) rows."""
    from corrla_rs_amd import _lib as L
    lib = L.load()
    dt = getattr(torch, dtype)
    npdt = np.float32 if dtype == "float32" else np.float64
    fn = getattr(lib, "corrla_spmm_csr_dev_" + ("f32" if dtype == "float32" else "f64"))
    mats = [_uniform_sparse(sp, 130, 333, 0.08, 1, npdt, values="int"), _uniform_sparse(sp, 1001, 203, 0.05, 2, npdt, values="int")]
    lil = _uniform_sparse(sp, 70, 6000, 0.01, 3, npdt, values="int").tolil()
    lil[3, :] = np.arange(6000) % 7 - 3          # a long row: the chunked kernels store it
    mats.append(lil.tocsr())
    for a in mats:
        m, n = a.shape
        vals = torch.from_numpy(a.data).cuda()
        ci = torch.from_numpy(a.indices.astype(np.int32)).cuda()
        rp = torch.from_numpy(a.indptr.astype(np.int64)).cuda()
        ad = torch.tensor(a.toarray(), device="cuda", dtype=dt)
        for trans in (0, 1):
            xin, xout = (m, n) if trans else (n, m)
            for l in (1, 17, 63, 64, 65, 138):
                x = ((torch.arange(xin * l, device="cuda").reshape(xin, l) * 7 + 3) % 11 - 5).to(dt)
                xc = x.t().contiguous()
                ref = (ad.t() if trans else ad) @ x
                for fill in (0.0, -77.0):
                    guard, ldres, extra = 128, xout + 37, 3
                    buf = torch.full((guard + (l + extra) * ldres + guard,), fill, dtype=dt, device="cuda")
                    torch.cuda.synchronize()
                    rc = fn(ctx._h, trans, vals.data_ptr(), ci.data_ptr(), rp.data_ptr(), m, n, a.nnz, xc.data_ptr(), xin, l, 1.0,
                            buf.data_ptr() + guard * buf.element_size(), ldres)
                    assert rc == L.OK, lib.corrla_last_error()
                    body = buf[guard: guard + (l + extra) * ldres].reshape(l + extra, ldres)   # row j = column j of res
                    assert torch.equal(body[:l, :xout].t(), ref), (a.shape, trans, l)
                    assert torch.all(body[:l, xout:] == fill), "padding rows were written"
                    assert torch.all(body[l:, :] == fill), "columns past l were written"
                    assert torch.all(buf[:guard] == fill) and torch.all(buf[-guard:] == fill)


# ---- rsvd parity against the oracle on the densified matrix ------------------------------------------------------
CASES = [((3000, 400), 0.05, 12, 2, 10), ((400, 3000), 0.02, 12, 4, 10), ((5000, 300), 0.01, 8, 8, 10)]


def _case_matrix(sp, shape, density, dtype):
    """seeded uniform pattern, Gaussian values, every 17th row and every 13th column empty"""
    m, n = shape
    a = _uniform_sparse(sp, m, n, density, m + 3 * n, dtype).tocoo()
    keep = (a.row % 17 != 0) & (a.col % 13 != 0)
    a = sp.csr_matrix((a.data[keep], (a.row[keep], a.col[keep])), shape=shape)
    a.sort_indices()
    return a


def _forms(torch, a):
    t = torch.sparse_csr_tensor(torch.from_numpy(a.indptr.astype(np.int64)), torch.from_numpy(a.indices.astype(np.int64)),
                                torch.from_numpy(a.data), size=a.shape)
    return {"scipy": a, "tuple": _tuple(a), "torch_cpu": t, "torch_cuda": t.to("cuda")}


def _to_np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _parity_sparse(ctx, a_form, dense, k, q, p, om, dtype, qr=None):
    """the asserts and tolerances of _parity in tests/test_gpu_parity.py, tight class"""
    f64 = dtype == np.float64
    s_rtol, rec_rtol = (1e-10, 1e-8) if f64 else (2e-5, 1e-3)
    m, n = dense.shape
    u, s, vt = (_to_np(x) for x in ctx.rsvd(a_form, k, q, p, omega=om, qr=qr))
    assert u.shape == (m, k) and s.shape == (k, 1) and vt.shape == (k, n)
    assert u.dtype == dtype
    uo, so, vto = orc.random_svd(dense, k, q, p, omega=om)
    check_factorization(dense, u, s, vt, k, 0)
    s1 = max(float(so[0, 0]), 1e-300)
    ds = np.max(np.abs(s.ravel().astype(np.float64) - so.ravel()))
    drel = abs(orc.relerr(dense, u, s, vt) - orc.relerr(dense, uo, so, vto))
    rec = (u.astype(np.float64) * s.ravel()) @ vt.astype(np.float64)
    reco = (uo.astype(np.float64) * so.ravel()) @ vto.astype(np.float64)
    drec = np.linalg.norm(rec - reco) / max(np.linalg.norm(reco), 1e-300)
    print(f"rsvd parity {m}x{n} {np.dtype(dtype).name}: dS/s1 {ds / s1:.3e} d relerr {drel:.3e} d rec {drec:.3e}")
    assert ds <= s_rtol * s1
    assert drel <= 1e-5
    assert drec <= rec_rtol
    nnz = int(np.sum(so.ravel() > 1e-5 * s1))
    eps = np.finfo(dtype).eps
    assert orth_err(u[:, :nnz]) <= 200 * eps * np.sqrt(m)
    assert orth_err(vt[:nnz, :].T) <= 200 * eps * np.sqrt(n)
    return u, s, vt


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", CASES)
def test_rsvd_sparse_matches_oracle(ctx, torch, sp, case, dtype):
    shape, density, k, q, p = case
    a = _case_matrix(sp, shape, density, dtype)
    assert (np.diff(a.indptr) == 0).sum() >= shape[0] // 17
    dense = a.toarray()
    rng = np.random.default_rng(sum(shape))
    om = rng.standard_normal((min(shape), k + p)).astype(dtype)
    outs = {name: _parity_sparse(ctx, f, dense, k, q, p, om, dtype) for name, f in _forms(torch, a).items()}
    # the host forms normalise to the same arrays and take the same entry: identical bits
    for name in ("tuple", "torch_cpu"):
        for x, y in zip(outs["scipy"], outs[name]):
            assert np.array_equal(x, y), name


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rsvd_sparse_householder(ctx, torch, sp, dtype):
    shape, density, k, q, p = CASES[0]
    a = _case_matrix(sp, shape, density, dtype)
    rng = np.random.default_rng(5)
    om = rng.standard_normal((min(shape), k + p)).astype(dtype)
    _parity_sparse(ctx, a, a.toarray(), k, q, p, om, dtype, qr="householder")


# ---- sparse path against the dense path of the same build -------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case", CASES)
def test_rsvd_sparse_equals_dense_path(ctx, sp, case, dtype):
    """same matrix, same Omega; the two paths differ only in product rounding -- the figures
    test_pca_fused_centring_equals_centred_copy allows between two such paths"""
    shape, density, k, q, p = case
    a = _case_matrix(sp, shape, density, dtype)
    rng = np.random.default_rng(sum(shape) + 1)
    om = rng.standard_normal((min(shape), k + p)).astype(dtype)
    us, ss, vs = ctx.rsvd(a, k, q, p, omega=om)
    ud, sd, vd = ctx.rsvd(a.toarray(), k, q, p, omega=om)
    f64 = dtype == np.float64
    pdiff = np.linalg.norm(vs.T.astype(np.float64) @ vs - vd.T.astype(np.float64) @ vd)
    print(f"sparse vs dense {shape} {np.dtype(dtype).name}: max rel dS {np.max(np.abs(ss - sd) / sd):.3e} projector {pdiff:.3e}")
    assert np.allclose(ss, sd, rtol=1e-10 if f64 else 2e-4, atol=0)
    assert pdiff < (1e-8 if f64 else 5e-3)


# ---- repeatability -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rsvd_sparse_bitwise_repeatable(ctx, sp, dtype):
    """Two calls with the same seed are bit-identical (no floating-point atomics, fixed summation order).  Permuting
    the entries WITHIN each CSR row changes the order in which a row's products are added, so that comparison holds
    to the tight-class tolerance of the parity tests, not bitwise."""
    shape, density, k, q, p = CASES[0]
    a = _case_matrix(sp, shape, density, dtype)
    r1 = ctx.rsvd(a, k, q, p, seed=1234)
    r2 = ctx.rsvd(a, k, q, p, seed=1234)
    for x, y in zip(r1, r2):
        assert np.array_equal(x, y)
    # a long row takes the chunked kernels: same requirement
    lil = _uniform_sparse(sp, 900, 5000, 0.002, 3, dtype).tolil()
    lil[5, :] = np.random.default_rng(1).standard_normal(5000).astype(dtype)
    b = lil.tocsr()
    r3 = ctx.rsvd(b, 6, 2, 6, seed=77)
    r4 = ctx.rsvd(b, 6, 2, 6, seed=77)
    for x, y in zip(r3, r4):
        assert np.array_equal(x, y)
    rng = np.random.default_rng(2)
    data, idx = a.data.copy(), a.indices.copy()
    for r in range(shape[0]):
        s, e = a.indptr[r], a.indptr[r + 1]
        perm = rng.permutation(e - s)
        data[s:e], idx[s:e] = data[s:e][perm], idx[s:e][perm]
    u, s, vt = ctx.rsvd((data, idx, a.indptr, a.shape), k, q, p, seed=1234)
    f64 = dtype == np.float64
    s1 = float(r1[1][0, 0])
    assert np.max(np.abs(s - r1[1])) <= (1e-10 if f64 else 2e-5) * s1
    rec = (u.astype(np.float64) * s.ravel()) @ vt.astype(np.float64)
    rec1 = (r1[0].astype(np.float64) * r1[1].ravel()) @ r1[2].astype(np.float64)
    assert np.linalg.norm(rec - rec1) <= (1e-8 if f64 else 1e-3) * np.linalg.norm(rec1)


# ---- a matrix that cannot exist densely ----------------------------------------------------------------------------
@pytest.mark.timeout(600)      # a time limit of its own: the one test that sorts 4e7 keys and holds ~3 GB on the device
def test_rsvd_matrix_too_large_to_densify(ctx, torch):
    """4e6 x 1e5 in f32 is 1.6 TB dense; as CSR it holds 4e7 nonzeros (320 MB).  Eight disjoint-support blocks
    sigma_i u_i v_i^T, each 20000 x 250 with random +-1 entries scaled to unit vectors, sigma = 8 .. 1: the singular
    values are known exactly.  A densifying implementation cannot run this."""
    m, n, nb, br, bc = 4_000_000, 100_000, 8, 20000, 250
    rng = np.random.default_rng(42)
    sig = np.arange(8, 0, -1).astype(np.float64)
    rp = np.zeros(m + 1, dtype=np.int64)
    datas, idxs = [], []
    lens = np.zeros(m, dtype=np.int64)
    for i in range(nb):
        r0, c0 = 123_457 + i * 400_000, 1_111 + i * 12_000      # disjoint row and column supports
        u = rng.choice([-1.0, 1.0], size=br) / np.sqrt(br)
        v = rng.choice([-1.0, 1.0], size=bc) / np.sqrt(bc)
        datas.append((sig[i] * np.outer(u, v)).astype(np.float32).ravel())
        idxs.append(np.tile(np.arange(c0, c0 + bc, dtype=np.int32), br))
        lens[r0:r0 + br] = bc
    np.cumsum(lens, out=rp[1:])
    data, idx = np.concatenate(datas), np.concatenate(idxs)      # blocks are in increasing row order
    assert data.size == 40_000_000 and rp[-1] == data.size
    t = torch.sparse_csr_tensor(torch.from_numpy(rp).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(data).cuda(), size=(m, n))
    u, s, vt = ctx.rsvd(t, 8, 2, 10, seed=9)
    assert tuple(u.shape) == (m, 8) and tuple(s.shape) == (8, 1) and tuple(vt.shape) == (8, n)
    got = s.cpu().numpy().ravel().astype(np.float64)
    print("known-spectrum matrix, S - sigma:", got - sig)
    assert np.max(np.abs(got - sig)) <= 2e-5 * sig[0]


# ---- PCA -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(2000, 64), (50, 400)])
def test_pca_sparse_matches_oracle_and_dense_fused(ctx, torch, sp, shape, dtype):
    m, n = shape
    a = _uniform_sparse(sp, m, n, 0.10, m + n, dtype)
    dense = a.toarray()
    k = 4
    p = min(n, 10)
    nt = min(m, n)
    rng = np.random.default_rng(m)
    omega = rng.standard_normal((nt, min(k + p, nt))).astype(dtype)
    f64 = dtype == np.float64
    mo, so, co, _ = orc.pca_rsvd(dense.astype(np.float64), k, omega=omega.astype(np.float64))
    for name, form in _forms(torch, a).items():
        means, s, comps = (_to_np(x) for x in ctx.pca(form, k, omega=omega))
        assert means.shape == (1, n) and s.shape == (k, 1) and comps.shape == (k, n), name
        assert means.dtype == dtype
        assert np.allclose(means, mo, atol=1e-12 if f64 else 1e-5), name
        assert np.allclose(s, so, rtol=1e-9 if f64 else 1e-4), name
        assert np.linalg.norm(comps.T.astype(np.float64) @ comps - co.T @ co) < (1e-7 if f64 else 2e-3), name
    # against the dense fused-centring path of the same build
    md, sd, cd = ctx.pca(dense, k, omega=omega, center="fused")
    means, s, comps = ctx.pca(a, k, omega=omega)
    assert np.allclose(means, md, atol=1e-12 if f64 else 1e-5)
    assert np.allclose(s, sd, rtol=1e-9 if f64 else 1e-4)
    assert np.linalg.norm(comps.T.astype(np.float64) @ comps - cd.T.astype(np.float64) @ cd) < (1e-7 if f64 else 2e-3)
    ms2, s2, c2 = ctx.pca(a, k, omega=omega, center="fused")
    assert np.array_equal(s, s2) and np.array_equal(comps, c2) and np.array_equal(means, ms2)
    with pytest.raises(ValueError):
        ctx.pca(a, k, omega=omega, center="copy")


def test_pca_center_copy_is_rejected_by_the_library(ctx, sp):
    """CORRLA_PCA_CENTER_COPY on a CSR entry: CORRLA_EINVAL with a message (through the C ABI, below the Python check)"""
    from corrla_rs_amd import _lib as L
    lib = L.load()
    a = _uniform_sparse(sp, 60, 20, 0.2, 1)
    o = L.Opts()
    o.struct_size = C.sizeof(L.Opts)
    o.flags = L.PCA_CENTER_COPY
    v, ci, rp = a.data, a.indices.astype(np.int32), a.indptr.astype(np.int64)
    mu, s, comps = np.empty((1, 20)), np.empty((3, 1)), np.empty((3, 20), order="F")
    rc = lib.corrla_pca_csr_f64(ctx._h, v.ctypes.data, ci.ctypes.data, rp.ctypes.data, 60, 20, a.nnz, 3, 2, 5, C.byref(o),
                                mu.ctypes.data, s.ctypes.data, comps.ctypes.data, 3)
    assert rc == L.EINVAL and b"densify" in lib.corrla_last_error()


def test_rpca_and_pcarsvd_on_scipy_input(ctx, sp):
    import corrla_rs as hrl
    a = _uniform_sparse(sp, 2000, 64, 0.10, 21)
    a = sp.csr_matrix(a.multiply(np.arange(1, 65)[None, :]))      # separated variances
    dense = a.toarray()
    ev = np.sort(np.linalg.eigvalsh(np.cov(dense, rowvar=False)))[::-1][:3]
    sv, pc = hrl.rpca(a, 3, 1, 0, seed=7)
    assert sv.shape == (3, 1) and pc.shape == (3, 64)
    assert np.allclose((sv ** 2 / (2000 - 1.0)).ravel(), ev, rtol=1e-6)
    for form in (a, a.tocsc(), a.tocoo()):
        pca = hrl.PcaRsvd(form, 3, seed=7)
        assert pca.n_samples == 2000
        assert np.allclose(pca.means, dense.mean(axis=0, keepdims=True), atol=1e-12)
        assert np.allclose(pca.explained_var().ravel(), ev, rtol=1e-6)
        assert pca.apply_tr(dense).shape == (2000, 3)           # dense targets, as before
        assert pca.apply_inv_tr(pca.apply_tr(dense)).shape == (2000, 64)
    u, s, vt = hrl.rsvd(a, 3, 2, 5, seed=1)
    assert u.shape == (2000, 3) and s.shape == (3, 1) and vt.shape == (3, 64)
    u2, s2, vt2 = hrl.random_svd(a, 3, 2, 5, seed=1)
    assert np.array_equal(s, s2)


# ---- rejection -----------------------------------------------------------------------------------------------------
def test_malformed_csr_is_rejected_with_a_message(ctx, torch, sp):
    from corrla_rs_amd import _lib as L
    lib = L.load()
    a = _uniform_sparse(sp, 200, 50, 0.1, 13)
    good = ctx.rsvd(a, 4, 2, 4, seed=2)

    def call(data, idx, ptr, shape, k=4):
        return ctx.rsvd((data, idx, ptr, shape), k, 2, 4, seed=2)

    bad_ptr = a.indptr.copy()
    bad_ptr[10], bad_ptr[11] = bad_ptr[11] + 3, bad_ptr[10]       # non-monotone
    with pytest.raises(ValueError, match="row_ptr"):
        call(a.data, a.indices, bad_ptr, a.shape)
    short = a.indptr.copy()
    short[-1] -= 1                                                 # row_ptr[m] != nnz
    with pytest.raises(ValueError, match="row_ptr"):
        call(a.data, a.indices, short, a.shape)
    idx = a.indices.copy()
    idx[a.nnz // 2] = 50                                           # == n
    with pytest.raises(ValueError, match="column index"):
        call(a.data, idx, a.indptr, a.shape)
    idx = a.indices.copy()
    idx[3] = -1
    with pytest.raises(ValueError, match="column index"):
        call(a.data, idx, a.indptr, a.shape)
    with pytest.raises(ValueError, match="rank"):
        call(a.data, a.indices, a.indptr, a.shape, k=51)
    # device entry: a column index equal to n comes back as a status (the validation kernel reads only the arrays
    # themselves), and the next valid call on the same context succeeds
    idx = a.indices.astype(np.int64)
    idx[7] = 50
    t = torch.sparse_csr_tensor(torch.from_numpy(a.indptr.astype(np.int64)), torch.from_numpy(idx), torch.from_numpy(a.data),
                                size=a.shape, check_invariants=False).to("cuda")
    with pytest.raises(ValueError, match="column index"):
        ctx.rsvd(t, 4, 2, 4, seed=2)
    assert b"invalid CSR" in lib.corrla_last_error()
    # an int64 index that would wrap into range as int32 (2^32 + 1 -> 1) must be rejected too, on the device path as well
    idx = a.indices.astype(np.int64)
    idx[9] = 2 ** 32 + 1
    t = torch.sparse_csr_tensor(torch.from_numpy(a.indptr.astype(np.int64)), torch.from_numpy(idx), torch.from_numpy(a.data),
                                size=a.shape, check_invariants=False)
    for form in (t, t.to("cuda")):
        with pytest.raises(ValueError, match="column index"):
            ctx.rsvd(form, 4, 2, 4, seed=2)
    again = ctx.rsvd(a, 4, 2, 4, seed=2)
    for x, y in zip(good, again):
        assert np.array_equal(x, y)
