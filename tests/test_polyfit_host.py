"""Host-side behaviour of the polynomial response-surface surface (corrla_rs_amd/api.py, callers.py, _lib.py, capi_impl.hpp),
no GPU needed: the prototypes of the header are bound and in the rust shim, Context.polyfit_gram / poly_eval build the call
each argument asks for (seen by a stub that stands where the entry would be), every bad argument raises before the library is
touched, a backend without the kernels -- the host emulation backend -- ends the call with EINVAL after the argument checks,
and the host solve with its coefficient back-map reproduces the restated reference (tests/polyfit_reference.py) when it is fed
numpy's own Gram matrix, shifted data and a constant column included."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from corrla_rs_amd import _lib as L
from corrla_rs_amd import api
from corrla_rs_amd import callers
from tests.api_stub import make_stub
from tests import polyfit_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "corrla_rsvd.h")).read()
KNOWN = os.path.join(ROOT, "tests", "golden", "polyfit", "polyfit_known.npz")
STEMS = ("corrla_polyfit_gram_", "corrla_polyfit_gram_dev_", "corrla_poly_eval_", "corrla_poly_eval_dev_")


def test_prototypes_are_declared_bound_and_in_the_rust_shim():
    body = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    for suf, ct in (("f32", "float"), ("f64", "double")):
        want = {"corrla_polyfit_gram_": ["corrla_ctx* ctx", f"const {ct}* x", "int64_t m", "int64_t k", "int64_t ldx", f"const {ct}* y",
                                         "int64_t r", "int64_t ldy", "int degree", "int normalize", "double* G", "int64_t ldg",
                                         "double* means", "double* scales"],
                "corrla_poly_eval_": ["corrla_ctx* ctx", f"const {ct}* x", "int64_t m", "int64_t k", "int64_t ldx", "const double* coeffs",
                                      "int64_t ldc", "int64_t r", "int degree", f"{ct}* out", "int64_t ld_out", f"{ct}* jac",
                                      "int64_t ld_jac"]}
        for stem, params in want.items():
            for dev in ("", "dev_"):
                name = stem + dev + suf
                m = re.search(r"corrla_status %s\(([^)]*)\)" % name, body)
                assert m, name
                assert [" ".join(p.split()) for p in m.group(1).split(",")] == params, name
                res, args = L.SIGNATURES[name]
                assert res is C.c_int and len(args) == len(params)
                assert args[params.index("int degree")] is C.c_int
                assert re.search(r"fn %s\(" % name, rs), name
    assert set(s for s in L.SIGNATURES if "_poly" in s and "last" not in s) == {st + suf for st in STEMS for suf in ("f32", "f64")}
    assert "corrla_ctx_last_polyfit" in L.SIGNATURES and re.search(r"fn corrla_ctx_last_polyfit\(", rs)
    # the header cites the reference's functions and states the limits
    assert "stats_corr.rs:146-169" in HDR and "stats_corr.rs:213-249" in HDR and "stats_corr.rs:112-142" in HDR
    assert "1 <= k <= 128" in HDR and "0 <= r <= 64" in HDR and "degree 1 or 2" in HDR and "m >= 1" in HDR


@pytest.fixture
def stub():
    return make_stub(last={"corrla_ctx_last_polyfit": (2,)})


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gram_and_eval_build_their_calls(stub, dtype):
    c, rec, names = stub
    ct = C.c_float if dtype == np.float32 else C.c_double
    suf = "f32" if dtype == np.float32 else "f64"
    x = np.arange(21, dtype=dtype).reshape(7, 3)
    y = np.arange(14.0).reshape(7, 2)                       # float64: converted to the dtype of x
    assert c.last_polyfit_route() is None
    rec.peek = {5: (ct, 14)}
    g, means, scales = c.polyfit_gram(x, y)
    rec.peek = {}
    a = rec.calls[-1]
    # (ctx, x, m, k, ldx, y, r, ldy, degree, normalize, G, ldg, means, scales)
    assert len(a) == 14 and a[1] == x.ctypes.data and a[2:5] == (7, 3, 3) and a[6:10] == (2, 2, 2, 1)
    assert np.array_equal(rec.seen[5], y.astype(dtype).ravel())
    order = 3 + 6 + 1 + 2
    assert type(g) is np.ndarray and g.shape == (order, order) and g.dtype == np.float64 and a[10] == g.ctypes.data and a[11] == order
    assert means.shape == scales.shape == (1, 3) and means.dtype == scales.dtype == np.float64
    assert a[12] == means.ctypes.data and a[13] == scales.ctypes.data
    assert c.last_polyfit_route() == "inplace_checked"     # what the stub's library reported
    # no y: r = 0 and a NULL pointer; degree 1: [x, 1]; normalize=False: no means, no scales
    g, means, scales = c.polyfit_gram(x, None, 1, normalize=False)
    a = rec.calls[-1]
    assert a[5] is None and a[6:10] == (0, 0, 1, 0) and g.shape == (4, 4) and means is None and scales is None
    assert a[12] is None and a[13] is None
    c.polyfit_gram(x, np.arange(7.0))                       # a vector is one column
    assert rec.calls[-1][6:8] == (1, 1) and rec.calls[-1][11] == 11
    # a view with a padded row stride is passed as it lies; a column-major one is not
    wide = np.zeros((7, 4), dtype=dtype)
    c.polyfit_gram(wide[:, :3], y)
    assert rec.calls[-1][1] == wide.ctypes.data and rec.calls[-1][4] == 4
    c.polyfit_gram(np.asfortranarray(x), y)
    assert rec.calls[-1][4] == 3
    n0 = len(rec.calls)
    coeffs = np.arange(20.0).reshape(10, 2)
    rec.peek = {5: (C.c_double, 20)}
    v = c.poly_eval(x, coeffs.astype(np.float32))           # coefficients travel as float64 whatever x is
    rec.peek = {}
    a = rec.calls[-1]
    # (ctx, x, m, k, ldx, coeffs, ldc, r, degree, out, ld_out, jac, ld_jac)
    assert len(a) == 13 and a[1] == x.ctypes.data and a[2:5] == (7, 3, 3) and a[6:9] == (2, 2, 2) and a[11] is None
    assert type(v) is np.ndarray and v.shape == (7, 2) and v.dtype == dtype and a[9] == v.ctypes.data and a[10] == 2
    assert np.array_equal(rec.seen[5], coeffs.ravel())
    v, jac = c.poly_eval(x, coeffs, jac=True)
    a = rec.calls[-1]
    assert jac.shape == (2, 7, 3) and jac.dtype == dtype and a[11] == jac.ctypes.data and a[12] == 3
    v, jac = c.poly_eval(x, np.arange(4.0), 1, jac=True)    # one column: (m, k)
    assert v.shape == (7, 1) and jac.shape == (7, 3) and rec.calls[-1][6:9] == (1, 1, 1)
    assert names[:n0] == ["corrla_polyfit_gram_" + suf] * n0 and names[n0:] == ["corrla_poly_eval_" + suf] * 3


def test_every_bad_argument_raises_before_the_library_is_touched(stub):
    c, rec, _ = stub
    x, y = np.zeros((6, 3)), np.zeros((6, 1))
    with pytest.raises(ValueError, match="2-D"):
        c.polyfit_gram(np.zeros(5), y)
    with pytest.raises(ValueError, match="non-empty"):
        c.polyfit_gram(np.zeros((0, 3)), None)
    with pytest.raises(ValueError, match="non-empty"):
        c.poly_eval(np.zeros((4, 0)), np.zeros(1))
    with pytest.raises(ValueError, match="129 features"):
        c.polyfit_gram(np.zeros((4, 129)), None)
    with pytest.raises(ValueError, match="129 features"):
        c.poly_eval(np.zeros((4, 129)), np.zeros(130), 1)
    with pytest.raises(ValueError, match="y must have 6 rows"):
        c.polyfit_gram(x, np.zeros((5, 1)))
    with pytest.raises(ValueError, match="65 columns"):
        c.polyfit_gram(x, np.zeros((6, 65)))
    for bad in (0, 3, 2.0, True, None):
        with pytest.raises(ValueError, match="degree must be 1 or 2"):
            c.polyfit_gram(x, y, bad)
        with pytest.raises(ValueError, match="degree must be 1 or 2"):
            c.poly_eval(x, np.zeros(10), bad)
    with pytest.raises(ValueError, match="normalize must be True or False"):
        c.polyfit_gram(x, y, normalize=1)
    with pytest.raises(TypeError):
        c.polyfit_gram(x, y, 2, False)                      # normalize is keyword-only
    with pytest.raises(ValueError, match="jac must be True or False"):
        c.poly_eval(x, np.zeros(10), jac="yes")
    with pytest.raises(ValueError, match=r"p = 10 rows for 3 features at degree 2, got shape \(4, 1\)"):
        c.poly_eval(x, np.zeros(4))
    with pytest.raises(ValueError, match=r"p = 4 rows for 3 features at degree 1"):
        c.poly_eval(x, np.zeros((10, 2)), 1)
    with pytest.raises(ValueError, match="65 columns"):
        c.poly_eval(x, np.zeros((10, 65)))
    csr = (np.array([1.0]), np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int64), (1, 3))
    with pytest.raises(ValueError, match="dense"):
        c.polyfit_gram(csr, None)
    with pytest.raises(ValueError, match="dense"):
        c.poly_eval(csr, np.zeros(10))
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match=r"no bfloat16 entry"):
        c.polyfit_gram(torch.zeros((4, 3), dtype=torch.bfloat16), None)
    with pytest.raises(ValueError, match=r"no bfloat16 entry"):
        c.polyfit_gram(x, torch.zeros((6, 1), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match=r"no bfloat16 entry"):
        c.poly_eval(torch.zeros((4, 3), dtype=torch.bfloat16), np.zeros(10))
    with pytest.raises(ValueError, match=r"no bfloat16 entry"):
        c.poly_eval(x, torch.zeros(10, dtype=torch.bfloat16))
    assert not rec.calls


EMU_PROBE = r"""
#include "emu_backend.cpp"
using corrla::PolyEvalCall;
using corrla::PolyGramCall;
#define API extern "C" __attribute__((visibility("default")))
API int probe_gram(const double* x, long long m, long long k, long long ldx, const double* y, long long r, long long ldy, int degree,
                   int normalize, double* g, long long ldg, double* means, double* scales) {
  EmuDev dev;
  bool ran = false;
  int st = (int)corrla::guarded([&] {
    const PolyGramCall<double> c{x, m, k, ldx, y, r, ldy, degree, normalize, g, ldg, means, scales};
    corrla::polyfit_gram_entry<EmuDev, double>(dev, c, [&] { ran = true; });
  });
  return ran ? -1 : st;
}
API int probe_eval(const double* x, long long m, long long k, long long ldx, const double* coeffs, long long ldc, long long r, int degree,
                   double* out, long long ld_out, double* jac, long long ld_jac) {
  EmuDev dev;
  bool ran = false;
  int st = (int)corrla::guarded([&] {
    const PolyEvalCall<double> c{x, m, k, ldx, coeffs, ldc, r, degree, out, ld_out, jac, ld_jac};
    corrla::poly_eval_entry<EmuDev, double>(dev, c, [&] { ran = true; });
  });
  return ran ? -1 : st;
}
API const char* probe_error() { return corrla::last_error_slot().c_str(); }
"""


@pytest.fixture(scope="module")
def emu_probe(tmp_path_factory):
    """The emulation backend itself (tests/emu/emu_backend.cpp, unchanged) behind the argument checks of the new entries."""
    tmp = tmp_path_factory.mktemp("polyfit_probe")
    src = tmp / "probe.cpp"
    src.write_text(EMU_PROBE)
    so = tmp / "libpolyfit_probe.so"
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "emu"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.probe_error.restype = C.c_char_p
    return lib


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class _Case:
    def __init__(self, m=9, k=3, r=2):
        rng = np.random.default_rng(0)
        self.x, self.y = rng.standard_normal((m, k)), rng.standard_normal((m, r))
        self.p = k + k * (k + 1) // 2 + 1
        self.g = np.empty((self.p + r, self.p + r))
        self.means, self.scales = np.empty(k), np.empty(k)
        self.coeffs = rng.standard_normal((self.p, r))
        self.out, self.jac = np.empty((m, r)), np.empty((r, m, k))
        self.m, self.k, self.r = m, k, r


def _gram(lib, cs, **kw):
    a = dict(x=cs.x, m=cs.m, k=cs.k, ldx=cs.k, y=cs.y, r=cs.r, ldy=cs.r, degree=2, normalize=1, g=cs.g, ldg=cs.p + cs.r, means=cs.means,
             scales=cs.scales)
    a.update(kw)
    LL = C.c_longlong
    rc = lib.probe_gram(_p(a["x"]), LL(a["m"]), LL(a["k"]), LL(a["ldx"]), _p(a["y"]), LL(a["r"]), LL(a["ldy"]), C.c_int(a["degree"]),
                        C.c_int(a["normalize"]), _p(a["g"]), LL(a["ldg"]), _p(a["means"]), _p(a["scales"]))
    return rc, lib.probe_error()


def _eval(lib, cs, **kw):
    a = dict(x=cs.x, m=cs.m, k=cs.k, ldx=cs.k, coeffs=cs.coeffs, ldc=cs.r, r=cs.r, degree=2, out=cs.out, ld_out=cs.r, jac=cs.jac, ld_jac=cs.k)
    a.update(kw)
    LL = C.c_longlong
    rc = lib.probe_eval(_p(a["x"]), LL(a["m"]), LL(a["k"]), LL(a["ldx"]), _p(a["coeffs"]), LL(a["ldc"]), LL(a["r"]), C.c_int(a["degree"]),
                        _p(a["out"]), LL(a["ld_out"]), _p(a["jac"]), LL(a["ld_jac"]))
    return rc, lib.probe_error()


def test_the_emulation_backend_ends_the_calls_with_einval(emu_probe):
    cs = _Case()
    for kw in ({}, dict(normalize=0, means=None, scales=None), dict(r=0, y=None, ldy=0), dict(degree=1), dict(means=None)):
        rc, msg = _gram(emu_probe, cs, **kw)
        assert rc == L.EINVAL and b"no polynomial response-surface kernels" in msg, (kw, msg)
    for kw in ({}, dict(jac=None), dict(degree=1), dict(r=1)):
        rc, msg = _eval(emu_probe, cs, **kw)
        assert rc == L.EINVAL and b"no polynomial response-surface kernels" in msg, (kw, msg)


def test_argument_checks_of_the_entries(emu_probe):
    """EINVAL with a message that names the argument, on every backend, before the backend is asked for anything"""
    cs = _Case()
    for kw, word in ((dict(x=None), b"x is NULL"), (dict(g=None), b"G is NULL"), (dict(y=None), b"y is NULL"), (dict(m=0), b"m must be >= 1"),
                     (dict(k=0), b"k must be in [1, 128]"), (dict(k=129, ldx=129), b"k must be in [1, 128]"),
                     (dict(degree=0), b"degree must be 1 or 2"), (dict(degree=3), b"degree must be 1 or 2"),
                     (dict(r=-1), b"r must be in [0, 64]"), (dict(r=65, ldy=65), b"r must be in [0, 64]"),
                     (dict(normalize=2), b"normalize must be 0 or 1"), (dict(ldx=2), b"ldx < k"), (dict(ldy=1), b"ldy < r"),
                     (dict(ldg=cs.p + cs.r - 1), b"ldg < p + r"), (dict(g=cs.x), b"G overlaps x"), (dict(g=cs.y), b"G overlaps y"),
                     (dict(means=cs.x), b"means overlaps x"), (dict(scales=cs.means), b"means overlaps scales")):
        rc, msg = _gram(emu_probe, cs, **kw)
        assert rc == L.EINVAL and b"polyfit_gram: " in msg and word in msg, (kw, msg)
    # without normalisation the means and scales are not written: no overlap to speak of
    rc, msg = _gram(emu_probe, cs, normalize=0, means=cs.x, scales=cs.x)
    assert rc == L.EINVAL and b"no polynomial response-surface kernels" in msg
    for kw, word in ((dict(x=None), b"x is NULL"), (dict(coeffs=None), b"coeffs is NULL"), (dict(out=None), b"out is NULL"),
                     (dict(m=0), b"m must be >= 1"), (dict(k=0), b"k must be in [1, 128]"), (dict(k=129, ldx=129), b"k must be in [1, 128]"),
                     (dict(degree=0), b"degree must be 1 or 2"), (dict(r=0), b"r must be in [1, 64]"), (dict(r=65), b"r must be in [1, 64]"),
                     (dict(ldx=2), b"ldx < k"), (dict(ldc=1), b"ldc < r"), (dict(ld_out=1), b"ld_out < r"), (dict(ld_jac=2), b"ld_jac < k"),
                     (dict(out=cs.x), b"out overlaps x"), (dict(out=cs.coeffs), b"out overlaps coeffs"), (dict(jac=cs.x), b"jac overlaps x"),
                     (dict(jac=cs.out), b"out overlaps jac")):
        rc, msg = _eval(emu_probe, cs, **kw)
        assert rc == L.EINVAL and b"poly_eval: " in msg and word in msg, (kw, msg)


# ---- the host solve ------------------------------------------------------------------------------------------------------------
def numpy_gram(x, y, degree, normalize):
    """what the kernel computes, with numpy in f64: z = (x - mean) * (1 / sd) (population sd, 1 for a constant column)"""
    if normalize:
        mu = x.mean(axis=0)
        sd = x.std(axis=0)
        sd = np.where(sd > 1e-14 * np.maximum(np.abs(mu), 1.0), sd, 1.0)
        z = (x - mu) * (1.0 / sd)
    else:
        mu = sd = None
        z = x
    w = np.hstack([R.build_full_vandermonde(z, degree), y])
    return w.T @ w, mu, sd


def host_fit(x, y, degree, normalize):
    g, mu, sd = numpy_gram(x, y, degree, normalize)
    return callers.polyfit_solve(g, x.shape[1], degree, mu, sd)


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def test_sym_and_unsym_are_inverse_and_match_the_reference_form():
    rng = np.random.default_rng(1)
    for k, degree in ((1, 1), (1, 2), (3, 1), (3, 2), (6, 2)):
        p = k + 1 if degree == 1 else k + k * (k + 1) // 2 + 1
        c = rng.standard_normal((p, 2))
        cm = callers._poly_sym(c, k, degree)
        for j in range(2):
            assert np.array_equal(cm[j], R.poly_sym(c[:, j], k, degree)) and np.array_equal(cm[j], cm[j].T)
        assert np.allclose(callers._poly_unsym(cm, k, degree), c, rtol=0, atol=1e-15)
        x = rng.standard_normal((5, k))
        xt = np.hstack([x, np.ones((5, 1))])
        want = R.build_full_vandermonde(x, degree) @ c
        got = np.stack([((xt @ cm[j]) * xt).sum(axis=1) for j in range(2)], axis=1)
        assert rel(got, want) < 1e-14


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("degree", [1, 2])
def test_host_solve_reproduces_the_reference_fit(k, degree):
    rng = np.random.default_rng(k + degree)
    x = rng.random((400, k))
    y = np.stack([np.sin(x.sum(axis=1)), x[:, 0] * x[:, -1] + 0.1 * rng.standard_normal(400)], axis=1)
    ref = (R.quad_fit if degree == 2 else R.linear_fit)(x, y)
    for normalize in (False, True):
        assert rel(host_fit(x, y, degree, normalize), ref) < 1e-10, normalize
    # Data shifted to [10, 11].  The polynomials of a degree are the same space after a shift, so the fitted surface is the
    # one of the unshifted problem, whose reference fit is the yardstick (the reference's own SVD of the shifted V is not:
    # cond(V) grows by 1e4 and more).  The normalised route keeps the accuracy of the unshifted problem.
    xs = x + 10.0
    want = R.build_full_vandermonde(x, degree) @ ref
    assert rel(R.build_full_vandermonde(xs, degree) @ host_fit(xs, y, degree, True), want) < 1e-11


def test_host_solve_on_the_golden_points():
    g = np.load(KNOWN)
    tol = float(g["lin_tol"])
    for tag in ("lin1", "lin2"):
        x, y = g[tag + "_x"], g[tag + "_y"]
        for normalize in (False, True):
            c = host_fit(x, y, 1, normalize)
            assert np.max(np.abs(c[:x.shape[1]].T - g[tag + "_jac"])) <= tol and abs(c[-1, 0]) <= tol
        assert np.max(np.abs(R.jac_from_lin(x, y) - g[tag + "_jac"])) <= tol
    # test_quad_fit: six points, six columns, but V has rank 5 -- predictions, not coefficients
    x, y = g["quad_x"], g["quad_y"]
    v = R.build_vandermonde(x)
    assert np.linalg.matrix_rank(v) < v.shape[1]
    # The reference's 1 / (s + 1e-14) turns the null direction into coefficients of order 1e12, and the predictions V c then
    # carry the rounding of that cancellation, p eps max|c| max|V|: that is the reference's own error and the bound against
    # it.  The least-squares predictions themselves are pinned by numpy's minimum-norm solution.
    c_ref = R.quad_fit(x, y)
    assert np.max(np.abs(c_ref)) > 1e10
    noise = v.shape[1] * 2.0 ** -52 * np.max(np.abs(c_ref)) * np.max(np.abs(v))
    lstsq = v @ np.linalg.lstsq(v, y, rcond=None)[0]
    for normalize in (False, True):
        c = host_fit(x, y, 2, normalize)
        assert np.max(np.abs(c)) < 10.0
        assert rel(v @ c, lstsq) < 1e-13
        assert np.max(np.abs(v @ c - v @ c_ref)) <= noise


def test_a_constant_column_gets_scale_one_and_drops_out():
    rng = np.random.default_rng(5)
    x = rng.random((200, 4))
    x[:, 2] = 0.75
    y = (x[:, 0] - 2.0 * x[:, 3] + x[:, 1] * x[:, 3])[:, None]
    g, mu, sd = numpy_gram(x, y, 2, True)
    assert sd[2] == 1.0
    c = callers.polyfit_solve(g, 4, 2, mu, sd)
    v = R.build_vandermonde(x)
    assert rel(v @ c, y) < 1e-11                      # V is rank-deficient: the predictions are what is determined
