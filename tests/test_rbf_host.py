"""Host-side behaviour of the radial-basis-function surface (corrla_rs_amd/api.py, callers.py, _lib.py, capi_impl.hpp), no GPU
needed: the prototypes of the header are bound and in the rust shim, Context.rbf_matrix / rbf_apply build the call each
argument asks for (seen by a stub that stands where the entry would be), every bad argument raises before the library is
touched, a backend without the kernels -- the host emulation backend -- ends the call with EINVAL after the argument checks,
and RbfInterp without `device` on numpy input is bit for bit the numpy formulas it was."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from corrla_rs_amd import _lib as L
from corrla_rs_amd import api
from tests.api_stub import make_stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "corrla_rsvd.h")).read()
STEMS = ("corrla_rbf_matrix_", "corrla_rbf_matrix_dev_", "corrla_rbf_apply_", "corrla_rbf_apply_dev_")


def test_prototypes_are_declared_bound_and_in_the_rust_shim():
    body = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    for suf, ct in (("f32", "float"), ("f64", "double")):
        points = ["corrla_ctx* ctx", f"const {ct}* xq", "int64_t n_q", "int64_t ldq", f"const {ct}* xs", "int64_t n_s", "int64_t lds",
                  "int64_t dim", "int kernel", "double eps"]
        want = {"corrla_rbf_matrix_": points + [f"{ct}* out", "int64_t ld_out"],
                "corrla_rbf_apply_": points + ["int poly_degree", f"const {ct}* coeffs", "int64_t ldw", "int64_t n_rhs", f"{ct}* out",
                                               "int64_t ld_out"]}
        for stem, params in want.items():
            for dev in ("", "dev_"):
                name = stem + dev + suf
                m = re.search(r"corrla_status %s\(([^)]*)\)" % name, body)
                assert m, name
                assert [" ".join(p.split()) for p in m.group(1).split(",")] == params, name
                res, args = L.SIGNATURES[name]
                assert res is C.c_int and len(args) == len(params)
                assert args[params.index("int kernel")] is C.c_int and args[params.index("double eps")] is C.c_double
                assert re.search(r"fn %s\(" % name, rs), name
    assert set(s for s in L.SIGNATURES if "_rbf_" in s) == {st + suf for st in STEMS for suf in ("f32", "f64")}
    # the header cites the reference's fit and predict, and states the limits and the exactness properties
    assert "interp_utils.rs:96-129" in HDR and "interp_utils.rs:146-153" in HDR
    assert "1 <= dim <= 128" in HDR and "transpose bitwise" in HDR


@pytest.fixture
def stub():
    return make_stub()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_matrix_and_apply_build_their_calls(stub, dtype):
    c, rec, names = stub
    ct = C.c_float if dtype == np.float32 else C.c_double
    suf = "f32" if dtype == np.float32 else "f64"
    xq = np.arange(21, dtype=dtype).reshape(7, 3)
    xs = np.arange(15.0).reshape(5, 3)                      # float64: converted to the queries' dtype
    out = c.rbf_matrix(xq, xs, 2, 0.5)
    a = rec.calls[-1]
    # (ctx, xq, n_q, ldq, xs, n_s, lds, dim, kernel, eps, out, ld_out)
    assert len(a) == 12 and a[1] == xq.ctypes.data and a[2:4] == (7, 3) and a[5:10] == (5, 3, 3, 2, 0.5)
    assert type(out) is np.ndarray and out.shape == (7, 5) and out.dtype == dtype and a[10] == out.ctypes.data and a[11] == 5
    # kernel ids as in PyRbfInterp::new: 1, 2, 3 themselves, anything else the Gaussian
    for given, want in ((1, 1), (2, 2), (3, 3), (4, 4), (0, 4), (7, 4), (-1, 4)):
        c.rbf_matrix(xq, xs, given)
        assert rec.calls[-1][8] == want and rec.calls[-1][9] == 0.0
    # a view with a padded row stride is passed as it lies
    wide = np.zeros((7, 4), dtype=dtype)
    c.rbf_matrix(wide[:, :3], xs.astype(dtype), 1)
    assert rec.calls[-1][1] == wide.ctypes.data and rec.calls[-1][3] == 4
    # ... a column-major one is not
    c.rbf_matrix(np.asfortranarray(xq), xs, 1)
    assert rec.calls[-1][3] == 3
    n0 = len(rec.calls)
    w = np.arange(18.0).reshape(9, 2)                        # 5 + (3 + 1) rows
    rec.peek = {4: (ct, 15), 11: (ct, 18)}
    res = c.rbf_apply(xq, xs, w, 4, 2.0, poly_degree=1)
    rec.peek = {}
    a = rec.calls[-1]
    # (ctx, xq, n_q, ldq, xs, n_s, lds, dim, kernel, eps, poly_degree, coeffs, ldw, n_rhs, out, ld_out)
    assert len(a) == 16 and a[1] == xq.ctypes.data and a[2:4] == (7, 3) and a[5:11] == (5, 3, 3, 4, 2.0, 1)
    assert a[12:14] == (2, 2) and a[14] == res.ctypes.data and a[15] == 2
    assert type(res) is np.ndarray and res.shape == (7, 2) and res.dtype == dtype
    assert np.array_equal(rec.seen[4], xs.astype(dtype).ravel()) and np.array_equal(rec.seen[11], w.astype(dtype).ravel())
    c.rbf_apply(xq, xs, np.arange(5.0), 1)                                  # no tail: n_s rows; a vector is one column
    assert rec.calls[-1][10] == -1 and rec.calls[-1][12:14] == (1, 1)
    c.rbf_apply(xq, xs, np.zeros((5 + 3 + 6 + 1, 4)), 3, poly_degree=2)     # [x, x_a x_b, 1]
    assert rec.calls[-1][10] == 2 and rec.calls[-1][12:14] == (4, 4)
    c.rbf_apply(xq, xs, np.zeros((9, 1)), 1, poly_degree=0)                 # degree 0 carries the linear tail too
    assert rec.calls[-1][10] == 0
    assert names[:n0] == ["corrla_rbf_matrix_" + suf] * n0 and names[n0:] == ["corrla_rbf_apply_" + suf] * 4


def test_every_bad_argument_raises_before_the_library_is_touched(stub):
    c, rec, _ = stub
    xq, xs, w = np.zeros((6, 3)), np.zeros((4, 3)), np.zeros((8, 2))
    with pytest.raises(ValueError, match="2-D"):
        c.rbf_matrix(np.zeros(5), xs, 1)
    with pytest.raises(ValueError, match="x_support must be 2-D"):
        c.rbf_matrix(xq, np.zeros(3), 1)
    with pytest.raises(ValueError, match="non-empty"):
        c.rbf_matrix(np.zeros((0, 3)), xs, 1)
    with pytest.raises(ValueError, match="non-empty"):
        c.rbf_apply(xq, np.zeros((0, 3)), w, 1)
    with pytest.raises(ValueError, match="x_query has 3 coordinates, x_support 2"):
        c.rbf_matrix(xq, np.zeros((4, 2)), 1)
    with pytest.raises(ValueError, match="x_query has 3 coordinates, x_support 4"):
        c.rbf_apply(xq, np.zeros((4, 4)), w, 1, poly_degree=1)
    with pytest.raises(ValueError, match=r"n_s \+ n_poly = 4 \+ 4 rows, got 7"):
        c.rbf_apply(xq, xs, np.zeros((7, 2)), 1, poly_degree=1)
    with pytest.raises(ValueError, match=r"n_s \+ n_poly = 4 \+ 0 rows, got 8"):
        c.rbf_apply(xq, xs, w, 1)
    with pytest.raises(ValueError, match=r"n_s \+ n_poly = 4 \+ 10 rows, got 8"):
        c.rbf_apply(xq, xs, w, 1, poly_degree=2)
    with pytest.raises(ValueError, match="poly_degree must be None or an integer"):
        c.rbf_apply(xq, xs, w, 1, poly_degree=1.5)
    with pytest.raises(ValueError, match="poly_degree must be None or an integer"):
        c.rbf_apply(xq, xs, w, 1, poly_degree=True)
    with pytest.raises(TypeError):
        c.rbf_apply(xq, xs, w, 1, 0.0, 1)                    # poly_degree is keyword-only
    with pytest.raises(ValueError, match="dense"):
        c.rbf_matrix((np.array([1.0]), np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int64), (1, 3)), xs, 1)
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match=r"no bfloat16 entry"):
        c.rbf_matrix(torch.zeros((4, 3), dtype=torch.bfloat16), xs, 1)
    with pytest.raises(ValueError, match=r"no bfloat16 entry"):
        c.rbf_apply(xq, torch.zeros((4, 3), dtype=torch.bfloat16), w, 1, poly_degree=1)
    with pytest.raises(ValueError, match=r"no bfloat16 entry"):
        c.rbf_apply(xq, xs, torch.zeros((8, 2), dtype=torch.bfloat16), 1, poly_degree=1)
    assert not rec.calls


EMU_PROBE = r"""
#include "emu_backend.cpp"
using corrla::RbfCall;
#define API extern "C" __attribute__((visibility("default")))
API int probe_apply(const double* xq, long long n_q, long long ldq, const double* xs, long long n_s, long long lds, long long dim,
                    int kernel, double eps, int poly_degree, const double* coeffs, long long ldw, long long n_rhs, double* out,
                    long long ld_out) {
  EmuDev dev;
  bool ran = false;
  int st = (int)corrla::guarded([&] {
    const RbfCall<double> c{xq, n_q, ldq, xs, n_s, lds, dim, kernel, eps, poly_degree, coeffs, ldw, n_rhs, out, ld_out};
    corrla::rbf_apply_entry<EmuDev, double>(dev, c, [&] { ran = true; });
  });
  return ran ? -1 : st;
}
API int probe_matrix(const double* xq, long long n_q, long long ldq, const double* xs, long long n_s, long long lds, long long dim,
                     int kernel, double eps, double* out, long long ld_out) {
  EmuDev dev;
  bool ran = false;
  int st = (int)corrla::guarded([&] {
    const RbfCall<double> c{xq, n_q, ldq, xs, n_s, lds, dim, kernel, eps, -1, nullptr, 0, 0, out, ld_out};
    corrla::rbf_matrix_entry<EmuDev, double>(dev, c, [&] { ran = true; });
  });
  return ran ? -1 : st;
}
API const char* probe_error() { return corrla::last_error_slot().c_str(); }
"""


@pytest.fixture(scope="module")
def emu_probe(tmp_path_factory):
    """The emulation backend itself (tests/emu/emu_backend.cpp, unchanged) behind the argument checks of the new entries."""
    tmp = tmp_path_factory.mktemp("rbf_probe")
    src = tmp / "probe.cpp"
    src.write_text(EMU_PROBE)
    so = tmp / "librbf_probe.so"
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "emu"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.probe_error.restype = C.c_char_p
    return lib


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class _Points:
    def __init__(self, n_q=9, n_s=6, dim=3, n_rhs=2):
        rng = np.random.default_rng(0)
        self.xq, self.xs = rng.standard_normal((n_q, dim)), rng.standard_normal((n_s, dim))
        self.w = rng.standard_normal((n_s + dim + 1, n_rhs))
        self.out, self.phi = np.empty((n_q, n_rhs)), np.empty((n_q, n_s))
        self.n_q, self.n_s, self.dim, self.n_rhs = n_q, n_s, dim, n_rhs


def _apply(lib, pt, **kw):
    a = dict(xq=pt.xq, n_q=pt.n_q, ldq=pt.dim, xs=pt.xs, n_s=pt.n_s, lds=pt.dim, dim=pt.dim, kernel=1, eps=0.0, degree=1, w=pt.w,
             ldw=pt.n_rhs, n_rhs=pt.n_rhs, out=pt.out, ld_out=pt.n_rhs)
    a.update(kw)
    LL = C.c_longlong
    rc = lib.probe_apply(_p(a["xq"]), LL(a["n_q"]), LL(a["ldq"]), _p(a["xs"]), LL(a["n_s"]), LL(a["lds"]), LL(a["dim"]), C.c_int(a["kernel"]),
                         C.c_double(a["eps"]), C.c_int(a["degree"]), _p(a["w"]), LL(a["ldw"]), LL(a["n_rhs"]), _p(a["out"]), LL(a["ld_out"]))
    return rc, lib.probe_error()


def _matrix(lib, pt, **kw):
    a = dict(xq=pt.xq, n_q=pt.n_q, ldq=pt.dim, xs=pt.xs, n_s=pt.n_s, lds=pt.dim, dim=pt.dim, kernel=1, eps=0.0, out=pt.phi, ld_out=pt.n_s)
    a.update(kw)
    LL = C.c_longlong
    rc = lib.probe_matrix(_p(a["xq"]), LL(a["n_q"]), LL(a["ldq"]), _p(a["xs"]), LL(a["n_s"]), LL(a["lds"]), LL(a["dim"]), C.c_int(a["kernel"]),
                          C.c_double(a["eps"]), _p(a["out"]), LL(a["ld_out"]))
    return rc, lib.probe_error()


def test_the_emulation_backend_ends_the_calls_with_einval(emu_probe):
    pt = _Points()
    for kw in ({}, dict(kernel=4, eps=0.3), dict(degree=-1), dict(xs=pt.xq, n_s=pt.n_q, w=np.zeros((pt.n_q + 4, 2)))):
        rc, msg = _apply(emu_probe, pt, **kw)
        assert rc == L.EINVAL and b"no radial-basis-function kernels" in msg, (kw, msg)
    for kw in ({}, dict(kernel=3), dict(xs=pt.xq, n_s=pt.n_q, out=np.empty((pt.n_q, pt.n_q)), ld_out=pt.n_q)):
        rc, msg = _matrix(emu_probe, pt, **kw)
        assert rc == L.EINVAL and b"no radial-basis-function kernels" in msg, (kw, msg)


def test_argument_checks_of_the_entries(emu_probe):
    """EINVAL with a message that names the argument, on every backend, before the backend is asked for anything"""
    pt = _Points()
    common = ((dict(xq=None), b"xq is NULL"), (dict(xs=None), b"xs is NULL"), (dict(out=None), b"out is NULL"),
              (dict(n_q=0), b"n_q must be >= 1"), (dict(n_s=0), b"n_s must be >= 1"), (dict(dim=0), b"dim must be in [1, 128]"),
              (dict(dim=129, ldq=129, lds=129), b"dim must be in [1, 128]"), (dict(kernel=0), b"kernel must be in [1, 4]"),
              (dict(kernel=5), b"kernel must be in [1, 4]"), (dict(eps=float("inf")), b"eps must be finite"),
              (dict(eps=float("nan")), b"eps must be finite"), (dict(ldq=2), b"ldq < dim"), (dict(lds=2), b"lds < dim"))
    for kw, word in common + ((dict(w=None), b"coeffs is NULL"), (dict(n_rhs=0), b"n_rhs must be >= 1"), (dict(ldw=1), b"ldw < n_rhs"),
                              (dict(ld_out=1), b"ld_out < n_rhs"), (dict(out=pt.xq), b"out overlaps xq"),
                              (dict(out=pt.xs), b"out overlaps xs"), (dict(out=pt.w), b"out overlaps coeffs")):
        rc, msg = _apply(emu_probe, pt, **kw)
        assert rc == L.EINVAL and b"rbf_apply: " in msg and word in msg, (kw, msg)
    for kw, word in common + ((dict(ld_out=pt.n_s - 1), b"ld_out < n_s"), (dict(out=pt.xq), b"out overlaps xq"),
                              (dict(out=pt.xs), b"out overlaps xs")):
        rc, msg = _matrix(emu_probe, pt, **kw)
        assert rc == L.EINVAL and b"rbf_matrix: " in msg and word in msg, (kw, msg)
    # the coefficient rows of the tail count: with degree 1 the last rows of a longer array belong to coeffs
    big = np.zeros((pt.n_s + pt.dim + 1 + 1, pt.n_rhs))
    rc, msg = _apply(emu_probe, pt, w=big, out=big[-1:], n_q=1)
    assert rc == L.EINVAL and b"no radial-basis-function kernels" in msg           # past the tail: no overlap
    rc, msg = _apply(emu_probe, pt, w=big, out=big[-2:-1], n_q=1)
    assert rc == L.EINVAL and b"out overlaps coeffs" in msg
    rc, msg = _apply(emu_probe, pt, w=big, out=big[pt.n_s:pt.n_s + 1], n_q=1, degree=-1)
    assert rc == L.EINVAL and b"no radial-basis-function kernels" in msg           # no tail: n_s rows


@pytest.mark.parametrize("kernel_type,param", [(1, 0.0), (2, 1.0), (3, 0.0), (4, 0.7), (9, 0.3)])
@pytest.mark.parametrize("degree", [1, 2])
def test_rbf_interp_on_numpy_is_bitwise_what_it_was(kernel_type, param, degree):
    """the formulas are restated here; without `device` numpy input never reaches a Context (there is none to reach)"""
    from corrla_rs_amd.callers import RbfInterp
    rng = np.random.default_rng(kernel_type * 10 + degree)
    x = rng.standard_normal((40, 2))
    y = np.hstack([(np.sin(x[:, 0]) + np.sin(x[:, 1])).reshape(-1, 1), np.cos(x[:, :1])])
    xq = rng.standard_normal((10, 2))

    def phi(r):
        if kernel_type == 1:
            return r
        if kernel_type == 2:
            return np.sqrt(1.0 + (param * r) ** 2)
        if kernel_type == 3:
            return r * r * r
        return np.exp(-((r * param) ** 2))

    def poly(p):
        cols = [p]
        if degree >= 2:
            cols += [p[:, a:a + 1] * p[:, b:b + 1] for a in range(2) for b in range(a, 2)]
        return np.hstack(cols + [np.ones((p.shape[0], 1))])

    def upper(p):
        r = np.sqrt(((p[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
        return np.hstack([phi(r), poly(p)])
    up = upper(x)
    pb = up[:, 40:]
    kp = np.vstack([up, np.hstack([pb.T, np.zeros((pb.shape[1], pb.shape[1]))])])
    u, sv, vt = np.linalg.svd(kp, full_matrices=False)
    coeffs = ((vt.T * (1.0 / (sv + 1.0e-14))) @ u.T) @ np.vstack([y, np.zeros((pb.shape[1], 2))])
    f = RbfInterp(kernel_type, param, 2, degree)
    f._ctx = None

    def no_context():
        raise AssertionError("the host path must not ask for a context")
    f._context = no_context
    f.fit(x, y)
    assert type(f.coeffs) is np.ndarray and np.array_equal(f.coeffs, coeffs) and np.array_equal(f.x_known, x)
    got = f.predict(xq)
    assert type(got) is np.ndarray and got.dtype == np.float64 and np.array_equal(got, upper(xq) @ coeffs)
    assert np.array_equal(f.predict(xq.tolist()), got)             # anything np.asarray takes, as before
    assert f.device is False
    with pytest.raises(ValueError):
        f.predict(np.zeros((3, 5)))


def test_the_device_switch_goes_through_the_context():
    """device=True on numpy: K from rbf_matrix(x, x), the block system on the host, predict through rbf_apply with the
    interpolant's degree"""
    from corrla_rs_amd.callers import RbfInterp
    rng = np.random.default_rng(3)
    x, y, xq = rng.standard_normal((12, 2)), rng.standard_normal((12, 1)), rng.standard_normal((5, 2))
    seen = []

    class Ctx:
        def rbf_matrix(self, a, b, kernel_type, eps=0.0):
            seen.append(("m", a is b, kernel_type, eps))
            return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2))

        def rbf_apply(self, q, xs, w, kernel_type, eps=0.0, *, poly_degree=None):
            seen.append(("a", q.shape, xs.shape, w.shape, kernel_type, eps, poly_degree))
            return "pred"
    f = RbfInterp(1, 0.0, 2, 1, device=True, ctx=Ctx())
    f.fit(x, y)
    host = RbfInterp(1, 0.0, 2, 1)
    host.fit(x, y)
    assert np.array_equal(f.coeffs, host.coeffs)                   # the same K, the same solve
    assert f.predict(xq) == "pred"
    assert seen == [("m", True, 1, 0.0), ("a", (5, 2), (12, 2), (15, 1), 1, 0.0, 1)]
    assert "on the host" in RbfInterp.__doc__ and "1 / (s + 1e-14)" in RbfInterp.__doc__
