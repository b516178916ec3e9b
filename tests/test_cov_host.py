"""Host-side behaviour of the covariance / correlation surface (corrla_rs_amd/api.py, callers.py, _lib.py, capi_impl.hpp), no
GPU needed: the flags and prototypes mirror the header, Context.cov builds the call each switch asks for (seen by a stub
that stands where the entry would be), every bad argument raises before the library is touched, a backend without the
symmetric kernel -- the host emulation backend -- ends the call with EINVAL, rsquared_sens on a stubbed correlation equals
its numpy restatement, and corrla_rs exports the three callers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from corrla_rs_amd import _lib as L
from corrla_rs_amd import api, callers
from tests.api_stub import make_stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "corrla_rsvd.h")).read()


def test_flags_and_routes_equal_the_headers_values():
    for name, val in (("CORRLA_COV_CORRELATION", L.COV_CORRELATION), ("CORRLA_COV_NO_CENTER", L.COV_NO_CENTER)):
        m = re.search(r"#define %s (0x[0-9a-fA-F]+)ull\b" % name, HDR)
        assert m and int(m.group(1), 16) == val, name
    assert L.COV_CORRELATION & L.COV_NO_CENTER == 0
    for name, val in (("CORRLA_COV_ROUTE_INPLACE", L.COV_ROUTE_INPLACE), ("CORRLA_COV_ROUTE_INPLACE_CHECKED", L.COV_ROUTE_INPLACE_CHECKED),
                      ("CORRLA_COV_ROUTE_REPACKED", L.COV_ROUTE_REPACKED)):
        m = re.search(r"#define %s (\d+)\b" % name, HDR)
        assert m and int(m.group(1)) == val, name
    assert sorted(L.COV_ROUTES) == [1, 2, 3]


def test_prototypes_are_declared_bound_and_in_the_rust_shim():
    body = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    for suf, ct in (("f32", "float"), ("f64", "double")):
        for stem in ("corrla_cov_", "corrla_cov_dev_"):
            name = stem + suf
            m = re.search(r"corrla_status %s\(([^)]*)\)" % name, body)
            assert m, name
            params = [p.strip() for p in m.group(1).split(",")]
            assert params == ["corrla_ctx* ctx", f"const {ct}* x", "int64_t m", "int64_t n", "int64_t row_stride", "int64_t col_stride",
                              "uint64_t flags", "int ddof", f"{ct}* means_out", f"{ct}* scales_out", f"{ct}* c", "int64_t ldc",
                              "int* route_out"], params
            res, args = L.SIGNATURES[name]
            assert res is C.c_int and len(args) == 13 and args[6] is C.c_uint64 and args[7] is C.c_int
        assert re.search(r"fn corrla_cov_%s\(" % suf, rs) and re.search(r"fn corrla_cov_dev_%s\(" % suf, rs)
    assert "pub const CORRLA_COV_CORRELATION: u64 = 0x1;" in rs and "pub const CORRLA_COV_NO_CENTER: u64 = 0x2;" in rs


@pytest.fixture
def stub():
    return make_stub(route_out=L.COV_ROUTE_INPLACE_CHECKED)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_each_switch_builds_its_call(stub, dtype):
    c, rec, names = stub
    x = np.arange(60, dtype=dtype).reshape(12, 5)
    assert c.last_cov_route() is None
    cm, means, scales = c.cov(x)
    assert cm.shape == (5, 5) and means.shape == (1, 5) and scales is None and cm.dtype == means.dtype == dtype
    assert type(cm) is np.ndarray and c.last_cov_route() == "inplace_checked"
    a = rec.calls[-1]
    # (ctx, x, m, n, rs, cs, flags, ddof, means_out, scales_out, c, ldc, route_out)
    assert len(a) == 13 and a[1] == x.ctypes.data and a[2:6] == (12, 5, 5, 1)
    assert a[6] == 0 and a[7] == 1 and a[8] == means.ctypes.data and a[9] is None and a[10] == cm.ctypes.data and a[11] == 5
    cm, means, scales = c.cov(x, correlation=True, ddof=0)
    a = rec.calls[-1]
    assert a[6] == L.COV_CORRELATION and a[7] == 0 and a[8] == means.ctypes.data and a[9] == scales.ctypes.data
    assert scales.shape == (1, 5) and scales.dtype == dtype
    cm, means, scales = c.cov(x, center=False)
    a = rec.calls[-1]
    assert means is None and scales is None and a[6] == L.COV_NO_CENTER and a[7] == 1 and a[8] is None and a[9] is None
    # a column-major view passes its strides on: the library, not Python, decides on the repack
    c.cov(np.asfortranarray(x))
    assert rec.calls[-1][2:6] == (12, 5, 1, 12)
    assert names == ["corrla_cov_" + ("f32" if dtype == np.float32 else "f64")] * 4


def test_other_dtypes_become_float64(stub):
    c, rec, names = stub
    cm, means, _ = c.cov(np.arange(12, dtype=np.int32).reshape(4, 3))
    assert cm.dtype == means.dtype == np.float64 and names == ["corrla_cov_f64"]
    cm, _, _ = c.cov([[1.0, 2.0], [3.0, 5.0], [4.0, 4.0]])
    assert cm.shape == (2, 2) and rec.calls[-1][2:4] == (3, 2)


def test_every_bad_argument_raises_before_the_library_is_touched(stub):
    c, rec, _ = stub
    x = np.zeros((6, 3))
    with pytest.raises(ValueError, match="correlation=True needs center=True"):
        c.cov(x, correlation=True, center=False)
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="correlation must be True or False"):
            c.cov(x, correlation=bad)
        with pytest.raises(ValueError, match="center must be True or False"):
            c.cov(x, center=bad)
    for bad in (2, -1, 0.5, 0.0, 1.0, None, True, "1"):
        with pytest.raises(ValueError, match="ddof must be 0 or 1"):
            c.cov(x, ddof=bad)
    with pytest.raises(ValueError, match="2-D"):
        c.cov(np.zeros(5))
    with pytest.raises(ValueError, match="non-empty"):
        c.cov(np.zeros((0, 3)))
    with pytest.raises(ValueError, match="no sparse entry.*dense"):
        c.cov((np.array([1.0]), np.array([0], dtype=np.int32), np.array([0, 1, 1], dtype=np.int64), (2, 2)))
    with pytest.raises(TypeError):
        c.cov(x, True)                      # the switches are keyword-only
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match=r"no bfloat16 entry: pass \.float\(\)"):
        c.cov(torch.zeros((4, 3), dtype=torch.bfloat16))
    assert not rec.calls


EMU_PROBE = r"""
#include "emu_backend.cpp"
extern "C" __attribute__((visibility("default"))) int probe_cov(const double* x, long long m, long long n, long long rs, long long cs,
                                                               unsigned long long flags, int ddof, double* c, long long ldc,
                                                               int* route) {
  EmuDev dev;
  bool ran = false;
  int st = (int)corrla::guarded([&] {
    const corrla::CovCall<double> call{x, m, n, rs, cs, flags, ddof, nullptr, nullptr, c, ldc, route};
    corrla::cov_entry<EmuDev, double>(dev, call, [&] { ran = true; });
  });
  return ran ? -1 : st;
}
extern "C" __attribute__((visibility("default"))) const char* probe_error() { return corrla::last_error_slot().c_str(); }
"""


@pytest.fixture(scope="module")
def emu_probe(tmp_path_factory):
    """The emulation backend itself (tests/emu/emu_backend.cpp, unchanged) behind the argument checks of corrla_cov_*."""
    tmp = tmp_path_factory.mktemp("cov_probe")
    src = tmp / "probe.cpp"
    src.write_text(EMU_PROBE)
    so = tmp / "libcov_probe.so"
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "emu"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.probe_error.restype = C.c_char_p
    return lib


def _probe(lib, x, flags=0, ddof=1, c=None, ldc=None, m=None, n=None):
    mm, nn = x.shape
    c = np.empty((nn, nn)) if c is None else c
    route = C.c_int(7)
    rc = lib.probe_cov(C.c_void_p(x.ctypes.data), C.c_longlong(mm if m is None else m), C.c_longlong(nn if n is None else n),
                       C.c_longlong(x.strides[0] // 8), C.c_longlong(x.strides[1] // 8), C.c_ulonglong(flags), C.c_int(ddof),
                       C.c_void_p(c.ctypes.data), C.c_longlong(nn if ldc is None else ldc), C.byref(route))
    return rc, route.value, lib.probe_error()


def test_the_emulation_backend_ends_the_call_with_einval(emu_probe):
    x = np.random.default_rng(0).standard_normal((30, 6))
    rc, route, msg = _probe(emu_probe, x)
    assert rc == L.EINVAL and route == 0 and b"no symmetric rank-k kernel" in msg
    rc, _, msg = _probe(emu_probe, x, flags=L.COV_CORRELATION)
    assert rc == L.EINVAL and b"no symmetric rank-k kernel" in msg


def test_argument_checks_of_the_entry(emu_probe):
    """EINVAL with its own message, on every backend, before the backend is asked for anything"""
    x = np.random.default_rng(1).standard_normal((30, 6))
    for kw, word in ((dict(flags=L.COV_CORRELATION | L.COV_NO_CENTER), b"mutually exclusive"), (dict(flags=4), b"unknown flag"),
                     (dict(ddof=2), b"ddof"), (dict(ddof=-1), b"ddof"), (dict(ldc=5), b"ldc < n"), (dict(n=0), b"empty"),
                     (dict(m=1, ddof=1), b"n_samples - ddof < 1"), (dict(m=0, ddof=0), b"empty")):
        rc, route, msg = _probe(emu_probe, x, **kw)
        assert rc == L.EINVAL and word in msg and route == 0, (kw, msg)
    # overlapping buffers: c inside x
    rc, _, msg = _probe(emu_probe, x, c=x[:6, :6])
    assert rc == L.EINVAL and b"cov: c overlaps x" in msg
    # m = 1 with ddof = 0 passes the checks (and then meets the backend's refusal)
    rc, _, msg = _probe(emu_probe, x, m=1, ddof=0)
    assert rc == L.EINVAL and b"no symmetric rank-k kernel" in msg


def test_rsquared_sens_on_a_stubbed_correlation_equals_its_numpy_restatement():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((100, 2)) @ np.array([[0.9, 0.5], [0.5, 0.9]])
    y = x[:, :1] + x[:, 1:] ** 2

    class Ctx:
        seen = []

        def cov(self, a, *, correlation=False, center=True, ddof=1):
            self.seen.append((a.shape, correlation, center, ddof))
            return np.corrcoef(a, rowvar=False), None, None

    r = np.corrcoef(np.hstack([x, y]), rowvar=False)
    u, s, vt = np.linalg.svd(r[:2, :2])
    want = r[:2, 2:].T @ ((vt.T * (1.0 / (s + 1.0e-14))) @ u.T) @ r[:2, 2:]
    ctx = Ctx()
    got = callers.rsquared_sens(x, y, False, ctx=ctx)
    assert got.shape == (1, 1) and abs(got[0, 0] - want[0, 0]) <= 1e-12 and 0.0 < got[0, 0] < 1.0
    got_dof = callers.rsquared_sens(x, y.ravel(), True, ctx=ctx)
    want_dof = 1.0 - (1.0 - want) * (99.0 / 97.0)
    assert abs(got_dof[0, 0] - want_dof[0, 0]) <= 1e-12 and got_dof[0, 0] < got[0, 0]
    assert ctx.seen == [((100, 3), True, True, 1)] * 2
    # the two matrix callers pass the context's first result through
    assert callers.pearson_corr(x, ctx=ctx).shape == (2, 2) and ctx.seen[-1] == ((100, 2), True, True, 1)
    assert callers.mat_cov_centered(x, ctx=ctx).shape == (2, 2) and ctx.seen[-1] == ((100, 2), False, True, 1)


def test_corrla_rs_exports_the_additive_callers():
    import corrla_rs
    import corrla_rs_amd
    for name in ("mat_cov_centered", "pearson_corr", "rsquared_sens"):
        assert getattr(corrla_rs, name) is getattr(callers, name) is getattr(corrla_rs_amd, name)
        assert name in corrla_rs.__all__ and name in callers.__all__
    assert "additive" in corrla_rs.__doc__.lower()
