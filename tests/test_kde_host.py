"""Host-side behaviour of the kernel-density surface (corrla_rs_amd/api.py, callers.py, _lib.py, capi_impl.hpp), no GPU needed:
the prototypes of the header are bound and in the rust shim, Context.kde_eval / kde_nll build the call each argument asks for
(seen by a stub that stands where the entry would be), every bad argument raises before the library is touched, a backend
without the kernels -- the host emulation backend -- ends the call with EINVAL after the argument checks, the numpy path of
KdeRv agrees with the committed fixture (tests/golden/kde/kde_known.npz) within the bounds of tests/test_gpu_kde.py, and
est_bandwidth / build_kde find what they say they find."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from corrla_rs_amd import _lib as L
from corrla_rs_amd import api
from tests.api_stub import make_stub
from tests.test_gpu_kde import assert_brackets_the_minimum, known, known_eval_bounds, nll_bounds, seeded_case
from tests.test_kde_plan import BASE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "corrla_rsvd.h")).read()
STEMS = ("corrla_kde_eval_", "corrla_kde_eval_dev_", "corrla_kde_nll_", "corrla_kde_nll_dev_")


def test_prototypes_are_declared_bound_and_in_the_rust_shim():
    body = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    for suf, ct in (("f32", "float"), ("f64", "double")):
        def points(n):
            return ["corrla_ctx* ctx", f"const {ct}* x", f"int64_t {n}", "int64_t incx", f"const {ct}* s", "int64_t n_s", "int64_t incs"]
        want = {"corrla_kde_eval_": points("n_q") + ["double h", "int what", f"{ct}* out", "int64_t inco"],
                "corrla_kde_nll_": points("n_t") + ["const double* h", "int64_t n_h", "double* nll", "double* dnll"]}
        for stem, params in want.items():
            for dev in ("", "dev_"):
                name = stem + dev + suf
                m = re.search(r"corrla_status %s\(([^)]*)\)" % name, body)
                assert m, name
                assert [" ".join(p.split()) for p in m.group(1).split(",")] == params, name
                res, args = L.SIGNATURES[name]
                assert res is C.c_int and len(args) == len(params)
                if stem == "corrla_kde_eval_":
                    assert args[params.index("double h")] is C.c_double and args[params.index("int what")] is C.c_int
                assert re.search(r"fn %s\(" % name, rs), name
    assert set(s for s in L.SIGNATURES if "_kde_" in s) == {st + suf for st in STEMS for suf in ("f32", "f64")}
    assert "corrla_ctx_last_kde" in L.SIGNATURES and re.search(r"fn corrla_ctx_last_kde\(", rs)
    # the header cites the reference's likelihood and its pdf / cdf, and states the limits and the stabilised form
    assert "univariate_rv.rs:165-170" in HDR and "univariate_rv.rs:423-444" in HDR
    assert "1 <= n_h <= 64" in HDR and "Stabilised form" in HDR and "deliberate difference" in HDR and "-inf" in HDR


@pytest.fixture
def stub():
    return make_stub(last={"corrla_ctx_last_kde": (2,)})


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_eval_and_nll_build_their_calls(stub, dtype):
    c, rec, names = stub
    suf = "f32" if dtype == np.float32 else "f64"
    x, s = np.arange(7, dtype=dtype), np.arange(5, dtype=dtype) + 0.5
    for what, code in (("pdf", 0), ("cdf", 1), ("logpdf", 2)):
        out = c.kde_eval(x, s, 0.25, what)
        a = rec.calls[-1]
        # (ctx, x, n_q, incx, s, n_s, incs, h, what, out, inco)
        assert len(a) == 11 and a[1] == x.ctypes.data and a[2:4] == (7, 1) and a[4] == s.ctypes.data and a[5:9] == (5, 1, 0.25, code)
        assert type(out) is np.ndarray and out.shape == (7,) and out.dtype == dtype and a[9] == out.ctypes.data and a[10] == 1
    assert c.last_kde_route() == "split"                    # what the stub's corrla_ctx_last_kde reported
    # an n x 1 column, as the reference's column matrices: the same call, a column back
    out = c.kde_eval(x.reshape(-1, 1), s.reshape(-1, 1), 2, "pdf")
    a = rec.calls[-1]
    assert a[1] == x.ctypes.data and a[2:4] == (7, 1) and a[5:8] == (5, 1, 2.0) and out.shape == (7, 1)
    # strided views are read where they lie: element strides, not copies
    wide_x, wide_s = np.zeros(21, dtype=dtype), np.zeros((5, 2), dtype=dtype)
    c.kde_eval(wide_x[1::3], wide_s[:, 1:], 1.0)
    a = rec.calls[-1]
    assert a[1] == wide_x.ctypes.data + wide_x.itemsize and a[2:4] == (7, 3)
    assert a[4] == wide_s.ctypes.data + wide_s.itemsize and a[5:7] == (5, 2) and a[8] == 0 and a[10] == 1
    # a reversed view has no stride >= 1: it is copied
    c.kde_eval(x[::-1], s, 1.0)
    assert rec.calls[-1][1] != x.ctypes.data and rec.calls[-1][3] == 1
    # one element: the stride does not matter
    c.kde_eval(wide_x[5:6], s, 1.0)
    assert rec.calls[-1][2:4] == (1, 1)
    # anything that is not float32 becomes float64 -- for both arrays alike
    c.kde_eval(np.arange(3), np.arange(4), 1.0)
    assert names[-1] == "corrla_kde_eval_f64"
    n0 = len(rec.calls)
    assert names == ["corrla_kde_eval_" + suf] * (n0 - 1) + ["corrla_kde_eval_f64"]
    rec.peek = {7: (C.c_double, 3)}
    nll, dnll = c.kde_nll(wide_x[1::3], s, [0.5, 1.0, 2.0])
    rec.peek = {}
    a = rec.calls[-1]
    # (ctx, x, n_t, incx, s, n_s, incs, h, n_h, nll, dnll)
    assert len(a) == 11 and a[1] == wide_x.ctypes.data + wide_x.itemsize and a[2:4] == (7, 3) and a[4] == s.ctypes.data and a[5:7] == (5, 1)
    assert a[8] == 3 and np.array_equal(rec.seen[7], [0.5, 1.0, 2.0])
    assert nll.dtype == dnll.dtype == np.float64 and nll.shape == dnll.shape == (3,) and a[9] == nll.ctypes.data and a[10] == dnll.ctypes.data
    c.kde_nll(x, s, 0.75)                                    # a scalar is one bandwidth
    assert rec.calls[-1][8] == 1
    c.kde_nll(x, s, np.geomspace(0.1, 10.0, 64))
    assert rec.calls[-1][8] == 64
    assert names[n0:] == ["corrla_kde_nll_" + suf] * 3


def test_every_bad_argument_raises_before_the_library_is_touched(stub):
    c, rec, _ = stub
    x, s = np.zeros(6), np.ones(4)
    with pytest.raises(ValueError, match="x is float32, supports float64"):
        c.kde_eval(x.astype(np.float32), s, 1.0)
    with pytest.raises(ValueError, match="x is float64, supports float32"):
        c.kde_nll(x, s.astype(np.float32), 1.0)
    with pytest.raises(ValueError, match="x must be non-empty"):
        c.kde_eval(np.zeros(0), s, 1.0)
    with pytest.raises(ValueError, match="supports must be non-empty"):
        c.kde_nll(x, np.zeros((0, 1)), 1.0)
    with pytest.raises(ValueError, match="x must be a vector or an n x 1 column"):
        c.kde_eval(np.zeros((3, 2)), s, 1.0)
    with pytest.raises(ValueError, match="supports must be a vector or an n x 1 column"):
        c.kde_eval(x, np.zeros((2, 2, 1)), 1.0)
    with pytest.raises(ValueError, match='what must be "pdf", "cdf" or "logpdf"'):
        c.kde_eval(x, s, 1.0, "sf")
    for h in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="bandwidth must be finite and > 0"):
            c.kde_eval(x, s, h)
        with pytest.raises(ValueError, match="every bandwidth must be finite and > 0"):
            c.kde_nll(x, s, [1.0, h])
    with pytest.raises(ValueError, match="bandwidths must be 1 to 64 values"):
        c.kde_nll(x, s, [])
    with pytest.raises(ValueError, match="bandwidths must be 1 to 64 values"):
        c.kde_nll(x, s, np.ones(65))
    with pytest.raises(ValueError, match="bandwidths must be 1 to 64 values"):
        c.kde_nll(x, s, np.ones((2, 2)))
    with pytest.raises(ValueError, match="dense"):
        c.kde_eval((np.array([1.0]), np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int64), (1, 3)), s, 1.0)
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match=r"no bfloat16 entry"):
        c.kde_eval(torch.zeros(4, dtype=torch.bfloat16), s, 1.0)
    with pytest.raises(ValueError, match=r"no bfloat16 entry"):
        c.kde_nll(x, torch.zeros(4, dtype=torch.bfloat16), 1.0)

    class OnGpu:                           # what api looks at of a CUDA tensor, without a GPU
        is_cuda, dtype, shape, ndim = True, torch.float64, (4,), 1

        def __init__(self, index):
            self.device = torch.device("cuda", index)

        def detach(self):
            return self

        def dim(self):
            return 1

        def stride(self, i):
            return 1
    OnGpu.__module__ = "torch"
    with pytest.raises(ValueError, match="tensor is on cuda:1, context is on cuda:0"):
        c.kde_eval(OnGpu(1), s, 1.0)
    with pytest.raises(ValueError, match="both be numpy arrays or both be tensors on cuda:0"):
        c.kde_eval(x, OnGpu(0), 1.0)
    with pytest.raises(ValueError, match="both be numpy arrays or both be tensors on cuda:0"):
        c.kde_nll(OnGpu(0), s, 1.0)
    assert not rec.calls


EMU_PROBE = r"""
#include "emu_backend.cpp"
using corrla::KdeEvalCall;
using corrla::KdeNllCall;
#define API extern "C" __attribute__((visibility("default")))
API int probe_eval(const double* x, long long n_q, long long incx, const double* s, long long n_s, long long incs, double h, int what,
                   double* out, long long inco) {
  EmuDev dev;
  bool ran = false;
  int st = (int)corrla::guarded([&] {
    const KdeEvalCall<double> c{x, n_q, incx, s, n_s, incs, h, what, out, inco};
    corrla::kde_eval_entry<EmuDev, double>(dev, c, [&] { ran = true; });
  });
  return ran ? -1 : st;
}
API int probe_nll(const double* x, long long n_t, long long incx, const double* s, long long n_s, long long incs, const double* h,
                  long long n_h, double* nll, double* dnll) {
  EmuDev dev;
  bool ran = false;
  int st = (int)corrla::guarded([&] {
    const KdeNllCall<double> c{x, n_t, incx, s, n_s, incs, h, n_h, nll, dnll};
    corrla::kde_nll_entry<EmuDev, double>(dev, c, [&] { ran = true; });
  });
  return ran ? -1 : st;
}
API const char* probe_error() { return corrla::last_error_slot().c_str(); }
"""


@pytest.fixture(scope="module")
def emu_probe(tmp_path_factory):
    """The emulation backend itself (tests/emu/emu_backend.cpp, unchanged) behind the argument checks of the new entries."""
    tmp = tmp_path_factory.mktemp("kde_probe")
    src = tmp / "probe.cpp"
    src.write_text(EMU_PROBE)
    so = tmp / "libkde_probe.so"
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "emu"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.probe_error.restype = C.c_char_p
    return lib


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class _Data:
    def __init__(self, n_q=9, n_s=6, n_h=3):
        rng = np.random.default_rng(0)
        self.x, self.s, self.h = rng.standard_normal(n_q), rng.standard_normal(n_s), np.array([0.5, 1.0, 2.0])[:n_h].copy()
        self.out, self.nll, self.dnll = np.empty(n_q), np.empty(n_h), np.empty(n_h)
        self.n_q, self.n_s, self.n_h = n_q, n_s, n_h


def _eval(lib, dt, **kw):
    a = dict(x=dt.x, n_q=dt.n_q, incx=1, s=dt.s, n_s=dt.n_s, incs=1, h=0.7, what=0, out=dt.out, inco=1)
    a.update(kw)
    LL = C.c_longlong
    rc = lib.probe_eval(_p(a["x"]), LL(a["n_q"]), LL(a["incx"]), _p(a["s"]), LL(a["n_s"]), LL(a["incs"]), C.c_double(a["h"]), C.c_int(a["what"]),
                        _p(a["out"]), LL(a["inco"]))
    return rc, lib.probe_error()


def _nll(lib, dt, **kw):
    a = dict(x=dt.x, n_t=dt.n_q, incx=1, s=dt.s, n_s=dt.n_s, incs=1, h=dt.h, n_h=dt.n_h, nll=dt.nll, dnll=dt.dnll)
    a.update(kw)
    LL = C.c_longlong
    rc = lib.probe_nll(_p(a["x"]), LL(a["n_t"]), LL(a["incx"]), _p(a["s"]), LL(a["n_s"]), LL(a["incs"]), _p(a["h"]), LL(a["n_h"]),
                       _p(a["nll"]), _p(a["dnll"]))
    return rc, lib.probe_error()


def test_the_emulation_backend_ends_the_calls_with_einval(emu_probe):
    dt = _Data()
    for kw in ({}, dict(what=1), dict(what=2, h=1e-9), dict(s=dt.x, n_s=dt.n_q), dict(x=np.zeros(30), incx=3, out=np.zeros(20), inco=2)):
        rc, msg = _eval(emu_probe, dt, **kw)
        assert rc == L.EINVAL and b"this backend has no kernel-density kernels" in msg, (kw, msg)
    for kw in ({}, dict(dnll=None), dict(n_h=1), dict(h=np.geomspace(0.1, 9.0, 64), n_h=64, nll=np.empty(64), dnll=np.empty(64))):
        rc, msg = _nll(emu_probe, dt, **kw)
        assert rc == L.EINVAL and b"this backend has no kernel-density kernels" in msg, (kw, msg)


def test_argument_checks_of_the_entries(emu_probe):
    """EINVAL with a message that names the argument, on every backend, before the backend is asked for anything"""
    dt = _Data()
    common = ((dict(x=None), b"x is NULL"), (dict(s=None), b"s is NULL"), (dict(n_s=0), b"n_s must be >= 1"),
              (dict(incx=0), b"incx must be >= 1"), (dict(incs=0), b"incs must be >= 1"), (dict(incs=-1), b"incs must be >= 1"))
    for kw, word in common + ((dict(out=None), b"out is NULL"), (dict(n_q=0), b"n_q must be >= 1"), (dict(inco=0), b"inco must be >= 1"),
                              (dict(h=0.0), b"h must be finite and > 0"), (dict(h=-1.0), b"h must be finite and > 0"),
                              (dict(h=float("inf")), b"h must be finite and > 0"), (dict(h=float("nan")), b"h must be finite and > 0"),
                              (dict(what=-1), b"what must be 0 (pdf), 1 (cdf) or 2 (logpdf)"), (dict(what=3), b"what must be 0"),
                              (dict(out=dt.x), b"out overlaps x"), (dict(out=dt.s, n_q=dt.n_s), b"out overlaps s")):
        rc, msg = _eval(emu_probe, dt, **kw)
        assert rc == L.EINVAL and b"kde_eval: " in msg and word in msg, (kw, msg)
    bad_h = dt.h.copy()
    bad_h[2] = float("nan")
    for kw, word in common + ((dict(h=None), b"h is NULL"), (dict(nll=None), b"nll is NULL"), (dict(n_t=0), b"n_t must be >= 1"),
                              (dict(n_h=0), b"n_h must be in [1, 64]"), (dict(n_h=65), b"n_h must be in [1, 64]"),
                              (dict(h=bad_h), b"every h must be finite and > 0"), (dict(h=-dt.h), b"every h must be finite and > 0"),
                              (dict(nll=dt.x), b"nll overlaps x"), (dict(dnll=dt.s), b"dnll overlaps s"),
                              (dict(dnll=dt.nll), b"nll overlaps dnll")):
        rc, msg = _nll(emu_probe, dt, **kw)
        assert rc == L.EINVAL and b"kde_nll: " in msg and word in msg, (kw, msg)
    # a strided span counts to its last element: out right behind it does not overlap, out on it does
    buf = np.zeros(40)
    rc, msg = _eval(emu_probe, dt, x=buf, incx=3, out=buf[25:], n_q=9)
    assert rc == L.EINVAL and b"no kernel-density kernels" in msg
    rc, msg = _eval(emu_probe, dt, x=buf, incx=3, out=buf[24:], n_q=9)
    assert rc == L.EINVAL and b"out overlaps x" in msg


def test_the_numpy_path_agrees_with_the_fixture():
    """KdeRv without `device` on numpy input: the stabilised formulas in float64, judged by the GPU file's bounds for f64 (the
    same operation order; numpy's pairwise sums and its exp stay within the n_s u and 2 ulp the bounds allow)."""
    from corrla_rs_amd.callers import KdeRv
    n_q, n_s, _ = BASE
    k = known(n_q, n_s)
    x, s, h = k["x"].astype(np.float64), k["s"].astype(np.float64), k["h"]
    rv = KdeRv(float(h[0]), s)
    rv._context = None                                     # the host path must not ask for a context
    for what in ("pdf", "cdf", "logpdf"):
        got = getattr(rv, what)(x)
        assert type(got) is np.ndarray and got.dtype == np.float64 and got.shape == x.shape
        assert np.all(np.abs(got - k[what]) <= known_eval_bounds(n_q, n_s, np.float64, what)), what
    # the far point: its plain density underflows (the reference's ln pdf is -inf there), logpdf and nll stay finite
    plain = np.exp(-(x[-1] - s) ** 2 / (2.0 * h[0] ** 2)).sum()
    assert plain == 0.0 and k["pdf"][-1] == 0.0 and np.isfinite(rv.logpdf(x[-1:])[0]) and rv.pdf(x[-1:])[0] == 0.0
    nll, dnll = rv.nll_dnll(x, h[:3])
    for b in range(3):
        nb, db = nll_bounds(n_q, n_s, b, np.float64)
        assert abs(nll[b] - k["nll"][b]) <= nb and abs(dnll[b] - k["dnll"][b]) <= db, b
    assert np.isfinite(rv.nll(x)) and rv.nll(x) == nll[0] and np.array_equal(rv.nll(x, h[:3]), nll)
    assert rv.logpdf(x.reshape(-1, 1)).shape == (n_q, 1) and np.array_equal(rv.logpdf(x.tolist()), rv.logpdf(x))
    # the blocks of the host path hold at most 2^21 pairs, whatever the sizes
    from corrla_rs_amd import callers
    for shape in ((n_q, n_s), (10 ** 5, 10 ** 5), (3, 10 ** 7), (10 ** 7, 3)):
        rows, sc = callers._kde_host_blocks(*shape)
        assert rows >= 1 and sc >= 1 and rows * sc <= callers._KDE_HOST_PAIRS == 1 << 21
    draws = rv.sample(1000, seed=5)
    assert draws.shape == (1000,) and np.array_equal(draws, rv.sample(1000, seed=5))
    assert np.all(np.abs(draws[:, None] - s[None, :]).min(axis=1) < 8.0 * h[0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=("f32", "f64"))
def test_est_bandwidth_on_the_seeded_case(dtype):
    from corrla_rs_amd.callers import KdeRv
    s, x = seeded_case(dtype)
    rtol = 1e-6
    rv = KdeRv(1.0, s)
    rv._context = None
    h = rv.est_bandwidth(x, 2, rtol=rtol)                    # `method` is accepted and ignored
    assert rv.bandwidth == h and 1e-9 <= h <= 1000.0 and 4.0 < h < 6.0 and rv.n_nll_calls <= 12
    assert_brackets_the_minimum(s, x, h, rtol)
    assert KdeRv(50.0, s).est_bandwidth(x, rtol=rtol) == h   # global over the bounds: the start does not matter
    # the result stays inside the bounds when the minimum does not
    assert KdeRv(1.0, s).est_bandwidth(x, bounds=(0.1, 2.0)) == 2.0
    assert KdeRv(1.0, s).est_bandwidth(x, bounds=(20.0, 100.0)) == 20.0
    # the search starts where the reference's likelihood is -inf
    assert np.isfinite(rv.nll(x, 1e-9))
    with pytest.raises(ValueError, match="bounds"):
        rv.est_bandwidth(x, bounds=(0.0, 1.0))
    assert "At most 12 evaluations" in KdeRv.__doc__
    assert "ignored" in KdeRv.__doc__ and "clamps to the bounds" in KdeRv.__doc__


def test_build_kde_is_seeded_and_takes_the_stated_order_statistic():
    from corrla_rs_amd.callers import build_kde
    from corrla_rs import KdeRv as exported, build_kde as exported_build
    rng = np.random.default_rng(11)
    samples = rng.normal(5.25, 10.0, 160)
    a, b = build_kde(1.0, samples, 6, 2, seed=7), build_kde(1.0, samples, 6, 2, seed=7)
    assert a.bandwidth == b.bandwidth and np.array_equal(a.bandwidth_estimates, b.bandwidth_estimates)
    assert a.bandwidth_estimates.shape == (6,) and a.bandwidth == np.sort(a.bandwidth_estimates)[6 // 2]
    assert np.array_equal(a.supports, samples) and isinstance(a, exported) and exported_build is build_kde
    assert build_kde(1.0, samples, 6, 2, seed=8).bandwidth != a.bandwidth
    one = build_kde(1.0, samples.reshape(-1, 1), 1, 0, seed=7)
    assert one.bandwidth == one.bandwidth_estimates[0] == a.bandwidth_estimates[0]
