"""Host-side behaviour of the fitted-model surface (corrla_rs_amd/api.py, _lib.py, capi_impl.hpp), no GPU needed: the flags and
prototypes mirror the header, Context.pca_transform / pca_inverse_transform build the call each switch asks for (seen by a
stub that stands where the entry would be), every bad argument raises before the library is touched, a backend without the
back-projection kernel -- the host emulation backend -- ends the call with EINVAL after the argument checks, and
PcaRsvd.apply_tr / apply_inv_tr on numpy input of a host-fitted model are bit for bit the numpy formulas they were."""
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
STEMS = ("corrla_pca_transform_", "corrla_pca_transform_dev_", "corrla_pca_transform_csr_", "corrla_pca_transform_csr_dev_",
         "corrla_pca_inverse_", "corrla_pca_inverse_dev_")


def test_flags_and_routes_equal_the_headers_values():
    m = re.search(r"#define CORRLA_PCA_APPLY_OWN_MEANS (0x[0-9a-fA-F]+)ull\b", HDR)
    assert m and int(m.group(1), 16) == L.PCA_APPLY_OWN_MEANS
    # the centre flags are those of corrla_opts.flags, reused by value
    for name, val in (("CORRLA_PCA_CENTER_FUSED", L.PCA_CENTER_FUSED), ("CORRLA_PCA_CENTER_COPY", L.PCA_CENTER_COPY)):
        m = re.search(r"#define %s (0x[0-9a-fA-F]+)u\b" % name, HDR)
        assert m and int(m.group(1), 16) == val, name
    assert L.PCA_APPLY_OWN_MEANS & (L.PCA_CENTER_FUSED | L.PCA_CENTER_COPY) == 0
    for name, val in (("CORRLA_PCA_APPLY_ROUTE_INPLACE", L.PCA_APPLY_ROUTE_INPLACE),
                      ("CORRLA_PCA_APPLY_ROUTE_INPLACE_CHECKED", L.PCA_APPLY_ROUTE_INPLACE_CHECKED),
                      ("CORRLA_PCA_APPLY_ROUTE_REPACKED", L.PCA_APPLY_ROUTE_REPACKED)):
        m = re.search(r"#define %s (\d+)\b" % name, HDR)
        assert m and int(m.group(1)) == val, name
    assert sorted(L.PCA_APPLY_ROUTES) == [1, 2, 3] and L.PCA_APPLY_CENTRINGS == {1: "fused", 2: "copy"}


def test_prototypes_are_declared_bound_and_in_the_rust_shim():
    body = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    for suf, ct in (("f32", "float"), ("f64", "double")):
        model = [f"const {ct}* means", f"const {ct}* scales", f"const {ct}* components", "int64_t ldc", "int64_t k", "uint64_t flags",
                 f"{ct}* scores", "int64_t ld_scores", f"{ct}* resid_out", f"{ct}* means_out"]
        want = {"corrla_pca_transform_": ["corrla_ctx* ctx", f"const {ct}* x", "int64_t m", "int64_t n", "int64_t row_stride",
                                          "int64_t col_stride"] + model,
                "corrla_pca_transform_csr_": ["corrla_ctx* ctx", f"const {ct}* values", "const int32_t* col_idx", "const int64_t* row_ptr",
                                              "int64_t m", "int64_t n", "int64_t nnz"] + model,
                "corrla_pca_inverse_": ["corrla_ctx* ctx", f"const {ct}* scores", "int64_t m", "int64_t k", "int64_t ld_scores",
                                        f"const {ct}* means", f"const {ct}* scales", f"const {ct}* components", "int64_t ldc", "int64_t n",
                                        f"{ct}* out", "int64_t row_stride_out"]}
        for stem, params in want.items():
            for dev in ("", "dev_"):
                name = stem + dev + suf
                m = re.search(r"corrla_status %s\(([^)]*)\)" % name, body)
                assert m, name
                assert [" ".join(p.split()) for p in m.group(1).split(",")] == params, name
                res, args = L.SIGNATURES[name]
                assert res is C.c_int and len(args) == len(params)
                flag_at = params.index("uint64_t flags") if "uint64_t flags" in params else None
                if flag_at is not None:
                    assert args[flag_at] is C.c_uint64
                assert re.search(r"fn %s\(" % name, rs), name
    assert "pub const CORRLA_PCA_APPLY_OWN_MEANS: u64 = 0x400;" in rs
    assert "corrla_ctx_last_pca_apply" in L.SIGNATURES and re.search(r"fn corrla_ctx_last_pca_apply\(", rs)
    assert set(s for s in L.SIGNATURES if "pca_transform" in s or "pca_inverse" in s) == {st + suf for st in STEMS for suf in ("f32", "f64")}
    # the header cites the reference's two methods
    assert "pca_rsvd.rs:43-46" in HDR and "pca_rsvd.rs:49-52" in HDR


@pytest.fixture
def stub():
    return make_stub(last={"corrla_ctx_last_pca_apply": (2, L.PCA_APPLY_ROUTE_INPLACE_CHECKED)})


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_each_switch_of_transform_builds_its_call(stub, dtype):
    c, rec, names = stub
    x = np.arange(60, dtype=dtype).reshape(12, 5)
    means, scales = np.arange(5.0), np.arange(1.0, 6.0)
    comps = np.arange(10.0).reshape(2, 5)
    assert c.last_pca_apply_route() is None and c.last_pca_apply_centring() is None
    ct = C.c_float if dtype == np.float32 else C.c_double
    rec.peek = {6: (ct, 5), 8: (ct, 10)}
    t = c.pca_transform(x, means, comps)
    rec.peek = {}
    assert type(t) is np.ndarray and t.shape == (12, 2) and t.dtype == dtype and t.flags.f_contiguous
    assert c.last_pca_apply_route() == "inplace_checked" and c.last_pca_apply_centring() == "copy"
    a = rec.calls[-1]
    # (ctx, x, m, n, rs, cs, means, scales, components, ldc, k, flags, scores, ld_scores, resid_out, means_out)
    assert len(a) == 16 and a[1] == x.ctypes.data and a[2:6] == (12, 5, 5, 1)
    assert a[6] is not None and a[7] is None and a[9:12] == (2, 2, 0) and a[12] == t.ctypes.data and a[13] == 12
    assert a[14] is None and a[15] is None
    # the model arrays arrive in x's dtype; the components column-major with ldc = k
    assert np.array_equal(rec.seen[8], comps.astype(dtype).ravel(order="F")) and np.array_equal(rec.seen[6], means.astype(dtype))
    t, q = c.pca_transform(x, means.reshape(1, 5), comps, scales.reshape(1, 5), residuals=True, center="fused")
    a = rec.calls[-1]
    assert a[7] is not None and a[11] == L.PCA_CENTER_FUSED and q.shape == (12,) and q.dtype == dtype and a[14] == q.ctypes.data
    t, own = c.pca_transform(x, means, comps, own_means=True, center="copy")
    a = rec.calls[-1]
    assert a[6] is None and a[11] == L.PCA_CENTER_COPY | L.PCA_APPLY_OWN_MEANS and own.shape == (1, 5) and a[15] == own.ctypes.data
    t, q, own = c.pca_transform(x, None, comps, own_means=True, residuals=True)
    assert rec.calls[-1][11] == L.PCA_APPLY_OWN_MEANS and rec.calls[-1][14] == q.ctypes.data
    c.pca_transform(x, None, comps)                      # no means: no centring
    assert rec.calls[-1][6] is None and rec.calls[-1][11] == 0
    # a column-major view passes its strides on: the library, not Python, decides on the repack
    c.pca_transform(np.asfortranarray(x), means, comps)
    assert rec.calls[-1][2:6] == (12, 5, 1, 12)
    assert names == ["corrla_pca_transform_" + ("f32" if dtype == np.float32 else "f64")] * 6


def test_a_sparse_target_takes_the_csr_entry(stub):
    c, rec, names = stub
    data, idx, ptr = np.array([1.0, 2.0, 3.0]), np.array([0, 2, 1], dtype=np.int32), np.array([0, 2, 2, 3], dtype=np.int64)
    t = c.pca_transform((data, idx, ptr, (3, 4)), np.zeros(4), np.ones((2, 4)), np.ones(4))
    a = rec.calls[-1]
    # (ctx, values, col_idx, row_ptr, m, n, nnz, means, scales, components, ldc, k, flags, scores, ld_scores, resid_out, means_out)
    assert names == ["corrla_pca_transform_csr_f64"] and len(a) == 17 and a[4:7] == (3, 4, 3)
    assert a[7] is not None and a[8] is not None and a[10:13] == (2, 2, 0) and a[15] is None and t.shape == (3, 2)
    with pytest.raises(ValueError, match="residuals=True on sparse input"):
        c.pca_transform((data, idx, ptr, (3, 4)), np.zeros(4), np.ones((2, 4)), residuals=True)
    with pytest.raises(ValueError, match="center='copy' on sparse input"):
        c.pca_transform((data, idx, ptr, (3, 4)), np.zeros(4), np.ones((2, 4)), center="copy")
    assert len(rec.calls) == 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_inverse_builds_its_call(stub, dtype):
    c, rec, names = stub
    t = np.arange(24, dtype=dtype).reshape(12, 2)
    comps = np.arange(10.0).reshape(2, 5)
    rec.peek = {1: (C.c_float if dtype == np.float32 else C.c_double, 24)}
    out = c.pca_inverse_transform(t, np.arange(5.0), comps)
    rec.peek = {}
    a = rec.calls[-1]
    # (ctx, scores, m, k, ld_scores, means, scales, components, ldc, n, out, row_stride_out)
    assert len(a) == 12 and a[2:5] == (12, 2, 12) and a[5] is not None and a[6] is None and a[8:10] == (2, 5)
    assert a[10] == out.ctypes.data and a[11] == 5 and out.shape == (12, 5) and out.dtype == dtype and out.flags.c_contiguous
    assert np.array_equal(rec.seen[1], t.ravel(order="F"))       # column-major with ld = m
    tf = np.asfortranarray(t)
    c.pca_inverse_transform(tf, None, comps, np.ones(5))
    assert rec.calls[-1][1] == tf.ctypes.data and rec.calls[-1][5] is None and rec.calls[-1][6] is not None   # no copy of F-ordered scores
    assert names == ["corrla_pca_inverse_" + ("f32" if dtype == np.float32 else "f64")] * 2


def test_every_bad_argument_raises_before_the_library_is_touched(stub):
    c, rec, _ = stub
    x, means, comps = np.zeros((6, 3)), np.zeros(3), np.ones((2, 3))
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="own_means must be True or False"):
            c.pca_transform(x, means, comps, own_means=bad)
        with pytest.raises(ValueError, match="residuals must be True or False"):
            c.pca_transform(x, means, comps, residuals=bad)
    with pytest.raises(ValueError, match="center must be"):
        c.pca_transform(x, means, comps, center="both")
    with pytest.raises(ValueError, match="2-D"):
        c.pca_transform(np.zeros(5), means, comps)
    with pytest.raises(ValueError, match="non-empty"):
        c.pca_transform(np.zeros((0, 3)), means, comps)
    with pytest.raises(ValueError, match=r"components must have shape \(k, 3\)"):
        c.pca_transform(x, means, np.ones((2, 4)))
    with pytest.raises(ValueError, match="components must have shape"):
        c.pca_transform(x, means, np.ones(3))
    with pytest.raises(ValueError, match="between 1 and n = 3 rows"):
        c.pca_transform(x, means, np.ones((4, 3)))
    with pytest.raises(ValueError, match="components must be given"):
        c.pca_transform(x, means, None)
    with pytest.raises(ValueError, match="means must have 3 entries"):
        c.pca_transform(x, np.zeros(4), comps)
    with pytest.raises(ValueError, match="scales must have 3 entries"):
        c.pca_transform(x, means, comps, np.ones(2))
    with pytest.raises(TypeError):
        c.pca_transform(x, means, comps, None, True)            # the switches are keyword-only
    with pytest.raises(ValueError, match="scores have 3 columns, components 2 rows"):
        c.pca_inverse_transform(np.zeros((6, 3)), means, comps)
    with pytest.raises(ValueError, match="non-empty"):
        c.pca_inverse_transform(np.zeros((0, 2)), means, comps)
    with pytest.raises(ValueError, match="means must have 3 entries"):
        c.pca_inverse_transform(np.zeros((6, 2)), np.zeros(2), comps)
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match=r"no bfloat16 entry: pass \.float\(\)"):
        c.pca_transform(torch.zeros((4, 3), dtype=torch.bfloat16), means, comps)
    with pytest.raises(ValueError, match=r"no bfloat16 entry"):
        c.pca_inverse_transform(torch.zeros((4, 2), dtype=torch.bfloat16), means, comps)
    assert not rec.calls


EMU_PROBE = r"""
#include "emu_backend.cpp"
using corrla::PcaTransformCall;
using corrla::PcaInverseCall;
using corrla::Span;
#define API extern "C" __attribute__((visibility("default")))
API int probe_transform(const double* x, long long m, long long n, long long rs, long long cs, const double* means, const double* scales,
                        const double* comps, long long ldc, long long k, unsigned long long flags, double* scores, long long ld_scores,
                        double* resid, double* means_out, int sparse) {
  EmuDev dev;
  bool ran = false;
  int st = (int)corrla::guarded([&] {
    const PcaTransformCall<double> c{m, n, means, scales, comps, ldc, k, flags, scores, ld_scores, resid, means_out};
    const Span xr(x, m, n, rs, cs, "x");
    corrla::pca_transform_entry<EmuDev, double>(dev, c, sparse != 0, &xr, 1, [&] { ran = true; });
  });
  return ran ? -1 : st;
}
API int probe_inverse(const double* scores, long long m, long long k, long long ld_scores, const double* means, const double* scales,
                      const double* comps, long long ldc, long long n, double* out, long long rso) {
  EmuDev dev;
  bool ran = false;
  int st = (int)corrla::guarded([&] {
    const PcaInverseCall<double> c{scores, m, k, ld_scores, means, scales, comps, ldc, n, out, rso};
    corrla::pca_inverse_entry<EmuDev, double>(dev, c, [&] { ran = true; });
  });
  return ran ? -1 : st;
}
API const char* probe_error() { return corrla::last_error_slot().c_str(); }
"""


@pytest.fixture(scope="module")
def emu_probe(tmp_path_factory):
    """The emulation backend itself (tests/emu/emu_backend.cpp, unchanged) behind the argument checks of the new entries."""
    tmp = tmp_path_factory.mktemp("pca_apply_probe")
    src = tmp / "probe.cpp"
    src.write_text(EMU_PROBE)
    so = tmp / "libpca_apply_probe.so"
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "emu"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.probe_error.restype = C.c_char_p
    return lib


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class _Model:
    def __init__(self, m=30, n=6, k=3):
        rng = np.random.default_rng(0)
        self.x, self.means, self.scales = rng.standard_normal((m, n)), rng.standard_normal(n), np.ones(n)
        self.comps = np.asfortranarray(rng.standard_normal((k, n)))
        self.scores, self.q, self.means_out, self.out = np.empty((m, k), order="F"), np.empty(m), np.empty(n), np.empty((m, n))
        self.m, self.n, self.k = m, n, k


def _transform(lib, mo, **kw):
    a = dict(x=mo.x, m=mo.m, n=mo.n, means=mo.means, scales=mo.scales, comps=mo.comps, ldc=mo.k, k=mo.k, flags=0, scores=mo.scores,
             ld_scores=mo.m, resid=None, means_out=None, sparse=0)
    a.update(kw)
    LL = C.c_longlong
    rc = lib.probe_transform(_p(a["x"]), LL(a["m"]), LL(a["n"]), LL(mo.x.strides[0] // 8), LL(mo.x.strides[1] // 8), _p(a["means"]),
                             _p(a["scales"]), _p(a["comps"]), LL(a["ldc"]), LL(a["k"]), C.c_ulonglong(a["flags"]), _p(a["scores"]),
                             LL(a["ld_scores"]), _p(a["resid"]), _p(a["means_out"]), C.c_int(a["sparse"]))
    return rc, lib.probe_error()


def _inverse(lib, mo, **kw):
    a = dict(scores=mo.scores, m=mo.m, k=mo.k, ld_scores=mo.m, means=mo.means, scales=mo.scales, comps=mo.comps, ldc=mo.k, n=mo.n,
             out=mo.out, rso=mo.n)
    a.update(kw)
    LL = C.c_longlong
    rc = lib.probe_inverse(_p(a["scores"]), LL(a["m"]), LL(a["k"]), LL(a["ld_scores"]), _p(a["means"]), _p(a["scales"]), _p(a["comps"]),
                           LL(a["ldc"]), LL(a["n"]), _p(a["out"]), LL(a["rso"]))
    return rc, lib.probe_error()


def test_the_emulation_backend_ends_the_calls_with_einval(emu_probe):
    mo = _Model()
    for kw in ({}, dict(resid=mo.q), dict(flags=L.PCA_APPLY_OWN_MEANS, means=None, means_out=mo.means_out), dict(means=None, scales=None)):
        rc, msg = _transform(emu_probe, mo, **kw)
        assert rc == L.EINVAL and b"no PCA back-projection kernel" in msg, (kw, msg)
    rc, msg = _inverse(emu_probe, mo)
    assert rc == L.EINVAL and b"no PCA back-projection kernel" in msg
    rc, msg = _inverse(emu_probe, mo, means=None, scales=None)
    assert rc == L.EINVAL and b"no PCA back-projection kernel" in msg


def test_argument_checks_of_the_entries(emu_probe):
    """EINVAL with a message that names the argument, on every backend, before the backend is asked for anything"""
    mo = _Model()
    for kw, word in ((dict(m=0), b"m and n"), (dict(n=0), b"m and n"), (dict(k=0), b"k must be in [1, n]"), (dict(k=7, ldc=7), b"k must be in [1, n]"),
                     (dict(comps=None), b"components is NULL"), (dict(scores=None), b"scores is NULL"), (dict(ldc=2), b"ldc < k"),
                     (dict(ld_scores=29), b"ld_scores < m"),
                     (dict(flags=L.PCA_CENTER_FUSED | L.PCA_CENTER_COPY), b"mutually exclusive"), (dict(flags=0x8), b"unknown flag"),
                     (dict(sparse=1, resid=mo.q), b"resid_out must be NULL"), (dict(sparse=1, flags=L.PCA_CENTER_COPY), b"densify"),
                     (dict(scores=mo.x), b"scores overlaps x"), (dict(resid=mo.means), b"resid_out overlaps means"),
                     (dict(resid=mo.scores[:, 0]), b"scores overlaps resid_out"),
                     (dict(flags=L.PCA_APPLY_OWN_MEANS, means_out=mo.scales), b"means_out overlaps scales")):
        rc, msg = _transform(emu_probe, mo, **kw)
        assert rc == L.EINVAL and word in msg, (kw, msg)
    # with own means, `means` is ignored: it may even be the output
    rc, msg = _transform(emu_probe, mo, flags=L.PCA_APPLY_OWN_MEANS, means=mo.means_out, means_out=mo.means_out)
    assert rc == L.EINVAL and b"no PCA back-projection kernel" in msg
    for kw, word in ((dict(m=0), b"m and n"), (dict(k=0), b"k must be in [1, n]"), (dict(k=7, ldc=7), b"k must be in [1, n]"),
                     (dict(scores=None), b"scores is NULL"), (dict(comps=None), b"components is NULL"), (dict(out=None), b"out is NULL"),
                     (dict(ldc=2), b"ldc < k"), (dict(ld_scores=29), b"ld_scores < m"), (dict(rso=5), b"row_stride_out < n"),
                     (dict(out=mo.means, m=1, n=3, k=3), b"out overlaps means"), (dict(out=mo.scores, m=3, n=3, rso=3), b"out overlaps scores")):
        rc, msg = _inverse(emu_probe, mo, **kw)
        assert rc == L.EINVAL and word in msg, (kw, msg)


def _host_model(dtype, with_scales):
    rng = np.random.default_rng(4)
    p = api.PcaRsvd.__new__(api.PcaRsvd)
    p.pca_rank, p.n_samples, p._ctx = 3, 40, None
    p.means = rng.standard_normal((1, 7)).astype(dtype)
    p.pca_s = np.array([[3.0], [2.0], [1.0]], dtype=dtype)
    p.components_ = np.asfortranarray(rng.standard_normal((3, 7)).astype(dtype))
    p.scales_ = rng.uniform(0.5, 2.0, (1, 7)).astype(dtype) if with_scales else None
    return p, rng


@pytest.mark.parametrize("with_scales", (False, True))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_apply_tr_and_apply_inv_tr_on_numpy_are_bitwise_what_they_were(dtype, with_scales):
    """the formulas are restated here; a host-fitted model given numpy never reaches a Context (there is none to reach)"""
    p, rng = _host_model(dtype, with_scales)
    targ = rng.standard_normal((11, 7))
    t = np.asarray(targ, dtype=dtype)
    tc = t - t.mean(axis=0, keepdims=True)
    if with_scales:
        tc = tc / p.scales_
    want = tc @ p.components_.T
    got = p.apply_tr(targ)
    assert type(got) is np.ndarray and got.dtype == dtype and np.array_equal(got, want)
    red = rng.standard_normal((11, 3))
    back = np.asarray(red, dtype=dtype) @ p.components_
    if with_scales:
        back = back * p.scales_
    back = back + p.means
    got = p.apply_inv_tr(red)
    assert type(got) is np.ndarray and got.dtype == dtype and np.array_equal(got, back)
    assert np.array_equal(p.apply_tr(targ.tolist()), want)            # anything np.asarray takes, as before


def test_the_new_methods_call_the_context_with_the_models_parts():
    p, rng = _host_model(np.float64, True)
    seen = []

    class Ctx:
        def pca_transform(self, x, means, comps, scales=None, **kw):
            seen.append(("t", means is p.means, comps is p.components_, scales is p.scales_, kw))
            return ("scores", "q") if kw.get("residuals") else "scores"

        def pca_inverse_transform(self, t, means, comps, scales=None):
            seen.append(("i", means is p.means, comps is p.components_, scales is p.scales_))
            return "back"
    p._ctx = Ctx()
    x = rng.standard_normal((5, 7))
    assert p.transform(x) == "scores" and p.residuals(x) == "q" and p.inverse_transform(x[:, :3]) == "back"
    assert seen == [("t", True, True, True, {}), ("t", True, True, True, {"residuals": True}), ("i", True, True, True)]
    assert "replicated model" in api.Context.pca_transform.__doc__
