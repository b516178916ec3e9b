"""Host-side behaviour of PCA on standardised columns (corrla_rs_amd/api.py, _lib.py), no GPU needed: the flag and the
options field mirror the header, standardize=True sets the flag and returns four items, standardize=False builds exactly
the call it built before, and PcaRsvd's two projections honour ``scales_``."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from corrla_rs_amd import _lib as L
from corrla_rs_amd import api
from tests.api_stub import make_stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_equals_the_headers_value():
    hdr = open(os.path.join(ROOT, "include", "corrla_rsvd.h")).read()
    m = re.search(r"#define CORRLA_PCA_STANDARDIZE (0x[0-9a-fA-F]+)u\b", hdr)
    assert m and int(m.group(1), 16) == L.PCA_STANDARDIZE == 0x200
    others = (L.OMEGA_ON_DEVICE, L.PCA_CENTER_FUSED, L.PCA_CENTER_COPY, L.QR_HOUSEHOLDER, L.SEED_EXPLICIT, L.POWER_FUSED,
              L.SHARD_COLS, L.SKETCH_BF16X3, L.SKETCH_BF16X6)
    assert all(L.PCA_STANDARDIZE & f == 0 for f in others)


def test_opts_ends_in_scales_out_behind_the_first_layout():
    names = [f for f, _ in L.Opts._fields_]
    assert names[-1] == "scales_out" and names[:5] == ["struct_size", "flags", "seed", "omega", "omega_ld"]
    assert L.Opts.scales_out.offset == 32           # the layout through omega_ld is what struct_size == 32 names
    assert C.sizeof(L.Opts) == 40


@pytest.fixture
def stub():
    return make_stub()


def _opts_of(call):
    """the corrla_opts a recorded PCA call passed (None for NULL); operand (x, m, n, rs, cs) -> opts is argument 9"""
    o = call[9]
    return None if o is None else o._obj


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_standardize_true_sets_the_flag_and_returns_four_items(stub, dtype):
    c, rec, names = stub
    x = np.arange(60, dtype=dtype).reshape(12, 5)
    out = c.pca(x, 2, seed=3, standardize=True)
    assert len(out) == 4 and len(rec.calls) == 1 and names == ["corrla_pca_" + ("f32" if dtype == np.float32 else "f64")]
    means, s, comps, scales = out
    assert scales.shape == (1, 5) == means.shape and scales.dtype == means.dtype == dtype and type(scales) is type(means)
    o = _opts_of(rec.calls[0])
    assert o.flags & L.PCA_STANDARDIZE and o.flags & L.SEED_EXPLICIT and o.struct_size == C.sizeof(L.Opts)
    assert o.scales_out == scales.ctypes.data
    # with a centring mode, and without a seed: the flag alone makes the options block
    c.pca(x, 2, center="fused", standardize=True)
    o = _opts_of(rec.calls[1])
    assert o.flags == (L.PCA_STANDARDIZE | L.PCA_CENTER_FUSED) and o.seed == 0


def test_standardize_false_builds_exactly_todays_call(stub):
    c, rec, names = stub
    x = np.arange(60, dtype=np.float64).reshape(12, 5)
    for kw in ({}, {"standardize": False}):
        assert len(c.pca(x, 2, **kw)) == 3
        assert len(c.pca(x, 2, seed=3, center="copy", **kw)) == 3
    a, b, a2, b2 = rec.calls
    assert _opts_of(a) is None and _opts_of(a2) is None             # no seed, no Omega, no flags: NULL opts as before
    for call in (b, b2):
        o = _opts_of(call)
        assert o.flags == (L.SEED_EXPLICIT | L.PCA_CENTER_COPY) and o.seed == 3 and not o.scales_out
    assert len(a) == len(a2) == 14 and a[1:9] == a2[1:9] and a[-1] == a2[-1]   # same operand, rank, iterations, ldc
    assert names == ["corrla_pca_f64"] * 4


def test_sparse_input_takes_the_flag_too(stub):
    c, rec, names = stub
    data, idx, ptr = np.array([1.0, 2.0, 3.0]), np.array([0, 1, 0], dtype=np.int32), np.array([0, 1, 2, 3, 3], dtype=np.int64)
    out = c.pca((data, idx, ptr, (4, 2)), 1, standardize=True)
    assert len(out) == 4 and names == ["corrla_pca_csr_f64"]
    o = rec.calls[0][10]._obj                                        # (values, col_idx, row_ptr, m, n, nnz) -> opts is argument 10
    assert o.flags == (L.PCA_STANDARDIZE | L.PCA_CENTER_FUSED)


def test_a_non_bool_standardize_raises_before_the_library_is_touched(stub):
    c, rec, _ = stub
    x = np.zeros((6, 3))
    for bad in (1, 0, "yes", None, 1.0, np.ones(3)):
        with pytest.raises(TypeError, match="standardize must be True or False"):
            c.pca(x, 1, standardize=bad)
        with pytest.raises(TypeError, match="standardize must be True or False"):
            api.rpca(x, 1, ctx=c, standardize=bad)
        with pytest.raises(TypeError, match="standardize must be True or False"):
            api.PcaRsvd(x, 1, ctx=c, standardize=bad)
    assert not rec.calls


def test_rpca_and_pcarsvd_pass_the_switch_on(stub):
    c, rec, _ = stub
    x = np.arange(40, dtype=np.float64).reshape(10, 4)
    assert len(api.rpca(x, 2, ctx=c, standardize=True)) == 2
    assert _opts_of(rec.calls[-1]).flags & L.PCA_STANDARDIZE
    assert len(api.rpca(x, 2, ctx=c)) == 2 and _opts_of(rec.calls[-1]) is None
    p = api.PcaRsvd(x, 2, ctx=c, standardize=True)
    assert p.scales_ is not None and p.scales_.shape == (1, 4) and _opts_of(rec.calls[-1]).flags & L.PCA_STANDARDIZE
    assert api.PcaRsvd(x, 2, ctx=c).scales_ is None and _opts_of(rec.calls[-1]) is None


def test_pcarsvd_projections_round_trip_a_standardised_matrix_on_hand_made_factors():
    """apply_tr divides the centred target by scales_, apply_inv_tr multiplies by it before adding the means: with a full
    orthonormal basis as components the round trip gives the matrix back, and the reduced coordinates are those of the
    explicitly standardised matrix."""
    rng = np.random.default_rng(5)
    n = 6
    x = rng.standard_normal((40, n)) * np.logspace(-3, 3, n) + rng.standard_normal((1, n)) * np.logspace(-2, 3, n)
    p = api.PcaRsvd.__new__(api.PcaRsvd)
    p.pca_rank, p.n_samples = n, 40
    p.means = x.mean(axis=0, keepdims=True)
    p.scales_ = x.std(axis=0, ddof=1, keepdims=True)
    p.components_ = np.linalg.qr(rng.standard_normal((n, n)))[0].T
    p.pca_s = np.ones((n, 1))
    red = p.apply_tr(x)
    z = (x - p.means) / p.scales_
    assert np.allclose(red, z @ p.components_.T, rtol=1e-12, atol=1e-12)
    assert np.allclose(p.apply_inv_tr(red), x, rtol=1e-10, atol=0)
    # unstandardised: scales_ is None and nothing is divided
    p.scales_ = None
    assert np.allclose(p.apply_tr(x), (x - p.means) @ p.components_.T, rtol=1e-12, atol=1e-9)
    assert np.allclose(p.apply_inv_tr(p.apply_tr(x)), x, rtol=1e-10, atol=1e-9)
    assert np.array_equal(p.explained_var(), p.pca_s * p.pca_s / 39.0)


def test_the_emulation_backend_refuses_a_standardised_call():
    """The host emulation backend has no column-variance kernels: CORRLA_PCA_STANDARDIZE ends with EINVAL and a message
    there -- on the sample-sharded entry too -- and on an entry that is not a PCA it is EINVAL on every backend."""
    from tests import emu_harness as H
    e = H.emu()
    x = np.random.default_rng(0).standard_normal((30, 6))
    o = L.Opts()
    o.struct_size = C.sizeof(L.Opts)
    o.flags = L.PCA_STANDARDIZE
    means, s, comps = np.empty((1, 6)), np.empty((2, 1)), np.empty((2, 6), order="F")
    i64 = C.c_int64
    for name in ("corrla_emu_pca_f64", "corrla_emu_pca_sharded_f64"):
        rc = getattr(e, name)(C.c_void_p(x.ctypes.data), i64(30), i64(6), i64(6), i64(1), i64(2), i64(2), i64(3), C.byref(o),
                              C.c_void_p(means.ctypes.data), C.c_void_p(s.ctypes.data), C.c_void_p(comps.ctypes.data), i64(2))
        assert rc == L.EINVAL and b"CORRLA_PCA_STANDARDIZE" in e.corrla_emu_last_error()
    u, vt = np.empty((30, 2), order="F"), np.empty((2, 6), order="F")
    passes = C.c_int(0)
    rc = e.corrla_emu_rsvd_f64(C.c_void_p(x.ctypes.data), i64(30), i64(6), i64(6), i64(1), i64(2), i64(2), i64(3), C.byref(o),
                               C.c_void_p(u.ctypes.data), i64(30), C.c_void_p(s.ctypes.data), C.c_void_p(vt.ctypes.data), i64(2),
                               C.byref(passes))
    assert rc == L.EINVAL and b"corrla_pca_" in e.corrla_emu_last_error()
    # the first layout of the options block (32 bytes, no scales_out) is accepted; any other size is not
    o.flags = 0
    o.struct_size = 32
    o.seed = 7
    assert getattr(e, "corrla_emu_pca_f64")(C.c_void_p(x.ctypes.data), i64(30), i64(6), i64(6), i64(1), i64(2), i64(2), i64(3), C.byref(o),
                                            C.c_void_p(means.ctypes.data), C.c_void_p(s.ctypes.data), C.c_void_p(comps.ctypes.data),
                                            i64(2)) == L.OK
    for bad in (0, 24, 36, 48):
        o.struct_size = bad
        assert getattr(e, "corrla_emu_pca_f64")(C.c_void_p(x.ctypes.data), i64(30), i64(6), i64(6), i64(1), i64(2), i64(2), i64(3),
                                                C.byref(o), C.c_void_p(means.ctypes.data), C.c_void_p(s.ctypes.data),
                                                C.c_void_p(comps.ctypes.data), i64(2)) == L.EINVAL
