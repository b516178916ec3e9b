"""CSR sparse input, the parts that need no GPU: the ten new C-ABI symbols (header, library, ctypes table), the SpMM /
transposition / validation kernels in the gfx950 code object, the input normaliser `_as_csr`, and the absence of any
CPU compute path behind the new entries."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from corrla_rs_amd import _lib as L
from corrla_rs_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = [f"corrla_{stem}_{suf}" for suf in ("f32", "f64")
               for stem in ("rsvd_csr", "rsvd_csr_dev", "pca_csr", "pca_csr_dev", "spmm_csr_dev")]


@pytest.fixture(scope="module")
def lib():
    B.build_product()
    return L.load()


def test_new_symbols_declared_exported_and_bound(lib):
    assert len(NEW_SYMBOLS) == 10
    hdr = open(os.path.join(ROOT, "include", "corrla_rsvd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), f"{s} is not declared in include/corrla_rsvd.h"
        assert hasattr(lib, s), f"{s} is not exported by the library"
        assert s in L.SIGNATURES, f"{s} has no ctypes signature"
    # index widths of the declaration: int32 column indices, int64 row pointers
    proto = re.search(r"corrla_rsvd_csr_dev_f32\s*\(([^)]*)\)", hdr).group(1)
    assert "const int32_t* col_idx" in proto and "const int64_t* row_ptr" in proto and "const float* values" in proto
    rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bfn %s\(" % s, rs), f"{s} missing from the Rust shim"


def test_device_code_object_holds_the_sparse_kernels():
    lib_path = B.build_product()
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    data = open(lib_path, "rb").read()
    dev = ""
    for mm in re.finditer(b"\x7fELF", data):
        i = mm.start()
        if data[i + 18: i + 20] == b"\xe0\x00":      # e_machine = EM_AMDGPU
            tmp = os.path.join(os.path.dirname(lib_path), "_device_code_object_sparse.tmp")
            with open(tmp, "wb") as f:
                f.write(data[i:])
            dev += subprocess.run([readelf, "-s", "--wide", tmp], capture_output=True, text=True).stdout
            os.remove(tmp)
    assert dev, "no gfx950 code object found in the library"
    kernels = set(re.findall(r"\s(_Z\S+)\.kd\b", dev))
    for name, typed in (("spmm_rows_kernel", True), ("spmm_xt_kernel", True), ("spmm_long_partial_kernel", True),
                        ("spmm_long_reduce_kernel", True), ("csr_transpose_finish_kernel", True),
                        ("csr_radix_hist_kernel", False), ("csr_radix_scatter_kernel", False), ("csr_scan_kernel", False),
                        ("csr_validate_kernel", False), ("csr_long_build_kernel", False)):
        hits = [k for k in kernels if name in k]
        assert hits, f"{name} has no kernel descriptor in the device code"
        if typed:  # both element types
            assert any("IfE" in k for k in hits) and any("IdE" in k for k in hits), (name, hits)


# ---- _as_csr ----------------------------------------------------------------------------------------------------------
def _random_sparse(m, n, density, seed, dtype=np.float64):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    a = sp.random(m, n, density=density, format="csr", random_state=rng, data_rvs=rng.standard_normal).astype(dtype)
    a.sort_indices()
    return a


def test_as_csr_accepts_every_form_and_gives_identical_arrays():
    import torch
    from corrla_rs_amd.api import _as_csr
    a = _random_sparse(37, 23, 0.2, 1)
    forms = {
        "csr": a,
        "csc": a.tocsc(),
        "coo": a.tocoo(),
        "tuple": (a.data, a.indices, a.indptr, a.shape),
        "torch": torch.sparse_csr_tensor(torch.from_numpy(a.indptr.astype(np.int64)), torch.from_numpy(a.indices.astype(np.int64)),
                                         torch.from_numpy(a.data), size=a.shape),
    }
    ref = None
    for name, f in forms.items():
        vals, ci, rp, shape, on_dev = _as_csr(f)
        assert not on_dev and shape == (37, 23), name
        assert vals.dtype == np.float64 and ci.dtype == np.int32 and rp.dtype == np.int64, name
        assert vals.flags.c_contiguous and ci.flags.c_contiguous and rp.flags.c_contiguous
        if ref is None:
            ref = (vals, ci, rp)
        else:
            assert np.array_equal(vals, ref[0]) and np.array_equal(ci, ref[1]) and np.array_equal(rp, ref[2]), name
    dense = np.zeros((37, 23))
    for r in range(37):
        for q in range(ref[2][r], ref[2][r + 1]):
            dense[r, ref[1][q]] += ref[0][q]
    assert np.array_equal(dense, a.toarray())


def test_as_csr_dtype_and_index_width_conversion():
    from corrla_rs_amd.api import _as_csr
    a = _random_sparse(12, 9, 0.3, 2)
    v32, ci, rp, _, _ = _as_csr((a.data.astype(np.float32), a.indices.astype(np.int64), a.indptr.astype(np.int32), a.shape))
    assert v32.dtype == np.float32 and ci.dtype == np.int32 and rp.dtype == np.int64
    assert np.array_equal(ci, a.indices) and np.array_equal(rp, a.indptr)
    for other in (np.float16, np.int32, np.int64, np.longdouble):
        v, _, _, _, _ = _as_csr((a.data.astype(other), a.indices, a.indptr, a.shape))
        assert v.dtype == np.float64
    assert _as_csr(a.astype(np.float32))[0].dtype == np.float32
    # an index that does not fit int32 must not wrap into range
    big = np.array([0, 2 ** 32 + 1], dtype=np.int64)
    _, ci, _, _, _ = _as_csr((np.ones(2), big, np.array([0, 2]), (1, 9)))
    assert ci[0] == 0 and not (0 <= ci[1] < 9)


def test_as_csr_rejects_malformed_inputs():
    from corrla_rs_amd.api import _as_csr
    a = _random_sparse(12, 9, 0.3, 3)
    with pytest.raises(ValueError):
        _as_csr((a.data, a.indices, a.indptr, (12,)))                 # not 2-D
    with pytest.raises(ValueError):
        _as_csr((a.data, a.indices, a.indptr, (2, 6, 9)))             # not 2-D
    with pytest.raises(ValueError):
        _as_csr((a.data, a.indices, a.indptr[:-1], a.shape))          # indptr length
    with pytest.raises(ValueError):
        _as_csr((a.data, a.indices, a.indptr, (11, 9)))               # shape does not match indptr
    with pytest.raises(ValueError):
        _as_csr((a.data[:-1], a.indices, a.indptr, a.shape))          # data / indices lengths
    with pytest.raises(ValueError):
        _as_csr((a.data.reshape(1, -1), a.indices, a.indptr, a.shape))
    with pytest.raises(ValueError):
        _as_csr((a.data, a.indices, a.indptr))                        # not a 4-tuple
    with pytest.raises(TypeError):
        _as_csr(np.ones((3, 3)))


def test_dense_inputs_that_look_like_tuples_stay_dense():
    """only (three 1-D arrays, length-2 shape) with consistent lengths is a CSR tuple; a dense matrix given as a tuple of
    four rows keeps going through np.asarray"""
    from corrla_rs_amd.api import _is_sparse
    a = _random_sparse(12, 9, 0.3, 5)
    assert _is_sparse((a.data, a.indices, a.indptr, a.shape))
    assert _is_sparse((list(a.data), list(a.indices), list(a.indptr), list(a.shape)))
    assert not _is_sparse(((1, 2), (3, 4), (5, 6), (7, 8)))
    assert not _is_sparse(((1.0, 2.0, 3.0), (4.0, 5.0, 6.0), (7.0, 8.0, 9.0), (1.0, 1.0, 1.0)))
    assert not _is_sparse((np.ones((2, 2)),) * 4)
    assert not _is_sparse(np.ones((4, 2))) and not _is_sparse([[1, 2], [3, 4]])


def test_sparse_dispatch_needs_no_scipy_import():
    """scipy stays optional: the module never imports it (inputs are duck-typed through .tocsr())."""
    src = open(os.path.join(ROOT, "corrla_rs_amd", "api.py")).read()
    assert not re.search(r"^\s*(import|from)\s+scipy", src, flags=re.M)
    for banned in ("rocsparse", "hipsparse", "rocblas"):
        for f in os.listdir(os.path.join(ROOT, "corrla_rs_amd", "csrc")):
            assert banned not in open(os.path.join(ROOT, "corrla_rs_amd", "csrc", f)).read().lower(), (banned, f)


def test_new_entries_have_no_cpu_path(lib):
    """NULL context -> CORRLA_EINVAL from every new compute entry: nothing is computed on the CPU."""
    a = _random_sparse(6, 4, 0.5, 4)
    rp = a.indptr.astype(np.int64)
    ci = a.indices.astype(np.int32)
    for suf, dt in (("f32", np.float32), ("f64", np.float64)):
        v = a.data.astype(dt)
        u = np.full((6, 2), 7.0, dtype=dt, order="F")
        s = np.full((2, 1), 7.0, dtype=dt)
        vt = np.full((2, 4), 7.0, dtype=dt, order="F")
        mu = np.full((1, 4), 7.0, dtype=dt)
        for dev in ("", "_dev"):
            rc = getattr(lib, f"corrla_rsvd_csr{dev}_{suf}")(None, v.ctypes.data, ci.ctypes.data, rp.ctypes.data, 6, 4, a.nnz, 2, 1, 1,
                                                            None, u.ctypes.data, 6, s.ctypes.data, vt.ctypes.data, 2)
            assert rc == L.EINVAL
            rc = getattr(lib, f"corrla_pca_csr{dev}_{suf}")(None, v.ctypes.data, ci.ctypes.data, rp.ctypes.data, 6, 4, a.nnz, 2, 1, 1,
                                                           None, mu.ctypes.data, s.ctypes.data, vt.ctypes.data, 2)
            assert rc == L.EINVAL
        rc = getattr(lib, f"corrla_spmm_csr_dev_{suf}")(None, 0, v.ctypes.data, ci.ctypes.data, rp.ctypes.data, 6, 4, a.nnz,
                                                        vt.ctypes.data, 4, 2, 1.0, u.ctypes.data, 6)
        assert rc == L.EINVAL
        assert b"ctx is NULL" in lib.corrla_last_error()
        for out in (u, s, vt, mu):
            assert np.all(out == 7.0)  # nothing was written
    if lib.corrla_device_count() == 0:
        import corrla_rs_amd as cr
        with pytest.raises(L.CorrlaError):
            cr.Context(0)
