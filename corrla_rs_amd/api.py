"""Host-side mirror of the reference's RSVD surfaces over the HIP library.

  rsvd(a_mat, n_rank, n_iters, n_oversamples)        <- corrla_rs.rsvd, src/lib_math_utils_py.rs:21-36
  random_svd(a_mat, omega_rank, n_iter, n_oversamples) <- random_svd.rs:63-66 (Rust name / argument names)
  power_iter(a_mat, omega_rank, n_iter)              <- random_svd.rs:15-18

Same positional order (rank, iters, oversamples), same return shapes: U (m, k), S (k, 1) -- a 2-D
column, not 1-D -- and Vt (k, n), column-major in memory like the reference's owned faer `Mat`s
(numpy: F-ordered).  Additive, keyword-only: `seed`, `omega` (shared sketch, the parity-test hook),
`ctx`.  numpy inputs take the host-pointer entry points (H2D + D2H around the device path); torch
CUDA tensors take the device-pointer entry points and return torch tensors on the same device.
float32 input runs the f32 path (the pyo3 surface is f64-only; anything that is not f32 is
converted to f64, as PyReadonlyArray2<f64> extraction would require).  torch.bfloat16 tensors are the
exception: they stay as they are and take the corrla_*_bf16 entries (float32 results; see _as_dense).
"""
import atexit
import ctypes as C
import sys
import threading
import weakref

import numpy as np

from . import _lib as L

__all__ = ["Context", "default_context", "rsvd", "random_svd", "power_iter", "rpca", "PcaRsvd", "algorithmic_flops"]


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _is_torch_csr(x):
    return _is_torch(x) and str(getattr(x, "layout", "")) == "torch.sparse_csr"


def _is_sparse(x):
    """True for what _as_csr takes: a scipy sparse matrix / array (duck-typed), a torch.sparse_csr tensor, or an explicit
    (data, indices, indptr, shape) tuple."""
    if isinstance(x, tuple):
        # (data, indices, indptr, shape): three 1-D arrays and a length-2 shape.  Anything else that happens to be a
        # 4-tuple (a dense matrix given as four rows) stays a dense input.
        def nd(v):
            return v.ndim if hasattr(v, "ndim") else np.ndim(v)
        if len(x) != 4 or not all(nd(v) == 1 for v in x[:3]):
            return False
        shp = x[3]
        if not (isinstance(shp, (tuple, list)) and len(shp) == 2 and all(nd(d) == 0 for d in shp)):
            return False
        try:  # ... consistent with each other (a 4 x 2 dense matrix has the same outline but not these lengths)
            return len(x[0]) == len(x[1]) and len(x[2]) == int(shp[0]) + 1
        except (TypeError, ValueError):
            return False
    if _is_torch(x):
        return _is_torch_csr(x)
    return hasattr(x, "tocsr") and hasattr(x, "nnz") and not isinstance(x, np.ndarray)


def _as_csr(x):
    """The one normaliser of sparse inputs -> (values, int32 col_idx, int64 row_ptr, (m, n), on_device).

    scipy sparse matrices / arrays of any format (through ``.tocsr()``; scipy itself is never imported), CPU
    ``torch.sparse_csr`` tensors and ``(data, indices, indptr, shape)`` tuples give C-contiguous numpy arrays
    (on_device False); a CUDA ``torch.sparse_csr`` tensor gives torch tensors on its device (on_device True) and the
    matrix is never copied to the host.  float32 values stay float32, everything else becomes float64 -- as for dense
    inputs.  Column indices within a row may be unsorted; duplicates add."""
    if _is_torch_csr(x):
        if x.dim() != 2:
            raise ValueError("sparse input must be 2-D")
        shape = tuple(int(d) for d in x.shape)
        vals, ci, rp = x.values(), x.col_indices(), x.crow_indices()
        if x.is_cuda:
            import torch
            if vals.dtype != torch.float32:
                vals = vals.to(torch.float64)
            m, n = shape
            if rp.numel() != m + 1 or ci.numel() != vals.numel():
                raise ValueError("inconsistent CSR arrays")
            if ci.dtype != torch.int32:
                # as on the host: an index that does not fit int32 must stay out of range, not wrap into it
                ci = torch.where((ci < 0) | (ci >= 2 ** 31), torch.full_like(ci, -1), ci).to(torch.int32)
            return vals.contiguous(), ci.contiguous(), rp.to(torch.int64).contiguous(), shape, True
        data, indices, indptr = vals.detach().numpy(), ci.numpy(), rp.numpy()
    elif isinstance(x, tuple):
        if len(x) != 4:
            raise ValueError("a CSR tuple is (data, indices, indptr, shape)")
        data, indices, indptr, shape = x
        shape = tuple(shape) if np.ndim(shape) == 1 else (shape,)
    elif hasattr(x, "tocsr"):
        if getattr(x, "ndim", 2) != 2:
            raise ValueError("sparse input must be 2-D")
        c = x.tocsr()
        data, indices, indptr, shape = c.data, c.indices, c.indptr, tuple(c.shape)
    else:
        raise TypeError("not a sparse matrix: expected scipy sparse, torch.sparse_csr or (data, indices, indptr, shape)")
    if len(shape) != 2:
        raise ValueError("sparse input must be 2-D")
    m, n = int(shape[0]), int(shape[1])
    data = np.asarray(data)
    if data.dtype != np.float32:
        data = data.astype(np.float64, copy=False)
    indices, indptr = np.asarray(indices), np.asarray(indptr)
    if data.ndim != 1 or indices.ndim != 1 or indptr.ndim != 1:
        raise ValueError("data, indices and indptr must be 1-D")
    if indptr.shape[0] != m + 1:
        raise ValueError(f"indptr has {indptr.shape[0]} entries, shape {(m, n)} needs {m + 1}")
    if indices.shape[0] != data.shape[0]:
        raise ValueError("data and indices differ in length")
    if m < 0 or n < 0 or n >= 2 ** 31 or m >= 2 ** 31:
        raise ValueError("shape out of range")
    if indices.dtype != np.int32:
        # a value that does not fit int32 cannot be a column index below 2^31: keep it out of range instead of wrapping
        wide = indices.astype(np.int64, copy=False)
        indices = np.where((wide < 0) | (wide >= 2 ** 31), -1, wide).astype(np.int32)
    indptr = indptr.astype(np.int64, copy=False)
    return np.ascontiguousarray(data), np.ascontiguousarray(indices), np.ascontiguousarray(indptr), (m, n), False


def _suffix(dtype):
    """Symbol suffix of a numpy or torch dtype (inputs are float32, float64 or torch.bfloat16 by the time they get here)."""
    name = str(dtype)
    if name.endswith("bfloat16"):
        return "bf16"
    return "f32" if name.endswith("float32") else "f64"


def _is_bf16(x):
    return _is_torch(x) and str(x.dtype) == "torch.bfloat16"


def _reject_bf16(x, what):
    """Surfaces without a bf16 entry say so: widening silently would quadruple the caller's memory behind their back."""
    if _is_bf16(x):
        raise ValueError(f"{what} has no bfloat16 entry: pass .float() (or use rsvd / pca, which take bfloat16 tensors)")


def _f32_like(a):
    """An empty float32 array of the kind and device of `a`: what the outputs of a bf16 call are modelled on.  A CPU
    tensor gives numpy outputs, as every host input does."""
    if _is_torch(a) and a.is_cuda:
        import torch
        return torch.empty(0, dtype=torch.float32, device=a.device)
    return np.empty(0, dtype=np.float32)


def _check_bool(name, v, exc):
    """a switch is a switch: anything but a bool (a tolerance, a vector of scales, "yes") is a mistake, not a truth value"""
    if not isinstance(v, (bool, np.bool_)):
        raise exc(f"{name} must be True or False, got {type(v).__name__}")
    return bool(v)


def _check_standardize(v):
    return _check_bool("standardize", v, TypeError)


def _ptr(t):
    return t.data_ptr() if _is_torch(t) else t.ctypes.data


def _c_args(operand):
    """The C arguments of an operand description: its arrays as pointers, its integers as they are.  The description
    itself holds the arrays, so they outlive the call."""
    return [v if isinstance(v, int) else _ptr(v) for v in operand]


def _as_dense(x, what):
    """The one normaliser of dense inputs -> (array, on_device): a torch CUDA tensor stays on its device, everything else
    becomes a numpy array without negative strides (torch has none).  float32 stays float32, the rest becomes float64.
    A torch.bfloat16 tensor is kept as it is, never widened here: on its device for a CUDA tensor, as the CPU tensor
    (numpy has no bfloat16) for the host entries."""
    if _is_bf16(x):
        if x.dim() != 2:
            raise ValueError(f"{what} must be 2-D")
        return x.detach(), bool(x.is_cuda)
    if _is_torch(x) and x.is_cuda:
        import torch
        if x.dim() != 2:
            raise ValueError(f"{what} must be 2-D")
        return (x if x.dtype in (torch.float32, torch.float64) else x.to(torch.float64)), True
    a = np.asarray(x.detach().cpu().numpy() if _is_torch(x) else x)
    if a.ndim != 2:
        raise ValueError(f"{what} must be 2-D")
    if a.dtype != np.float32:
        a = a.astype(np.float64, copy=False)
    if any(st < 0 for st in a.strides):
        a = np.ascontiguousarray(a)
    return a, False


def _strides(a):
    """(row, column) strides in elements."""
    return tuple(a.stride()) if _is_torch(a) else (a.strides[0] // a.itemsize, a.strides[1] // a.itemsize)


def _empty_colmajor(like, rows, cols):
    """Uninitialised (rows, cols) output, column-major like the reference's owned faer `Mat`s, of the array kind, dtype
    and device of `like`: a numpy F-ordered array, or the transpose of a (cols, rows) torch tensor."""
    if _is_torch(like):
        import torch
        return torch.empty((cols, rows), dtype=like.dtype, device=like.device).t()
    return np.empty((rows, cols), dtype=like.dtype, order="F")


def _empty(like, shape, dtype=None):
    """Uninitialised row-major output of `shape`, of the array kind, device and -- unless `dtype`, a numpy dtype, names
    another -- dtype of `like`.  `like` is an array or, for the entries that have none to model on, a device index (a tensor
    on that device) or None (numpy)."""
    if _is_torch(like) or isinstance(like, int):
        import torch
        return torch.empty(shape, dtype=like.dtype if dtype is None else getattr(torch, np.dtype(dtype).name),
                           device=like.device if _is_torch(like) else f"cuda:{like}")
    return np.empty(shape, dtype=like.dtype if dtype is None else dtype)


def _opt_ptr(v):
    """an optional array as the entries take it: NULL for None"""
    return None if v is None else _ptr(v)


def _reject(v, what, sparse):
    """the two kinds of input the statistics entries have no kernels for; `sparse`: what the entry says about the second"""
    _reject_bf16(v, what)
    if _is_sparse(v):
        raise ValueError(sparse)


def _rowmajor(a):
    """`a` as the entries read a matrix: unit stride along the columns, rows that do not overlap; a view with a padded row
    stride stays the view it is."""
    rs, cs = _strides(a)
    if (cs != 1 and a.shape[1] > 1) or (rs < a.shape[1] and a.shape[0] > 1):
        return a.contiguous() if _is_torch(a) else np.ascontiguousarray(a)
    return a


def _row_stride(a):
    """the row stride of what _rowmajor returned (a single row has none: its length serves)"""
    return int(_strides(a)[0]) if a.shape[0] > 1 else int(a.shape[1])


def _poly_terms(k, degree):
    """The columns of ``build_vandermonde`` (stats_corr.rs:201-209) over k features: [x, 1] below degree 2,
    [x, x_a x_b (a <= b), 1] from there on.  Also the rows of the polynomial tail of an RBF interpolant."""
    return k + 1 if degree < 2 else k + k * (k + 1) // 2 + 1


def _rbf_tail(poly_degree, dim):
    """-> (poly_degree as the RBF entries take it: -1 for no tail, the rows of the tail over dim coordinates)"""
    if poly_degree is not None and (isinstance(poly_degree, (bool, np.bool_)) or not isinstance(poly_degree, (int, np.integer))):
        raise ValueError("poly_degree must be None or an integer")
    degree = -1 if poly_degree is None or poly_degree < 0 else int(poly_degree)
    return degree, (0 if degree < 0 else _poly_terms(dim, degree))


# What a corrla_ctx_last_* function reports -> the entries of Context._last that the last_* accessors read.  The out-values
# arrive in the order of the C function's out-parameters.
_RECORDS = {
    "pca_apply": lambda centring, route: {"pca_apply_centring": L.PCA_APPLY_CENTRINGS.get(centring),
                                          "pca_apply_route": L.PCA_APPLY_ROUTES.get(route)},
    "polyfit": lambda route: {"polyfit_route": L.POLYFIT_ROUTES.get(route)},
    "kde": lambda route: {"kde_route": L.KDE_ROUTES.get(route)},
    "mvn": lambda route: {"mvn_route": L.MVN_ROUTES.get(route)},
    "dirichlet": lambda word: {"dirichlet_route": L.DIRICHLET_ROUTES.get(word & 0xFF), "dirichlet_readbacks": word >> 8},
    "solve": lambda route, info, min_pivot, max_u: {"solve_route": L.SOLVE_ROUTES.get(route),
                                                    "solve_info": {"info": info, "min_pivot": min_pivot, "max_u": max_u}},
    "chol": lambda route, info, min_diag, max_diag, logdet: {
        "chol_route": L.CHOL_ROUTES.get(route),
        "chol_info": {"info": info, "min_diag": min_diag, "max_diag": max_diag, "logdet": logdet}},
    "eigh": lambda route, sweeps, off, shift, info: {
        "eigh_route": L.EIGH_ROUTES.get(route),
        "eigh_info": {"info": info, "sweeps": sweeps, "off": off, "shift": shift, "dropped": None}},
}
# The status records: they are valid after a numeric failure too (CORRLA_ENUMERIC), and the device entries that write them
# (LU, Cholesky, RBF fit, eigensolver) synchronise themselves.
_STATUS_RECORDS = ("solve", "chol", "eigh")


def _sync_stream(t):
    """Inputs produced on torch's current stream are complete before the library's own (non-blocking) stream reads them:
    called last before a library call, after every torch operation that prepares an argument."""
    import torch
    torch.cuda.current_stream(t.device).synchronize()


# Contexts own HIP streams / allocations / RCCL communicators: destroy them before the interpreter (and
# the HIP runtime's own static destructors) tear down, never from a late __del__.
_live = weakref.WeakSet()


def _close_all():
    for c in list(_live):
        try:
            c.close()
        except Exception:
            pass


atexit.register(_close_all)


class Context:
    """One device, one stream, one workspace arena (corrla_ctx).  Not thread-parallel: calls on one
    context serialise, as calls on one faer global thread pool do in the reference."""

    def __init__(self, device=0):
        self._lib = L.load()
        h = C.c_void_p()
        L.check(self._lib.corrla_ctx_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        _live.add(self)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.corrla_ctx_destroy(h)

    def __del__(self):
        if sys is None or sys.is_finalizing():
            return  # too late to touch the HIP runtime; atexit already closed live contexts
        try:
            self.close()
        except Exception:
            pass

    # ---- communicator ------------------------------------------------------------------
    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(L.UNIQUE_ID_BYTES)
        L.check(L.load().corrla_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id, rank, nranks):
        buf = C.create_string_buffer(bytes(unique_id), L.UNIQUE_ID_BYTES)
        L.check(self._lib.corrla_ctx_comm_init(self._h, buf, int(rank), int(nranks)))

    def comm_info(self):
        """(rank, nranks) of the context's communicator as RCCL reports them; nranks = 0 without a communicator."""
        r, n = C.c_int(0), C.c_int(0)
        L.check(self._lib.corrla_ctx_comm_info(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def set_phase_timings(self, on):
        """Per-phase device times (hipEvents at the phase boundaries, ~5 us of idle GPU each).  Off: timings() keeps
        total_ms, sketch_kernel_ms and the counters, the phase entries read 0."""
        L.check(self._lib.corrla_ctx_set_phase_timings(self._h, 1 if on else 0))

    def timings(self):
        t = L.Timings()
        L.check(self._lib.corrla_ctx_get_timings(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in t._fields_}

    # ---- helpers -----------------------------------------------------------------------
    @staticmethod
    def _qr_flag(qr):
        """qr=None / "cholesky": the default CholeskyQR2; "householder": Householder TSQR with an explicit thin Q
        (CORRLA_QR_HOUSEHOLDER; the reference's `qr().compute_thin_q()` as written, random_svd.rs:38,57)."""
        if qr in (None, "cholesky"):
            return 0
        if qr == "householder":
            return L.QR_HOUSEHOLDER
        raise ValueError("qr must be None, 'cholesky' or 'householder'")

    @staticmethod
    def _mixed_flag(mixed):
        """mixed=None: exact f32 / f64 products (default).  "bf16x6" / "bf16x3": the tall products of the range finder
        (random_svd.rs:31, 42-51) on the bf16 matrix units with f32 accumulation, every f32 operand split on the fly into
        three / two bf16 pieces (CORRLA_SKETCH_BF16X6 / X3; f32 row-major inputs with l <= 144, ignored elsewhere)."""
        if mixed in (None, False, "f32"):
            return 0
        if mixed == "bf16x6":
            return L.SKETCH_BF16X6
        if mixed == "bf16x3":
            return L.SKETCH_BF16X3
        raise ValueError("mixed must be None, 'bf16x3' or 'bf16x6'")

    def _opts(self, seed, omega, nt, l, dtype, on_device, extra_flags=0):
        if seed is None and omega is None and not extra_flags:
            return None, None
        o = L.Opts()
        o.struct_size = C.sizeof(L.Opts)
        o.seed = int(seed) if seed is not None else 0
        o.flags = int(extra_flags) | (L.SEED_EXPLICIT if seed is not None else 0)   # seed=0 is a real seed
        keep = None
        if omega is not None:
            if on_device:
                import torch
                om = omega if _is_torch(omega) else torch.as_tensor(np.asarray(omega))
                om = om.to(device=f"cuda:{self.device}", dtype=dtype)
                if tuple(om.shape) != (nt, l):
                    raise ValueError(f"omega must have shape {(nt, l)}, got {tuple(om.shape)}")
                keep = om.t().contiguous()  # (l, nt) row-major == (nt, l) column-major
                o.omega = keep.data_ptr()
                o.flags |= L.OMEGA_ON_DEVICE
            else:
                om = np.asarray(omega, dtype=dtype)
                if om.shape != (nt, l):
                    raise ValueError(f"omega must have shape {(nt, l)}, got {om.shape}")
                keep = np.asfortranarray(om)
                o.omega = keep.ctypes.data
            o.omega_ld = nt
        return o, keep

    def _on_my_device(self, t):
        if t.device.index != self.device:
            raise ValueError(f"tensor is on {t.device}, context is on cuda:{self.device}")

    def _csr_operand(self, a):
        """Sparse input -> (operand description of the corrla_*_csr_* entries, m, n, an array of its kind, on_device)."""
        vals, ci, rp, (m, n), on_dev = _as_csr(a)
        if m == 0 or n == 0:
            raise ValueError("a_mat must be non-empty")
        if on_dev:
            self._on_my_device(vals)
        return (vals, ci, rp, m, n, int(vals.shape[0])), m, n, vals, on_dev

    def _entry(self, stem, on_device, dtype):
        return getattr(self._lib, stem + ("dev_" if on_device else "") + _suffix(dtype))

    @property
    def _last(self):
        """How this context's last calls ran, by the names the last_* accessors read: one store for every record, made on
        first use (so that a Context made without __init__ has one too)."""
        return self.__dict__.setdefault("_last_store", {})

    def _read_last(self, record):
        """corrla_ctx_last_<record> into _last: one out-value per POINTER(t) the signature lists after the context."""
        name = "corrla_ctx_last_" + record
        outs = [p._type_() for p in L.SIGNATURES[name][1][1:]]
        L.check(getattr(self._lib, name)(self._h, *[C.byref(v) for v in outs]))
        self._last.update(_RECORDS[record](*[v.value for v in outs]))

    def _call(self, stem, dtype, args, on_device, inputs=None, last=None):
        """What every statistics entry ends with: the call of `stem`[dev_]<dtype>(ctx, *args), and the three ordering rules
        around it, which live here and nowhere else.
        1. `inputs` (a tensor the call reads) were prepared on torch's current stream: that stream is waited for last before
           the call, so after every torch operation that prepared an argument.
        2. A status record (`last` in _STATUS_RECORDS) is read before a failure is raised: it describes a numeric failure too.
        3. A device entry only enqueues, unless it writes a status record: the context is synchronised before torch sees the
           outputs, and before `last`, the corrla_ctx_last_* record of the entry if it has one, is read."""
        status = last in _STATUS_RECORDS
        if on_device and inputs is not None:
            _sync_stream(inputs)
        rc = self._entry(stem, on_device, dtype)(self._h, *args)
        if status and rc in (L.OK, L.ENUMERIC):
            self._read_last(last)
        L.check(rc)
        if not status:
            self._finish(on_device, last)

    def _finish(self, on_device, last):
        """rule 3 of _call, after a call that succeeded"""
        if on_device:
            L.check(self._lib.corrla_ctx_synchronize(self._h))
        if last is not None:
            self._read_last(last)

    def _pca_apply_done(self, on_device):
        """what a caller of the raw transform / inverse entries ends with (tests/test_gpu_pca_apply.py)"""
        self._finish(on_device, "pca_apply")

    def _dense_arg(self, v, name, what, *, sparse=None, like=None, f64=False, nonempty=True, rowmajor=False):
        """The one adapter of the dense matrix argument `name` of the entry `what` -> (array, on_device).  bfloat16 raises, a
        sparse input raises `sparse` (None: the entry has dealt with it).  Then `v` as _as_dense gives it -- 2-D, float32
        as it is and anything else as float64, numpy or a CUDA tensor, which has to be on this context's device -- or, with
        `like`, converted to the kind, device and dtype of that array.  f64: float64 whatever came.  nonempty: neither side
        may be 0.  rowmajor: see _rowmajor."""
        _reject_bf16(v, what)
        if sparse is not None and _is_sparse(v):
            raise ValueError(sparse)
        if like is None:
            a, on_dev = _as_dense(v, name)
            if on_dev:
                self._on_my_device(a)
        else:
            on_dev = _is_torch(like)
            a = self._model_array(v, like, on_dev)
            if a.ndim != 2:
                raise ValueError(f"{name} must be 2-D")
        if f64 and on_dev:
            import torch
            a = a.detach().to(torch.float64)
        elif f64:
            a = a.astype(np.float64, copy=False)
        if nonempty and (a.shape[0] == 0 or a.shape[1] == 0):
            raise ValueError(f"{name} must be non-empty")
        return (_rowmajor(a) if rowmajor else a), on_dev

    def _run_rsvd(self, stem, operand, m, n, nt, like, on_device, k, q, p, seed, omega, flags, in_dtype=None):
        """The one caller of the rsvd entries `stem`[dev_]{f32,f64,bf16}: `operand` describes the m x n matrix (its arrays
        and integer arguments, see _c_args), `like` an array of the kind, dtype and device the outputs and Omega take,
        `in_dtype` the operand's dtype where it differs from theirs (bf16 input: float32 outputs).
        -> (U (m, k), S (k, 1), Vt (k, n))"""
        l = min(k + max(p, 0), nt)
        o, keep = self._opts(seed, omega, nt, l, like.dtype, on_device, flags)
        kk = max(k, 1)
        u, s, vt = (_empty_colmajor(like, *shape) for shape in ((m, kk), (kk, 1), (kk, n)))
        if on_device:
            _sync_stream(like)  # after _opts: the device copy of omega is made on torch's stream too
        L.check(self._entry(stem, on_device, in_dtype or like.dtype)(self._h, *_c_args(operand), k, q, p,
                                                                     C.byref(o) if o is not None else None,
                                                                     _ptr(u), m, _ptr(s), _ptr(vt), kk))
        del keep
        return u, s, vt

    def _run_pca(self, stem, operand, m, n, nt, like, on_device, rank, n_iter, n_oversamples, seed, omega, flags, in_dtype=None,
                 standardize=False):
        """The same for the PCA entries.  -> (means (1, n), S (k, 1), components (k, n)); n_iter / n_oversamples default as
        in pca_rsvd.rs:65-66.  standardize: CORRLA_PCA_STANDARDIZE, and a fourth item, scales (1, n) of the kind of means."""
        q = 20 if n_iter is None else int(n_iter)
        p = min(n, 10) if n_oversamples is None else int(n_oversamples)
        l = min(rank + max(p, 0), nt)
        o, keep = self._opts(seed, omega, nt, l, like.dtype, on_device, flags | (L.PCA_STANDARDIZE if standardize else 0))
        kk = max(rank, 1)
        means, s, comps = (_empty_colmajor(like, *shape) for shape in ((1, n), (kk, 1), (kk, n)))
        if standardize:
            scales = _empty_colmajor(like, 1, n)
            o.scales_out = _ptr(scales)
        if on_device:
            _sync_stream(like)  # after _opts, as in _run_rsvd
        L.check(self._entry(stem, on_device, in_dtype or like.dtype)(self._h, *_c_args(operand), rank, q, p,
                                                                     C.byref(o) if o is not None else None,
                                                                     _ptr(means), _ptr(s), _ptr(comps), kk))
        del keep
        return (means, s, comps, scales) if standardize else (means, s, comps)

    # ---- random_svd ----------------------------------------------------------------------
    def rsvd(self, a_mat, n_rank, n_iters, n_oversamples, *, seed=None, omega=None, qr=None, fused=False, mixed=None):
        """fused=True: CORRLA_POWER_FUSED (one-sweep A^T (A Z) power iteration; f32 row-major inputs with <= 512 columns).
        mixed="bf16x6" | "bf16x3": see _mixed_flag."""
        k, q, p = int(n_rank), int(n_iters), int(n_oversamples)
        if _is_sparse(a_mat):  # fused / mixed have no sparse kernels: ignored, as for every operand outside their domain
            operand, m, n, like, on_dev = self._csr_operand(a_mat)
            return self._run_rsvd("corrla_rsvd_csr_", operand, m, n, min(m, n), like, on_dev, k, q, p, seed, omega, self._qr_flag(qr))
        return self._rsvd_dense(a_mat, k, q, p, seed, omega, qr=qr, fused=fused, mixed=mixed)

    def _rsvd_dense(self, a_mat, k, q, p, seed, omega, sharded=False, qr=None, fused=False, shard_cols=False, mixed=None):
        if sharded:
            _reject_bf16(a_mat, "rsvd_sharded")
        a, on_dev = _as_dense(a_mat, "a_mat")
        if on_dev:
            self._on_my_device(a)
        elif sharded:
            raise ValueError("rsvd_sharded takes torch CUDA tensors")
        m, n = a.shape
        # an EMPTY shard (no rows; no columns with shard="cols") is legal on the sharded entry point: the rank takes part
        # in the collectives with zero contributions and gets a 0-row (0-column) block of the sharded factor
        empty_shard = sharded and ((n == 0 and m > 0) if shard_cols else (m == 0 and n > 0))
        if (m == 0 or n == 0) and not empty_shard:
            raise ValueError("a_mat must be non-empty")
        rs, cs = (max(n, 1), 1) if empty_shard else _strides(a)
        nt = (m if shard_cols else n) if sharded else min(m, n)
        flags = self._qr_flag(qr) | (L.POWER_FUSED if fused else 0) | (L.SHARD_COLS if shard_cols else 0) | self._mixed_flag(mixed)
        if _is_bf16(a):  # float32 outputs and Omega; fused / mixed have no bf16-input kernels and are ignored
            return self._run_rsvd("corrla_rsvd_", (a, m, n, rs, cs), m, n, nt, _f32_like(a), on_dev, k, q, p, seed, omega, flags,
                                  in_dtype=a.dtype)
        return self._run_rsvd("corrla_rsvd_sharded_" if sharded else "corrla_rsvd_", (a, m, n, rs, cs), m, n, nt, a, on_dev,
                              k, q, p, seed, omega, flags)

    def rsvd_sharded(self, a_local, n_rank, n_iters, n_oversamples, *, seed=None, omega=None, fused=False, shard="rows", qr=None,
                     mixed=None):
        """Sharded random_svd, one process per GPU.  shard="rows": `a_local` holds this rank's
        rows of a TALL matrix (torch CUDA tensor); returns (U_local, S, Vt) with S, Vt replicated.  shard="cols":
        `a_local` holds this rank's COLUMNS of a FAT matrix; returns (U, S, Vt_local) with U, S replicated
        (CORRLA_SHARD_COLS: the long side is what gets sharded, after the reference's fat -> tall transpose)."""
        if shard not in ("rows", "cols"):
            raise ValueError("shard must be 'rows' or 'cols'")
        return self._rsvd_dense(a_local, int(n_rank), int(n_iters), int(n_oversamples), seed, omega, sharded=True, fused=fused,
                                shard_cols=(shard == "cols"), qr=qr, mixed=mixed)

    # ---- PCA caller (pca_rsvd.rs:56-82) ---------------------------------------------------
    def _pca_dense(self, x_mat, rank, n_iter, n_oversamples, seed, omega, center, sharded, standardize=False):
        cflags = {None: 0, "fused": L.PCA_CENTER_FUSED, "copy": L.PCA_CENTER_COPY}[center]
        if sharded:
            _reject_bf16(x_mat, "pca_sharded")
        x, on_dev = _as_dense(x_mat, "x_mat")
        m, n = x.shape
        if _is_bf16(x):
            if on_dev:
                self._on_my_device(x)
            return self._run_pca("corrla_pca_", (x, m, n, *_strides(x)), m, n, min(m, n), _f32_like(x), on_dev, int(rank), n_iter,
                                 n_oversamples, seed, omega, cflags, in_dtype=x.dtype, standardize=standardize)
        return self._run_pca("corrla_pca_sharded_" if sharded else "corrla_pca_", (x, m, n, *_strides(x)), m, n,
                             n if sharded else min(m, n), x, on_dev, int(rank), n_iter, n_oversamples, seed, omega, cflags,
                             standardize=standardize)

    def pca_sharded(self, x_local, rank, n_iter=None, n_oversamples=None, *, seed=None, omega=None, center=None, standardize=False):
        """PcaRsvd::new on SAMPLE-sharded data (one process per GPU, `comm_init` done): `x_local` = this rank's samples
        (CUDA tensor m_local x n_dim).  Returns (means, S, components), replicated on every rank; with standardize=True
        (see pca) also the scales, from one more all-reduce of n_dim values."""
        _reject_bf16(x_local, "pca_sharded")
        if not (_is_torch(x_local) and x_local.is_cuda):
            raise ValueError("pca_sharded takes torch CUDA tensors")
        return self._pca_dense(x_local, rank, n_iter, n_oversamples, seed, omega, center, sharded=True,
                               standardize=_check_standardize(standardize))

    def pca(self, x_mat, rank, n_iter=None, n_oversamples=None, *, seed=None, omega=None, center=None, standardize=False):
        """PcaRsvd::new(x, rank): returns (means (1, n), singular values (k, 1), components (k, n)).
        n_iter / n_oversamples default to the reference's hard-coded 20 / min(n_dim, 10) (pca_rsvd.rs:65-66).
        center: None (library default: implicit rank-1 corrections for f64 and bfloat16, a centred copy for f32), "fused"
        or "copy" (CORRLA_PCA_CENTER_* in include/corrla_rsvd.h; "copy" on a bfloat16 tensor centres a widened f32 copy).  Sparse x_mat (see _as_csr): always "fused"; "copy" raises.
        standardize=True: PCA on standardised columns (CORRLA_PCA_STANDARDIZE) -- every column is also divided by its sample
        standard deviation (n_samples - 1 divisor; 1 for a constant column), i.e. PCA of the correlation matrix, what
        StandardScaler -> PCA gives.  x_mat is not rewritten, widened or densified for it.  Returns
        (means, S, components, scales) with scales (1, n) of the kind and dtype of means; the components are directions in
        STANDARDISED coordinates (project (x - means) / scales onto them).  False: today's call and today's three items."""
        rank = int(rank)
        standardize = _check_standardize(standardize)
        if center not in (None, "fused", "copy"):
            raise ValueError("center must be None, 'fused' or 'copy'")
        if not _is_sparse(x_mat):
            return self._pca_dense(x_mat, rank, n_iter, n_oversamples, seed, omega, center, sharded=False, standardize=standardize)
        if center == "copy":  # always the fused centring: the matrix stays sparse
            raise ValueError("center='copy' on sparse input: a centred copy would densify the matrix")
        operand, m, n, like, on_dev = self._csr_operand(x_mat)
        return self._run_pca("corrla_pca_csr_", operand, m, n, min(m, n), like, on_dev, rank, n_iter, n_oversamples, seed, omega,
                             L.PCA_CENTER_FUSED, standardize=standardize)

    # ---- covariance / correlation matrices (stats_corr.rs:14-43) --------------------------------
    def cov(self, x, *, correlation=False, center=True, ddof=1):
        """Covariance matrix of the columns of x (n_samples x n_dim), ``mat_cov_centered`` (stats_corr.rs:32-43), or with
        correlation=True their Pearson correlation matrix, ``pearson_corr`` (:14-28) -> (C (n, n), means (1, n), scales (1, n)).

        One symmetric MFMA kernel (corrla_cov_*): only the tile pairs on and above the diagonal are computed, x is centred
        in registers -- never rewritten, and never copied when its features have unit stride -- and C is bitwise symmetric.
        center=False: the second-moment matrix x^T x / (n_samples - ddof); means is then None.  scales is None without
        correlation; with it, the column standard deviations (divisor n_samples - ddof; 1 for a constant column, whose row,
        column and diagonal entry of C are 0).  ddof: 0 or 1.
        numpy in -> numpy out; a CUDA tensor in -> tensors on its device.  float32 stays float32, anything else becomes
        float64.  bfloat16 and sparse inputs raise ValueError.  ``last_cov_route()`` names the route that served the call."""
        correlation, center = _check_bool("correlation", correlation, ValueError), _check_bool("center", center, ValueError)
        if isinstance(ddof, (bool, np.bool_)) or not isinstance(ddof, (int, np.integer)) or ddof not in (0, 1):
            raise ValueError("ddof must be 0 or 1")
        if correlation and not center:
            raise ValueError("correlation=True needs center=True: a correlation matrix is one of centred columns")
        if _is_sparse(x):
            raise ValueError("cov has no sparse entry: a covariance matrix is dense; pass a dense matrix (.toarray() / .to_dense())")
        a, on_dev = self._dense_arg(x, "x", "cov")
        m, n = a.shape
        flags = (L.COV_CORRELATION if correlation else 0) | (0 if center else L.COV_NO_CENTER)
        c = _empty(a, (n, n))
        means = _empty(a, (1, n)) if center else None
        scales = _empty(a, (1, n)) if correlation else None
        route = C.c_int(0)   # this entry reports its route itself
        self._call("corrla_cov_", a.dtype, (_ptr(a), m, n, *_strides(a), flags, int(ddof), _opt_ptr(means), _opt_ptr(scales), _ptr(c), n,
                   C.byref(route)), on_dev, a)
        self._last["cov_route"] = L.COV_ROUTES.get(route.value)
        return c, means, scales

    def last_cov_route(self):
        """The route of this context's last ``cov`` call: "inplace" (x read where it lies with 16-byte loads),
        "inplace_checked" (in place through bounds-checked element loads: base or row stride not 16-byte aligned) or
        "repacked" (feature-strided x, transposed once into workspace); None before the first call."""
        return self._last.get("cov_route")

    # ---- the fitted PCA model on the device (pca_rsvd.rs:43-52) ----------------------------------
    def _model_array(self, v, like, on_device):
        """A small array of the model (means, scales, components, scores) as the dtype, kind and device of `like`."""
        if on_device:
            import torch
            t = v if _is_torch(v) else torch.tensor(np.asarray(v))  # (a copy: the model arrays are small, and may be read-only)
            return t.detach().to(device=like.device, dtype=like.dtype)
        return np.asarray(v.detach().cpu().numpy() if _is_torch(v) else v, dtype=like.dtype)

    def _model(self, means, components, scales, n, like, on_device):
        """-> (means (n,) or None, scales (n,) or None, components as k x n column-major with ldc = k, k); ValueError on
        any shape that does not fit n features (n None: the components say how many there are)."""
        if components is None:
            raise ValueError("components must be given")
        comps = self._model_array(components, like, on_device)
        if comps.ndim != 2 or (n is not None and comps.shape[1] != n):
            raise ValueError(f"components must have shape (k, {'n' if n is None else n}), got {tuple(comps.shape)}")
        n = int(comps.shape[1])
        k = int(comps.shape[0])
        if k < 1 or k > n:
            raise ValueError(f"components must have between 1 and n = {n} rows, got {k}")
        # (k, n) column-major: numpy F order; torch: the (n, k) row-major transpose
        comps = comps.t().contiguous() if on_device else np.asfortranarray(comps)
        vecs = []
        for name, v in (("means", means), ("scales", scales)):
            if v is None:
                vecs.append(None)
                continue
            a = self._model_array(v, like, on_device).reshape(-1)
            if a.shape[0] != n:
                raise ValueError(f"{name} must have {n} entries, got {a.shape[0]}")
            vecs.append(a.contiguous() if on_device else np.ascontiguousarray(a))
        return vecs[0], vecs[1], comps, k

    def pca_transform(self, x, means, components, scales=None, *, own_means=False, residuals=False, center=None):
        """A fitted PCA model applied to x (m x n) on the device (corrla_pca_transform_*): the scores
        t = ((x - means) / scales) @ components.T, shape (m, k), column-major like U.  `means` (n values), `components`
        (k, n) and `scales` (n values, None: 1) are what ``pca`` returned; they are converted to x's dtype and device.
        means=None: no centring.

        own_means=True: x is centred by its OWN column means (the reference's ``apply_tr``, pca_rsvd.rs:43-46); `means` is
        ignored and the means of x, (1, n), are appended to the result.
        residuals=True: also q (m,), the Q / SPE statistic q_i = ||z_i - t_i V||^2 of every sample, formed directly from
        z - t V by the back-projection kernel (never as a difference of norms, never through an m x n temporary) from the
        scores as stored.  -> scores | (scores, q) [+ (means,)].
        center: None (library default: fused for float64, a centred and scaled copy in workspace for float32), "fused" or
        "copy", as for ``pca``.  x: dense numpy, a CUDA tensor, or any sparse form ``_as_csr`` takes (always "fused", never
        densified; residuals=True raises ValueError).  numpy in -> numpy out, a tensor in -> tensors on its device; float32
        stays float32, anything else becomes float64; bfloat16 raises.
        Row-sharded data needs nothing more: every rank calls this on its own rows with the replicated model.
        ``last_pca_apply_route()`` / ``last_pca_apply_centring()`` say how the call ran."""
        own_means = _check_bool("own_means", own_means, ValueError)
        residuals = _check_bool("residuals", residuals, ValueError)
        if center not in (None, "fused", "copy"):
            raise ValueError("center must be None, 'fused' or 'copy'")
        flags = {None: 0, "fused": L.PCA_CENTER_FUSED, "copy": L.PCA_CENTER_COPY}[center] | (L.PCA_APPLY_OWN_MEANS if own_means else 0)
        _reject_bf16(x, "pca_transform")
        if _is_sparse(x):
            if residuals:
                raise ValueError("residuals=True on sparse input: the residual over a sparse row's implicit zeros is a dense computation")
            if center == "copy":
                raise ValueError("center='copy' on sparse input: a centred copy would densify the matrix")
            operand, m, n, like, on_dev = self._csr_operand(x)
            stem = "corrla_pca_transform_csr_"
        else:
            a, on_dev = self._dense_arg(x, "x", "pca_transform")
            m, n = a.shape
            operand, like, stem = (a, m, n, *_strides(a)), a, "corrla_pca_transform_"
        mu, sd, comps, k = self._model(None if own_means else means, components, scales, n, like, on_dev)
        scores = _empty_colmajor(like, m, k)
        q = _empty(like, (m,)) if residuals else None
        mu_out = _empty(like, (1, n)) if own_means else None
        self._call(stem, like.dtype, (*_c_args(operand), _opt_ptr(mu), _opt_ptr(sd), _ptr(comps), k, k, flags, _ptr(scores), m, _opt_ptr(q),
                   _opt_ptr(mu_out)), on_dev, like, "pca_apply")
        out = (scores,) + ((q,) if residuals else ()) + ((mu_out,) if own_means else ())
        return out[0] if len(out) == 1 else out

    def pca_inverse_transform(self, scores, means, components, scales=None):
        """The reconstruction (scores @ components) * scales + means, (m, n) row-major, in one kernel and one write of m x n
        (corrla_pca_inverse_*; ``apply_inv_tr``, pca_rsvd.rs:49-52).  means / scales None: 0 / 1.  numpy in -> numpy out, a
        CUDA tensor in -> a tensor on its device; float32 stays float32, anything else becomes float64."""
        t, on_dev = self._dense_arg(scores, "scores", "pca_inverse_transform", sparse="pca_inverse_transform takes dense scores")
        m, k_in = t.shape
        mu, sd, comps, k = self._model(means, components, scales, None, t, on_dev)
        n = int(comps.shape[0] if on_dev else comps.shape[1])
        if k != k_in:
            raise ValueError(f"scores have {k_in} columns, components {k} rows")
        # (m, k) column-major with ld = m: no copy for what pca_transform returned
        tc = t.t().contiguous() if on_dev else np.asfortranarray(t)
        out = _empty(t, (m, n))
        self._call("corrla_pca_inverse_", t.dtype, (_ptr(tc), m, k, m, _opt_ptr(mu), _opt_ptr(sd), _ptr(comps), k, n, _ptr(out), n), on_dev, t,
                   "pca_apply")
        return out

    def last_pca_apply_route(self):
        """How the back-projection kernel of this context's last ``pca_transform`` / ``pca_inverse_transform`` call touched
        its m x n operand (x of the residuals, the output of the inverse): "inplace" (16-byte accesses), "inplace_checked"
        (element accesses: base or row stride not 16-byte aligned) or "repacked" (feature-strided x, transposed once into
        workspace); None when the call ran no such kernel, and before the first call."""
        return self._last.get("pca_apply_route")

    def last_pca_apply_centring(self):
        """The centring of the last ``pca_transform`` call: "fused", "copy", or None (no centring, or no such call yet)."""
        return self._last.get("pca_apply_centring")

    # ---- radial-basis-function kernel matrices (interp_utils.rs:96-129, 146-153) -------------------
    @staticmethod
    def _rbf_kernel_id(kernel_type):
        """``PyRbfInterp::new``: 1 linear, 2 multiquadric, 3 cubic, anything else Gaussian (4)."""
        k = int(kernel_type)
        return k if k in (1, 2, 3) else 4

    def _rbf_points(self, x_query, x_support, what):
        """-> (queries, supports, on_device): both row-major with unit stride along the coordinates, the supports in the
        kind, dtype and device of the queries."""
        for v in (x_query, x_support):
            _reject(v, what, f"{what} takes dense points")
        xq, on_dev = self._dense_arg(x_query, "x_query", what, nonempty=False)
        xs, _ = self._dense_arg(x_support, "x_support", what, like=xq, nonempty=False)
        if xq.shape[0] == 0 or xs.shape[0] == 0 or xq.shape[1] == 0:
            raise ValueError("x_query and x_support must be non-empty")
        if xs.shape[1] != xq.shape[1]:
            raise ValueError(f"x_query has {xq.shape[1]} coordinates, x_support {xs.shape[1]}")
        return _rowmajor(xq), _rowmajor(xs), on_dev

    def rbf_matrix(self, x_query, x_support, kernel_type, kernel_param=0.0):
        """The kernel matrix Phi[i, j] = phi(||x_query_i - x_support_j||_2), (n_q, n_s) row-major, on the device
        (corrla_rbf_matrix_*): 1 linear r, 2 multiquadric sqrt(1 + (eps r)^2), 3 cubic r^3, anything else the Gaussian
        exp(-(eps r)^2), eps = kernel_param -- the ids of ``PyRbfInterp``.  Distances are the direct sum of squared
        differences, so ``rbf_matrix(x, x)`` equals its transpose bitwise and has the exact diagonal phi(0).  dim <= 128.
        numpy in -> numpy out, a CUDA tensor as x_query -> a tensor on its device; float32 stays float32, anything else
        becomes float64; bfloat16 and sparse inputs raise ValueError."""
        xq, xs, on_dev = self._rbf_points(x_query, x_support, "rbf_matrix")
        n_q, dim = (int(v) for v in xq.shape)
        n_s = int(xs.shape[0])
        out = _empty(xq, (n_q, n_s))
        self._call("corrla_rbf_matrix_", xq.dtype, (_ptr(xq), n_q, _row_stride(xq), _ptr(xs), n_s, _row_stride(xs), dim,
                   self._rbf_kernel_id(kernel_type), float(kernel_param), _ptr(out), n_s), on_dev, xq)
        return out

    def rbf_apply(self, x_query, x_support, coeffs, kernel_type, kernel_param=0.0, *, poly_degree=None):
        """Phi(x_query, x_support) @ W_rbf + P(x_query) @ W_poly, (n_q, n_rhs) row-major, on the device (corrla_rbf_apply_*)
        without ever storing the (n_q, n_s) kernel matrix: what ``RbfInterp.predict`` computes (interp_utils.rs:146-153).
        `coeffs` is (n_s + n_poly, n_rhs) as ``RbfInterp.fit`` lays it out: the first n_s rows weight the kernel columns,
        the rest the polynomial tail [x, 1] (poly_degree 0 or 1: dim + 1 rows) or [x, x_a x_b (a <= b), 1] (poly_degree >= 2:
        dim + dim (dim + 1) / 2 + 1 rows); poly_degree=None: no tail, n_s rows.  Kernel ids and kernel_param as for
        ``rbf_matrix``.  x_support and coeffs are converted to the kind, dtype and device of x_query.  numpy in -> numpy out,
        a CUDA tensor as x_query -> a tensor on its device; float32 stays float32, anything else becomes float64; bfloat16
        and sparse inputs raise ValueError."""
        xq, xs, on_dev = self._rbf_points(x_query, x_support, "rbf_apply")
        n_q, dim = (int(v) for v in xq.shape)
        n_s = int(xs.shape[0])
        degree, n_poly = _rbf_tail(poly_degree, dim)
        _reject(coeffs, "rbf_apply", "rbf_apply takes dense coefficients")
        w = self._model_array(coeffs, xq, on_dev)
        if w.ndim == 1:
            w = w.reshape(-1, 1)
        if w.ndim != 2 or w.shape[1] == 0:
            raise ValueError("coeffs must be a non-empty matrix")
        if w.shape[0] != n_s + n_poly:
            raise ValueError(f"coeffs must have n_s + n_poly = {n_s} + {n_poly} rows, got {w.shape[0]}")
        w = _rowmajor(w)
        n_rhs = int(w.shape[1])
        out = _empty(xq, (n_q, n_rhs))
        self._call("corrla_rbf_apply_", xq.dtype, (_ptr(xq), n_q, _row_stride(xq), _ptr(xs), n_s, _row_stride(xs), dim,
                   self._rbf_kernel_id(kernel_type), float(kernel_param), degree, _ptr(w), _row_stride(w), n_rhs, _ptr(out), n_rhs), on_dev, xq)
        return out

    # ---- dense LU solve and the RBF fit on it (corrla_lu_solve_* / corrla_rbffit_system_* / corrla_rbffit_*) ---------
    def _f64_matrix(self, v, name, what, like=None, nonempty=False):
        """-> (v as a float64 matrix the solve entries read: row-major, unit column stride, rows that do not overlap;
        on_device).  like: an array whose kind and device v is converted to; None: v's own."""
        return self._dense_arg(v, name, what, sparse=f"{what} takes a dense {name}", like=like, f64=True, nonempty=nonempty, rowmajor=True)

    def solve(self, a, b, *, overwrite=False, assume="general"):
        """x with a x = b on the device (corrla_lu_solve_*): LU with partial pivoting (P A = L U, ties to the lowest row,
        |l_ij| <= 1 exactly, no atomics: a fixed input gives bitwise fixed output), then the substitutions.  a is (n, n), b is
        (n,) or (n, n_rhs); x has the shape of b.  float64 only: anything else is converted.  numpy `a` -> numpy out (a and b
        are left untouched), a CUDA tensor as `a` -> a tensor on its device; b is converted to the kind and device of a.
        overwrite=True (tensors only, float64 row-major): a is overwritten with L and U and b with x, nothing is copied.
        A pivot that is exactly zero or not finite raises RuntimeError (``CorrlaError``, code ENUMERIC) naming the 1-based
        column.  ``last_solve_route`` ("small": n <= 128, one workgroup in LDS; "blocked") and ``last_solve_info`` (info, the
        smallest |pivot|, the largest |u_ij|) describe the call.  ValueError: a not square, b with other than n rows, empty,
        sparse or bfloat16 inputs, a tensor on another device, n above 131072.
        assume="general" (the default) is that route.  assume="pos": a is symmetric positive definite and the solve goes
        through its Cholesky factor (corrla_chol_solve_*): only the LOWER triangle of a is read, overwrite=True leaves L in
        it (the strict upper triangle as it was) and x in b, a pivot that is not positive or not finite raises the same
        ``CorrlaError`` naming the column, and ``last_chol_route`` / ``last_chol_info`` describe the call instead.  Any other
        value of assume is a ValueError."""
        if assume not in ("general", "pos"):
            raise ValueError("assume must be 'general' or 'pos'")
        pos = assume == "pos"
        overwrite = _check_bool("overwrite", overwrite, ValueError)
        am, on_dev = self._f64_matrix(a, "a", "solve")
        n = int(am.shape[0])
        if n == 0 or am.shape[1] != n:
            raise ValueError(f"a must be square and non-empty, got {tuple(am.shape)}")
        vec = (b.dim() if _is_torch(b) else np.ndim(b)) == 1
        b2 = b.reshape(-1, 1) if vec else b
        bm, _ = self._f64_matrix(b2, "b", "solve", like=am)
        if bm.shape[0] != n or bm.shape[1] == 0:
            raise ValueError(f"b must have n = {n} rows and at least one column, got {tuple(bm.shape)}")
        n_rhs = int(bm.shape[1])
        if on_dev:
            if overwrite:
                if not (_is_torch(a) and _is_torch(b) and am.data_ptr() == a.data_ptr() and bm.data_ptr() == b.data_ptr()):
                    raise ValueError("overwrite=True takes float64 row-major CUDA tensors that need no conversion")
            else:
                am, bm = am.clone(), bm.clone()
            x, out = bm, (() if pos else (None,))   # in place: x over b; the interchanges of the LU entry (ipiv) are not wanted
        else:
            if overwrite:
                raise ValueError("overwrite=True needs CUDA tensors: the host entry leaves a and b untouched")
            x = _empty(am, (n, n_rhs))
            out = (_ptr(x), n_rhs)
        self._call("corrla_chol_solve_" if pos else "corrla_lu_solve_", np.float64, (_ptr(am), n, _row_stride(am), _ptr(bm), n_rhs, _row_stride(bm),
                   *out), on_dev, am, "chol" if pos else "solve")
        return x.reshape(-1) if vec else x

    # ---- dense Cholesky factor and SPD solve (corrla_chol_factor_* / corrla_chol_solve_*) ----------------------------
    def cholesky(self, a, *, overwrite=False):
        """The Cholesky factor L of a symmetric positive definite a, a = L L^T, on the device (corrla_chol_factor_*): (n, n),
        lower triangular with a positive diagonal, its strict upper triangle zero.  Only the LOWER triangle of a is read: what
        lies above the diagonal is never looked at (nobody checks the symmetry).  float64 only: anything else is converted.
        numpy in -> numpy out (a is left untouched), a CUDA tensor in -> a tensor on its device.  overwrite=True (float64
        row-major CUDA tensors only) factors in place and returns `a` itself: L over its lower triangle, the strict upper
        triangle as it was.  No pivoting, no atomics: a fixed input gives bitwise fixed output.  A pivot that is not positive
        or not finite raises RuntimeError (``CorrlaError``, code ENUMERIC) naming the 1-based column.  ``last_chol_route``
        ("small": n <= 128, one workgroup in LDS; "blocked") and ``last_chol_info`` (info, the smallest and largest l_jj,
        logdet = log det a) describe the call.  ValueError: a not square, empty, sparse or bfloat16, a tensor on another
        device, n above 131072."""
        overwrite = _check_bool("overwrite", overwrite, ValueError)
        am, on_dev = self._f64_matrix(a, "a", "cholesky")
        n = int(am.shape[0])
        if n == 0 or am.shape[1] != n:
            raise ValueError(f"a must be square and non-empty, got {tuple(am.shape)}")
        if on_dev:
            if overwrite:
                if not (_is_torch(a) and am.data_ptr() == a.data_ptr()):
                    raise ValueError("overwrite=True takes a float64 row-major CUDA tensor that needs no conversion")
            else:
                am = am.clone()
            self._call("corrla_chol_factor_", np.float64, (_ptr(am), n, _row_stride(am)), True, am, "chol")
            return a if overwrite else am.tril_()
        if overwrite:
            raise ValueError("overwrite=True needs a CUDA tensor: the host entry leaves a untouched")
        out = _empty(am, (n, n))
        self._call("corrla_chol_factor_", np.float64, (_ptr(am), n, _row_stride(am), _ptr(out), n), False, last="chol")
        return out

    @property
    def last_chol_route(self):
        """"small" or "blocked": the route of this context's last ``cholesky`` / ``solve(assume="pos")``; None before the first."""
        return self._last.get("chol_route")

    @property
    def last_chol_info(self):
        """{"info": 0 or the 1-based column of the failed pivot, "min_diag", "max_diag": smallest and largest l_jj of the
        columns factored, "logdet": log det a (0.0 when info != 0)} of this context's last ``cholesky`` /
        ``solve(assume="pos")``; None before the first."""
        return self._last.get("chol_info")

    # ---- symmetric eigendecomposition (corrla_eigh_*) ------------------------------------------------------------------
    def eigh(self, a):
        """(w, v) with a = v diag(w) v^T for a symmetric a, on the device (corrla_eigh_*): w (n,) ascending as
        ``numpy.linalg.eigh`` returns it, v (n, n) row-major with the eigenvectors in its columns, each with its component of
        largest magnitude positive.  Only the LOWER triangle of a is read (nobody checks the symmetry) and a is left
        untouched.  float64 only: anything else is converted.  numpy in -> numpy out; a CUDA tensor in -> tensors on its
        device, and nothing visits the host.
        The route is a shift to a positive definite matrix, its Cholesky factor and one-sided block Jacobi on that factor
        (DESIGN 7l).  It is normwise backward stable: the absolute errors of w are of order n u |a|, like LAPACK's for an
        indefinite matrix; it is NOT relatively accurate for eigenvalues much smaller than |a|.  No atomics: a fixed input
        gives bitwise fixed output, the same from numpy and from a tensor.  A non-finite entry in the lower triangle, or an
        iteration beyond 40 sweeps, raises RuntimeError (``CorrlaError``, code ENUMERIC).  ``last_eigh_route`` ("small":
        n <= 64, one workgroup; "blocked") and ``last_eigh_info`` describe the call.  ValueError: a not square, empty,
        sparse or bfloat16, a tensor on another device, n above 32768."""
        am, on_dev = self._f64_matrix(a, "a", "eigh")
        n = int(am.shape[0])
        if n == 0 or am.shape[1] != n:
            raise ValueError(f"a must be square and non-empty, got {tuple(am.shape)}")
        w, v = _empty(am, (n,)), _empty(am, (n, n))
        self._call("corrla_eigh_", np.float64, (_ptr(am), n, _row_stride(am), _ptr(w), _ptr(v), n), on_dev, am if on_dev else None, "eigh")
        return w, v

    def eigh_solve(self, a, b, *, rcond=None, reg=None):
        """x = V f(L) V^T b with (L, V) = ``eigh(a)``: the pseudo-inverse solve of a symmetric a that may be singular or
        indefinite.  a is (n, n), b is (n,) or (n, n_rhs); x has the shape of b; numpy `a` -> numpy out, a CUDA tensor -> a
        tensor.  The decomposition, the two products (``matmul``) and the scaling between them run on the device.
        Default rule: f(l) = 1 / l where |l| > rcond max|l|, else 0, with rcond = n 2^-52 (the rule of ``polyfit_solve``).
        reg=eps: f(l) = sign(l) / (|l| + eps) with sign(0) = + (the rule of ``mat_pinv`` on a symmetric matrix).  rcond and
        reg exclude each other.  ``last_eigh_info["dropped"]`` holds the number of directions the default rule set to zero (0
        with reg).  The accuracy is that of ``eigh``: absolute in the eigenvalues, so the cut is meaningful only as an
        absolute one, which rcond max|l| is."""
        import torch
        if rcond is not None and reg is not None:
            raise ValueError("eigh_solve takes rcond or reg, not both")
        if reg is not None and not (np.isfinite(reg) and reg >= 0.0):
            raise ValueError("reg must be finite and >= 0")
        if rcond is not None and not (np.isfinite(rcond) and rcond >= 0.0):
            raise ValueError("rcond must be finite and >= 0")
        am, on_dev = self._f64_matrix(a, "a", "eigh_solve")
        n = int(am.shape[0])
        if n == 0 or am.shape[1] != n:
            raise ValueError(f"a must be square and non-empty, got {tuple(am.shape)}")
        vec = (b.dim() if _is_torch(b) else np.ndim(b)) == 1
        b2 = b.reshape(-1, 1) if vec else b
        bm, _ = self._f64_matrix(b2, "b", "eigh_solve", like=am)
        if bm.shape[0] != n or bm.shape[1] == 0:
            raise ValueError(f"b must have n = {n} rows and at least one column, got {tuple(bm.shape)}")
        dev = torch.device(f"cuda:{self.device}")
        at = am if on_dev else torch.from_numpy(am).to(dev)
        bt = bm if on_dev else torch.from_numpy(bm).to(dev)
        w, v = self.eigh(at)
        if reg is not None:
            f = torch.where(w < 0, -1.0, 1.0) / (w.abs() + float(reg))
            dropped = 0
        else:
            keep = w.abs() > (n * 2.0 ** -52 if rcond is None else float(rcond)) * w.abs().max()
            f = torch.where(keep, 1.0 / torch.where(keep, w, torch.ones_like(w)), torch.zeros_like(w))
            dropped = n - int(keep.sum().item())
        t = self.matmul(v, bt.contiguous(), trans=True)          # V^T b
        L.check(self._lib.corrla_ctx_synchronize(self._h))
        t = (t * f[:, None]).contiguous()
        x = self.matmul(v, t).contiguous()                       # V (f(L) V^T b)
        L.check(self._lib.corrla_ctx_synchronize(self._h))
        self._last["eigh_info"] = dict(self._last["eigh_info"], dropped=dropped)
        if not on_dev:
            x = x.cpu().numpy()
        return x.reshape(-1) if vec else x

    @property
    def last_eigh_route(self):
        """"small" or "blocked": the route of this context's last ``eigh`` / ``eigh_solve``; None before the first."""
        return self._last.get("eigh_route")

    @property
    def last_eigh_info(self):
        """{"info": 0, or 1 non-finite entry / 2 Cholesky pivot / 3 sweep cap, "sweeps": the sweeps that rotated, "off": the
        largest measure max |g_ij| / sqrt(g_ii g_jj) of the last sweep, "shift": sigma, "dropped": the directions the last
        ``eigh_solve`` set to zero (None after a plain ``eigh``)} of this context's last ``eigh`` / ``eigh_solve``; None
        before the first."""
        return self._last.get("eigh_info")

    @property
    def last_solve_route(self):
        """"small" or "blocked": the route of this context's last ``solve`` / ``rbf_fit``; None before the first."""
        return self._last.get("solve_route")

    @property
    def last_solve_info(self):
        """{"info": 0 or the 1-based column of the failed pivot, "min_pivot": smallest |pivot|, "max_u": largest |u_ij|} of
        this context's last ``solve`` / ``rbf_fit``; None before the first."""
        return self._last.get("solve_info")

    def _rbf_fit_args(self, x, poly_degree, what):
        xs, on_dev = self._f64_matrix(x, "x", what, nonempty=True)
        n_s, dim = (int(v) for v in xs.shape)
        degree, n_poly = _rbf_tail(poly_degree, dim)
        return xs, on_dev, n_s, dim, degree, n_s + n_poly

    def rbf_system(self, x, kernel_type, kernel_param=0.0, *, poly_degree=None):
        """The block system M = [[K, P], [P^T, 0]] of an RBF fit over the supports x (n_s, dim), (N, N) with
        N = n_s + n_poly, float64, on the device (corrla_rbffit_system_*): K is bitwise ``rbf_matrix(x, x)``, P the polynomial
        tail of ``rbf_apply`` ([x, 1] for poly_degree 0 or 1, [x, x_a x_b (a <= b), 1] from 2 on, none for None) with one
        rounding per product, the corner exactly zero.  numpy in -> numpy out, a CUDA tensor in -> a tensor on its device."""
        xs, on_dev, n_s, dim, degree, n = self._rbf_fit_args(x, poly_degree, "rbf_system")
        out = _empty(xs, (n, n))
        self._call("corrla_rbffit_system_", np.float64, (_ptr(xs), n_s, _row_stride(xs), dim, self._rbf_kernel_id(kernel_type), float(kernel_param),
                   degree, _ptr(out), n), on_dev, xs)
        return out

    def rbf_fit(self, x, y, kernel_type, kernel_param=0.0, *, poly_degree=None):
        """The coefficients of the RBF interpolant through (x, y) by an LU solve that never leaves the device
        (corrla_rbffit_*): ``solve(rbf_system(x, ...), [y; 0])`` bitwise, with the system in workspace.  x is (n_s, dim), y
        (n_s,) or (n_s, n_rhs); the result is (n_s + n_poly, n_rhs), the layout ``rbf_apply`` reads.  float64.  numpy x ->
        numpy out, a CUDA tensor as x -> a tensor on its device (y is converted to the kind and device of x; no N-sized
        array comes back to the host).  A singular system raises RuntimeError naming the column; ``last_solve_route`` and
        ``last_solve_info`` describe the call.  This is NOT the reference's solve: ``RbfInterp`` takes the regularised
        pseudo-inverse unless asked for solver="lu"."""
        xs, on_dev, n_s, dim, degree, n = self._rbf_fit_args(x, poly_degree, "rbf_fit")
        y2 = y.reshape(n_s, -1) if (y.dim() if _is_torch(y) else np.ndim(y)) == 1 else y
        ym, _ = self._f64_matrix(y2, "y", "rbf_fit", like=xs)
        if ym.shape[0] != n_s or ym.shape[1] == 0:
            raise ValueError(f"y must have n_s = {n_s} rows and at least one column, got {tuple(ym.shape)}")
        n_rhs = int(ym.shape[1])
        out = _empty(xs, (n, n_rhs))
        self._call("corrla_rbffit_", np.float64, (_ptr(xs), n_s, _row_stride(xs), dim, _ptr(ym), n_rhs, _row_stride(ym),
                   self._rbf_kernel_id(kernel_type), float(kernel_param), degree, _ptr(out), n_rhs), on_dev, xs, "solve")
        return out

    # ---- polynomial response surfaces (stats_corr.rs:146-249) ---------------------------------------
    @staticmethod
    def _poly_degree(degree):
        if isinstance(degree, (bool, np.bool_)) or not isinstance(degree, (int, np.integer)) or degree not in (1, 2):
            raise ValueError("degree must be 1 or 2")
        return int(degree)

    def _poly_x(self, x, what):
        """-> (x row-major with unit stride along the features, on_device)"""
        a, on_dev = self._dense_arg(x, "x", what, sparse=f"{what} takes a dense x")
        if a.shape[1] > 128:
            raise ValueError(f"{what}: x has {a.shape[1]} features, the kernels take 1 to 128")
        return _rowmajor(a), on_dev

    def polyfit_gram(self, x, y=None, degree=2, *, normalize=True):
        """The normal equations of a polynomial least-squares fit without the Vandermonde matrix -> (G, means, scales).

        With V = [z, z_a z_b (a <= b, a outer), 1] (degree 2; [z, 1] for degree 1 -- ``build_vandermonde``,
        stats_corr.rs:201-209) of the samples z = (x - means) * (1 / scales) and W = [V, y], G = W^T W of order p + r
        (p = k + k (k + 1) / 2 + 1 or k + 1; r the columns of y, 0 without y): ``G[:p, :p]`` is V^T V, ``G[:p, p:]`` is
        V^T y and ``G[p:, p:]`` is y^T y.  One fused MFMA kernel (corrla_polyfit_gram_*) forms the columns of W in registers;
        all arithmetic is f64 and float32 input is widened in place.  G, means (1, k) and scales (1, k) are float64 for
        either input type; G is bitwise symmetric and bitwise reproducible.  normalize=True (the default) centres and scales
        every feature by its mean and population standard deviation (1 for a constant column) inside the kernel, which is
        what keeps V^T V solvable for data away from the origin; normalize=False takes x as it is and returns None for
        means and scales.  1 <= k <= 128, at most 64 columns of y.
        numpy in -> numpy out; a CUDA tensor in -> tensors on its device.  bfloat16 and sparse inputs raise ValueError.
        ``last_polyfit_route()`` names the route that served the call."""
        degree = self._poly_degree(degree)
        normalize = _check_bool("normalize", normalize, ValueError)
        a, on_dev = self._poly_x(x, "polyfit_gram")
        m, kf = (int(v) for v in a.shape)
        if y is None:
            yy, r, ldy = None, 0, 0
        else:
            _reject(y, "polyfit_gram", "polyfit_gram takes a dense y")
            yy = self._model_array(y, a, on_dev)
            if yy.ndim == 1:
                yy = yy.reshape(-1, 1)
            if yy.ndim != 2 or yy.shape[0] != m:
                raise ValueError(f"y must have {m} rows, one per sample, got shape {tuple(yy.shape)}")
            r = int(yy.shape[1])
            if r > 64:
                raise ValueError(f"polyfit_gram: y has {r} columns, the kernels take at most 64")
            yy = _rowmajor(yy) if r else None
            ldy = _row_stride(yy) if r else 0
        order = _poly_terms(kf, degree) + r
        g = _empty(a, (order, order), np.float64)
        means = _empty(a, (1, kf), np.float64) if normalize else None
        scales = _empty(a, (1, kf), np.float64) if normalize else None
        self._call("corrla_polyfit_gram_", a.dtype, (_ptr(a), m, kf, _row_stride(a), _opt_ptr(yy), r, ldy, degree, int(normalize), _ptr(g), order,
                   _opt_ptr(means), _opt_ptr(scales)), on_dev, a, "polyfit")
        return g, means, scales

    def poly_eval(self, x, coeffs, degree=2, *, jac=False):
        """The polynomial with the coefficients `coeffs` at the rows of x -> values (m, r), or (values, gradients) with jac.

        `coeffs` is (p, r) -- a vector is one column -- in the column order of ``build_vandermonde`` (stats_corr.rs:201-209):
        [x, x_a x_b (a <= b, a outer), 1] for degree 2, [x, 1] for degree 1, in the coordinates of x; they are taken as
        float64 whatever the type of x.  What ``quad_eval`` (stats_corr.rs:222-226) computes as V(x) @ coeffs is computed
        here as xt^T C xt with xt = [x, 1] and C the symmetric (k + 1) x (k + 1) matrix of one coefficient column, on the
        f64 MFMAs (corrla_poly_eval_*); V is never formed.  jac=True also returns the analytic gradients 2 (C xt)[:k] from
        the same product: shape (m, k) for r = 1 and (r, m, k) otherwise.  Values and gradients have the dtype of x.
        numpy in -> numpy out; a CUDA tensor in -> tensors on its device.  bfloat16 and sparse inputs raise ValueError."""
        degree = self._poly_degree(degree)
        jac = _check_bool("jac", jac, ValueError)
        a, on_dev = self._poly_x(x, "poly_eval")
        m, kf = (int(v) for v in a.shape)
        _reject(coeffs, "poly_eval", "poly_eval takes dense coefficients")
        c = self._model_array(coeffs, _empty(a, 0, np.float64), on_dev)
        if c.ndim == 1:
            c = c.reshape(-1, 1)
        p = _poly_terms(kf, degree)
        if c.ndim != 2 or c.shape[0] != p or c.shape[1] == 0:
            raise ValueError(f"coeffs must have p = {p} rows for {kf} features at degree {degree}, got shape {tuple(c.shape)}")
        r = int(c.shape[1])
        if r > 64:
            raise ValueError(f"poly_eval: coeffs has {r} columns, the kernels take at most 64")
        c = _rowmajor(c)
        out = _empty(a, (m, r))
        grad = _empty(a, (r, m, kf)) if jac else None
        self._call("corrla_poly_eval_", a.dtype, (_ptr(a), m, kf, _row_stride(a), _ptr(c), _row_stride(c), r, degree, _ptr(out), r, _opt_ptr(grad),
                   kf), on_dev, a, "polyfit")
        if not jac:
            return out
        return out, (grad[0] if r == 1 else grad)

    def last_polyfit_route(self):
        """The route of this context's last ``polyfit_gram`` / ``poly_eval`` call: "inplace" (x read where it lies with 16-byte
        loads) or "inplace_checked" (element loads: the base or the row stride of x not 16-byte aligned); None before the
        first call.  y, the narrow operand, is read by its own alignment and does not change the route."""
        return self._last.get("polyfit_route")

    # ---- Gaussian kernel density estimates (univariate_rv.rs:165-170, 423-444) ----------------------
    def _kde_vector(self, v, name, what):
        """-> (array as the entries read it, on_device, n, element stride, its shape): a vector, or an n x 1 column as the
        reference's column matrices, read in place at its stride; float32 stays float32, anything else becomes float64."""
        _reject(v, what, f"{what} takes dense vectors")
        if _is_torch(v) and v.is_cuda:
            import torch
            self._on_my_device(v)
            a, on_dev = (v.detach() if v.dtype in (torch.float32, torch.float64) else v.detach().to(torch.float64)), True
        else:
            a = np.asarray(v.detach().numpy() if _is_torch(v) else v)
            if a.dtype != np.float32:
                a = a.astype(np.float64, copy=False)
            on_dev = False
        if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] != 1):
            raise ValueError(f"{name} must be a vector or an n x 1 column, got shape {tuple(a.shape)}")
        n = int(a.shape[0])
        if n == 0:
            raise ValueError(f"{name} must be non-empty")
        if on_dev:
            inc = int(a.stride(0))
        else:
            inc = a.strides[0] // a.itemsize if a.strides[0] % a.itemsize == 0 else 0
        if n > 1 and inc < 1:     # reversed or broadcast views: the entries take strides >= 1
            a = a.contiguous() if on_dev else np.ascontiguousarray(a)
            inc = 1
        return a, on_dev, n, (inc if n > 1 else 1), tuple(a.shape)

    def _kde_pair(self, x, supports, what):
        xa, x_dev, n_q, incx, shape = self._kde_vector(x, "x", what)
        sa, s_dev, n_s, incs, _ = self._kde_vector(supports, "supports", what)
        if x_dev != s_dev:
            raise ValueError(f"{what}: x and supports must both be numpy arrays or both be tensors on cuda:{self.device}")
        if str(xa.dtype).split(".")[-1] != str(sa.dtype).split(".")[-1]:
            raise ValueError(f"{what}: x is {xa.dtype}, supports {sa.dtype}: convert one of them")
        return xa, n_q, incx, sa, n_s, incs, x_dev, shape

    def kde_eval(self, x, supports, bandwidth, what="pdf"):
        """The Gaussian kernel density estimate over `supports` (uniform weights) with the given bandwidth at the points x
        (corrla_kde_eval_*; ``KdeRv::pdf`` / ``cdf``, univariate_rv.rs:423-444): what="pdf" the density, "cdf" the distribution
        function (through erfc: relative accuracy in the lower tail), "logpdf" the log-density.  The sums are taken in the
        stabilised form exp(-t*) sum exp(-(t - t*)) with t* the term of the nearest support, so "logpdf" is finite wherever
        the reference's ``pdf(x).ln()`` is -inf, and "pdf" is right down to the underflow of the final product.  The
        (n_q, n_s) matrix is never stored.  x and supports are vectors or n x 1 columns of one dtype (float32 stays float32,
        anything else becomes float64), both numpy or both CUDA tensors, read in place at any stride.  Returns an array of the
        shape, dtype and kind of x.  ValueError before the library is touched: dtypes that differ, bfloat16, an empty array,
        a tensor on another device, a bandwidth that is not finite and > 0.  ``last_kde_route()`` names the route."""
        if what not in L.KDE_WHAT:
            raise ValueError(f'what must be "pdf", "cdf" or "logpdf", got {what!r}')
        xa, n_q, incx, sa, n_s, incs, on_dev, shape = self._kde_pair(x, supports, "kde_eval")
        h = float(bandwidth)
        if not (np.isfinite(h) and h > 0.0):
            raise ValueError(f"bandwidth must be finite and > 0, got {bandwidth!r}")
        out = _empty(xa, shape)
        self._call("corrla_kde_eval_", xa.dtype, (_ptr(xa), n_q, incx, _ptr(sa), n_s, incs, h, L.KDE_WHAT[what], _ptr(out), 1), on_dev, xa, "kde")
        return out

    def kde_nll(self, x_test, supports, bandwidths):
        """-> (nll, dnll): for every bandwidth h_b the negative log-likelihood -sum_i logpdf_i(h_b) of the test points under the
        estimate over `supports`, and its derivative in h at h_b (corrla_kde_nll_*; ``UniRv::nll``, univariate_rv.rs:165-170).
        Up to 64 bandwidths per call share one sweep: the squared distance of a pair is formed once per group of bandwidths.
        Both are float64 of length n_h for either input dtype -- numpy arrays for numpy input, tensors on the device for CUDA
        tensors -- finite for every h > 0 (stabilised sums, see ``kde_eval``), bitwise reproducible, and a bandwidth's values
        do not depend on the others of the call.  The derivative is analytic.  Inputs as for ``kde_eval``; `bandwidths` is a
        scalar or a sequence on the host."""
        xa, n_t, incx, sa, n_s, incs, on_dev, _ = self._kde_pair(x_test, supports, "kde_nll")
        hb = np.ascontiguousarray(np.atleast_1d(np.asarray(bandwidths.detach().cpu().numpy() if _is_torch(bandwidths) else bandwidths,
                                                           dtype=np.float64)))
        if hb.ndim != 1 or not 1 <= hb.shape[0] <= L.KDE_MAX_BANDWIDTHS:
            raise ValueError(f"bandwidths must be 1 to {L.KDE_MAX_BANDWIDTHS} values, got shape {tuple(hb.shape)}")
        if not (np.all(np.isfinite(hb)) and np.all(hb > 0.0)):
            raise ValueError("every bandwidth must be finite and > 0")
        n_h = int(hb.shape[0])
        nll, dnll = (_empty(xa, n_h, np.float64) for _ in range(2))
        self._call("corrla_kde_nll_", xa.dtype, (_ptr(xa), n_t, incx, _ptr(sa), n_s, incs, hb.ctypes.data, n_h, _ptr(nll), _ptr(dnll)), on_dev, xa,
                   "kde")
        return nll, dnll

    def last_kde_route(self):
        """The route of this context's last ``kde_eval`` / ``kde_nll`` call: "single" (every workgroup swept all supports) or
        "split" (few points: the supports were split over workgroups and the partial sums added in index order); None before
        the first call."""
        return self._last.get("kde_route")

    # ---- constrained Dirichlet sampling (space_samplers.rs:14-126) ------------------------------------
    @staticmethod
    def _dirichlet_stream(alphas, d, c_scale, seed):
        """-> (alphas as d float64, c_scale, seed), checked as the entries check them.  alphas: None (all ones), one value
        (symmetric) or d values -- the rules of ``constr_dirichlet_sample``, space_samplers.rs:73-95."""
        if alphas is None:
            al = np.ones(d if d is not None else 0, dtype=np.float64)
        else:
            al = np.atleast_1d(np.asarray(alphas.detach().cpu().numpy() if _is_torch(alphas) else alphas, dtype=np.float64))
            if al.ndim != 1:
                raise ValueError(f"alphas must be a scalar or a vector, got shape {tuple(al.shape)}")
            if d is not None and al.shape[0] == 1:
                al = np.full(d, al[0])
        if d is not None and al.shape[0] != d:
            raise ValueError(f"alphas must hold {d} values or 1 (the symmetric case), got {al.shape[0]}")
        if not 2 <= al.shape[0] <= L.DIRICHLET_MAX_D:
            raise ValueError(f"d must be in [2, {L.DIRICHLET_MAX_D}], got {al.shape[0]}")
        if not (np.all(np.isfinite(al)) and np.all(al > 0.0)):
            raise ValueError("every alphas[j] must be finite and > 0")
        c = float(c_scale)
        if not (np.isfinite(c) and c > 0.0):
            raise ValueError(f"c_scale must be finite and > 0, got {c_scale!r}")
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be in [0, 2^64), got {seed}")
        return np.ascontiguousarray(al), c, seed

    def dirichlet_draws(self, n, alphas, *, c_scale=1.0, seed=0, first=0, device=False):
        """Rows [first, first + n) of the Dirichlet stream of (seed, alphas, c_scale) (corrla_dirichlet_draws_*): row t is
        x_j = c_scale g_j / sum_i g_i with g_j ~ Gamma(alphas[j], 1), a pure function of (seed, alphas, c_scale, t) -- the
        stream is defined in include/corrla_rsvd.h -- so any slice of the stream is the same bits whichever call makes it.
        Returns (n, d) float64, numpy by default, a CUDA tensor with device=True.  alphas: d values, d in [2, 128].
        ValueError before the library is touched: alphas or c_scale not finite and > 0, d outside [2, 128], n < 1, first < 0,
        first + n > 2^62."""
        al, c, seed = self._dirichlet_stream(alphas, None, c_scale, seed)
        n, first = int(n), int(first)
        if n < 1:
            raise ValueError(f"n must be >= 1, got {n}")
        if first < 0 or first + n > L.DIRICHLET_MAX_DRAWS:
            raise ValueError(f"first must be >= 0 and first + n <= 2^62, got first = {first}, n = {n}")
        d = int(al.shape[0])
        out = _empty(self.device if device else None, (n, d), np.float64)
        self._call("corrla_dirichlet_draws_", np.float64, (al.ctypes.data, d, c, seed, first, n, _ptr(out), d), device, last="dirichlet")
        return out

    def dirichlet_sample(self, bounds, n_samples, alphas=None, *, c_scale=1.0, seed=0, max_zshots=500, chunk_size=1_000_000,
                         device=False):
        """-> (samples, n_found, n_drawn): the first n_samples draws of the Dirichlet stream of (seed, alphas, c_scale) that lie
        in the box bounds[j, 0] <= x_j <= bounds[j, 1] (closed, as space_samplers.rs:42), among the draws
        [0, max_zshots * chunk_size), in increasing draw index (corrla_dirichlet_sample_*; ``constr_dirichlet_sample``).
        samples is (n_samples, d) float64 -- numpy by default, a CUDA tensor with device=True -- with rows [n_found, n_samples)
        zero, which is what the reference leaves where it found nothing; n_drawn = chunk_size times the shots that were needed.
        The samples do not depend on chunk_size (n_drawn does), are bitwise reproducible for a seed, and lie inside the box
        exactly: the test is made on the stored doubles.  No candidate row is stored on the device: a draw is tested where it
        is generated and the accepted ones are generated again.  bounds: (d, 2); alphas: None (all ones), one value
        (symmetric) or d values.  ValueError before the library is touched: the conditions of ``dirichlet_draws``, n_samples,
        max_zshots or chunk_size < 1, max_zshots * chunk_size >= 2^62, a bound that is not finite, a lower bound above its
        upper bound, a box that holds no point with sum c_scale.  ``last_dirichlet_route()`` names the route,
        ``last_dirichlet_readbacks()`` how often the call waited for the device's count."""
        b = np.ascontiguousarray(np.asarray(bounds.detach().cpu().numpy() if _is_torch(bounds) else bounds, dtype=np.float64))
        if b.ndim != 2 or b.shape[1] != 2:
            raise ValueError(f"bounds must be (d, 2), got shape {tuple(b.shape)}")
        d = int(b.shape[0])
        al, c, seed = self._dirichlet_stream(alphas, d, c_scale, seed)
        n_samples, max_zshots, chunk_size = int(n_samples), int(max_zshots), int(chunk_size)
        for name, v in (("n_samples", n_samples), ("max_zshots", max_zshots), ("chunk_size", chunk_size)):
            if v < 1:
                raise ValueError(f"{name} must be >= 1, got {v}")
        if max_zshots * chunk_size >= L.DIRICHLET_MAX_DRAWS:
            raise ValueError("max_zshots * chunk_size must be < 2^62")
        if not np.all(np.isfinite(b)):
            raise ValueError("every bounds[j] must be finite")
        if np.any(b[:, 0] > b[:, 1]):
            raise ValueError("bounds[j][0] must be <= bounds[j][1]")
        slack = 8.0 * np.finfo(np.float64).eps * d * c
        if sum(b[:, 0].tolist()) > c + slack or sum(b[:, 1].tolist()) < c - slack:
            raise ValueError("bounds leave no point with sum c_scale (infeasible box)")
        out = _empty(self.device if device else None, (n_samples, d), np.float64)
        n_found, n_drawn = C.c_int64(0), C.c_int64(0)
        self._call("corrla_dirichlet_sample_", np.float64, (b.ctypes.data, al.ctypes.data, d, c, seed, n_samples, max_zshots, chunk_size, _ptr(out),
                   d, C.byref(n_found), C.byref(n_drawn)), device, last="dirichlet")
        return out, int(n_found.value), int(n_drawn.value)

    def last_dirichlet_route(self):
        """The route of this context's last ``dirichlet_draws`` / ``dirichlet_sample`` call: "registers/..." (d <= 16: the
        gammas of a row stay in registers) or "regenerate/..." (wider rows: one sweep forms the sum, a second draws each gamma
        again from its counter), then ".../exponential" (every alpha is 1) or ".../general"; None before the first call."""
        return self._last.get("dirichlet_route")

    def last_dirichlet_readbacks(self):
        """How many times the last ``dirichlet_sample`` call read the device's running count back (0 for ``dirichlet_draws``)."""
        return self._last.get("dirichlet_readbacks")

    # ---- multivariate normal rows and sandwich variances (stats_corr.rs:46-68) -----------------------------
    def _mvn_small(self, v, name, on_device, dtype_of=None):
        """A dense float32 / float64 argument (factor, mean, cov, jac) as a numpy array (host call) or a tensor on this
        context's device (device call); bfloat16, sparse and other dtypes raise ValueError.  dtype_of: the array whose type
        it has to share."""
        _reject(v, name, f"{name} must be dense")
        if _is_torch(v) and v.is_cuda:
            self._on_my_device(v)
            a = v.detach()
            if str(a.dtype) not in ("torch.float32", "torch.float64"):
                raise ValueError(f"{name} must be float32 or float64, got {a.dtype}")
            if not on_device:
                a = a.cpu().numpy()
        else:
            a = np.asarray(v.detach().numpy() if _is_torch(v) else v)
            if a.dtype not in (np.float32, np.float64):
                raise ValueError(f"{name} must be float32 or float64, got {a.dtype}")
            if on_device:
                import torch
                a = torch.tensor(a, device=f"cuda:{self.device}")
        if dtype_of is not None and _suffix(a.dtype) != _suffix(dtype_of.dtype):
            raise ValueError(f"{name} must have the dtype of the other arguments ({dtype_of.dtype}), got {a.dtype}")
        return a

    def mvn_sample(self, n, factor, mean=None, *, seed=0, first=0, lower=False, device=False, out=None):
        """Rows of N(mean, factor factor^T): X (n, d) with x_i = mean + factor z_i on the device (corrla_mvn_sample_*).

        `factor` is (d, r), 1 <= r <= d, float32 or float64 -- the dtype of X; `mean` (d,) of the same dtype, None: zeros.
        z_i[j] is the N(0,1) value of counter (first + i) r + j of the library's Philox4x32-10 / Box-Muller stream under
        `seed`: the values ``fill_normal(t, seed, row0=first, global_cols=r)`` writes into an (n, r) tensor (the stream is
        defined in include/corrla_rsvd.h).  So X is a pure function of (seed, first, factor, mean): bitwise reproducible,
        and rows [a, b) of a call are bitwise the call with first + a and n = b - a.
        lower=True: factor is square lower-triangular (a Cholesky factor); its strict upper triangle is taken as zero and
        the products above the diagonal are skipped -- bitwise the result of lower=False on the same triangular matrix.
        numpy by default; a CUDA `factor`, device=True or a CUDA `out` give a CUDA tensor.  out: an (n, d) array of that
        kind with unit stride along d, filled in place (any row stride >= d).  n = 0 returns an empty array without a
        launch.  ``last_mvn_route()``: "fused" (z lives in LDS only; r <= 288 in float32, 144 in float64) or "staged".
        ValueError before the library is touched: r < 1, r > d, n < 0, first < 0, (first + n) r >= 2^63, lower with a
        non-square factor, bfloat16 or sparse arguments, mismatched dtypes, an `out` of another shape or layout."""
        lower = _check_bool("lower", lower, ValueError)
        device = _check_bool("device", device, ValueError)
        on_dev = device or (_is_torch(factor) and factor.is_cuda) or (out is not None and _is_torch(out) and out.is_cuda)
        f = self._mvn_small(factor, "factor", on_dev)
        if f.ndim != 2:
            raise ValueError(f"factor must be (d, r), got shape {tuple(f.shape)}")
        d, r = (int(v) for v in f.shape)
        n, first, seed = int(n), int(first), int(seed)
        if r < 1 or d < 1:
            raise ValueError(f"factor must have r >= 1 columns, got shape {(d, r)}")
        if r > d:
            raise ValueError(f"factor has more columns than rows (r = {r} > d = {d})")
        if lower and r != d:
            raise ValueError(f"lower=True takes a square factor, got shape {(d, r)}")
        if n < 0:
            raise ValueError(f"n must be >= 0, got {n}")
        if first < 0 or (first + n) * r >= 1 << 63:
            raise ValueError(f"first must be >= 0 and (first + n) * r < 2^63, got first = {first}, n = {n}, r = {r}")
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be in [0, 2^64), got {seed}")
        f = _rowmajor(f)
        mu = None
        if mean is not None:
            mu = self._mvn_small(mean, "mean", on_dev, f).reshape(-1)
            if mu.shape[0] != d:
                raise ValueError(f"mean must have d = {d} entries, got {mu.shape[0]}")
            mu = mu.contiguous() if on_dev else np.ascontiguousarray(mu)
        if out is None:
            out = _empty(f, (n, d))
        else:
            _reject_bf16(out, "out")
            if (_is_torch(out) and out.is_cuda) != on_dev or not (_is_torch(out) or isinstance(out, np.ndarray)):
                raise ValueError("out must be a numpy array for a host call and a CUDA tensor for a device call")
            if tuple(out.shape) != (n, d) or _suffix(out.dtype) != _suffix(f.dtype) or str(out.dtype) != str(f.dtype):
                raise ValueError(f"out must be ({n}, {d}) of {f.dtype}, got {tuple(out.shape)} of {out.dtype}")
            rs, cs = _strides(out)
            if (cs != 1 and d > 1) or (rs < d and n > 1):
                raise ValueError("out must have unit stride along d and a row stride >= d")
            if on_dev:
                self._on_my_device(out)
        if n == 0:
            self._last["mvn_route"] = "empty"
            return out
        self._call("corrla_mvn_sample_", f.dtype, (n, d, r, _ptr(f), _row_stride(f), _opt_ptr(mu), seed, first, int(lower), _ptr(out),
                   _row_stride(out)), on_dev, f, "mvn")
        return out

    def last_mvn_route(self):
        """The route of this context's last ``mvn_sample`` call: "fused" (the normals of a row tile are generated once into
        LDS and multiplied there), "staged" (r > 288 in float32 / 144 in float64: ``fill_normal`` into a bounded workspace, then the
        back-projection kernel, a row chunk at a time) or "empty" (n = 0: nothing launched); None before the first call."""
        return self._last.get("mvn_route")

    def sandwich_diag(self, jac, cov):
        """The first-order output variances v_i = jac[i] @ cov @ jac[i] -> (m,), on the device (corrla_sandwich_diag_*; the
        diagonal of ``sandwich_prop``, stats_corr.rs:64-68) without the (m, d) temporary jac @ cov: a row tile of jac is
        staged once, multiplied with cov on the MFMAs and contracted with itself in registers.  jac: (m, d), float32 or
        float64, numpy or a CUDA tensor, any row stride (one gradient block of ``poly_eval(..., jac=True)`` as it is); cov:
        (d, d) of the same dtype, d <= 512, used as given -- it is not symmetrised.  Bitwise reproducible.  numpy in -> numpy
        out, a CUDA jac -> a tensor on its device.  ValueError: d > 512, shapes that do not fit, bfloat16 or sparse arguments,
        mismatched dtypes."""
        on_dev = _is_torch(jac) and jac.is_cuda
        j = self._mvn_small(jac, "jac", on_dev)
        if j.ndim != 2 or j.shape[0] == 0 or j.shape[1] == 0:
            raise ValueError(f"jac must be a non-empty (m, d) matrix, got shape {tuple(j.shape)}")
        m, d = (int(v) for v in j.shape)
        if d > L.SANDWICH_MAX_D:
            raise ValueError(f"sandwich_diag: jac has d = {d} features, the kernel takes at most {L.SANDWICH_MAX_D}")
        c = self._mvn_small(cov, "cov", on_dev, j)
        if c.ndim != 2 or tuple(c.shape) != (d, d):
            raise ValueError(f"cov must be ({d}, {d}), got shape {tuple(c.shape)}")
        j, c = _rowmajor(j), _rowmajor(c)
        v = _empty(j, (m,))
        self._call("corrla_sandwich_diag_", j.dtype, (_ptr(j), m, d, _row_stride(j), _ptr(c), _row_stride(c), _ptr(v)), on_dev, j)
        return v

    # ---- op(A) @ X hooks used by tests / bench ----------------------------------------------
    def _run_product(self, name, operand, m, n, xt, trans, beta, in_dtype=None):
        """res = beta * op(A) @ xt through corrla_matmul_dev_* / corrla_spmm_csr_dev_* (`operand`: the arguments that
        describe A); xt a device tensor with as many rows as op(A) has columns; in_dtype: A's dtype where it is not xt's."""
        import torch
        xin, xout = (m, n) if trans else (n, m)
        l = xt.shape[1]
        xc = xt.t().contiguous()  # column-major (xin, l)
        res = torch.empty((l, xout), dtype=xt.dtype, device=xt.device)
        _sync_stream(xt)
        L.check(self._entry(name, True, in_dtype or xt.dtype)(self._h, 1 if trans else 0, *_c_args(operand), xc.data_ptr(), xin, l, float(beta),
                                                  res.data_ptr(), xout))
        return res.t()

    def spmm(self, a_csr, x, trans=False, beta=1.0):
        """res = beta * op(a_csr) @ x for a sparse a_csr (any form _as_csr takes) and a dense x (n x l, or m x l with
        trans); the sparse twin of matmul.  Runs on the device; returns a torch CUDA tensor."""
        import torch
        vals, ci, rp, (m, n), on_dev = _as_csr(a_csr)
        dev = torch.device(f"cuda:{self.device}")
        if not on_dev:
            vals, ci, rp = (torch.from_numpy(v).to(dev) for v in (vals, ci, rp))
        xt = x if _is_torch(x) else torch.as_tensor(np.asarray(x))
        xt = xt.to(device=dev, dtype=vals.dtype)
        if xt.dim() != 2 or xt.shape[0] != (m if trans else n):
            raise ValueError(f"x must have {m if trans else n} rows")
        return self._run_product("corrla_spmm_csr_", (vals, ci, rp, m, n, int(vals.shape[0])),
                                 m, n, xt, trans, beta)

    def matmul(self, a, x, trans=False, beta=1.0):
        """res = beta * op(a) @ x on device tensors (par_matmul_helper, mat_utils.rs:20-33).  A bfloat16 `a` takes a
        float32 `x` and gives a float32 result (corrla_matmul_dev_bf16); a bfloat16 `x` is an error."""
        m, n = a.shape
        if _is_bf16(x):
            raise ValueError("matmul: x must be float32 or float64 (only the matrix a may be bfloat16)")
        if _is_bf16(a):
            if not str(x.dtype).endswith("float32"):
                raise ValueError("matmul: a bfloat16 a takes a float32 x")
            assert x.shape[0] == (m if trans else n)
            return self._run_product("corrla_matmul_", (a, m, n, *a.stride()), m, n, x, trans, beta, in_dtype=a.dtype)
        assert x.shape[0] == (m if trans else n) and x.dtype == a.dtype
        return self._run_product("corrla_matmul_", (a, m, n, *a.stride()), m, n, x, trans, beta)

    # ---- active-subspace gradient stage ---------------------------------------
    def grad_mat(self, x_mat, y, est_order, n_nbrs, x_query=None, *, scale=1.0):
        """``ActiveSsRsvd::create_grad_mat`` with a ``PolyGradientEstimator(x_mat, y, est_order, n_nbrs)``
        (active_subspaces.rs:66-141, 215-229): returns (G, n_regularised) with G the k x n_q gradient matrix (column i =
        gradient at query i; queries default to the support points), scaled by `scale`.  numpy in -> numpy out;
        torch CUDA tensors in -> torch CUDA tensor out (no host copies).  Any number of features and neighbours: calls
        beyond k <= 64 / n_nbrs <= 512 take the wide kernels (see include/corrla_rsvd.h for the remaining limits)."""
        est_order, n_nbrs = int(est_order), int(n_nbrs)
        nreg = C.c_int(0)
        if _is_torch(x_mat) and x_mat.is_cuda:
            import torch
            x = x_mat.to(torch.float64).contiguous()
            yv = (y if _is_torch(y) else torch.as_tensor(np.asarray(y))).to(device=x.device, dtype=torch.float64).reshape(-1).contiguous()
            xq = x if x_query is None else x_query.to(device=x.device, dtype=torch.float64).contiguous()
            if x.dim() != 2 or xq.dim() != 2 or xq.shape[1] != x.shape[1] or yv.numel() != x.shape[0]:
                raise ValueError("x_mat (n, k), y (n,), x_query (n_q, k) expected")
            g = torch.empty((xq.shape[0], x.shape[1]), dtype=torch.float64, device=x.device)
            _sync_stream(x)
            L.check(self._lib.corrla_grad_mat_dev_f64(self._h, x.data_ptr(), x.shape[0], x.shape[1], yv.data_ptr(), xq.data_ptr(),
                                                      xq.shape[0], est_order, n_nbrs, float(scale), g.data_ptr(), x.shape[1],
                                                      C.byref(nreg)))
            return g.t(), nreg.value
        x = np.ascontiguousarray(np.asarray(x_mat, dtype=np.float64))
        yv = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
        xq = x if x_query is None else np.ascontiguousarray(np.asarray(x_query, dtype=np.float64))
        if x.ndim != 2 or xq.ndim != 2 or xq.shape[1] != x.shape[1] or yv.size != x.shape[0]:
            raise ValueError("x_mat (n, k), y (n,), x_query (n_q, k) expected")
        g = np.empty((xq.shape[0], x.shape[1]), dtype=np.float64)
        L.check(self._lib.corrla_grad_mat_f64(self._h, x.ctypes.data, x.shape[0], x.shape[1], yv.ctypes.data, xq.ctypes.data,
                                              xq.shape[0], est_order, n_nbrs, float(scale), g.ctypes.data, x.shape[1],
                                              C.byref(nreg)))
        return g.T, nreg.value

    # ---- power_iter ----------------------------------------------------------------------
    def power_iter(self, a_mat, omega_rank, n_iter, *, seed=None, omega=None, qr=None):
        _reject_bf16(a_mat, "power_iter")
        a = np.asarray(a_mat)
        if a.ndim != 2:
            raise ValueError("a_mat must be 2-D")
        if a.dtype != np.float32:
            a = a.astype(np.float64, copy=False)
        m, n = a.shape
        w = int(omega_rank)
        rs, cs = _strides(a)
        o, keep = self._opts(seed, omega, n, w, a.dtype, False, self._qr_flag(qr))
        q = _empty_colmajor(a, m, max(w, 1))
        fn = self._entry("corrla_power_iter_", False, a.dtype)
        L.check(fn(self._h, a.ctypes.data, m, n, rs, cs, w, int(n_iter), C.byref(o) if o is not None else None,
                   q.ctypes.data, m))
        del keep
        return q

    # ---- low-level hooks used by tests / bench ---------------------------------------------
    def fill_normal(self, t, seed, row0=0, global_cols=None):
        """In-place N(0,1) fill of a 2-D device tensor (random_mat_normal, mat_utils.rs:161-175)."""
        rows, cols = t.shape
        rs, cs = t.stride()
        _sync_stream(t)
        fn = self._entry("corrla_fill_normal_", True, t.dtype)
        L.check(fn(self._h, t.data_ptr(), rows, cols, rs, cs, int(seed), int(row0),
                   int(global_cols if global_cols is not None else cols)))
        return t

    def time_sketch(self, a, x, reps=10):
        """Average duration (ms) of the sketch GEMM Y = A @ X measured with hipEvents on the library's
        stream; returns (ms, Y)."""
        import torch
        m, n = a.shape
        rs, cs = a.stride()
        l = x.shape[1]
        xc = x.t().contiguous()
        y = torch.empty((l, m), dtype=a.dtype, device=a.device)
        ms = C.c_double()
        _sync_stream(a)
        fn = self._entry("corrla_time_sketch_", True, a.dtype)
        L.check(fn(self._h, a.data_ptr(), m, n, rs, cs, xc.data_ptr(), n, l, y.data_ptr(), m, int(reps), C.byref(ms)))
        return ms.value, y.t()


_default = None
_default_lock = threading.Lock()


def default_context():
    global _default
    with _default_lock:
        if _default is None:
            _default = Context(0)
        return _default


def rsvd(a_mat, n_rank, n_iters, n_oversamples, *, seed=None, omega=None, ctx=None, qr=None):
    """corrla_rs.rsvd(a_mat, n_rank, n_iters, n_oversamples) -> (U (m,k), S (k,1), Vt (k,n)).
    src/lib_math_utils_py.rs:21-36.  qr="householder" selects the Householder TSQR thin-Q (default: CholeskyQR2)."""
    return (ctx or default_context()).rsvd(a_mat, n_rank, n_iters, n_oversamples, seed=seed, omega=omega, qr=qr)


def random_svd(a_mat, omega_rank, n_iter, n_oversamples, *, seed=None, omega=None, ctx=None, qr=None):
    """random_svd(a_mat, omega_rank, n_iter, n_oversamples), random_svd.rs:63-66."""
    return rsvd(a_mat, omega_rank, n_iter, n_oversamples, seed=seed, omega=omega, ctx=ctx, qr=qr)


def power_iter(a_mat, omega_rank, n_iter, *, seed=None, omega=None, ctx=None, qr=None):
    """power_iter(a_mat, omega_rank, n_iter) -> Q (m, omega_rank), random_svd.rs:15-18.  `omega_rank` is
    the already-oversampled sketch width."""
    return (ctx or default_context()).power_iter(a_mat, omega_rank, n_iter, seed=seed, omega=omega, qr=qr)


def rpca(a_mat, n_rank, n_iters=None, n_oversamples=None, *, seed=None, omega=None, ctx=None, standardize=False):
    """pyo3 ``rpca(a_mat, n_rank, n_iters, n_oversamples) -> (singular_values (k, 1), components (k, n))``,
    src/lib_math_utils_py.rs:38-55.  Like the reference, the last two positional arguments are accepted and
    IGNORED: PcaRsvd::new hard-codes n_iter = 20 and n_oversamples = min(n_dim, 10) (pca_rsvd.rs:65-66).
    standardize=True (additive, keyword-only): PCA on standardised columns, see Context.pca; same two results."""
    del n_iters, n_oversamples
    if not _check_standardize(standardize):
        _means, s, comps = (ctx or default_context()).pca(a_mat, n_rank, seed=seed, omega=omega)
    else:
        _means, s, comps, _scales = (ctx or default_context()).pca(a_mat, n_rank, seed=seed, omega=omega, standardize=True)
    return s, comps


def normal_stream_host(seed, first, n, r, dtype=np.float64):
    """The library's N(0,1) stream restated in numpy -> (n, r): element (i, j) is the value of counter t = (first + i) r + j
    under `seed` -- one Philox4x32-10 block with key (seed mod 2^32, seed >> 32) and counter (t mod 2^32, t >> 32, 0, 0),
    the uniforms and the cosine branch of Box-Muller as include/corrla_rsvd.h defines them.  The integer part is exact; log,
    sqrt and cos are numpy's, so a value agrees with the device's to a few ulp, not bitwise.  What a host-fitted
    ``PcaRsvd.sample`` draws from."""
    dtype = np.dtype(dtype)
    if dtype not in (np.float32, np.float64):
        raise ValueError(f"dtype must be float32 or float64, got {dtype}")
    n, r, seed, first = int(n), int(r), int(seed), int(first)
    if n < 0 or r < 1 or first < 0 or (first + n) * r >= 1 << 63:
        raise ValueError("need n >= 0, r >= 1, first >= 0 and (first + n) * r < 2^63")
    m32, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    t = (np.uint64(first) + np.arange(n, dtype=np.uint64))[:, None] * np.uint64(r) + np.arange(r, dtype=np.uint64)[None, :]
    c0, c1, c2, c3 = t & m32, t >> sh, np.zeros_like(t), np.zeros_like(t)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2  # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & m32, (p0 >> sh) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    if dtype == np.float64:
        u1 = ((((c0 << sh) | c1) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
        u2 = ((((c2 << sh) | c3) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    else:
        u1 = ((c0 >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
        u2 = ((c1 >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    # cos(2 pi u2) with the argument folded exactly into [0, 1/2] half turns, so that the zeros keep relative accuracy
    x = dtype.type(2.0) * u2
    y = np.where(x > 1.0, dtype.type(2.0) - x, x)
    pi = dtype.type(np.pi)
    c = np.where(y < 0.25, np.cos(pi * y), np.where(y > 0.75, -np.cos(pi * (dtype.type(1.0) - y)), np.sin(pi * (dtype.type(0.5) - y))))
    return (np.sqrt(dtype.type(-2.0) * np.log(u1)) * c).astype(dtype)


class PcaRsvd:
    """Mirror of ``PcaRsvd`` (src/lib_math_utils/pca_rsvd.rs:13-112): fit on construction, keeps the means, the
    singular values (k, 1) and ``components_`` (k, n_dim).  The fit (means, centring, RSVD) runs on the GPU.  A host input
    gives a host-fitted model (numpy arrays) whose apply_tr / apply_inv_tr on numpy arguments are plain numpy on the
    stored k x n_dim factors; a CUDA tensor gives a device-fitted model (``means``, ``pca_s``, ``components_``, ``scales_``
    are tensors on its device).  transform / inverse_transform / residuals / fit_transform, and apply_tr / apply_inv_tr on
    CUDA tensors or on a device-fitted model, run on the GPU (Context.pca_transform / pca_inverse_transform)."""

    def __init__(self, x_mat, rank, *, seed=None, omega=None, ctx=None, standardize=False):
        """standardize=True: the fit is on standardised columns (see Context.pca); ``scales_`` (1, n_dim) keeps the column
        standard deviations (None otherwise), ``components_`` are directions in standardised coordinates, and apply_tr /
        apply_inv_tr divide / multiply by ``scales_`` accordingly."""
        self.pca_rank = int(rank)
        x = x_mat if _is_sparse(x_mat) or (_is_torch(x_mat) and x_mat.is_cuda) else np.asarray(x_mat)
        self._ctx = ctx
        self.n_samples = int(x[3][0] if isinstance(x, tuple) else x.shape[0])
        self.scales_ = None
        if not _check_standardize(standardize):
            self.means, self.pca_s, self.components_ = (ctx or default_context()).pca(x, rank, seed=seed, omega=omega)
        else:
            self.means, self.pca_s, self.components_, self.scales_ = (ctx or default_context()).pca(x, rank, seed=seed, omega=omega,
                                                                                                    standardize=True)

    def fit(self, x_mat, rank, **kw):  # pca_rsvd.rs:85-88
        self.__init__(x_mat, rank, **kw)

    def explained_var(self):  # pca_rsvd.rs:91-99: s^2 / (n_samples - 1)
        return self.pca_s * self.pca_s / (self.n_samples - 1.0)

    def components(self):
        return self.components_

    def singular_values(self):
        return self.pca_s

    # ---- the model applied on the device ----------------------------------------------------------------------------
    def _context(self):
        return self._ctx or default_context()

    def _on_device(self, arg):
        """the device path serves CUDA arguments and every argument of a device-fitted model"""
        return (_is_torch(arg) and arg.is_cuda) or _is_torch(self.components_)

    def transform(self, x_mat):
        """Scores of x_mat under the fitted model, centred by the MODEL's means (scikit-learn's transform): (m, k)."""
        return self._context().pca_transform(x_mat, self.means, self.components_, self.scales_)

    def inverse_transform(self, red_mat):
        """(m, k) scores back to (m, n_dim): (red_mat @ components_) * scales_ + means."""
        return self._context().pca_inverse_transform(red_mat, self.means, self.components_, self.scales_)

    def residuals(self, x_mat):
        """Q / SPE statistic of every sample of x_mat under the fitted model: (m,), see Context.pca_transform."""
        return self._context().pca_transform(x_mat, self.means, self.components_, self.scales_, residuals=True)[1]

    def fit_transform(self, x_mat, rank, **kw):
        """fit(x_mat, rank, **kw), then the scores of x_mat."""
        self.fit(x_mat, rank, **kw)
        return self.transform(x_mat)

    def sample(self, n, *, seed=None, first=0):
        """n draws from the fitted model, (n, n_dim): means + scales_ * ((z * pca_s / sqrt(n_samples - 1)) @ components_) with
        z (n, k) the rows [first, first + n) of the library's N(0,1) stream under `seed` (width k; include/corrla_rsvd.h) --
        the Gaussian whose covariance is the model's rank-k estimate.  A device-fitted model draws z with
        ``Context.fill_normal`` and back-projects with ``Context.pca_inverse_transform``: k is small and n_dim may be large,
        which is that kernel's shape.  A host-fitted model does the same in numpy (``normal_stream_host``), like apply_inv_tr.
        seed=None takes a fresh one from ``numpy.random.SeedSequence``."""
        n, first = int(n), int(first)
        if n < 0 or first < 0:
            raise ValueError(f"n and first must be >= 0, got n = {n}, first = {first}")
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
        k = int(self.components_.shape[0])
        if _is_torch(self.components_):
            import torch
            comps = self.components_
            z = torch.empty((n, k), dtype=comps.dtype, device=comps.device)
            if n == 0:
                return torch.empty((0, int(comps.shape[1])), dtype=comps.dtype, device=comps.device)
            self._context().fill_normal(z, seed, row0=first, global_cols=k)
            L.check(self._context()._lib.corrla_ctx_synchronize(self._context()._h))  # fill_normal only enqueues
            sig = (self.pca_s.reshape(1, -1) / float(np.sqrt(self.n_samples - 1.0))).to(comps.dtype)
            return self.inverse_transform(z * sig)
        dt = self.components_.dtype
        z = normal_stream_host(seed, first, n, k, dt)
        sig = (np.asarray(self.pca_s, dtype=dt).reshape(1, -1) / dt.type(np.sqrt(self.n_samples - 1.0))).astype(dt)
        return self.apply_inv_tr(z * sig)

    def apply_tr(self, targ_mat):  # pca_rsvd.rs:43-46: centres the TARGET by its own column means
        if self._on_device(targ_mat):
            return self._context().pca_transform(targ_mat, None, self.components_, self.scales_, own_means=True)[0]
        t = np.asarray(targ_mat, dtype=self.components_.dtype)
        tc = t - t.mean(axis=0, keepdims=True)
        if self.scales_ is not None:
            tc = tc / self.scales_
        return tc @ self.components_.T

    def apply_inv_tr(self, red_mat):  # pca_rsvd.rs:49-52
        if self._on_device(red_mat):
            return self.inverse_transform(red_mat)
        back = np.asarray(red_mat, dtype=self.components_.dtype) @ self.components_
        if self.scales_ is not None:
            back = back * self.scales_
        return back + self.means


def algorithmic_flops(m, n, k, q, p):
    """(4q+4) m n l + 2 m l^2 + (1 + max(0, q-3)) (4 m l^2 - 4/3 l^3), unpadded l."""
    if m < n:
        m, n = n, m
    l = min(k + p, n)
    return (4 * q + 4) * m * n * l + 2.0 * m * l * l + (1 + max(0, q - 3)) * (4.0 * m * l * l - 4.0 / 3.0 * l ** 3)
