"""What the host tests of the Python entry layer put in the library's place: a ``Context`` made without a device, a recorder
where its entries would be and a fake library behind ``_lib``.  A plain helper module: every ``*_host.py`` file builds its own
``stub`` fixture from ``make_stub`` with what its entries need answered."""
import ctypes as C

import numpy as np

from corrla_rs_amd import _lib as L
from corrla_rs_amd import api


class Recorder:
    """stands where an entry would be: keeps its arguments and reports `rc` (success, unless a test sets another code)"""

    def __init__(self, route_out=None):
        self.calls = []
        self.peek = {}     # argument index -> (ctypes type, count): arrays to copy while the call's temporaries are alive
        self.seen = {}
        self.log = []      # "entry" for every call of the recorder, the symbol for every other call of the fake library, in order
        self.rc = L.OK
        self.route_out = route_out   # what the entry writes through its own trailing int* route_out (corrla_cov_*)

    def __call__(self, *args):
        self.calls.append(args)
        self.log.append("entry")
        self.seen = {i: np.ctypeslib.as_array(C.cast(args[i], C.POINTER(ct)), shape=(cnt,)).copy() for i, (ct, cnt) in self.peek.items()}
        if self.route_out is not None:
            args[-1]._obj.value = self.route_out
        return self.rc


class FakeLib:
    """stands behind ``Context._lib``: corrla_ctx_synchronize succeeds, a corrla_ctx_last_* function named in `last` fills its
    out-parameters with the values given there (any other one is missing, as in a library without it), and every other
    corrla_* symbol is the recorder under that name -- what the entries called as ``self._lib.corrla_...`` meet."""

    def __init__(self, rec, names, last):
        self.rec, self.names, self.last = rec, names, dict(last or {})

    def corrla_last_error(self):
        return b"what the fake library says"

    def __getattr__(self, name):
        if not name.startswith("corrla_") or (name.startswith("corrla_ctx_last_") and name not in self.last):
            raise AttributeError(name)

        def fn(*args):
            if name == "corrla_ctx_synchronize":
                self.rec.log.append(name)
                return L.OK
            if name in self.last:
                self.rec.log.append(name)
                for out, v in zip(args[1:], self.last[name]):
                    out._obj.value = v
                return L.OK
            self.names.append(name)
            return self.rec(*args)
        return fn


def make_stub(last=None, route_out=None):
    """-> (context, recorder, names): a Context with no device and no library.  `names` collects the symbol of every entry
    asked for, through ``_entry`` or from the fake library; `last`: {corrla_ctx_last_* name: the values it reports};
    `route_out`: see Recorder."""
    c = api.Context.__new__(api.Context)   # no device, no library
    rec = Recorder(route_out)
    names = []
    c._lib, c._h, c.device = FakeLib(rec, names, last), None, 0

    def entry(stem, on_device, dtype):
        names.append(stem + ("dev_" if on_device else "") + api._suffix(dtype))
        return rec
    c._entry = entry
    return c, rec, names


def last_records(c):
    """every ``last_*`` accessor of the context, by name"""
    return {"cov_route": c.last_cov_route(), "pca_apply_route": c.last_pca_apply_route(),
            "pca_apply_centring": c.last_pca_apply_centring(), "polyfit_route": c.last_polyfit_route(),
            "kde_route": c.last_kde_route(), "dirichlet_route": c.last_dirichlet_route(),
            "dirichlet_readbacks": c.last_dirichlet_readbacks(), "mvn_route": c.last_mvn_route(),
            "solve_route": c.last_solve_route, "solve_info": c.last_solve_info,
            "chol_route": c.last_chol_route, "chol_info": c.last_chol_info}


def on_gpu(torch, index, shape, dtype=None):
    """What api looks at of a CUDA tensor before it touches the device, without a GPU: enough for the errors that name the
    device, and nothing that could be computed with."""
    class OnGpu:
        is_cuda, ndim = True, len(shape)

        def __init__(self):
            self.device, self.shape, self.dtype = torch.device("cuda", index), tuple(shape), dtype or torch.float64

        def detach(self):
            return self

        def dim(self):
            return len(shape)

        def stride(self, i=None):
            return 1
    OnGpu.__module__ = "torch"
    return OnGpu()
