"""One GPU case per route thinq_plan.hpp can select (run with -m gpu on an MI355X): the single factor kernel with the
products in place (l <= 144) and with conditional passes in pairs (145 ...), the 2 x 2 blocked factor (f32 177 ... 352, f64
153 ... 304) and the host-controlled loop beyond it, each at the widths on both sides of the switch, on a flat and on a
0.7^i spectrum (the latter makes the context escalate to the conditional passes).  The inputs are those of
tests/test_driver_emu.py::_thin_q_route_input.  What pins the ROUTE is qr_passes: a sketch that silently fell back to the
host-controlled loop would still give the right S, but not the same count.

`python tests/test_gpu_thinq_routes.py` prints the table below from the library that is built (the generator)."""
import functools

import numpy as np
import pytest

from oracle import rsvd_oracle as orc
from tests.helpers import orth_err
from tests.test_driver_emu import _thin_q_route_input

# (dtype, l, spectrum, qr_passes).  qr_passes as measured on an MI355X on commit 5f6dc07 (the parent of the commit that
# moved the stage into thinq_plan.hpp / thinq_stage.hpp), every row, with the generator at the end of this file.  Not
# the emulation's counts: f32 rounding on the device may run a conditional pass the f64-exact host arithmetic does not.
_ROUTES = [
    (np.float32, 9, "flat", 5), (np.float32, 9, "decay", 5),
    (np.float32, 144, "flat", 6), (np.float32, 144, "decay", 11),
    (np.float32, 145, "flat", 6), (np.float32, 145, "decay", 11),
    (np.float32, 176, "flat", 6), (np.float32, 176, "decay", 12),
    (np.float32, 177, "flat", 6), (np.float32, 177, "decay", 13),
    (np.float32, 352, "flat", 7), (np.float32, 352, "decay", 12),
    (np.float32, 353, "flat", 5), (np.float32, 353, "decay", 9),
    (np.float64, 152, "flat", 5), (np.float64, 152, "decay", 10),
    (np.float64, 153, "flat", 5), (np.float64, 153, "decay", 10),
    (np.float64, 304, "flat", 5), (np.float64, 304, "decay", 10),
    (np.float64, 305, "flat", 5), (np.float64, 305, "decay", 7),
]


@functools.lru_cache(maxsize=None)
def _case(dtype, l, spectrum):
    a, om = _thin_q_route_input(dtype, l, spectrum)
    k = l - 2
    _, so, _ = orc.random_svd(a, k, 0, 2, omega=om)
    return a, om, k, so


def _run(dtype, l, spectrum):
    import corrla_rs_amd as cr
    a, om, k, so = _case(dtype, l, spectrum)
    ctx = cr.Context(0)  # a fresh context: two unconditional passes enqueued, no more
    u, s, vt = ctx.rsvd(a, k, 0, 2, omega=om)
    return a, so, u, s, vt, int(ctx.timings()["qr_passes"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,l,spectrum,passes", _ROUTES)
def test_thin_q_route_per_width_on_the_device(dtype, l, spectrum, passes):
    a, so, u, s, vt, got = _run(dtype, l, spectrum)
    m, n = a.shape
    eps = np.finfo(dtype).eps
    ds = float(np.max(np.abs(s.ravel().astype(np.float64) - so.ravel())) / so[0, 0])
    print(f"{np.dtype(dtype).name} l={l} {spectrum}: qr_passes {got}, max|dS|/s1 {ds:.3g}, orth U {orth_err(u):.3g} "
          f"V {orth_err(vt.T):.3g} (bound {200 * eps * np.sqrt(m):.3g})")
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(s)) and np.all(np.isfinite(vt))
    assert ds <= (3e-5 if dtype == np.float32 else 1e-10)
    assert orth_err(u) <= 200 * eps * np.sqrt(m) and orth_err(vt.T) <= 200 * eps * np.sqrt(n)
    assert got == passes


if __name__ == "__main__":
    for dtype, widths in ((np.float32, (9, 144, 145, 176, 177, 352, 353)), (np.float64, (152, 153, 304, 305))):
        for l in widths:
            row = [f'(np.{np.dtype(dtype).name}, {l}, "{sp}", {_run(dtype, l, sp)[-1]})' for sp in ("flat", "decay")]
            print("    " + ", ".join(row) + ",", flush=True)
