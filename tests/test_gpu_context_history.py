"""GPU test (run with -m gpu on an MI355X): what a Context carries from one call to the next.

  a. kNeedV      the W-only shortcut of the multi-workgroup Jacobi chosen from the diagonal and refused by the computed sigma
                 (fail 4): the call repeats with V accumulated, and the context keeps accumulating V
  b. kMoreSweeps too few sweeps enqueued (fail 1): the call repeats with more, and returns the bits of an undisturbed call
  c. the sweep hint: a call after a one-sweep call enqueues three sweeps, fails, repeats -- same bits again
  d. order independence: a dozen calls of every entry kind, each behind a call of another kind that leaves 1e18-sized
     values or an error's debris in the workspace, reproduce the bits they give alone on a fresh context
  e. the enqueue-only entries back to back without a synchronisation in between

Every test creates its own Context(0) and closes it: these calls change a context for good.  The routes are pinned through
the CORRLA_DEBUG lines of driver.hpp (status record ... (core SVD): fail F) and core_svd_stage.hpp (jacobi_svd
(multi-workgroup, N sweeps enqueued, W only | V accumulated) ... sweeps run=R); a test that has not seen the verdicts it
is about fails.  The bitwise comparisons rest on the library's fixed summation order: a difference means that a call
read something it did not write, or that its result depends on the context's history."""
import re

import numpy as np
import pytest

from oracle import rsvd_oracle as orc
from tests import core_cases as cc
from tests.test_gpu_core_svd_routes import route_case

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
_IDS = ["f32", "f64"]
_SVD_LINE = re.compile(r"jacobi_svd \(multi-workgroup, (\d+) sweeps enqueued, (W only|V accumulated)\).*? sweeps run=(\d+)")
_REC_LINE = re.compile(r"status record \d+ \(core SVD\): fail (\d+)")


@pytest.fixture
def ctx():
    import corrla_rs_amd as cr
    c = cr.Context(0)
    yield c
    c.close()


def _fresh(call):
    import corrla_rs_amd as cr
    c = cr.Context(0)
    try:
        return call(c)
    finally:
        c.close()


def attempts(err):
    """The optimistic attempts of one call, from its debug lines: [(sweeps enqueued, mode, sweeps run, fail)].  fail is None
    for an attempt that was abandoned before its core-SVD record was judged (an earlier record decided)."""
    out = []
    for line in err.splitlines():
        m = _SVD_LINE.search(line)
        if m:
            out.append([int(m.group(1)), m.group(2), int(m.group(3)), None])
            continue
        m = _REC_LINE.search(line)
        if m:
            assert out and out[-1][3] is None, err
            out[-1][3] = int(m.group(1))
    return [tuple(a) for a in out if a[3] is not None]


def _same_bits(x, y):
    return all(np.asarray(a).dtype == np.asarray(b).dtype and np.asarray(a).shape == np.asarray(b).shape and
               np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(x, y)) and len(x) == len(y)


def _oracle_bound(a, k, q, p, om, s):
    so = orc.random_svd(a, k, q, p, omega=om)[1].ravel()
    assert np.max(np.abs(s.ravel().astype(np.float64) - so)) <= (3e-5 if a.dtype == np.float32 else 1e-10) * so[0]


# ---- a. kNeedV -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
@pytest.mark.parametrize("l", [96, 138, 288])
def test_w_only_refused_by_sigma_repeats_with_v_and_the_context_keeps_v(ctx, monkeypatch, capfd, l, dtype):
    monkeypatch.setenv("CORRLA_DEBUG", "1")
    c = cc.case("equicorr", l, dtype)
    a, k, q, p = c.args
    capfd.readouterr()
    u, s, vt = ctx.rsvd(a, k, q, p, omega=c.omega)
    att = attempts(capfd.readouterr().err)
    # force_v stays set: a Gaussian call on the same context accumulates V from its first attempt
    a2, k2, q2, p2, om2 = route_case(138, dtype)
    u2, s2, vt2 = ctx.rsvd(a2, k2, q2, p2, omega=om2)
    att2 = attempts(capfd.readouterr().err)
    print("equicorr(%.2f) l=%d %s:" % (cc.EQUICORR_RHO, l, np.dtype(dtype).name), att, "then route_case(138):", att2)
    assert [(mode, fail) for _, mode, _, fail in att] == [("W only", 4), ("V accumulated", 0)], att
    cc.check(c, u, s, vt, "kNeedV")
    assert att2 and all(mode == "V accumulated" for _, mode, _, _ in att2) and att2[-1][3] == 0, att2
    assert np.all(np.isfinite(u2)) and np.all(np.isfinite(vt2))
    _oracle_bound(a2, k2, q2, p2, om2, s2)


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_w_only_kept_in_one_attempt_when_sigma_confirms_it(ctx, monkeypatch, capfd, dtype):
    monkeypatch.setenv("CORRLA_DEBUG", "1")
    c = cc.case("equicorr_kept", 138, dtype)
    a, k, q, p = c.args
    capfd.readouterr()
    u, s, vt = ctx.rsvd(a, k, q, p, omega=c.omega)
    err = capfd.readouterr().err
    att = attempts(err)
    print("equicorr(%.2f) l=138 %s:" % (cc.EQUICORR_RHO_KEPT, np.dtype(dtype).name), att)
    assert len(_SVD_LINE.findall(err)) == 1 and [(mode, fail) for _, mode, _, fail in att] == [("W only", 0)], att
    cc.check(c, u, s, vt, "W-only kept")


# ---- b. kMoreSweeps, c. the sweep hint -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def undisturbed():
    """route_case(138) on a fresh context with an empty environment, once per element type: the bits b and c must reproduce."""
    out = {}
    for dtype in DTYPES:
        a, k, q, p, om = route_case(138, dtype)
        out[np.dtype(dtype).name] = _fresh(lambda c: c.rsvd(a, k, q, p, omega=om))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_too_few_sweeps_repeat_with_more_and_give_the_undisturbed_bits(ctx, monkeypatch, capfd, undisturbed, dtype):
    """Sweeps past convergence are launches that test a flag, and nothing else in the repeated attempt differs."""
    a, k, q, p, om = route_case(138, dtype)
    monkeypatch.setenv("CORRLA_DEBUG", "1")
    monkeypatch.setenv("CORRLA_JMC_SWEEPS", "2")
    capfd.readouterr()
    got = ctx.rsvd(a, k, q, p, omega=om)
    att = attempts(capfd.readouterr().err)
    print("CORRLA_JMC_SWEEPS=2, route_case(138) %s:" % np.dtype(dtype).name, att)
    fails = [fail for _, _, _, fail in att]
    assert len(fails) >= 2 and fails[-1] == 0 and all(f == 1 for f in fails[:-1]), att
    assert att[0][0] == 2 and all(y[0] == x[0] + 8 for x, y in zip(att, att[1:])), att   # 8 more sweeps per verdict
    _oracle_bound(a, k, q, p, om, got[1])
    assert _same_bits(got, undisturbed[np.dtype(dtype).name])


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_a_hard_call_after_a_one_sweep_call_fails_its_hint_and_gives_the_undisturbed_bits(ctx, monkeypatch, capfd, undisturbed, dtype):
    """The diagonal core converges in its first sweep, the hint becomes 1 and the Gaussian call enqueues min(default, 1 + 2)
    sweeps where a flat spectrum needs 7 - 8."""
    monkeypatch.setenv("CORRLA_DEBUG", "1")
    c = cc.case("scaled_perm_diag", 138, dtype)
    a1, k1, q1, p1 = c.args
    capfd.readouterr()
    u1, s1, vt1 = ctx.rsvd(a1, k1, q1, p1, omega=c.omega)
    att1 = attempts(capfd.readouterr().err)
    a, k, q, p, om = route_case(138, dtype)
    got = ctx.rsvd(a, k, q, p, omega=om)
    att = attempts(capfd.readouterr().err)
    cc.check(c, u1, s1, vt1, "cheap call")
    print("scaled_perm_diag l=138 %s:" % np.dtype(dtype).name, att1, "then route_case(138):", att)
    # measured on the MI355X: the diagonal core 10 (f32) / 13 (f64) sweeps enqueued, 1 run; the Gaussian call 3 enqueued and
    # all 3 run (fail 1), then 18 / 21 enqueued and 7 / 8 run -- what a fresh context's 10 / 13 give it, to the bit
    default = 10 if dtype == np.float32 else 13
    assert att1 ==[(default, "V accumulated", 1, 0)], att1              # one attempt, one sweep: nothing to rotate
    assert [(nsw, fail) for nsw, _, _, fail in att] == [(3, 1), (default + 8, 0)], att
    _oracle_bound(a, k, q, p, om, got[1])
    assert _same_bits(got, undisturbed[np.dtype(dtype).name])


# ---- d. order independence -------------------------------------------------------------------------------------------
def _csr(rng, m, n, density, dtype):
    dense = rng.standard_normal((m, n)) * (rng.random((m, n)) < density)
    indptr = np.concatenate([[0], np.cumsum((dense != 0).sum(axis=1))]).astype(np.int64)
    rows, cols = np.nonzero(dense)
    return (dense[rows, cols].astype(dtype), cols.astype(np.int32), indptr, (m, n))


def _listed_calls(torch):
    """name -> call(ctx) -> tuple of numpy arrays.  Shapes: the smallest of each feature's own GPU test file."""
    rng = np.random.default_rng(2024)
    calls = {}
    for dtype, tag in zip(DTYPES, _IDS):
        for l in (24, 138, 300):
            a, k, q, p, om = route_case(l, dtype)
            calls["rsvd-%s-l%d" % (tag, l)] = (lambda c, a=a, k=k, q=q, p=p, om=om: c.rsvd(a, k, q, p, omega=om))
    csr = _csr(rng, 333, 130, 0.05, np.float64)
    om_csr = rng.standard_normal((130, 17))
    calls["rsvd-csr"] = lambda c: c.rsvd(csr, 10, 2, 7, omega=om_csr)
    a16 = torch.tensor(rng.standard_normal((256, 32)), dtype=torch.bfloat16)
    om16 = rng.standard_normal((32, 16)).astype(np.float32)
    calls["rsvd-bf16"] = lambda c: c.rsvd(a16, 8, 1, 8, omega=om16)
    x = rng.standard_normal((1031, 77)) * (0.9 ** np.arange(77)) * 10.0 ** rng.integers(-2, 3, 77) + rng.standard_normal(77)
    om_pca = rng.standard_normal((77, 15))
    calls["pca-standardize"] = lambda c: c.pca(x, 5, 3, 10, omega=om_pca, standardize=True)
    x32 = x.astype(np.float32)
    calls["cov-correlation"] = lambda c: c.cov(x32, correlation=True)
    comps = np.linalg.qr(rng.standard_normal((77, 6)))[0].T
    means, scales = x.mean(axis=0), x.std(axis=0, ddof=1)
    calls["pca-transform-residuals"] = lambda c: c.pca_transform(x, means, comps, scales, residuals=True)
    xq, xs, w = rng.standard_normal((200, 3)), rng.standard_normal((150, 3)), rng.standard_normal((154, 2))
    calls["rbf-apply"] = lambda c: (c.rbf_apply(xq, xs, w, 4, 1.0, poly_degree=1),)
    xp, yp, coef = rng.standard_normal((500, 3)), rng.standard_normal((500, 2)), rng.standard_normal((10, 2))
    calls["polyfit"] = lambda c: c.polyfit_gram(xp, yp, 2) + c.poly_eval(xp, coef, 2, jac=True)
    xg = rng.standard_normal((300, 4))
    yg = np.sin(xg @ np.array([1.0, -0.5, 0.25, 2.0]))
    calls["grad-mat"] = lambda c: (c.grad_mat(xg, yg, 1, 12, xg[:20])[0],)
    xsp, ysp = rng.standard_normal((130, 17)), rng.standard_normal((333, 17))
    calls["spmm"] = lambda c: (c.spmm(csr, xsp).cpu().numpy(), c.spmm(csr, ysp, trans=True).cpu().numpy())
    am = torch.tensor(rng.standard_normal((300, 70)), dtype=torch.float32, device="cuda")
    xm = torch.tensor(rng.standard_normal((70, 5)), dtype=torch.float32, device="cuda")
    ym = torch.tensor(rng.standard_normal((300, 5)), dtype=torch.float32, device="cuda")
    calls["matmul"] = lambda c: (c.matmul(am, xm).cpu().numpy(), c.matmul(am, ym, trans=True).cpu().numpy())
    return calls


def _dirtying_calls():
    """Three calls that leave the workspace in a state no fresh context is in.
    huge:      a finite f32 rsvd on 20000 rows and l = 64, so that its m x l buffers (5 MB) take the alloc_bytes route of
               alloc_skinny_out.  Its columns have norm 3e18 and its entries 2e16, not 1e18: the Gram matrices of a thin-Q
               (9e36) are the largest f32 holds, and 20000 entries of 1e18 per column would put them at 2e40
    nan:       the NaN input of test_non_finite_input_is_an_error_not_garbage, which ends in CORRLA_ENUMERIC
    transform: a finite f32 pca_transform of 20000 x 64 entries of magnitude 1e18 (centred copy in workspace, scores of
               1e18): the call of another kind that goes in front of the listed rsvd calls"""
    from corrla_rs_amd._lib import CorrlaError
    rng = np.random.default_rng(18)
    m, n, l = 20000, 80, 64
    big = (3e18 * np.linalg.qr(rng.standard_normal((m, n)))[0]).astype(np.float32)
    om = np.linalg.qr(rng.standard_normal((n, l)))[0].astype(np.float32)
    bad = np.ones((64, 32))
    bad[3, 5] = np.nan
    x18 = (1e18 * rng.standard_normal((m, 64))).astype(np.float32)
    mu18 = (1e17 * rng.standard_normal(64)).astype(np.float32)
    comps = np.linalg.qr(rng.standard_normal((64, 8)))[0].T.astype(np.float32)

    def huge(c):
        u, s, vt = c.rsvd(big, l - 8, 0, 8, omega=om)
        assert np.all(np.isfinite(s)) and abs(float(s[0, 0]) / 3e18 - 1) < 1e-3

    def nan(c):
        with pytest.raises(CorrlaError) as e:
            c.rsvd(bad, 4, 2, 4)
        assert e.value.code == 5

    def transform(c):
        t = c.pca_transform(x18, mu18, comps, center="copy")
        assert np.all(np.isfinite(t)) and 1e17 < float(np.abs(t).max()) < 1e20

    return huge, nan, transform


@pytest.fixture(scope="module")
def listed():
    import torch
    assert torch.cuda.is_available()
    calls = _listed_calls(torch)
    alone = {name: tuple(np.array(v, copy=True) if v is not None else np.zeros(0) for v in _fresh(call)) for name, call in calls.items()}
    return calls, alone


def test_the_list_covers_every_entry_kind(listed):
    calls, alone = listed
    assert len(calls) == 16 and set(alone) == set(calls)
    for name, res in alone.items():
        assert res and all(np.all(np.isfinite(v)) for v in res), name


@pytest.mark.parametrize("seed", [1, 2])
def test_every_call_reproduces_its_fresh_context_bits_in_any_order_on_a_dirty_context(ctx, listed, seed):
    calls, alone = listed
    huge, nan, transform = _dirtying_calls()
    order = [sorted(calls)[i] for i in np.random.default_rng(seed).permutation(len(calls))]
    differ = []
    for i, name in enumerate(order):
        # the call right in front is of another kind: the listed rsvd calls get the transform (every other time behind the NaN
        # rsvd, whose debris it does not clear), every other entry the huge or the NaN rsvd in turn
        if name.startswith("rsvd"):
            if (i + seed) % 2:
                nan(ctx)
            transform(ctx)
        else:
            (huge, nan)[(i + seed) % 2](ctx)
        got = tuple(v if v is not None else np.zeros(0) for v in calls[name](ctx))
        if not _same_bits(got, alone[name]):
            differ.append((i, name, ["%.3e" % float(np.max(np.abs(np.asarray(g, np.float64) - np.asarray(r, np.float64))))
                                     for g, r in zip(got, alone[name])]))
    assert not differ, (order, differ)


# ---- e. enqueue-only entries back to back ----------------------------------------------------------------------------
class _NoSynchronize:
    """The library as a Context sees it, with corrla_ctx_synchronize turned into a count: the device entries of cov,
    pca_transform / inverse, rbf_* and polyfit_* "enqueue and return; the arena is reused by later calls in stream order"."""

    def __init__(self, lib):
        self._lib, self.skipped = lib, 0

    def __getattr__(self, name):
        if name == "corrla_ctx_synchronize":
            return self._skip
        return getattr(self._lib, name)

    def _skip(self, handle):
        self.skipped += 1
        return 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_IDS)
def test_enqueue_only_entries_back_to_back_equal_the_synchronised_calls(ctx, dtype):
    """Every operand is a CUDA tensor already in the layout its entry reads, so that the Python layer makes no temporary
    and launches nothing on torch's stream between the calls: all the library's stream sees is six calls in a row."""
    import torch
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    rng = np.random.default_rng(5)

    def dev(v, dt=tdt):
        return torch.tensor(np.asarray(v), dtype=dt, device="cuda")

    x = dev(rng.standard_normal((1031, 77)) * (0.9 ** np.arange(77)) + rng.standard_normal(77))
    means, s, comps, scales = ctx.pca(x, 6, 3, 10, seed=3, standardize=True)      # the model, column-major as the entries read it
    scores = ctx.pca_transform(x, means, comps, scales)
    xq, xs, w = dev(rng.standard_normal((200, 3))), dev(rng.standard_normal((150, 3))), dev(rng.standard_normal((154, 2)))
    xp, yp = dev(rng.standard_normal((500, 3))), dev(rng.standard_normal((500, 2)))
    coef = dev(rng.standard_normal((10, 2)), torch.float64)
    torch.cuda.synchronize()

    def run(c):
        out = []
        out += c.cov(x, correlation=True)
        out += c.pca_transform(x, means, comps, scales, residuals=True)
        out += [c.pca_inverse_transform(scores, means, comps, scales)]
        out += [c.rbf_apply(xq, xs, w, 4, 1.0, poly_degree=1)]
        out += c.polyfit_gram(xp, yp, 2)
        out += c.poly_eval(xp, coef, 2, jac=True)
        return out

    want = [t.cpu().numpy() for t in run(ctx)]
    real = ctx._lib
    ctx._lib = proxy = _NoSynchronize(real)
    try:
        pending = run(ctx)
    finally:
        ctx._lib = real
    assert proxy.skipped == 6
    from corrla_rs_amd import _lib as L
    L.check(real.corrla_ctx_synchronize(ctx._h))
    got = [t.cpu().numpy() for t in pending]
    assert all(np.all(np.isfinite(v)) for v in want)
    differ = [i for i, (g, r) in enumerate(zip(got, want)) if not _same_bits((g,), (r,))]
    assert not differ and len(got) == len(want) == 12, differ
