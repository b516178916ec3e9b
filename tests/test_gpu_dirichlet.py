"""corrla_dirichlet_draws_* / corrla_dirichlet_sample_* on the GPU against the numpy restatement of the stream
(tests/dirichlet_reference.py, judged against the distribution by tests/test_dirichlet_host.py on the CPU); the shape tables
come from tests/test_dirichlet_plan.py.

THE TOLERANCE of a row, derived from the operation order of the stream (include/corrla_rsvd.h), not from what the device gives.
Device and restatement run the same IEEE operations in the same order on the same uniforms (the Philox words are integers:
equal bits); they differ only in the library functions log, sqrt, cospi and pow.  With every library value within L = 2 ulp of
the truth (u = 2^-53) and every other operation rounded once, to first order:
  alpha = 1   g = -log(u1): L.
  otherwise   z = sqrt(-2 log u1) cospi(2 u2): log L, halved by the root, the root L, cospi L, the product 1/2 -- L / 2 + 2 L + 1/2,
              another 1/2 for C z; w = 1 + C z keeps that absolute error, (5/2 L + 1) |w - 1| / w relative to w, plus 1/2; the cube
              triples it; two more products for (w w) w and D v: e_g = 3 ((5/2 L + 1) |w - 1| / w + 1/2) + 3/2, which depends on the
              draw (a draw with w near 0 is a tiny gamma with a large relative error); alpha < 1 adds pow and a product: L + 1/2.
  the row     S adds the e_g weighted by g_i / S and (d - 1) / 2 for its additions; x_j = (c g_j) / S adds 1 for its two operations:
              e_x[j] = e_g[j] + sum_i (g_i / S) e_g[i] + (d - 1) / 2 + 1.
The restatement returns e_x per element (`relerr`); tests/test_dirichlet_host.py holds the restatement itself against a
50-digit mpmath evaluation of the same draws and finds it inside e_x, so e_x is the larger of the two.  The device gets a
factor 4 for a math library that may differ from numpy's by an ulp or two per call:  |x_dev - x| <= 4 e_x u x.
The measured error is printed by every case (pytest -s) and recorded in profiles/dirichlet.jsonl by tools/bench_dirichlet.py.

A row may disagree outright only if an attempt was accepted on one side and rejected on the other, or a draw was inside the
box on one side only.  The seeds below give the restatement no attempt with an acceptance margin below 10^-9 and no examined draw
with a component x_j within 10^-9 x_j of a bound -- asserted in every case -- so the allowed number of such rows is zero, and
accepted draw indices, n_found and n_drawn are compared exactly.  (The distance to a bound is taken relative to x_j because the
error of x_j is relative, some 10^-14 x_j: box C has lower bounds of 0 and alpha_j = 0.3, where one draw in 500 has x_j < 10^-9
and no seed could keep every draw 10^-9 away from 0 in absolute terms, while no positive x_j can cross 0.)"""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

from tests import dirichlet_reference as R
from tests.test_dirichlet_plan import BOXES, FIRST_BATCH, GPU_CALLS, MIXED5, RANGE, REG_D, SAMPLE_CHUNK, SAMPLE_N, URANIUM_BOX

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
DEVICE_FACTOR = 4.0
MARGIN = 1e-9
DRAW_SEED = 20241008
BOX_SEEDS = {"A": 101, "B": 102, "C": 103, "D": 104}
KINDS = ("host", "dev")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx():
    import corrla_rs_amd as cr
    c = cr.Context(0)
    yield c
    c.close()


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


@functools.lru_cache(maxsize=None)
def ref_draws(alphas, n, first, c_scale=1.0, seed=DRAW_SEED):
    out = R.draws(first, n, alphas, c_scale, seed, full=True)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_sample(box, n_samples=SAMPLE_N, chunk=SAMPLE_CHUNK, max_zshots=500, c_scale=1.0):
    bounds, alphas, _ = BOXES[box]
    b = np.asarray(bounds) * c_scale
    out = R.sample(b, n_samples, alphas, c_scale, BOX_SEEDS[box], max_zshots, chunk, full=True)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def assert_rows_agree(got, want, rel, what):
    got = _np(got)
    err = np.abs(got - want)
    bound = DEVICE_FACTOR * rel * U * want
    ratio = float(np.max(err / bound)) if err.size else 0.0
    print(f"{what}: max |x_dev - x| / x = {float(np.max(err / want)) / U:.2f} u, {ratio:.3f} of the bound")
    assert np.all(err <= bound), (what, ratio)


# ---- 1. draws against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("alphas,n,first", GPU_CALLS, ids=lambda v: f"d{len(v)}a{v[0]}+{v[-1]}" if isinstance(v, tuple) else str(v))
def test_draws_agree_with_the_restatement(ctx, torch, alphas, n, first, kind):
    want, margin, rel = ref_draws(alphas, n, first)
    assert margin.min() >= MARGIN, "choose another seed: an attempt of the restatement is too close to call"
    got = ctx.dirichlet_draws(n, alphas, seed=DRAW_SEED, first=first, device=kind == "dev")
    assert (torch.is_tensor(got) and got.is_cuda and got.dtype == torch.float64) if kind == "dev" else isinstance(got, np.ndarray)
    assert tuple(got.shape) == (n, len(alphas))
    registers, exp_only = len(alphas) <= REG_D, all(a == 1.0 for a in alphas)
    assert ctx.last_dirichlet_route() == ("registers" if registers else "regenerate") + "/" + ("exponential" if exp_only else "general")
    assert ctx.last_dirichlet_readbacks() == 0
    assert_rows_agree(got, want, rel, f"draws d={len(alphas)} n={n} first={first} {kind}")
    g = _np(got)
    assert np.max(np.abs(g.sum(axis=1) - 1.0)) <= 4 * U * len(alphas)


def test_draws_scale_with_c_scale(ctx):
    want, margin, rel = ref_draws(MIXED5, 300, 5, c_scale=2.5)
    assert margin.min() >= MARGIN
    got = ctx.dirichlet_draws(300, MIXED5, c_scale=2.5, seed=DRAW_SEED, first=5)
    assert_rows_agree(got, want, rel, "draws c_scale=2.5")
    assert np.max(np.abs(got.sum(axis=1) - 2.5)) <= 4 * U * 2.5 * 5


# ---- 2. slices are the same bits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphas", [(1.0,) * 3, MIXED5, (0.6,) * REG_D, (0.6,) * (REG_D + 1), (1.0,) * 40], ids=lambda a: f"d{len(a)}")
def test_a_slice_is_the_same_bits(ctx, alphas):
    a, b = RANGE - 3, RANGE + 10
    whole = ctx.dirichlet_draws(a + b, alphas, seed=7)
    part = ctx.dirichlet_draws(b, alphas, seed=7, first=a)
    assert np.array_equal(part, whole[a:])
    assert np.array_equal(ctx.dirichlet_draws(1, alphas, seed=7, first=a + 5)[0], whole[a + 5])
    far = (1 << 33) + 7
    assert np.array_equal(ctx.dirichlet_draws(3, alphas, seed=7, first=far + 2), ctx.dirichlet_draws(5, alphas, seed=7, first=far)[2:])


# ---- 3. constrained sampling against the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("box", sorted(BOXES))
def test_sampling_agrees_with_the_restatement(ctx, box, kind):
    bounds, alphas, acceptance = BOXES[box]
    want, n_found, n_drawn, idx, margin, dist, rel = ref_sample(box)
    assert margin >= MARGIN and dist >= MARGIN, "choose another seed: the restatement is too close to call"
    assert n_found == SAMPLE_N and 0.5 * acceptance < SAMPLE_N / (idx[-1] + 1) < 2.0 * acceptance
    got, got_found, got_drawn = ctx.dirichlet_sample(bounds, SAMPLE_N, alphas, seed=BOX_SEEDS[box], chunk_size=SAMPLE_CHUNK,
                                                     device=kind == "dev")
    assert (got_found, got_drawn) == (n_found, n_drawn) and got_drawn % SAMPLE_CHUNK == 0
    assert 1 <= ctx.last_dirichlet_readbacks() <= 1 + int(np.ceil(np.log2(500 * 4 / FIRST_BATCH)))
    assert_rows_agree(got, want, rel, f"sample {box} {kind}")
    g, b = _np(got), np.asarray(bounds)
    # hard properties: inside the box exactly, on the simplex, and in increasing draw index -- the indices recovered from the
    # device's own stream: the rows are, bit for bit, the first SAMPLE_N rows of dirichlet_draws that lie in the box
    assert np.all((b[:, 0] <= g) & (g <= b[:, 1]))
    assert np.max(np.abs(g.sum(axis=1) - 1.0)) <= 4 * U * len(alphas)
    stream = ctx.dirichlet_draws(n_drawn, alphas, seed=BOX_SEEDS[box])
    inside = np.nonzero(R.in_box(stream, b))[0][:SAMPLE_N]
    assert np.array_equal(inside, idx) and np.all(np.diff(inside) > 0)
    assert np.array_equal(stream[inside], g)


def test_sampling_with_c_scale(ctx):
    bounds, alphas, _ = BOXES["C"]
    want, n_found, n_drawn, idx, margin, dist, rel = ref_sample("C", 50, 512, 500, 2.5)
    assert margin >= MARGIN and dist >= MARGIN and n_found == 50
    got, f, dr = ctx.dirichlet_sample(np.asarray(bounds) * 2.5, 50, alphas, c_scale=2.5, seed=BOX_SEEDS["C"], chunk_size=512)
    assert (f, dr) == (n_found, n_drawn)
    assert_rows_agree(got, want, rel, "sample C c_scale=2.5")
    assert np.max(np.abs(got.sum(axis=1) - 2.5)) <= 4 * U * 2.5 * 5


# ---- 4. the stop rule --------------------------------------------------------------------------------------------------------
def test_the_samples_do_not_depend_on_the_chunk_size(ctx):
    bounds, alphas, _ = BOXES["B"]
    idx = ref_sample("B")[3]
    base = None
    for chunk in (1000, SAMPLE_CHUNK, 10 ** 6):
        got, found, drawn = ctx.dirichlet_sample(bounds, SAMPLE_N, alphas, seed=BOX_SEEDS["B"], chunk_size=chunk)
        assert found == SAMPLE_N and drawn == chunk * (idx[-1] // chunk + 1)
        base = got if base is None else base
        assert np.array_equal(got, base)


def test_n_samples_reached_inside_a_shot_and_exactly_at_its_end(ctx):
    bounds, alphas, _ = BOXES["A"]
    want, _, _, idx = ref_sample("A")[:4]
    k = 40
    chunk = int(idx[k]) + 1                       # draw idx[k], the (k + 1)-th accepted, is the last of shot 0
    for n, shots in ((k, 1), (k + 1, 1), (k + 2, int(idx[k + 1]) // chunk + 1)):
        got, found, drawn = ctx.dirichlet_sample(bounds, n, alphas, seed=BOX_SEEDS["A"], chunk_size=chunk)
        assert (found, drawn) == (n, shots * chunk) and shots in (1, 2)
        assert np.array_equal(got, ctx.dirichlet_sample(bounds, SAMPLE_N, alphas, seed=BOX_SEEDS["A"], chunk_size=SAMPLE_CHUNK)[0][:n])


def test_too_few_draws_leave_a_zero_tail_and_the_caller_warns(ctx):
    from corrla_rs_amd.callers import constr_dirichlet_sample
    bounds, alphas, _ = BOXES["B"]
    idx = ref_sample("B")[3]
    expect = int(np.sum(idx < 2000))
    assert 0 < expect < SAMPLE_N
    got, found, drawn = ctx.dirichlet_sample(bounds, SAMPLE_N, alphas, seed=BOX_SEEDS["B"], max_zshots=2, chunk_size=1000)
    assert (found, drawn) == (expect, 2000)
    assert np.all(got[found:] == 0.0) and np.all(got[:found].sum(axis=1) > 0.5)
    full = ctx.dirichlet_sample(bounds, SAMPLE_N, alphas, seed=BOX_SEEDS["B"], chunk_size=SAMPLE_CHUNK)[0]
    assert np.array_equal(got[:found], full[:found])
    with pytest.warns(RuntimeWarning, match=f"found {expect} of {SAMPLE_N}"):
        out = constr_dirichlet_sample(bounds, SAMPLE_N, 2, 1000, 1.0, alphas, seed=BOX_SEEDS["B"], ctx=ctx)
    assert np.array_equal(out, got)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.array_equal(constr_dirichlet_sample(bounds, SAMPLE_N, 500, SAMPLE_CHUNK, 1.0, alphas, seed=BOX_SEEDS["B"], ctx=ctx), full)


def test_chunk_size_one(ctx):
    bounds, alphas, _ = BOXES["A"]
    want, _, _, idx = ref_sample("A")[:4]
    expect = int(np.sum(idx < 500))
    got, found, drawn = ctx.dirichlet_sample(bounds, SAMPLE_N, alphas, seed=BOX_SEEDS["A"], max_zshots=500, chunk_size=1)
    assert (found, drawn) == (expect, 500) and 0 < expect < SAMPLE_N and np.all(got[found:] == 0.0)
    few, found, drawn = ctx.dirichlet_sample(bounds, 20, alphas, seed=BOX_SEEDS["A"], max_zshots=500, chunk_size=1)
    assert (found, drawn) == (20, int(idx[19]) + 1) and np.array_equal(few, got[:20])


# ---- 5. reproducibility and kinds --------------------------------------------------------------------------------------------
def test_same_call_same_bits_and_kinds_agree(ctx, torch):
    bounds, alphas, _ = BOXES["C"]
    kw = dict(seed=BOX_SEEDS["C"], chunk_size=SAMPLE_CHUNK)
    a = ctx.dirichlet_sample(bounds, SAMPLE_N, alphas, **kw)
    b = ctx.dirichlet_sample(bounds, SAMPLE_N, alphas, **kw)
    c = ctx.dirichlet_sample(bounds, SAMPLE_N, alphas, device=True, **kw)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] == c[1:]
    assert torch.is_tensor(c[0]) and c[0].is_cuda and np.array_equal(a[0], c[0].cpu().numpy())
    other = ctx.dirichlet_sample(bounds, SAMPLE_N, alphas, seed=BOX_SEEDS["C"] + 1, chunk_size=SAMPLE_CHUNK)
    assert not np.array_equal(a[0], other[0])
    assert np.array_equal(ctx.dirichlet_draws(100, alphas, seed=3), ctx.dirichlet_draws(100, alphas, seed=3, device=True).cpu().numpy())
    assert not np.array_equal(ctx.dirichlet_draws(100, alphas, seed=3), ctx.dirichlet_draws(100, alphas, seed=4))
    # alphas: None is all ones, one value is the symmetric case
    ones = ctx.dirichlet_sample(BOXES["A"][0], 10, None, seed=1, chunk_size=100)
    assert np.array_equal(ones[0], ctx.dirichlet_sample(BOXES["A"][0], 10, 1.0, seed=1, chunk_size=100)[0])
    assert np.array_equal(ones[0], ctx.dirichlet_sample(BOXES["A"][0], 10, (1.0,) * 3, seed=1, chunk_size=100)[0])


def _raw_sample(ctx, bounds, alphas, d, c_scale, seed, n_samples, max_zshots, chunk, out_ptr, ldo, dev=False, found=True, drawn=True):
    f, dr = C.c_int64(-1), C.c_int64(-1)
    fn = ctx._lib.corrla_dirichlet_sample_dev_f64 if dev else ctx._lib.corrla_dirichlet_sample_f64
    rc = fn(ctx._h, bounds.ctypes.data if bounds is not None else None, alphas.ctypes.data if alphas is not None else None, d, c_scale, seed,
            n_samples, max_zshots, chunk, out_ptr, ldo, C.byref(f) if found else None, C.byref(dr) if drawn else None)
    return rc, f.value, dr.value


def _raw_draws(ctx, alphas, d, c_scale, seed, first, n, out_ptr, ldo, dev=False):
    fn = ctx._lib.corrla_dirichlet_draws_dev_f64 if dev else ctx._lib.corrla_dirichlet_draws_f64
    return fn(ctx._h, alphas.ctypes.data if alphas is not None else None, d, c_scale, seed, first, n, out_ptr, ldo)


@pytest.mark.parametrize("kind", KINDS)
def test_a_wider_row_stride_leaves_the_gaps_unwritten(ctx, torch, kind):
    bounds, alphas, _ = BOXES["C"]
    b, al, d, ldo, n = np.ascontiguousarray(bounds, dtype=np.float64), np.asarray(alphas), 5, 8, 40
    want = ctx.dirichlet_sample(bounds, n, alphas, seed=9, max_zshots=1, chunk_size=100)      # about 19 found: a zero tail too
    assert 0 < want[1] < n
    sentinel = -7.25
    if kind == "dev":
        buf = torch.full((n, ldo), sentinel, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        rc, f, dr = _raw_sample(ctx, b, al, d, 1.0, 9, n, 1, 100, buf.data_ptr(), ldo, dev=True)
        out = buf.cpu().numpy()
    else:
        out = np.full((n, ldo), sentinel)
        rc, f, dr = _raw_sample(ctx, b, al, d, 1.0, 9, n, 1, 100, out.ctypes.data, ldo)
    assert rc == 0 and (f, dr) == want[1:]
    assert np.array_equal(out[:, :d], want[0]) and np.all(out[:, d:] == sentinel)
    if kind == "dev":
        buf.fill_(sentinel)
        torch.cuda.synchronize()
        rc = _raw_draws(ctx, al, d, 1.0, 9, 3, n, buf.data_ptr(), ldo, dev=True)
        ctx._lib.corrla_ctx_synchronize(ctx._h)
        out = buf.cpu().numpy()
    else:
        out = np.full((n, ldo), sentinel)
        rc = _raw_draws(ctx, al, d, 1.0, 9, 3, n, out.ctypes.data, ldo)
    assert rc == 0 and np.array_equal(out[:, :d], ctx.dirichlet_draws(n, alphas, seed=9, first=3)) and np.all(out[:, d:] == sentinel)


# ---- 6. rejections -----------------------------------------------------------------------------------------------------------
BOX_A = BOXES["A"][0]
BAD_SAMPLE = [
    (dict(bounds=((0.0, 1.0),)), "d must be"),
    (dict(bounds=((0.0, 1.0),) * 129), "d must be"),
    (dict(alphas=(1.0, 0.0, 1.0)), "alphas"),
    (dict(alphas=(1.0, float("nan"), 1.0)), "alphas"),
    (dict(alphas=(1.0, float("inf"), 1.0)), "alphas"),
    (dict(c_scale=0.0), "c_scale"),
    (dict(c_scale=float("inf")), "c_scale"),
    (dict(n_samples=0), "n_samples"),
    (dict(max_zshots=0), "max_zshots"),
    (dict(chunk_size=0), "chunk_size"),
    (dict(max_zshots=2 ** 31, chunk_size=2 ** 31), "max_zshots \\* chunk_size"),
    (dict(bounds=((0.0, 1.0), (0.5, 0.4), (0.0, 1.0))), "bounds"),
    (dict(bounds=((0.0, 1.0), (0.0, float("inf")), (0.0, 1.0))), "bounds"),
    (dict(bounds=((0.5, 1.0), (0.4, 1.0), (0.2, 1.0))), "infeasible"),
    (dict(bounds=((0.0, 0.3),) * 3), "infeasible"),
]


@pytest.mark.parametrize("kw,names", BAD_SAMPLE)
def test_sample_rejections_and_their_einval_twins(ctx, kw, names):
    from corrla_rs_amd import _lib as L
    ctx.dirichlet_draws(4, (1.0,) * 40, seed=1)
    before = (ctx.last_dirichlet_route(), ctx.last_dirichlet_readbacks())
    assert before == ("regenerate/exponential", 0)
    a = dict(bounds=BOX_A, n_samples=5, alphas=(1.0, 1.0, 1.0), c_scale=1.0, max_zshots=5, chunk_size=100)
    a.update(kw)
    with pytest.raises(ValueError, match=names):
        ctx.dirichlet_sample(a["bounds"], a["n_samples"], a["alphas"] if len(a["bounds"]) == 3 else None, c_scale=a["c_scale"],
                             max_zshots=a["max_zshots"], chunk_size=a["chunk_size"])
    b = np.ascontiguousarray(a["bounds"], dtype=np.float64)
    al = np.asarray(a["alphas"], dtype=np.float64) if len(a["bounds"]) == 3 else np.ones(len(a["bounds"]))
    out = np.full((max(a["n_samples"], 1), len(b)), 3.5)
    rc, f, dr = _raw_sample(ctx, b, al, len(b), a["c_scale"], 1, a["n_samples"], a["max_zshots"], a["chunk_size"], out.ctypes.data, len(b))
    assert rc == L.EINVAL and (f, dr) == (-1, -1) and np.all(out == 3.5)
    import re
    assert re.search(names, ctx._lib.corrla_last_error().decode()), ctx._lib.corrla_last_error()
    route = C.c_int(0)
    assert ctx._lib.corrla_ctx_last_dirichlet(ctx._h, C.byref(route)) == 0 and route.value == 3      # no kernel ran: unchanged
    assert (ctx.last_dirichlet_route(), ctx.last_dirichlet_readbacks()) == before


def test_null_pointers_strides_and_draw_rejections(ctx):
    from corrla_rs_amd import _lib as L
    b, al, out = np.ascontiguousarray(BOX_A, dtype=np.float64), np.ones(3), np.zeros((5, 3))
    err = lambda: ctx._lib.corrla_last_error().decode()
    for kw, name in ((dict(bounds=None), "bounds"), (dict(alphas=None), "alphas"), (dict(out_ptr=None), "out"), (dict(found=False), "n_found"),
                     (dict(drawn=False), "n_drawn"), (dict(ldo=2), "ldo")):
        a = dict(bounds=b, alphas=al, d=3, c_scale=1.0, seed=1, n_samples=5, max_zshots=5, chunk=100, out_ptr=out.ctypes.data, ldo=3)
        a.update(kw)
        assert _raw_sample(ctx, **a)[0] == L.EINVAL and name in err(), (name, err())
    for kw, name in ((dict(alphas=None), "alphas"), (dict(out_ptr=None), "out"), (dict(ldo=2), "ldo"), (dict(n=0), "n must"), (dict(first=-1), "first"),
                     (dict(first=2 ** 62 - 2), "first \\+ n"), (dict(d=1), "d must"), (dict(c_scale=-1.0), "c_scale")):
        a = dict(alphas=al, d=3, c_scale=1.0, seed=1, first=0, n=5, out_ptr=out.ctypes.data, ldo=3)
        a.update(kw)
        import re
        assert _raw_draws(ctx, **a) == L.EINVAL and re.search(name, err()), (name, err())
    for args, kw in (((0, (1.0,) * 3), {}), ((5, (1.0,)), {}), ((5, (1.0, -1.0)), {}), ((5, (1.0,) * 3), dict(first=-1)),
                     ((5, (1.0,) * 3), dict(first=2 ** 62 - 2)), ((5, (1.0,) * 3), dict(c_scale=float("nan"))), ((5, (1.0,) * 3), dict(seed=-1)),
                     ((5, np.ones((2, 2))), {})):
        with pytest.raises(ValueError):
            ctx.dirichlet_draws(*args, **kw)
    for alphas in ((1.0, 1.0), (1.0,) * 4, np.ones((3, 1))):
        with pytest.raises(ValueError, match="alphas"):
            ctx.dirichlet_sample(BOX_A, 5, alphas)
    with pytest.raises(ValueError, match="bounds"):
        ctx.dirichlet_sample(np.zeros((3, 3)), 5)
    assert np.all(out == 0.0)


# ---- 7. the example's own workload -------------------------------------------------------------------------------------------
def test_the_uranium_box_through_the_pyo3_names():
    import corrla_rs
    bounds, alphas = np.array(URANIUM_BOX), np.ones(3)
    s = corrla_rs.cs_dirichlet_sample(bounds, 64, 500, 1_000_000, 1.0, alphas)          # about 3.6 * 10^6 draws
    assert s.shape == (64, 3) and s.dtype == np.float64
    assert np.all((bounds[:, 0] <= s) & (s <= bounds[:, 1])) and np.max(np.abs(s.sum(axis=1) - 1.0)) < 1e-12
    assert not np.array_equal(s, corrla_rs.cs_dirichlet_sample(bounds, 64, 500, 1_000_000, 1.0, alphas))    # a fresh seed per call
    out, ratio = corrla_rs.cs_mcmc_dirichlet_sample(bounds, 200, 12, 500, 1_000_000, 1.0, np.array([0.6]), 0.8, 1e-12)
    assert out.shape == (200 * 12, 3) and 0.0 < ratio <= 1.0
    assert np.all((bounds[:, 0] <= out) & (out <= bounds[:, 1])) and np.max(np.abs(out.sum(axis=1) - 1.0)) < 1e-12
    with pytest.raises(TypeError):
        corrla_rs.cs_dirichlet_sample(bounds, 4, 5, 100, 1.0, np.ones((3, 1)))
