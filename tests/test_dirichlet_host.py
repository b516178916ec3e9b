"""The numpy restatement of the Dirichlet stream (tests/dirichlet_reference.py) judged against the distribution, on the CPU, so
that the GPU test only has to agree with the restatement; and the differential-evolution stage of cs_mcmc_dirichlet_sample
(corrla_rs_amd.callers.DeMcSampler), which is numpy and needs no GPU, on seeds made by the restatement.

Fixed seeds, 2 * 10^5 draws per parameter set.  Component means and variances lie within 5 standard errors of
alpha_j / alpha_0 and alpha_j (alpha_0 - alpha_j) / (alpha_0^2 (alpha_0 + 1)) -- the standard error of the mean is
sqrt(var / n), that of the variance sqrt((m4 - var^2) / n) with the fourth central moment m4 of Beta(alpha_j, alpha_0 - alpha_j)
from scipy -- and every marginal passes a Kolmogorov-Smirnov test against that Beta with p > 10^-3.  The thresholds are for these
seeds and are not re-rolled.  numpy's own Philox is the 4x64 variant, whose layout does not allow a comparison, so the
Philox4x32-10 words are held against the known-answer vectors published with Random123 (kat_vectors), typed in below."""
import numpy as np
import pytest

from tests import dirichlet_reference as R

N = 200_000
SETS = {
    "ones3": ((1.0, 1.0, 1.0), 11),
    "sym06": ((0.6,) * 3, 12),
    "mixed5": ((0.3, 1.0, 2.5, 7.0, 0.6), 13),
    "ones17": ((1.0,) * 17, 14),
}

# Random123 kat_vectors, philox4x32 10 rounds: counter, key -> output
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_10_known_answers(ctr, key, want):
    got = R.philox4x32_10(*(np.array([c], dtype=np.uint64) for c in ctr), *key)
    assert tuple(int(w[0]) for w in got) == want


def test_uniforms_are_53_bits_above_zero_and_follow_the_counter_layout():
    u1, u2 = R.uniform_pair(*(np.array([v], dtype=np.uint64) for v in (0, 0, 0xFFFFFFFF, 0xFFFFF000)))
    assert u1[0] == 2.0 ** -54 and u2[0] == 1.0 - 2.0 ** -52      # 2^53 - 2 + 0.5 rounds to the even 2^53 - 2
    # the one pattern of 53 ones: 2^53 - 1 + 0.5 rounds to 2^53, the uniform is 1 -- as the header says, and every formula is finite
    _, top = R.uniform_pair(*(np.array([v], dtype=np.uint64) for v in (0, 0, 0xFFFFFFFF, 0xFFFFFFFF)))
    assert top[0] == 1.0 and np.isfinite(np.log(top[0])) and np.power(top[0], 1.0 / 0.3) == 1.0
    t, seed = (1 << 33) + 7, (5 << 32) + 9
    w = R.philox4x32_10(*(np.array([c], dtype=np.uint64) for c in (7, 2, 3 + 65536 * R.ACCEPT, 4)), 9, 5)
    a, b = R.uniforms(np.array([t], dtype=np.uint64), 3, 4, R.ACCEPT, seed)
    assert (a[0], b[0]) == tuple(v[0] for v in R.uniform_pair(*w))


def test_cospi_keeps_its_zeros_and_signs():
    x = np.array([0.5, 1.5, 1.0, 0.25, 1.75, 2.0 ** -30, 2.0 - 2.0 ** -30, 0.5 + 2.0 ** -40])
    got = R.cospi(x)
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == -1.0
    assert abs(got[3] - np.sqrt(0.5)) < 2e-16 and abs(got[4] - np.sqrt(0.5)) < 2e-16 and got[5] == got[6]
    assert got[7] == -np.sin(np.pi * 2.0 ** -40)


@pytest.fixture(scope="module", params=sorted(SETS))
def drawn(request):
    alphas, seed = SETS[request.param]
    x, margin, rel = R.draws(0, N, alphas, 1.0, seed, full=True)
    return np.asarray(alphas), x, margin, rel


def test_rows_sum_to_one_and_are_positive(drawn):
    alphas, x, _, _ = drawn
    assert x.shape == (N, alphas.shape[0]) and np.all(x > 0.0)
    assert np.max(np.abs(x.sum(axis=1) - 1.0)) <= 4 * 2.0 ** -53 * alphas.shape[0]


def test_means_and_variances_within_five_standard_errors(drawn):
    from scipy import stats
    alphas, x, _, _ = drawn
    a0 = alphas.sum()
    for j, a in enumerate(alphas):
        mean, var = a / a0, a * (a0 - a) / (a0 * a0 * (a0 + 1.0))
        kurt = float(stats.beta(a, a0 - a).stats(moments="k"))
        m4 = (kurt + 3.0) * var * var
        assert abs(x[:, j].mean() - mean) <= 5.0 * np.sqrt(var / N), j
        assert abs(x[:, j].var() - var) <= 5.0 * np.sqrt((m4 - var * var) / N), j


def test_every_marginal_passes_kolmogorov_smirnov(drawn):
    from scipy import stats
    alphas, x, _, _ = drawn
    a0 = alphas.sum()
    for j, a in enumerate(alphas):
        assert stats.kstest(x[:, j], stats.beta(a, a0 - a).cdf).pvalue > 1e-3, j


def test_margins_and_error_bounds_are_what_the_gpu_test_takes_them_for(drawn):
    alphas, x, margin, rel = drawn
    if np.all(alphas == 1.0):
        assert np.all(np.isinf(margin)) and np.allclose(rel, 2.0 * R.LIB_ULP + 0.5 * (alphas.shape[0] - 1) + 1.0, rtol=1e-12, atol=0.0)
    else:
        assert np.all(margin > 0.0) and np.all(np.isfinite(rel)) and np.all(rel >= R.LIB_ULP)


def test_a_slice_of_the_stream_is_the_same_bits():
    alphas = SETS["mixed5"][0]
    whole = R.draws(0, 3000, alphas, 2.5, 99)
    assert np.array_equal(R.draws(1234, 500, alphas, 2.5, 99), whole[1234:1734])
    assert not np.array_equal(R.draws(0, 100, alphas, 2.5, 98), whole[:100])


def test_the_stop_rule_does_not_depend_on_the_chunk_size():
    bounds, alphas = ((0.1, 0.6), (0.05, 0.5), (0.2, 0.7)), (1.0,) * 3
    a = R.sample(bounds, 50, alphas, seed=3, max_zshots=500, chunk_size=64)
    b = R.sample(bounds, 50, alphas, seed=3, max_zshots=500, chunk_size=1000)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and a[1] == b[1] == 50
    assert a[2] == 64 * (a[3][-1] // 64 + 1) and b[2] == 1000
    assert np.all(R.in_box(a[0], bounds)) and np.all(np.diff(a[3]) > 0)
    short = R.sample(bounds, 50, alphas, seed=3, max_zshots=2, chunk_size=20)
    assert short[1] < 50 and short[2] == 40 and np.all(short[0][short[1]:] == 0.0) and np.array_equal(short[0][:short[1]], a[0][:short[1]])


# ---- the differential-evolution stage ----------------------------------------------------------------------------------------
BOX = np.array(((0.1, 0.6), (0.05, 0.5), (0.2, 0.7)))


def _chains(c_scale, n_chains=12, steps=200, seed=5):
    from corrla_rs_amd.callers import DeMcSampler
    seeds, found, _, _ = R.sample(BOX * c_scale, n_chains, (0.6,) * 3, c_scale=c_scale, seed=21, max_zshots=50, chunk_size=256)
    assert found == n_chains
    s = DeMcSampler(BOX * c_scale, seeds, np.ones(3), 0.8, 1e-12, c_scale=c_scale, seed=seed)
    s.sample_mcmc(steps)
    return s, seeds


@pytest.mark.parametrize("c_scale", [1.0, 2.5])
def test_demc_samples_stay_in_the_box_on_the_simplex(c_scale):
    s, seeds = _chains(c_scale)
    out = s.get_samples(200)
    assert out.shape == (200 * 12, 3)
    assert np.all((BOX[:, 0] * c_scale <= out) & (out <= BOX[:, 1] * c_scale))
    assert np.max(np.abs(out.sum(axis=1) - c_scale)) <= 4 * 2.0 ** -53 * c_scale * 3
    assert 0.0 < s.accept_ratio() <= 1.0
    assert s.n_accept + s.n_reject == 200 * 12
    # chain-fastest: row i of the tail belongs to chain i mod 12; the whole history starts at the seeds
    assert np.array_equal(s.get_samples(201)[:12], seeds)
    assert len({tuple(r) for r in out}) > 12      # the chains moved


def test_demc_is_reproducible_by_seed():
    a, _ = _chains(1.0, seed=5)
    b, _ = _chains(1.0, seed=5)
    c, _ = _chains(1.0, seed=6)
    assert np.array_equal(a.get_samples(200), b.get_samples(200)) and a.accept_ratio() == b.accept_ratio()
    assert not np.array_equal(a.get_samples(200), c.get_samples(200))


def test_demc_needs_three_chains_and_rejects_nonpositive_proposals():
    from corrla_rs_amd.callers import DeMcSampler, cs_mcmc_dirichlet_sample
    with pytest.raises(ValueError, match="3 chains"):
        DeMcSampler(BOX, np.full((2, 3), 1.0 / 3.0), np.ones(3), 0.8, 1e-12)
    with pytest.raises(ValueError, match="3 chains"):
        cs_mcmc_dirichlet_sample(BOX, 10, 2, 5, 100, 1.0, np.ones(3), 0.8, 1e-12, seed=1)   # before any context is made
    s = DeMcSampler(np.array(((-1.0, 2.0),) * 3), np.full((3, 3), 1.0 / 3.0), np.array((0.5, 2.0, 1.0)), 0.8, 1e-12)
    lp = s.ln_prob(np.array(((0.2, 0.3, 0.5), (-0.1, 0.6, 0.5), (0.0, 0.5, 0.5))))
    from scipy import stats
    assert abs(lp[0] - stats.dirichlet.logpdf((0.2, 0.3, 0.5), (0.5, 2.0, 1.0))) < 1e-12
    assert np.isneginf(lp[1]) and np.isneginf(lp[2])


# ---- the restatement against 50 digits ---------------------------------------------------------------------------------------
def _mp_rows(alphas, n, c_scale, seed):
    """the stream evaluated with mpmath at 50 digits on the restatement's own uniforms (doubles: exact in mpmath), with the
    documented formulas; an attempt's outcome is decided at 50 digits"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    t = np.arange(n, dtype=np.uint64)
    rows = []
    for i in range(n):
        g = []
        for j, alpha in enumerate(alphas):
            method, D, C, inv_alpha = R.component(alpha)
            own = mp.mpf(float(R.uniforms(t[i:i + 1], j, 0, R.OWN, seed)[0][0]))
            if method == "exp":
                g.append(-mp.log(own))
                continue
            D, C = mp.mpf(D), mp.mpf(C)         # the constants are part of the stream as the doubles the host computes
            for a in range(R.MAX_ATTEMPTS):
                u1, u2 = (mp.mpf(float(v[0])) for v in R.uniforms(t[i:i + 1], j, a, R.NORMAL, seed))
                z = mp.sqrt(-2 * mp.log(u1)) * mp.cospi(2 * u2)
                w = 1 + C * z
                if w <= 0:
                    continue
                v = w ** 3
                q = mp.mpf(float(R.uniforms(t[i:i + 1], j, a, R.ACCEPT, seed)[0][0]))
                if q < 1 - mp.mpf(0.0331) * z ** 4 or mp.log(q) < z * z / 2 + D * (1 - v + mp.log(v)):
                    break
            else:
                raise AssertionError("64 rejected attempts")
            gj = D * v
            g.append(gj * own ** mp.mpf(inv_alpha) if method == "boost" else gj)
        s = mp.fsum(g)
        rows.append([mp.mpf(c_scale) * gj / s for gj in g])
    return rows


@pytest.mark.parametrize("alphas", [(0.3, 1.0, 2.5, 7.0, 0.6), (1.0, 50.0, 1.0), (0.6,) * 3, (1.0,) * 17], ids=lambda a: f"d{len(a)}")
def test_the_restatement_is_within_its_own_error_bound_of_50_digits(alphas):
    """The bound the GPU test gives the device, e_x u x (before its factor 4), also covers numpy: the restatement's distance to
    the 50-digit value of the same draw is inside it, so the derived bound is the larger of the two."""
    mp = pytest.importorskip("mpmath")
    n, seed = 48, 20241008
    x, margin, rel = R.draws(0, n, alphas, 2.5, seed, full=True)
    assert margin.min() >= 1e-9
    exact = _mp_rows(alphas, n, 2.5, seed)
    worst = 0.0
    for i in range(n):
        for j in range(len(alphas)):
            err = abs(mp.mpf(float(x[i, j])) - exact[i][j]) / exact[i][j]
            worst = max(worst, float(err / (rel[i, j] * R.U)))
    print(f"d = {len(alphas)}: the restatement is at most {worst:.3f} of its bound from the 50-digit value")
    assert worst <= 1.0
