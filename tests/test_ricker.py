"""CPU: the NumPy statement of the Ricker model (tests/ricker_ref.py) is ELFI's own example bit for bit -- pinned to recorded
runs (tests/golden/ricker.npz, scripts/make_golden_ricker.py) and, where the reference is present, to fresh runs; the NumPy
statement of the library's Poisson sampler has the Poisson distribution (scipy.stats.poisson); and the device functions
refuse bad arguments before any device context exists."""
import os

import numpy as np
import pytest

import ricker_ref as R

POISSON_LAMS = [1e-3, 0.5, 3, 9.999, 10, 12.5, 50, 1e3, 1e6]


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'ricker.npz'))


def test_stochastic_restatement_is_the_recorded_run(golden):
    g = golden
    assert g['Z'].shape == g['St'].shape == g['Y'].shape == (64, 50) and g['S'].shape == (64, 3)
    St = R.ricker_stock(g['t1'], g['t2'], g['Z'])
    assert np.array_equal(St, g['St'])
    assert np.array_equal(R.ricker_summaries(g['Y']), g['S'])
    assert np.array_equal(R.chi_squared(g['S'], g['obs']), g['D'], equal_nan=True)
    # the recorded counts are integers with the recorded intensities' scale: crashed populations are observed as zeros
    lam = g['t3'][:, None] * g['St']
    assert np.all(g['Y'] == np.floor(g['Y'])) and np.all(g['Y'][lam == 0] == 0)
    assert np.array_equal(g['S'][:, 2], np.sum(g['Y'] == 0, axis=1))


def test_deterministic_restatement_is_the_recorded_run(golden):
    g = golden
    Y = R.ricker_series_deterministic(g['det_t1'], n_obs=50)
    assert Y.shape == (16, 50) and np.array_equal(Y, g['det_Y'])
    assert np.array_equal(R.ricker_summaries(Y)[:, 0], g['det_mean'])
    assert np.array_equal(np.sqrt((g['det_mean'] - g['det_obs'][0]) ** 2), g['det_D'])


@pytest.mark.reference
def test_restatement_is_the_reference_on_fresh_seeds():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import scipy.stats as ss
    from elfi.examples import ricker
    for seed, (B, n_obs) in enumerate([(1, 50), (33, 37), (7, 1), (20, 130)]):
        rs = np.random.RandomState(300 + seed)
        t1 = ss.expon.rvs(np.e, 2, size=B, random_state=rs)
        t2 = ss.truncnorm.rvs(0, 5, size=B, random_state=rs)
        t3 = ss.uniform.rvs(0, 100, size=B, random_state=rs)
        Y = ricker.stochastic_ricker(t1, t2, t3, n_obs=n_obs, batch_size=B, random_state=np.random.RandomState(3000 + seed))
        Z, St, Yr = R.stochastic_ricker_from_state(np.random.RandomState(3000 + seed), t1, t2, t3, n_obs=n_obs, batch=B)
        assert np.array_equal(Yr, Y)
        assert np.array_equal(R.ricker_stock(t1, t2, Z), St)
        S = np.column_stack([np.mean(Y, axis=1), np.var(Y, axis=1), ricker.num_zeros(Y)])
        assert np.array_equal(R.ricker_summaries(Y), S)
        obs = (np.array([3.5]), np.array([40.25]), np.array([7.0]))
        assert np.array_equal(R.chi_squared(S, np.concatenate(obs)), ricker.chi_squared(*S.T, observed=obs))
        Yd = ricker.ricker(t1, n_obs=n_obs, batch_size=B)
        assert np.array_equal(R.ricker_series_deterministic(t1, n_obs=n_obs), Yd)


@pytest.mark.parametrize('lam', POISSON_LAMS)
def test_poisson_statement_has_the_poisson_distribution(lam):
    """200 000 draws per intensity: chi-square goodness of fit against scipy.stats.poisson over cells of expected count
    >= 5 (both tails pooled), p >= 1e-4, and mean and variance within 4 standard errors."""
    import scipy.stats as ss
    n = 200000
    x, sens, attempts = R.poisson_ref(np.full(n, lam), 20274, 5, return_attempts=True)
    assert np.all(x == np.floor(x)) and np.all(x >= 0)
    # an attempt rejects with probability at most 0.25 (at lam = 10): 17 attempts among 200 000 draws have probability 5e-5
    assert attempts.max() <= (1 if lam < 10 else 16)
    # cells: integers lo .. hi with both tails pooled into the end cells, then neighbours merged up to an expected count of 5
    lo, hi = int(ss.poisson.ppf(1e-7, lam)), int(ss.poisson.ppf(1 - 1e-7, lam))
    if hi - lo > 4000:          # lam = 1e6: cells of equal width, about 200 of them
        edges = np.unique(np.linspace(lo, hi + 1, 201).astype(np.int64))
    else:
        edges = np.arange(lo, hi + 2)
    cdf = ss.poisson.cdf(edges[1:-1] - 1, lam)                  # P(X < edge)
    prob = np.diff(np.concatenate(([0.0], cdf, [1.0])))
    cell = np.clip(np.searchsorted(edges, x, side='right') - 1, 0, len(prob) - 1)
    count = np.bincount(cell, minlength=len(prob)).astype(np.float64)
    exp_m, obs_m, e_acc, o_acc = [], [], 0.0, 0.0
    for e, o in zip(n * prob, count):
        e_acc, o_acc = e_acc + e, o_acc + o
        if e_acc >= 5:
            exp_m.append(e_acc)
            obs_m.append(o_acc)
            e_acc = o_acc = 0.0
    if exp_m:
        exp_m[-1] += e_acc
        obs_m[-1] += o_acc
    else:
        exp_m, obs_m = [e_acc], [o_acc]
    exp_m, obs_m = np.array(exp_m), np.array(obs_m)
    z_mean = (x.mean() - lam) / np.sqrt(lam / n)
    # Var of the sample variance of a Poisson: (mu4 - sigma^4) / n with mu4 = lam + 3 lam^2, i.e. (lam + 2 lam^2) / n
    z_var = (x.var(ddof=1) - lam) / np.sqrt((lam + 2 * lam * lam) / n)
    p = 1.0
    if len(exp_m) > 1:
        chi2 = np.sum((obs_m - exp_m) ** 2 / exp_m)
        p = ss.chi2.sf(chi2, len(exp_m) - 1)
    else:
        assert obs_m[0] == n
    print('lam %g: cells %d p %.4f z_mean %.2f z_var %.2f attempts mean %.3f max %d sensitive %d' %
          (lam, len(exp_m), p, z_mean, z_var, attempts.mean(), attempts.max(), sens.sum()))
    assert p >= 1e-4
    assert abs(z_mean) <= 4 and abs(z_var) <= 4


def test_poisson_statement_special_values():
    lam = np.array([0.0, np.nan, np.inf, -1.0, 2.0 ** 54, -0.0, 1e-300])
    x, sens = R.poisson_ref(lam, 3, 0)
    assert np.array_equal(x, [0, np.nan, np.nan, np.nan, np.nan, 0, 0], equal_nan=True) and not sens.any()
    # element e is a function of (lam[e], e): a prefix of a longer draw, and the shape is kept
    a, _ = R.poisson_ref(np.full(50, 12.5), 3, 9)
    b, _ = R.poisson_ref(np.full((20, 5), 12.5), 3, 9)
    assert b.shape == (20, 5) and np.array_equal(a, b.reshape(-1)[:50])
    c, _ = R.poisson_ref(np.full(50, 12.5), 3, 10)
    assert not np.array_equal(a, c)


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib
    from elfi_amd.summaries import SERIES_MAX_OBS

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    assert SERIES_MAX_OBS == 2048
    t = np.full(4, 0.5)
    bad = [dict(n_obs=0), dict(n_obs=2049), dict(noise=np.zeros((4, 49))), dict(noise=np.zeros(50)),
           dict(noise=np.zeros((3, 50))), dict(distance='euclidean'), dict(observed=np.zeros(2)),
           dict(observed=np.zeros(3), distance='manhattan')]
    for kw in bad:
        with pytest.raises(ValueError):
            elfi_amd.ricker_summaries(t, t, t, **kw)
    for kw in (dict(std=t), dict(scale=t), dict(noise=np.zeros((4, 50))), dict(return_draws=True)):
        with pytest.raises(ValueError):
            elfi_amd.ricker_summaries(t, **kw)
    with pytest.raises(ValueError):
        elfi_amd.ricker_summaries(t, t, np.zeros(3))               # a parameter of another batch size
