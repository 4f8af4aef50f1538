"""CPU: the NumPy statement of the ARCH(1) and M/G/1 models (tests/series_ref.py) is ELFI's own examples bit for bit --
pinned to recorded runs (tests/golden/series_models.npz, scripts/make_golden_series.py) and, where the reference is
present, to fresh runs -- and the device functions refuse bad arguments before any device context exists."""
import os

import numpy as np
import pytest

import series_ref as R


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'series_models.npz'))


def test_arch_series_and_summaries_are_the_recorded_ones(golden):
    g = golden
    assert g['arch_W'].shape == (64, 102) and int(g['arch_n_lags']) == 5
    Y = R.arch_series(g['arch_t1'], g['arch_t2'], g['arch_W'])
    assert np.array_equal(Y, g['arch_Y'])
    S = R.arch_summaries(Y, 5)
    assert S.shape == (64, 17) and np.array_equal(S, g['arch_S'])
    assert R.arch_names(5)[:4] == ['MU', 'VAR', 'AC_1', 'AC_2'] and R.arch_names(5)[7:9] == ['PW_1_2', 'PW_1_3']
    assert R.arch_names(5)[-1] == 'PW_4_5' and len(R.arch_names(8)) == 38


def test_mg1_series_quantiles_and_logs_are_the_recorded_ones(golden):
    g = golden
    assert g['mg1_E'].shape == g['mg1_V'].shape == (64, 50)
    Y = R.mg1_series(g['mg1_t1'], g['mg1_t2'], g['mg1_t3'], g['mg1_E'], g['mg1_V'])
    assert np.array_equal(Y, g['mg1_Y'])
    assert np.array_equal(R.mg1_quantiles(Y, g['mg1_q']), g['mg1_Q'])
    assert np.array_equal(R.log_identity(Y), g['mg1_logY'])


@pytest.mark.parametrize('n_obs', [2, 37, 50, 130])
@pytest.mark.parametrize('nq', [1, 2, 4, 10])
def test_quantile_positions_reproduce_np_quantile(n_obs, nq):
    from elfi_amd.summaries import quantile_positions
    rs = np.random.RandomState(100 * n_obs + nq)
    Y = rs.exponential(3.0, (9, n_obs))
    Y[3, : n_obs // 2] = Y[3, 0]          # ties
    for q in (np.linspace(0, 1, nq), np.sort(rs.uniform(0, 1, nq))):
        lo, hi, t = R.quantile_positions(q, n_obs)
        assert lo.dtype == hi.dtype == np.int32 and np.all((lo >= 0) & (lo < n_obs) & (hi >= 0) & (hi < n_obs))
        assert np.array_equal(R.quantiles_at(Y, lo, hi, t), np.quantile(Y, q, axis=1).T)
        # the package's own host-side positions are the same numbers
        for mine, ref in zip(quantile_positions(q, n_obs), (lo, hi, t)):
            assert mine.dtype == ref.dtype and np.array_equal(mine, ref)
    Yn = Y.copy()
    Yn[1, n_obs // 2] = np.nan            # np.quantile answers NaN for the whole row
    q = np.linspace(0, 1, nq)
    assert np.array_equal(R.mg1_quantiles(Yn, q), np.quantile(Yn, q, axis=1).T, equal_nan=True)


def test_weighted_euclidean_is_cdists():
    from scipy.spatial.distance import cdist
    rs = np.random.RandomState(5)
    S, obs, w = rs.randn(50, 17), rs.randn(17), rs.uniform(0.01, 1, 17)
    assert np.array_equal(R.weighted_euclidean(S, obs), cdist(S, obs[None], 'euclidean')[:, 0])
    assert np.array_equal(R.weighted_euclidean(S, obs, w), cdist(S, obs[None], 'euclidean', w=w)[:, 0])


@pytest.mark.reference
def test_restatement_is_the_reference_on_fresh_seeds():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    from itertools import combinations
    from elfi.examples import arch, mg1
    for seed, (B, n_obs, L) in enumerate([(1, 100, 5), (33, 37, 3), (20, 200, 8), (7, 7, 5)]):
        rs = np.random.RandomState(seed)
        t1, t2 = rs.uniform(-1, 1, B), rs.uniform(0, 1, B)
        Y = arch.arch(t1, t2, n_obs=n_obs, batch_size=B, random_state=np.random.RandomState(1000 + seed))
        W = R.arch_noise_from_state(np.random.RandomState(1000 + seed), B, n_obs)
        assert np.array_equal(R.arch_series(t1, t2, W), Y)
        lags = range(1, L + 1)
        S = np.column_stack([arch.sample_mean(Y), arch.sample_variance(Y)] + [arch.autocorr(Y, i) for i in lags] +
                            [arch.pairwise_autocorr(Y, i, j) for i, j in combinations(lags, 2)])
        assert np.array_equal(R.arch_summaries(Y, L), S)
    for seed, (B, n_obs, nq) in enumerate([(1, 50, 10), (33, 37, 4), (20, 130, 10), (7, 2, 2)]):
        rs = np.random.RandomState(50 + seed)
        t1 = rs.uniform(0, 10, B)
        t2, t3 = t1 + rs.uniform(0, 10, B), rs.uniform(0.01, 0.5, B)
        Y = mg1.MG1(t1, t2, t3, n_obs=n_obs, batch_size=B, random_state=np.random.RandomState(2000 + seed))
        E, V = R.mg1_draws_from_state(np.random.RandomState(2000 + seed), B, n_obs)
        assert np.array_equal(R.mg1_series(t1, t2, t3, E, V), Y)
        q = np.linspace(0, 1, nq)
        assert np.array_equal(R.mg1_quantiles(Y, q), mg1.quantiles(Y, q))
        assert np.array_equal(R.log_identity(Y), mg1.log_identity(Y))


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib
    from elfi_amd.summaries import SERIES_MAX_OBS

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    t = np.full(4, 0.5)
    bad_arch = [dict(n_lags=0), dict(n_lags=9), dict(n_obs=6, n_lags=5), dict(n_obs=3, n_lags=2),
                dict(noise=np.zeros((4, 101))), dict(noise=np.zeros(102)), dict(noise=np.zeros((3, 102))),
                dict(observed=np.zeros(16)), dict(observed=np.zeros(17), n_lags=4),
                dict(n_obs=SERIES_MAX_OBS + 1)]
    for kw in bad_arch:
        with pytest.raises(ValueError):
            elfi_amd.arch_summaries(t, t, **kw)
    e = np.ones((4, 50))
    bad_mg1 = [dict(n_obs=1), dict(draws=(np.ones((4, 49)), np.ones((4, 49)))), dict(draws=(e, np.ones((4, 51)))),
               dict(draws=(np.ones(50), np.ones(50))), dict(draws=(np.ones((3, 50)), np.ones((3, 50)))),
               dict(observed=np.zeros(9)), dict(w=np.ones(10)), dict(observed=np.zeros(10), w=np.ones(9)),
               dict(q=[-0.1, 0.5]), dict(q=[0.5, 1.5]), dict(q=np.linspace(0, 1, 65)), dict(q=[]),
               dict(n_obs=SERIES_MAX_OBS + 1)]
    for kw in bad_mg1:
        with pytest.raises(ValueError):
            elfi_amd.mg1_summaries(t, t + 1, t, **kw)
