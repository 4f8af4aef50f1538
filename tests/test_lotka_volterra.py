"""CPU: the NumPy statement of the stochastic Lotka-Volterra model (tests/lv_ref.py) is ELFI's own example bit for bit --
pinned to recorded runs on replayed draws (tests/golden/lotka_volterra.npz, scripts/make_golden_lv.py) and, where the
reference is present, to fresh runs; the boundary mask of the drawn form covers next to nothing; ExpUniform's density is
the reference's; and the device functions refuse bad arguments before any device context exists."""
import os

import numpy as np
import pytest

import lv_ref as L


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'lotka_volterra.npz'))


@pytest.mark.parametrize('name,noisy', [('true', True), ('prior', False)])
def test_statement_is_the_recorded_run(golden, name, noisy):
    g = golden
    Yg = g[name + '_Y']
    B, n_obs = Yg.shape[:2]
    assert (B, n_obs) == (16, 16) and Yg.dtype == np.int32
    E, U, Z = L.golden_draws(g[name + '_seed'], B, int(g[name + '_n_events']), n_obs)
    sigma = np.full(B, 10.) if noisy else None
    Y, T, status, events = L.simulate(*g[name + '_params'], sigma, E, U, Z, n_obs, float(g[name + '_time_end']))
    assert np.array_equal(Y, Yg.astype(np.float64))
    assert np.array_equal(events, g[name + '_events'])
    assert np.all(status <= L.EXTINCT) and np.all(T >= float(g[name + '_time_end']))
    assert np.array_equal(status == L.EXTINCT, Y[:, -1, 1] == 0) or noisy
    S = L.summaries(Y)
    assert np.array_equal(S, g[name + '_S'], equal_nan=True)
    assert np.array_equal(L.euclidean(S, g['obs']), g[name + '_D'], equal_nan=True)
    if not noisy:      # the planted row with nothing alive: a constant series, one event, NaN correlations
        assert np.all(Y[0] == 0) and events[0] == 1 and status[0] == L.EXTINCT
        assert np.array_equal(S[0], [0, 0, 0, 0] + [np.nan] * 5, equal_nan=True)
        assert np.all(np.isfinite(S[1:, :4]))


def test_statement_marks_what_cannot_be_simulated():
    rs = np.random.RandomState(5)
    E, U = rs.exponential(size=(6, 40)), rs.uniform(size=(6, 40))
    r1 = np.array([1.0, np.nan, 1.0, np.exp(2.0), 1.0, 1.0])
    r2 = np.array([0.005, 0.005, 0.005, np.exp(-6.0), 0.005, np.inf])
    prey = np.array([50, 50, 0.5, 50, -1.0, 50])
    pred = np.array([0.5, 100, 0.9, 100, 100, 100])
    Y, T, status, events = L.simulate(r1, r2, 0.6, prey, pred, None, E, U, n_obs=5, time_end=2.)
    assert status.tolist() == [L.EXTINCT, L.INVALID, L.EXTINCT, L.OUT_OF_EVENTS, L.INVALID, L.INVALID]
    assert events.tolist() == [1, 0, 1, 40, 0, 0]
    assert np.all(Y[0, :, 1] == 0) and np.all(Y[0, 1:, 0] >= 50) and np.all(Y[2] == 0)
    assert np.all(np.isnan(Y[[1, 4, 5]])) and np.all(np.isnan(T[[1, 4, 5]])) and T[0] == T[2] == 2.
    assert np.isnan(Y[3, -1]).all() and np.isfinite(Y[3, 0]).all() and T[3] < 2.
    assert np.all(np.isnan(L.summaries(Y)[[1, 3, 4, 5]]))
    # a negative sigma is invalid too
    assert L.simulate(1., .005, .6, 50, 100, [-1.] * 6, E, U, np.zeros((6, 8)), n_obs=5, time_end=2.)[2].tolist() == [3] * 6
    # stored as an int32 slot keeps it
    assert np.array_equal(L.store_int(np.array([-0.5, 0.5, -1.5, 2.0 ** 31, -2.0 ** 31, 2.0 ** 31 - 0.5, np.nan, np.inf])),
                          [0, 0, -1, np.nan, np.nan, 2.0 ** 31 - 1, np.nan, np.nan], equal_nan=True)
    assert not np.signbit(L.store_int(np.array([-0.5])))[0]


def test_observation_times_are_linspace():
    for time_end, n_obs in [(30., 16), (2., 50), (0.1, 3), (7.3, 2048), (1e-3, 7)]:
        assert np.array_equal(L.times_out(time_end, n_obs), np.linspace(0, time_end, n_obs))


def test_boundary_mask_covers_next_to_nothing():
    """The drawn form's exponentials go through the device's log; the statement marks the observations that a last-bit
    change of an event time can move.  Share seen over 2000 simulations x 16 observations from the priors: 0."""
    rs = np.random.RandomState(11)
    n = 2000
    p = [np.exp(rs.uniform(-6, 2, n)) for _ in range(3)] + [rs.normal(50, np.sqrt(50), n), rs.normal(100, 10, n)]
    E, U, _ = L.draws(7, 2, n, 600)
    out = L.simulate(*p, None, E, U, n_obs=16, time_end=2., return_mask=True)
    share = out[-1][:, 1:].mean()
    print('boundary share %.3g, out of events %d' % (share, (out[2] == L.OUT_OF_EVENTS).sum()))
    assert share <= 1e-3
    # scaling every exponential by 1 +- 4 eps moves no observation outside the mask
    for f in (1 - 4 * L.EPS, 1 + 4 * L.EPS):
        other = L.simulate(*p, None, E * f, U, n_obs=16, time_end=2.)
        same = np.all((other[0] == out[0]) | np.isnan(out[0]), axis=2)
        assert np.all(same | out[-1])


def test_draw_layout():
    E, U, A = L.draws(3, 9, 5, 7)
    assert E.shape == U.shape == (5, 7) and np.all(E >= 0) and np.all((U >= 0) & (U < 1)) and np.all((A > 0) & (A <= 1))
    E2, U2, _ = L.draws(3, 9, 3, 12, first=2)              # simulation i of one call is simulation 0 of another
    assert np.array_equal(E2[:, :7], E[2:]) and np.array_equal(U2[:, :7], U[2:])
    assert not np.array_equal(L.draws(3, 10, 5, 7)[0], E)


@pytest.mark.reference
def test_statement_is_the_reference_on_fresh_seeds():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    from functools import partial
    from scipy.spatial.distance import cdist
    from elfi.examples import lotka_volterra as lv
    fns = [partial(lv.stock_mean, species=0), partial(lv.stock_mean, species=1), partial(lv.stock_log_variance, species=0),
           partial(lv.stock_log_variance, species=1), partial(lv.stock_autocorr, species=0, lag=1),
           partial(lv.stock_autocorr, species=1, lag=1), partial(lv.stock_autocorr, species=0, lag=2),
           partial(lv.stock_autocorr, species=1, lag=2), lv.stock_crosscorr]
    for seed, (B, n_obs, time_end, noisy) in enumerate([(1, 3, 1., False), (33, 50, 2., True), (7, 130, 3., False),
                                                        (5, 300, 2., True), (6, 129, 2., True), (4, 2048, 2., False)]):
        rs = np.random.RandomState(400 + seed)
        p = [np.exp(rs.uniform(-6, 2, B)) for _ in range(3)] + [rs.normal(50, np.sqrt(50), B), rs.normal(100, 10, B)]
        p[0], p[1] = np.minimum(p[0], 1.0), np.minimum(p[1], 0.05)     # keeps the slowest simulation of the lock-step short
        if B > 2:
            p[3][0], p[4][0] = 0.2, 0.4               # nothing alive
            p[4][1] = 0.7                             # no predators
        E, U, Z = L.golden_draws(500 + seed, B, 6000, n_obs)
        sigma = np.exp(rs.uniform(np.log(0.5), np.log(50), B)) if noisy else 0.
        replay = L.Replay(E, U, Z if noisy else None)
        Yr, _, _, times = lv.lotka_volterra(*p, sigma=sigma, n_obs=n_obs, time_end=time_end, batch_size=B,
                                            random_state=replay, return_full=True)
        assert replay.ke <= 6000
        Y, T, status, events = L.simulate(*p, sigma if noisy else None, E, U, Z, n_obs, time_end)
        assert np.array_equal(Y, Yr.astype(np.float64))
        assert np.array_equal(events, np.argmax(times >= time_end, axis=1))
        with np.errstate(all='ignore'):
            Sr = np.column_stack([f(Yr) for f in fns])
            assert np.array_equal(L.summaries(Y), Sr, equal_nan=True)
            obs = np.linspace(1, 2, 9)
            assert np.array_equal(L.euclidean(Sr, obs), cdist(Sr, obs[None, :])[:, 0], equal_nan=True)


def test_exp_uniform_density_is_the_reference():
    from elfi_amd.priors import ExpUniform
    x = np.concatenate([np.exp(np.linspace(-7, 3, 41)), [np.exp(-6.), np.exp(2.), 0.0]])
    want = np.where((x < np.exp(-6.)) | (x > np.exp(2.)), 0, 1 / np.maximum(x, 1e-300)) / 8.
    assert np.array_equal(ExpUniform.pdf(x, -6., 2.), want)
    grid = np.exp(np.linspace(-6, 2, 200001))
    f = ExpUniform.pdf(grid, -6., 2.)
    assert abs(np.sum((f[1:] + f[:-1]) / 2 * np.diff(grid)) - 1) < 1e-6
    import ref_shim
    if ref_shim.available():
        ref_shim.install()
        from elfi.examples import lotka_volterra as lv
        for a, b in [(-6., 2.), (np.log(0.5), np.log(50))]:
            assert np.array_equal(ExpUniform.pdf(x, a, b), lv.ExpUniform.pdf(x, a, b))


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    t = np.full(4, 0.5)
    E = np.ones((4, 10))
    bad = [dict(n_obs=2), dict(n_obs=2049), dict(time_end=0.), dict(time_end=np.inf), dict(time_end=np.nan),
           dict(max_events=0), dict(max_events=(1 << 30) + 1), dict(draws=(E, E[:3])), dict(draws=(E[0], E[0])),
           dict(noise=np.zeros((4, 30))), dict(sigma=t, noise=np.zeros((4, 29))), dict(sigma=t, noise=np.zeros((3, 30))),
           dict(observed=np.zeros(8)), dict(first_index=-1), dict(first_index=2 ** 32 - 3), dict(sigma=np.zeros(3))]
    for kw in bad:
        with pytest.raises(ValueError):
            elfi_amd.lotka_volterra_summaries(t, t, t, **kw)
    with pytest.raises(ValueError):
        elfi_amd.lotka_volterra_summaries(t, t, np.zeros(3))        # a parameter of another batch size
    for kw in (dict(n=0, n_events=5), dict(n=3, n_events=0), dict(n=3, n_events=(1 << 30) + 1), dict(n=3, n_events=5, first_index=-1)):
        with pytest.raises(ValueError):
            elfi_amd.lotka_volterra_draws(**kw)
    with pytest.raises(ValueError):
        elfi_amd.lotka_volterra_model(true_params=[1., .005, .6, 50, 100, 10.])
    with pytest.raises(ValueError):
        elfi_amd.lotka_volterra_model(true_params=[1., .005, .6, 50, 100], observation_noise=True)
