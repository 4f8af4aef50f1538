"""CPU: the NumPy statement of the day-care-centre transmission model (tests/daycare_ref.py) reproduces recorded runs of
ELFI's own example on replayed draws (tests/golden/daycare.npz, scripts/make_golden_daycare.py: every centre a reference call of
its own with batch_size = 1, n_dcc = 1) -- final states and event counts bit for bit, the three counting summaries exactly,
Shannon bit for bit (NumPy's own log), the distance within n_ss n_dcc eps relative (a sum of that many non-negative terms
whose order may differ); the model graph has the reference's nodes and shapes; and the device functions refuse bad arguments
before any device context exists."""
import os

import numpy as np
import pytest

import daycare_ref as R


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'daycare.npz'))


SETS = ['true', 'prior', 'small_2_1', 'small_5_3', 'small_2_3', 'small_5_1', 'zero']


def golden_set(g, name):
    """(parameters (n_dcc, 3), E, U (n_dcc, 1, n_events), shape, time_end) of a recorded set: every centre a simulation of
    its own with one centre, as it was recorded."""
    n_dcc = g[name + '_state'].shape[0]
    E, U = R.golden_draws(g[name + '_seed'], n_dcc, int(g[name + '_n_events']))
    return g[name + '_params'], E[:, None, :], U[:, None, :], tuple(int(v) for v in g[name + '_shape']), float(g[name + '_time_end'])


def test_the_recorded_sets_are_the_ones_the_issue_asks_for(golden):
    assert list(golden['sets']) == SETS
    assert golden['true_state'].shape == golden['prior_state'].shape == (16, 36, 33)
    assert np.all(golden['true_params'] == [3.6, 0.6, 0.1]) and np.all(golden['zero_params'] == 0)
    shapes = {tuple(golden[name + '_shape']) for name in SETS if name.startswith('small')}
    assert {s[0] for s in shapes} == {2, 5} and {s[1] for s in shapes} == {1, 3}
    assert np.all(golden['zero_events'] == 1) and golden['prior_events'].max() > 400


@pytest.mark.parametrize('name', SETS)
def test_statement_is_the_recorded_run(golden, name):
    g = golden
    p, E, U, (n_ind, n_strains, n_obs), time_end = golden_set(g, name)
    state, T, status, events = R.simulate(p[:, 0], p[:, 1], p[:, 2], E, U, n_ind, n_strains, None, n_obs, time_end)
    assert state.dtype == np.bool_ and state.shape == (len(p), 1, n_obs, n_strains)
    assert np.array_equal(state[:, 0], g[name + '_state'])
    assert np.array_equal(events[:, 0], g[name + '_events'])
    assert np.all(status == R.REACHED_END) and np.all(T >= time_end)
    # the centres of the set as ONE simulation: the summaries and the distance by the reference's own functions
    S = R.summaries(state.transpose(1, 0, 2, 3), status.T)
    want = g[name + '_S']
    assert S.shape == (1, 4, len(p))
    for j in (1, 2, 3):
        assert np.array_equal(S[0, j], want[j])
    assert np.array_equal(S[0, 0], want[0])
    D, Dw = R.distance(S, g[name + '_obs']), g[name + '_D']
    assert D.shape == Dw.shape == (1,)
    assert abs(D[0] - Dw[0]) <= 4 * len(p) * R.EPS * abs(Dw[0])


def test_statement_marks_what_cannot_be_simulated():
    rs = np.random.RandomState(5)
    E, U = rs.exponential(size=(7, 2, 60)), rs.uniform(size=(7, 2, 60))
    t1 = np.array([3.6, np.nan, 0.0, 11.0, 3.6, 3.6, 3.6])
    t2 = np.array([0.6, 0.6, 0.0, 200.0, -0.1, 0.6, 0.6])
    t3 = np.array([0.1, 0.1, 0.0, 1.0, 0.1, np.inf, 2.5])
    state, T, status, events = R.simulate(t1, t2, t3, E, U, n_ind=8, n_strains=5, n_obs=6, time_end=1.)
    assert status[:, 0].tolist() == [R.REACHED_END, R.INVALID, R.REACHED_END, R.OUT_OF_EVENTS, R.INVALID, R.INVALID, R.REACHED_END]
    assert np.array_equal(status[:, 0], status[:, 1])
    assert events[2].tolist() == [1, 1] and events[3].tolist() == [60, 60] and not events[[1, 4, 5]].any()
    assert np.all(np.isnan(T[[1, 4, 5]])) and np.all(T[3] < 1.) and not state[[1, 4, 5]].any()
    S = R.summaries(state, status)
    assert np.all(np.isnan(S[[1, 3, 4, 5]])) and np.all(np.isfinite(S[[0, 2, 6]]))
    D = R.distance(S, S[0])
    assert D[0] == 0 and np.all(np.isnan(D[[1, 3, 4, 5]])) and np.all(np.isfinite(D[[2, 6]]))


def test_summaries_and_distance_corner_cases():
    state = np.zeros((2, 3, 4, 5), dtype=bool)                   # nobody carries anything: 0 / 0 -> 0, p == 0 -> 1
    state[1, 0, 0, 2] = state[1, 0, 1, 2] = state[1, 0, 1, 4] = True
    S = R.summaries(state)
    assert np.all(S[0] == 0) and not np.signbit(S[0, 1:]).any()
    p = np.array([2 / 3, 1 / 3])
    assert S[1, 0, 0] == -np.sum(p * np.log(p)) and S[1, 1:, 0].tolist() == [2, 0.5, 0.25]
    # an observed row of zeros is divided by 1; sorting makes the distance blind to the order of the centres
    obs = np.array([[0., 0., 0.], [3., 1., 2.]])
    X = np.array([[[1., 0., 2.], [1., 2., 3.]], [[2., 1., 0.], [3., 2., 1.]]])
    assert R.distance(X, obs).tolist() == [0.5, 0.5]
    X[1, 0, 1] = np.nan
    assert np.isnan(R.distance(X, obs)[1]) and R.distance(X, obs)[0] == 0.5


def test_draw_layout():
    E, U, A = R.draws(3, 9, 4, 3, 7)
    assert E.shape == U.shape == (4, 3, 7) and np.all(E >= 0) and np.all((U >= 0) & (U < 1)) and np.all((A > 0) & (A <= 1))
    E2, U2, _ = R.draws(3, 9, 2, 5, 12, first=2)           # simulation i of one call is simulation 0 of another; centres too
    assert np.array_equal(E2[:, :3, :7], E[2:]) and np.array_equal(U2[:, :3, :7], U[2:])
    assert not np.array_equal(R.draws(3, 10, 4, 3, 7)[0], E)
    assert len(np.unique(U)) == U.size


@pytest.mark.reference
def test_statement_is_the_reference_on_a_fresh_centre_and_model_graph():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi_amd
    from elfi.examples import daycare as dc
    # one fresh centre per shape
    for seed, (n_ind, n_strains, n_obs, time_end) in enumerate([(7, 4, 5, 3.), (53, 33, 36, 0.5)]):
        E, U = R.golden_draws(700 + seed, 1, 2000)
        replay = R.Replay(E[None], U[None])
        y = dc.daycare(3.6, 0.6, 0.1, n_dcc=1, n_ind=n_ind, n_strains=n_strains, n_obs=n_obs, time_end=time_end,
                       batch_size=1, random_state=replay)
        state, _, status, events = R.simulate(3.6, 0.6, 0.1, E[None], U[None], n_ind, n_strains, None, n_obs, time_end)
        assert np.array_equal(state, y) and events[0, 0] == replay.ke and status[0, 0] == R.REACHED_END
        for j, f in enumerate((dc.ss_shannon, dc.ss_strains, dc.ss_prevalence, dc.ss_prevalence_multi)):
            assert np.array_equal(R.summaries(state)[:, j], f(y))
    # the graph: the reference's node names, its observed summaries
    kw = dict(n_dcc=3, n_ind=6, n_strains=4, n_obs=5, time_end=1.)
    m, ref = elfi_amd.daycare_model(seed_obs=4, **kw), dc.get_model(seed_obs=4, **kw)
    public = [sorted(k for k in mdl.nodes if not k.startswith('_')) for mdl in (m, ref)]
    assert public[0] == public[1] == sorted(['t1', 't2', 't3', 'DCC', 'd', 'logd'] + list(R.NAMES))
    assert m.parameter_names == ref.parameter_names == ['t1', 't2', 't3']
    for name in R.NAMES:
        assert m[name].observed.shape == ref[name].observed.shape == (1, 3)
        assert np.array_equal(m[name].observed, ref[name].observed)
    assert m['DCC'].observed.shape == (1, 4, 3)
    assert sorted(m.get_parents('d')) == sorted(R.NAMES) and m.get_parents('logd') == ['d']


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    t = np.full(4, 0.5)
    E = np.ones((4, 29, 10))
    bad = [dict(n_ind=1), dict(n_ind=65), dict(n_strains=0), dict(n_strains=65), dict(n_obs=0), dict(n_obs=54), dict(n_dcc=0),
           dict(n_dcc=1025), dict(time_end=0.), dict(time_end=-1.), dict(time_end=np.inf), dict(time_end=np.nan),
           dict(max_events=0), dict(max_events=(1 << 21) + 1), dict(freq_strains_commun=np.full(32, 0.1)),
           dict(freq_strains_commun=np.full(33, -0.1)), dict(freq_strains_commun=np.full(33, np.nan)),
           dict(freq_strains_commun=np.full(33, np.inf)), dict(draws=(E, E[:3])), dict(draws=(E[0], E[0])),
           dict(draws=(E[:, :28], E[:, :28])), dict(observed=np.zeros((4, 28))), dict(observed=np.full((4, 29), np.nan)),
           dict(first_index=-1), dict(first_index=2 ** 32 - 3)]
    for kw in bad:
        with pytest.raises(ValueError):
            elfi_amd.daycare_summaries(t, t, t, **kw)
    with pytest.raises(ValueError):
        elfi_amd.daycare_summaries(t, t, np.zeros(3))               # a parameter of another batch size
    for kw in (dict(n=0, n_dcc=2, n_events=5), dict(n=3, n_dcc=0, n_events=5), dict(n=3, n_dcc=1025, n_events=5),
               dict(n=3, n_dcc=2, n_events=0), dict(n=3, n_dcc=2, n_events=(1 << 21) + 1),
               dict(n=3, n_dcc=2, n_events=5, first_index=-1)):
        with pytest.raises(ValueError):
            elfi_amd.daycare_draws(**kw)
    x = np.ones((5, 7))
    for args, obs in [((x, x), [x[:1]]), ((x,) * 17, [x[:1]] * 17), ((np.ones((5, 1025)),), [np.ones((1, 1025))]),
                      ((np.ones((5, 600)),) * 8, [np.ones((1, 600))] * 8), ((x, x), [x[:1], np.full((1, 7), np.inf)])]:
        with pytest.raises(ValueError):
            elfi_amd.daycare_distance(*args, observed=obs)
    with pytest.raises(ValueError):
        elfi_amd.daycare_model(true_params=[3.6, 0.6])


def test_library_refuses_bad_limits_without_a_device():
    """The C entry points check their arguments before they touch the device: a NULL context is refused, never a crash."""
    import elfi_amd
    lib = elfi_amd.load_library()
    assert lib.elfihip_daycare_summaries(None, *([None] * 2), 0, 0, 0, 1, 29, 53, 33, 36, 10., 100, *([None] * 11)) != 0
    assert lib.elfihip_daycare_draws(None, 0, 0, 0, 1, 29, 10, None, None) != 0
    assert lib.elfihip_daycare_distance(None, None, 1, 4, 29, None, None) != 0
