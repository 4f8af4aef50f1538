"""CPU: the NumPy statement of the birth-death-mutation model (tests/bdm_ref.py) reproduces recorded runs of the reference's
own simulator (tests/golden/bdm.npz, scripts/make_golden_bdm.py) exactly -- every cluster of every row, from a replay of the
binary's one generator per file; the given form on the replayed rows is the same run; the statement's T1 and T2 are the
reference's functions; the drawn form's uniforms have the documented layout; the model graph has the reference's nodes, prior
and observed data; and the device functions refuse bad arguments before any device context exists."""
import os

import numpy as np
import pytest

import bdm_ref as R
import philox_ref

SETS = ['truth', 'prior', 'slow', 'deaths', 'mode0', 'N1', 'N2', 'N64', 'N65', 'N473']
N_EVENTS = 1 << 11            # more than any recorded row needs (1419)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'bdm.npz'))


_replayed = {}


def replay(g, name):
    """a recorded set from its seed -> (params, N, mode, clusters, status, events, reopened, U); made once per set"""
    if name not in _replayed:
        p, N, mode = g[name + '_params'], int(g[name + '_N']), int(g[name + '_mode'])
        _replayed[name] = (p, N, mode) + R.replay(p, N, mode, int(g[name + '_seed']), N_EVENTS)
    return _replayed[name]


def test_the_recorded_sets_are_the_ones_the_issue_asks_for(golden):
    g = golden
    assert list(g['sets']) == SETS
    for name in SETS:
        assert g[name + '_params'].shape == (16, 3) and g[name + '_clusters'].shape == (16, int(g[name + '_N']))
        assert np.array_equal(g[name + '_params'], np.round(g[name + '_params'], 4))      # as the binary parsed them
    assert np.all(g['truth_params'] == [0.2, 0, 0.198]) and g['truth_N'] == 20 and g['truth_mode'] == 1
    assert g['prior_params'][0, 0] == 0.005 and g['prior_params'][-1, 0] == 2.005 and np.all(g['prior_params'][:, 1:] == [0, 0.198])
    assert np.all(g['deaths_params'][:, 1] > g['deaths_params'][:, 0] - 0.21) and np.sum(g['deaths_params'][:, 1] > 0.5) >= 8
    assert g['mode0_mode'] == 0 and [int(g[s + '_N']) for s in SETS[5:]] == [1, 2, 64, 65, 473]
    assert [int(g[s + '_seed']) for s in SETS[:4]] == [1, 12345, 777, 4000000000]
    # at least one extinct row, one mutation into a slot a death freed, one row above 400 events
    assert any((g[s + '_status'] == R.EXTINCT).any() for s in SETS)
    assert any(g[s + '_reopened'].any() for s in SETS)
    assert max(int(g[s + '_events'].max()) for s in SETS) > 400 and g['slow_events'].max() > 400
    assert g['dist_count'].shape == g['dist_largest'].shape == (4096,)
    assert g['dist_count'].min() >= 1 and g['dist_count'].max() <= 20 and g['dist_largest'].max() <= 20


@pytest.mark.parametrize('name', SETS)
def test_statement_is_the_recorded_run(golden, name):
    g = golden
    p, N, mode, Cl, st, ev, reopened, U = replay(g, name)
    assert Cl.shape == g[name + '_clusters'].shape and np.array_equal(Cl, g[name + '_clusters'])
    assert np.array_equal(ev, g[name + '_events']) and np.array_equal(st, g[name + '_status'])
    assert np.array_equal(reopened, g[name + '_reopened']) and ev.max() < N_EVENTS
    # a run ends at N individuals (mode 1: just before N + 1) or extinct
    total = Cl.sum(axis=1)
    assert np.all(total[st == R.REACHED_N] == N) and np.all(total[st == R.EXTINCT] == 0) and set(st) <= {0, 1}
    # the per-simulation rows that the replay cut from the one stream give the same run through the given form ...
    C2, s2, e2 = R.simulate(p[:, 0], p[:, 1], p[:, 2], N, mode, U)
    assert np.array_equal(C2, Cl) and np.array_equal(s2, st) and np.array_equal(e2, ev)
    # ... which reads nothing past the draws a simulation used, and stops short with fewer events
    V = U.copy()
    for i in range(len(p)):
        V[i, 2 * ev[i]:] = np.nan
    assert np.array_equal(R.simulate(p[:, 0], p[:, 1], p[:, 2], N, mode, V)[0], Cl)
    i = int(np.argmax(ev))
    if ev[i] > 1:
        c, s, e, _ = R.simulate_one(*p[i], N, mode, U[i], max_events=int(ev[i]) - 1)
        assert s == R.OUT_OF_EVENTS and e == ev[i] - 1


def test_uniforms_of_the_binary():
    """Two 32-bit words per double, the low word first; a value that rounds to 1 becomes the double below it."""
    bg = np.random.MT19937()
    bg._legacy_seeding(5489)
    assert int(bg.random_raw(10000)[-1]) == 4123659995           # the C++ standard's check value of mt19937
    u = R.mt_uniforms(1, 1000)
    assert u.dtype == np.float64 and np.all((u >= 0) & (u < 1)) and abs(u.mean() - 0.5) < 0.03
    raw = np.random.RandomState(1).randint(0, 2 ** 32, 4, dtype=np.uint64)       # the same generator, the same seeding
    assert u[0] == (float(raw[0]) + float(raw[1]) * 2.0 ** 32) / 2.0 ** 64


def test_status_and_edge_cases_of_the_statement():
    U = R.draws(3, 1, 4, 64)
    assert R.simulate_one(0.0, 0.0, 0.5, 20, 1, U[0])[1:3] == (R.OUT_OF_EVENTS, 64)             # mutations of a singleton for ever
    for bad in ((np.nan, 0, 0.1), (-0.1, 0, 0.1), (np.inf, 0, 0.1), (0, 0, 0), (0.1, -1e-300, 0.1), (1e308, 1e308, 0.1)):
        c, s, e, _ = R.simulate_one(*bad, 20, 1, U[0])
        assert s == R.INVALID and e == 0 and not c.any()
    c, s, e, _ = R.simulate_one(0.5, 0.1, 0.2, 1, 0, U[1])       # N = 1, mode 0: nothing happens
    assert (c.tolist(), s, e) == ([1], R.REACHED_N, 0)
    for value in (1.0, np.nan, -1e-9, 2.0):
        for col in (4, 5):
            V = U[2].copy()
            V[col] = value
            c, s, e, _ = R.simulate_one(0.3, 0.0, 0.2, 20, 1, V)
            assert s == R.INVALID and e == 2 and not c.any()
    T = R.summaries(np.zeros((1, 20), dtype=np.int32), [R.EXTINCT], 20)
    assert np.isnan(T[0, 0]) and T[0, 1] == 1.0
    assert np.isnan(R.summaries(np.ones((1, 20), dtype=np.int32), [R.OUT_OF_EVENTS], 20)).all()


def test_drawn_uniforms_have_the_documented_layout():
    U = R.draws(7, 2, 3, 5, first=11)
    assert U.shape == (3, 10) and np.all((U >= 0) & (U < 1))
    for i, k in ((0, 1), (2, 5), (1, 3)):
        w = philox_ref.philox4x32_10((k, 11 + i, 2, 0), (7, 0))
        assert U[i, 2 * (k - 1)] == ((w[0] << 21) | (w[1] >> 11)) * 2.0 ** -53
        assert U[i, 2 * (k - 1) + 1] == ((w[2] << 21) | (w[3] >> 11)) * 2.0 ** -53
    assert np.array_equal(R.draws(7, 2, 1, 5, first=12), U[1:2])


def _reference():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    from elfi.examples import bdm
    return bdm


def test_summaries_are_the_references(golden):
    bdm = _reference()
    for name in SETS:
        cl = golden[name + '_clusters']
        with np.errstate(all='ignore'):
            assert np.array_equal(R.T1(cl), bdm.T1(cl), equal_nan=True)
            for n in (20, int(golden[name + '_N']), 7.5):
                assert np.array_equal(R.T2(cl, n), bdm.T2(cl, n=n))
            T = R.summaries(cl, golden[name + '_status'], 20)
            assert np.array_equal(T[:, 0], bdm.T1(cl), equal_nan=True) and np.array_equal(T[:, 1], bdm.T2(cl))


def test_model_graph_is_the_references():
    import warnings
    bdm = _reference()
    import elfi_amd
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                # the reference warns that its executable is missing
        ref = bdm.get_model()
    with warnings.catch_warnings():
        warnings.simplefilter('error')                 # the device model has no executable to miss
        m = elfi_amd.bdm_model()
    public = [sorted(k for k in mdl.nodes if not k.startswith('_')) for mdl in (m, ref)]
    assert public[0] == public[1] == sorted(['alpha', 'BDM', 'T1', 'd'])
    assert m.name == ref.name == 'bdm' and m.parameter_names == ref.parameter_names == ['alpha']
    assert m['BDM'].observed.dtype == ref['BDM'].observed.dtype == np.int16
    assert np.array_equal(m['BDM'].observed, ref['BDM'].observed) and m['BDM'].observed.shape == ref['BDM'].observed.shape
    assert m['BDM'].observed.reshape(-1).tolist() == [6, 3, 2, 2, 1, 1, 1, 1, 1, 1, 1] + [0] * 9
    assert np.array_equal(m['T1'].observed, ref['T1'].observed) and m['T1'].observed.reshape(-1).tolist() == [11 / 20]
    assert m.get_parents('d') == ['T1'] and m.get_parents('T1') == ['BDM'] and m.get_parents('BDM')[0] == 'alpha'
    for mdl in (m, ref):
        assert [mdl[p].state['attr_dict']['_output'] for p in mdl.get_parents('alpha')] == [.005, 2]
        assert [mdl[p].state['attr_dict']['_output'] for p in mdl.get_parents('BDM')[1:]] == [0, 0.198, 20]
    assert m['alpha'].distribution is elfi_amd.priors.uniform and ref['alpha'].state['attr_dict']['distribution'] == 'uniform'
    d = m['d'].state['attr_dict']['_operation'].args[0]
    assert d.metric == 'minkowski' and d.p == 1
    assert elfi_amd.bdm_model(device_priors=False)['alpha'].state['attr_dict']['distribution'] == 'uniform'


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    a = np.full(4, 0.2)
    U = np.zeros((4, 64))
    bad = [dict(N=0), dict(N=4097), dict(mode=2), dict(mode=-1), dict(max_events=0), dict(max_events=2 ** 30 + 1),
           dict(first_index=-1), dict(first_index=2 ** 32 - 3), dict(draws=U[0]), dict(draws=U[:, :63]), dict(draws=U[:, :0]),
           dict(draws=U[:3]), dict(observed=[0.5, 0.5]), dict(delta=np.zeros(3))]
    for kw in bad:
        with pytest.raises(ValueError):
            elfi_amd.bdm_clusters(a, **kw)
    for args, kw in (((0, 8), {}), ((2, 0), {}), ((2, 2 ** 30 + 1), {}), ((2, 8), dict(first_index=-1)),
                     ((2, 8), dict(first_index=2 ** 32 - 1))):
        with pytest.raises(ValueError):
            elfi_amd.bdm_draws(*args, **kw)


def test_library_refuses_bad_limits_without_a_device():
    """The C entry points check their arguments before they touch the device: a NULL context is refused, never a crash."""
    import elfi_amd
    lib = elfi_amd.load_library()
    assert lib.elfihip_bdm_clusters(None, None, 0, 0, 0, 1, 20, 1, 64, None, None, None, 20.0, *([None] * 6)) != 0
    assert lib.elfihip_bdm_clusters_dev(None, None, 0, 0, 0, 0, 1, 20, 1, 64, None, None, None, 20.0, None, None, 20, None, None,
                                        None, 2, None) != 0
    assert lib.elfihip_bdm_draws(None, 0, 0, 0, 1, 8, None) != 0
    assert lib.elfihip_bdm_draws_dev(None, 0, 0, 0, 1, 8, None, 16) != 0
