"""CPU: the NumPy statement of the AR(1) model (tests/ar1_ref.py) reproduces recorded runs of ELFI's own example
(tests/golden/bdm.npz, scripts/make_golden_bdm.py) bit for bit; the model graph has the reference's nodes, prior and observed
series; and the device function refuses bad arguments before any device context exists."""
import os

import numpy as np
import pytest

import ar1_ref as A


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'bdm.npz'))


def test_statement_is_the_recorded_run(golden):
    g = golden
    assert g['ar1_runs'] == 4
    for k in range(int(g['ar1_runs'])):
        X, phi, seed = g['ar1_%d_X' % k], float(g['ar1_%d_phi' % k]), int(g['ar1_%d_seed' % k])
        batch, n_obs = X.shape
        W = A.noise_from_state(np.random.RandomState(seed), batch, n_obs)
        got = A.series(phi, W)
        assert got.dtype == np.float64 and got.shape == X.shape and np.array_equal(got, X)
    assert g['ar1_0_X'].shape == (3, 200) and g['ar1_0_phi'] == 0.9


def test_statement_rounds_the_product_first_and_propagates_specials():
    W = np.random.RandomState(3).randn(5, 9)
    X = A.series([0.0, 0.9, -1.0, np.nan, np.inf], W)
    assert np.array_equal(X[0], W[0, 1:]) and X[1, 0] == W[1, 1] and X[1, 1] == 0.9 * W[1, 1] + W[1, 2]
    assert np.isnan(X[3]).all() and np.isnan(X[4]).all()              # inf * 0 = NaN at i = 1
    big = A.series(1.5, np.ones((1, 2049)))
    assert np.isinf(big[0, -1]) and np.isfinite(big[0, 1000])


def test_model_graph_is_the_references():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi_amd
    from elfi.examples import ar1
    m, ref = elfi_amd.ar1_model(seed_obs=4), ar1.get_model(seed_obs=4)
    public = [sorted(k for k in mdl.nodes if not k.startswith('_')) for mdl in (m, ref)]
    assert public[0] == public[1] == sorted(['phi', 'AR1', 'd'])
    assert m.parameter_names == ref.parameter_names == ['phi']
    assert m['AR1'].observed.shape == ref['AR1'].observed.shape == (1, 200) and np.array_equal(m['AR1'].observed, ref['AR1'].observed)
    assert m.get_parents('d') == ['AR1'] and m.get_parents('AR1') == ['phi']
    for mdl in (m, ref):
        assert [mdl[p].state['attr_dict']['_output'] for p in mdl.get_parents('phi')] == [-1, 2]
    assert m['phi'].distribution is elfi_amd.priors.uniform and ref['phi'].state['attr_dict']['distribution'] == 'uniform'
    assert m['d'].state['attr_dict']['_operation'].args[0].metric == 'euclidean'
    m2, r2 = elfi_amd.ar1_model(n_obs=7, true_params=[-0.3], seed_obs=2, device_priors=False), ar1.get_model(7, [-0.3], 2)
    assert np.array_equal(m2['AR1'].observed, r2['AR1'].observed) and m2['AR1'].observed.shape == (1, 7)


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    phi = np.full(4, 0.5)
    for kw in (dict(n_obs=0), dict(n_obs=2049), dict(noise=np.zeros((4, 200))), dict(noise=np.zeros(201)),
               dict(noise=np.zeros((3, 201))), dict(observed=np.zeros(199)), dict(noise=np.zeros((0, 201)))):
        with pytest.raises(ValueError):
            elfi_amd.ar1_series(phi, **kw)
    with pytest.raises(ValueError):
        elfi_amd.ar1_model(true_params=[0.5, 0.5])
    lib = elfi_amd.load_library()
    assert lib.elfihip_ar1_series(None, None, 0, 0, 1, 200, None, None, None, None) != 0
    assert lib.elfihip_ar1_series_dev(None, None, 201, 0, 0, 1, 200, None, None, None, 200, None) != 0
