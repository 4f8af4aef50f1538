"""CPU: the NumPy statement of the stochastic Lorenz-96 model (tests/lorenz_ref.py) is ELFI's own example bit for bit --
pinned to recorded runs (tests/golden/lorenz.npz, scripts/make_golden_lorenz.py) and, where the reference is present, to
fresh runs; the summation orders the kernel implements (sequential along time, NumPy's pairwise sum over the flattened
terms) are np.mean's and np.var's; and elfi_amd.lorenz_summaries refuses bad arguments before any device context exists."""
import os
import re

import numpy as np
import pytest

import lorenz_ref as R

from conftest import ROOT


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'lorenz.npz'))


def _replay(seed, B, T, K):
    return R.lorenz_noise_from_state(np.random.RandomState(int(seed)), B, T, K)


def test_default_block_is_the_recorded_one(golden):
    g = golden
    assert g['default_X'].shape == (2, 160, 40) and g['y0_default'].shape == (40,)
    c, h = R.lorenz_constants(0.984, 160, 4)
    X = R.lorenz_series(g['default_t1'], g['default_t2'], _replay(g['default_seed'], 2, 160, 40), g['y0_default'], 10., c,
                        0.984, h)
    assert np.array_equal(X, g['default_X'])
    assert np.array_equal(X[:, 0], np.tile(g['y0_default'], (2, 1)))
    assert np.array_equal(R.lorenz_summaries(X), g['default_S'])
    assert np.array_equal(R.lorenz_summaries_explicit(X), g['default_S'])


def test_small_block_with_its_own_initial_states_is_the_recorded_one(golden):
    g = golden
    assert g['small_X'].shape == (16, 20, 8) and g['small_y0'].shape == (16, 8)
    c, h = R.lorenz_constants(0.984, 20, 4)
    X = R.lorenz_series(g['small_t1'], g['small_t2'], _replay(g['small_seed'], 16, 20, 8), g['small_y0'], 10., c, 0.984, h)
    assert np.array_equal(X, g['small_X'])
    assert np.array_equal(R.lorenz_summaries(X), g['small_S'])
    assert np.array_equal(R.lorenz_summaries_explicit(X), g['small_S'])


def test_end_to_end_record_is_complete(golden):
    g = golden
    assert list(g['e2e_settings']) == [4, 5000, 2, 200, 20000]
    assert g['e2e_centre'].shape == g['e2e_margin'].shape == (2,) and g['e2e_obs'].shape == (6,)
    # the centre lies inside the priors U(0.5, 3.5) and U(0, 0.3); four standard errors of a 200-sample mean are narrower
    # than the prior's own standard error
    assert 0.5 < g['e2e_centre'][0] < 3.5 and 0 < g['e2e_centre'][1] < 0.3
    assert np.all(g['e2e_margin'] > 0) and np.all(g['e2e_margin'] < 4 * np.array([3.0, 0.3]) / np.sqrt(12 * 200))


# T K = 132: one split of the pairwise sum; (T - 1) K = 35, 10, 18: not multiples of 8; 4 = the in-order branch; 8192 =
# NumPy's whole reduction buffer (64 leaves of 128) and 8128 - 64 terms below it; 21 x 7: odd everything
@pytest.mark.parametrize('B,T,K', [(5, 33, 4), (3, 2, 4), (7, 3, 5), (3, 21, 7), (2, 8, 5), (4, 3, 9), (2, 128, 64),
                                   (1, 127, 64), (3, 160, 40), (2, 2047, 4), (1, 585, 14)])
def test_explicit_orders_are_numpys(B, T, K):
    rs = np.random.RandomState(1000 * T + K)
    X = rs.randn(B, T, K) * rs.uniform(0.1, 30, K) + rs.uniform(-5, 5, K)
    S = R.lorenz_summaries_explicit(X)
    assert np.array_equal(S, R.lorenz_summaries(X))
    # ... and, written out with np.mean / np.var as the reference's summary functions have them
    assert np.array_equal(S[:, 0], np.mean(X, axis=(1, 2)))
    assert np.array_equal(S[:, 1], np.mean(np.var(X, axis=1), axis=1))
    head, tail = X[:, :-1], X[:, 1:]
    assert np.array_equal(S[:, 2], np.mean((head - np.mean(head, keepdims=True, axis=1)) *
                                           (tail - np.mean(tail, keepdims=True, axis=1)), axis=(1, 2)))
    # the mean of a rolled array is the neighbour column's mean: the same additions
    assert np.array_equal(np.mean(np.roll(X, -1, axis=2), axis=1), np.roll(np.mean(X, axis=1), -1, axis=1))


def test_pairwise_sum_is_np_sum_at_every_length():
    rs = np.random.RandomState(3)
    a = rs.randn(8192) * 10 ** rs.uniform(-3, 3, 8192)
    for n in list(range(1, 300)) + [1023, 1024, 1031, 4103, 6360, 6400, 8128, 8191, 8192]:
        assert R.pairwise(list(a[:n])) == np.sum(a[:n]), n


@pytest.mark.reference
def test_restatement_is_the_reference_on_fresh_seeds():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    from elfi.examples import lorenz

    class Given(np.ndarray):      # forecast_lorenz tests `if not initial_state`
        def __bool__(self):
            return True
    for seed, (B, T, K) in enumerate([(1, 160, 40), (16, 20, 8), (5, 33, 4), (3, 2, 4), (4, 128, 64), (7, 3, 5)]):
        rs = np.random.RandomState(seed)
        t1, t2, y0 = rs.uniform(0.5, 3.5, B), rs.uniform(0, 0.3, B), 3.0 * rs.randn(B, K)
        if seed == 2:
            t2[-1] = -5.0            # the series overflows: the same non-finite values
        with np.errstate(all='ignore'):
            X = np.asarray(lorenz.forecast_lorenz(t1, t2, n_obs=K, n_timestep=T, batch_size=B, initial_state=y0.view(Given),
                                                  random_state=np.random.RandomState(3000 + seed)))
            S = np.column_stack([lorenz.mean(X), lorenz.var(X), lorenz.autocov(X), lorenz.cov(X), lorenz.xcov(X, True),
                                 lorenz.xcov(X, False)])
        c, h = R.lorenz_constants(0.984, T, 4)
        Xr = R.lorenz_series(t1, t2, _replay(3000 + seed, B, T, K), y0, 10., c, 0.984, h)
        assert np.array_equal(Xr, X, equal_nan=True)
        assert seed != 2 or not np.all(np.isfinite(X[-1]))
        assert np.array_equal(R.lorenz_summaries(X), S, equal_nan=True)
        assert np.array_equal(R.lorenz_summaries_explicit(X), S, equal_nan=True)


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    t, y0 = np.full(4, 1.0), np.zeros(40)
    bad = [dict(n_obs=3, initial_state=np.zeros(3)), dict(n_obs=65, initial_state=np.zeros(65)), dict(n_timestep=1),
           dict(n_timestep=205), dict(n_obs=64, n_timestep=129, initial_state=np.zeros(64)),
           dict(initial_state=np.zeros(39)), dict(initial_state=np.zeros((3, 40))), dict(initial_state=np.zeros((4, 2, 40))),
           dict(initial_state=None), dict(noise=np.zeros((4, 160, 40))), dict(noise=np.zeros((4, 159, 39))),
           dict(noise=np.zeros((4, 159 * 40))), dict(noise=np.zeros((3, 159, 40))), dict(observed=np.zeros(5)),
           dict(phi=1.5)]
    for kw in bad:
        kw.setdefault('initial_state', y0)
        with pytest.raises(ValueError):
            elfi_amd.lorenz_summaries(t, t, **kw)
    with pytest.raises(AssertionError, match='device context'):      # good arguments do reach the device
        elfi_amd.lorenz_summaries(t, t, y0)


def test_symbols_are_declared_exported_and_bound():
    from elfi_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'elfihip.h')).read()
    export = open(os.path.join(ROOT, 'elfi_amd', 'csrc', 'export.map')).read()
    assert re.search(r'global:\s*elfihip_\*;', export)
    for name in ('elfihip_lorenz_summaries', 'elfihip_lorenz_summaries_dev'):
        assert re.search(r'\bint %s\(' % name, header) and name in _lib.PROTOTYPES
    # the prototypes carry as many arguments as the declarations
    for name in ('elfihip_lorenz_summaries', 'elfihip_lorenz_summaries_dev'):
        decl = re.search(r'\bint %s\((.*?)\);' % name, header, flags=re.S).group(1)
        assert len(decl.split(',')) == len(_lib.PROTOTYPES[name][1])
    import elfi_amd
    assert elfi_amd.lorenz_summaries is elfi_amd.summaries.lorenz_summaries
    assert elfi_amd.lorenz_model is elfi_amd.fused_models.lorenz_model
