"""CPU: the NumPy statement of the g-and-k models (tests/gnk_ref.py) is ELFI's own examples bit for bit -- pinned to
recorded runs (tests/golden/gnk.npz, scripts/make_golden_gnk.py) and, where the reference is present, to fresh runs --
the recorded error of the reference's own series is what the file's 40-digit values give, the octile positions are
np.percentile's, the device functions refuse bad arguments before any device context exists, and the device models have
the reference models' nodes and observed shapes."""
import os

import numpy as np
import pytest

import gnk_ref as R

BLOCKS = ('gnk', 'bignk', 'edge', 'biedge')


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'gnk.npz'))


def test_golden_shapes(golden):
    g = golden
    assert g['gnk_z'].shape == (64, 50) and g['gnk_y'].shape == (64, 50, 1) and g['gnk_P'].shape == (64, 4)
    assert g['bignk_z'].shape == g['bignk_y'].shape == (16, 150, 2) and g['bignk_P'].shape == (16, 9)
    assert g['gnk_octile'].shape == (64, 7, 1) and g['bignk_octile'].shape == (16, 14, 1)
    assert g['gnk_robust'].shape == (64, 4, 1) and g['bignk_robust'].shape == (16, 8, 1)
    assert not g['gnk_order_swaps'].any() and not g['edge_order_swaps'].any()      # one value per observation: nothing to sort
    assert g['bignk_order_swaps'].any() and not g['bignk_order_swaps'].all()


@pytest.mark.parametrize('block', BLOCKS)
def test_series_summaries_and_distance_are_the_recorded_ones(golden, block):
    g = golden
    y = R.series(g[block + '_P'], g[block + '_z'])
    assert np.array_equal(y, g[block + '_y'], equal_nan=True)
    assert np.array_equal(np.isnan(y), np.isnan(g[block + '_y']))
    recorded = dict(order=R.order_from_swaps(g[block + '_y'], g[block + '_order_swaps']), octile=g[block + '_octile'],
                    robust=g[block + '_robust'])
    for name, fn in (('order', R.ss_order), ('octile', R.ss_octile), ('robust', R.ss_robust)):
        s = fn(y)
        assert s.shape == recorded[name].shape and np.array_equal(s, recorded[name], equal_nan=True), name
        assert np.array_equal(R.euclidean_multiss(s, s[:1]), g[block + '_d_' + name], equal_nan=True), name
    # the summaries against NumPy's own calls
    with np.errstate(all='ignore'):
        E = np.percentile(y, R.OCTILES, axis=1)
    assert np.array_equal(R.octiles(y), E, equal_nan=True)
    assert np.array_equal(R.sorted_rows(y), np.sort(y, axis=1), equal_nan=True)


def test_edge_rows_are_what_they_are_named(golden):
    g = golden
    names = list(g['edge_names'])
    y, rob = g['edge_y'][:, :, 0], g['edge_robust'][:, :, 0]
    i = names.index('overflow')
    assert np.array_equal(np.flatnonzero(np.isnan(y[i])), [3, 10, 49]) and np.all(g['edge_z'][i, [3, 10, 49]] <= -2)
    assert np.isnan(rob[i]).all() and np.isnan(g['edge_octile'][i]).all() and np.isnan(g['edge_d_robust'][i])
    assert np.isnan(g['edge_d_order'][i]) and np.isfinite(np.delete(y, i, axis=0)).all()
    assert np.isfinite(np.delete(g['edge_d_robust'], i)).all()
    i = names.index('B0')
    assert np.all(y[i] == 3.0) and np.array_equal(rob[i], [3.0, R.EPS, 0.0, 0.0])
    assert g['edge_P'][names.index('g0'), 2] == 0 and g['edge_P'][names.index('kneg'), 3] == -0.5
    assert g['edge_P'][names.index('gneg'), 2] < 0
    i = names.index('zero')
    assert g['edge_z'][i, 5] == 0 and y[i, 5] == 3.0 and y[i, 6] == 3.0
    i = names.index('ties')
    assert np.unique(y[i]).shape[0] == 50 - 9 - 3
    bn = list(g['biedge_names'])
    yb = g['biedge_y']
    assert g['biedge_P'][bn.index('rho_plus'), 8] == 1 and g['biedge_P'][bn.index('rho_minus'), 8] == -1
    i = bn.index('overflow_d0')
    assert np.array_equal(np.argwhere(np.isnan(yb)), [[i, 7, 0], [i, 29, 0]])
    assert np.array_equal(np.isnan(g['biedge_robust'][i, :, 0]), [True, False] * 4)
    assert np.array_equal(np.isnan(g['biedge_octile'][i, :, 0]), [True, False] * 7)


def test_e_ref_is_what_the_file_gives(golden):
    g = golden
    assert R.e_ref(g) == float(g['E_ref'])
    assert 1.0 < float(g['E_ref']) < 20.0          # a few units: roundings amplified by a bracket as small as 0.2
    for p in ('gnk', 'bignk'):                      # the pair is a double-double: hi is the rounded value, |lo| <= ulp(hi) / 2
        assert np.all(np.abs(g[p + '_y_lo']) <= 0.5 * np.spacing(np.abs(g[p + '_y_hi'])))
        assert np.all(np.isfinite(g[p + '_y']))


@pytest.mark.parametrize('n_obs', [2, 8, 50, 150])
def test_octile_positions_reproduce_np_percentile(n_obs):
    from elfi_amd.summaries import GNK_OCTILES, quantile_positions
    assert np.array_equal(GNK_OCTILES, R.OCTILES)
    lo, hi, t = quantile_positions(np.true_divide(GNK_OCTILES, 100), n_obs)
    rlo, rhi, rt = R.octile_positions(n_obs)
    assert lo.dtype == hi.dtype == np.int32
    assert np.array_equal(lo, rlo) and np.array_equal(hi, rhi) and np.array_equal(t, rt)
    rs = np.random.RandomState(n_obs)
    y = rs.standard_normal((9, n_obs, 2)) * 3
    y[3, : n_obs // 2, 0] = y[3, 0, 0]          # ties
    assert np.array_equal(R.octiles(y), np.percentile(y, GNK_OCTILES, axis=1))
    y[1, n_obs // 2, 1] = np.nan                # np.percentile answers NaN for the whole column
    assert np.array_equal(R.octiles(y), np.percentile(y, GNK_OCTILES, axis=1), equal_nan=True)
    assert np.isnan(R.octiles(y)[:, 1, 1]).all() and np.isfinite(R.octiles(y)[:, 1, 0]).all()


def test_pairwise_and_left_to_right_sums_differ_but_within_the_bound(golden):
    """euclidean_multiss sums a (batch, m, 1) summary pairwise, the library left to right: the same m non-negative terms."""
    import series_ref
    g = golden
    s = g['gnk_y']
    d_lr = series_ref.weighted_euclidean(s[:, :, 0], s[0, :, 0])
    d = g['gnk_d_order']
    assert np.all(np.abs(d_lr - d) <= 50 * R.EPS * d)


def _reference():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi
    return elfi


@pytest.mark.reference
def test_restatement_is_the_reference_on_fresh_seeds():
    _reference()
    from elfi.examples import bignk, gnk
    for seed, (B, n_obs) in enumerate([(1, 50), (33, 37), (20, 130), (7, 2)]):
        rs = np.random.RandomState(seed)
        P = rs.uniform(0, 10, (B, 4))
        y = gnk.GNK(*P.T, n_obs=n_obs, batch_size=B, random_state=np.random.RandomState(3000 + seed))
        z = R.gnk_draws_from_state(np.random.RandomState(3000 + seed), B, n_obs)
        assert np.array_equal(R.series(P, z), y)
        for mine, ref in ((R.ss_order, gnk.ss_order), (R.ss_octile, gnk.ss_octile), (R.ss_robust, gnk.ss_robust)):
            assert np.array_equal(mine(y), ref(y))
            assert np.array_equal(R.euclidean_multiss(mine(y), mine(y)[:1]), gnk.euclidean_multiss(ref(y), observed=(ref(y)[:1],)))
    for seed, (B, n_obs) in enumerate([(1, 150), (9, 11), (5, 64)]):
        rs = np.random.RandomState(60 + seed)
        P = np.column_stack([rs.uniform(0, 5, (B, 4)), rs.uniform(-5, 5, (B, 2)), rs.uniform(-.5, 5, (B, 2)),
                             rs.uniform(-0.99, 0.99, B)])
        y = bignk.BiGNK(*P.T, n_obs=n_obs, batch_size=B, random_state=np.random.RandomState(4000 + seed))
        z = R.bignk_draws_from_state(np.random.RandomState(4000 + seed), P[:, 8], n_obs)
        assert z.shape == (B, n_obs, 2) and np.array_equal(R.series(P, z), y)
        for mine, ref in ((R.ss_order, gnk.ss_order), (R.ss_octile, gnk.ss_octile), (R.ss_robust, gnk.ss_robust)):
            assert np.array_equal(mine(y), ref(y))


def _named(model):
    """The nodes a user names (constants get hidden nodes with generated names)."""
    return sorted(n for n in model.nodes if not n.startswith('_'))


@pytest.mark.reference
@pytest.mark.parametrize('device_priors', [True, False])
def test_models_have_the_reference_models_nodes_and_observed_shapes(device_priors):
    _reference()
    from elfi.examples import bignk, gnk
    import elfi_amd
    ref = gnk.get_model(n_obs=50, seed=4)
    m = elfi_amd.gnk_model(n_obs=50, seed=4, device_priors=device_priors)
    assert _named(m) == _named(ref) == sorted(['A', 'B', 'g', 'k', 'GNK', 'ss_order', 'd'])
    assert m.parameter_names == ref.parameter_names
    assert np.array_equal(m['ss_order'].observed, ref['ss_order'].observed) and m['ss_order'].observed.shape == (1, 50, 1)
    for name, length in (('octile', 7), ('robust', 4), ('sorted', 50)):
        mm = elfi_amd.gnk_model(n_obs=50, seed=4, summary=name, device_priors=device_priors)
        assert 'ss_' + name in mm.nodes and mm['ss_' + name].observed.shape == (1, length, 1)
    ref = bignk.get_model(n_obs=150, seed=4)
    m = elfi_amd.bignk_model(n_obs=150, seed=4, device_priors=device_priors)
    assert _named(m) == _named(ref)
    assert m.parameter_names == ref.parameter_names == ['a1', 'a2', 'b1', 'b2', 'g1', 'g2', 'k1', 'k2', 'rho']
    assert np.array_equal(m['ss_robust'].observed, ref['ss_robust'].observed) and m['ss_robust'].observed.shape == (1, 8, 1)
    assert elfi_amd.bignk_model(seed=4, summary='octile')['ss_octile'].observed.shape == (1, 14, 1)
    with pytest.raises(ValueError):
        elfi_amd.bignk_model(summary='order')
    with pytest.raises(ValueError):
        elfi_amd.gnk_model(summary='median')


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib
    from elfi_amd.summaries import SERIES_MAX_OBS

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    t = np.full(4, 0.5)
    bad = [dict(n_obs=1), dict(n_obs=SERIES_MAX_OBS + 1), dict(z=np.zeros((4, 49))), dict(z=np.zeros(50)),
           dict(z=np.zeros((4, 50, 1))), dict(z=np.zeros((3, 50))), dict(summary='median'), dict(summary=()),
           dict(summary=('robust', 'mean')), dict(summary=None), dict(observed=np.zeros(5)),
           dict(summary='octile', observed=np.zeros(4)), dict(summary=('order', 'robust'), observed=np.zeros(4)),
           dict(summary='sorted', observed=np.zeros(49))]
    for kw in bad:
        with pytest.raises(ValueError):
            elfi_amd.gnk_summaries(t, t, t, t, **kw)
    with pytest.raises(ValueError):
        elfi_amd.gnk_summaries(t, t, np.zeros(3), t)                # a parameter of another batch size
    p = [t] * 8
    bad2 = [dict(n_obs=1), dict(n_obs=SERIES_MAX_OBS // 2 + 1), dict(z=np.zeros((4, 150))), dict(z=np.zeros((4, 150, 1))),
            dict(z=np.zeros((4, 149, 2))), dict(z=np.zeros((3, 150, 2))), dict(summary='median'),
            dict(observed=np.zeros(4)), dict(summary='octile', observed=np.zeros(7))]
    for kw in bad2:
        with pytest.raises(ValueError):
            elfi_amd.bignk_summaries(*p, 0.5, **kw)
    for rho in (1.5, -1.0000001, np.nan, np.array([0.1, 0.2, 0.3, 1.01])):
        with pytest.raises(ValueError):
            elfi_amd.bignk_summaries(*p, rho)
    with pytest.raises(ValueError):
        elfi_amd.bignk_summaries(*p, np.zeros(3))
