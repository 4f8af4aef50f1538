"""CPU: the NumPy statement of Marchand's toad model (tests/toad_ref.py) reproduces recorded runs of ELFI's own example on
replayed draws (tests/golden/toad.npz, scripts/make_golden_toad.py) bit for bit -- the positions X and all 48 summaries, inf
patterns included, on both sides of np.nanmedian's change of path at 600 displacements; its alpha-stable step lies within
its own first-order bound B of a 50-digit evaluation of the same expression on the same doubles, on the inputs the GPU test
of the sampler uses (which makes `within B of the exact value` a condition the reference itself meets, so that the device
may be held to 2 B of it); and the device functions refuse bad arguments before any device context exists."""
import os

import numpy as np
import pytest

import toad_ref as R

SETS = ['true', 'prior', 'p0_one', 'p0_zero', 'gamma_zero', 'alpha_one', 'alpha_two', 'small_585', 'small_603', 'small_2']
LAGS = (1, 2, 4, 8)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'toad.npz'))


def golden_set(g, name):
    """(alpha, gamma, p0, (U, TH, W, R), X, S) of a recorded set; the draws replayed from the recorded seed."""
    n_toads, n_days = (int(v) for v in g[name + '_shape'])
    p = g[name + '_params']
    draws = R.draws_from_state(np.random.RandomState(int(g[name + '_seed'])), n_toads, n_days, p.shape[0])
    return p[:, 0], p[:, 1], p[:, 2], draws, g[name + '_X'], g[name + '_S']


def test_the_recorded_sets_are_the_ones_the_issue_asks_for(golden):
    g = golden
    assert list(g['sets']) == SETS and tuple(g['lags']) == LAGS
    assert np.all(g['true_params'] == [1.7, 35., 0.6]) and g['true_X'].shape == (1, 63, 66)
    assert g['prior_X'].shape == (8, 63, 66) and g['prior_S'].shape == (8, 48)
    lo, hi = g['prior_params'].min(axis=0), g['prior_params'].max(axis=0)
    assert np.all(lo >= [1, 0, 0]) and np.all(hi <= [2, 100, 0.9])
    assert g['p0_one_params'][0, 2] == 1 and g['p0_zero_params'][0, 2] == 0 and g['gamma_zero_params'][0, 1] == 0
    assert g['alpha_one_params'][0, 0] == 1 and g['alpha_two_params'][0, 0] == 2
    # every toad returned (or none moved): the counts are the displacement counts, every other column is inf
    for name in ('p0_one', 'gamma_zero'):
        S = g[name + '_S'].reshape(4, 12)
        assert S[:, 0].tolist() == [66 * (63 - lag) for lag in LAGS] and np.all(np.isposinf(S[:, 1:]))
    # nobody returns: the 4 092 displacements of lag 1 less the steps that happen to be shorter than thd (with thd = 0 the
    # GPU test sorts all 4 092 of this set)
    assert 3000 < 4092 - g['p0_zero_S'][0, 0] <= 4092 and np.all(np.isfinite(g['p0_zero_S']))
    # displacement counts on both sides of np.nanmedian's 600
    counts = {name: [int(g[name + '_shape'][0]) * (int(g[name + '_shape'][1]) - lag) for lag in LAGS] for name in SETS[7:]}
    assert counts['small_585'][0] == 585 and counts['small_603'][:2] == [603, 536] and counts['small_2'][3] == 2
    assert g['cdf_p'].shape == (2, 3) and list(g['cdf_alpha']) == [0.8, 1.5]


@pytest.mark.parametrize('name', SETS)
def test_statement_is_the_recorded_run(golden, name):
    alpha, gamma, p0, (U, TH, W, Rr), X, S = golden_set(golden, name)
    dx, B = R.stable_step(alpha[:, None, None], gamma[:, None, None], TH, W)
    got = R.simulate(alpha, gamma, p0, U, dx, Rr)
    assert got.shape == X.shape and np.array_equal(got, X)
    Sg = R.all_summaries(got, LAGS)
    assert Sg.shape == S.shape == (len(alpha), 48)
    assert np.array_equal(Sg, S)                       # (inf == inf: the inf patterns are part of it; no NaN is left)
    assert not np.isnan(S).any() and np.array_equal(np.isinf(Sg), np.isinf(S))


def exact_step(alpha, scale, TH, W):
    """The expression of stable_step on the same doubles in 50-digit arithmetic."""
    import mpmath as mp
    mp.mp.dps = 50
    al, sc, th, w = (mp.mpf(float(v)) for v in (alpha, scale, TH, W))
    if al == 1:
        return mp.mpf(R.TWO_BY_PI) * (mp.mpf(R.HALF_PI) * mp.tan(th)) * sc
    ath = al * th
    return w / (mp.cos(th) / mp.tan(ath) + mp.sin(th)) * ((mp.cos(ath) + mp.sin(ath) * mp.tan(th)) / w) ** (1 / al) * sc


def test_numpy_step_is_within_its_bound_of_the_exact_value():
    import mpmath as mp
    alpha, scale, TH, W = R.step_inputs()
    x, B = R.stable_step(alpha, scale, TH, W)
    valid = R.stable_valid(alpha, scale)
    assert np.array_equal(np.isnan(x), ~valid) and np.all(B[~valid] == 0) and 500 < (~valid).sum() < 1000
    compared = R.step_mask(x, B)
    assert not compared[~valid].any()
    share = (valid & ~compared).mean()
    print('masked share', share)
    assert share <= R.MASK_SHARE
    assert (alpha[compared] == 1).sum() >= 1500 and (alpha[compared] == 2).sum() >= 1500
    assert (R.HALF_PI - np.abs(TH[compared]) < 1e-10).sum() > 1000
    worst = 0.0
    for i in np.flatnonzero(compared):
        err = abs(mp.mpf(float(x[i])) - exact_step(alpha[i], scale[i], TH[i], W[i]))
        if B[i] == 0:
            assert err == 0
            continue
        worst = max(worst, float(err / mp.mpf(float(B[i]))))
    print('worst |numpy - exact| / B', worst)
    assert worst <= 1.0


def test_summaries_corner_cases():
    # sort sizes 0, 1, 2 and a non-power of two; NaN displacements are neither counted nor sorted
    X = np.zeros((5, 4, 3))
    X[1, 3, 0] = 50.                                   # one long displacement at lag 1
    X[2, 2:, 1] = 30.
    X[2, 3, 2] = -70.                                  # two
    X[3] = np.arange(12).reshape(4, 3) * 25.           # nine, all 75
    X[4] = X[3]
    X[4, 1, 1] = np.nan                                # two displacements become NaN
    S = R.summaries(X, 1)
    assert S.shape == (5, 12) and S[:, 0].tolist() == [9, 8, 7, 0, 0]
    assert np.all(np.isposinf(S[0, 1:]))
    assert S[1, 1] == 50 and np.all(S[1, 2:] == -20)
    assert S[2, 1] == 50 and S[2, 2] == np.log(4.) and S[2, -1] == np.log(4.)
    assert S[3, 1] == 75 and np.all(S[3, 2:] == -20) and np.array_equal(S[4], S[3])
    # nan_to_num also moves an infinite median to the largest double
    X[1, 3, 0] = np.inf
    assert R.summaries(X, 1)[1, 1] == np.finfo(float).max


def test_device_draw_layout():
    U, TH, W, Rr = R.philox_draws(3, 9, 5, 4, n_toads=3, n_days=7)
    assert U.shape == TH.shape == W.shape == Rr.shape == (4, 6, 3) and Rr.dtype == np.int32
    assert np.all((U >= 0) & (U < 1)) and np.all(np.abs(TH) <= R.HALF_PI) and np.all(W >= 0)
    assert np.all((Rr >= 0) & (Rr < np.arange(1, 7)[None, :, None])) and np.all(Rr[:, 0] == 0)
    # a row is moved by first_index as by position, and does not depend on the shape around it
    U2, TH2, W2, R2 = R.philox_draws(3, 9, 7, 2, n_toads=5, n_days=9)
    for a, b in ((U, U2), (TH, TH2), (W, W2), (Rr, R2)):
        assert np.array_equal(b[:, :6, :3], a[2:])
    assert not np.array_equal(R.philox_draws(3, 10, 5, 4, n_toads=3, n_days=7)[0], U)
    # the angle and exponential of a cell are the sampler's element e = (g << 32) | (day << 16) | toad
    th, w = R.angle_expo(3, 9, (6 << 32) | (2 << 16) | 1)
    assert th == TH[1, 1, 1] and w == W[1, 1, 1]


@pytest.mark.reference
def test_model_graph_is_the_references():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi_amd
    from elfi.examples import toad
    m, ref = elfi_amd.toad_model(seed_obs=4), toad.get_model(seed_obs=4)
    public = [sorted(k for k in mdl.nodes if not k.startswith('_')) for mdl in (m, ref)]
    assert public[0] == public[1] == sorted(['alpha', 'gamma', 'p0', 'toad', 'S1', 'S2', 'S4', 'S8', 'd'])
    assert m.parameter_names == ref.parameter_names == ['alpha', 'gamma', 'p0']
    for name in ('S1', 'S2', 'S4', 'S8'):
        assert m[name].observed.shape == ref[name].observed.shape == (1, 12)
        assert np.array_equal(m[name].observed, ref[name].observed)
    assert sorted(m.get_parents('d')) == ['S1', 'S2', 'S4', 'S8']
    with pytest.raises(ValueError):
        elfi_amd.toad_model(true_params=[1.7, 35.])


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    t = np.full(4, 0.5)
    D = np.zeros((4, 62, 66))
    Ri = np.zeros((4, 62, 66), dtype=np.int32)
    late = Ri.copy()
    late[2, 0, 5] = 1                                  # day 1 can only return to day 0
    bad = [dict(n_days=1), dict(n_toads=0), dict(n_days=128, n_toads=65), dict(lags=()), dict(lags=(0,)), dict(lags=(63,)),
           dict(lags=(1.5,)), dict(lags=tuple(range(1, 10))), dict(p=[]), dict(p=np.linspace(0, 1, 65)), dict(p=[0., 1.2]),
           dict(p=[-0.1, 0.5]), dict(p=[0.5, 0.5]), dict(p=[0.6, 0.4]), dict(thd=np.nan), dict(first_index=-1),
           dict(first_index=2 ** 32 - 3), dict(draws=(D, D, D)), dict(draws=(D, D, D, Ri[:3])), dict(draws=(D, D, D[:, :61], Ri)),
           dict(draws=(D[0], D[0], D[0], Ri[0])), dict(draws=(D, D, D, late)), dict(draws=(D, D, D, Ri - 1)),
           dict(draws=(D, D, D, Ri + 0.5))]
    for kw in bad:
        with pytest.raises(ValueError):
            elfi_amd.toad_summaries(t, t, t, **kw)
    with pytest.raises(ValueError):
        elfi_amd.toad_summaries(t, t, np.zeros(3))                   # a parameter of another batch size
    for kw in (dict(angle=t), dict(expo=t), dict(angle=t, expo=t[:3]), dict(scale=t[:3])):
        with pytest.raises(ValueError):
            elfi_amd.levy_stable(t, **kw)
    assert elfi_amd.levy_stable(np.zeros((0, 3))).shape == (0, 3)   # nothing to draw: no device either


def test_library_refuses_bad_limits_without_a_device():
    """The C entry points check their arguments before they touch the device: a NULL context is refused, never a crash."""
    import elfi_amd
    lib = elfi_amd.load_library()
    assert lib.elfihip_stable(None, 0, 0, 1, *([None] * 5)) != 0
    assert lib.elfihip_stable_dev(None, 0, 0, 1, *([None] * 5)) != 0
    assert lib.elfihip_toad_summaries(None, *([None] * 4), 0, 0, 0, 1, 66, 63, 1, None, 1, None, 10., *([None] * 10)) != 0
