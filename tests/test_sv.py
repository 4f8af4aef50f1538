"""CPU: the NumPy statement of the alpha-stable stochastic-volatility model (tests/sv_ref.py) reproduces recorded runs of
ELFI's own example on replayed draws (tests/golden/sv.npz, scripts/make_golden_sv.py) bit for bit -- the returns y and the two
summaries, NaN patterns included; its general alpha-stable step lies within its own first-order bound B of a 50-digit
evaluation of the same expression on the same doubles, on the inputs the GPU test of the sampler uses (which makes `within B
of the exact value` a condition the reference itself meets, so that the device may be held to 2 B of it), with at most
MASK_SHARE of the elements masked; and the device functions refuse bad arguments before any device context exists."""
import os

import numpy as np
import pytest

import sv_ref as R

SETS = ['true', 'prior', 'alpha_one', 'alpha_two', 'beta_zero', 'beta_plus', 'beta_minus', 'kappa_zero', 'x0', 'n_1', 'n_2', 'n_65']


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'sv.npz'))


def golden_set(g, name):
    """(params (batch, 7), x_0 or None, (Z, TH, W), y, S) of a recorded set; the draws replayed from the recorded seed."""
    p, y = g[name + '_params'], g[name + '_y']
    draws = R.draws_from_state(np.random.RandomState(int(g[name + '_seed'])), y.shape[1], y.shape[0])
    x_0 = None if np.isnan(p[:, 7]).all() else p[:, 7]
    return p[:, :7], x_0, draws, y, g[name + '_S']


def test_the_recorded_sets_are_the_ones_the_issue_asks_for(golden):
    g = golden
    assert list(g['sets']) == SETS and list(g['order']) == ['alpha', 'beta', 'kappa', 'eta', 'mu', 'phi', 'sigma', 'x_0']
    assert np.all(g['true_params'][0, :7] == [1.2, 0.5, 1, 0, 0, 0.95, 0.2]) and g['true_y'].shape == (1, 50)
    assert g['prior_y'].shape == (8, 50) and g['prior_S'].shape == (8, 2)
    lo, hi = g['prior_params'][:, :2].min(axis=0), g['prior_params'][:, :2].max(axis=0)
    assert np.all(lo >= [0.5, -1]) and np.all(hi <= [2, 1])
    assert np.all(g['alpha_one_params'][0, :2] == [1, 0.5]) and g['alpha_two_params'][0, 0] == 2
    assert g['beta_zero_params'][0, 1] == 0 and g['beta_plus_params'][0, 1] == 1 and g['beta_minus_params'][0, 1] == -1
    assert g['kappa_zero_params'][0, 2] == 0 and np.all(g['kappa_zero_y'] == 0) and np.isnan(g['kappa_zero_S']).all()
    assert np.all(g['x0_params'][:, 7] == 0.7) and all(np.isnan(g[n + '_params'][:, 7]).all() for n in SETS if n != 'x0')
    assert [g[n + '_y'].shape[1] for n in ('n_1', 'n_2', 'n_65')] == [1, 2, 65] and np.isnan(g['n_1_S']).all()
    assert all(np.isfinite(g[n + '_S']).all() for n in SETS if n not in ('kappa_zero', 'n_1'))
    assert g['cdf_p'].shape == (2, 3) and g['cdf_params'].tolist() == [[0.8, 0.5], [1.5, -0.7]]
    # no draws are stored, and the file stays below the toad example's
    assert not any(k.endswith(('_Z', '_TH', '_W')) for k in g.files)
    here = os.path.dirname(os.path.abspath(R.__file__))
    assert os.path.getsize(os.path.join(here, 'golden', 'sv.npz')) <= os.path.getsize(os.path.join(here, 'golden', 'toad.npz'))


@pytest.mark.parametrize('name', SETS)
def test_statement_is_the_recorded_run(golden, name):
    p, x_0, (Z, TH, W), y, S = golden_set(golden, name)
    x, v, B, got = R.simulate(*p.T, Z, TH, W, x_0=x_0)
    assert got.shape == y.shape and np.array_equal(got, y, equal_nan=True)
    Sg = R.summaries(got)
    assert Sg.shape == S.shape == (len(p), 2) and np.array_equal(Sg, S, equal_nan=True)
    with np.errstate(all='ignore'):
        assert np.array_equal(Sg, np.column_stack([_np_kurt(y), _np_skew(y)]), equal_nan=True)


def _np_kurt(y):
    qs = np.quantile(y, q=[0.05, 0.25, 0.75, 0.95], axis=1)
    return (qs[3] - qs[0]) / (qs[2] - qs[1])


def _np_skew(y):
    qs = np.quantile(y, q=[0.05, 0.50, 0.95], axis=1)
    return ((qs[2] - qs[1]) - (qs[1] - qs[0])) / (qs[2] - qs[0])


def test_summaries_are_numpys_quantiles_with_nan_and_inf():
    rs = np.random.RandomState(3)
    with np.errstate(all='ignore'):
        for n_obs in (1, 2, 3, 7, 50, 65, 257):
            y = rs.standard_cauchy((6, n_obs))
            if n_obs >= 3:
                y[1, 1] = np.nan
                y[2, 0], y[3, 2], y[4, :2] = np.inf, -np.inf, (np.inf, -np.inf)
                y[5, :] = 0.0
                y[5, ::2] = -0.0
            assert np.array_equal(R.summaries(y), np.column_stack([_np_kurt(y), _np_skew(y)]), equal_nan=True), n_obs
        q = (0.0, 0.3, 0.31, 1.0), (0.1, 0.2, 0.9)
        y = rs.standard_cauchy((4, 33))
        k, s = np.quantile(y, q[0], axis=1), np.quantile(y, q[1], axis=1)
        want = np.column_stack([(k[3] - k[0]) / (k[2] - k[1]), ((s[2] - s[1]) - (s[1] - s[0])) / (s[2] - s[0])])
        assert np.array_equal(R.summaries(y, *q), want)


def test_general_step_is_scipys_rvs():
    """The statement against SciPy itself, where SciPy is installed: the same RandomState, both parameterisations."""
    ss = pytest.importorskip('scipy.stats')
    n = 4000
    prs = np.random.RandomState(1)
    alpha, beta = prs.uniform(0.3, 2, n), prs.uniform(-1, 1, n)
    loc, scale = prs.uniform(-5, 5, n), prs.uniform(0, 10, n)
    alpha[:600], alpha[600:900] = 1, 2
    beta[300:700], beta[700:800], beta[800:900], beta[100:150] = 0, 1, -1, 1
    scale[::50] = 0
    for par in ('S1', 'S0'):
        d = ss.levy_stable(alpha, beta, loc=loc, scale=scale)
        d.dist.parameterization = par
        try:
            d.random_state = np.random.RandomState(5)
            with np.errstate(all='ignore'):
                x = d.rvs(size=n)
        finally:
            d.dist.parameterization = 'S1'
        rs = np.random.RandomState(5)
        TH, W = rs.uniform(size=n) * R.PI + (-R.HALF_PI), rs.standard_exponential(n)
        got, B = R.stable_general_step(alpha, beta, loc, scale, TH, W, par)
        assert np.array_equal(got, x, equal_nan=True), par
        # scale == 0 at alpha == 1 is 0 log 0, for every beta
        assert np.array_equal(np.isnan(x), (alpha == 1) & (scale == 0))


def exact_general(alpha, beta, loc, scale, TH, W, s0=True):
    """The expression of stable_general_step on the same doubles in 50-digit arithmetic."""
    import mpmath as mp
    mp.mp.dps = 50
    al, be, lo, sc, th, w = (mp.mpf(float(v)) for v in (alpha, beta, loc, scale, TH, W))
    pi, hp, tbp = mp.mpf(R.PI), mp.mpf(R.HALF_PI), mp.mpf(R.TWO_BY_PI)
    if al == 1:
        s = hp + be * th
        z = tbp * (s * mp.tan(th) - be * mp.log((hp * w * mp.cos(th)) / s))
    elif be == 0:
        ath = al * th
        z = w / (mp.cos(th) / mp.tan(ath) + mp.sin(th)) * ((mp.cos(ath) + mp.sin(ath) * mp.tan(th)) / w) ** (1 / al)
    else:
        val0 = be * mp.tan(pi * al / 2)
        th0 = mp.atan(val0) / al
        ath = al * th
        val3 = w / (mp.cos(th) / mp.tan(al * (th0 + th)) + mp.sin(th))
        z = val3 * ((mp.cos(ath) + mp.sin(ath) * mp.tan(th) - val0 * (mp.sin(ath) - mp.cos(ath) * mp.tan(th))) / w) ** (1 / al)
    x = z * sc + lo
    if al == 1:
        x = x + 2 * be * sc * mp.log(sc) / pi
        if s0:
            x = x - be * 2 * sc * mp.log(sc) / pi
    elif s0:
        x = x - sc * be * mp.tan(pi * al / 2)
    return x


def test_numpy_step_is_within_its_bound_of_the_exact_value():
    import mpmath as mp
    alpha, beta, loc, scale, TH, W = R.general_inputs()
    assert alpha.shape == (30000,)
    x, B = R.stable_general_step(alpha, beta, loc, scale, TH, W, 'S0')
    ok = R.stable_valid(alpha, beta, scale)
    valid = ~np.isnan(x)
    # NaN where a parameter is invalid, and at scale == 0 with alpha == 1 (SciPy's 0 log 0)
    assert np.array_equal(~valid, ~ok | ((alpha == 1) & (scale == 0))) and np.all(B[~valid] == 0) and 500 < (~ok).sum() < 1000
    compared = R.step_mask(x, B)
    assert not compared[~valid].any()
    share = (valid & ~compared).mean()
    print('masked share', share)
    assert share <= R.MASK_SHARE
    # the S1 value of the same inputs is masked no more often
    x1, B1 = R.stable_general_step(alpha, beta, loc, scale, TH, W, 'S1')
    assert (~np.isnan(x1) & ~R.step_mask(x1, B1)).mean() <= share
    c = compared
    assert (alpha[c] == 1).sum() >= 1500 and (alpha[c] == 2).sum() >= 1500 and (beta[c] == 0).sum() >= 1500
    assert (beta[c] == 1).sum() >= 500 and (beta[c] == -1).sum() >= 500
    assert ((alpha[c] == 1) & (np.abs(beta[c]) == 1)).sum() >= 500 and ((alpha[c] == 1) & (beta[c] == 0)).sum() >= 500
    assert (R.HALF_PI - np.abs(TH[c]) < 1e-10).sum() > 500
    near = np.abs(alpha[c] - 1)
    assert ((near > 0) & (near < 1e-3)).sum() >= 500 and near[near > 0].min() < 1e-4
    worst = 0.0
    for i in np.flatnonzero(compared):
        err = abs(mp.mpf(float(x[i])) - exact_general(alpha[i], beta[i], loc[i], scale[i], TH[i], W[i]))
        if B[i] == 0:
            assert err == 0
            continue
        worst = max(worst, float(err / mp.mpf(float(B[i]))))
    print('worst |numpy - exact| / B', worst)
    assert worst <= 1.0
    # S1 on a part of the set (the same expression without the last shift)
    for i in np.flatnonzero(R.step_mask(x1, B1))[::10]:
        err = abs(mp.mpf(float(x1[i])) - exact_general(alpha[i], beta[i], loc[i], scale[i], TH[i], W[i], s0=False))
        assert err <= mp.mpf(float(B1[i]))


def test_log_vol_and_returns():
    rs = np.random.RandomState(2)
    Z = rs.standard_normal((3, 5))
    mu, phi, sigma = np.array([0.0, -0.3, 1.0]), np.array([0.95, 0.9999999, -0.5]), np.array([0.2, 0.0, 1.5])
    x = R.log_vol(mu, phi, sigma, Z)
    assert np.array_equal(x[:, 0], Z[:, 0] * (sigma / np.sqrt(1 - np.minimum(phi ** 2, 0.99999))) + mu)
    assert np.array_equal(x[:, 3], Z[:, 3] * sigma + (mu + phi * (x[:, 2] - mu))) and np.all(x[1] == -0.3)
    x = R.log_vol(mu, phi, sigma, Z, x_0=0.7)
    assert np.array_equal(x[:, 0], Z[:, 0] * sigma + (mu + phi * (0.7 - mu)))
    assert np.array_equal(R.returns(x, 2 * x), np.exp(0.5 * x) * (2 * x))
    ok = R.valid_rows([1.2, 0.0, 1.2, 1.2, 1.2, 1.2], [0.5, 0.5, 1.5, 0.5, 0.5, 0.5], [1, 1, 1, -1, 1, 1], 0, [0, 0, 0, 0, np.nan, 0],
                      0.95, [0.2, 0.2, 0.2, 0.2, 0.2, -0.2])
    assert ok.tolist() == [True, False, False, False, False, False]


def test_device_draw_layout():
    Z, TH, W = R.philox_draws(3, 9, 5, 4, n_obs=7)
    assert Z.shape == TH.shape == W.shape == (4, 7)
    assert np.all(np.abs(TH) <= R.HALF_PI) and np.all(W >= 0) and np.all(np.isfinite(Z))
    # a row is moved by first_index as by position, and does not depend on the shape around it
    for a, b in zip((Z, TH, W), R.philox_draws(3, 9, 7, 2, n_obs=9)):
        assert np.array_equal(b[:, :7], a[2:])
    assert not np.array_equal(R.philox_draws(3, 10, 5, 4, n_obs=7)[0], Z)
    # the angle and exponential of a cell are the sampler's element e = (g << 32) | t; the normal comes from the next stream
    import toad_ref
    th, w = toad_ref.angle_expo(3, 9, (6 << 32) | 2)
    assert th == TH[1, 2] and w == W[1, 2] and R.normal_first(3, 10, (6 << 32) | 2) == Z[1, 2]
    # the normals are standard: 4 sigma on mean and variance of 40 000
    z = R.philox_draws(1, 0, 0, 800, n_obs=50)[0].ravel()
    assert abs(z.mean()) <= 4 / np.sqrt(z.size) and abs(z.var() - 1) <= 4 * np.sqrt(2.0 / z.size)


@pytest.mark.reference
def test_model_graph_is_the_references():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi_amd
    from elfi.examples import stochastic_volatility_model as svm
    m, ref = elfi_amd.sv_model(n_obs=20, seed_obs=4), svm.get_model(n_obs=20, seed_obs=4)
    public = [sorted(k for k in mdl.nodes if not k.startswith('_')) for mdl in (m, ref)]
    names = ['alpha', 'beta', 'kappa', 'eta', 'mu', 'phi', 'sigma', 'a_svm', 'kurt', 'skew', 'd']
    assert public[1] == sorted(names) and public[0] == sorted(names + ['returns'])
    assert m.parameter_names == ref.parameter_names == ['alpha', 'beta']
    assert np.array_equal(m['returns'].observed, ref['a_svm'].observed) and m['returns'].observed.shape == (1, 20)
    for name in ('kurt', 'skew'):
        assert np.array_equal(np.ravel(m[name].observed), np.ravel(ref[name].observed))
    assert sorted(m.get_parents('d')) == ['kurt', 'skew']
    with pytest.raises(ValueError):
        elfi_amd.sv_model(true_params=[1.2])


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    t = np.full(4, 0.5)
    D = np.zeros((4, 50))
    bad = [dict(n_obs=0), dict(n_obs=4097), dict(q_kurt=(.05, .25, .75)), dict(q_skew=(.05, .5, .95, .99)), dict(q_kurt=(.05, .25, .75, 1.2)),
           dict(q_skew=(-.1, .5, .95)), dict(first_index=-1), dict(first_index=2 ** 32 - 3), dict(draws=(D, D)), dict(draws=(D, D, D[:3])),
           dict(draws=(D, D, D[:, :49])), dict(draws=(D[0], D[0], D[0])), dict(kappa=np.zeros(3)), dict(x_0=np.zeros(3))]
    for kw in bad:
        with pytest.raises(ValueError):
            elfi_amd.sv_summaries(t, t, **kw)
    for kw in (dict(angle=t), dict(expo=t), dict(angle=t, expo=t[:3]), dict(scale=t[:3]), dict(loc=t[:3]), dict(parameterization='S2')):
        with pytest.raises(ValueError):
            elfi_amd.levy_stable_general(t, t, **kw)
    with pytest.raises(ValueError):
        elfi_amd.levy_stable_general(t, t[:3])
    assert elfi_amd.levy_stable_general(np.zeros((0, 3)), 0.5).shape == (0, 3)   # nothing to draw: no device either


def test_library_refuses_bad_limits_without_a_device():
    """The C entry points check their arguments before they touch the device: a NULL context is refused, never a crash."""
    import elfi_amd
    lib = elfi_amd.load_library()
    assert lib.elfihip_stable_general(None, 0, 0, 1, 0, *([None] * 7)) != 0
    assert lib.elfihip_stable_general_dev(None, 0, 0, 1, 0, *([None] * 7)) != 0
    assert lib.elfihip_sv_summaries(None, *([None] * 3), 0, 0, 0, 1, 50, *([None] * 16)) != 0
    assert lib.elfihip_sv_summaries_dev(None, *([None] * 3), 50, 0, 0, 0, 1, 50, *([None] * 10), 2, None, 50, None, 50, None, 50,
                                        None, None, None, 50) != 0
