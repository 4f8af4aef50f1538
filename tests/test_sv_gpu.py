"""GPU: the general stable-law sampler (csrc/stable.hpp: stable_general) and the fused stochastic-volatility model
(csrc/sv.hip) against their NumPy statement (tests/sv_ref.py), which tests/test_sv.py holds to recorded runs of ELFI's own
example, to SciPy and to 50-digit arithmetic.

The sampler evaluates SciPy's expression in SciPy's order, so it differs from NumPy on the same angle and exponential only
through tan, sin, cos, atan, log and pow: each side within the first-order bound B of the exact value (4 ulp per
transcendental call, half an ulp per operation; sv_ref.stable_general_step makes B beside the value), hence within 2 B of each
other; elements whose B exceeds 2^-20 of |x| are masked, at most 10^-3 of them.  On given normals the log-volatilities are
NumPy's bit for bit; a return y = exp(x / 2) v is within exp(x / 2) B + (4 + 1/2) ulp of the exact value on either side; on
the device's own returns the two summaries are NumPy's bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import sv_ref as R
from device_layout import SENTINEL, guarded_out, to_device
from test_sv import SETS, golden_set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'sv.npz'))


@pytest.fixture(scope='module')
def inputs():
    """The fixed 30 000-element input set and its NumPy values and bounds, made once."""
    args = R.general_inputs()
    return args, {par: R.stable_general_step(*args, par) for par in ('S0', 'S1')}


def check_steps(got, ref, B, what=''):
    """|device - NumPy| <= 2 B on the compared elements, equal NaN patterns, at most MASK_SHARE masked -> worst distance in ulp."""
    compared = R.step_mask(ref, B)
    valid = ~np.isnan(ref)
    assert (valid & ~compared).mean() <= R.MASK_SHARE, what
    assert np.array_equal(np.isnan(got[compared | ~valid]), np.isnan(ref[compared | ~valid])), what
    err = np.abs(got[compared] - ref[compared])
    ulps = R.ulp_distance(got[compared], ref[compared])
    worst = float(ulps.max()) if ulps.size else 0.0
    print('%s: %d compared, worst |device - NumPy| %.1f ulp, worst / 2B %.3f'
          % (what, compared.sum(), worst, float(np.max(err / np.maximum(2 * B[compared], 1e-300))) if err.size else 0.0))
    assert np.all(err <= 2 * B[compared]), what
    return worst


def col(p, shape):
    return np.broadcast_to(np.asarray(p, dtype=np.float64).reshape(-1, 1), shape)


# ---- 1. the sampler on given angles and exponentials ---------------------------------------------------------------------
@pytest.mark.parametrize('par', ['S0', 'S1'])
def test_sampler_on_given_angles_is_scipys_expression(hip_ctx, inputs, par):
    import elfi_amd
    (alpha, beta, loc, scale, TH, W), refs = inputs
    ref, B = refs[par]
    got = elfi_amd.levy_stable_general(alpha, beta, loc, scale, par, angle=TH, expo=W)
    assert got.shape == alpha.shape
    check_steps(got, ref, B, 'sampler ' + par)
    # the shape of alpha is kept; scalars broadcast
    g2 = elfi_amd.levy_stable_general(alpha[:12].reshape(3, 4), 0.5, -1.0, 2.0, par, angle=TH[:12].reshape(3, 4), expo=W[:12].reshape(3, 4))
    want = elfi_amd.levy_stable_general(alpha[:12], np.full(12, 0.5), np.full(12, -1.0), np.full(12, 2.0), par, angle=TH[:12], expo=W[:12])
    assert g2.shape == (3, 4) and np.array_equal(g2.ravel(), want)


def test_sampler_dev_form_writes_n_elements(hip_ctx, inputs):
    import torch
    import elfi_amd
    args = [a[20000:22077] for a in inputs[0]]
    n = len(args[0]) - 5
    want = elfi_amd.levy_stable_general(*[a[:n] for a in args[:4]], 'S0', angle=args[4][:n], expo=args[5][:n])
    d = [to_device(a) for a in args]
    torch.cuda.synchronize()
    out = guarded_out(n, 1, 1)
    hip_ctx.call('elfihip_stable_general_dev', C.c_uint64(0), C.c_uint64(0), n, 1, *[t.data_ptr() for t in d], out.ptr)
    hip_ctx.synchronize()
    assert np.array_equal(out.check(), want, equal_nan=True)
    out = guarded_out(n, 1, 0)
    hip_ctx.call('elfihip_stable_general_dev', C.c_uint64(5), C.c_uint64(2), n, 0, *[t.data_ptr() for t in d[:4]], None, None, out.ptr)
    hip_ctx.synchronize()
    assert np.array_equal(out.check(), elfi_amd.levy_stable_general(*[a[:n] for a in args[:4]], 'S1', seed=5, stream=2), equal_nan=True)


# ---- 2. the sampler's own draws ---------------------------------------------------------------------------------------------
def test_sampler_draws_are_the_symmetric_samplers_at_beta_zero(hip_ctx):
    import elfi_amd
    rs = np.random.RandomState(4)
    alpha = rs.uniform(0.3, 2.0, 3000)
    alpha[:300], alpha[300:600] = 1.0, 2.0
    scale = rs.uniform(0.1, 50, 3000)
    x = elfi_amd.levy_stable_general(alpha, 0.0, 0.0, scale, 'S1', seed=11, stream=4)
    assert np.array_equal(x, elfi_amd.levy_stable(alpha, scale, seed=11, stream=4)) and not np.isnan(x).any()
    assert np.array_equal(elfi_amd.levy_stable_general(alpha.reshape(30, 100), 0.0, seed=11, stream=4).ravel(),
                          elfi_amd.levy_stable(alpha, 1.0, seed=11, stream=4))


def test_sampler_draws_are_counter_based(hip_ctx):
    import toad_ref
    import elfi_amd
    a, b = np.full(1000, 1.5), np.full(1000, -0.7)
    kw = dict(loc=0.3, scale=3.0, parameterization='S0')
    x = elfi_amd.levy_stable_general(a, b, seed=11, stream=4, **kw)
    assert np.array_equal(elfi_amd.levy_stable_general(a[:10], b[:10], seed=11, stream=4, **kw), x[:10])
    assert np.array_equal(elfi_amd.levy_stable_general(a[:257], b[:257], seed=11, stream=4, **kw), x[:257])
    assert not np.any(elfi_amd.levy_stable_general(a, b, seed=11, stream=5, **kw) == x)
    assert not np.any(elfi_amd.levy_stable_general(a, b, seed=12, stream=4, **kw) == x)
    # element e is the transform of the angle and exponential of Philox counter e; the exponential goes through the device's
    # log (4 ulp), and Z varies as W^(1 - 1 / alpha), |1 - 1 / alpha| = 1 / 3 here: at most 4 EPS |Z scale| more, to first order
    TH, W = toad_ref.angle_expo(11, 4, np.arange(1000))
    ref, B = R.stable_general_step(a, b, 0.3, 3.0, TH, W, 'S0')
    zs = np.abs(ref - 0.3) + np.abs(3.0 * -0.7 * np.tan(R.PI * 1.5 / 2))          # |Z scale| <= |x - loc| + |shift|
    ok = R.step_mask(ref, B)
    assert (~ok).mean() <= R.MASK_SHARE and np.all(np.abs(x[ok] - ref[ok]) <= 2 * B[ok] + 4 * R.EPS * zs[ok])


def test_sampler_distribution(hip_ctx, golden):
    import elfi_amd
    n = 100000
    for (a, b), probs in zip(golden['cdf_params'], golden['cdf_p']):
        x = elfi_amd.levy_stable_general(np.full(n, a), b, 0.0, 1.0, 'S0', seed=23)
        for point, q in zip(golden['cdf_x'], probs):
            z = ((x < point).mean() - q) / np.sqrt(q * (1 - q) / n)
            print('alpha = %.1f, beta = %.1f: z(share below %.1f) %.2f' % (a, b, point, z))
            assert abs(z) <= 4
    # alpha = 2 is normal with variance 2 scale^2 around loc, whatever beta
    x = elfi_amd.levy_stable_general(np.full(n, 2.0), 0.8, 1.0, 1.5, 'S0', seed=21)
    z_mean = (x.mean() - 1.0) / np.sqrt(4.5 / n)
    z_var = (x.var() - 4.5) / (4.5 * np.sqrt(2.0 / n))
    print('alpha = 2: z(mean) %.2f, z(variance) %.2f' % (z_mean, z_var))
    assert abs(z_mean) <= 4 and abs(z_var) <= 4


# ---- 3. the model on the recorded draws ------------------------------------------------------------------------------------
def check_model(p, x_0, draws, S, y, x, v, what):
    """x bit-equal to the statement's chain; v within 2 B; y within twice (exp(x / 2) B + (4 + 1/2) EPS |y|); S bit-equal to the
    statement's summaries of the device's own y."""
    xr, vr, B, yr = R.simulate(*p.T, *draws, x_0=x_0)
    assert np.array_equal(x, xr, equal_nan=True), what
    worst = check_steps(v, vr, B, what + ' shocks')
    with np.errstate(all='ignore'):
        ok = R.step_mask(vr, B) & np.isfinite(yr)
        By = np.exp(0.5 * xr) * B + (R.TRANSCENDENTAL_ULP + 0.5) * R.EPS * np.abs(yr)
        err = np.abs(y - yr)
    print('%s returns: worst / 2By %.3f' % (what, float(np.max(err[ok] / np.maximum(2 * By[ok], 1e-300))) if ok.any() else 0.0))
    assert np.array_equal(np.isnan(y), np.isnan(yr)) and np.array_equal(y[np.isinf(yr)], yr[np.isinf(yr)]), what
    assert np.all(err[ok] <= 2 * By[ok]), what
    assert np.array_equal(S, R.summaries(y), equal_nan=True), what
    return worst


@pytest.mark.parametrize('name', SETS)
def test_model_on_golden_draws(hip_ctx, golden, name):
    import elfi_amd
    p, x_0, draws, yg, Sg = golden_set(golden, name)
    S, y, x, v = elfi_amd.sv_summaries(*p.T, n_obs=yg.shape[1], x_0=x_0, draws=draws, return_logvol=True, return_shocks=True)
    assert S.shape == Sg.shape and y.shape == x.shape == v.shape == yg.shape
    check_model(p, x_0, draws, S, y, x, v, name)
    if name in ('kappa_zero', 'n_1'):
        assert np.isnan(S).all()                       # 0 / 0
    if np.array_equal(y, yg):
        assert np.array_equal(S, Sg, equal_nan=True)


def test_summaries_with_nan_inf_and_other_quantiles(hip_ctx):
    import elfi_amd
    # eta steers single returns: exp(x / 2) v with kappa = 0 is exp(x / 2) eta -- inf, -inf and NaN rows, and all equal rows
    n_obs = 21
    rs = np.random.RandomState(8)
    Z, TH, W = rs.standard_normal((6, n_obs)), rs.uniform(-1.5, 1.5, (6, n_obs)), rs.standard_exponential((6, n_obs))
    eta = np.array([1.0, np.inf, -np.inf, 0.0, -2.0, 1e308])
    mu = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 3.0])
    S, y = elfi_amd.sv_summaries(1.5, 0.5, 0.0, eta, mu, 0.95, 0.2, n_obs=n_obs, draws=(Z, TH, W))
    assert np.all(y[1] == np.inf) and np.all(y[2] == -np.inf) and np.all(y[3] == 0) and np.isinf(y[5]).any()
    assert np.array_equal(S, R.summaries(y), equal_nan=True) and np.isnan(S[1:4]).all() and np.isfinite(S[[0, 4]]).all()
    # a NaN draw makes that row's summaries NaN and no other's
    TH2 = TH.copy()
    TH2[4, 7] = np.nan
    S2, y2 = elfi_amd.sv_summaries(1.5, 0.5, 1.0, 0.0, mu, 0.95, 0.2, n_obs=n_obs, draws=(Z, TH2, W))
    assert np.isnan(y2[4, 7]) and np.isnan(y2).sum() == 1 and np.isnan(S2[4]).all() and np.isfinite(S2[:4]).all()
    assert np.array_equal(S2, R.summaries(y2), equal_nan=True)
    for q in (((0.0, 0.3, 0.31, 1.0), (0.1, 0.2, 0.9)), ((0.5, 0.5, 0.5, 0.5), (0.0, 0.5, 1.0))):
        S3, y3 = elfi_amd.sv_summaries(1.5, 0.5, 1.0, 0.0, mu, 0.95, 0.2, n_obs=n_obs, draws=(Z, TH, W), q_kurt=q[0], q_skew=q[1])
        assert np.array_equal(S3, R.summaries(y3, *q), equal_nan=True)


# ---- 4. the model on its own draws ------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 3), (3, 1), (50, 130), (63, 2), (64, 2), (65, 3), (1024, 2), (1025, 2), (4096, 1)]


@pytest.mark.parametrize('n_obs,n', SHAPES)
def test_model_on_its_own_draws(hip_ctx, n_obs, n):
    import elfi_amd
    rs = np.random.RandomState(n_obs * 10 + n)
    alpha, beta = rs.uniform(0.5, 2, n), rs.uniform(-1, 1, n)
    rest = [rs.uniform(0.5, 2, n), rs.uniform(-1, 1, n), rs.uniform(-1, 1, n), rs.uniform(-0.99, 0.99, n), rs.uniform(0, 0.5, n)]
    p = np.column_stack([alpha, beta] + rest)
    kw = dict(n_obs=n_obs)
    S, y, x, v, draws = elfi_amd.sv_summaries(*p.T, seed=31, stream=6, first_index=5, return_logvol=True, return_shocks=True,
                                              return_draws=True, **kw)
    Z, TH, W = R.philox_draws(31, 6, 5, n, n_obs)
    assert np.array_equal(draws[1], TH) and R.ulp_distance(draws[2], W).max() <= 4 and R.ulp_distance(draws[0], Z).max() <= 4
    # the shock of a cell is the sampler's transform of the cell's angle and exponential, in S0 with loc = eta, scale = kappa
    shape = TH.shape
    assert np.array_equal(v, elfi_amd.levy_stable_general(col(alpha, shape), col(beta, shape), col(p[:, 3], shape), col(p[:, 2], shape),
                                                          'S0', angle=draws[1], expo=draws[2]), equal_nan=True)
    check_model(p, None, draws, S, y, x, v, '%d x %d' % (n_obs, n))
    # replaying the returned draws gives the same numbers; the optional outputs do not change S
    S2, y2, x2, v2 = elfi_amd.sv_summaries(*p.T, draws=draws, return_logvol=True, return_shocks=True, **kw)
    assert np.array_equal(S2, S, equal_nan=True) and np.array_equal(y2, y) and np.array_equal(x2, x) and np.array_equal(v2, v)
    assert np.array_equal(elfi_amd.sv_summaries(*p.T, seed=31, stream=6, first_index=5, return_series=False, **kw), S, equal_nan=True)
    # a row does not depend on the batch: it is moved by first_index exactly as by position
    k = n // 2
    S3, y3 = elfi_amd.sv_summaries(*p[k:].T, seed=31, stream=6, first_index=5 + k, **kw)
    assert np.array_equal(S3, S[k:], equal_nan=True) and np.array_equal(y3, y[k:])
    # with x_0 only the start of the chain changes
    S4, y4, x4 = elfi_amd.sv_summaries(*p.T, x_0=0.4, draws=draws, return_logvol=True, **kw)
    assert np.array_equal(x4, R.log_vol(p[:, 4], p[:, 5], p[:, 6], draws[0], x_0=0.4)) and np.array_equal(S4, R.summaries(y4), equal_nan=True)


def test_invalid_rows_are_nan_and_alone(hip_ctx):
    import elfi_amd
    good = [1.5, 0.5, 1.0, 0.0, 0.0, 0.95, 0.2]
    p = np.tile(good, (16, 1))
    bad = np.zeros(16, dtype=bool)
    for row, (c, value) in zip(range(1, 16, 2) , [(0, 0.0), (0, 2.5), (0, np.nan), (1, -1.5), (2, -1.0), (6, -0.1), (4, np.nan), (5, np.nan)]):
        p[row, c] = value
        bad[row] = True
    S, y, x, v = elfi_amd.sv_summaries(*p.T, n_obs=12, seed=3, return_logvol=True, return_shocks=True)
    for a in (S, y, x, v):
        assert np.all(np.isnan(a[bad])) and not np.isnan(a[~bad]).any()
    for row in np.flatnonzero(~bad)[:3]:
        assert np.array_equal(elfi_amd.sv_summaries(*p[row], n_obs=12, seed=3, first_index=row, return_series=False), S[row:row + 1])
    # a NaN x_0 is a NaN parameter
    x_0 = np.zeros(16)
    x_0[2] = np.nan
    S2 = elfi_amd.sv_summaries(*p.T, n_obs=12, x_0=x_0, seed=3, return_series=False)
    assert np.array_equal(np.isnan(S2[:, 0]), bad | np.isnan(x_0))


def test_dev_form_at_a_callers_pitch(hip_ctx):
    import torch
    import elfi_amd
    n, n_obs = 5, 37
    rs = np.random.RandomState(9)
    p = np.column_stack([rs.uniform(0.5, 2, n), rs.uniform(-1, 1, n), rs.uniform(0.5, 2, n), rs.uniform(-1, 1, n), rs.uniform(-1, 1, n),
                         rs.uniform(-0.9, 0.9, n), rs.uniform(0, 0.5, n)])
    x_0 = rs.uniform(-1, 1, n)
    S, y, x, v, draws = elfi_amd.sv_summaries(*p.T, n_obs=n_obs, x_0=x_0, seed=8, return_logvol=True, return_shocks=True, return_draws=True)
    q = np.array(R.Q_KURT + R.Q_SKEW)
    guard = np.float64(SENTINEL).view(np.int64)

    def rows_of(t, pitch, width, lead):
        h = t.cpu().numpy()
        body = h[lead:lead + n * pitch].reshape(n, pitch)
        outside = np.concatenate([h[:lead], body[:, width:].ravel(), h[lead + n * pitch:]])
        assert np.all(outside.view(np.int64) == guard), 'a store outside the rows'
        return body[:, :width].copy()

    def buf(pitch, lead):
        return torch.full((lead + n * pitch + 8,), SENTINEL, dtype=torch.float64, device='cuda')

    dpar = [to_device(a) for a in list(p.T) + [x_0]]
    for given in (False, True):
        pitches = dict(S=5, Y=n_obs + 1, X=n_obs + 3, V=n_obs + 2, echo=n_obs + 1, draws=n_obs + 5)
        tS, tY, tX, tV = buf(pitches['S'], 1), buf(pitches['Y'], 3), buf(pitches['X'], 2), buf(pitches['V'], 1)
        tE = [buf(pitches['echo'], 1) for _ in range(3)]
        din, in_ptrs = [], [None] * 3
        if given:
            for a in draws:
                host = np.full((n, pitches['draws']), np.nan)
                host[:, :n_obs] = a
                din.append(torch.from_numpy(host).cuda())
            in_ptrs = [t.data_ptr() for t in din]
        torch.cuda.synchronize()
        hip_ctx.call('elfihip_sv_summaries_dev', *in_ptrs, pitches['draws'], C.c_uint64(8), C.c_uint64(0), 0, n, n_obs, q.ctypes.data,
                     *[t.data_ptr() for t in dpar], tS.data_ptr() + 8, pitches['S'], tY.data_ptr() + 24, pitches['Y'],
                     tX.data_ptr() + 16, pitches['X'], tV.data_ptr() + 8, pitches['V'], tE[0].data_ptr() + 8, tE[1].data_ptr() + 8,
                     tE[2].data_ptr() + 8, pitches['echo'])
        hip_ctx.synchronize()
        assert np.array_equal(rows_of(tS, pitches['S'], 2, 1), S)
        assert np.array_equal(rows_of(tY, pitches['Y'], n_obs, 3), y)
        assert np.array_equal(rows_of(tX, pitches['X'], n_obs, 2), x)
        assert np.array_equal(rows_of(tV, pitches['V'], n_obs, 1), v)
        for t, a in zip(tE, draws):
            assert np.array_equal(rows_of(t, pitches['echo'], n_obs, 1), a)


# ---- 5. through ELFI --------------------------------------------------------------------------------------------------------
def _reference():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi
    return elfi


def test_sv_model_through_elfi(hip_ctx):
    _reference()
    import elfi_amd
    m = elfi_amd.sv_model(n_obs=20, seed_obs=4)
    names = ['alpha', 'beta', 'kappa', 'eta', 'mu', 'phi', 'sigma', 'a_svm', 'kurt', 'skew', 'returns', 'd']
    assert all(name in m.nodes for name in names) and m.parameter_names == ['alpha', 'beta']
    out = m.generate(5, outputs=['alpha', 'beta', 'a_svm', 'kurt', 'skew', 'returns', 'd'], seed=2)
    assert out['a_svm'].shape == (5, 22) and out['d'].shape == (5,) and out['alpha'].shape == (5,)
    assert out['returns'].shape == (5, 20) and out['kurt'].shape == (5,) and out['skew'].shape == (5,)
    assert np.array_equal(out['returns'], out['a_svm'][:, :20]) and np.array_equal(out['kurt'], out['a_svm'][:, 20]) and \
        np.array_equal(out['skew'], out['a_svm'][:, 21])
    assert np.array_equal(out['a_svm'][:, 20:], R.summaries(out['returns']))
    assert np.all((out['alpha'] >= 0.5) & (out['alpha'] <= 2) & (out['beta'] >= -1) & (out['beta'] <= 1))
    bsl = elfi_amd.HipBSL(elfi_amd.sv_model(n_obs=20, seed_obs=4), n_sim_round=100, feature_names=['returns'],
                          likelihood=elfi_amd.semiparametric_likelihood(), seed=1)
    res = bsl.sample(20, sigma_proposals=np.diag([1e-3, 1e-3]), params0=[1.2, 0.5], bar=False)
    assert type(res).__name__ == 'BslSample' and np.all(np.isfinite(bsl.state['logposterior']))
    moves = np.count_nonzero(np.any(np.diff(bsl.state['params'], axis=0) != 0, axis=1))
    print('semiBSL on the stochastic-volatility model: %d accepted moves of 19' % moves)
    assert moves >= 1
