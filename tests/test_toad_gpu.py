"""GPU: the stable-law sampler (csrc/stable.hpp) and the fused toad model (csrc/toad.hip) against their NumPy statement
(tests/toad_ref.py), which tests/test_toad.py holds to recorded runs of ELFI's own example and to 50-digit arithmetic.

The sampler evaluates SciPy's expression in SciPy's order, so it differs from NumPy on the same angle and exponential only
through tan, sin, cos and pow: each side within the first-order bound B of the exact value (4 ulp per transcendental call, half
an ulp per operation; toad_ref.stable_step makes B beside the value), hence within 2 B of each other; elements whose B exceeds
2^-20 of |x| are masked, at most 10^-3 of them.  On the device's own steps the positions are NumPy's bit for bit, on the
positions the counts and medians are; the log differences are within 4 ulp, inf and -20 entries exact."""
import ctypes as C
import os

import numpy as np
import pytest

import toad_ref as R
from device_layout import SENTINEL, guarded_out, to_device
from test_toad import LAGS, SETS, golden_set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'toad.npz'))


def check_steps(dx, ref, B, what=''):
    """|device - NumPy| <= 2 B on the compared elements, equal NaN patterns, at most MASK_SHARE masked -> worst distance in ulp."""
    compared = R.step_mask(ref, B)
    valid = ~np.isnan(ref)
    assert (valid & ~compared).mean() <= R.MASK_SHARE, what
    assert np.array_equal(np.isnan(dx[compared | ~valid]), np.isnan(ref[compared | ~valid])), what
    err = np.abs(dx[compared] - ref[compared])
    ulps = R.ulp_distance(dx[compared], ref[compared])
    worst = float(ulps.max()) if ulps.size else 0.0
    print('%s steps: %d compared, worst |device - NumPy| %.1f ulp, worst / 2B %.3f'
          % (what, compared.sum(), worst, float(np.max(err / np.maximum(2 * B[compared], 1e-300))) if err.size else 0.0))
    assert np.all(err <= 2 * B[compared]), what
    return worst


def check_summaries(S, ref, what=''):
    """Counts and medians (the first two columns of every lag) bit-equal; log differences within 4 ulp, inf and -20 exact."""
    assert S.shape == ref.shape, what
    w = S.shape[1] // 12 if S.shape[1] % 12 == 0 else 1
    S3, r3 = S.reshape(S.shape[0], w, -1), ref.reshape(S.shape[0], w, -1)
    assert np.array_equal(S3[:, :, :2], r3[:, :, :2], equal_nan=True), what
    a, b = S3[:, :, 2:], r3[:, :, 2:]
    special = np.isinf(b) | (b == -20) | np.isnan(b)
    assert np.array_equal(a[special], b[special], equal_nan=True), what
    assert np.array_equal(np.isinf(a) | (a == -20) | np.isnan(a), special), what
    ulps = R.ulp_distance(a[~special], b[~special])
    if ulps.size:
        assert ulps.max() <= 4, (what, ulps.max())
    return float(ulps.max()) if ulps.size else 0.0


# ---- 1. the sampler on given angles and exponentials ---------------------------------------------------------------------
def test_sampler_on_given_angles_is_scipys_expression(hip_ctx):
    import elfi_amd
    alpha, scale, TH, W = R.step_inputs()
    ref, B = R.stable_step(alpha, scale, TH, W)
    got = elfi_amd.levy_stable(alpha, scale, angle=TH, expo=W)
    assert got.shape == alpha.shape
    check_steps(got, ref, B, 'sampler')
    assert np.all(got[scale == 0][~np.isnan(ref[scale == 0])] == 0)
    # the shape of alpha is kept; scalars broadcast
    g2 = elfi_amd.levy_stable(alpha[:12].reshape(3, 4), 2.0, angle=TH[:12].reshape(3, 4), expo=W[:12].reshape(3, 4))
    assert g2.shape == (3, 4) and np.array_equal(g2.ravel(), elfi_amd.levy_stable(alpha[:12], np.full(12, 2.0), angle=TH[:12], expo=W[:12]))


def test_sampler_dev_form_writes_n_elements(hip_ctx):
    import elfi_amd
    alpha, scale, TH, W = [a[13000:15077] for a in R.step_inputs()]
    n = len(alpha) - 5
    want = elfi_amd.levy_stable(alpha[:n], scale[:n], angle=TH[:n], expo=W[:n])
    d = [to_device(a) for a in (alpha, scale, TH, W)]
    import torch
    torch.cuda.synchronize()
    out = guarded_out(n, 1, 1)
    hip_ctx.call('elfihip_stable_dev', C.c_uint64(0), C.c_uint64(0), n, *[t.data_ptr() for t in d], out.ptr)
    hip_ctx.synchronize()
    assert np.array_equal(out.check(), want, equal_nan=True)
    out = guarded_out(n, 1, 0)
    hip_ctx.call('elfihip_stable_dev', C.c_uint64(5), C.c_uint64(2), n, d[0].data_ptr(), d[1].data_ptr(), None, None, out.ptr)
    hip_ctx.synchronize()
    assert np.array_equal(out.check(), elfi_amd.levy_stable(alpha[:n], scale[:n], seed=5, stream=2), equal_nan=True)


# ---- 2. the sampler's own draws ---------------------------------------------------------------------------------------------
def test_sampler_draws_are_counter_based(hip_ctx):
    import elfi_amd
    a = np.full(1000, 1.5)
    x = elfi_amd.levy_stable(a, 3.0, seed=11, stream=4)
    assert np.array_equal(elfi_amd.levy_stable(a[:10], 3.0, seed=11, stream=4), x[:10])
    assert np.array_equal(elfi_amd.levy_stable(a[:257], 3.0, seed=11, stream=4), x[:257])
    other = elfi_amd.levy_stable(a, 3.0, seed=11, stream=5)
    assert not np.any(other == x) and not np.any(elfi_amd.levy_stable(a, 3.0, seed=12, stream=4) == x)
    # element e is the transform of the angle and exponential of Philox counter e; the exponential goes through the device's
    # log (4 ulp), and x varies as W^(1 - 1 / alpha), |1 - 1 / alpha| = 1 / 3 here: at most 4 EPS |x| more, to first order
    TH, W = R.angle_expo(11, 4, np.arange(1000))
    ref, B = R.stable_step(a, 3.0, TH, W)
    ok = R.step_mask(ref, B)
    assert (~ok).mean() <= R.MASK_SHARE and np.all(np.abs(x[ok] - ref[ok]) <= 2 * B[ok] + 4 * R.EPS * np.abs(ref[ok]))


def test_sampler_distribution(hip_ctx, golden):
    import elfi_amd
    n = 100000
    # alpha = 2: normal with variance 2 scale^2
    s = 1.5
    x = elfi_amd.levy_stable(np.full(n, 2.0), s, seed=21)
    z_mean = x.mean() / np.sqrt(2 * s * s / n)
    z_var = (x.var() - 2 * s * s) / (2 * s * s * np.sqrt(2.0 / n))
    print('alpha = 2: z(mean) %.2f, z(variance) %.2f' % (z_mean, z_var))
    assert abs(z_mean) <= 4 and abs(z_var) <= 4
    # alpha = 1: Cauchy of scale s, quartiles -s, 0, s
    x = elfi_amd.levy_stable(np.full(n, 1.0), s, seed=22)
    for q, point in ((0.25, -s), (0.5, 0.0), (0.75, s)):
        z = ((x < point).mean() - q) / np.sqrt(q * (1 - q) / n)
        print('alpha = 1: z(share below %.2f) %.2f' % (point, z))
        assert abs(z) <= 4
    # alpha in {0.8, 1.5}: SciPy's recorded levy_stable.cdf
    for a, probs in zip(golden['cdf_alpha'], golden['cdf_p']):
        x = elfi_amd.levy_stable(np.full(n, a), 1.0, seed=23)
        for point, q in zip(golden['cdf_x'], probs):
            z = ((x < point).mean() - q) / np.sqrt(q * (1 - q) / n)
            print('alpha = %.1f: z(share below %.1f) %.2f' % (a, point, z))
            assert abs(z) <= 4


# ---- 3. the model on the recorded draws ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SETS)
def test_model_on_golden_draws(hip_ctx, golden, name):
    import elfi_amd
    alpha, gamma, p0, draws, Xg, Sg = golden_set(golden, name)
    n_toads, n_days = (int(v) for v in golden[name + '_shape'])
    S, X, dx = elfi_amd.toad_summaries(alpha, gamma, p0, n_toads=n_toads, n_days=n_days, draws=draws, return_series=True,
                                       return_steps=True)
    assert S.shape == Sg.shape and X.shape == Xg.shape and dx.shape == draws[0].shape
    ref, B = R.stable_step(alpha[:, None, None], gamma[:, None, None], draws[1], draws[2])
    check_steps(dx, ref, B, name)
    assert np.array_equal(R.simulate(alpha, gamma, p0, draws[0], dx, draws[3]), X)
    worst = check_summaries(S, R.all_summaries(X, LAGS), name)
    print(name, 'log differences: worst %.1f ulp from NumPy on the same positions' % worst)
    if name in ('gamma_zero', 'p0_one'):
        assert np.array_equal(X, Xg)                   # no step is used, or every step is 0 gamma
    if np.array_equal(X, Xg):
        check_summaries(S, Sg, name + ' against the recorded summaries')


def test_sort_sizes(hip_ctx, golden):
    import elfi_amd
    # the full 4 092: nobody returns and nothing is shorter than thd = 0
    alpha, gamma, p0, draws, Xg, _ = golden_set(golden, 'p0_zero')
    S, X = elfi_amd.toad_summaries(alpha, gamma, p0, draws=draws, thd=0., return_series=True)
    assert S[0, 0] == 0 and S[0, 12] == 0
    check_summaries(S, R.all_summaries(X, LAGS, thd=0.))
    # 0, 1, 2 and 3 displacements to sort at lag 1: 3 toads, 4 days; everybody returns to day 0 but the cells named here
    U = np.zeros((4, 3, 3))
    U[1, 2, 0] = U[2, 0, 0] = U[3, 2, :] = 0.9         # row 1: one move on the last day; row 2: out and back; row 3: three moves
    TH, W = np.full(U.shape, 0.7), np.full(U.shape, 1.3)
    TH[3, 2] = [0.7, -0.9, 1.2]
    Rr = np.zeros(U.shape, dtype=np.int32)
    for lags in ((1,), (1, 2)):
        S, X = elfi_amd.toad_summaries(2.0, 100., 0.5, n_toads=3, n_days=4, lags=lags, draws=(U, TH, W, Rr), return_series=True)
        assert S.shape == (4, 12 * len(lags)) and (9 - S[:, 0]).tolist() == [0, 1, 2, 3]
        check_summaries(S, R.all_summaries(X, lags))
        assert np.all(np.isposinf(S[0, 1:12])) and np.all(S[1, 2:12] == -20) and np.isfinite(S[3, 1:12]).all()
    # other quantiles, one quantile, another threshold
    for p in (np.array([0.5]), np.array([0.05, 0.3, 0.31, 0.99]), np.linspace(0, 1, 64)):
        S, X = elfi_amd.toad_summaries(alpha, gamma, p0, draws=draws, lags=(3, 1), p=p, thd=25., return_series=True)
        assert S.shape == (1, 2 * (len(p) + 1))
        ref = np.hstack([R.summaries(X, lag, p, 25.) for lag in (3, 1)])
        assert np.array_equal(S.reshape(2, -1)[:, :2], ref.reshape(2, -1)[:, :2])
        assert np.array_equal(np.isfinite(S), np.isfinite(ref)) and np.all(R.ulp_distance(S, ref)[np.isfinite(ref)] <= 4)


# ---- 4. the model on its own draws ------------------------------------------------------------------------------------------
SHAPES = [(1, 2, 1, (1,)), (2, 9, 3, (1, 2, 4, 8)), (64, 9, 3, (8, 1)), (65, 63, 3, (1, 2, 4, 8)), (66, 63, 130, (1, 2, 4, 8)),
          (66, 2, 3, (1,)), (1, 63, 3, (1, 2, 4, 8))]


@pytest.mark.parametrize('n_toads,n_days,n,lags', SHAPES)
def test_model_on_its_own_draws(hip_ctx, n_toads, n_days, n, lags):
    import elfi_amd
    rs = np.random.RandomState(n_toads * 100 + n_days)
    alpha, gamma, p0 = rs.uniform(1, 2, n), rs.uniform(0, 100, n), rs.uniform(0, 0.9, n)
    kw = dict(n_toads=n_toads, n_days=n_days, lags=lags)
    S, X, dx, draws = elfi_amd.toad_summaries(alpha, gamma, p0, seed=31, stream=6, first_index=5, return_series=True,
                                              return_steps=True, return_draws=True, **kw)
    U, TH, W, Rr = R.philox_draws(31, 6, 5, n, n_toads, n_days)
    assert np.array_equal(draws[0], U) and np.array_equal(draws[1], TH) and np.array_equal(draws[3], Rr)
    assert draws[3].dtype == np.int32 and R.ulp_distance(draws[2], W).max() <= 4
    # the step of a cell is the sampler's transform of the cell's angle and exponential
    a3, g3 = np.broadcast_to(alpha[:, None, None], TH.shape), np.broadcast_to(gamma[:, None, None], TH.shape)
    assert np.array_equal(dx, elfi_amd.levy_stable(a3, g3, angle=draws[1], expo=draws[2]))
    assert np.array_equal(R.simulate(alpha, gamma, p0, draws[0], dx, draws[3]), X)
    check_summaries(S, R.all_summaries(X, lags))
    # replaying the returned draws gives the same numbers; the optional outputs do not change S
    S2, X2 = elfi_amd.toad_summaries(alpha, gamma, p0, draws=draws, return_series=True, **kw)
    assert np.array_equal(S2, S) and np.array_equal(X2, X)
    assert np.array_equal(elfi_amd.toad_summaries(alpha, gamma, p0, seed=31, stream=6, first_index=5, **kw), S)
    # a row does not depend on the batch: it is moved by first_index exactly as by position
    k = n // 2
    S3, X3 = elfi_amd.toad_summaries(alpha[k:], gamma[k:], p0[k:], seed=31, stream=6, first_index=5 + k, return_series=True, **kw)
    assert np.array_equal(S3, S[k:]) and np.array_equal(X3, X[k:])


def test_invalid_rows_are_nan_and_alone(hip_ctx):
    import elfi_amd
    alpha = np.array([1.5, 0.0, 1.5, 2.5, 1.5, np.nan, 1.5, 1.5, 1.5, 1.5, 1.2])
    gamma = np.array([30., 30., 30., 30., 30., 30., -1., np.nan, 30., 30., 10.])
    p0 = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 1.5, np.nan, 0.0])
    bad = np.array([0, 1, 0, 1, 0, 1, 1, 1, 1, 1, 0], dtype=bool)
    S, X, dx = elfi_amd.toad_summaries(alpha, gamma, p0, n_toads=7, n_days=12, seed=3, return_series=True, return_steps=True)
    assert np.all(np.isnan(S[bad])) and np.all(np.isnan(X[bad])) and np.all(np.isnan(dx[bad]))
    assert not np.isnan(S[~bad]).any() and not np.isnan(X[~bad]).any()
    for row in np.flatnonzero(~bad):
        assert np.array_equal(elfi_amd.toad_summaries(alpha[row], gamma[row], p0[row], n_toads=7, n_days=12, seed=3, first_index=row), S[row:row + 1])


def test_dev_form_at_a_callers_pitch(hip_ctx):
    import torch
    import elfi_amd
    n, n_toads, n_days, lags = 5, 5, 9, np.array([1, 8], dtype=np.int32)
    p = np.linspace(0, 1, 11)
    cells, grid, ns = (n_days - 1) * n_toads, n_days * n_toads, 24
    rs = np.random.RandomState(9)
    alpha, gamma, p0 = rs.uniform(1, 2, n), rs.uniform(0, 100, n), rs.uniform(0, 0.9, n)
    S, X, dx, draws = elfi_amd.toad_summaries(alpha, gamma, p0, n_toads=n_toads, n_days=n_days, lags=lags, seed=8,
                                              return_series=True, return_steps=True, return_draws=True)
    guard = np.float64(SENTINEL).view(np.int64)

    def rows_of(t, pitch, width, lead, dtype=np.float64):
        h = t.cpu().numpy()
        body = h[lead:lead + n * pitch].reshape(n, pitch)
        outside = np.concatenate([h[:lead], body[:, width:].ravel(), h[lead + n * pitch:]])
        assert np.all(outside.view(np.int64 if dtype == np.float64 else np.int32) == (guard if dtype == np.float64 else -77)), 'a store outside the rows'
        return body[:, :width].copy()

    def buf(pitch, lead, dtype=torch.float64):
        return torch.full((lead + n * pitch + 8,), SENTINEL if dtype == torch.float64 else -77, dtype=dtype, device='cuda')

    dpar = [to_device(a) for a in (alpha, gamma, p0)]
    for given in (False, True):
        pitches = dict(S=ns + 3, X=grid + 1, Dx=cells + 2, echo=cells + 1, draws=cells + 5)
        tS, tX, tDx = buf(pitches['S'], 1), buf(pitches['X'], 3), buf(pitches['Dx'], 2)
        tE = [buf(pitches['echo'], 1) for _ in range(3)] + [buf(pitches['echo'], 2, torch.int32)]
        din, in_ptrs = [], [None] * 4
        if given:
            for a in draws:
                host = np.full((n, pitches['draws']), np.nan if a.dtype == np.float64 else 0, dtype=a.dtype)
                host[:, :cells] = a.reshape(n, cells)
                din.append(torch.from_numpy(host).cuda())
            in_ptrs = [t.data_ptr() for t in din]
        torch.cuda.synchronize()
        hip_ctx.call('elfihip_toad_summaries_dev', *in_ptrs, pitches['draws'], C.c_uint64(8), C.c_uint64(0), 0, n, n_toads, n_days,
                     len(lags), lags.ctypes.data, len(p), p.ctypes.data, C.c_double(10.), *[t.data_ptr() for t in dpar],
                     tS.data_ptr() + 8, pitches['S'], tX.data_ptr() + 24, pitches['X'], tDx.data_ptr() + 16, pitches['Dx'],
                     tE[0].data_ptr() + 8, tE[1].data_ptr() + 8, tE[2].data_ptr() + 8, tE[3].data_ptr() + 8, pitches['echo'])
        hip_ctx.synchronize()
        assert np.array_equal(rows_of(tS, pitches['S'], ns, 1), S)
        assert np.array_equal(rows_of(tX, pitches['X'], grid, 3), X.reshape(n, grid))
        assert np.array_equal(rows_of(tDx, pitches['Dx'], cells, 2), dx.reshape(n, cells))
        for t, a in zip(tE[:3], draws[:3]):
            assert np.array_equal(rows_of(t, pitches['echo'], cells, 1), a.reshape(n, cells))
        assert np.array_equal(rows_of(tE[3], pitches['echo'], cells, 2, np.int32), draws[3].reshape(n, cells))


# ---- 5. through ELFI --------------------------------------------------------------------------------------------------------
def _reference():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi
    return elfi


def test_toad_model_through_elfi(hip_ctx):
    _reference()
    import elfi_amd
    m = elfi_amd.toad_model(seed_obs=4)
    assert all(name in m.nodes for name in ['alpha', 'gamma', 'p0', 'toad', 'S1', 'S2', 'S4', 'S8', 'd'])
    assert m.parameter_names == ['alpha', 'gamma', 'p0']
    out = m.generate(5, outputs=['alpha', 'gamma', 'p0', 'toad', 'S1', 'S2', 'S4', 'S8', 'd'], seed=2)
    assert out['toad'].shape == (5, 48) and out['d'].shape == (5,) and out['alpha'].shape == (5,)
    for k, name in enumerate(('S1', 'S2', 'S4', 'S8')):
        assert out[name].shape == (5, 12) and np.array_equal(out[name], out['toad'][:, 12 * k:12 * k + 12])
    assert np.all(out['toad'][:, 0] >= 0) and np.all(out['toad'][:, 0] <= 66 * 62)
    bsl = elfi_amd.HipBSL(elfi_amd.toad_model(seed_obs=4), n_sim_round=100, feature_names=['S1', 'S2', 'S4', 'S8'], seed=1)
    res = bsl.sample(20, sigma_proposals=np.diag([1e-4, 1e-2, 1e-5]), params0=[1.7, 35.0, 0.6], bar=False)
    assert type(res).__name__ == 'BslSample' and np.all(np.isfinite(bsl.state['logposterior']))
    moves = np.count_nonzero(np.any(np.diff(bsl.state['params'], axis=0) != 0, axis=1))
    print('BSL on the toad model: %d accepted moves of 19' % moves)
    assert moves >= 1
