"""GPU: the counter-based Poisson sampler (csrc/poisson.hpp, elfi_amd.poisson) and the Ricker example model on the device
(csrc/series.hip: ricker_kernel, elfi_amd.ricker_summaries, fused_models.ricker_model).

The sampler equals its NumPy statement (tests/ricker_ref.py: poisson_ref, itself held to scipy.stats.poisson in
tests/test_ricker.py) exactly, outside the draws that statement marks as decided in the last bits.  The stock satisfies the
one-step relation against NumPy within 4 ulp (the map is chaotic: whole trajectories are not comparable), the counts are
the sampler's on the device's own stock, and summaries and distances are NumPy's bit for bit on the device's counts.
"""
import ctypes as C

import numpy as np
import pytest

import ricker_ref as R

pytestmark = pytest.mark.gpu

U64 = C.c_uint64
EXACT_LAM_MAX = 1e6      # above it the two sides of the PTRS log test are differences of numbers near 1e16


def _z_scores(x, lam):
    n = x.size
    return (x.mean() - lam) / np.sqrt(lam / n), (x.var(ddof=1) - lam) / np.sqrt((lam + 2 * lam * lam) / n)


def _compare_counts(got, lam, seed, stream):
    """The device's counts against the statement on the same intensities: exact (NaN pattern and zeros included) outside
    the boundary-sensitive mask, for every intensity up to EXACT_LAM_MAX and every invalid one; the mask covers at most 1e-3
    of the elements.  Returns the masked share."""
    want, sens = R.poisson_ref(lam, seed, stream)
    share = float(sens[~(lam > EXACT_LAM_MAX)].mean())
    print('boundary-sensitive share %.3g (%d of %d)' % (share, sens.sum(), sens.size))
    assert share <= 1e-3
    check = ~sens & ~(lam > EXACT_LAM_MAX)
    assert np.array_equal(got[check], want[check], equal_nan=True)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    big = (lam > EXACT_LAM_MAX) & ~np.isnan(want)
    # only the distribution is claimed there: whole numbers within 8 standard deviations (probability 1e-15 each)
    assert np.all(got[big] == np.floor(got[big])) and np.all(np.abs(got[big] - lam[big]) <= 8 * np.sqrt(lam[big]) + 1)
    return share


# ---- 1. the sampler ---------------------------------------------------------------------------------------------------
def _intensities():
    rs = np.random.RandomState(20275)
    special = [0.0, np.nextafter(10.0, 0.0), 10.0, 2.0 ** 53, 1e15, np.nan, np.inf, -1.0, 2.0 ** 54]
    return np.concatenate([rs.uniform(0, 10, 10000), 10 ** rs.uniform(1, 6, 10000), 10 ** rs.uniform(-6, 1.5, 10000), special])


def test_poisson_is_the_statement(hip_ctx):
    import torch
    import elfi_amd
    lam = _intensities()
    n, seed, stream = lam.size, 77, 3
    x = elfi_amd.poisson(lam, seed=seed, stream=stream)
    assert x.shape == lam.shape and x.dtype == np.float64
    _compare_counts(x, lam, seed, stream)
    assert x[30000] == 0 and np.all(np.isnan(x[30005:])) and np.all(np.isfinite(x[:30005]))
    # element e does not depend on n: the prefix of a draw twice as long
    x2 = elfi_amd.poisson(np.concatenate([lam, lam]), seed=seed, stream=stream)
    assert np.array_equal(x2[:n], x, equal_nan=True)
    assert not np.array_equal(x2[n:2 * n - 9], x[:n - 9])       # other counters, other draws
    # another stream gives other draws, the shape of lam is kept
    y = elfi_amd.poisson(lam[:30000].reshape(300, 100), seed=seed, stream=stream + 1)
    assert y.shape == (300, 100) and np.mean(y.reshape(-1) != x[:30000]) > 0.3
    # the _dev form
    dl = torch.from_numpy(lam).cuda()
    do = torch.full((n + 4,), -7.0, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    assert hip_ctx.lib.elfihip_poisson_dev(hip_ctx.handle, U64(seed), U64(stream), n, dl.data_ptr(), do.data_ptr()) == 0
    hip_ctx.synchronize()
    o = do.cpu().numpy()
    assert np.array_equal(o[:n], x, equal_nan=True) and np.all(o[n:] == -7.0)


@pytest.mark.parametrize('lam', [1e9, 1e12])
def test_poisson_distribution_at_large_intensities(hip_ctx, lam):
    import elfi_amd
    x = elfi_amd.poisson(np.full(100000, lam), seed=5, stream=11)
    z_mean, z_var = _z_scores(x, lam)
    print('lam %g: z_mean %.2f z_var %.2f' % (lam, z_mean, z_var))
    assert np.all(x == np.floor(x))
    assert abs(z_mean) <= 4 and abs(z_var) <= 4


# ---- 2. Ricker on given normals ----------------------------------------------------------------------------------------
def _prior_draws(n, rs):
    import scipy.stats as ss
    return (ss.expon.rvs(np.e, 2, size=n, random_state=rs), ss.truncnorm.rvs(0, 5, size=n, random_state=rs),
            ss.uniform.rvs(0, 100, size=n, random_state=rs))


def _ulp_distance(got, want):
    """Largest distance in ulp of `want` over its finite nonzero entries; NaN, inf and zero patterns must be equal."""
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == 0, want == 0)
    assert np.array_equal(np.isinf(got), np.isinf(want))
    ok = np.isfinite(want) & (want != 0)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - want[ok]) / np.spacing(np.abs(want[ok]))))


def _one_step(t1, t2, Z, St, stock_init):
    prev = np.column_stack([np.full(St.shape[0], float(stock_init)), St[:, :-1]])
    with np.errstate(all='ignore'):
        return prev * np.exp((t1[:, None] - prev) + t2[:, None] * Z)


@pytest.mark.parametrize('n,n_obs', [(1, 50), (65, 1), (777, 50), (4097, 37), (100, 2048), (333, 129)])
def test_ricker_on_given_normals(hip_ctx, n, n_obs):
    import elfi_amd
    rs = np.random.RandomState(17 * n + n_obs)
    t1, t2, t3 = _prior_draws(n, rs)
    Z = rs.randn(n, n_obs)
    if n > 2:
        t1[1], t2[1] = 25.0, 0.0       # crashes: exp(24), then exactly 0 for good
        t1[2] = 800.0                  # overflows: inf, then NaN
    seed, stream, stock_init = 99, 4, 1.0
    obs = np.array([3.5, 40.25, 7.0])
    S, Y, St, Zo, D = elfi_amd.ricker_summaries(t1, t2, t3, stock_init=stock_init, n_obs=n_obs, noise=Z, seed=seed,
                                                stream=stream, observed=obs, return_series=True, return_stock=True,
                                                return_draws=True)
    assert S.shape == (n, 3) and Y.shape == St.shape == Zo.shape == (n, n_obs) and D.shape == (n,)
    assert np.array_equal(Zo, Z)
    ulp = _ulp_distance(St, _one_step(t1, t2, Z, St, stock_init))
    print('largest one-step ulp distance %.2f' % ulp)
    assert ulp <= 4
    if n > 2:
        assert np.all(St[1, 1:] == 0) and St[1, 0] > 1e10 and np.all(Y[1, 1:] == 0)
        assert np.isinf(St[2, 0]) and np.all(np.isnan(St[2, 1:])) and np.all(np.isnan(Y[2])) and np.all(np.isnan(S[2, :2]))
        assert S[2, 2] == 0 and S[1, 2] == n_obs - 1
    _compare_counts(Y, t3[:, None] * St, seed, stream + 1)
    assert np.array_equal(S, R.ricker_summaries(Y), equal_nan=True)
    assert np.array_equal(D, R.chi_squared(S, obs), equal_nan=True)
    # an observed #0 of 0: inf, or NaN where the simulated #0 is 0 too, as the reference's division gives them
    obs0 = np.array([3.5, 40.25, 0.0])
    S0, D0 = elfi_amd.ricker_summaries(t1, t2, t3, stock_init=stock_init, n_obs=n_obs, noise=Z, seed=seed, stream=stream,
                                       observed=obs0)
    assert np.array_equal(S0, S, equal_nan=True) and np.array_equal(D0, R.chi_squared(S, obs0), equal_nan=True)
    assert not np.any(np.isfinite(D0))
    # without the optional outputs the summaries are the same
    assert np.array_equal(elfi_amd.ricker_summaries(t1, t2, t3, stock_init=stock_init, n_obs=n_obs, noise=Z, seed=seed,
                                                    stream=stream), S, equal_nan=True)


# ---- 3. the deterministic form -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,n_obs', [(1, 50), (65, 1), (1000, 50), (100, 300)])
def test_ricker_deterministic(hip_ctx, n, n_obs):
    import scipy.stats as ss
    import elfi_amd
    rs = np.random.RandomState(n + n_obs)
    t1 = ss.expon.rvs(np.e, size=n, random_state=rs)
    stock_init, obs = 1.5, np.array([2.25, 1.0, 1.0])
    S, Y, St, D = elfi_amd.ricker_summaries(t1, stock_init=stock_init, n_obs=n_obs, observed=obs, distance='euclidean_mean',
                                            return_series=True, return_stock=True)
    assert np.all(Y[:, 0] == stock_init) and np.array_equal(St, Y)
    if n_obs > 1:
        with np.errstate(all='ignore'):
            want = Y[:, :-1] * np.exp((t1[:, None] - Y[:, :-1]))
        ulp = _ulp_distance(Y[:, 1:], want)
        print('largest one-step ulp distance %.2f' % ulp)
        assert ulp <= 4
    assert np.array_equal(S, R.ricker_summaries(Y))
    assert np.array_equal(S[:, 0], np.mean(Y, axis=1))
    assert np.array_equal(D, elfi_amd.HipDistance('euclidean')(S[:, :1], obs[None, :1]))
    assert np.array_equal(elfi_amd.ricker_summaries(t1, stock_init=stock_init, n_obs=n_obs), S)


# ---- 4. normals drawn in the kernel = normals materialised by elfihip_randn_dev ---------------------------------------------
def _ricker_dev(hip_ctx, dZ, ldz, seed, stream, n, n_obs, t, obs, pad=0):
    import torch
    dt = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in t]
    dS = torch.full((n, 3 + pad), -7.0, dtype=torch.float64, device='cuda')
    dY, dSt, dZo = [torch.full((n, n_obs + pad), -7.0, dtype=torch.float64, device='cuda') for _ in range(3)]
    dD = torch.empty(n, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    rc = hip_ctx.lib.elfihip_ricker_summaries_dev(hip_ctx.handle, dZ, ldz, U64(seed), U64(stream), n, n_obs, dt[0].data_ptr(),
                                                  dt[1].data_ptr(), dt[2].data_ptr(), C.c_double(1.0), obs.ctypes.data, 0,
                                                  dS.data_ptr(), 3 + pad, dY.data_ptr(), n_obs + pad, dSt.data_ptr(),
                                                  n_obs + pad, dZo.data_ptr(), n_obs + pad, dD.data_ptr())
    assert rc == 0, hip_ctx.lib.elfihip_last_error(hip_ctx.handle)
    hip_ctx.synchronize()
    S, Y, St, Zo = [a.cpu().numpy() for a in (dS, dY, dSt, dZo)]
    assert np.all(S[:, 3:] == -7.0)                                       # nothing written beyond a row
    assert all(np.all(a[:, n_obs:] == -7.0) for a in (Y, St, Zo))
    return Zo[:, :n_obs], St[:, :n_obs], Y[:, :n_obs], S[:, :3], dD.cpu().numpy()


@pytest.mark.parametrize('n,n_obs', [(1, 50), (777, 51), (50000, 50)])
def test_ricker_drawn_is_materialised(hip_ctx, n, n_obs):
    import torch
    seed, stream = 1234, 6
    t = _prior_draws(n, np.random.RandomState(n))
    obs = np.array([3.5, 40.25, 7.0])
    dZ = torch.empty(n * n_obs, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    assert hip_ctx.lib.elfihip_randn_dev(hip_ctx.handle, U64(seed), U64(stream), n * n_obs, C.c_double(0.0), C.c_double(1.0),
                                         dZ.data_ptr()) == 0
    hip_ctx.synchronize()
    given = _ricker_dev(hip_ctx, dZ.data_ptr(), n_obs, seed, stream, n, n_obs, t, obs)
    drawn = _ricker_dev(hip_ctx, None, n_obs, seed, stream, n, n_obs, t, obs)
    for a, b in zip(given, drawn):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(drawn[0], dZ.cpu().numpy().reshape(n, n_obs))
    assert np.array_equal(drawn[3], R.ricker_summaries(drawn[2]), equal_nan=True)
    # the caller's pitch: rows of Z, S, Y, St and Zo further apart than their length
    dZp = torch.full((n, n_obs + 5), np.nan, dtype=torch.float64, device='cuda')
    dZp[:, :n_obs] = dZ.view(n, n_obs)
    torch.cuda.synchronize()
    pitched = _ricker_dev(hip_ctx, dZp.data_ptr(), n_obs + 5, seed, stream, n, n_obs, t, obs, pad=3)
    for a, b in zip(given, pitched):
        assert np.array_equal(a, b, equal_nan=True)
    # a different stream: different normals
    other = _ricker_dev(hip_ctx, None, n_obs, seed, stream + 1, n, n_obs, t, obs)
    assert not np.any(other[0] == drawn[0])


# ---- 5. argument errors of the C entry points ----------------------------------------------------------------------------
def test_library_refuses_what_it_cannot_hold(hip_ctx):
    import torch
    from elfi_amd import _lib
    lib, h = hip_ctx.lib, hip_ctx.handle
    buf = torch.ones(4096, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    p, obs = buf.data_ptr(), np.ones(3)
    out = p + 8 * 1024

    def ricker(n_obs, observed=None, dD=None, n=2, sd=p, scale=p, which=0, dZ=None, dZo=None):
        return lib.elfihip_ricker_summaries_dev(h, dZ, n_obs, U64(1), U64(0), n, n_obs, p, sd, scale, C.c_double(1.0), observed,
                                                which, out, 3, None, n_obs, None, n_obs, dZo, n_obs, dD)
    assert ricker(2049) == _lib.ERR_ARG and b'2048' in lib.elfihip_last_error(h)
    assert ricker(0) == _lib.ERR_ARG and ricker(50, n=0) == _lib.ERR_ARG
    assert ricker(50, None, out + 64) == _lib.ERR_ARG               # a distance without observed summaries
    assert ricker(50, sd=None) == _lib.ERR_ARG and ricker(50, scale=None) == _lib.ERR_ARG
    assert ricker(50, sd=None, scale=None, dZ=p) == _lib.ERR_ARG    # the deterministic form takes no normals
    assert ricker(50, obs.ctypes.data, out + 64, which=2) == _lib.ERR_ARG
    assert ricker(50, obs.ctypes.data, out + 64) == 0 and ricker(50, sd=None, scale=None) == 0
    hip_ctx.synchronize()
    assert np.all(buf.cpu().numpy()[:1024] == 1.0)


# ---- 6. the models through ELFI's loops ------------------------------------------------------------------------------------
def _reference():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi
    return elfi


@pytest.mark.parametrize('stochastic', [True, False])
def test_ricker_model_through_the_loops(hip_ctx, stochastic):
    elfi = _reference()
    import elfi_amd
    from elfi.examples import ricker
    m = elfi_amd.ricker_model(seed_obs=4, stochastic=stochastic)
    ref = ricker.get_model(seed_obs=4, stochastic=stochastic)
    names = ['t1', 't2', 't3'] if stochastic else ['t1']
    public = [sorted(k for k in mdl.nodes if not k.startswith('_')) for mdl in (m, ref)]     # (_name_hash: constants)
    assert public[0] == public[1] == sorted(names + ['Ricker', 'd'] + (['Mean', 'Var', '#0'] if stochastic else ['Mean']))
    assert m.parameter_names == ref.parameter_names == names
    summaries = ['Mean', 'Var', '#0'] if stochastic else ['Mean']
    for name in summaries:          # the observed summaries are the reference's own
        assert np.array_equal(np.ravel(m[name].observed), np.ravel(ref[name].observed))
    batch = m.generate(1000, outputs=names + ['Ricker', 'd'] + summaries, seed=1)
    assert batch['Ricker'].shape == (1000, 3) and batch['d'].shape == (1000,)
    assert all(batch[k].shape == (1000,) for k in names + summaries)
    assert np.array_equal(batch['Mean'], batch['Ricker'][:, 0])
    rb = ref.generate(10, outputs=summaries + ['d'], seed=1)
    assert all(rb[k].shape == batch[k][:10].shape for k in summaries + ['d'])
    res = elfi_amd.HipRejection(m['d'], batch_size=2000, seed=2).sample(100, n_sim=10000)
    assert res.samples['t1'].shape == (100,) and np.all(np.isfinite(res.discrepancies))
    res2 = elfi.Rejection(m['d'], batch_size=2000, seed=2).sample(100, n_sim=10000)
    for k in names:
        assert np.array_equal(res2.samples[k], res.samples[k])
    assert np.array_equal(res2.discrepancies, res.discrepancies)
