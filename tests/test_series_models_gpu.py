"""GPU: the ARCH(1) and M/G/1 example models on the device (csrc/series.hip, elfi_amd.arch_summaries / mg1_summaries,
fused_models.arch_model / mg1_model).

On given draws the device series, summaries and quantiles equal the NumPy statement tests/series_ref.py bit for bit (that
statement is pinned to ELFI's own examples in tests/test_series_models.py); the logarithm of the inter-departure times is
the device library's, held to 4 ulp of np.log.  The draws made in the kernel are the words of the
library's generator (tests/philox_ref.py), the fused distances are HipDistance's, and the models run through ELFI's loops.
"""
import ctypes as C
import os

import numpy as np
import pytest

import series_ref as R

pytestmark = pytest.mark.gpu

U64 = C.c_uint64


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'series_models.npz'))


def _within_ulp(got, want, ulps=4):
    return np.all(np.abs(got - want) <= ulps * np.spacing(np.abs(want)))


def _arch_case(n, n_obs, seed):
    rs = np.random.RandomState(seed)
    t1, t2 = rs.uniform(-1, 1, n), rs.uniform(0, 1, n)
    W = R.arch_noise_from_state(rs, n, n_obs)
    return t1, t2, W


# ---- 1. ARCH on given noise ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,n_obs,n_lags', [(1, 100, 5), (777, 100, 5), (4097, 100, 5), (333, 37, 3), (200, 200, 5),
                                            (65, 7, 5), (100, 512, 8)])
def test_arch_on_given_noise_is_numpys(hip_ctx, n, n_obs, n_lags):
    import elfi_amd
    t1, t2, W = _arch_case(n, n_obs, 11 * n + n_obs)
    if n > 1:
        t1[-1], t2[-1] = 0.9, 40.0      # |e| grows by a factor of about e^1.2 per step: huge values, an overflow at 512 steps
    Yr = R.arch_series(t1, t2, W)
    Sr = R.arch_summaries(Yr, n_lags)
    if n_obs == 512:
        assert not np.all(np.isfinite(Sr[-1])) and not np.all(np.isfinite(Yr[-1]))
    S, Y = elfi_amd.arch_summaries(t1, t2, n_obs=n_obs, n_lags=n_lags, noise=W, return_series=True)
    assert S.shape == (n, 2 + n_lags + n_lags * (n_lags - 1) // 2) and Y.shape == (n, n_obs)
    assert np.array_equal(Y, Yr, equal_nan=True)
    assert np.array_equal(S, Sr, equal_nan=True)
    assert np.array_equal(np.isfinite(S), np.isfinite(Sr))
    # without the series output (no store pass in the kernel) the summaries are the same
    assert np.array_equal(elfi_amd.arch_summaries(t1, t2, n_obs=n_obs, n_lags=n_lags, noise=W), Sr, equal_nan=True)


def test_arch_golden_block(hip_ctx, golden):
    import elfi_amd
    g = golden
    S, Y = elfi_amd.arch_summaries(g['arch_t1'], g['arch_t2'], n_obs=100, n_lags=5, noise=g['arch_W'], return_series=True)
    assert np.array_equal(Y, g['arch_Y']) and np.array_equal(S, g['arch_S'])


# ---- 2. ARCH: noise drawn in the kernel = noise materialised by elfihip_randn_dev --------------------------------------
def _arch_dev(hip_ctx, dW, ldw, seed, stream, n, n_obs, n_lags, t1, t2, obs, pad=0):
    import torch
    m = 2 + n_lags + n_lags * (n_lags - 1) // 2
    dt1, dt2 = torch.from_numpy(t1).cuda(), torch.from_numpy(t2).cuda()
    dS = torch.full((n, m + pad), -7.0, dtype=torch.float64, device='cuda')
    dY = torch.full((n, n_obs + pad), -7.0, dtype=torch.float64, device='cuda')
    dD = torch.empty(n, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    rc = hip_ctx.lib.elfihip_arch_summaries_dev(hip_ctx.handle, dW, ldw, U64(seed), U64(stream), n, n_obs, n_lags,
                                                dt1.data_ptr(), dt2.data_ptr(), obs.ctypes.data, dS.data_ptr(), m + pad,
                                                dY.data_ptr(), n_obs + pad, dD.data_ptr())
    assert rc == 0, hip_ctx.lib.elfihip_last_error(hip_ctx.handle)
    hip_ctx.synchronize()
    S, Y = dS.cpu().numpy(), dY.cpu().numpy()
    assert np.all(S[:, m:] == -7.0) and np.all(Y[:, n_obs:] == -7.0)      # nothing written beyond a row
    return S[:, :m], Y[:, :n_obs], dD.cpu().numpy()


@pytest.mark.parametrize('n', [1, 777, 50000])
def test_arch_drawn_is_materialised(hip_ctx, n):
    import torch
    n_obs, n_lags, seed, stream = 100, 5, 1234, 6
    L = n_obs + 2
    rs = np.random.RandomState(n)
    t1, t2, obs = rs.uniform(-1, 1, n), rs.uniform(0, 1, n), rs.randn(17)
    dW = torch.empty(n * L, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    assert hip_ctx.lib.elfihip_randn_dev(hip_ctx.handle, U64(seed), U64(stream), n * L, C.c_double(0.0), C.c_double(1.0),
                                         dW.data_ptr()) == 0
    hip_ctx.synchronize()
    given = _arch_dev(hip_ctx, dW.data_ptr(), L, 0, 0, n, n_obs, n_lags, t1, t2, obs)
    drawn = _arch_dev(hip_ctx, None, L, seed, stream, n, n_obs, n_lags, t1, t2, obs)
    for a, b in zip(given, drawn):
        assert np.array_equal(a, b)
    W = dW.cpu().numpy().reshape(n, L)
    assert np.array_equal(given[1], R.arch_series(t1, t2, W))
    # the caller's pitch: rows of W, S and Y further apart than their length
    dWp = torch.full((n, L + 5), np.nan, dtype=torch.float64, device='cuda')
    dWp[:, :L] = dW.view(n, L)
    torch.cuda.synchronize()
    pitched = _arch_dev(hip_ctx, dWp.data_ptr(), L + 5, 0, 0, n, n_obs, n_lags, t1, t2, obs, pad=3)
    for a, b in zip(given, pitched):
        assert np.array_equal(a, b)
    # a different stream: different draws
    other = _arch_dev(hip_ctx, None, L, seed, stream + 1, n, n_obs, n_lags, t1, t2, obs)
    assert not np.any(other[1] == drawn[1])


def test_library_refuses_what_it_cannot_hold(hip_ctx):
    """Past the Python checks: a series longer than the LDS budget allows, lags or quantile counts outside the kernels'
    range and a distance without observed values are argument errors of the C entry points, never a truncated result."""
    import torch
    from elfi_amd import _lib
    lib, h = hip_ctx.lib, hip_ctx.handle
    buf = torch.zeros(4096, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    p, obs = buf.data_ptr(), np.zeros(64)
    out, out2 = p + 8 * 1024, p + 8 * 2048      # parameters: the zeros at p; outputs from element 1024 and 2048 on
    lo = np.zeros(65, dtype=np.int32)

    def arch(n_obs, n_lags, observed, dD):
        return lib.elfihip_arch_summaries_dev(h, None, n_obs + 2, U64(1), U64(0), 2, n_obs, n_lags, p, p, observed, out, 64,
                                              None, n_obs, dD)

    def mg1(n_obs, nq, observed, dD, hi_pos=0):
        hi = np.full(65, hi_pos, dtype=np.int32)
        return lib.elfihip_mg1_summaries_dev(h, None, n_obs, None, n_obs, U64(1), U64(0), 2, n_obs, p, p, p, nq,
                                             lo.ctypes.data, hi.ctypes.data, obs.ctypes.data, observed, None, out, n_obs,
                                             out2, 64, None, n_obs, None, n_obs, None, n_obs, dD)
    assert arch(2049, 5, None, None) == _lib.ERR_ARG and b'2048' in lib.elfihip_last_error(h)
    assert arch(100, 9, None, None) == _lib.ERR_ARG and arch(100, 0, None, None) == _lib.ERR_ARG
    assert arch(6, 5, None, None) == _lib.ERR_ARG
    assert arch(100, 5, None, out) == _lib.ERR_ARG                   # a distance without observed summaries
    assert mg1(2049, 10, None, None) == _lib.ERR_ARG and mg1(1, 1, None, None) == _lib.ERR_ARG
    assert mg1(50, 65, None, None) == _lib.ERR_ARG and mg1(50, 0, None, None) == _lib.ERR_ARG
    assert mg1(50, 10, None, out) == _lib.ERR_ARG
    assert mg1(50, 10, None, None, hi_pos=50) == _lib.ERR_ARG     # a quantile position outside the series
    assert arch(100, 5, None, None) == 0 and mg1(50, 10, None, None) == 0
    hip_ctx.synchronize()


# ---- 3. M/G/1 on given draws ---------------------------------------------------------------------------------------------
def _mg1_case(n, n_obs, seed):
    rs = np.random.RandomState(seed)
    t1 = rs.uniform(0, 10, n)
    t2, t3 = t1 + rs.uniform(0, 10, n), rs.uniform(0.01, 0.5, n)
    E, V = R.mg1_draws_from_state(rs, n, n_obs)
    return t1, t2, t3, E, V


@pytest.mark.parametrize('n,n_obs,nq', [(1, 50, 10), (1000, 50, 10), (4097, 50, 10), (333, 37, 4), (200, 130, 10),
                                        (64, 2, 2), (100, 512, 64)])
def test_mg1_on_given_draws_is_numpys(hip_ctx, n, n_obs, nq):
    import elfi_amd
    t1, t2, t3, E, V = _mg1_case(n, n_obs, 13 * n + n_obs)
    q = np.linspace(0, 1, nq)
    Yr = R.mg1_series(t1, t2, t3, E, V)
    logy, Q, Y = elfi_amd.mg1_summaries(t1, t2, t3, n_obs=n_obs, q=q, draws=(E, V), return_series=True)
    assert logy.shape == Y.shape == (n, n_obs) and Q.shape == (n, nq)
    assert np.array_equal(Y, Yr)
    assert np.array_equal(Q, R.mg1_quantiles(Yr, q))
    assert np.array_equal(Q, np.quantile(Yr, q, axis=1).T)
    assert _within_ulp(logy, R.log_identity(Yr))


def test_mg1_golden_block(hip_ctx, golden):
    import elfi_amd
    g = golden
    logy, Q, Y = elfi_amd.mg1_summaries(g['mg1_t1'], g['mg1_t2'], g['mg1_t3'], n_obs=50, q=g['mg1_q'],
                                        draws=(g['mg1_E'], g['mg1_V']), return_series=True)
    assert np.array_equal(Y, g['mg1_Y']) and np.array_equal(Q, g['mg1_Q'])
    assert _within_ulp(logy, g['mg1_logY'])


# ---- 4. M/G/1 with the draws made in the kernel -------------------------------------------------------------------------
def test_mg1_drawn_form(hip_ctx):
    import elfi_amd
    import philox_ref as P
    n, n_obs, seed, stream = 2000, 50, 4321, 10          # 10^5 draws of each kind
    t1, t2, t3, _, _ = _mg1_case(n, n_obs, 3)
    logy, Q, Y, E, V = elfi_amd.mg1_summaries(t1, t2, t3, n_obs=n_obs, seed=seed, stream=stream, return_series=True,
                                              return_draws=True)
    again = elfi_amd.mg1_summaries(t1, t2, t3, n_obs=n_obs, draws=(E, V), return_series=True, return_draws=True)
    for a, b in zip((logy, Q, Y, E, V), again):
        assert np.array_equal(a, b)
    assert np.array_equal(Y, R.mg1_series(t1, t2, t3, E, V))
    Ef, Vf = E.reshape(-1), V.reshape(-1)
    for e in (0, 1, 12345, 50 * 777 + 49, n * n_obs - 1):
        words = []
        for s in (stream, stream + 1):
            r = P.philox4x32_10(((e // 2) & 0xFFFFFFFF, (e // 2) >> 32, s, 0), (seed, 0))
            hi, lo = (r[0], r[1]) if e % 2 == 0 else (r[2], r[3])
            words.append((hi << 21) | (lo >> 11))
        assert Vf[e] == words[1] * 2.0 ** -53
        assert _within_ulp(Ef[e], -np.log((words[0] + 1) * 2.0 ** -53))
    assert np.all(Ef > 0) and np.all(np.isfinite(Ef)) and np.all((Vf >= 0) & (Vf < 1))
    # 5 standard errors over 10^5 draws: 5 / sqrt(10^5) = 0.016 for Exp(1), 5 / sqrt(12 10^5) = 0.0046 for U(0, 1)
    assert abs(Ef.mean() - 1.0) < 0.016 and abs(Vf.mean() - 0.5) < 0.0046
    # a different seed: different draws
    other = elfi_amd.mg1_summaries(t1, t2, t3, n_obs=n_obs, seed=seed + 1, stream=stream, return_draws=True)
    assert not np.any(other[2] == E) and not np.any(other[3] == V)


# ---- 5. the fused distances are HipDistance's -----------------------------------------------------------------------------
def test_fused_distances_are_hipdistances(hip_ctx):
    import elfi_amd
    n = 3001
    t1, t2, W = _arch_case(n, 100, 5)
    obs = R.arch_summaries(R.arch_series(0.3, 0.7, W[:1]), 5)[0]
    for kw in (dict(noise=W), dict(seed=5, stream=2)):
        S, D = elfi_amd.arch_summaries(t1, t2, n_obs=100, n_lags=5, observed=obs, **kw)
        assert np.array_equal(D, elfi_amd.HipDistance('euclidean')(S, obs[None]))
        assert np.array_equal(D, R.weighted_euclidean(S, obs))
    m1, m2, m3, E, V = _mg1_case(n, 50, 6)
    q = np.linspace(0, 1, 10)
    qobs = R.mg1_quantiles(R.mg1_series(1.0, 5.0, 0.2, E[:1], V[:1]), q)[0]
    w = (1 / 100) ** q
    for kw in (dict(draws=(E, V)), dict(seed=5, stream=2)):
        _, Q, D = elfi_amd.mg1_summaries(m1, m2, m3, n_obs=50, q=q, observed=qobs, **kw)
        assert np.array_equal(D, elfi_amd.HipDistance('euclidean')(Q, qobs[None]))
        _, Q, Dw = elfi_amd.mg1_summaries(m1, m2, m3, n_obs=50, q=q, observed=qobs, w=w, **kw)
        assert np.array_equal(Dw, elfi_amd.HipDistance('euclidean', w=w)(Q, qobs[None]))
        assert np.array_equal(Dw, R.weighted_euclidean(Q, qobs, w)) and not np.array_equal(D, Dw)


# ---- 6. the models through ELFI's loops ---------------------------------------------------------------------------------
def _reference():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi
    return elfi


def test_arch_model_through_the_loops(hip_ctx):
    elfi = _reference()
    import elfi_amd
    m = elfi_amd.arch_model(seed_obs=4)
    names = R.arch_names(5)
    assert all(name in m.nodes for name in ['t1', 't2', 'Y', 'd'] + names) and m.parameter_names == ['t1', 't2']
    res = elfi_amd.HipRejection(m['d'], batch_size=20000, seed=2).sample(200, n_sim=100000)
    t1, t2 = res.samples['t1'], res.samples['t2']
    assert t1.shape == (200,) and np.all(np.isfinite(res.discrepancies))
    print('ARCH posterior means', np.mean(t1), np.mean(t2))
    assert abs(np.mean(t1) - 0.23) < 0.1 and abs(np.mean(t2) - 0.60) < 0.1
    res2 = elfi.Rejection(m['d'], batch_size=20000, seed=2).sample(200, n_sim=100000)
    assert np.array_equal(res2.samples['t1'], t1) and np.array_equal(res2.samples['t2'], t2)
    assert np.array_equal(res2.discrepancies, res.discrepancies)


def test_mg1_model_through_the_loops(hip_ctx):
    elfi = _reference()
    import elfi_amd
    m = elfi_amd.mg1_model(seed_obs=4)
    assert all(name in m.nodes for name in ['t1', 't2', 't3', 'MG1', 'log_identity', 'quantiles', 'd'])
    res = elfi_amd.HipRejection(m['d'], batch_size=20000, seed=2).sample(200, n_sim=100000)
    s = res.samples
    assert s['t1'].shape == (200,) and np.all(np.isfinite(res.discrepancies))
    means = [np.mean(s[k]) for k in ('t1', 't2', 't3')]
    print('M/G/1 posterior means', means)
    for got, centre, margin in zip(means, (1.05, 4.75, 0.202), (0.3, 1.0, 0.03)):
        assert abs(got - centre) < margin
    res2 = elfi.Rejection(m['d'], batch_size=20000, seed=2).sample(200, n_sim=100000)
    for k in ('t1', 't2', 't3'):
        assert np.array_equal(res2.samples[k], s[k])
    assert np.array_equal(res2.discrepancies, res.discrepancies)
    # the simulator feeds the synthetic likelihood: 500 simulations of the 50 log inter-departure times at the true point
    sims = m.generate(500, outputs=['log_identity'], with_values=dict(t1=1.0, t2=5.0, t3=0.2), seed=1)
    ssx = np.asarray(sims['log_identity'])
    assert ssx.shape == (500, 50)
    ll = elfi_amd.syn_loglik(ssx, np.ravel(m['log_identity'].observed))
    assert np.all(np.isfinite(ll))
    bsl = elfi_amd.HipBSL(elfi_amd.mg1_model(seed_obs=4), n_sim_round=200, feature_names=['log_identity'], seed=1)
    out = bsl.sample(20, sigma_proposals=np.diag([0.01, 0.05, 1e-5]), params0=[1.0, 5.0, 0.2], bar=False)
    assert type(out).__name__ == 'BslSample' and np.all(np.isfinite(bsl.state['logposterior']))
