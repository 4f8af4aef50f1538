"""GPU: the stochastic Lorenz-96 example model on the device (csrc/lorenz.hip, elfi_amd.lorenz_summaries,
fused_models.lorenz_model).

On given draws the device series and all six summaries equal the NumPy statement tests/lorenz_ref.py bit for bit (that
statement is pinned to ELFI's own example in tests/test_lorenz.py), non-finite values included.  The draws made in the
kernel are those elfihip_randn_dev writes, the fused distance is HipDistance's, the library refuses what it cannot hold,
and the model runs through ELFI's loops.
"""
import ctypes as C
import os

import numpy as np
import pytest

import lorenz_ref as R
from series_ref import weighted_euclidean

pytestmark = pytest.mark.gpu

U64, DBL = C.c_uint64, C.c_double
PHI, F = 0.984, 10.0


def _duration(T):
    """The example's step h = 4 / 160 at every length: short series stay finite (a step of 4 / 20 diverges)."""
    return T / 40


def _constants(T):
    return R.lorenz_constants(PHI, T, _duration(T))


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'lorenz.npz'))


_cases = {}


def _case(n, T, K):
    """Parameters, draws, initial states and the NumPy statement's series and summaries: computed once per shape."""
    if (n, T, K) not in _cases:
        rs = np.random.RandomState(7 * n + 1000 * T + K)
        t1, t2 = rs.uniform(0.5, 3.5, n), rs.uniform(0, 0.3, n)
        y0 = 3.0 * rs.randn(n, K)
        E = R.lorenz_noise_from_state(rs, n, T, K)
        c, h = _constants(T)
        X = R.lorenz_series(t1, t2, E, y0, F, c, PHI, h)
        case = dict(t1=t1, t2=t2, y0=y0, E=E, X=X, S=R.lorenz_summaries(X))
        assert np.all(np.isfinite(case['S']))
        for v in case.values():
            v.setflags(write=False)
        _cases[(n, T, K)] = case
    return _cases[(n, T, K)]


# ---- 1. given draws: series and summaries are the NumPy statement's ----------------------------------------------------
# 1 x 160 x 40: the example's shape; 65 x 20 x 8 and 257 x 3 x 5: more simulations than one pass of a small grid, an odd
# number of variables; 3 x 2 x 4: a single step, means of one term, the in-order branch of the sum, k - 2 = k + 2;
# 4 x 128 x 64: a full wavefront at the 8192 terms of NumPy's buffer; 5 x 33 x 4: 132 terms, one split
@pytest.mark.parametrize('n,T,K', [(1, 160, 40), (65, 20, 8), (257, 3, 5), (3, 2, 4), (4, 128, 64), (5, 33, 4)])
def test_lorenz_on_given_draws_is_numpys(hip_ctx, n, T, K):
    import elfi_amd
    g = _case(n, T, K)
    kw = dict(f=F, phi=PHI, n_obs=K, n_timestep=T, total_duration=_duration(T), noise=g['E'])
    S, X = elfi_amd.lorenz_summaries(g['t1'], g['t2'], g['y0'], return_series=True, **kw)
    assert S.shape == (n, 6) and X.shape == (n, T, K)
    assert np.array_equal(X, g['X'], equal_nan=True)
    assert np.array_equal(S, g['S'], equal_nan=True)
    # without the series output the summaries are the same
    assert np.array_equal(elfi_amd.lorenz_summaries(g['t1'], g['t2'], g['y0'], **kw), g['S'], equal_nan=True)


def test_lorenz_golden_blocks(hip_ctx, golden):
    """2 x 160 x 40 from the example's own initial state (one shared row) and 16 x 20 x 8 with a row per simulation: the
    reference's recorded series and summaries."""
    import elfi_amd
    g = golden
    E = R.lorenz_noise_from_state(np.random.RandomState(int(g['default_seed'])), 2, 160, 40)
    S, X = elfi_amd.lorenz_summaries(g['default_t1'], g['default_t2'], g['y0_default'], noise=E, return_series=True)
    assert np.array_equal(X, g['default_X']) and np.array_equal(S, g['default_S'])
    assert np.array_equal(elfi_amd.lorenz_summaries(g['default_t1'], g['default_t2'], g['y0_default'], noise=E), g['default_S'])
    Es = R.lorenz_noise_from_state(np.random.RandomState(int(g['small_seed'])), 16, 20, 8)
    S, X = elfi_amd.lorenz_summaries(g['small_t1'], g['small_t2'], g['small_y0'], n_obs=8, n_timestep=20, noise=Es,
                                     return_series=True)
    assert np.array_equal(X, g['small_X']) and np.array_equal(S, g['small_S'])


def test_shared_and_per_simulation_initial_state(hip_ctx):
    import elfi_amd
    g = _case(65, 20, 8)
    c, h = _constants(20)
    shared = g['y0'][3]
    Xr = R.lorenz_series(g['t1'], g['t2'], g['E'], shared, F, c, PHI, h)
    kw = dict(n_obs=8, n_timestep=20, total_duration=_duration(20), noise=g['E'], return_series=True)
    S, X = elfi_amd.lorenz_summaries(g['t1'], g['t2'], shared, **kw)
    assert np.array_equal(X, Xr) and np.array_equal(S, R.lorenz_summaries(Xr))
    S2, X2 = elfi_amd.lorenz_summaries(g['t1'], g['t2'], np.tile(shared, (65, 1)), **kw)
    assert np.array_equal(X2, X) and np.array_equal(S2, S)
    assert not np.array_equal(X, g['X'])                  # ... and the rows of a (n, K) state are each simulation's own


def test_overflowing_simulation_gives_the_same_non_finite_values(hip_ctx):
    """theta2 = -5 turns the damping term into growth: the reference's series overflows within the 160 rows."""
    import elfi_amd
    n, T, K = 3, 160, 40
    rs = np.random.RandomState(9)
    t1, t2 = np.array([2.0, 2.0, 2.0]), np.array([0.1, -5.0, 0.1])
    y0 = 3.0 * rs.randn(K)
    E = R.lorenz_noise_from_state(rs, n, T, K)
    c, h = _constants(T)
    Xr = R.lorenz_series(t1, t2, E, y0, F, c, PHI, h)
    Sr = R.lorenz_summaries(Xr)
    assert not np.any(np.isfinite(Sr[1])) and not np.all(np.isfinite(Xr[1])) and np.all(np.isfinite(Sr[[0, 2]]))
    S, X = elfi_amd.lorenz_summaries(t1, t2, y0, noise=E, return_series=True)
    assert np.array_equal(X, Xr, equal_nan=True) and np.array_equal(np.isnan(X), np.isnan(Xr))
    assert np.array_equal(S, Sr, equal_nan=True)
    assert np.array_equal(elfi_amd.lorenz_summaries(t1, t2, y0, noise=E), Sr, equal_nan=True)


# ---- 2. the device-pointer form ---------------------------------------------------------------------------------------
def _lorenz_dev(hip_ctx, dE, ldE, seed, stream, n, T, K, t1, t2, y0, obs, pad=0):
    import torch
    c, h = _constants(T)
    dt1, dt2 = torch.from_numpy(np.ascontiguousarray(t1)).cuda(), torch.from_numpy(np.ascontiguousarray(t2)).cuda()
    y0 = np.asarray(y0)
    if y0.ndim == 2:
        dy0 = torch.full((n, K + pad), np.nan, dtype=torch.float64, device='cuda')
        dy0[:, :K] = torch.from_numpy(np.ascontiguousarray(y0)).cuda()
        ldy0 = K + pad
    else:
        dy0, ldy0 = torch.from_numpy(np.ascontiguousarray(y0)).cuda(), 0
    dS = torch.full((n, 6 + pad), -7.0, dtype=torch.float64, device='cuda')
    dY = torch.full((n, T * K + pad), -7.0, dtype=torch.float64, device='cuda')
    dD = torch.empty(n, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    rc = hip_ctx.lib.elfihip_lorenz_summaries_dev(hip_ctx.handle, dE, ldE, U64(seed), U64(stream), n, K, T, dt1.data_ptr(),
                                                  dt2.data_ptr(), DBL(F), DBL(c), DBL(PHI), DBL(h), dy0.data_ptr(), ldy0,
                                                  obs.ctypes.data, dS.data_ptr(), 6 + pad, dY.data_ptr(), T * K + pad,
                                                  dD.data_ptr())
    assert rc == 0, hip_ctx.lib.elfihip_last_error(hip_ctx.handle)
    hip_ctx.synchronize()
    S, Y = dS.cpu().numpy(), dY.cpu().numpy()
    assert np.all(S[:, 6:] == -7.0) and np.all(Y[:, T * K:] == -7.0)      # nothing written beyond a row
    return S[:, :6], Y[:, :T * K].reshape(n, T, K), dD.cpu().numpy()


@pytest.mark.parametrize('n,T,K', [(1, 160, 40), (300, 20, 8), (77, 6, 5)])
def test_lorenz_drawn_is_materialised(hip_ctx, n, T, K):
    """The draws made in the kernel are the normals elfihip_randn_dev writes for the same (seed, stream); the caller's
    pitches for E, S, Y and the initial states are respected and the padding stays untouched."""
    import torch
    seed, stream = 4321, 9
    L = (T - 1) * K
    rs = np.random.RandomState(n + T)
    t1, t2, obs = rs.uniform(0.5, 3.5, n), rs.uniform(0, 0.3, n), rs.randn(6)
    y0 = 3.0 * rs.randn(n, K)
    dE = torch.empty(n * L, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    assert hip_ctx.lib.elfihip_randn_dev(hip_ctx.handle, U64(seed), U64(stream), n * L, DBL(0.0), DBL(1.0), dE.data_ptr()) == 0
    hip_ctx.synchronize()
    given = _lorenz_dev(hip_ctx, dE.data_ptr(), L, 0, 0, n, T, K, t1, t2, y0, obs)
    drawn = _lorenz_dev(hip_ctx, None, L, seed, stream, n, T, K, t1, t2, y0, obs)
    for a, b in zip(given, drawn):
        assert np.array_equal(a, b)
    E = dE.cpu().numpy().reshape(n, T - 1, K)
    c, h = _constants(T)
    Xr = R.lorenz_series(t1, t2, E, y0, F, c, PHI, h)
    assert np.all(np.isfinite(Xr))
    assert np.array_equal(given[1], Xr) and np.array_equal(given[0], R.lorenz_summaries(Xr))
    # the caller's pitch: rows of E, S, Y and y0 further apart than their length
    dEp = torch.full((n, L + 5), np.nan, dtype=torch.float64, device='cuda')
    dEp[:, :L] = dE.view(n, L)
    torch.cuda.synchronize()
    pitched = _lorenz_dev(hip_ctx, dEp.data_ptr(), L + 5, 0, 0, n, T, K, t1, t2, y0, obs, pad=3)
    for a, b in zip(given, pitched):
        assert np.array_equal(a, b)
    # a different seed, a different stream: different draws
    for sd, st in ((seed + 1, stream), (seed, stream + 1)):
        other = _lorenz_dev(hip_ctx, None, L, sd, st, n, T, K, t1, t2, y0, obs)
        assert not np.any(other[1][:, 1:] == drawn[1][:, 1:])
    # the host form draws the same stream
    import elfi_amd
    S, X = elfi_amd.lorenz_summaries(t1, t2, y0, n_obs=K, n_timestep=T, total_duration=_duration(T), seed=seed, stream=stream,
                                     return_series=True)
    assert np.array_equal(X, drawn[1]) and np.array_equal(S, drawn[0])


def test_fused_distance_is_hipdistances(hip_ctx):
    import elfi_amd
    g = _case(65, 20, 8)
    obs = g['S'][0] + 0.25
    for kw in (dict(noise=g['E']), dict(seed=5, stream=2)):
        S, D = elfi_amd.lorenz_summaries(g['t1'], g['t2'], g['y0'], n_obs=8, n_timestep=20, total_duration=_duration(20),
                                         observed=obs, **kw)
        assert np.array_equal(D, elfi_amd.HipDistance('euclidean')(S, obs[None]))
        assert np.array_equal(D, weighted_euclidean(S, obs))
    assert np.array_equal(S.shape, (65, 6)) and np.all(D > 0)


def test_library_refuses_what_it_cannot_hold(hip_ctx):
    """Past the Python checks: every shape outside 4 <= n_obs <= 64, n_timestep >= 2, n_timestep n_obs <= 8192, a pitch
    below the row length and a distance without observed values are argument errors of the C entry points, and nothing
    is written."""
    import torch
    from elfi_amd import _lib
    lib, h = hip_ctx.lib, hip_ctx.handle
    par = torch.ones(128, dtype=torch.float64, device='cuda')
    out = torch.full((2 * 8192 + 64,), -7.0, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    p, obs6 = par.data_ptr(), np.zeros(6)
    dS, dD, dY = out.data_ptr(), out.data_ptr() + 8 * 16, out.data_ptr() + 8 * 32

    def dev(K, T, ldE=None, lds=6, ldy=None, ldy0=0, observed=obs6.ctypes.data, D=dD, E=None):
        return lib.elfihip_lorenz_summaries_dev(h, E, (T - 1) * K if ldE is None else ldE, U64(1), U64(0), 2, K, T, p, p,
                                                DBL(F), DBL(0.178), DBL(PHI), DBL(0.025), p, ldy0, observed, dS, lds, dY,
                                                T * K if ldy is None else ldy, D)

    def host(K, T, observed=obs6.ctypes.data, with_D=True):
        S, D, t, y0 = np.full((2, 6), -7.0), np.full(2, -7.0), np.ones(2), np.ones(64)
        rc = lib.elfihip_lorenz_summaries(h, None, U64(1), U64(0), 2, K, T, t.ctypes.data, t.ctypes.data, DBL(F), DBL(0.178),
                                          DBL(PHI), DBL(0.025), y0.ctypes.data, 0, observed, S.ctypes.data, None,
                                          D.ctypes.data if with_D else None)
        assert rc == 0 or (np.all(S == -7.0) and np.all(D == -7.0))
        return rc
    for K, T in [(3, 10), (65, 10), (0, 10), (-1, 10), (40, 1), (40, 0), (40, -3), (40, 205), (64, 129), (4, 2049),
                 (8, 2 ** 28 + 1)]:
        assert dev(K, T) == _lib.ERR_ARG, (K, T)
        assert host(K, T) == _lib.ERR_ARG, (K, T)
    assert b'8192' in lib.elfihip_last_error(h)
    assert dev(40, 160, observed=None) == _lib.ERR_ARG and host(40, 160, observed=None) == _lib.ERR_ARG
    assert dev(40, 160, E=p, ldE=159 * 40 - 1) == _lib.ERR_ARG        # pitches below the row length
    assert dev(40, 160, lds=5) == _lib.ERR_ARG and dev(40, 160, ldy=160 * 40 - 1) == _lib.ERR_ARG
    assert dev(40, 160, ldy0=39) == _lib.ERR_ARG
    hip_ctx.synchronize()
    assert bool(torch.all(out == -7.0))                               # no refused call wrote anything
    assert dev(40, 160) == 0 and dev(64, 128) == 0 and dev(4, 2048) == 0 and dev(4, 2) == 0
    assert dev(40, 160, observed=None, D=None) == 0 and host(40, 160) == 0 and host(40, 160, None, False) == 0
    hip_ctx.synchronize()
    assert bool(torch.all(out[6:12] != -7.0)) and bool(torch.all(out[12:16] == -7.0))


# ---- 3. the model through ELFI's loops ----------------------------------------------------------------------------------
def _reference():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi
    return elfi


def test_lorenz_model_through_the_loops(hip_ctx, golden):
    """HipRejection and elfi.Rejection over the fused model give identical samples; the posterior means lie within four
    standard errors of a 200-sample mean of the centre the reference's own get_model(seed_obs=4) gave under elfi.Rejection
    with the same settings (tests/golden/lorenz.npz: a different random realisation of the same run)."""
    elfi = _reference()
    import elfi_amd
    g = golden
    seed_obs, batch, seed, n_samples, n_sim = [int(v) for v in g['e2e_settings']]
    m = elfi_amd.lorenz_model(seed_obs=seed_obs)
    assert all(name in m.nodes for name in ['theta1', 'theta2', 'Lorenz', 'd'] + R.NAMES)
    assert m.parameter_names == ['theta1', 'theta2']
    assert np.array_equal(np.ravel(m['Lorenz'].observed), g['e2e_obs'])
    res = elfi_amd.HipRejection(m['d'], batch_size=batch, seed=seed).sample(n_samples, n_sim=n_sim)
    t1, t2 = res.samples['theta1'], res.samples['theta2']
    assert t1.shape == (n_samples,) and np.all(np.isfinite(res.discrepancies))
    print('Lorenz posterior means', np.mean(t1), np.mean(t2), 'centre', g['e2e_centre'], 'margin', g['e2e_margin'])
    assert abs(np.mean(t1) - g['e2e_centre'][0]) < g['e2e_margin'][0]
    assert abs(np.mean(t2) - g['e2e_centre'][1]) < g['e2e_margin'][1]
    res2 = elfi.Rejection(m['d'], batch_size=batch, seed=seed).sample(n_samples, n_sim=n_sim)
    assert np.array_equal(res2.samples['theta1'], t1) and np.array_equal(res2.samples['theta2'], t2)
    assert np.array_equal(res2.discrepancies, res.discrepancies)
    # an explicit initial state reaches both the observed series and the simulator
    m2 = elfi_amd.lorenz_model(seed_obs=seed_obs, initial_state=g['y0_default'])
    assert np.array_equal(np.ravel(m2['Lorenz'].observed), g['e2e_obs'])
