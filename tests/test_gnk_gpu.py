"""GPU: the g-and-k example models on the device (csrc/gnk.hip, elfi_amd.gnk_summaries / bignk_summaries,
fused_models.gnk_model / bignk_model).

The series goes through the device's exp and pow, so it is held to ONE tolerance, in units u = eps (|A| + |y - A|) (the
sum A + term may cancel: an error relative to |y| is unbounded for any implementation, the error in this unit is not):
E_ref is the largest error of the reference's own series against 40-digit values over the golden block (recorded in
tests/golden/gnk.npz; 7.09 -- roundings amplified by a bracket 1 + 0.8 t as small as 0.2).  On the golden block the device
is within 2 E_ref of the 40-digit values (device functions of 1 to 2 ulp against glibc's below 1 ulp, through the same
amplification); on other draws within 3 E_ref of tests/gnk_ref.py evaluated by the NumPy at hand (the triangle of the
two errors).  NaN positions coincide exactly.  Everything after the series -- the order statistics, the octiles, the
robust statistics -- is NumPy's bit for bit on the device's own series; the fused distance is HipDistance's bit for bit and
within m eps D of the reference's euclidean_multiss (the same m non-negative terms in two orders).
"""
import ctypes as C
import os

import numpy as np
import pytest

import gnk_ref as R

pytestmark = pytest.mark.gpu

U64 = C.c_uint64
ALL = ('order', 'sorted', 'octile', 'robust')


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'gnk.npz'))


def _fn(dim):
    import elfi_amd
    return elfi_amd.gnk_summaries if dim == 1 else elfi_amd.bignk_summaries


def _case(n, n_obs, dim, seed):
    """Parameters over the models' prior ranges and draws as the reference holds them."""
    rs = np.random.RandomState(seed)
    if dim == 1:
        return rs.uniform(0, 10, (n, 4)), rs.standard_normal((n, n_obs))
    P = np.column_stack([rs.uniform(0, 5, (n, 4)), rs.uniform(-5, 5, (n, 2)), rs.uniform(-.5, 5, (n, 2)), rs.uniform(-1, 1, n)])
    return P, R.correlate(rs.standard_normal((n, n_obs, 2)), P[:, 8])


def _units(Y3, Yr, P):
    """max |Y3 - Yr| / (eps (|A| + |Yr - A|)) over the finite elements; the NaN positions must be the same."""
    assert np.array_equal(np.isnan(Y3), np.isnan(Yr))
    A = R.split_params(P)[0]
    ok = ~np.isnan(Yr)
    with np.errstate(all='ignore'):
        e = np.abs(Y3 - Yr) / (R.EPS * (np.abs(A) + np.abs(Yr - A)))
    return float(np.max(e[ok])) if ok.any() else 0.0


def _summaries_are_numpys(Y3, order, srt, octl, rob):
    """The four summaries against NumPy on the device's own series, bit for bit."""
    n, n_obs, dim = Y3.shape
    assert order.shape == srt.shape == (n, n_obs * dim) and octl.shape == (n, 7 * dim) and rob.shape == (n, 4 * dim)
    assert np.array_equal(order, R.flat(Y3), equal_nan=True)
    assert np.array_equal(srt, R.flat(np.sort(Y3, axis=1)), equal_nan=True)
    with np.errstate(all='ignore'):
        E = np.percentile(Y3, np.linspace(12.5, 87.5, 7), axis=1)          # (7, n, dim)
    assert np.array_equal(octl, np.hstack(list(E)), equal_nan=True)
    assert np.array_equal(octl, R.flat(R.ss_octile(Y3)), equal_nan=True)
    assert np.array_equal(rob, R.flat(R.ss_robust(Y3)), equal_nan=True)


# ---- 1. given draws ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,n_obs,dim', [(1, 50, 1), (777, 50, 1), (4097, 50, 1), (333, 37, 1), (64, 2, 1), (200, 130, 1),
                                         (70, 2048, 1), (1, 150, 2), (777, 150, 2), (333, 11, 2), (40, 1024, 2)])
def test_given_draws(hip_ctx, golden, n, n_obs, dim):
    E_ref = float(golden['E_ref'])
    P, z = _case(n, n_obs, dim, 17 * n + n_obs + dim)
    order, srt, octl, rob, Y3 = _fn(dim)(*P.T, n_obs=n_obs, z=z, summary=ALL, return_series=True)
    Y3 = Y3.reshape(n, n_obs, dim)
    err = _units(Y3, R.series(P, z), P)
    print('n=%d n_obs=%d dim=%d: series within %.2f units of NumPy (bound %.2f)' % (n, n_obs, dim, err, 3 * E_ref))
    assert err <= 3 * E_ref
    _summaries_are_numpys(Y3, order, srt, octl, rob)
    # a row does not depend on the batch or the grid: the first rows of this call are a smaller call
    k = min(n, 37)
    small = _fn(dim)(*P[:k].T, n_obs=n_obs, z=z[:k], summary=ALL, return_series=True)
    for a, b in zip((order, srt, octl, rob, Y3), small):
        assert np.array_equal(a[:k].reshape(b.shape), b, equal_nan=True)
    # one summary alone (no series output, no sort for 'order') is the same array
    assert np.array_equal(_fn(dim)(*P.T, n_obs=n_obs, z=z, summary='robust'), rob, equal_nan=True)
    assert np.array_equal(_fn(dim)(*P.T, n_obs=n_obs, z=z, summary='order'), order, equal_nan=True)


# ---- 2. the golden block -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('block,dim', [('gnk', 1), ('bignk', 2)])
def test_golden_block(hip_ctx, golden, block, dim):
    g = golden
    E_ref = float(g['E_ref'])
    P, z, y_ref = g[block + '_P'], g[block + '_z'], g[block + '_y']
    n, n_obs = z.shape[:2]
    order, srt, octl, rob, Y3 = _fn(dim)(*P.T, n_obs=n_obs, z=z, summary=ALL, return_series=True)
    Y3 = Y3.reshape(y_ref.shape)
    err = float(np.max(R.error_in_units(Y3, g[block + '_y_hi'], g[block + '_y_lo'], P)))
    print('%s: device series within %.2f units of the 40-digit values; E_ref %.2f, bound %.2f' % (block, err, E_ref, 2 * E_ref))
    assert err <= 2 * E_ref
    _summaries_are_numpys(Y3, order, srt, octl, rob)
    # the summaries move with the series only: those of the reference's series are close to the recorded ones
    assert np.allclose(octl, R.flat(g[block + '_octile']), rtol=1e-12, atol=1e-12)
    # the fused distance against the reference's euclidean_multiss on the same (device) summaries: m eps D
    for name, s in zip(ALL, (order, srt, octl, rob)):
        got = _fn(dim)(*P.T, n_obs=n_obs, z=z, summary=name, observed=s[0])
        assert len(got) == 2 and np.array_equal(got[0], s)
        D, m = got[1], s.shape[1]
        want = R.euclidean_multiss(s[:, :, None], s[:1, :, None])
        assert D[0] == 0 and np.all(np.abs(D - want) <= m * R.EPS * want)


# ---- 3. edge rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('block,dim', [('edge', 1), ('biedge', 2)])
def test_edge_rows(hip_ctx, golden, block, dim):
    g = golden
    E_ref = float(g['E_ref'])
    names = list(g[block + '_names'])
    P, z, y_ref = g[block + '_P'], g[block + '_z'], g[block + '_y']
    n, n_obs = z.shape[:2]
    order, srt, octl, rob, Y3 = _fn(dim)(*P.T, n_obs=n_obs, z=z, summary=ALL, return_series=True)
    Y3 = Y3.reshape(y_ref.shape)
    # NaNs exactly where the reference has them (an overflowing exp), the rest of every row within the bound
    assert np.isnan(y_ref).sum() in (2, 3) and _units(Y3, y_ref, P) <= 3 * E_ref
    _summaries_are_numpys(Y3, order, srt, octl, rob)
    # ... last after sorting; octiles, robust statistics and distances NaN where the reference's are, and nowhere else
    nan_cols = np.isnan(y_ref).sum(axis=1)                                   # (n, dim)
    S3 = srt.reshape(y_ref.shape)
    for i, d in np.argwhere(nan_cols > 0):
        assert np.isnan(S3[i, n_obs - nan_cols[i, d]:, d]).all() and np.isfinite(S3[i, :n_obs - nan_cols[i, d], d]).all()
    assert np.array_equal(np.isnan(octl), np.isnan(R.flat(g[block + '_octile'])))
    assert np.array_equal(np.isnan(rob), np.isnan(R.flat(g[block + '_robust'])))
    i = names.index('overflow' if dim == 1 else 'overflow_d0')
    assert np.isnan(rob[i]).any() and np.isfinite(np.delete(rob, i, axis=0)).all()
    recorded_order = R.order_from_swaps(y_ref, g[block + '_order_swaps'])
    for name, s in (('octile', g[block + '_octile']), ('robust', g[block + '_robust'])):
        D = _fn(dim)(*P.T, n_obs=n_obs, z=z, summary=name, observed=s[0])[1]
        assert np.array_equal(np.isnan(D), np.isnan(g[block + '_d_' + name])) and np.isnan(D[i])
        ok = ~np.isnan(D)
        assert np.allclose(D[ok], g[block + '_d_' + name][ok], rtol=1e-9, atol=1e-9)
    D = _fn(dim)(*P.T, n_obs=n_obs, z=z, summary='order', observed=y_ref[0])[1]
    assert np.array_equal(np.isnan(D), np.isnan(R.euclidean_multiss(y_ref, y_ref[:1]))) and np.isnan(D[i])
    if dim == 1:
        assert np.array_equal(recorded_order, y_ref, equal_nan=True)
        Y = Y3[:, :, 0]
        b = names.index('B0')                    # a constant series: ss_B = eps, ss_g = ss_k = 0, exactly the reference's row
        assert np.all(Y[b] == P[b, 0]) and np.array_equal(rob[b], [P[b, 0], R.EPS, 0.0, 0.0])
        assert np.array_equal(rob[b], g['edge_robust'][b, :, 0]) and np.array_equal(octl[b], g['edge_octile'][b, :, 0])
        zr = names.index('zero')                 # z = +-0: the element is A exactly
        assert Y[zr, 5] == P[zr, 0] and Y[zr, 6] == P[zr, 0]
        t = names.index('ties')                  # equal draws give equal values: the ties survive the device's exp and pow
        assert np.all(Y[t, :10] == Y[t, 0]) and np.all(Y[t, 20:24] == Y[t, 20])
        for name in ('g0', 'kneg', 'gneg', 'g400_finite'):
            assert np.isfinite(Y[names.index(name)]).all()
    else:
        p, m = names.index('rho_plus'), names.index('rho_minus')
        assert np.array_equal(z[p, :, 0], z[p, :, 1]) and np.array_equal(z[m, :, 0], -z[m, :, 1])
        assert np.isfinite(Y3[[p, m]]).all()


# ---- 4. the draws made in the kernel -------------------------------------------------------------------------------------
def _normals(hip_ctx, seed, stream, count):
    import torch
    d = torch.empty(count, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    assert hip_ctx.lib.elfihip_randn_dev(hip_ctx.handle, U64(seed), U64(stream), count, C.c_double(0.0), C.c_double(1.0),
                                         d.data_ptr()) == 0
    hip_ctx.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize('dim,n_obs', [(1, 50), (2, 150)])
@pytest.mark.parametrize('n', [1, 777, 50000])
def test_drawn_form(hip_ctx, n, dim, n_obs):
    seed, stream = 9876, 12
    P, _ = _case(n, 2, dim, n)
    if dim == 2:
        P[:, 8] = 0.6
    fn = _fn(dim)
    rob, Y, Zo = fn(*P.T, n_obs=n_obs, seed=seed, stream=stream, summary='robust', return_series=True, return_draws=True)
    e = _normals(hip_ctx, seed, stream, n * n_obs * dim)
    if dim == 1:
        assert Zo.shape == (n, n_obs) and np.array_equal(Zo, e.reshape(n, n_obs))
    else:
        e = e.reshape(n, n_obs, 2)
        assert Zo.shape == (n, n_obs, 2) and np.array_equal(Zo, R.correlate(e, P[:, 8]))
        if n == 50000:
            N = n * n_obs
            r = np.corrcoef(Zo[:, :, 0].reshape(-1), Zo[:, :, 1].reshape(-1))[0, 1]
            print('sample correlation over %d pairs: %.5f' % (N, r))
            assert abs(r - 0.6) <= 5 * (1 - 0.6 ** 2) / np.sqrt(N)
    del e
    # the given-draw form on these draws is the same computation
    rob2, Y2 = fn(*P.T, n_obs=n_obs, z=Zo, summary='robust', return_series=True)
    assert np.array_equal(Y, Y2, equal_nan=True) and np.array_equal(rob, rob2, equal_nan=True)
    # the same seed gives the same bits, another stream others
    again = fn(*P.T, n_obs=n_obs, seed=seed, stream=stream, summary='order', return_draws=True)
    assert np.array_equal(again[1], Zo) and np.array_equal(again[0], R.flat(Y), equal_nan=True)
    other = fn(*P.T, n_obs=n_obs, seed=seed, stream=stream + 1, summary='order', return_draws=True)[1]
    assert not np.any(other == Zo)


# ---- 5. device pointers at the caller's pitch ------------------------------------------------------------------------------
def _dev_call(hip_ctx, dim, n, n_obs, P, z, seed, stream, obs, which, pad):
    import torch
    from elfi_amd.summaries import GNK_OCTILES, quantile_positions
    L, npar = n_obs * dim, P.shape[1]
    lo, hi, t = [np.ascontiguousarray(a) for a in quantile_positions(np.true_divide(GNK_OCTILES, 100), n_obs)]
    dP = torch.full((n, npar + pad), np.nan, dtype=torch.float64, device='cuda')
    dP[:, :npar] = torch.from_numpy(P).cuda()
    dZ = None
    if z is not None:
        dZ = torch.full((n, L + pad), np.nan, dtype=torch.float64, device='cuda')
        dZ[:, :L] = torch.from_numpy(np.ascontiguousarray(z).reshape(n, L)).cuda()
    widths = [L, L, L, 7 * dim, 4 * dim]
    outs = [torch.full((n, w + pad), -7.0, dtype=torch.float64, device='cuda') for w in widths]
    dD = torch.full((n,), -7.0, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    args = [hip_ctx.handle, dZ.data_ptr() if dZ is not None else None, L + pad, U64(seed), U64(stream), n, n_obs, dim,
            dP.data_ptr(), npar + pad, C.c_double(0.8), lo.ctypes.data, hi.ctypes.data, t.ctypes.data, obs.ctypes.data, which]
    for o, w in zip(outs, widths):
        args += [o.data_ptr(), w + pad]
    rc = hip_ctx.lib.elfihip_gnk_summaries_dev(*args, dD.data_ptr())
    assert rc == 0, hip_ctx.lib.elfihip_last_error(hip_ctx.handle)
    hip_ctx.synchronize()
    res = []
    for o, w in zip(outs, widths):
        a = o.cpu().numpy()
        assert np.all(a[:, w:] == -7.0)                      # nothing written beyond a row
        res.append(a[:, :w])
    return res + [dD.cpu().numpy()]


@pytest.mark.parametrize('dim,n,n_obs', [(1, 203, 50), (2, 131, 37), (1, 20, 301)])
def test_dev_form_at_the_callers_pitch(hip_ctx, dim, n, n_obs):
    P, z = _case(n, n_obs, dim, 5 * n)
    fn = _fn(dim)
    for which, name in enumerate(ALL):
        rest = tuple(s for s in ALL if s != name)
        host = fn(*P.T, n_obs=n_obs, z=z, summary=(name,) + rest, return_series=True, return_draws=True, observed=None)
        by_name = dict(zip((name,) + rest, host[:4]))
        obs = np.ascontiguousarray(by_name[name][n // 2])
        D = fn(*P.T, n_obs=n_obs, z=z, summary=name, observed=obs)[1]
        want = [R.flat(host[4]), R.flat(host[5]), by_name['sorted'], by_name['octile'], by_name['robust'], D]
        for pad in (0, 5):
            got = _dev_call(hip_ctx, dim, n, n_obs, P, z, 0, 0, obs, which, pad)
            for a, b in zip(got, want):
                assert np.array_equal(a, b, equal_nan=True)
    # ... and with the draws made in the kernel
    obs0 = np.full(n_obs * dim, 0.5)
    host = fn(*P.T, n_obs=n_obs, seed=3, stream=4, summary=ALL, return_series=True, return_draws=True, observed=obs0)
    got = _dev_call(hip_ctx, dim, n, n_obs, P, None, 3, 4, obs0, 0, 3)
    want = [R.flat(host[4]), R.flat(host[5]), host[1], host[2], host[3], host[6]]
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=True)


# ---- 6. the fused distance is HipDistance's ---------------------------------------------------------------------------------
@pytest.mark.parametrize('dim,n_obs', [(1, 50), (1, 299), (1, 300), (1, 400), (2, 20), (2, 149), (2, 150), (2, 1024)])
def test_fused_distance_is_hipdistances(hip_ctx, dim, n_obs):
    """Rows of up to 299 values are summed left to right, longer ones by 64 lane-strided partial sums and a butterfly, in
    the fused kernel as in elfihip_dist_rows: both sides of that threshold, for each of the four rows."""
    import elfi_amd
    n = 333 if n_obs < 1000 else 45
    P, z = _case(n, n_obs, dim, 7 * n_obs + dim)
    fn = _fn(dim)
    for kw in (dict(z=z), dict(seed=5, stream=2)):
        outs = fn(*P.T, n_obs=n_obs, summary=ALL, **kw)
        for name, s in zip(ALL, outs):
            obs = s[n // 3] + 0.25
            got, D = fn(*P.T, n_obs=n_obs, summary=name, observed=obs, **kw)
            assert np.array_equal(got, s, equal_nan=True)
            assert np.array_equal(D, elfi_amd.HipDistance('euclidean')(s, obs[None]))
            want = R.euclidean_multiss(s[:, :, None], obs[None, :, None])
            assert np.all(np.abs(D - want) <= s.shape[1] * R.EPS * want)


# ---- 7. what the library refuses ---------------------------------------------------------------------------------------------
def test_library_refuses_what_it_cannot_hold(hip_ctx):
    import torch
    from elfi_amd import _lib
    lib, h = hip_ctx.lib, hip_ctx.handle
    buf = torch.zeros(3 * 8192, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    p = buf.data_ptr()
    out = [p + 8 * 8192 * i for i in (1, 2)]
    pos = np.zeros(7, dtype=np.int32)
    t = np.zeros(7)
    obs = np.zeros(4096)

    def call(n_obs, dim, ldp=9, ldy=None, observed=None, dD=None, ldo=14, which=3):
        ldy = n_obs * dim if ldy is None else ldy
        return lib.elfihip_gnk_summaries_dev(h, None, n_obs * dim, U64(1), U64(0), 2, n_obs, dim, p, ldp, C.c_double(0.8),
                                             pos.ctypes.data, pos.ctypes.data, t.ctypes.data, observed, which, out[0], ldy,
                                             None, 0, None, 0, out[1], ldo, None, 0, dD)
    assert call(1, 1) == _lib.ERR_ARG
    assert call(2049, 1) == _lib.ERR_ARG and b'2048' in lib.elfihip_last_error(h)
    assert call(1025, 2) == _lib.ERR_ARG
    assert call(50, 3) == _lib.ERR_ARG and call(50, 0) == _lib.ERR_ARG
    assert call(50, 1, ldy=49) == _lib.ERR_ARG and call(50, 2, ldy=99) == _lib.ERR_ARG
    assert call(50, 1, ldp=3) == _lib.ERR_ARG and call(50, 2, ldp=8) == _lib.ERR_ARG
    assert call(50, 2, ldo=13) == _lib.ERR_ARG
    assert call(50, 1, dD=out[1]) == _lib.ERR_ARG                                  # a distance without observed values
    assert call(50, 1, observed=obs.ctypes.data, dD=out[1], which=4) == _lib.ERR_ARG
    assert call(50, 1) == 0 and call(1024, 2) == 0 and call(2048, 1) == 0 and call(2, 2) == 0
    assert call(50, 1, observed=obs.ctypes.data, dD=p + 8 * 4096) == 0
    hip_ctx.synchronize()


# ---- 8. the models through ELFI's loops ---------------------------------------------------------------------------------------
def _reference():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi
    return elfi


@pytest.mark.parametrize('model,names', [('gnk_model', ['A', 'B', 'g', 'k']),
                                         ('bignk_model', ['a1', 'a2', 'b1', 'b2', 'g1', 'g2', 'k1', 'k2', 'rho'])])
def test_models_through_the_loops(hip_ctx, model, names):
    elfi = _reference()
    import elfi_amd
    m = getattr(elfi_amd, model)(seed=4)
    assert m.parameter_names == names
    res = elfi_amd.HipRejection(m['d'], batch_size=2000, seed=2).sample(100, n_sim=10000)
    assert res.samples[names[0]].shape == (100,) and np.all(np.isfinite(res.discrepancies))
    res2 = elfi.Rejection(m['d'], batch_size=2000, seed=2).sample(100, n_sim=10000)
    for k in names:
        assert np.array_equal(res2.samples[k], res.samples[k])
    assert np.array_equal(res2.discrepancies, res.discrepancies)
