"""GPU: the AR(1) model of csrc/series.hip (ar1_kernel) against its NumPy statement (tests/ar1_ref.py), which
tests/test_ar1.py pins to recorded runs of ELFI's own example: the series bit for bit on given noise, the distance bit for bit
elfi_amd's row distance on the series, the drawn form the given form on the normals elfihip_randn_dev writes, the _dev form at
the caller's pitch and in stream order, the model through ELFI."""
import ctypes as C
import faulthandler
import os

import numpy as np
import pytest

import ar1_ref as A
import stream_order as SO

pytestmark = pytest.mark.gpu
U64 = C.c_uint64
PHIS = np.array([0.0, 0.9, -1.0, 1.5, np.nan])


@pytest.fixture(autouse=True)
def time_limit():
    """A hung kernel ends the run instead of holding the device: the process exits after 120 s in one test."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def device_normals(hip_ctx, seed, stream, count):
    import torch
    t = torch.empty(count + (count & 1), dtype=torch.float64, device='cuda')
    hip_ctx.call('elfihip_randn_dev', U64(seed), U64(stream), t.numel(), C.c_double(0.0), C.c_double(1.0), t.data_ptr())
    hip_ctx.synchronize()
    return t.cpu().numpy()[:count]


@pytest.mark.parametrize('n_obs', [1, 2, 200, 2048])
@pytest.mark.parametrize('n', [1, 63, 65, 130])
def test_given_noise_is_the_statement(hip_ctx, n, n_obs):
    import elfi_amd
    rs = np.random.RandomState(n * 7 + n_obs)
    phi = PHIS[(np.arange(n) + n_obs) % len(PHIS)]
    W = rs.randn(n, n_obs + 1)
    obs = rs.randn(n_obs)
    want = A.series(phi, W)
    X, D = elfi_amd.ar1_series(phi, n_obs=n_obs, noise=W, observed=obs)
    assert X.shape == (n, n_obs) and X.dtype == np.float64 and np.array_equal(X, want, equal_nan=True)
    if n_obs == 2048 and n > 3:
        assert np.isinf(X[phi == 1.5, -1]).all() and np.isfinite(X[phi == 0.9]).all()      # 1.5^2048 overflows
    assert np.isnan(X[np.isnan(phi)]).all()
    dist = elfi_amd.HipDistance('euclidean')(X, obs[None, :])
    assert D.shape == (n,) and np.array_equal(D, dist, equal_nan=True)
    fine = np.isfinite(X).all(axis=1)
    ref = np.sqrt(np.sum((X[fine] - obs) ** 2, axis=1))
    assert np.all(np.abs(D[fine] - ref) <= 1e-13 * ref)
    assert np.array_equal(elfi_amd.ar1_series(phi, n_obs=n_obs, noise=W), X, equal_nan=True)     # the series alone


@pytest.mark.parametrize('n,n_obs', [(1, 1), (3, 2), (65, 200), (130, 201), (5, 2048)])
def test_drawn_form_is_the_given_form_on_the_device_normals(hip_ctx, n, n_obs):
    import elfi_amd
    phi = np.random.RandomState(n_obs).uniform(-1, 1, n)
    obs = np.random.RandomState(n).randn(n_obs)
    W = device_normals(hip_ctx, 21, 4, n * (n_obs + 1)).reshape(n, n_obs + 1)
    X, D = elfi_amd.ar1_series(phi, n_obs=n_obs, seed=21, stream=4, observed=obs)
    Xg, Dg = elfi_amd.ar1_series(phi, n_obs=n_obs, noise=W, observed=obs)
    assert np.array_equal(X, Xg) and np.array_equal(D, Dg) and np.array_equal(X, A.series(phi, W))
    assert not np.array_equal(elfi_amd.ar1_series(phi, n_obs=n_obs, seed=21, stream=5), X)


def _dev_inputs(which):
    n, n_obs = 70 + which, (200, 301)[which]
    rs = np.random.RandomState(800 + which)
    return n, n_obs, rs.uniform(-1, 1, n), rs.randn(n, n_obs + 1), rs.randn(n_obs)


def test_dev_form_at_the_callers_pitch(hip_ctx):
    import torch
    import elfi_amd
    lib, h = hip_ctx.lib, hip_ctx.handle
    pad, guard = 3, -7.0625e300
    for which in (0, 1):
        n, n_obs, phi, W, obs = _dev_inputs(which)
        ldw, ldx = n_obs + 1 + pad, n_obs + pad
        Wp = np.full((n, ldw), np.nan)
        Wp[:, :n_obs + 1] = W
        dphi, dW = torch.from_numpy(phi).cuda(), torch.from_numpy(Wp).cuda()
        for given in (True, False):
            want = elfi_amd.ar1_series(phi, n_obs=n_obs, noise=W if given else None, seed=6, stream=1, observed=obs)
            dX = torch.full((2 + n * ldx + 2,), guard, dtype=torch.float64, device='cuda')
            dD = torch.full((n + 2,), guard, dtype=torch.float64, device='cuda')
            torch.cuda.synchronize()
            rc = lib.elfihip_ar1_series_dev(h, dW.data_ptr() if given else None, ldw, U64(6), U64(1), n, n_obs, dphi.data_ptr(),
                                            obs.ctypes.data, dX.data_ptr() + 16, ldx, dD.data_ptr())
            assert rc == 0, lib.elfihip_last_error(h)
            hip_ctx.synchronize()
            X, D = dX.cpu().numpy(), dD.cpu().numpy()
            rows = X[2:2 + n * ldx].reshape(n, ldx)
            assert np.all(X[:2] == guard) and np.all(X[2 + n * ldx:] == guard) and np.all(rows[:, n_obs:] == guard)
            assert np.all(D[n:] == guard) and np.array_equal(rows[:, :n_obs], want[0]) and np.array_equal(D[:n], want[1])
    p = dX.data_ptr()
    for args in ((None, 0, 0, 0, -1, 5, p, None, p, 5, None), (None, 0, 0, 0, 2, 0, p, None, p, 5, None),
                 (None, 0, 0, 0, 2, 2049, p, None, p, 2049, None), (None, 0, 0, 0, 2, 5, p, None, p, 4, None),
                 (p, 5, 0, 0, 2, 5, p, None, p, 5, None), (None, 0, 0, 0, 2, 5, None, None, p, 5, None),
                 (None, 0, 0, 0, 2, 5, p, None, p, 5, p)):
        a = list(args)
        a[2], a[3] = U64(a[2]), U64(a[3])
        assert lib.elfihip_ar1_series_dev(h, *a) != 0, args
    hip_ctx.synchronize()


def _ar1_case(drawn):
    def case(d):
        issues = []
        for which in (0, 1):
            n, n_obs, phi, W, obs = _dev_inputs(which)
            issues.append((which, n, n_obs, None if drawn else d.input(W), d.input(phi), d.host(obs), d.out(n, n_obs), d.out(n)))
        d.go()
        for which, n, n_obs, W, phi, obs, X, D in issues:
            d.call('elfihip_ar1_series_dev', d.cx, W.ptr if W else None, n_obs + 1, U64(3 + which), U64(which), n, n_obs, phi.ptr,
                   obs.ctypes.data, X.ptr, n_obs, D.ptr, host=(obs,))
        d.done()
    return case


@pytest.mark.parametrize('name,case', [('ar1 given', _ar1_case(False)), ('ar1 drawn', _ar1_case(True))], ids=['given', 'drawn'])
def test_dev_entry_point_in_stream_order(hip_ctx, name, case):
    ref, got, d = SO.run_both(hip_ctx, case, name)
    SO.guards_intact(ref, d.guarded)
    SO.guards_intact(got, d.guarded)
    SO.assert_same(ref, got, name)
    assert d.still_busy, '%s: the stream was idle when the last call had returned: a call waited for the stream on the host' % name


def test_model_through_elfi(hip_ctx):
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi
    import elfi_amd
    m = elfi_amd.ar1_model(seed_obs=1)
    out = m.generate(4, outputs=['phi', 'AR1', 'd'], seed=2)
    assert out['AR1'].shape == (4, 200) and out['d'].shape == (4,) and np.all((out['phi'] >= -1) & (out['phi'] <= 1))
    want = np.sqrt(np.sum((out['AR1'] - m['AR1'].observed) ** 2, axis=1))
    assert np.all(np.abs(out['d'] - want) <= 1e-13 * want)
    res = elfi.Rejection(m['d'], batch_size=64, seed=1).sample(8, n_sim=192)
    assert res.samples['phi'].shape == (8,) and np.isfinite(res.threshold) and np.all(np.isfinite(res.discrepancies))
    res = elfi_amd.HipRejection(m['d'], batch_size=64, seed=1).sample(8, n_sim=128)
    assert res.samples['phi'].shape == (8,) and np.isfinite(res.threshold)
