"""GPU: the stochastic Lotka-Volterra example on the device (csrc/gillespie.hip, elfi_amd.lotka_volterra_summaries,
fused_models.lotka_volterra_model).

On given draws the device equals the NumPy statement (tests/lv_ref.py, itself held to ELFI's example in
tests/test_lotka_volterra.py) bit for bit: observations, status, event counts, final times -- no device transcendental is
involved.  The summaries are NumPy's bit for bit on the device's observations, the two log-variances within 4 ulp of np.log
on the same argument; the distance is the distance kernels' euclidean on the device's summaries.  The drawn form is the given
form on the draws elfihip_lv_draws materialises; its exponentials are within 4 ulp of the statement's, its uniforms and its
jump chain are the statement's, its observations the statement's outside the boundary mask.  A simulation does not depend
on the batch, the index it is given by or max_events.
"""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import lv_ref as L

pytestmark = pytest.mark.gpu

U64 = C.c_uint64
EXACT = [0, 1, 4, 5, 6, 7, 8]        # every summary but the two log-variances
OBS = np.array([170., 180., 8.9, 9.8, 0.8, 0.85, 0.55, 0.6, 0.1])


@pytest.fixture(autouse=True)
def time_limit():
    """A hung kernel ends the run instead of holding the device: the process exits after 120 s in one test."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _prior_draws(n, rs, noisy):
    p = [np.exp(rs.uniform(-6, 2, n)) for _ in range(3)] + [rs.normal(50, np.sqrt(50), n), rs.normal(100, 10, n)]
    if noisy:
        p.append(np.exp(rs.uniform(np.log(0.5), np.log(50), n)))
    return p


PLANTED = [dict(pred=0.5), dict(prey=0.3, pred=0.9), dict(r1=np.exp(2.), r2=np.exp(-6.)), dict(r1=np.nan), dict(sigma=-1.)]
KEYS = ['r1', 'r2', 'r3', 'prey', 'pred', 'sigma']


def _plant(p, row, what):
    for k, v in what.items():
        if KEYS.index(k) < len(p):
            p[KEYS.index(k)][row] = v


def _ulp(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    ok = np.isfinite(want)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - want[ok]) / np.spacing(np.abs(want[ok]))))


def _check_summaries(S, D, Y):
    """S against NumPy on the device's own observations, D against the distance kernel on the device's own S."""
    import elfi_amd
    want = L.summaries(Y)
    assert np.array_equal(np.isnan(S), np.isnan(want))
    assert np.array_equal(S[:, EXACT], want[:, EXACT], equal_nan=True)
    with np.errstate(all='ignore'):
        ulp = _ulp(S[:, 2:4], np.log(L.log_arguments(Y)))
    print('largest log-variance distance %.2f ulp' % ulp)
    assert ulp <= 4
    assert np.array_equal(D, elfi_amd.HipDistance('euclidean')(S, OBS[None, :]), equal_nan=True)
    return ulp


def _given(p, E, U, Z, n_obs, time_end):
    import elfi_amd
    noisy = len(p) == 6
    S, Y, status, events, T, D = elfi_amd.lotka_volterra_summaries(
        *p[:5], sigma=p[5] if noisy else None, n_obs=n_obs, time_end=time_end, draws=(E, U), noise=Z if noisy else None,
        observed=OBS, return_series=True, return_status=True)
    want = L.simulate(*p[:5], p[5] if noisy else None, E, U, Z, n_obs, time_end)
    assert Y.shape == want[0].shape and status.dtype == np.int32 and events.dtype == np.int64
    assert np.array_equal(Y, want[0], equal_nan=True)
    assert np.array_equal(T, want[1], equal_nan=True)
    assert np.array_equal(status, want[2]) and np.array_equal(events, want[3])
    _check_summaries(S, D, Y)
    assert np.all(np.isnan(S[status >= L.OUT_OF_EVENTS])) and np.all(np.isnan(D[status >= L.OUT_OF_EVENTS]))
    return status, events


# ---- 1. given draws --------------------------------------------------------------------------------------------------
EXPECTED = [L.EXTINCT, L.EXTINCT, L.OUT_OF_EVENTS, L.INVALID, L.INVALID]      # of the PLANTED rows, the last with sigma only


# (70, 129) and (9, 2048): the summary kernel's form for more than 128 observations (NumPy's recursive pairwise sum), the
# second at the largest n_obs the library takes
@pytest.mark.parametrize('n,n_obs', [(1, 3), (63, 16), (65, 16), (777, 50), (4097, 7), (70, 129), (9, 2048)])
def test_given_form_is_the_statement(hip_ctx, n, n_obs):
    import elfi_amd
    n_events, time_end = 300, 2.
    for noisy in (False, True):
        rs = np.random.RandomState(31 * n + n_obs + noisy)
        if n == 1:          # one simulation per call: an ordinary one, then each planted row alone
            cases = [{}] + PLANTED
        else:               # the planted rows spread over the batch, wavefront boundaries included
            cases = [None]
        for c, what in enumerate(cases):
            p = _prior_draws(n, rs, noisy)
            E, U, Z = rs.exponential(size=(n, n_events)), rs.uniform(size=(n, n_events)), rs.randn(n, 2 * (n_obs - 1))
            if what is None:
                rows = np.linspace(0, n - 1, len(PLANTED)).astype(int)
                for row, w in zip(rows, PLANTED):
                    _plant(p, row, w)
            else:
                rows = [0] if what else []
                _plant(p, 0, what)
            status, events = _given(p, E, U, Z, n_obs, time_end)
            expected = EXPECTED if what is None else EXPECTED[c - 1:c]
            for row, w, st in zip(rows, PLANTED if what is None else [what], expected):
                if 'sigma' in w and not noisy:
                    continue            # nothing was planted: the model without noise has no sigma
                assert status[row] == st
                assert events[row] == {L.EXTINCT: 1, L.OUT_OF_EVENTS: n_events, L.INVALID: 0}[st]
            if n >= 63:
                assert (status == L.REACHED_END).any()
        if n_obs > 128:     # the same summaries when the caller keeps no observations (they go to the context's buffer)
            kw = dict(sigma=p[5] if noisy else None, noise=Z if noisy else None, n_obs=n_obs, time_end=time_end, draws=(E, U))
            S = elfi_amd.lotka_volterra_summaries(*p[:5], **kw)
            full = elfi_amd.lotka_volterra_summaries(*p[:5], return_series=True, **kw)
            assert np.array_equal(S, full[0], equal_nan=True) and np.isfinite(S).any()


def test_long_lanes_next_to_refilled_ones(hip_ctx):
    """64 simulations at the example's true parameters up to time 30: about 10 000 events each."""
    n, n_obs, n_events = 64, 16, 16384
    rs = np.random.RandomState(99)
    p = [np.full(n, v) for v in (1.0, 0.005, 0.6, 50., 100.)]
    for row, w in zip([3, 17, 33, 40], PLANTED[:4]):
        _plant(p, row, w)
    E, U = rs.exponential(size=(n, n_events)), rs.uniform(size=(n, n_events))
    status, events = _given(p, E, U, None, n_obs, 30.)
    print('events: median %d, max %d' % (np.median(events), events.max()))
    assert np.median(events) > 5000 and status[33] == L.OUT_OF_EVENTS


# ---- 2. draws made in the kernel ----------------------------------------------------------------------------------------
def _normals(hip_ctx, seed, stream, count):
    import torch
    dz = torch.empty(count, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    assert hip_ctx.lib.elfihip_randn_dev(hip_ctx.handle, U64(seed), U64(stream), count, C.c_double(0.0), C.c_double(1.0),
                                         dz.data_ptr()) == 0
    hip_ctx.synchronize()
    return dz.cpu().numpy()


@pytest.mark.parametrize('noisy', [False, True])
def test_drawn_form(hip_ctx, noisy):
    import elfi_amd
    n, n_obs, time_end, n_events, seed, stream = 777, 16, 2., 400, 4321, 6
    p = _prior_draws(n, np.random.RandomState(7 + noisy), noisy)
    sigma = p[5] if noisy else None
    kw = dict(n_obs=n_obs, time_end=time_end, observed=OBS, return_series=True, return_status=True)
    drawn = elfi_amd.lotka_volterra_summaries(*p[:5], sigma=sigma, max_events=n_events, seed=seed, stream=stream, **kw)
    E, U = elfi_amd.lotka_volterra_draws(n, n_events, seed=seed, stream=stream)
    Z = _normals(hip_ctx, seed, stream + 1, n * 2 * (n_obs - 1)).reshape(n, -1) if noisy else None
    # the drawn form is the given form on the materialised draws, and the statement on them
    given = elfi_amd.lotka_volterra_summaries(*p[:5], sigma=sigma, draws=(E, U), noise=Z, **kw)
    for a, b in zip(drawn, given):
        assert np.array_equal(a, b, equal_nan=True)
    S, Y, status, events, T, D = drawn
    on_dev = L.simulate(*p[:5], sigma, E, U, Z, n_obs, time_end, return_chain=True)
    assert np.array_equal(Y, on_dev[0], equal_nan=True) and np.array_equal(T, on_dev[1], equal_nan=True)
    assert np.array_equal(status, on_dev[2]) and np.array_equal(events, on_dev[3])
    _check_summaries(S, D, Y)
    # the draws against the statement's: uniforms bit for bit, exponentials within 4 ulp
    Er, Ur, _ = L.draws(seed, stream, n, n_events)
    assert np.array_equal(U, Ur)
    ulp = _ulp(E, Er)
    print('largest exponential distance %.2f ulp' % ulp)
    assert ulp <= 4 and np.array_equal(E == 0, Er == 0)
    # the statement on its own exponentials: the same jump chain, the same observations outside the boundary mask
    ref = L.simulate(*p[:5], sigma, Er, Ur, Z, n_obs, time_end, return_chain=True, return_mask=True)
    common = np.minimum(events, ref[3])
    for k, ((xa, ya, _), (xb, yb, _)) in enumerate(zip(on_dev[4], ref[4])):
        rows = common > k
        assert np.array_equal(xa[rows], xb[rows]) and np.array_equal(ya[rows], yb[rows])
    mask = ref[5]
    share = mask[:, 1:].mean()
    print('boundary share %.3g (%d observations), event counts differ in %d rows' % (share, mask.sum(), (events != ref[3]).sum()))
    assert share <= 1e-3
    same = np.all((Y == ref[0]) | (np.isnan(Y) & np.isnan(ref[0])), axis=2)
    assert np.all(same | mask)
    assert np.all((events == ref[3]) | mask[:, -1])


def test_a_simulation_does_not_depend_on_its_schedule(hip_ctx):
    import elfi_amd
    n, n_obs, time_end, seed, stream = 777, 16, 2., 555, 3
    p = _prior_draws(n, np.random.RandomState(12), True)
    kw = dict(n_obs=n_obs, time_end=time_end, seed=seed, stream=stream, observed=OBS, return_series=True, return_status=True)
    base = elfi_amd.lotka_volterra_summaries(*p[:5], sigma=p[5], max_events=2000, **kw)
    status, events = base[2], base[3]
    assert (status == L.OUT_OF_EVENTS).any() and (status == L.REACHED_END).any() and (status == L.EXTINCT).any()
    # alone, as simulation 0 of a call whose indices start at i
    finished = np.flatnonzero(status != L.OUT_OF_EVENTS)
    for i in [0, 63, 64, 776, int(finished[np.argmax(events[finished])]), int(np.flatnonzero(status == L.OUT_OF_EVENTS)[0])]:
        alone = elfi_amd.lotka_volterra_summaries(*[a[i:i + 1] for a in p[:5]], sigma=p[5][i:i + 1], max_events=2000,
                                                  first_index=i, **kw)
        for a, b in zip(alone, base):
            assert np.array_equal(a[0], b[i], equal_nan=True)
    # inside a larger batch
    q = [np.concatenate([a, a[::-1][:300]]) for a in p]
    larger = elfi_amd.lotka_volterra_summaries(*q[:5], sigma=q[5], max_events=2000, **kw)
    for a, b in zip(larger, base):
        assert np.array_equal(a[:n], b, equal_nan=True)
    # with twice the events allowed: whatever finished is unchanged, and some of what was cut off now finishes
    twice = elfi_amd.lotka_volterra_summaries(*p[:5], sigma=p[5], max_events=4000, **kw)
    for a, b in zip(twice, base):
        assert np.array_equal(a[finished], b[finished], equal_nan=True)
    assert (twice[2] == L.OUT_OF_EVENTS).sum() < (status == L.OUT_OF_EVENTS).sum()
    # another stream: other draws
    other = elfi_amd.lotka_volterra_summaries(*p[:5], sigma=p[5], max_events=2000, **dict(kw, stream=stream + 2))
    assert np.mean(np.any(other[1] != base[1], axis=(1, 2))) > 0.5


# ---- 3. the _dev form and the limits ---------------------------------------------------------------------------------------
def test_dev_form_at_the_callers_pitch(hip_ctx):
    import torch
    import elfi_amd
    n, n_obs, time_end, n_events, pad = 130, 7, 2., 200, 3
    rs = np.random.RandomState(3)
    p = _prior_draws(n, rs, True)
    E, U, Z = rs.exponential(size=(n, n_events)), rs.uniform(size=(n, n_events)), rs.randn(n, 2 * (n_obs - 1))
    want = elfi_amd.lotka_volterra_summaries(*p[:5], sigma=p[5], n_obs=n_obs, time_end=time_end, draws=(E, U), noise=Z,
                                             observed=OBS, return_series=True, return_status=True)

    def padded(a, fill=np.nan):
        out = np.full((a.shape[0], a.shape[1] + pad), fill)
        out[:, :a.shape[1]] = a
        return torch.from_numpy(out).cuda()
    dE, dU, dZ = padded(E), padded(U), padded(Z)
    dp = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in p]
    dY = torch.full((n, 2 * n_obs + pad), -7.0, dtype=torch.float64, device='cuda')
    dS = torch.full((n, 9 + pad), -7.0, dtype=torch.float64, device='cuda')
    dT, dD = [torch.full((n + 2,), -7.0, dtype=torch.float64, device='cuda') for _ in range(2)]
    dst = torch.full((n + 2,), -7, dtype=torch.int32, device='cuda')
    dev = torch.full((n + 2,), -7, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    rc = hip_ctx.lib.elfihip_lv_summaries_dev(
        hip_ctx.handle, dE.data_ptr(), n_events + pad, dU.data_ptr(), n_events + pad, dZ.data_ptr(), 2 * (n_obs - 1) + pad,
        U64(0), U64(0), 0, n, n_obs, C.c_double(time_end), n_events, *[a.data_ptr() for a in dp], OBS.ctypes.data,
        dY.data_ptr(), 2 * n_obs + pad, dT.data_ptr(), dst.data_ptr(), dev.data_ptr(), dS.data_ptr(), 9 + pad, dD.data_ptr())
    assert rc == 0, hip_ctx.lib.elfihip_last_error(hip_ctx.handle)
    hip_ctx.synchronize()
    Y, S, T, D, st, ev = [a.cpu().numpy() for a in (dY, dS, dT, dD, dst, dev)]
    assert np.all(Y[:, 2 * n_obs:] == -7.0) and np.all(S[:, 9:] == -7.0)           # nothing written beyond a row
    assert all(np.all(a[n:] == -7) for a in (T, D, st, ev))
    got = (S[:, :9], Y[:, :2 * n_obs].reshape(n, n_obs, 2), st[:n], ev[:n], T[:n], D[:n])
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=True)
    for d, h in ((dE, E), (dU, U), (dZ, Z)):                                       # the inputs are untouched
        assert np.array_equal(d.cpu().numpy()[:, :h.shape[1]], h)


def test_library_refuses_what_it_cannot_hold(hip_ctx):
    import torch
    from elfi_amd import _lib
    lib, h = hip_ctx.lib, hip_ctx.handle
    buf = torch.ones(8192, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    p, out = buf.data_ptr(), buf.data_ptr() + 8 * 4096

    def lv(n=2, n_obs=16, time_end=2., max_events=50, dE=None, dU=None, dZ=None, sigma=None, observed=None, dD=None, first=0,
           ld=64):
        return lib.elfihip_lv_summaries_dev(h, dE, ld, dU, ld, dZ, ld, U64(1), U64(0), first, n, n_obs, C.c_double(time_end),
                                            max_events, p, p, p, p, p, sigma, observed, out, 2 * n_obs, None, None, None,
                                            out + 8 * 1024, 9, dD)
    assert lv(n_obs=2) == _lib.ERR_ARG and lv(n_obs=2049) == _lib.ERR_ARG and b'2048' in lib.elfihip_last_error(h)
    assert lv(max_events=0) == _lib.ERR_ARG and lv(max_events=(1 << 30) + 1) == _lib.ERR_ARG
    assert lv(n=0) == _lib.ERR_ARG
    for t in (0.0, -1.0, float('inf'), float('nan')):
        assert lv(time_end=t) == _lib.ERR_ARG
    assert lv(dD=out + 8 * 2048) == _lib.ERR_ARG                     # a distance without observed summaries
    assert lv(dE=p) == _lib.ERR_ARG and lv(dU=p) == _lib.ERR_ARG     # E without U
    assert lv(dZ=p) == _lib.ERR_ARG                                  # noise without sigma
    assert lv(dE=p, dU=p, ld=49) == _lib.ERR_ARG                     # a pitch below the row
    assert lv(first=-1) == _lib.ERR_ARG and lv(first=2 ** 32 - 1) == _lib.ERR_ARG
    assert lib.elfihip_lv_draws_dev(h, U64(1), U64(0), 0, 2, 0, out, 8, out, 8) == _lib.ERR_ARG
    assert lib.elfihip_lv_draws_dev(h, U64(1), U64(0), 0, 2, 8, out, 7, out, 8) == _lib.ERR_ARG
    assert lv(observed=OBS.ctypes.data, dD=out + 8 * 2048) == 0 and lv(dE=p, dU=p, dZ=p, sigma=p) == 0
    hip_ctx.synchronize()
    assert np.all(buf.cpu().numpy()[:4096] == 1.0)


# ---- 4. the model through ELFI's loops -------------------------------------------------------------------------------------
def _reference():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi
    return elfi


@pytest.mark.parametrize('noise', [False, True])
def test_model_through_the_loops(hip_ctx, noise):
    elfi = _reference()
    import elfi_amd
    from elfi.examples import lotka_volterra as lv
    m = elfi_amd.lotka_volterra_model(n_obs=20, observation_noise=noise, seed_obs=4, time_end=10., max_events=1 << 14)
    ref = lv.get_model(n_obs=20, observation_noise=noise, seed_obs=4, time_end=10.)
    names = ['r1', 'r2', 'r3', 'prey0', 'predator0'] + (['sigma'] if noise else [])
    public = [sorted(k for k in mdl.nodes if not k.startswith('_')) for mdl in (m, ref)]
    assert public[0] == public[1] == sorted(names + ['LV', 'd'] + list(L.NAMES))
    assert m.parameter_names == ref.parameter_names == sorted(names)
    for name in L.NAMES:            # the observed summaries are the reference's own
        assert np.array_equal(np.ravel(m[name].observed), np.ravel(ref[name].observed), equal_nan=True)
    batch = m.generate(300, outputs=names + ['LV', 'd'] + list(L.NAMES), seed=1)
    assert batch['LV'].shape == (300, 9) and batch['d'].shape == (300,)
    assert np.array_equal(batch['crosscorr'], batch['LV'][:, 8], equal_nan=True)
    res = elfi_amd.HipRejection(m['d'], batch_size=300, seed=2).sample(20, n_sim=1500)
    assert res.samples['r1'].shape == (20,)
    res2 = elfi.Rejection(m['d'], batch_size=300, seed=2).sample(20, n_sim=1500)
    for k in names:
        assert np.array_equal(res2.samples[k], res.samples[k])
    assert np.array_equal(res2.discrepancies, res.discrepancies)
