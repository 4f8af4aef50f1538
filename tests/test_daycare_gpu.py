"""GPU: the day-care-centre transmission example on the device (csrc/daycare.hip, elfi_amd.daycare_summaries,
daycare_distance, fused_models.daycare_model).

On given draws the device equals the NumPy statement (tests/daycare_ref.py, itself held to recorded runs of ELFI's example in
tests/test_daycare.py) bit for bit: states, status, event counts, final times -- no device transcendental is involved.  The
three counting summaries are the statement's on the device's own states, Shannon within a bound computed from its terms with
every logarithm within 4 ulp, and the distance is the statement's sort and L1 bit for bit on the device's own summaries.  The
drawn form is the given form on the draws elfihip_daycare_draws materialises.  A simulation does not depend on the batch, the
index it is given by, max_events or the call.  The recorded reference runs come out of the device state for state.
"""
import ctypes as C
import faulthandler
import os

import numpy as np
import pytest

import daycare_ref as R

pytestmark = pytest.mark.gpu

U64 = C.c_uint64
DEFAULT = (53, 33, 36)
# t1, t2, t3 planted over a batch: zero rates (one event), the priors' upper corner (runs out of the events of a test),
# NaN / negative / infinite parameters (invalid), t3 > 1 (co-infection favoured: valid)
PLANTED = [(0., 0., 0.), (11., 2., 1.), (np.nan, 0.6, 0.1), (3.6, -0.5, 0.1), (3.6, 0.6, np.inf), (3.6, 0.6, 2.5)]
INVALID_ROWS = [2, 3, 4]


@pytest.fixture(autouse=True)
def time_limit():
    """A hung kernel ends the run instead of holding the device: the process exits after 120 s in one test."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _observed(n_dcc, rs):
    obs = np.stack([rs.uniform(0, 2, n_dcc), rs.randint(0, 11, n_dcc).astype(float), rs.uniform(0, 1, n_dcc), rs.uniform(0, 1, n_dcc)])
    if n_dcc % 2:
        obs[3] = 0.0               # a row whose maximum is 0 is divided by 1
    return obs


def _ulp(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    ok = np.isfinite(want)
    return float(np.max(np.abs(got[ok] - want[ok]) / np.spacing(np.abs(want[ok])))) if ok.any() else 0.0


def _check_summaries(S, D, state, status, obs):
    """S against the statement on the device's own states, D against the statement on the device's own S."""
    import elfi_amd
    want = R.summaries(state, status)
    assert S.shape == want.shape and np.array_equal(np.isnan(S), np.isnan(want))
    assert np.array_equal(S[:, 1:], want[:, 1:], equal_nan=True)
    ok = ~np.isnan(want[:, 0])
    err, bound = np.abs(S[:, 0] - want[:, 0])[ok], R.shannon_bound(state)[ok]
    print('largest Shannon distance %.3g, %.3g of its bound' % (err.max(initial=0), (err / np.maximum(bound, 1e-300)).max(initial=0)))
    assert np.all(err <= bound)
    assert np.array_equal(D, R.distance(S, obs), equal_nan=True)
    assert np.array_equal(elfi_amd.daycare_distance(*[S[:, j] for j in range(4)], observed=[o[None, :] for o in obs]), D, equal_nan=True)
    bad = np.any(status != R.REACHED_END, axis=1)
    assert np.all(np.isnan(D[bad])) and np.all(np.isfinite(D[~bad]))


def _given(t, E, U, shape, time_end, obs, freq=None):
    import elfi_amd
    n_ind, n_strains, n_obs = shape
    S, state, status, events, T, D = elfi_amd.daycare_summaries(
        *t, n_dcc=E.shape[1], n_ind=n_ind, n_strains=n_strains, n_obs=n_obs, freq_strains_commun=freq, time_end=time_end,
        draws=(E, U), observed=obs, return_state=True, return_status=True)
    want = R.simulate(*t, E, U, n_ind, n_strains, freq, n_obs, time_end)
    assert state.shape == want[0].shape and state.dtype == np.bool_ and status.dtype == np.int32 and events.dtype == np.int64
    assert np.array_equal(state, want[0])
    assert np.array_equal(T, want[1], equal_nan=True)
    assert np.array_equal(status, want[2]) and np.array_equal(events, want[3])
    _check_summaries(S, D, state, status, obs)
    return status, events


# ---- 1. given draws --------------------------------------------------------------------------------------------------
# n in {1, 3, 70}, n_dcc in {1, 2, 29, 31} and the five shapes; time_end and the number of events keep the statement's own
# run short: the larger the centre, the faster its clock
CASES = [(1, 29, DEFAULT, 0.5, 250), (3, 1, (2, 1, 1), 2., 60), (70, 31, (5, 3, 4), 2., 100), (70, 2, DEFAULT, 0.5, 250),
         (3, 31, (64, 64, 64), 0.25, 150), (1, 2, (33, 64, 33), 1., 200), (3, 29, (2, 1, 1), 2., 60), (1, 1, (5, 3, 4), 2., 100)]


@pytest.mark.parametrize('n,n_dcc,shape,time_end,n_events', CASES)
def test_given_form_is_the_statement(hip_ctx, n, n_dcc, shape, time_end, n_events):
    rs = np.random.RandomState(31 * n + n_dcc + shape[0])
    t = [rs.uniform(0, 11, n), rs.uniform(0, 2, n), rs.uniform(0, 1, n)]
    if shape == DEFAULT:
        t = [np.minimum(t[0], 5.), np.minimum(t[1], 1.), t[2]]        # the ordinary rows finish within the events of the test
    rows = []
    if n >= len(PLANTED):         # the planted rows spread over the batch
        rows = np.linspace(0, n - 1, len(PLANTED)).astype(int)
        for row, what in zip(rows, PLANTED):
            for a, v in zip(t, what):
                a[row] = v
    E, U = rs.exponential(size=(n, n_dcc, n_events)), rs.uniform(size=(n, n_dcc, n_events))
    freq = rs.uniform(0, 0.3, shape[1]) if n == 3 else None
    status, events = _given(t, E, U, shape, time_end, _observed(n_dcc, rs), freq)
    if len(rows):
        assert np.all(status[rows[INVALID_ROWS]] == R.INVALID) and not events[rows[INVALID_ROWS]].any()
        assert np.all(status[rows[0]] == R.REACHED_END) and np.all(events[rows[0]] == 1)
        assert np.all(status[rows[5]] != R.INVALID)
        if shape == DEFAULT:
            assert np.all(status[rows[1]] == R.OUT_OF_EVENTS) and np.all(events[rows[1]] == n_events)
            assert (status == R.REACHED_END).sum() > status.size // 2
    if shape == DEFAULT:
        assert (status == R.REACHED_END).any() and events.max() > 60


@pytest.mark.parametrize('which,want', enumerate([R.REACHED_END, R.OUT_OF_EVENTS, R.INVALID, R.INVALID, R.INVALID, R.REACHED_END]))
def test_a_planted_simulation_alone(hip_ctx, which, want):
    rs = np.random.RandomState(17)
    E, U = rs.exponential(size=(1, 3, 400)), rs.uniform(size=(1, 3, 400))
    status, events = _given([np.array([v]) for v in PLANTED[which]], E, U, DEFAULT, 0.5, _observed(3, rs))
    assert np.all(status == want)


def test_the_recorded_reference_runs_through_the_device(hip_ctx, golden_dir):
    import elfi_amd
    g = np.load(os.path.join(golden_dir, 'daycare.npz'))
    for name in g['sets']:
        p, (n_ind, n_strains, n_obs) = g[name + '_params'], [int(v) for v in g[name + '_shape']]
        E, U = R.golden_draws(g[name + '_seed'], len(p), int(g[name + '_n_events']))
        kw = dict(n_ind=n_ind, n_strains=n_strains, n_obs=n_obs, time_end=float(g[name + '_time_end']), return_state=True,
                  return_status=True)
        # every centre a simulation of its own, as it was recorded
        S, state, status, events, T = elfi_amd.daycare_summaries(p[:, 0], p[:, 1], p[:, 2], n_dcc=1, draws=(E[:, None], U[:, None]), **kw)
        assert np.array_equal(state[:, 0], g[name + '_state']) and np.array_equal(events[:, 0], g[name + '_events'])
        assert np.all(status == R.REACHED_END)
        assert np.array_equal(S[:, 1:, 0].T, g[name + '_S'][1:])
        assert np.all(np.abs(S[:, 0, 0] - g[name + '_S'][0]) <= R.shannon_bound(state)[:, 0])
        if np.all(p == p[0]):     # ... and, where they share their parameters, as the centres of ONE simulation
            one = elfi_amd.daycare_summaries(*p[0], n_dcc=len(p), draws=(E[None], U[None]), observed=g[name + '_obs'], **kw)
            assert np.array_equal(one[1][0], g[name + '_state']) and np.array_equal(one[3][0], g[name + '_events'])
            assert np.array_equal(one[0][0], S[:, :, 0].T)
            # the reference's distance on its own summaries: Shannon's bound divided by the observed maximum, and the
            # rounding of 4 n_dcc non-negative terms summed in another order
            D, Dw = one[5][0], float(g[name + '_D'][0])
            slack = np.sum(R.shannon_bound(one[1])[0]) / max(g[name + '_obs'][0].max(), 1e-300) / (4 * len(p))
            assert abs(D - Dw) <= slack + 4 * len(p) * R.EPS * abs(Dw)


# ---- 2. the distance alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,k,m', [(130, 1, 1), (1, 4, 29), (1000, 4, 29), (5, 16, 256), (70, 3, 1024), (67, 7, 33), (3, 1, 1024)])
def test_distance_is_the_statement(hip_ctx, n, k, m):
    import elfi_amd
    rs = np.random.RandomState(n + k + m)
    X = np.round(rs.uniform(0, 3, (n, k, m)), 1)          # rounded: ties within a row
    obs = np.round(rs.uniform(0, 2, (k, m)), 1)
    obs[k // 2] = 0.0
    if n > 2:
        X[n // 2, k - 1, m // 2] = np.nan
        X[n - 1, 0, :] = np.nan
    D = elfi_amd.daycare_distance(X, observed=obs)
    want = R.distance(X, obs)
    assert D.shape == (n,) and np.array_equal(D, want, equal_nan=True)
    assert np.isnan(D).sum() == (2 if n > 2 else 0)
    cols = elfi_amd.daycare_distance(*[X[:, j] for j in range(k)], observed=[obs[j][None] for j in range(k)])
    assert np.array_equal(cols, D, equal_nan=True)


# ---- 3. draws made in the kernel ----------------------------------------------------------------------------------------
def test_drawn_form(hip_ctx):
    import elfi_amd
    n, n_dcc, time_end, n_events, seed, stream = 5, 3, 1., 300, 4321, 6
    rs = np.random.RandomState(7)
    t = [rs.uniform(0, 5, n), rs.uniform(0, 1, n), rs.uniform(0, 1, n)]
    t[0][1], t[1][1], t[2][1] = PLANTED[1]
    obs = _observed(n_dcc, rs)
    kw = dict(n_dcc=n_dcc, time_end=time_end, observed=obs, return_state=True, return_status=True)
    drawn = elfi_amd.daycare_summaries(*t, max_events=n_events, seed=seed, stream=stream, **kw)
    E, U = elfi_amd.daycare_draws(n, n_dcc, n_events, seed=seed, stream=stream)
    given = elfi_amd.daycare_summaries(*t, draws=(E, U), **kw)
    for a, b in zip(drawn, given):
        assert np.array_equal(a, b, equal_nan=True)
    S, state, status, events, T, D = drawn
    want = R.simulate(*t, E, U, time_end=time_end)
    assert np.array_equal(state, want[0]) and np.array_equal(T, want[1]) and np.array_equal(status, want[2])
    assert np.array_equal(events, want[3])
    assert np.all(status[1] == R.OUT_OF_EVENTS) and np.all(status[[0, 2, 3, 4]] == R.REACHED_END)
    _check_summaries(S, D, state, status, obs)
    # the draws against the statement's layout: uniforms bit for bit, exponentials within 4 ulp
    Er, Ur, _ = R.draws(seed, stream, n, n_dcc, n_events)
    assert np.array_equal(U, Ur)
    ulp = _ulp(E, Er)
    print('largest exponential distance %.2f ulp' % ulp)
    assert ulp <= 4 and np.array_equal(E == 0, Er == 0)
    E2, U2 = elfi_amd.daycare_draws(2, n_dcc + 2, n_events + 9, seed=seed, stream=stream, first_index=3)
    assert np.array_equal(E2[:, :n_dcc, :n_events], E[3:]) and np.array_equal(U2[:, :n_dcc, :n_events], U[3:])


def test_a_simulation_does_not_depend_on_its_schedule(hip_ctx):
    import elfi_amd
    n, n_dcc, seed, stream = 9, 4, 555, 3
    rs = np.random.RandomState(12)
    t = [rs.uniform(0, 5, n), rs.uniform(0, 1, n), rs.uniform(0, 1, n)]
    t[0][4], t[1][4], t[2][4] = PLANTED[1]
    t[0][7] = np.nan
    obs = _observed(n_dcc, rs)
    kw = dict(n_dcc=n_dcc, time_end=0.5, seed=seed, stream=stream, observed=obs, return_state=True, return_status=True)
    base = elfi_amd.daycare_summaries(*t, max_events=400, **kw)
    status = base[2]
    assert np.all(status[4] == R.OUT_OF_EVENTS) and np.all(status[7] == R.INVALID) and (status == R.REACHED_END).sum() == 7 * n_dcc
    again = elfi_amd.daycare_summaries(*t, max_events=400, **kw)                  # the same call
    for a, b in zip(again, base):
        assert np.array_equal(a, b, equal_nan=True)
    for i in (0, 4, 7, 8):        # alone, as simulation 0 of a call whose indices start at i
        alone = elfi_amd.daycare_summaries(*[a[i:i + 1] for a in t], max_events=400, first_index=i, **kw)
        for a, b in zip(alone, base):
            assert np.array_equal(a[0], b[i], equal_nan=True)
    q = [np.concatenate([a, a[::-1], a[:5]]) for a in t]                           # inside a larger batch
    larger = elfi_amd.daycare_summaries(*q, max_events=400, **kw)
    for a, b in zip(larger, base):
        assert np.array_equal(a[:n], b, equal_nan=True)
    # with twice the events allowed: whatever finished is unchanged, and what was cut off now finishes
    twice = elfi_amd.daycare_summaries(*t, max_events=800, **kw)
    finished = np.all(status != R.OUT_OF_EVENTS, axis=1)
    for a, b in zip(twice, base):
        assert np.array_equal(a[finished], b[finished], equal_nan=True)
    assert np.all(twice[2][4] == R.REACHED_END) and np.all(twice[3][4] > 400)
    other = elfi_amd.daycare_summaries(*t, max_events=400, **dict(kw, stream=stream + 2))      # another stream: other draws
    assert np.mean(np.any(other[1] != base[1], axis=(2, 3))) > 0.5


# ---- 4. the _dev forms and the limits --------------------------------------------------------------------------------------
def test_dev_forms_at_the_callers_pitch(hip_ctx):
    import torch
    import elfi_amd
    n, n_dcc, shape, time_end, n_events, pad = 7, 5, (9, 6, 7), 2., 120, 3
    n_ind, n_strains, n_obs = shape
    rs = np.random.RandomState(3)
    t = [rs.uniform(0, 11, n), rs.uniform(0, 2, n), rs.uniform(0, 1, n)]
    E, U = rs.exponential(size=(n, n_dcc, n_events)), rs.uniform(size=(n, n_dcc, n_events))
    obs, freq = _observed(n_dcc, rs), rs.uniform(0, 0.3, n_strains)
    want = elfi_amd.daycare_summaries(*t, n_dcc=n_dcc, n_ind=n_ind, n_strains=n_strains, n_obs=n_obs, freq_strains_commun=freq,
                                      time_end=time_end, draws=(E, U), observed=obs, return_state=True, return_status=True)
    pairs = n * n_dcc

    def padded(a):
        out = np.full((pairs, n_events + pad), np.nan)
        out[:, :n_events] = a.reshape(pairs, n_events)
        return torch.from_numpy(out).cuda()
    dE, dU = padded(E), padded(U)
    dt = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in t]
    dM = torch.full((pairs, n_obs + pad), -7, dtype=torch.int64, device='cuda')
    dS = torch.full((n, 4 * n_dcc + pad), -7.0, dtype=torch.float64, device='cuda')
    dT = torch.full((pairs + 2,), -7.0, dtype=torch.float64, device='cuda')
    dD = torch.full((n + 2,), -7.0, dtype=torch.float64, device='cuda')
    dst = torch.full((pairs + 2,), -7, dtype=torch.int32, device='cuda')
    dev = torch.full((pairs + 2,), -7, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    rc = hip_ctx.lib.elfihip_daycare_summaries_dev(
        hip_ctx.handle, dE.data_ptr(), n_events + pad, dU.data_ptr(), n_events + pad, U64(0), U64(0), 0, n, n_dcc, n_ind,
        n_strains, n_obs, C.c_double(time_end), n_events, *[a.data_ptr() for a in dt], freq.ctypes.data, obs.ctypes.data,
        dM.data_ptr(), n_obs + pad, dT.data_ptr(), dst.data_ptr(), dev.data_ptr(), dS.data_ptr(), 4 * n_dcc + pad, dD.data_ptr())
    assert rc == 0, hip_ctx.lib.elfihip_last_error(hip_ctx.handle)
    hip_ctx.synchronize()
    M, S, T, D, st, ev = [a.cpu().numpy() for a in (dM, dS, dT, dD, dst, dev)]
    assert np.all(M[:, n_obs:] == -7) and np.all(S[:, 4 * n_dcc:] == -7.0)        # nothing written beyond a row
    assert all(np.all(a[pairs:] == -7) for a in (T, st, ev)) and np.all(D[n:] == -7)
    state = ((M[:, :n_obs, None].astype(np.uint64) >> np.arange(n_strains, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    got = (S[:, :4 * n_dcc].reshape(n, 4, n_dcc), state.reshape(n, n_dcc, n_obs, n_strains), st[:pairs].reshape(n, n_dcc),
           ev[:pairs].reshape(n, n_dcc), T[:pairs].reshape(n, n_dcc), D[:n])
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=True)
    # the distance alone on the padded summaries
    dD2 = torch.full((n + 2,), -7.0, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    assert hip_ctx.lib.elfihip_daycare_distance_dev(hip_ctx.handle, dS.data_ptr(), 4 * n_dcc + pad, n, 4, n_dcc, obs.ctypes.data,
                                                    dD2.data_ptr()) == 0
    hip_ctx.synchronize()
    D2 = dD2.cpu().numpy()
    assert np.array_equal(D2[:n], want[5], equal_nan=True) and np.all(D2[n:] == -7)
    # the draws at a pitch
    dE2, dU2 = [torch.full((pairs, n_events + pad), -7.0, dtype=torch.float64, device='cuda') for _ in range(2)]
    torch.cuda.synchronize()
    assert hip_ctx.lib.elfihip_daycare_draws_dev(hip_ctx.handle, U64(5), U64(2), 0, n, n_dcc, n_events, dE2.data_ptr(),
                                                 n_events + pad, dU2.data_ptr(), n_events + pad) == 0
    hip_ctx.synchronize()
    Eh, Uh = elfi_amd.daycare_draws(n, n_dcc, n_events, seed=5, stream=2)
    for d, h in ((dE2, Eh), (dU2, Uh)):
        a = d.cpu().numpy()
        assert np.array_equal(a[:, :n_events], h.reshape(pairs, n_events)) and np.all(a[:, n_events:] == -7)


def test_library_refuses_what_it_cannot_hold(hip_ctx):
    import torch
    from elfi_amd import _lib
    lib, h = hip_ctx.lib, hip_ctx.handle
    buf = torch.ones(16384, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    p, out = buf.data_ptr(), buf.data_ptr() + 8 * 8192
    obs = np.ones((4, 1024))

    def dc(n=2, n_dcc=3, n_ind=8, n_strains=5, n_obs=6, time_end=1., max_events=20, dE=None, dU=None, freq=None, observed=None,
           dD=None, first=0, ld=64, ldm=8, lds=16):
        return lib.elfihip_daycare_summaries_dev(h, dE, ld, dU, ld, U64(1), U64(0), first, n, n_dcc, n_ind, n_strains, n_obs,
                                                 C.c_double(time_end), max_events, p, p, p, freq, observed, out, ldm, None, None,
                                                 None, out + 8 * 1024, lds, dD)
    for kw in (dict(n_ind=1), dict(n_ind=65), dict(n_strains=0), dict(n_strains=65), dict(n_obs=0), dict(n_obs=9), dict(n_dcc=0),
               dict(n_dcc=1025), dict(n=0), dict(max_events=0), dict(max_events=(1 << 21) + 1), dict(first=-1),
               dict(first=2 ** 32 - 1), dict(ldm=5), dict(lds=11), dict(dE=p), dict(dU=p), dict(dE=p, dU=p, ld=19),
               dict(dD=out + 8 * 2048)):
        assert dc(**kw) == _lib.ERR_ARG, kw
    for t in (0.0, -1.0, float('inf'), float('nan')):
        assert dc(time_end=t) == _lib.ERR_ARG
    for f in (-0.1, float('nan'), float('inf')):
        freq = np.array([0.1, 0.1, f, 0.1, 0.1])
        assert dc(freq=freq.ctypes.data) == _lib.ERR_ARG
    assert b'strains' in lib.elfihip_last_error(h) or b'freq' in lib.elfihip_last_error(h)
    assert lib.elfihip_daycare_draws_dev(h, U64(1), U64(0), 0, 2, 3, 0, out, 8, out, 8) == _lib.ERR_ARG
    assert lib.elfihip_daycare_draws_dev(h, U64(1), U64(0), 0, 2, 3, 8, out, 7, out, 8) == _lib.ERR_ARG
    assert lib.elfihip_daycare_draws_dev(h, U64(1), U64(0), 0, 2, 1025, 8, out, 8, out, 8) == _lib.ERR_ARG

    def dist(n=2, k=4, m=3, ldx=16, observed=obs.ctypes.data):
        return lib.elfihip_daycare_distance_dev(h, p, ldx, n, k, m, observed, out)
    for kw in (dict(n=0), dict(k=0), dict(k=17), dict(m=0), dict(m=1025), dict(k=8, m=600, ldx=4800), dict(ldx=11), dict(observed=None)):
        assert dist(**kw) == _lib.ERR_ARG, kw
    bad = obs.copy()
    bad[0, 1] = np.nan
    assert dist(observed=bad.ctypes.data) == _lib.ERR_ARG
    assert dc(observed=obs.ctypes.data, dD=out + 8 * 2048) == 0 and dc(dE=p, dU=p) == 0 and dist() == 0
    hip_ctx.synchronize()
    assert np.all(buf.cpu().numpy()[:8192] == 1.0)


# ---- 5. the model through ELFI's loops -------------------------------------------------------------------------------------
def _reference():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi
    return elfi


SMALL = dict(n_dcc=4, n_ind=10, n_strains=6, n_obs=8, time_end=2., max_events=1 << 12)
BOUNDS = {'t1': (0, 11), 't2': (0, 2), 't3': (0, 1)}


def test_model_through_rejection(hip_ctx):
    elfi = _reference()
    import elfi_amd
    m = elfi_amd.daycare_model(seed_obs=4, **SMALL)
    names = ['t1', 't2', 't3']
    batch = m.generate(50, outputs=names + ['DCC', 'd', 'logd'] + list(R.NAMES), seed=1)
    assert batch['DCC'].shape == (50, 4, 4) and batch['d'].shape == batch['logd'].shape == (50,)
    assert np.array_equal(batch['multi'], batch['DCC'][:, 3]) and np.all(np.isfinite(batch['d']))
    obs = [m[name].observed for name in R.NAMES]
    assert np.array_equal(batch['d'], R.distance(batch['DCC'], np.concatenate(obs)))
    assert np.array_equal(batch['logd'], np.log(batch['d']))
    res = elfi_amd.HipRejection(m['d'], batch_size=100, seed=2).sample(10, n_sim=300)
    assert res.samples['t1'].shape == (10,) and np.all(np.isfinite(res.discrepancies))
    res2 = elfi.Rejection(m['d'], batch_size=100, seed=2).sample(10, n_sim=300)
    for k in names:
        assert np.array_equal(res2.samples[k], res.samples[k])
    assert np.array_equal(res2.discrepancies, res.discrepancies)


def test_bolfi_fits_logd(hip_ctx):
    elfi = _reference()
    import elfi_amd
    from elfi.model.extensions import ModelPrior
    names = ['t1', 't2', 't3']
    # the reference's own BOLFI loop, unmodified, over the device surrogate
    m = elfi_amd.daycare_model(seed_obs=4, **SMALL)
    gp = elfi_amd.HipGPRegression(names, bounds=BOUNDS)
    acq = elfi_amd.HipLCBSC(gp, prior=ModelPrior(m, parameter_names=names), noise_var=0.1, exploration_rate=10, seed=1)
    b = elfi.BOLFI(m['logd'], batch_size=1, initial_evidence=8, update_interval=4, bounds=BOUNDS, acq_noise_var=0.1,
                   target_model=gp, acquisition_method=acq, seed=1)
    b.fit(n_evidence=12, bar=False)
    assert b.target_model.X.shape == (12, 3) and np.all(np.isfinite(b.target_model.Y))
    assert set(b.extract_result().x_min) == set(names)
    # ... and HipBOLFI
    m2 = elfi_amd.daycare_model(seed_obs=4, **SMALL)
    hb = elfi_amd.HipBOLFI(m2['logd'], batch_size=1, initial_evidence=8, update_interval=4, bounds=BOUNDS, acq_noise_var=0.1, seed=1)
    hb.fit(n_evidence=12, bar=False)
    assert hb.target_model.X.shape == (12, 3) and np.all(np.isfinite(hb.target_model.Y))
