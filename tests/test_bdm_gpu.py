"""GPU: the birth-death-mutation model of csrc/bdm.hip against its NumPy statement (tests/bdm_ref.py), which tests/test_bdm.py
pins to recorded runs of the reference's own simulator.  Clusters, status and event counts are integers, T1 is one division
of two of them, T2 a sum in NumPy's order, the distance one subtraction: everything is compared for EQUALITY.

  1. the given form over population sizes on both sides of every path (registers up to 64, LDS blocks of 2 .. 64 slots, a
     ragged last block), batches of 1, 3 and 130, both stopping modes, with planted rows: out of events, extinct, invalid
     rates, a uniform that is none
  2. every recorded reference run through the kernel on the replayed uniforms
  3. the drawn form is the given form on bdm_draws; a simulation does not depend on the batch, on first_index or on max_events
     -- nor on the kernel: from two full grids of simulations on, N <= 32 runs two simulations per wavefront, and such a batch
     equals the same simulations run in small batches
  4. the _dev forms at the caller's pitch between guard words, and on a busy adopted stream in stream order
  5. the distribution of the device's own draws against 4096 recorded runs of the reference binary
  6. the model through ELFI
"""
import ctypes as C
import faulthandler
import os

import numpy as np
import pytest

import bdm_ref as R
import stream_order as SO
from test_bdm import SETS, replay

pytestmark = pytest.mark.gpu
U64 = C.c_uint64
MAX_EVENTS = 4096


@pytest.fixture(autouse=True)
def time_limit():
    """A hung kernel ends the run instead of holding the device: the process exits after 120 s in one test."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'bdm.npz'))


def same(got, want, what):
    for a, b, part in zip(got, want, ('clusters', 'T', 'status', 'events', 'D')):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), '%s: %s differs' % (what, part)


def statement(alpha, delta, tau, N, mode, U, obs, t2_n=None, max_events=None):
    Cl, st, ev = R.simulate(alpha, delta, tau, N, mode, U, max_events)
    T = R.summaries(Cl, st, N if t2_n is None else t2_n)
    return Cl, T, st, ev, R.distance(T, obs)


# ---- 1. the given form ------------------------------------------------------------------------------------------------------
def planted_batch(n, N, mode, seed):
    """Rates and uniforms of a batch, and the statuses its planted rows must end with (row -> status).  The statement walks
    every event in Python, so where n N is large only every few rows run long; the others die out early (delta >> alpha)."""
    rs = np.random.RandomState(seed)
    alpha, tau = rs.uniform(0.2, 2.0, n), rs.uniform(0.05, 1.0, n)
    delta = alpha * rs.uniform(0.0, 0.3, n)
    stride = max(1, n * N // 6000)
    short = np.arange(n) % stride != 0
    delta[short] = alpha[short] * rs.uniform(3.0, 10.0, n)[short]
    U = rs.random_sample((n, 2 * MAX_EVENTS))
    must = {}
    if n == 3:
        U[1, 5] = 1.0                                    # event 3's cluster draw
        alpha[1], delta[1] = 1.0, 0.0
        if N >= 20:                                      # (a smaller population may be complete before event 3)
            must[1] = R.INVALID
        delta[2] = 10 * alpha[2]
    if n >= 100:
        alpha[1], delta[1], tau[1] = 1.0, 0.0, 1.0       # many clusters: every block of the wide form is reached
        alpha[5], delta[5], tau[5] = 0.0, 0.0, 0.3
        if N + mode > 1:                                 # (N = 1 in mode 0 is complete before the first event)
            must[5] = R.OUT_OF_EVENTS
        delta[6] = 10 * alpha[6]
        for row, rates in ((7, (np.nan, 0.1, 0.1)), (8, (0.5, -0.1, 0.1)), (9, (0.5, 0.1, np.inf)), (10, (0.0, 0.0, 0.0)),
                           (11, (0.5, np.nan, 0.1)), (12, (-0.0, 0.0, -1e-300))):
            alpha[row], delta[row], tau[row] = rates
            must[row] = R.INVALID
        alpha[[13, 14, 66]], delta[[13, 14, 66]] = 1.0, 0.0            # (births and mutations only: at least N - 1 events)
        U[13, 4], U[14, 5], U[66, 4] = 1.0, np.nan, -0.25
        if N >= 20:
            must.update({13: R.INVALID, 14: R.INVALID, 66: R.INVALID})
        alpha[64], delta[64], tau[64] = 1.0, 0.0, 0.0                  # births only: one cluster of N
        must[64] = R.REACHED_N
    return alpha, delta, tau, U, must


@pytest.mark.parametrize('mode', [1, 0])
@pytest.mark.parametrize('N', [1, 2, 20, 63, 64, 65, 128, 473, 4096])
@pytest.mark.parametrize('n', [1, 3, 130])
def test_given_form_is_the_statement(hip_ctx, n, N, mode):
    import elfi_amd
    alpha, delta, tau, U, must = planted_batch(n, N, mode, 1000 * n + N + mode)
    want = statement(alpha, delta, tau, N, mode, U, 0.55)
    got = elfi_amd.bdm_clusters(alpha, delta, tau, N=N, mode=mode, draws=U, observed=0.55, return_summaries=True, return_status=True)
    Cl, T, st, ev, D = got
    assert Cl.dtype == np.int32 and st.dtype == np.int32 and ev.dtype == np.int64 and T.shape == (n, 2)
    same(got, want, 'given form n=%d N=%d mode=%d' % (n, N, mode))
    for row, status in must.items():
        assert st[row] == status, (row, st[row], status)
    bad = st == R.INVALID
    assert not Cl[bad].any() and np.isnan(T[st >= 2]).all() and np.isnan(D[st >= 2]).all()
    assert np.all(Cl.sum(axis=1)[st == R.REACHED_N] == N) and not Cl[st == R.EXTINCT].any()
    assert np.all(T[st == R.EXTINCT, 1] == 1.0) and np.isnan(T[st == R.EXTINCT, 0]).all()
    assert np.all(ev[st == R.OUT_OF_EVENTS] == MAX_EVENTS)
    if n >= 100:
        assert ev[7:13].tolist() == [0] * 6 and (N < 20 or ev[[13, 14, 66]].tolist() == [2, 2, 2])
        assert ((st == R.EXTINCT).any() or N + mode == 1) and Cl[64, 0] == N and ev[64] == N - 1 + mode
        if N == 4096:
            assert st[1] == R.OUT_OF_EVENTS and (Cl[1] > 0).sum() > 1000 and np.flatnonzero(Cl[1])[-1] >= 1024
    # another divisor of T2, and nothing but the clusters asked for
    only = elfi_amd.bdm_clusters(alpha, delta, tau, N=N, mode=mode, draws=U)
    assert isinstance(only, np.ndarray) and np.array_equal(only, Cl)
    T7 = elfi_amd.bdm_clusters(alpha, delta, tau, N=N, mode=mode, draws=U, t2_n=7.5, return_summaries=True)[1]
    assert np.array_equal(T7, R.summaries(Cl, st, 7.5), equal_nan=True)


# ---- 2. the recorded runs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SETS)
def test_recorded_runs_through_the_kernel(hip_ctx, golden, name):
    import elfi_amd
    p, N, mode, Cl, st, ev, _, U = replay(golden, name)
    got = elfi_amd.bdm_clusters(p[:, 0], p[:, 1], p[:, 2], N=N, mode=mode, draws=U, observed=0.55, t2_n=20, return_summaries=True,
                                return_status=True)
    T = R.summaries(Cl, st, 20)
    same(got, (Cl, T, st, ev, R.distance(T, 0.55)), name)
    assert np.array_equal(got[0], golden[name + '_clusters'])          # cluster for cluster what the binary printed


# ---- 3. the drawn form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,n,n_events', [(20, 130, 1024), (473, 20, 2048), (64, 3, 512), (2, 1, 16)])
def test_drawn_form_is_the_given_form_on_its_draws(hip_ctx, N, n, n_events):
    import elfi_amd
    rs = np.random.RandomState(N)
    alpha, tau = rs.uniform(0.1, 2.0, n), rs.uniform(0.05, 1.0, n)
    delta = alpha * rs.uniform(0.0, 0.5, n)
    seed, stream, first = 2017, 3, 2 ** 32 - n if N == 64 else 40
    U = elfi_amd.bdm_draws(n, n_events, seed=seed, stream=stream, first_index=first)
    assert U.shape == (n, 2 * n_events) and np.array_equal(U, R.draws(seed, stream, n, n_events, first))
    kw = dict(N=N, mode=1, observed=0.55, return_summaries=True, return_status=True)
    given = elfi_amd.bdm_clusters(alpha, delta, tau, draws=U, **kw)
    drawn = elfi_amd.bdm_clusters(alpha, delta, tau, max_events=n_events, seed=seed, stream=stream, first_index=first, **kw)
    same(drawn, given, 'drawn form')
    same(drawn, statement(alpha, delta, tau, N, 1, U, 0.55), 'statement')
    st, ev = drawn[2], drawn[3]
    assert (st == R.REACHED_N).any() and ev.max() > (64 if N >= 20 else 1)         # the draws are fetched more than once
    # max_events above a simulation's own count does not enter its result; below it cuts it off there
    more = elfi_amd.bdm_clusters(alpha, delta, tau, max_events=4 * n_events + 3, seed=seed, stream=stream, first_index=first, **kw)
    done = st != R.OUT_OF_EVENTS
    for a, b in zip(more, drawn):
        assert np.array_equal(a[done], b[done], equal_nan=True)
    i = int(np.argmax(np.where(done, ev, 0)))
    if ev[i] > 1:
        cut = elfi_amd.bdm_clusters(alpha[i], delta[i], tau[i], max_events=int(ev[i]) - 1, seed=seed, stream=stream,
                                    first_index=first + i, **kw)
        assert cut[2][0] == R.OUT_OF_EVENTS and cut[3][0] == ev[i] - 1 and np.isnan(cut[1]).all()
    # simulation i of the call is simulation 0 of a call with first_index + i: neither n nor the wavefront enters
    for i in sorted({0, n // 2, n - 1}):
        one = elfi_amd.bdm_clusters(alpha[i], delta[i], tau[i], max_events=n_events, seed=seed, stream=stream, first_index=first + i, **kw)
        same(one, [a[i:i + 1] for a in drawn], 'single call %d' % i)
    if n > 1:       # another stream: other draws
        other = elfi_amd.bdm_clusters(alpha, delta, tau, max_events=n_events, seed=seed, stream=stream + 1, first_index=first, **kw)
        assert not np.array_equal(other[3], ev)


# ---- 3b. two simulations per wavefront ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [1, 0])
@pytest.mark.parametrize('N', [1, 20, 32])
def test_a_full_device_runs_pairs_and_gives_the_same_simulations(hip_ctx, N, mode):
    """A batch of two full grids (32 wavefronts per CU) and three more -- an odd number: the last wavefront holds one
    simulation -- goes to bd_pair_kernel; cut into batches of 4096 it goes to bd_sim_kernel.  Both forms, every output equal;
    some rows against the statement."""
    import torch
    import elfi_amd
    n, n_events = 64 * torch.cuda.get_device_properties(0).multi_processor_count + 3, 128
    rs = np.random.RandomState(N + mode)
    alpha, tau = rs.uniform(0.005, 2.005, n), np.full(n, 0.198)
    delta = np.where(np.arange(n) % 3 == 0, alpha * rs.uniform(0.0, 10.0, n), 0.0)
    alpha[5], delta[5] = 0.0, 0.0                                 # out of events
    alpha[7], tau[n - 1], delta[n - 2] = np.nan, np.inf, -1.0      # invalid, the lone last simulation among them
    alpha[[13, 14, n - 3]], delta[[13, 14, n - 3]] = 1.0, 0.0
    U = rs.random_sample((n, 2 * n_events))
    U[13, 4], U[14, 5], U[n - 3, 0] = 1.0, np.nan, -0.5
    kw = dict(N=N, mode=mode, observed=0.55, return_summaries=True, return_status=True)
    for form in ('given', 'drawn'):
        def run(lo, hi):
            if form == 'given':
                return elfi_amd.bdm_clusters(alpha[lo:hi], delta[lo:hi], tau[lo:hi], draws=U[lo:hi], **kw)
            return elfi_amd.bdm_clusters(alpha[lo:hi], delta[lo:hi], tau[lo:hi], max_events=n_events, seed=4, stream=1, first_index=lo + 9, **kw)
        whole = run(0, n)
        parts = [run(lo, min(lo + 4096, n)) for lo in range(0, n, 4096)]
        same(whole, [np.concatenate([p[j] for p in parts]) for j in range(5)], 'pairs, %s form' % form)
        st, ev = whole[2], whole[3]
        assert st[7] == st[n - 1] == st[n - 2] == R.INVALID and ev[7] == ev[n - 1] == ev[n - 2] == 0
        if N + mode > 1:
            assert st[5] == R.OUT_OF_EVENTS and ev[5] == n_events and (st == R.EXTINCT).any() and (st == R.REACHED_N).any()
        if form == 'given':
            assert N < 20 or (st[[13, 14, n - 3]].tolist() == [R.INVALID] * 3 and ev[[13, 14, n - 3]].tolist() == [2, 2, 0])
            rows = np.r_[0:24, n - 6:n]
            same([a[rows] for a in whole], statement(alpha[rows], delta[rows], tau[rows], N, mode, U[rows], 0.55), 'pairs, statement')


# ---- 4. the _dev forms ------------------------------------------------------------------------------------------------------
def _dev_inputs(which):
    n, N, n_events = 7, (20, 150)[which], 256
    rs = np.random.RandomState(700 + which)
    alpha, tau = rs.uniform(0.3, 2.0, n), rs.uniform(0.05, 1.0, n)
    delta = alpha * rs.uniform(0.0, 0.5, n)
    alpha[3] = np.nan
    return n, N, n_events, alpha, delta, tau, rs.random_sample((n, 2 * n_events))


@pytest.mark.parametrize('which', [0, 1], ids=['N20', 'N150'])
def test_dev_forms_at_the_callers_pitch(hip_ctx, which):
    import torch
    import elfi_amd
    n, N, n_events, alpha, delta, tau, U = _dev_inputs(which)
    lib, h = hip_ctx.lib, hip_ctx.handle
    pad, guard = 3, -7.0625e300
    ldu, ldc, ldt = 2 * n_events + pad, N + pad, 2 + pad
    Up = np.full((n, ldu), np.nan)
    Up[:, :2 * n_events] = U
    da, dd, dt, dU = (torch.from_numpy(a).cuda() for a in (alpha, delta, tau, Up))
    obs = np.array([0.55])
    for given in (True, False):
        want = elfi_amd.bdm_clusters(alpha, delta, tau, N=N, mode=1, max_events=n_events, draws=U if given else None, seed=9, stream=2,
                                     first_index=3, observed=0.55, return_summaries=True, return_status=True)
        dCl = torch.full((2 + n * ldc + 2,), -7, dtype=torch.int32, device='cuda')
        dT = torch.full((2 + n * ldt + 2,), guard, dtype=torch.float64, device='cuda')
        dD = torch.full((n + 2,), guard, dtype=torch.float64, device='cuda')
        dst = torch.full((n + 2,), -7, dtype=torch.int32, device='cuda')
        dev = torch.full((n + 2,), -7, dtype=torch.int64, device='cuda')
        torch.cuda.synchronize()
        rc = lib.elfihip_bdm_clusters_dev(h, dU.data_ptr() if given else None, ldu, U64(9), U64(2), 3, n, N, 1, n_events, da.data_ptr(),
                                          dd.data_ptr(), dt.data_ptr(), C.c_double(N), obs.ctypes.data, dCl.data_ptr() + 8, ldc,
                                          dst.data_ptr(), dev.data_ptr(), dT.data_ptr() + 16, ldt, dD.data_ptr())
        assert rc == 0, lib.elfihip_last_error(h)
        hip_ctx.synchronize()
        Cl, T, D, st, ev = (t.cpu().numpy() for t in (dCl, dT, dD, dst, dev))
        rows, trows = Cl[2:2 + n * ldc].reshape(n, ldc), T[2:2 + n * ldt].reshape(n, ldt)
        assert np.all(Cl[:2] == -7) and np.all(Cl[2 + n * ldc:] == -7) and np.all(rows[:, N:] == -7)
        assert np.all(T[:2] == guard) and np.all(T[2 + n * ldt:] == guard) and np.all(trows[:, 2:] == guard)
        assert np.all(D[n:] == guard) and np.all(st[n:] == -7) and np.all(ev[n:] == -7)
        same((rows[:, :N], trows[:, :2], st[:n], ev[:n], D[:n]), want, '_dev form')
        # only the distance is asked for
        dD.fill_(guard)
        torch.cuda.synchronize()
        rc = lib.elfihip_bdm_clusters_dev(h, dU.data_ptr() if given else None, ldu, U64(9), U64(2), 3, n, N, 1, n_events, da.data_ptr(),
                                          dd.data_ptr(), dt.data_ptr(), C.c_double(N), obs.ctypes.data, None, 0, None, None, None, 0,
                                          dD.data_ptr())
        assert rc == 0, lib.elfihip_last_error(h)
        hip_ctx.synchronize()
        D = dD.cpu().numpy()
        assert np.array_equal(D[:n], want[4], equal_nan=True) and np.all(D[n:] == guard)
    # the draws into the caller's memory
    dW = torch.full((n * ldu + 2,), guard, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    assert lib.elfihip_bdm_draws_dev(h, U64(9), U64(2), 3, n, n_events, dW.data_ptr(), ldu) == 0, lib.elfihip_last_error(h)
    hip_ctx.synchronize()
    W = dW.cpu().numpy()
    assert np.all(W[n * ldu:] == guard) and np.all(W[:n * ldu].reshape(n, ldu)[:, 2 * n_events:] == guard)
    assert np.array_equal(W[:n * ldu].reshape(n, ldu)[:, :2 * n_events], R.draws(9, 2, n, n_events, 3))


def test_library_refuses_what_it_cannot_hold(hip_ctx):
    import torch
    lib, h = hip_ctx.lib, hip_ctx.handle
    d = torch.full((4096,), 0.5, dtype=torch.float64, device='cuda')
    p, obs = d.data_ptr(), np.array([0.5])

    def call(first=0, n=2, N=20, mode=1, max_events=16, U=None, ldu=32, rates=(p, p, p), o=obs.ctypes.data, Cl=p + 1024, ldc=20,
             T=p + 2048, ldt=2, D=p + 4096):
        return lib.elfihip_bdm_clusters_dev(h, U, ldu, U64(0), U64(0), first, n, N, mode, max_events, *rates, C.c_double(20.0), o, Cl,
                                            ldc, None, None, T, ldt, D)
    assert call() == 0
    assert call(U=p + 8192) == 0
    hip_ctx.synchronize()
    for kw in (dict(n=0), dict(N=0), dict(N=4097), dict(mode=2), dict(mode=-1), dict(max_events=0), dict(max_events=2 ** 30 + 1),
               dict(first=-1), dict(first=2 ** 32 - 1), dict(rates=(p, None, p)), dict(o=None), dict(U=p + 8192, ldu=31),
               dict(ldc=19), dict(ldt=1)):
        assert call(**kw) != 0, kw
    assert call(o=None, D=None) == 0
    for args in ((0, 0, 8, p, 16), (0, 2, 0, p, 16), (0, 2, 8, None, 16), (0, 2, 8, p, 15), (-1, 2, 8, p, 16), (2 ** 32 - 1, 2, 8, p, 16)):
        assert lib.elfihip_bdm_draws_dev(h, U64(0), U64(0), *args) != 0, args
    hip_ctx.synchronize()


def _bdm_case(drawn):
    def case(d):
        import torch
        issues = []
        for which in (0, 1):
            n, N, n_events, alpha, delta, tau, U = _dev_inputs(which)
            issues.append((which, n, N, n_events, None if drawn else d.input(U), d.input(alpha), d.input(delta), d.input(tau),
                           d.host(np.array([0.55 + which])), d.out_raw(n * N, torch.int32), d.out_raw(n, torch.int32),
                           d.out_raw(n, torch.int64), d.out(n, 2), d.out(n)))
        d.go()
        for which, n, N, n_events, U, a, de, t, obs, Cl, st, ev, T, D in issues:
            d.call('elfihip_bdm_clusters_dev', d.cx, U.ptr if U else None, 2 * n_events, U64(17 + which), U64(which), 50 * which, n, N,
                   1, n_events, a.ptr, de.ptr, t.ptr, C.c_double(N), obs.ctypes.data, Cl.ptr, N, st.ptr, ev.ptr, T.ptr, 2, D.ptr,
                   host=(obs,))
        d.done()
    return case


def _draws_case(d):
    issues = [(which, 5, 24 + which, d.out(5 * 2 * (24 + which))) for which in (0, 1)]
    d.go()
    for which, n, n_events, U in issues:
        d.call('elfihip_bdm_draws_dev', d.cx, U64(5 + which), U64(2), 9 * which, n, n_events, U.ptr, 2 * n_events)
    d.done()


@pytest.mark.parametrize('name,case', [('bdm given', _bdm_case(False)), ('bdm drawn', _bdm_case(True)), ('bdm_draws', _draws_case)],
                         ids=['given', 'drawn', 'draws'])
def test_dev_entry_points_in_stream_order(hip_ctx, name, case):
    ref, got, d = SO.run_both(hip_ctx, case, name)
    SO.guards_intact(ref, d.guarded)
    SO.guards_intact(got, d.guarded)
    SO.assert_same(ref, got, name)
    assert d.still_busy, '%s: the stream was idle when the last call had returned: a call waited for the stream on the host' % name


# ---- 5. the distribution ----------------------------------------------------------------------------------------------------
def moments_z(a, b):
    """z of the difference of the means, and of the variances (the variance of a sample variance to first order: (m4 - v^2) / n),
    of two independent samples."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ma, mb, va, vb = a.mean(), b.mean(), a.var(ddof=1), b.var(ddof=1)
    sa = (np.mean((a - ma) ** 4) - va ** 2) / len(a)
    sb = (np.mean((b - mb) ** 4) - vb ** 2) / len(b)
    return (ma - mb) / np.sqrt(va / len(a) + vb / len(b)), (va - vb) / np.sqrt(sa + sb)


def test_distribution_of_the_devices_own_draws(hip_ctx, golden):
    """4096 device simulations at the example's truth against 4096 recorded runs of the reference binary: the means and the
    variances of the number of clusters and of the largest cluster within |z| <= 4, the bound of the other models'
    distribution tests.  (Two independent reference samples of that size: |z| <= 2.7, scripts/make_golden_bdm.py --check.)"""
    import elfi_amd
    Cl, st, ev = elfi_amd.bdm_clusters(np.full(4096, 0.2), 0.0, 0.198, N=20, mode=1, seed=1, stream=5, return_status=True)
    assert not st.any() and np.all(Cl.sum(axis=1) == 20)
    z = moments_z((Cl > 0).sum(axis=1), golden['dist_count']) + moments_z(Cl.max(axis=1), golden['dist_largest'])
    print('z of (clusters mean, clusters variance, largest mean, largest variance) = %s; events %d .. %d, mean %.1f'
          % (np.round(z, 2), ev.min(), ev.max(), ev.mean()))
    assert np.abs(z).max() <= 4


# ---- 6. through ELFI --------------------------------------------------------------------------------------------------------
def _reference():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi
    return elfi


def test_model_through_elfi(hip_ctx):
    elfi = _reference()
    import elfi_amd
    from elfi.examples import bdm
    m = elfi_amd.bdm_model()
    out = m.generate(5, outputs=['alpha', 'BDM', 'T1', 'd'], seed=2)
    assert out['BDM'].shape == (5, 20) and out['BDM'].dtype == np.int16 and out['T1'].shape == out['d'].shape == (5,)
    assert np.all((out['alpha'] >= .005) & (out['alpha'] <= 2.005)) and np.all(out['BDM'].sum(axis=1) == 20)
    assert np.array_equal(out['T1'], bdm.T1(out['BDM'])) and np.array_equal(out['d'], np.abs(out['T1'] - 11 / 20))
    res = elfi.Rejection(m['d'], batch_size=64, seed=1).sample(8, n_sim=192)
    assert res.samples['alpha'].shape == (8,) and np.isfinite(res.threshold) and np.all(np.isfinite(res.discrepancies))
    res = elfi_amd.HipRejection(m['d'], batch_size=64, seed=1).sample(8, n_sim=128)
    assert res.samples['alpha'].shape == (8,) and np.isfinite(res.threshold)
    # observed data from the device: one simulation with seed_obs
    m2 = elfi_amd.bdm_model(alpha=0.5, N=33, seed_obs=3)
    y = m2['BDM'].observed
    assert y.dtype == np.int16 and y.reshape(-1).shape == (33,) and y.sum() == 33
    assert np.array_equal(y, elfi_amd.bdm_model(alpha=0.5, N=33, seed_obs=3)['BDM'].observed)
    assert m2.generate(3, outputs=['BDM'], seed=1)['BDM'].shape == (3, 33)
