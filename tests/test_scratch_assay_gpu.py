"""GPU: the scratch-assay model of csrc/scratch_assay.hip against its NumPy statement (tests/assay_ref.py), which
tests/test_scratch_assay.py pins to recorded runs of ELFI's own example.  Every output is an integer or a bit: everything is
compared for EQUALITY.

  1. every recorded reference run through the kernel in the given form, on the draws its RandomState hands out
  2. the drawn form over shapes that straddle the slot loop's trip boundary (63, 64, 65 cells), the last lane's last bit and
     the transition to the full-grid skip (1023 of 1024 cells), one cell, one column: the echoed draws are the statement's, the
     result is the statement's on them, replay, a row moved by first_index, a batch against single calls
  3. a draw that is no draw ends its simulation alone (a checked branch; nothing is read out of bounds)
  4. the _dev forms at the caller's pitch between guard words, and on a busy adopted stream in stream order
  5. the distribution of the device's own draws against moments of reference runs recorded in the golden file
  6. the model through ELFI
"""
import ctypes as C
import os

import numpy as np
import pytest

import assay_ref as R
import stream_order as SO
from test_scratch_assay import SETS, replay

pytestmark = pytest.mark.gpu
U64 = C.c_uint64


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'scratch_assay.npz'))


def grid_with(nrows, ncols, n_cells, seed):
    g = np.zeros(nrows * ncols, dtype=np.uint8)
    g[np.random.RandomState(seed).permutation(nrows * ncols)[:n_cells]] = 1
    return g.reshape(nrows, ncols)


def time_of(n_iter, obs_every):
    """(obs_period, obs_interval, tau) that give exactly these integers"""
    return dict(obs_period=n_iter, obs_interval=obs_every, tau=1)


def same(got, want, what):
    for a, b, part in zip(got, want, ('S', 'frames', 'status', 'events')):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), '%s: %s differs' % (what, part)


# ---- 1. the recorded runs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SETS)
def test_recorded_runs_through_the_kernel(hip_ctx, golden, name):
    import elfi_amd
    p, init, _, S, frames, events, draws = replay(golden, name)
    t = golden[name + '_time']
    got = elfi_amd.scratch_assay_summaries(p[:, 0], p[:, 1], init, *t, draws=draws, return_frames=True, return_events=True)
    same(got, (S, frames, np.zeros(len(p), dtype=np.int32), events), name)
    assert np.array_equal(got[0], golden[name + '_S'])
    assert np.array_equal(R.pack_frames(got[1][:, :, :, -1:])[:, 0], golden[name + '_last'])


def test_an_empty_grid_stays_empty(hip_ctx, golden):
    import elfi_amd
    S, frames, status, events = elfi_amd.scratch_assay_summaries([0.5, 1.0], 0.5, np.zeros((3, 5)), **time_of(24, 2), seed=3,
                                                                 return_frames=True, return_events=True)
    assert np.array_equal(S, np.repeat(golden['empty_S'], 2, axis=0)) and not frames.any() and not status.any() and not events.any()


# ---- 2. the drawn form ------------------------------------------------------------------------------------------------------
#         grid      cells n_iter batch  pm, pp (None: drawn from U(0, 1), U(0, 0.2))
SHAPES = [((1, 1),    1,   4,    1, None),
          ((1, 2),    1,   8,    3, None),
          ((3, 5),    4,   24, 130, None),
          ((8, 8),   63,   6,    2, None),
          ((8, 8),   64,   6,    2, None),
          ((9, 8),   65,   6,    2, None),
          ((27, 36), 100, 288,   3, ([0.25, 0.5, 0.1], [0.002, 0.01, 0.03])),
          ((32, 32), 1023, 4,    2, ([0.9, 0.5], [1.0, 0.0005]))]


@pytest.mark.parametrize('grid,n_cells,n_iter,n,par', SHAPES, ids=['%dx%d_%d' % (s[0] + (s[1],)) for s in SHAPES])
def test_drawn_form(hip_ctx, grid, n_cells, n_iter, n, par):
    import elfi_amd
    init = grid_with(*grid, n_cells, n_cells)
    rs = np.random.RandomState(n_cells + n)
    pm, pp = (rs.uniform(0, 1, n), rs.uniform(0, 0.2, n)) if par is None else (np.array(par[0]), np.array(par[1]))
    obs_every = 2 if n_iter > 4 else 1
    seed, stream, first = 31, 6, 5
    kw = dict(time_of(n_iter, obs_every), return_frames=True, return_events=True)
    S, frames, events, status, nc = R.simulate_philox(pm, pp, init, n_iter, obs_every, seed, stream, first, n)
    want = (S, frames, status, events)
    got = elfi_amd.scratch_assay_summaries(pm, pp, init, seed=seed, stream=stream, first_index=first, **kw)
    same(got, want, 'drawn form')
    assert not status.any() and S.shape == (n, n_iter // obs_every + 1)
    if n_cells == 1023:
        assert S[0, -1] == 1024 and 0 in nc[0, 1:] and S[1, -1] < 1024          # one fills and skips, one does not
    # the echoed draws are the statement's, and the given form on them is the drawn form
    draws = elfi_amd.scratch_assay_draws(nc, init.size, seed=seed, stream=stream, first_index=first)
    for a, b in zip(draws, R.philox_draws(seed, stream, first, nc, init.size)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    same(elfi_amd.scratch_assay_summaries(pm, pp, init, draws=draws, **kw), want, 'given form on the echoed draws')
    # replay
    same(elfi_amd.scratch_assay_summaries(pm, pp, init, seed=seed, stream=stream, first_index=first, **kw), got, 'replay')
    # a row moved by first_index is the row moved by position
    moved = elfi_amd.scratch_assay_summaries(pm[-1:], pp[-1:], init, seed=seed, stream=stream, first_index=first + n - 1, **kw)
    same(moved, [a[-1:] for a in got], 'first_index')
    if n >= 100:         # which wavefront ran which simulation does not enter the result
        for i in range(n):
            one = elfi_amd.scratch_assay_summaries(pm[i], pp[i], init, seed=seed, stream=stream, first_index=first + i, **kw)
            same(one, [a[i:i + 1] for a in got], 'single call %d' % i)
    # another stream: other draws
    if n_cells < grid[0] * grid[1] and n_iter > 4:
        other = elfi_amd.scratch_assay_summaries(pm, pp, init, seed=seed, stream=stream + 1, first_index=first, **kw)
        assert not np.array_equal(other[1], got[1])


# ---- 3. a draw that is no draw ----------------------------------------------------------------------------------------------
def test_bad_draws_end_their_simulation_alone(hip_ctx):
    import elfi_amd
    init = grid_with(3, 5, 4, 1)
    rs = np.random.RandomState(3)
    runs = [R.from_random_state(0.5, 0.05, init, rs, 24, 2) for _ in range(3)]
    Cd, P, M = (np.stack([r[3][j] for r in runs]) for j in range(3))
    kw = dict(time_of(24, 2), return_frames=True, return_events=True)
    good = elfi_amd.scratch_assay_summaries(0.5, 0.05, init, draws=(Cd, P, M), **kw)
    assert not good[2].any()
    C2, M2 = Cd.copy(), M.copy()
    C2[1, 0, 0, 2] = 4                      # == num_cells
    M2[1, 3, 1, 0] = 4
    for Cx, Mx in ((C2, M), (Cd, M2), (C2, M2)):
        S, frames, status, events = elfi_amd.scratch_assay_summaries(0.5, 0.05, init, draws=(Cx, P, Mx), **kw)
        Sw, fw, ew, stw = R.simulate(0.5, 0.05, init, Cx, P, Mx, 24, 2)
        same((S, frames, status, events), (Sw, fw, stw, ew), 'bad draw')
        assert status.tolist() == [R.OK, R.BAD_DRAW, R.OK] and np.isnan(S[1]).all()
        for a, b in zip((S, frames, status, events), good):
            assert np.array_equal(a[[0, 2]], b[[0, 2]])
    C3 = Cd.copy()
    C3[:, :, :, 14] = -7                    # a slot past every cell count the runs reach: never read
    C3[1, 0, 0, 4] = 1 << 30                # past num_cells = 4 in that row
    same(elfi_amd.scratch_assay_summaries(0.5, 0.05, init, draws=(C3, P, M), **kw), good, 'entries past num_cells')


# ---- 4. the _dev forms ------------------------------------------------------------------------------------------------------
def _dev_inputs(which):
    init = grid_with(5, 9, 12, 40 + which)
    n, n_iter, obs_every = 5, 24, 4 + which
    rs = np.random.RandomState(600 + which)
    pm, pp = rs.uniform(0, 1, n), rs.uniform(0, 0.2, n)
    runs = [R.from_random_state(pm[i], pp[i], init, rs, n_iter, obs_every) for i in range(n)]
    draws = [np.stack([r[3][j] for r in runs]) for j in range(3)]
    return init, n, n_iter, obs_every, pm, pp, draws


def test_dev_forms_at_the_callers_pitch(hip_ctx):
    import torch
    import elfi_amd
    init, n, n_iter, obs_every, pm, pp, draws = _dev_inputs(0)
    n_obs, pad, guard = n_iter // obs_every, 3, -7.0625e300
    kw = dict(time_of(n_iter, obs_every), return_frames=True, return_events=True)
    lib, h = hip_ctx.lib, hip_ctx.handle
    dpm, dpp = (torch.from_numpy(a).cuda() for a in (pm, pp))
    dd = [torch.from_numpy(a).cuda() for a in draws]
    for given in (True, False):
        want = elfi_amd.scratch_assay_summaries(pm, pp, init, draws=draws if given else None, seed=9, stream=2, first_index=3, **kw)
        lds = n_obs + 1 + pad
        dS = torch.full((2 + n * lds + 8,), guard, dtype=torch.float64, device='cuda')           # guard words before and after
        dst = torch.full((n + 2,), -7, dtype=torch.int32, device='cuda')
        dev = torch.full((2 * n + 2,), -7, dtype=torch.int64, device='cuda')
        dfr = torch.full((n * (n_obs + 1) * 32 + 2,), -7, dtype=torch.int32, device='cuda')
        torch.cuda.synchronize()
        rc = lib.elfihip_assay_summaries_dev(h, *[(t.data_ptr() if given else None) for t in dd], U64(9), U64(2), 3, n, *init.shape,
                                             n_iter, obs_every, init.ctypes.data, dpm.data_ptr(), dpp.data_ptr(),
                                             dS.data_ptr() + 16, lds, dst.data_ptr(), dev.data_ptr(), dfr.data_ptr())
        assert rc == 0, lib.elfihip_last_error(h)
        hip_ctx.synchronize()
        S, st, ev, fr = dS.cpu().numpy(), dst.cpu().numpy(), dev.cpu().numpy(), dfr.cpu().numpy()
        rows = S[2:2 + n * lds].reshape(n, lds)
        assert np.all(S[:2] == guard) and np.all(S[2 + n * lds:] == guard) and np.all(rows[:, n_obs + 1:] == guard)
        assert np.all(st[n:] == -7) and np.all(ev[2 * n:] == -7) and np.all(fr[-2:] == -7)
        frames = R.pack_frames(want[1]).view(np.int32)
        assert np.array_equal(rows[:, :n_obs + 1], want[0]) and np.array_equal(st[:n], want[2])
        assert np.array_equal(ev[:2 * n].reshape(n, 2), want[3]) and np.array_equal(fr[:-2].reshape(frames.shape), frames)
        # only S is asked for
        dS.fill_(guard)
        torch.cuda.synchronize()
        rc = lib.elfihip_assay_summaries_dev(h, *[(t.data_ptr() if given else None) for t in dd], U64(9), U64(2), 3, n, *init.shape,
                                             n_iter, obs_every, init.ctypes.data, dpm.data_ptr(), dpp.data_ptr(),
                                             dS.data_ptr() + 16, lds, None, None, None)
        assert rc == 0, lib.elfihip_last_error(h)
        hip_ctx.synchronize()
        assert np.array_equal(dS.cpu().numpy()[2:2 + n * lds].reshape(n, lds)[:, :n_obs + 1], want[0])
    # the draws into the caller's memory
    nc = R.simulate_philox(pm, pp, init, n_iter, obs_every, 9, 2, 3, n)[4]
    total = nc.size * init.size
    dnc = torch.from_numpy(nc).cuda()
    dC = torch.full((total + 2,), -7, dtype=torch.int32, device='cuda')
    dP = torch.full((total + 2,), -7.0, dtype=torch.float64, device='cuda')
    dM = torch.full((total + 2,), 0xA5, dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    rc = lib.elfihip_assay_draws_dev(h, U64(9), U64(2), 3, n, n_iter, init.size, dnc.data_ptr(), dC.data_ptr(), dP.data_ptr(), dM.data_ptr())
    assert rc == 0, lib.elfihip_last_error(h)
    hip_ctx.synchronize()
    for d, w in zip((dC, dP, dM), elfi_amd.scratch_assay_draws(nc, init.size, seed=9, stream=2, first_index=3)):
        a = d.cpu().numpy()
        assert np.array_equal(a[:total], w.reshape(-1)) and np.all(a[total:] == a[-1]) and a[-1] in (-7, 0xA5)


def test_library_refuses_what_it_cannot_hold(hip_ctx):
    import torch
    lib, h = hip_ctx.lib, hip_ctx.handle
    init = grid_with(3, 5, 4, 1)
    d = torch.zeros(64, dtype=torch.float64, device='cuda')
    p = d.data_ptr()

    def call(first=0, n=2, nrows=3, ncols=5, n_iter=4, obs_every=2, grid=init, draws=(None, None, None), lds=3, S=p + 256):
        return lib.elfihip_assay_summaries_dev(h, *draws, U64(0), U64(0), first, n, nrows, ncols, n_iter, obs_every,
                                               grid.ctypes.data if grid is not None else None, p, p, S, lds, None, None, None)
    assert call() == 0
    hip_ctx.synchronize()
    two = np.full((3, 5), 2, dtype=np.uint8)
    for kw in (dict(n=0), dict(nrows=0), dict(nrows=33, ncols=32), dict(n_iter=0), dict(n_iter=(1 << 21) + 1), dict(obs_every=0),
               dict(obs_every=5), dict(first=-1), dict(first=2 ** 32 - 1), dict(grid=None), dict(grid=two), dict(draws=(p, None, None)),
               dict(draws=(p, p, None)), dict(lds=2), dict(S=None)):
        assert call(**kw) != 0, kw
    assert lib.elfihip_assay_draws_dev(h, U64(0), U64(0), 0, 1, 4, 1025, p, p, p, p) != 0
    assert lib.elfihip_assay_draws_dev(h, U64(0), U64(0), 0, 1, 4, 15, None, p, p, p) != 0
    hip_ctx.synchronize()


def _assay_case(drawn):
    def case(d):
        import torch
        issues = []
        for which in (0, 1):
            init, n, n_iter, obs_every, pm, pp, draws = _dev_inputs(which)
            n_obs = n_iter // obs_every
            dd = [None] * 3 if drawn else [d.input(a) for a in draws]
            dpm, dpp, grid = d.input(pm), d.input(pp), d.host(init)
            S, st = d.out(n, n_obs + 1), d.out_raw(n, torch.int32)
            ev, fr = d.out_raw(2 * n, torch.int64), d.out_raw(n * (n_obs + 1) * 32, torch.int32)
            issues.append((dd, which, n, init.shape, n_iter, obs_every, grid, dpm, dpp, S, n_obs + 1, st, ev, fr))
        d.go()
        for dd, which, n, shape, n_iter, obs_every, grid, dpm, dpp, S, lds, st, ev, fr in issues:
            d.call('elfihip_assay_summaries_dev', d.cx, *[b.ptr if b else None for b in dd], U64(17 + which), U64(which), 50 * which,
                   n, *shape, n_iter, obs_every, grid.ctypes.data, dpm.ptr, dpp.ptr, S.ptr, lds, st.ptr, ev.ptr, fr.ptr, host=(grid,))
        d.done()
    return case


def _draws_case(d):
    import torch
    issues = []
    for which in (0, 1):
        n, n_iter, cells = 5, 24 + which, 45
        nc = np.random.RandomState(620 + which).randint(0, cells + 1, (n, n_iter, 2)).astype(np.int32)
        total = nc.size * cells
        issues.append((which, n, n_iter, cells, d.input(nc), d.out_raw(total, torch.int32), d.out(total), d.out_raw(total, torch.uint8)))
    d.go()
    for which, n, n_iter, cells, nc, Cd, P, M in issues:
        d.call('elfihip_assay_draws_dev', d.cx, U64(5 + which), U64(2), 9 * which, n, n_iter, cells, nc.ptr, Cd.ptr, P.ptr, M.ptr)
    d.done()


@pytest.mark.parametrize('name,case', [('assay given', _assay_case(False)), ('assay drawn', _assay_case(True)),
                                       ('assay_draws', _draws_case)], ids=['given', 'drawn', 'draws'])
def test_dev_entry_points_in_stream_order(hip_ctx, name, case):
    ref, got, d = SO.run_both(hip_ctx, case, name)
    SO.guards_intact(ref, d.guarded)
    SO.guards_intact(got, d.guarded)
    SO.assert_same(ref, got, name)
    assert d.still_busy, '%s: the stream was idle when the last call had returned: a call waited for the stream on the host' % name


# ---- 5. the distribution ----------------------------------------------------------------------------------------------------
def test_distribution_of_the_devices_own_draws(hip_ctx, golden):
    """256 device simulations per point at seed 1 against the mean and SD of 64 recorded reference runs, five statistics
    (assay_ref.moments): z = (device mean - reference mean) / (reference SD sqrt(1 / 256 + 1 / 64)), |z| < 4 -- the bound
    of the toad and stochastic-volatility distribution tests."""
    import elfi_amd
    init, worst = golden['true_init'], 0.0
    for j, (pm, pp) in enumerate(golden['moment_points']):
        S = elfi_amd.scratch_assay_summaries(np.full(256, pm), pp, init, seed=1, stream=j)
        z = (R.moments(S).mean(axis=0) - golden['moment_mean'][j]) / (golden['moment_sd'][j] * np.sqrt(1 / 256 + 1 / 64))
        print('pm = %g, pp = %g: z of (count, sum ds, ds[0], ds[71], ds[143]) = %s' % (pm, pp, np.round(z, 2)))
        worst = max(worst, np.abs(z).max())
    print('largest |z| %.2f' % worst)
    assert worst < 4


# ---- 6. through ELFI --------------------------------------------------------------------------------------------------------
def _reference():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi
    return elfi


def test_model_through_elfi(hip_ctx):
    _reference()
    import elfi_amd
    m = elfi_amd.scratch_assay_model(seed_obs=1)
    out = m.generate(3, outputs=['pm', 'pp', 'sim', 'sums', 'd'], seed=2)
    assert out['sim'].shape == out['sums'].shape == (3, 145) and out['d'].shape == (3,) and np.array_equal(out['sim'], out['sums'])
    assert np.all((out['pm'] >= 0) & (out['pm'] <= 1) & (out['pp'] >= 0) & (out['pp'] <= 1))
    assert np.all(out['sums'] == np.floor(out['sums'])) and np.all(out['sums'][:, -1] >= 100) and np.all(np.isfinite(out['d']))
    w = np.concatenate((np.ones(144) / 144, [1])) / 100 ** 2
    want = np.sqrt(np.sum(w * (out['sums'] - m['sums'].observed) ** 2, axis=1))
    assert np.all(np.abs(out['d'] - want) <= 1e-12 * want)
    res = elfi_amd.HipRejection(m['d'], batch_size=64, seed=1).sample(8, n_sim=128)
    assert res.samples['pm'].shape == res.samples['pp'].shape == (8,) and np.all(np.isfinite(res.discrepancies))
