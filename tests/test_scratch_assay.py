"""CPU: the NumPy statement of the scratch-assay model (tests/assay_ref.py) reproduces recorded runs of ELFI's own example
(tests/golden/scratch_assay.npz, scripts/make_golden_scratch_assay.py) exactly -- every summary and the last frame, from a
RandomState consumed in the reference's order and again from the slot-keyed draws that replay hands back; cell_summaries is
the statement's reduction of the frames; the draw layout is the documented one; the model graph has the reference's nodes,
priors, weights and observed shape; and the device functions refuse bad arguments before any device context exists."""
import os

import numpy as np
import pytest

import assay_ref as R
import philox_ref

SETS = ['true', 'prior', 'pm_one', 'pp_one', 'pm_nan', 'pm_big', 'g3x5', 'g1x1', 'g1x7', 'g32x32', 'ragged', 'one_iter']


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'scratch_assay.npz'))


def replay(g, name):
    """every simulation of a recorded set from its seed -> (params, init, (n_iter, obs_every), S, frames, events, (C, P, M))"""
    init, (n_iter, obs_every, _) = g[name + '_init'], R.shape(*g[name + '_time'])
    runs = [R.from_random_state(pm, pp, init, np.random.RandomState(seed), n_iter, obs_every)
            for (pm, pp), seed in zip(g[name + '_params'], g[name + '_seed'])]
    draws = tuple(np.stack([r[3][j] for r in runs]) for j in range(3))
    return (g[name + '_params'], init, (n_iter, obs_every), np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs]),
            np.stack([r[2] for r in runs]), draws)


def test_the_recorded_sets_are_the_ones_the_issue_asks_for(golden):
    g = golden
    assert list(g['sets']) == SETS
    assert g['true_init'].shape == (27, 36) and g['true_init'].sum() == 100 and np.all(g['true_params'] == [0.25, 0.002])
    assert g['true_S'].shape == (1, 145) and g['prior_S'].shape == (4, 145)
    assert np.all(g['pm_one_params'] == [1, 0]) and g['pm_one_S'][0, -1] == 100
    assert np.all(g['pp_one_params'] == [0, 1]) and g['pp_one_S'][0, -1] == 972           # the grid fills: the skip branch
    assert np.isnan(g['pm_nan_params'][0, 0]) and g['pm_big_params'][0, 0] == 1.5
    assert g['g3x5_init'].shape == (3, 5) and g['g3x5_init'].sum() == 4 and not g['g3x5_init'][2].any()
    assert g['g1x1_init'].tolist() == [[1]] and g['g1x7_init'].shape == (1, 7)
    assert g['g32x32_init'].sum() == 1023 and g['g32x32_S'][:, -1].tolist() == [1024, 1023]
    assert R.shape(*g['ragged_time']) == (24, 4, 6) and R.shape(*g['one_iter_time']) == (1, 1, 1)
    assert R.shape() == (288, 2, 144)
    assert not g['empty_raises'] and not g['empty_S'].any()             # the reference runs an empty grid: it stays empty
    assert g['moment_mean'].shape == g['moment_sd'].shape == (2, 5) and g['moment_runs'] == 64
    assert g['moment_points'].tolist() == [[0.25, 0.002], [0.6, 0.01]]


@pytest.mark.parametrize('name', SETS)
def test_statement_is_the_recorded_run(golden, name):
    g = golden
    p, init, (n_iter, obs_every), S, frames, events, (C, P, M) = replay(g, name)
    assert S.dtype == np.float64 and S.shape == g[name + '_S'].shape and np.array_equal(S, g[name + '_S'])
    assert np.array_equal(R.pack_frames(frames[:, :, :, -1:])[:, 0], g[name + '_last'])
    assert np.array_equal(frames[:, :, :, 0], np.broadcast_to(init, frames.shape[:3]))
    # the summaries are cell_summaries of the frames
    assert np.array_equal(R.summaries(frames), S)
    # the slot-keyed draws that the replay hands back give the same run through the given form
    S2, frames2, events2, status = R.simulate(p[:, 0], p[:, 1], init, C, P, M, n_iter, obs_every)
    assert np.array_equal(S2, S) and np.array_equal(frames2, frames) and np.array_equal(events2, events) and not status.any()
    assert np.all(C >= 0) and np.all(M <= 3) and events.dtype == np.int64


def test_an_empty_grid_stays_empty(golden):
    S, frames, events, (C, P, M) = R.from_random_state(0.5, 0.5, np.zeros((3, 5)), np.random.RandomState(40413), 24, 2)
    assert np.array_equal(S[None], golden['empty_S']) and not frames.any() and not events.any()


def test_statement_marks_a_draw_that_is_no_draw():
    rs = np.random.RandomState(3)
    init = np.zeros((3, 5), dtype=np.uint8)
    init[0, :4] = 1
    runs = [R.from_random_state(0.5, 0.05, init, rs, 24, 2) for _ in range(3)]
    C, P, M = (np.stack([r[3][j] for r in runs]) for j in range(3))
    good = R.simulate(0.5, 0.05, init, C, P, M, 24, 2)
    C2, M2 = C.copy(), M.copy()
    C2[1, 0, 0, 2] = 4                      # == num_cells
    M2[1, 3, 1, 0] = 4
    for Cx, Mx in ((C2, M), (C, M2), (C2, M2)):
        S, frames, events, status = R.simulate(0.5, 0.05, init, Cx, P, Mx, 24, 2)
        assert status.tolist() == [R.OK, R.BAD_DRAW, R.OK] and np.isnan(S[1]).all() and not frames[1].any() and not events[1].any()
        for a, b in zip((S, frames, events), good):
            assert np.array_equal(a[[0, 2]], b[[0, 2]])
    C3 = C.copy()
    C3[1, 0, 0, 4] = -7                     # past num_cells = 4: never read
    assert np.array_equal(R.simulate(0.5, 0.05, init, C3, P, M, 24, 2)[0], good[0])


def test_draw_layout():
    """Counter packing, the candidate from multiply-high, the uniform from words 1 and 2, the direction from the top of word 3."""
    seed, stream, g, t, f, nc = 0x123456789, (7 << 32) | 5, 41, 287, 1, 972
    C, P, M = R.philox_phase(seed, stream, g, t, f, nc)
    assert C.dtype == np.int32 and P.dtype == np.float64 and M.dtype == np.uint8 and C.shape == (nc,)
    for k in (0, 1, 63, 64, 971):
        w = philox_ref.philox4x32_10((((2 * t + f) << 10) | k, g, 5, 7), (0x23456789, 0x1))
        assert C[k] == (w[0] * nc) >> 32 and P[k] == ((w[1] << 21) | (w[2] >> 11)) * 2.0 ** -53 and M[k] == w[3] >> 30
    assert np.all((C >= 0) & (C < nc)) and np.all((P >= 0) & (P < 1)) and set(M.tolist()) == {0, 1, 2, 3}
    # the candidate alone depends on the number of slots
    C2, P2, M2 = R.philox_phase(seed, stream, g, t, f, 100)
    assert np.array_equal(P2, P[:100]) and np.array_equal(M2, M[:100]) and np.all(C2 < 100)
    # a slot, a phase, an iteration and a simulation each have their own counter
    base = R.philox_phase(3, 0, 2, 5, 0, 64)[1]
    for other in (R.philox_phase(3, 0, 2, 5, 1, 64), R.philox_phase(3, 0, 2, 6, 0, 64), R.philox_phase(3, 0, 3, 5, 0, 64),
                  R.philox_phase(4, 0, 2, 5, 0, 64), R.philox_phase(3, 1, 2, 5, 0, 64)):
        assert not np.any(other[1] == base)
    assert ((2 * ((1 << 21) - 1) + 1) << 10 | 1023) < 1 << 32          # the largest counter word fits
    # the drawn form as arrays is the lazy one: the statement on philox_draws is simulate_philox
    init = np.zeros((3, 5), dtype=np.uint8)
    init[1, 1:5] = 1
    S, frames, events, status, nc = R.simulate_philox([0.5, 0.9], 0.1, init, 24, 2, 11, 3, 7, 2)
    C, P, M = R.philox_draws(11, 3, 7, nc, 15)
    assert nc.shape == (2, 24, 2) and nc[:, 0].tolist() == [[4, 4], [4, 4]] and nc.max() <= 15
    for a, b in zip(R.simulate([0.5, 0.9], 0.1, init, C, P, M, 24, 2), (S, frames, events, status)):
        assert np.array_equal(a, b)
    assert np.array_equal(R.simulate_philox(0.9, 0.1, init, 24, 2, 11, 3, 8, 1)[0][0], S[1])     # first_index moves the row


def test_row_of_a_cell_by_multiplication():
    pos = np.arange(1024)
    for ncols in range(1, 1025):
        assert np.array_equal((pos * R.magic(ncols)) >> 20, pos // ncols)


def test_pack_frames_layout():
    fr = np.zeros((1, 5, 9, 2), dtype=np.uint8)
    fr[0, 3, 7, 1] = fr[0, 0, 0, 0] = 1                    # cell 34 -> bit 2 of word 1
    W = R.pack_frames(fr)
    assert W.shape == (1, 2, 32) and W.dtype == np.uint32 and W[0, 0, 0] == 1 and W[0, 1, 1] == 4 and W.sum() == 5


@pytest.mark.reference
def test_statement_is_the_reference_on_a_fresh_run_and_model_graph():
    import ref_shim
    if not ref_shim.available():
        pytest.skip('reference ELFI not available')
    ref_shim.install()
    import elfi_amd
    from elfi.examples import scratch_assay as sa
    init = sa._random_init(4, 6, 7, 2, np.random.RandomState(1))
    x = sa.cell_sim(0.7, 0.03, init, None, 2, 1 / 12, 1 / 24, random_state=np.random.RandomState(5))
    S, frames, _, _ = R.from_random_state(0.7, 0.03, init, np.random.RandomState(5), *R.shape(2, 1 / 12, 1 / 24)[:2])
    assert np.array_equal(frames, x) and np.array_equal(S, sa.cell_summaries(x[None])[0])
    assert np.array_equal(R.summaries(x[None]), sa.cell_summaries(x[None]))
    # the graph: the reference's node names, priors, weights and observed summaries
    m, ref = elfi_amd.scratch_assay_model(seed_obs=4), sa.get_model(seed_obs=4)
    public = [sorted(k for k in mdl.nodes if not k.startswith('_')) for mdl in (m, ref)]
    assert public[0] == public[1] == sorted(['pm', 'pp', 'sim', 'sums', 'd'])
    assert m.parameter_names == ref.parameter_names == ['pm', 'pp']
    assert m['sums'].observed.shape == ref['sums'].observed.shape == (1, 145)
    assert np.array_equal(m['sums'].observed, ref['sums'].observed) and np.array_equal(m['sim'].observed, ref['sums'].observed)
    assert m.get_parents('d') == ['sums'] and m.get_parents('sums') == ['sim'] and m.get_parents('sim')[:2] == ['pm', 'pp']
    for name in ('pm', 'pp'):                       # U(0, 1): loc 0, scale 1 as Constant parents, the uniform distribution
        for mdl in (m, ref):
            assert [mdl[p].state['attr_dict']['_output'] for p in mdl.get_parents(name)] == [0, 1]
        assert m[name].distribution is elfi_amd.priors.uniform and ref[name].state['attr_dict']['distribution'] == 'uniform'
    w = m['d'].state['attr_dict']['_operation'].args[0].w
    w_ref = ref['d'].state['attr_dict']['_operation'].args[0].keywords['w']
    assert w.shape == (145,) and np.array_equal(w, w_ref)
    assert np.array_equal(w, np.concatenate((np.ones(144) / 144, np.array([1]))) / 100 ** 2)
    # an initial grid of the caller's, and the host-side priors
    m2 = elfi_amd.scratch_assay_model(true_params=[0.5, 0.05], init_arr=init, seed_obs=2, device_priors=False)
    r2 = sa.get_model(true_params=[0.5, 0.05], init_arr=init, seed_obs=2)
    assert np.array_equal(m2['sums'].observed, r2['sums'].observed)


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    init = np.zeros((3, 5))
    init[0, :3] = 1
    p = np.full(4, 0.5)
    d = (np.zeros((4, 288, 2, 15), dtype=np.int32), np.zeros((4, 288, 2, 15)), np.zeros((4, 288, 2, 15), dtype=np.uint8))
    bad = [dict(init_arr=np.zeros(15)), dict(init_arr=np.zeros((33, 32))), dict(init_arr=np.zeros((0, 4))), dict(init_arr=init * 2),
           dict(init_arr=np.full((3, 5), np.nan)), dict(tau=0.), dict(tau=np.nan), dict(tau=13.), dict(obs_interval=0.01),
           dict(obs_interval=13.), dict(obs_period=1e6), dict(first_index=-1), dict(first_index=2 ** 32 - 3),
           dict(draws=(d[0], d[1][:3], d[2])), dict(draws=(d[0][:, :287], d[1][:, :287], d[2][:, :287])),
           dict(draws=(d[0][..., :14], d[1][..., :14], d[2][..., :14])), dict(draws=(d[0][0], d[1][0], d[2][0]))]
    for kw in bad:
        args = dict(dict(init_arr=init), **kw)
        with pytest.raises(ValueError):
            elfi_amd.scratch_assay_summaries(p, p, **args)
    with pytest.raises(ValueError):
        elfi_amd.scratch_assay_summaries(p, np.zeros(3), init)              # a parameter of another batch size
    nc = np.full((2, 24, 2), 4, dtype=np.int32)
    for args, kw in (((nc, 0), {}), ((nc, 1025), {}), ((nc, 3), {}), ((-nc, 15), {}), ((nc[0], 15), {}), ((nc[:0], 15), {}),
                     ((nc, 15), dict(first_index=-1)), ((nc, 15), dict(first_index=2 ** 32 - 1))):
        with pytest.raises(ValueError):
            elfi_amd.scratch_assay_draws(*args, **kw)
    with pytest.raises(ValueError):
        elfi_amd.scratch_assay_model(true_params=[0.25])
    assert elfi_amd.scratch_assay_shape() == (288, 2, 144) and elfi_amd.scratch_assay_shape(1, 1 / 5, 1 / 24) == (24, 4, 6)


def test_library_refuses_bad_limits_without_a_device():
    """The C entry points check their arguments before they touch the device: a NULL context is refused, never a crash."""
    import elfi_amd
    lib = elfi_amd.load_library()
    assert lib.elfihip_assay_summaries(None, None, None, None, 0, 0, 0, 1, 27, 36, 288, 2, *([None] * 7)) != 0
    assert lib.elfihip_assay_summaries_dev(None, None, None, None, 0, 0, 0, 1, 27, 36, 288, 2, *([None] * 4), 145, None, None, None) != 0
    assert lib.elfihip_assay_draws(None, 0, 0, 0, 1, 24, 15, None, None, None, None) != 0
    assert lib.elfihip_assay_draws_dev(None, 0, 0, 0, 1, 24, 15, None, None, None, None) != 0
