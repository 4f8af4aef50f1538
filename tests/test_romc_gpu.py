"""GPU: ROMC on the device (csrc/romc.hip through elfi_amd/romc.py) against the NumPy statements of tests/romc_ref.py, which
tests/test_romc.py pins to SciPy and to the reference.

Everything that is the same arithmetic must be equal bit for bit: the objective (against the fused MA2 distance squared and
the statement), Nelder-Mead and the Hessian, the rotation, the limits and the evaluation counts of the line searches, the
indicator counts, the device-pointer forms against the host forms.  The sampler's points go through a different but
equivalent order of roundings on the host side of the comparison only where the test says so (2 ulp per term).
n_obs = 8, 100 and 126 hit the fewer-than-eight-terms, tail and longest branches of the pairwise sums.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import device_layout as DL
import philox_ref as PH
import romc_ref as R
import stream_order as SO

ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle')
sys.path.insert(0, ORACLE)
import ref_shim  # noqa: E402

pytestmark = pytest.mark.gpu
needs_reference = pytest.mark.skipif(not ref_shim.available(), reason='no reference package (run oracle/make_ref.sh)')

OBS = (0.35, 0.05)
N_OBS = (8, 100, 126)
N1 = 32
EPS_REGION = 0.01      # a distance of 0.1 (the minimal values themselves are zero up to the simplex tolerance)
DBL, U64 = C.c_double, C.c_uint64
_cache = {}


def _same(a, b):
    """Bit for bit, NaNs included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _starts(n, seed):
    rs = np.random.RandomState(seed)
    return np.column_stack((rs.uniform(-1.5, 1.5, n), rs.uniform(-1, 1, n)))


def setup(n_obs):
    """Noise, starts and the statement's solutions of N1 problems, computed once per n_obs and left unchanged."""
    if n_obs not in _cache:
        W = R.make_noise(N1, n_obs, 900 + n_obs)
        x0 = _starts(N1, 901 + n_obs)
        x0[2, 1] = 0.0
        want = R.solve(W, OBS, x0)
        for a in (W, x0) + tuple(want.values()):
            a.setflags(write=False)
        _cache[n_obs] = (W, x0, want)
    return _cache[n_obs]


@pytest.fixture(scope='module')
def problems(hip_ctx):
    import elfi_amd
    made = {n_obs: elfi_amd.RomcProblems(n_obs, OBS, W=setup(n_obs)[0]) for n_obs in N_OBS}
    yield made
    for p in made.values():
        p.free()


def _pairs(P, n1, seed):
    rs = np.random.RandomState(seed)
    theta = np.column_stack((rs.uniform(-2, 2, P), rs.uniform(-1.25, 1.25, P)))
    prob = rs.randint(0, n1, P)
    prob[:3] = [n1 - 1, 0, n1 - 1]
    return theta, prob


# ---- objective --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_obs', N_OBS)
def test_objective_on_given_noise(hip_ctx, n_obs):
    import elfi_amd
    W = setup(n_obs)[0][:16]
    theta, prob = _pairs(200, 16, n_obs)
    p = elfi_amd.RomcProblems(n_obs, OBS, W=W)
    try:
        f = elfi_amd.romc_objective(p, theta, prob)
    finally:
        p.free()
    _, _, D = elfi_amd.ma2_distance(W[prob], theta[:, 0], theta[:, 1], OBS)
    assert _same(f, D * D), 'not the square of the fused MA2 distance'
    assert _same(f, R.objective_rows(W[prob], theta[:, 0], theta[:, 1], OBS)), 'not the NumPy statement'


@pytest.mark.parametrize('n_obs', N_OBS)
def test_objective_on_drawn_noise(hip_ctx, n_obs):
    import elfi_amd
    rs = np.random.RandomState(n_obs)
    seeds = rs.randint(0, 2 ** 31 - 1, 16).astype(np.uint64)
    streams = np.full(16, elfi_amd.priors.SIMULATOR_STREAM_BASE, dtype=np.uint64)
    streams[5:9] += np.arange(4, dtype=np.uint64) << np.uint64(33)
    seeds[9] += np.uint64(2 ** 40)
    theta, prob = _pairs(200, 16, n_obs + 1)
    p = elfi_amd.RomcProblems(n_obs, OBS, seeds=seeds, streams=streams)
    try:
        f = elfi_amd.romc_objective(p, theta, prob)
    finally:
        p.free()
    want = np.empty(200)
    for k in range(200):
        i = prob[k]
        want[k] = elfi_amd.ma2_draw_distance(theta[k, 0], theta[k, 1], OBS, n_obs=n_obs, seed=int(seeds[i]), stream=int(streams[i]))[2][0]
    assert _same(f, want * want)


def test_objective_rejects_a_problem_that_does_not_exist(hip_ctx, problems):
    import elfi_amd
    with pytest.raises(ValueError, match='outside'):
        elfi_amd.romc_objective(problems[8], [[0.1, 0.2]], [N1])


# ---- solve ------------------------------------------------------------------------------------------------------------------
def _assert_solution(got, want, rows=slice(None)):
    for key in ('x_min', 'f_min', 'hess', 'nfev', 'nit', 'status'):
        assert _same(got[key], want[key][rows]), key


@pytest.mark.parametrize('n_obs', N_OBS)
def test_solve_is_the_statement(hip_ctx, problems, n_obs):
    import elfi_amd
    W, x0, want = setup(n_obs)
    got = elfi_amd.romc_solve(problems[n_obs], x0)
    print('n_obs %d: solved %d of %d, nfev %d..%d' % (n_obs, np.sum(got['status'] == R.SOLVED), N1, got['nfev'].min(), got['nfev'].max()))
    assert np.sum(want['status'] == R.SOLVED) >= N1 // 2
    _assert_solution(got, want)


@pytest.mark.parametrize('n_obs', N_OBS)
def test_solve_with_an_iteration_limit(hip_ctx, problems, n_obs):
    import elfi_amd
    W, x0, _ = setup(n_obs)
    got = elfi_amd.romc_solve(problems[n_obs], x0, maxiter=5)
    want = R.solve(W, OBS, x0, maxiter=5)
    assert np.all(want['status'] == R.MAXITER) and np.all(np.isnan(got['hess']))
    _assert_solution(got, want)


def test_solve_with_an_evaluation_limit(hip_ctx, problems):
    import elfi_amd
    W, x0, _ = setup(100)
    for maxfev in (2, 37):
        got = elfi_amd.romc_solve(problems[100], x0, maxfev=maxfev)
        want = R.solve(W, OBS, x0, maxfev=maxfev)
        assert np.all(want['status'] == R.MAXFEV)
        _assert_solution(got, want)


@pytest.mark.parametrize('n1', [1, 5])
def test_solve_few_problems_and_a_value_that_is_not_finite(hip_ctx, n1):
    import elfi_amd
    W, x0, want = setup(100)
    p = elfi_amd.RomcProblems(100, OBS, W=W[:n1])
    try:
        _assert_solution(elfi_amd.romc_solve(p, x0[:n1]), want, slice(0, n1))
        bad = x0[:n1].copy()
        bad[0, 0] = np.nan
        got = elfi_amd.romc_solve(p, bad)
    finally:
        p.free()
    assert got['status'][0] == R.NONFINITE and got['nfev'][0] == 1 and np.isnan(got['f_min'][0]) and np.all(np.isnan(got['x_min'][0]))
    _assert_solution({k: v[1:] for k, v in got.items()}, want, slice(1, n1))


# ---- regions ----------------------------------------------------------------------------------------------------------------
def _solved16(n_obs):
    W, _, want = setup(n_obs)
    idx = np.flatnonzero(want['status'] == R.SOLVED)[:16]
    assert len(idx) == 16
    return W, idx, want['x_min'][idx], want['hess'][idx], EPS_REGION


@pytest.mark.parametrize('n_obs', N_OBS)
def test_regions_are_the_statement(hip_ctx, problems, n_obs):
    import elfi_amd
    W, idx, centre, hess, eps = _solved16(n_obs)
    got = elfi_amd.romc_regions(problems[n_obs], idx, centre, hess, eps)
    want = R.regions(W, OBS, idx, centre, hess, eps)
    for key in ('rotation', 'limits', 'nfev'):
        assert _same(got[key], want[key]), key
    assert np.all(got['limits'][:, :, 0] < 0) and np.all(got['limits'][:, :, 1] > 0)


def test_region_edge_cases(hip_ctx, problems):
    import elfi_amd
    W, idx, centre, hess, eps = _solved16(100)
    p = problems[100]
    bad = np.array([[[2., 2.], [2., 2.]], [[0., 0.], [0., 0.]], [[1., 0.], [0., 1e-17]], [[np.nan, 0.], [0., 1.]], [[np.inf, 1.], [1., 1.]],
                    [[2., 1.], [1., 3.]], [[2., 0.5], [1.5, 3.]]])
    got = elfi_amd.romc_regions(p, idx[:7], centre[:7], bad, eps)
    want = R.regions(W, OBS, idx[:7], centre[:7], bad, eps)
    assert np.all(got['rotation'][:5] == np.eye(2)) and _same(got['rotation'][5], got['rotation'][6])
    for key in ('rotation', 'limits', 'nfev'):
        assert _same(got[key], want[key]), key
    f_min = setup(100)[2]['f_min'][idx[0]]
    got = elfi_amd.romc_regions(p, idx[:1], centre[:1], hess[:1], f_min * 0.5)          # no step is accepted: the last step
    assert np.array_equal(got['limits'][0], [[-2.0 ** -10, 2.0 ** -10]] * 2) and np.all(got['nfev'] == 10)
    got = elfi_amd.romc_regions(p, idx[:1], centre[:1], hess[:1], 1e300, eta=0.125, rep_lim=7)   # the rep_lim break
    assert np.array_equal(got['limits'][0], [[-7 * 0.125, 7 * 0.125]] * 2) and np.all(got['nfev'] == 9)
    want = R.regions(W, OBS, idx[:3], centre[:3], hess[:3], eps, K=3, eta=0.3, rep_lim=2)
    got = elfi_amd.romc_regions(p, idx[:3], centre[:3], hess[:3], eps, K=3, eta=0.3, rep_lim=2)
    for key in ('rotation', 'limits', 'nfev'):
        assert _same(got[key], want[key]), key


# ---- sample -----------------------------------------------------------------------------------------------------------------
def _boxes(n_obs, R_):
    W, idx, centre, hess, eps = _solved16(n_obs)
    reg = R.regions(W, OBS, idx[:R_], centre[:R_], hess[:R_], eps)
    return W, idx[:R_], centre[:R_], reg['rotation'], reg['limits'], eps


@pytest.mark.parametrize('n2', [64, 70])
def test_sample(hip_ctx, problems, n2):
    import elfi_amd
    W, idx, centre, rot, lim, eps = _boxes(100, 8)
    p = problems[100]
    seed, base = 20240, elfi_amd.priors.ROMC_STREAM_BASE
    theta, f = elfi_amd.romc_sample(p, idx, centre, rot, lim, n2, seed=seed)
    assert theta.shape == (8, n2, 2) and f.shape == (8, n2)
    for r in range(8):
        u = np.column_stack([PH.uniform53_first(seed, base + r, 2 * np.arange(n2) + k) for k in range(2)])
        want = R.box_transform(u, centre[r], rot[r], lim[r])
        # theta_i = (rot[i, 0] t_0 + rot[i, 1] t_1) + c_i in the same order of operations: 2 ulp of the largest term allow for
        # the one rounding of the scaling t_k = u (hi - lo) + lo that a fused multiply-add on either side would change
        scale = np.abs(rot[r]) @ np.abs(lim[r]).max(axis=1) + np.abs(centre[r])
        assert np.all(np.abs(theta[r] - want) <= 2 * R.EPS * scale)
        y = (theta[r] - centre[r]) @ rot[r]                       # R^-1 = R^T for a rotation
        tol = 8 * R.EPS * (np.abs(lim[r]).max() + np.abs(centre[r]).max())
        assert np.all(y >= lim[r][:, 0] - tol) and np.all(y <= lim[r][:, 1] + tol)
    assert _same(f.reshape(-1), elfi_amd.romc_objective(p, theta.reshape(-1, 2), np.repeat(idx, n2)))
    again = elfi_amd.romc_sample(p, idx, centre, rot, lim, n2, seed=seed)
    assert _same(theta, again[0]) and _same(f, again[1])
    other = elfi_amd.romc_sample(p, idx, centre, rot, lim, n2, seed=seed + 1)[0]
    assert not np.any(other == theta)
    same_box = elfi_amd.romc_sample(p, idx[[0, 0]], centre[[0, 0]], rot[[0, 0]], lim[[0, 0]], n2, seed=seed)[0]
    assert _same(same_box[0], theta[0]) and not np.any(same_box[0] == same_box[1]), 'regions must draw from streams of their own'


# ---- count ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('BS', [50, 130])
@pytest.mark.parametrize('contain', [False, True])
def test_count(hip_ctx, problems, BS, contain):
    import elfi_amd
    W, idx, centre, rot, lim, eps = _boxes(100, 16)
    rs = np.random.RandomState(BS)
    theta = np.vstack((centre[rs.randint(0, 16, BS // 2)] + rs.normal(0, 0.2, (BS // 2, 2)), _starts(BS - BS // 2, BS + 1)))
    boxes = (centre, np.array([np.linalg.inv(v) for v in rot]), lim) if contain else None
    got = elfi_amd.romc_count(problems[100], theta, idx, eps, boxes)
    want = R.count(W, OBS, theta, idx, eps, boxes)
    print('counts: %d points, largest %d, sum %d' % (BS, want.max(), want.sum()))
    assert got.dtype == np.int32 and np.array_equal(got, want) and want.max() > 1
    if contain:
        assert want.sum() < R.count(W, OBS, theta, idx, eps).sum()
    assert np.array_equal(elfi_amd.romc_count(problems[100], theta, idx[:0], eps), np.zeros(BS, dtype=np.int32))


# ---- the _dev forms ---------------------------------------------------------------------------------------------------------
def _dev_case(n_obs, handle_of, make_handle=False):
    """Every _dev form once: inputs at a pitch wider than the row, outputs between guard words."""
    W, x0, want = setup(n_obs)
    _, idx, centre, rot, lim, eps = _boxes(n_obs, 8)
    hess = want['hess'][idx]
    theta, prob = _pairs(100, N1, 5)
    pitch = 3

    def wide(a):
        out = np.full((len(a), pitch), np.nan)
        out[:, :2] = a
        return out

    def case(d):
        th, pr = d.input(wide(theta)), d.input(prob.astype(np.int64))
        sx0 = d.input(wide(x0))
        ri, rc, rh = d.input(idx.astype(np.int64)), d.input(centre), d.input(hess)
        rr, rl, rinv = d.input(rot), d.input(lim), d.input(np.array([np.linalg.inv(v) for v in rot]))
        f = d.out(100)
        xm, fm, hs = d.out(N1, 2), d.out(N1), d.out_raw(N1 * 4, __import__('torch').float64)
        nf, ni, st = (d.out_raw(N1, __import__('torch').int32) for _ in range(3))
        orot, olim, onf = d.out(8, 4), d.out(8, 4), d.out_raw(32, __import__('torch').int32)
        sth, sf = d.out(8 * 40, 2), d.out(8 * 40)
        cnt = d.out_raw(100, __import__('torch').int32)
        dW = d.input(W) if make_handle else None
        d.go()
        if make_handle:
            h = C.c_void_p()
            d.call('elfihip_romc_create_dev', d.cx, 0, N1, n_obs, DBL(OBS[0]), DBL(OBS[1]), dW.ptr, n_obs + 2, None, None, C.byref(h))
            d.cleanup.append(lambda: d.lib.elfihip_romc_free(h))
        else:
            h = handle_of(n_obs)
        d.call('elfihip_romc_objective_dev', h, 100, th.ptr, pitch, pr.ptr, f.ptr)
        d.call('elfihip_romc_solve_dev', h, sx0.ptr, pitch, 400, 400, xm.ptr, 2, fm.ptr, hs.ptr, nf.ptr, ni.ptr, st.ptr)
        d.call('elfihip_romc_regions_dev', h, 8, ri.ptr, rc.ptr, rh.ptr, DBL(eps), 10, DBL(1.0), 300, orot.ptr, olim.ptr, onf.ptr)
        d.call('elfihip_romc_sample_dev', h, 8, ri.ptr, rc.ptr, rr.ptr, rl.ptr, 40, U64(7), U64(11), sth.ptr, 2, sf.ptr)
        d.call('elfihip_romc_count_dev', h, 100, th.ptr, pitch, 8, ri.ptr, DBL(eps), 1, rc.ptr, rinv.ptr, rl.ptr, cnt.ptr)
        d.done()
    return case, dict(theta=theta, prob=prob, idx=idx, centre=centre, hess=hess, rot=rot, lim=lim, eps=eps, x0=x0)


def _doubles(res, name):
    return res[name].view(np.float64)[DL._LEAD:-DL._TAIL]


@pytest.mark.parametrize('n_obs', [8, 126])
def test_dev_forms_between_guard_words_equal_the_host_forms(hip_ctx, problems, n_obs):
    import elfi_amd
    case, a = _dev_case(n_obs, lambda n: problems[n]._h())
    d = SO.Driver(hip_ctx, False, 'romc dev forms')
    try:
        case(d)
    except BaseException:
        d.abort()
        raise
    res = d.finish()
    SO.guards_intact(res, d.guarded)
    p = problems[n_obs]
    assert _same(_doubles(res, 'out0'), elfi_amd.romc_objective(p, a['theta'], a['prob']))
    sol = elfi_amd.romc_solve(p, a['x0'])
    assert _same(_doubles(res, 'out1'), sol['x_min'].reshape(-1)) and _same(_doubles(res, 'out2'), sol['f_min'])
    assert _same(res['out3'][:N1 * 32].view(np.float64), sol['hess'].reshape(-1))
    for name, key in (('out4', 'nfev'), ('out5', 'nit'), ('out6', 'status')):
        assert _same(res[name][:N1 * 4].view(np.int32), sol[key]) and np.all(res[name][N1 * 4:] == 0xA5)
    reg = elfi_amd.romc_regions(p, a['idx'], a['centre'], a['hess'], a['eps'])
    assert _same(_doubles(res, 'out7'), reg['rotation'].reshape(-1)) and _same(_doubles(res, 'out8'), reg['limits'].reshape(-1))
    assert _same(res['out9'][:128].view(np.int32), reg['nfev'].reshape(-1)) and np.all(res['out9'][128:] == 0xA5)
    th, f = elfi_amd.romc_sample(p, a['idx'], a['centre'], a['rot'], a['lim'], 40, seed=7, stream=11)
    assert _same(_doubles(res, 'out10'), th.reshape(-1)) and _same(_doubles(res, 'out11'), f.reshape(-1))
    cnt = elfi_amd.romc_count(p, a['theta'], a['idx'], a['eps'], (a['centre'], np.array([np.linalg.inv(v) for v in a['rot']]), a['lim']))
    assert _same(res['out12'][:400].view(np.int32), cnt) and np.all(res['out12'][400:] == 0xA5)


def test_dev_outputs_at_a_pitch_leave_the_gaps_alone(hip_ctx, problems):
    import torch
    import elfi_amd
    W, x0, want = setup(100)
    _, idx, centre, rot, lim, eps = _boxes(100, 8)
    p = problems[100]
    dx0 = DL.to_device(x0)
    xm = torch.full((N1, 5), DL.SENTINEL, dtype=torch.float64, device='cuda')
    th = torch.full((8 * 10, 3), DL.SENTINEL, dtype=torch.float64, device='cuda')
    fm, hs, sf = (torch.empty(n, dtype=torch.float64, device='cuda') for n in (N1, 4 * N1, 80))
    ints = [torch.empty(N1, dtype=torch.int32, device='cuda') for _ in range(3)]
    di, dc, dr, dl = DL.to_device(idx.astype(np.float64)).to(torch.int64), DL.to_device(centre), DL.to_device(rot), DL.to_device(lim)
    lib = hip_ctx.lib
    assert lib.elfihip_romc_solve_dev(p._h(), dx0.data_ptr(), 2, 400, 400, xm.data_ptr(), 5, fm.data_ptr(), hs.data_ptr(),
                                      *[t.data_ptr() for t in ints]) == 0
    assert lib.elfihip_romc_sample_dev(p._h(), 8, di.data_ptr(), dc.data_ptr(), dr.data_ptr(), dl.data_ptr(), 10, U64(7), U64(11),
                                       th.data_ptr(), 3, sf.data_ptr()) == 0
    hip_ctx.synchronize()
    xm, th = xm.cpu().numpy(), th.cpu().numpy()
    assert _same(xm[:, :2], want['x_min']) and np.all(xm[:, 2:] == DL.SENTINEL)
    assert _same(th[:, :2].reshape(8, 10, 2), elfi_amd.romc_sample(p, idx, centre, rot, lim, 10, seed=7, stream=11)[0])
    assert np.all(th[:, 2] == DL.SENTINEL)


def test_dev_forms_on_a_busy_adopted_stream(hip_ctx, problems):
    case, _ = _dev_case(100, lambda n: problems[n]._h())
    ref, got, d = SO.run_both(hip_ctx, case, 'romc dev forms')
    SO.guards_intact(ref, d.guarded)
    SO.guards_intact(got, d.guarded)
    SO.assert_same(ref, got, 'romc dev forms')
    assert d.still_busy, 'the stream was idle when the last call had returned: a call waited for the stream on the host'


def test_create_dev_on_a_busy_adopted_stream(hip_ctx, problems):
    """The handle's noise arrives in stream order too.  (Its allocation is a hipMalloc, which may wait for the device: only
    the results are compared here, not whether the stream was still busy.)"""
    case, _ = _dev_case(100, None, make_handle=True)
    ref, got, d = SO.run_both(hip_ctx, case, 'romc create_dev', syncs=True)
    SO.guards_intact(got, d.guarded)
    SO.assert_same(ref, got, 'romc create_dev')
    own, _, _ = SO.run_both(hip_ctx, _dev_case(100, lambda n: problems[n]._h())[0], 'romc dev forms')
    SO.assert_same(own, got, 'romc create_dev against the host-made handle')


# ---- end to end -------------------------------------------------------------------------------------------------------------
@needs_reference
def test_hip_romc_end_to_end(hip_ctx):
    import scipy.optimize as optim
    elfi = ref_shim.install()
    import elfi.clients.native as native
    native.set_as_default()
    import elfi_amd
    bounds = [(-2, 2), (-1.25, 1.25)]
    m = elfi_amd.ma2_model(seed_obs=4)
    romc = elfi_amd.HipROMC(m, bounds=bounds, discrepancy_name='d')
    assert isinstance(romc, elfi.ROMC)
    romc.solve_problems(n1=16, seed=21)
    solved = [p for p in romc.optim_problems if p.state['solved']]
    assert len(solved) >= 8
    # every solved minimum against the reference's own optimiser on the reference's own frozen-seed objective, from the same
    # start: within the simplex tolerance (not exact: the reference squares with pow)
    for p in solved:
        want = optim.minimize(p.objective, p.initial_point, method='Nelder-Mead')
        assert want.success
        assert np.max(np.abs(want.x - p.result.x_min)) <= 1e-4 and abs(want.fun - p.result.f_min) <= 1e-4
        assert abs(p.objective(p.result.x_min) - p.result.f_min) <= 4 * R.EPS * max(p.result.f_min, 1e-3)
    # the filter is the 0.75 quantile of the minimal values.  With two summaries and two parameters those are zero up to the
    # simplex tolerance, so the quantile is no scale for a region: the boxes and the indicator take the thresholds of the
    # reference's own ROMC test on this model (eps_region = its eps_filter 0.02, eps_cutoff 0.1)
    eps = romc.compute_eps(0.75)
    romc.estimate_regions(eps_filter=eps, fit_models=False, eps_region=0.02, eps_cutoff=0.1)
    assert sum(romc.inference_state['accepted']) >= 4 and romc.inference_state['computed_BB'] == romc.inference_state['accepted']
    np.random.seed(5)          # (ROMC.sample hands its posterior seed=None, as the reference does)
    romc.sample(n2=32)
    R_ = sum(romc.inference_state['accepted'])
    assert romc.samples.shape == (R_, 32, 2) and romc.weights.shape == (R_, 32) and romc.distances.shape == (R_ * 32,)
    assert np.all(np.isfinite(romc.weights)) and np.sum(romc.weights > 0) > 0
    mean = romc.result.sample_means_array
    assert np.all(np.isfinite(mean)) and bounds[0][0] < mean[0] < bounds[0][1] and bounds[1][0] < mean[1] < bounds[1][1]
    assert np.isfinite(romc.compute_ess())
    # nine points: minima of accepted problems (each inside at least its own indicator) and points of a coarse grid
    accepted = [p for p, a in zip(romc.optim_problems, romc.inference_state['accepted']) if a]
    pts = np.array([p.result.x_min for p in accepted[:5]] + [[a, b] for a in (0.3, 0.6, 0.9) for b in (0.0, 0.2, 0.4)])[:9]
    got = romc.eval_unnorm_posterior(pts)
    want = np.array([romc.posterior._pdf_unnorm_single_point(t) for t in pts])
    print('unnormalised posterior at 9 points:', got)
    assert np.array_equal(got, want) and np.any(got > 0)
