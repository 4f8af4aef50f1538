"""CPU: the NumPy statements of the device ROMC (tests/romc_ref.py) pinned to SciPy and to the reference, and the argument
handling of the Python layer (elfi_amd/romc.py), which happens before any device call.

  * Nelder-Mead: the statement equals scipy.optimize.minimize(method='Nelder-Mead') on 200 MA2 objectives in x, fun, nfev,
    nit and success, exactly; the same with maxiter = 5, where every problem is unsolved.
  * Regions: the statement against the reference's RegionConstructor on 32 fixed problems -- limits equal, rotations within
    1e-12 -- after both are brought to one order and sign of the eigenvectors (the reference takes numpy.linalg.eig, the
    statement a Jacobi rotation); the three edge cases of the line search and the rank rule.
  * Hessian: the difference Hessian against the exact Hessian of the quartic f_i, within a bound computed from the
    polynomial's coefficients.
"""
import os
import sys

import numpy as np
import pytest

import romc_ref as R

ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle')
sys.path.insert(0, ORACLE)
import ref_shim  # noqa: E402

needs_reference = pytest.mark.skipif(not ref_shim.available(), reason='no reference package (run oracle/make_ref.sh)')

OBS = (0.35, 0.05)          # observed summaries of the order ma2_model(seed_obs=...) has
N_OBS = 100
NM_SEED, REGION_SEED = 1234, 77


def _starts(n, seed):
    rs = np.random.RandomState(seed)
    return np.column_stack((rs.uniform(-1.5, 1.5, n), rs.uniform(-1, 1, n)))


# ---- Nelder-Mead ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def nm_problems():
    return R.make_noise(200, N_OBS, NM_SEED), _starts(200, NM_SEED + 1)


@pytest.mark.parametrize('maxiter', [None, 5])
def test_nelder_mead_is_scipys(nm_problems, maxiter):
    import scipy.optimize as optim
    W, x0 = nm_problems
    x0 = x0.copy()
    x0[3, 0] = 0.0          # the zero-coordinate rule of the initial simplex
    bad = []
    for i in range(len(W)):
        f = R.make_objective(W[i], OBS)
        want = optim.minimize(f, x0[i], method='Nelder-Mead', options=None if maxiter is None else dict(maxiter=maxiter))
        x, fun, nfev, nit, status = R.nelder_mead(f, x0[i], maxiter=maxiter)
        same = (np.array_equal(x, want.x) and fun == want.fun and nfev == want.nfev and nit == want.nit
                and (status == R.SOLVED) == bool(want.success) and status == want.status)
        if not same:
            bad.append(i)
        if maxiter is not None:
            assert not want.success and status == R.MAXITER and nit == maxiter
    assert not bad, 'problems where the statement is not SciPy\'s: %r' % bad


def test_nelder_mead_evaluation_limit_and_non_finite_values():
    import scipy.optimize as optim
    W = R.make_noise(4, N_OBS, NM_SEED + 2)
    x0 = _starts(4, NM_SEED + 3)
    for i in range(4):
        f = R.make_objective(W[i], OBS)
        for maxfev in (2, 3, 10, 37):        # a limit inside the initial simplex, at its end, inside an iteration
            want = optim.minimize(f, x0[i], method='Nelder-Mead', options=dict(maxfev=maxfev))
            x, fun, nfev, nit, status = R.nelder_mead(f, x0[i], maxfev=maxfev)
            assert np.array_equal(x, want.x) and fun == want.fun and (nfev, nit, status) == (want.nfev, want.nit, want.status)
    x, fun, nfev, nit, status = R.nelder_mead(R.make_objective(W[0], OBS), [np.nan, 0.1])
    assert status == R.NONFINITE and nfev == 1 and np.isnan(fun) and np.all(np.isnan(x))


# ---- Hessian ----------------------------------------------------------------------------------------------------------------
def _quadratic(w, lag, absolute=False):
    """Coefficients (1, t1, t2, t1^2, t1 t2, t2^2) of S_lag(theta) = mean(x[k + lag] x[k]), x = a + t1 b + t2 c; with
    `absolute` of the majorant mean(|x[k + lag]| |x[k]|) <= the same polynomial in |theta| over |a|, |b|, |c|."""
    parts = [w[2:], w[1:-1], w[:-2]]
    if absolute:
        parts = [np.abs(p) for p in parts]
    m = lambda u, v: float(np.mean(u[lag:] * v[:-lag]))
    a, b, c = parts
    return np.array([m(a, a), m(a, b) + m(b, a), m(a, c) + m(c, a), m(b, b), m(b, c) + m(c, b), m(c, c)])


def _exact_hessian(w, x):
    H = np.zeros((2, 2))
    for lag, o in ((1, OBS[0]), (2, OBS[1])):
        q = _quadratic(w, lag)
        S = q @ [1, x[0], x[1], x[0] ** 2, x[0] * x[1], x[1] ** 2]
        g = np.array([q[1] + 2 * q[3] * x[0] + q[4] * x[1], q[2] + q[4] * x[0] + 2 * q[5] * x[1]])
        S2 = np.array([[2 * q[3], q[4]], [q[4], 2 * q[5]]])
        H += 2 * (np.outer(g, g) + (S - o) * S2)
    return H


def test_difference_hessian_is_within_its_bound_of_the_exact_hessian():
    """f = sum_j (S_j - o_j)^2 with S_j quadratic in theta is a quartic: its fourth derivatives are the constants
    2 (S_ab S_cd + S_ac S_bd + S_ad S_bc), at most 6 max |S_ab|^2 per summary.  Bound = truncation h^2 / 12 max |f''''| plus
    round-off 4 eps max |f| / h^2 with h the smaller step, max |f| the value of f's majorant (every product and difference
    taken in absolute value: the scale the rounding errors of the sums have) at the stencil's farthest point."""
    W = R.make_noise(24, N_OBS, 4321)
    pts = _starts(24, 4322) * 0.6
    worst = 0.0
    for w, x in zip(W, pts):
        f = R.make_objective(w, OBS)
        H = R.hessian(f, x, f(x))
        h = 2.0 ** -13 * np.maximum(1.0, np.abs(x))
        f4 = sum(6 * max(abs(2 * q[3]), abs(q[4]), abs(2 * q[5])) ** 2 for q in (_quadratic(w, 1), _quadratic(w, 2)))
        ax = np.abs(x) + h
        mono = np.array([1, ax[0], ax[1], ax[0] ** 2, ax[0] * ax[1], ax[1] ** 2])
        fmax = sum((_quadratic(w, lag, True) @ mono + abs(o)) ** 2 for lag, o in ((1, OBS[0]), (2, OBS[1])))
        bound = h.max() ** 2 / 12 * f4 + 4 * R.EPS * fmax / h.min() ** 2
        err = np.max(np.abs(H - _exact_hessian(w, x)))
        worst = max(worst, err / bound)
        assert H[0, 1] == H[1, 0]
        assert err <= bound, (err, bound)
    print('largest error / bound: %.3f' % worst)


# ---- regions ----------------------------------------------------------------------------------------------------------------
def _canonical(rot, limits, H):
    """Columns by eigenvalue (v^T H v), each with its largest component positive; a sign flip swaps and negates the pair."""
    rot, limits = np.array(rot, dtype=float), np.array(limits, dtype=float)
    lam = [rot[:, d] @ H @ rot[:, d] for d in range(2)]
    order = np.argsort(lam, kind='stable')
    rot, limits = rot[:, order], limits[order]
    for d in range(2):
        if rot[np.argmax(np.abs(rot[:, d])), d] < 0:
            rot[:, d] = -rot[:, d]
            limits[d] = -limits[d, 1], -limits[d, 0]
    return rot, limits


@pytest.fixture(scope='module')
def region_problems():
    """32 solved problems: noise, minima, Hessians and a threshold.  (Two summaries and two parameters: the minimal values
    are zero up to the simplex tolerance, a quantile of them would make every box the last step of the search wide; 0.01 is
    a distance of 0.1, a tenth of the scale of the summaries.)"""
    W = R.make_noise(32, N_OBS, REGION_SEED)
    res = R.solve(W, OBS, _starts(32, REGION_SEED + 1))
    assert np.all(res['status'] == R.SOLVED)
    return W, res, 0.01


@needs_reference
def test_regions_are_the_reference_constructors(region_problems):
    ref_shim.install()
    from elfi.methods.inference import romc as ref
    W, res, eps = region_problems
    got = R.regions(W, OBS, np.arange(32), res['x_min'], res['hess'], eps)
    diff_limits, worst_rot = 0, 0.0
    for i in range(32):
        f = R.make_objective(W[i], OBS)
        result = ref.RomcOptimisationResult(res['x_min'][i], res['f_min'][i], res['hess'][i])
        box = ref.RegionConstructor(result, f, 2, eps_region=eps, K=10, eta=1., rep_lim=300).build()[0]
        lam = np.linalg.eigvalsh(res['hess'][i])
        assert abs(lam[1] - lam[0]) > 1e-3 * np.abs(lam).max(), 'problem %d: eigenvalues too close for a comparison of vectors' % i
        want_rot, want_lim = _canonical(box.rotation, box.limits, res['hess'][i])
        got_rot, got_lim = _canonical(got['rotation'][i], got['limits'][i], res['hess'][i])
        diff_limits += int(np.sum(want_lim != got_lim))
        worst_rot = max(worst_rot, float(np.max(np.abs(want_rot - got_rot))))
    print('limits that differ: %d of 128; largest rotation difference %.2e' % (diff_limits, worst_rot))
    assert diff_limits == 0
    assert worst_rot <= 1e-12


def test_region_edge_cases(region_problems):
    W, res, eps = region_problems
    c, H = res['x_min'][:1], res['hess'][:1]
    # a singular or non-finite Hessian: the identity
    for bad in ([[2., 2.], [2., 2.]], [[0., 0.], [0., 0.]], [[1., 0.], [0., 1e-17]], [[np.nan, 0.], [0., 1.]], [[np.inf, 1.], [1., 1.]]):
        assert np.array_equal(R.rotation(np.array(bad)), np.eye(2))
    assert not np.array_equal(R.rotation(H[0]), np.eye(2))
    V = R.rotation(np.array([[2., 1.], [1., 3.]]))
    assert np.allclose(V.T @ V, np.eye(2), atol=1e-15) and np.allclose(V.T @ np.array([[2., 1.], [1., 3.]]) @ V, np.diag([V[:, 0] @ [[2., 1.], [1., 3.]] @ V[:, 0], V[:, 1] @ [[2., 1.], [1., 3.]] @ V[:, 1]]), atol=1e-14)
    # eps_region below f_min: no step is accepted, the offset is the last (halved) step
    got = R.regions(W, OBS, [0], c, H, res['f_min'][0] * 0.5, K=10, eta=1.)
    assert np.array_equal(got['limits'][0], [[-2.0 ** -10, 2.0 ** -10]] * 2) and np.all(got['nfev'] == 10)
    # a huge eps_region: the first refinement runs into rep_lim and ends the search
    got = R.regions(W, OBS, [0], c, H, 1e300, K=10, eta=0.125, rep_lim=7)
    assert np.array_equal(got['limits'][0], [[-7 * 0.125, 7 * 0.125]] * 2) and np.all(got['nfev'] == 9)


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
def test_argument_checks_come_before_any_device_call():
    from elfi_amd import romc
    with pytest.raises(ValueError, match='3 to 126'):
        romc.RomcProblems(127, OBS, W=np.zeros((2, 129)))
    with pytest.raises(ValueError, match='either'):
        romc.RomcProblems(10, OBS)
    with pytest.raises(ValueError, match='either'):
        romc.RomcProblems(10, OBS, W=np.zeros((2, 12)), seeds=[1, 2])
    with pytest.raises(ValueError, match='shape'):
        romc.RomcProblems(10, OBS, W=np.zeros((2, 11)))
    with pytest.raises(ValueError, match='observed'):
        romc.RomcProblems(10, (0.1, np.nan), W=np.zeros((2, 12)))
    assert romc._limits(None, None) == (400, 400)
    assert romc._limits(5, None) == (5, 2 ** 31 - 1) and romc._limits(None, 7) == (2 ** 31 - 1, 7)
    for bad in ((0, None), (None, 2.5), (2 ** 21, 2 ** 21)):
        with pytest.raises(ValueError):
            romc._limits(*bad)
    with pytest.raises(ValueError, match='shape'):
        romc._points(np.zeros((3, 3)), 'theta')
    with pytest.raises(ValueError, match='outside'):
        romc._index([0, 4], 4)
    with pytest.raises(ValueError, match='integer'):
        romc._index([0.5], 4)
    with pytest.raises(ValueError, match='entries'):
        romc._index([0, 1], 4, count=3)
    for bad in (dict(K=0), dict(K=65), dict(eta=0.), dict(eta=np.inf), dict(rep_lim=-1), dict(eps_region=np.nan)):
        with pytest.raises(ValueError):
            romc._search_args(**dict(dict(eps_region=1., K=10, eta=1., rep_lim=300), **bad))


@needs_reference
def test_problem_streams_are_what_the_models_simulator_is_handed(monkeypatch):
    """model.generate(batch_size=1, with_values=..., seed=nuisance) on ma2_model: the (seed, stream) pair the device
    simulator receives is the pair HipROMC freezes for that nuisance."""
    ref_shim.install()
    import elfi_amd
    from elfi_amd import fused_models, romc
    seen = []

    def recorder(t1, t2, observed, n_obs=100, seed=0, stream=0, ctx=None):
        seen.append((int(seed), int(stream), int(n_obs)))
        z = np.zeros(1)
        return z, z, z

    monkeypatch.setattr(fused_models, 'ma2_draw_distance', recorder)
    m = elfi_amd.ma2_model(n_obs=50, seed_obs=4, device_priors=False)
    assert romc.ma2_model_parts(m, 'd')[0] == 50
    nuisance = [1, 17, 2 ** 32 - 2, 123456789]
    for v in nuisance:
        m.generate(batch_size=1, outputs=['MA2'], with_values=dict(t1=np.array([0.5]), t2=np.array([0.1])), seed=int(v))
    seeds, streams = romc.problem_streams(nuisance)
    assert [(s, t) for s, t, _ in seen] == list(zip(seeds.tolist(), streams.tolist()))
    assert all(t == elfi_amd.priors.SIMULATOR_STREAM_BASE for _, t, _ in seen) and all(n == 50 for _, _, n in seen)


@needs_reference
def test_unsupported_settings_name_what_is_supported():
    elfi = ref_shim.install()
    import elfi_amd
    m = elfi_amd.ma2_model(n_obs=50, seed_obs=4, device_priors=False)
    with pytest.raises(NotImplementedError, match='custom_optim_class'):
        elfi_amd.HipROMC(m, bounds=[(-2, 2), (-1.25, 1.25)], discrepancy_name='d', custom_optim_class=object)
    from elfi.examples import ma2
    with pytest.raises(NotImplementedError, match='ma2_model'):
        elfi_amd.HipROMC(ma2.get_model(n_obs=50, seed_obs=4), bounds=[(-2, 2), (-1.25, 1.25)], discrepancy_name='d')
    with pytest.raises(NotImplementedError, match='ma2_model'):
        elfi_amd.HipROMC(elfi_amd.ma2_model(n_obs=200, seed_obs=4, device_priors=False), discrepancy_name='d')
    romc = elfi_amd.HipROMC(m, bounds=[(-2, 2), (-1.25, 1.25)], discrepancy_name='d')
    assert isinstance(romc, elfi.ROMC)
    romc._define_objectives(n1=3, seed=1)
    with pytest.raises(NotImplementedError, match='seed and x0'):
        romc._solve_gradients(method='BFGS')
