"""Parity of the HIP GP core (through the C ABI) with the CPU oracle at FIXED hyper-parameters.

Tolerances: L and L^-T relative 1e-10 (of the largest entry), alpha, mu,
var, gradients, log-marginal relative 1e-8 -- the conditioning of K with the default noise
max(y)^2/100 is benign.  The hyper-parameter search has its own file (tests/test_gp_hyper_gpu.py: pinned to the
reference's documented BOLFI run).
"""
import numpy as np
import pytest

import gp_oracle as G

pytestmark = pytest.mark.gpu


def _problem(n, d, seed=0):
    rs = np.random.RandomState(seed)
    X = rs.uniform(-2, 2, (n, d))
    y = np.linalg.norm(X - 0.5, axis=1) + 0.1 * rs.randn(n)
    return X, y.reshape(-1, 1), [(-2., 2.)] * d


def _fit(X, y, bounds, hyper=None):
    from elfi_amd.gp import GPHandle
    h = hyper or G.default_hyper(bounds, y)
    gp = GPHandle(X.shape[1], X.shape[0])
    gp.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    gp.set_data(X, y)
    logz = gp.factorize()
    return gp, logz, G.Posterior(X, y, h['var'], h['ls'], h['bias'], h['noise'])


def _close(a, b, rtol, what):
    scale = np.max(np.abs(b)) + 1e-300
    err = np.max(np.abs(a - b)) / scale
    assert err <= rtol, '%s: scaled max error %g > %g' % (what, err, rtol)


@pytest.mark.parametrize('n,d', [(5, 1), (100, 2), (128, 2), (129, 3), (300, 10), (1000, 10), (1500, 20)])
def test_factorization_vs_oracle(hip_ctx, n, d):
    X, y, bounds = _problem(n, d, seed=n)
    gp, logz, ref = _fit(X, y, bounds)
    _close(gp.get(0), ref.L, 1e-10, 'L')
    _close(gp.get(1), ref.Linv.T, 1e-9, 'L^-T')
    _close(gp.get(2), ref.alpha, 1e-8, 'alpha')
    assert abs(logz - ref.log_marginal) <= 1e-9 * abs(ref.log_marginal)
    # transpose-detecting structural check: L lower, L^-T upper, L L^-1 = I
    L, WT = gp.get(0), gp.get(1)
    assert np.allclose(L @ WT.T, np.eye(n), atol=1e-8)


@pytest.mark.parametrize('n,d,S', [(50, 2, 1), (300, 2, 7), (1000, 10, 10), (1000, 10, 37), (700, 5, 16),
                                   (600, 3, 129), (900, 4, 300), (500, 20, 10), (400, 23, 5), (400, 30, 7)])
def test_predict_and_gradients_vs_oracle(hip_ctx, n, d, S):
    X, y, bounds = _problem(n, d, seed=7 * n + S)
    gp, _, ref = _fit(X, y, bounds)
    xs = np.random.RandomState(3).uniform(-2, 2, (S, d))
    xs[0] = X[0]   # exactly on an evidence point
    mu, var = gp.predict(xs, noiseless=True)
    rmu, rvar = ref.predict(xs, noiseless=True)
    _close(mu, rmu, 1e-8, 'mu')
    assert np.max(np.abs(var - rvar)) <= 1e-8 * (ref.var + ref.bias), 'var'
    mu2, var2 = gp.predict(xs, noiseless=False)
    assert np.allclose(var2, var + ref.noise, rtol=1e-14, atol=0)
    assert np.array_equal(mu2, mu)
    m3, v3, dmu, dvar = gp.predict_grad(xs)
    gmu, gvar = ref.predictive_gradients(xs)
    assert np.array_equal(m3, mu) and np.array_equal(v3, var)
    _close(dmu, gmu, 1e-8, 'grad mu')
    _close(dvar, gvar, 1e-7, 'grad var')
    # the reference's own sampling-phase closed form (gpy_regression.py:127-140), point by point
    for s in range(min(S, 4)):
        cm, cv = ref.predict_closed_form(xs[s])
        assert abs(cm[0, 0] - mu[s, 0]) <= 1e-8 * np.max(np.abs(rmu))
        assert abs(cv[0, 0] - ref.noise - var[s, 0]) <= 1e-8 * (ref.var + ref.bias)


def test_lcb_vs_oracle(hip_ctx):
    X, y, bounds = _problem(800, 4, seed=11)
    gp, _, ref = _fit(X, y, bounds)
    xs = np.random.RandomState(5).uniform(-2, 2, (10, 4))
    for t in (0, 5, 200):
        beta = G.lcb_beta(t, 4)
        val, grad = gp.lcb(xs, beta)
        _close(val, G.lcb_evaluate(ref, xs, t), 1e-8, 'lcb')
        _close(grad, G.lcb_evaluate_gradient(ref, xs, t), 1e-7, 'lcb grad')
        # gradient is the derivative of the value (finite differences on the device function)
    eps = 1e-6
    val0, g0 = gp.lcb(xs[:1], beta)
    for a in range(4):
        xp = xs[:1].copy()
        xp[0, a] += eps
        fd = (gp.lcb(xp, beta, with_grad=False)[0][0, 0] - val0[0, 0]) / eps
        assert abs(fd - g0[0, a]) <= 1e-4 * (1 + abs(g0[0, a]))


def _jitter_problem(n, seed=3):
    """Evidence on which the PLAIN Cholesky fails on every implementation, by exact arithmetic rather than by rounding
    luck: coordinates are small integers (squared distances exact), rows 0 and 1 are the same point, and the signal
    variance 2^30 = (2^15)^2 swallows GPy's 1e-8 on the diagonal, so Ky[0:2, 0:2] = 2^30 [[1, 1], [1, 1]] exactly and the
    second pivot is 2^30 - (2^15)^2 = 0.  One rung of the ladder (jitter = 2^30 * 1e-6) makes the matrix comfortably
    positive definite."""
    rs = np.random.RandomState(seed)
    X = rs.randint(-2, 3, (n, 2)).astype(float)
    X[0] = X[1] = 0.0
    y = np.linalg.norm(X - 0.5, axis=1) + 0.1 * rs.randn(n)
    return X, y.reshape(-1, 1), dict(var=float(2 ** 30), ls=1.0, bias=0.0, noise=0.0)


@pytest.mark.parametrize('n', [10, 128, 200, 300])
def test_jitchol_ladder_equals_the_oracle(hip_ctx, n):
    """GPy's jitchol inside elfihip_gp_factorize ([GPy-upstream] util/linalg.py: jitchol, behind GPyRegression.update /
    .optimize, gpy_regression.py:286-323): where the plain Cholesky fails the factor comes from Ky + jitter I with
    jitter = mean(diag Ky) * 1e-6 * 10^k, and L, alpha and log Z belong to that matrix -- HIP against oracle/gp_oracle.py's
    jitchol on the same evidence (tolerances: cond(Ky + jitter I) ~ n * 1e6 here, so L to 1e-8, alpha to 1e-5, log Z to
    1e-8 of their scales)."""
    from elfi_amd.gp import GPHandle
    import scipy.linalg as sl
    X, y, h = _jitter_problem(n)
    Ky = G.kern_K(X, None, h['var'], h['ls'], h['bias'])
    Ky[np.diag_indices(n)] += h['noise'] + 1e-8
    with pytest.raises(sl.LinAlgError):
        sl.cholesky(Ky, lower=True)                       # the premise: LAPACK's plain Cholesky fails
    ref = G.Posterior(X, y, **h)                          # ... and the oracle's jitchol goes one rung up
    gp = GPHandle(2, n)
    gp.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    gp.set_data(X, y)
    logz = gp.factorize()
    jitter, tries = gp.jitchol()
    assert tries == 1
    assert jitter == np.diag(Ky).mean() * 1e-6
    _close(gp.get(0), ref.L, 1e-8, 'L')
    _close(gp.get(2), ref.alpha, 1e-5, 'alpha')
    assert abs(logz - ref.log_marginal) <= 1e-8 * abs(ref.log_marginal)
    xs = np.random.RandomState(1).uniform(-2, 2, (7, 2))
    mu, var = gp.predict(xs, noiseless=True)
    rmu, rvar = ref.predict(xs, noiseless=True)
    _close(mu, rmu, 1e-5, 'mu')
    assert np.max(np.abs(var - rvar)) <= 1e-5 * h['var']
    # with the ladder switched off the same evidence fails at once, as round 4's library did
    gp.jitchol(maxtries=0)
    with pytest.raises(np.linalg.LinAlgError):
        gp.factorize()
    assert gp.jitchol() == (0.0, 0)
    # a matrix that needs no jitter reports none
    gp.jitchol(maxtries=5)
    gp.set_hyper(1.0, 1.0, 0.0, 0.5)
    gp.factorize()
    assert gp.jitchol() == (0.0, 0)


def test_not_positive_definite_even_with_jitter(hip_ctx):
    """What no jitter repairs (a NaN in the evidence) ends the ladder after GPy's five tries with LinAlgError -- never a
    crash, never a factor with NaN in it; prediction before any factorisation is refused."""
    from elfi_amd.gp import GPHandle
    X = np.zeros((10, 2))
    X[3, 1] = np.nan
    gp = GPHandle(2, 10)
    gp.set_hyper(1.0, 1.0, 0.0, 0.0)
    gp.set_data(X, np.ones(10))
    with pytest.raises(np.linalg.LinAlgError, match='even with jitter'):
        gp.factorize()
    assert gp.jitchol()[1] == 5
    with pytest.raises(Exception):
        gp.predict(np.zeros((1, 2)))                    # the failed object is not factorised
    with pytest.raises(Exception):
        GPHandle(2, 10).predict(np.zeros((1, 2)))       # predict before factorize
    # ten identical points without noise: singular in exact arithmetic, positive definite with GPy's 1e-8 -- factors plainly
    gp2 = GPHandle(2, 10)
    gp2.set_hyper(1.0, 1.0, 0.0, 0.0)
    gp2.set_data(np.zeros((10, 2)), np.ones(10))
    gp2.factorize()
    assert gp2.jitchol() == (0.0, 0)
    ref = G.Posterior(np.zeros((10, 2)), np.ones((10, 1)), 1.0, 1.0, 0.0, 0.0)
    _close(gp2.get(0), ref.L, 1e-7, 'L of the nearly singular block')


def test_update_on_a_jittered_factor_rebuilds_like_the_reference(hip_ctx):
    """GPyRegression.update rebuilds the GP on every call (gpy_regression.py:304-312), so the plain Cholesky gets its
    chance again each time.  The bordering shortcut must therefore not extend a factor that carries jitter, and a
    bordered pivot that is not positive must go to the ladder instead of failing the update."""
    from elfi_amd.gp import GPHandle
    X, y, h = _jitter_problem(140)
    gp = GPHandle(2, 256)
    gp.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    gp.set_data(X[:130], y[:130])
    gp.factorize()
    assert gp.jitchol()[1] == 1
    for i in range(130, 140):
        gp.extend(X[i:i + 1], y[i:i + 1])                # each one a rebuild through the ladder
        assert gp.jitchol()[1] == 1
    ref = G.Posterior(X, y, **h)
    _close(gp.get(0), ref.L, 1e-8, 'L')
    _close(gp.get(2), ref.alpha, 1e-5, 'alpha')
    # a clean factor bordered by a duplicate of an evidence point: the new pivot is exactly zero -> ladder, not an error
    X2 = X[2:60].copy()
    gp3 = GPHandle(2, 128)
    gp3.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    keep = [0]
    for i in range(1, len(X2)):                          # distinct points only: the plain Cholesky goes through
        if not any(np.array_equal(X2[i], X2[j]) for j in keep):
            keep.append(i)
    Xc, yc = X2[keep], y[2:60][keep]
    gp3.set_data(Xc, yc)
    gp3.factorize()
    assert gp3.jitchol() == (0.0, 0)
    gp3.extend(Xc[:1], yc[:1])                           # an exact duplicate of row 0
    jitter, tries = gp3.jitchol()
    assert tries == 1 and jitter > 0
    Xd, yd = np.r_[Xc, Xc[:1]], np.r_[yc, yc[:1]]
    ref3 = G.Posterior(Xd, yd, **h)
    _close(gp3.get(0), ref3.L, 1e-8, 'L after the bordered duplicate')


def test_update_matches_rebuild(hip_ctx):
    """GPyRegression.update semantics: appending == rebuilding with np.r_[X_old, x]."""
    from elfi_amd.gp import HipGPRegression
    X, y, bounds = _problem(260, 2, seed=2)
    names = ['a', 'b']
    b = dict(zip(names, bounds))
    m1 = HipGPRegression(names, bounds=b)
    m1.update(X[:200], y[:200])
    for i in range(200, 260, 20):
        m1.update(X[i:i + 20], y[i:i + 20])
    m2 = HipGPRegression(names, bounds=b)
    m2.update(X[:200], y[:200])          # same initial heuristics (they depend on the first batch)
    m2._X, m2._Y = X.copy(), y.copy()
    m2._handle.set_data(X, y)
    m2._refit()
    xs = np.random.RandomState(1).uniform(-2, 2, (5, 2))
    a, b2 = m1.predict(xs), m2.predict(xs)
    _close(a[0], b2[0], 1e-9, 'mu: incremental updates vs one rebuild')
    _close(a[1], b2[1], 1e-9, 'var: incremental updates vs one rebuild')
    assert m1.n_evidence == 260 and m1.X.shape == (260, 2) and m1.Y.shape == (260, 1)
    ref = G.Posterior(X, y, **{k: m1._hyper[k] for k in ('var', 'ls', 'bias', 'noise')})
    _close(a[0], ref.predict(xs)[0], 1e-8, 'mu after updates')


def test_metric_shape_n4096_d10(hip_ctx):
    """BASELINE config 3 metric shape: properties that need no O(n^3) CPU pass, plus a
    CPU cross-check of the factor through K = L L^T on a row sample."""
    X, y, bounds = G.synthetic_gp_problem(4096, 10)
    h = G.default_hyper(bounds, y)
    from elfi_amd.gp import GPHandle
    gp = GPHandle(10, 4096)
    gp.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    gp.set_data(X, y)
    logz = gp.factorize()
    L, WT, alpha = gp.get(0), gp.get(1), gp.get(2)
    K = G.kern_K(X, None, h['var'], h['ls'], h['bias'])
    K[np.diag_indices(4096)] += h['noise'] + G.JITTER
    rows = np.random.RandomState(0).choice(4096, 64, replace=False)
    assert np.max(np.abs((L[rows] @ L.T) - K[rows])) <= 1e-10 * np.max(K)        # L L^T = K
    assert np.max(np.abs(K[rows] @ alpha - y[rows])) <= 1e-8 * np.max(np.abs(y))  # K alpha = y
    assert np.max(np.abs(L[rows] @ WT.T - np.eye(4096)[rows])) <= 1e-9            # L L^-1 = I
    assert np.isfinite(logz)
    # prediction at the evidence reproduces y up to the noise-induced shrinkage; variance >= 0
    mu, var = gp.predict(X[:32], noiseless=True)
    assert np.all(var > 0) and np.all(var < h['var'] + h['bias'])
    kx = G.kern_K(X, X[:32], h['var'], h['ls'], h['bias'])
    assert np.max(np.abs(mu - kx.T @ alpha)) <= 1e-9 * np.max(np.abs(mu))


@pytest.mark.parametrize('n0,k,d', [(100, 5, 2), (127, 1, 3), (128, 3, 2), (250, 10, 4), (1000, 30, 10)])
def test_extend_matches_rebuild(hip_ctx, n0, k, d):
    """Bordering (elfihip_gp_extend) == append + full factorisation, incl. crossing a 128 boundary."""
    from elfi_amd.gp import GPHandle
    X, y, bounds = _problem(n0 + k, d, seed=n0 + k)
    h = G.default_hyper(bounds, y)
    a = GPHandle(d, n0 + k)
    a.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    a.set_data(X[:n0], y[:n0])
    a.factorize()
    lz_a = a.extend(X[n0:], y[n0:])
    b = GPHandle(d, n0 + k)
    b.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    b.set_data(X, y)
    lz_b = b.factorize()
    ref = G.Posterior(X, y, h['var'], h['ls'], h['bias'], h['noise'])
    assert abs(lz_a - lz_b) <= 1e-10 * abs(lz_b) and abs(lz_a - ref.log_marginal) <= 1e-9 * abs(ref.log_marginal)
    for which, tol in ((0, 1e-10), (1, 1e-9), (2, 1e-8)):
        _close(a.get(which), b.get(which), tol, 'extend vs rebuild, item %d' % which)
    _close(a.get(0), ref.L, 1e-10, 'L after extend')
    xs = np.random.RandomState(1).uniform(-2, 2, (6, d))
    ma, va = a.predict(xs, noiseless=True)
    rm, rv = ref.predict(xs, noiseless=True)
    _close(ma, rm, 1e-8, 'mu after extend')
    assert np.max(np.abs(va - rv)) <= 1e-8 * (ref.var + ref.bias)
    _, _, dmu, dvar = a.predict_grad(xs)
    gmu, gvar = ref.predictive_gradients(xs)
    _close(dmu, gmu, 1e-8, 'grad mu after extend')
    _close(dvar, gvar, 1e-7, 'grad var after extend')
    _, g = a.nlml_grad()
    assert np.max(np.abs(g - ref.log_marginal_grad())) <= 1e-7 * np.max(np.abs(g))


def test_bolfi_style_updates_use_the_incremental_path(hip_ctx):
    from elfi_amd import HipGPRegression
    X, y, bounds = _problem(300, 2, seed=21)
    names = ['a', 'b']
    m = HipGPRegression(names, bounds=dict(zip(names, bounds)))
    m.update(X[:200], y[:200])
    calls = []
    orig = m._handle.extend
    m._handle.extend = lambda *a: (calls.append(1), orig(*a))[1]
    for i in range(200, 300):
        m.update(X[i:i + 1], y[i:i + 1])
    assert len(calls) == 100 and m.n_evidence == 300
    ref = G.Posterior(X, y, **m._hyper)
    xs = np.random.RandomState(0).uniform(-2, 2, (7, 2))
    _close(m.predict(xs)[0], ref.predict(xs)[0], 1e-8, 'mu after 100 single-point updates')
    assert abs(m._log_marginal - ref.log_marginal) <= 1e-9 * abs(ref.log_marginal)
    m._hyper = dict(m._hyper, ls=0.7)      # a hyper-parameter change forces a rebuild
    m.update(X[:1], y[:1])
    assert len(calls) == 100


def test_against_the_reference_closed_forms(hip_ctx):
    """tests/golden/gp_closed_forms.npz: outputs of the reference's own GPyRegression closed forms
    (gpy_regression.py:127-140,206-218) and LCBSC (acquisition.py:256-301), see oracle/make_golden_gp.py."""
    import os
    from conftest import GOLDEN
    from elfi_amd.gp import GPHandle
    g = np.load(os.path.join(GOLDEN, 'gp_closed_forms.npz'))
    for tag in g['cases']:
        tag = str(tag)
        X, y, xs = g['X_' + tag], g['y_' + tag], g['xs_' + tag]
        var, ls, bias, noise = (float(v) for v in g['hyper_' + tag])
        gp = GPHandle(X.shape[1], X.shape[0])
        gp.set_hyper(var, ls, bias, noise)
        gp.set_data(X, y)
        gp.factorize()
        mu, v = gp.predict(xs, noiseless=False)
        _close(mu[:, 0], g['mu_' + tag], 1e-8, 'mu vs reference closed form ' + tag)
        assert np.max(np.abs(v[:, 0] - g['var_' + tag])) <= 1e-8 * (var + bias + noise)
        _, _, dmu, dvar = gp.predict_grad(xs)
        _close(dmu, g['gmu_' + tag], 1e-8, 'grad mu vs reference closed form ' + tag)
        _close(dvar, g['gvar_' + tag], 1e-7, 'grad var vs reference closed form ' + tag)
        for t in (0, 17):
            val, grad = gp.lcb(xs, float(g['beta_%s_%d' % (tag, t)]))
            _close(val, g['lcb_%s_%d' % (tag, t)], 1e-8, 'LCB vs reference LCBSC ' + tag)
            _close(grad, g['lcbg_%s_%d' % (tag, t)], 1e-7, 'LCB gradient vs reference LCBSC ' + tag)


_ORACLE_CACHE = {}


def _oracle_for(n, d):
    """One CPU posterior per shape (the O(n^3) LAPACK passes are the slow part of these tests)."""
    key = (n, d)
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE.clear()            # at most one large posterior alive (8192^2 doubles = 0.5 GB per matrix)
        X, y, bounds = G.synthetic_gp_problem(n, d, seed=n + d)
        h = G.default_hyper(bounds, y)
        _ORACLE_CACHE[key] = (X, y, bounds, h, G.Posterior(X, y, h['var'], h['ls'], h['bias'], h['noise']))
    return _ORACLE_CACHE[key]


def _fit_with_schedule(X, y, h, schedule, group=0):
    from elfi_amd.gp import GPHandle
    gp = GPHandle(X.shape[1], X.shape[0])
    gp.set_schedule(schedule, group)
    gp.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    gp.set_data(X, y)
    return gp, gp.factorize()


@pytest.mark.parametrize('schedule', [3, 4, 5, 6, -1])
def test_set_schedule_rejects_other_values(hip_ctx, schedule):
    from elfi_amd.gp import GPHandle
    gp = GPHandle(2, 100)
    with pytest.raises(ValueError, match='schedule'):    # ELFIHIP_ERR_ARG
        gp.set_schedule(schedule, 0)


# schedule 1 = two-stream look-ahead with panel groups, 2 = fused steps (include/elfihip.h: elfihip_gp_set_schedule);
# 0 = the size-dependent default.  Block columns nb = ceil(n / 128): every branch of the stream schedule's group / pass
# selection (nb < 30: single panels, fine pass; 30..39: groups of 4, square tiles; 40..47: groups of 2, fine pass;
# >= 48: groups of 4, fine pass) and the fused schedule on both sides of its default range are in the list.
@pytest.mark.parametrize('n,d,schedule,group', [
    (100, 2, 1, 0), (100, 2, 2, 0), (129, 3, 1, 0), (129, 3, 2, 0), (700, 5, 1, 2), (700, 5, 2, 0),
    (1500, 10, 1, 4), (1500, 10, 2, 0), (2500, 4, 1, 0), (2500, 4, 2, 0)])
def test_both_sweep_schedules_vs_oracle(hip_ctx, n, d, schedule, group):
    X, y, bounds, h, post = _oracle_for(n, d)
    gp, logz = _fit_with_schedule(X, y, h, schedule, group)
    assert abs(logz - post.log_marginal) <= 1e-9 * abs(post.log_marginal)
    _close(gp.get(0), post.L, 1e-10, 'L')
    _close(gp.get(1), post.Linv.T, 1e-9, 'L^-T')
    _close(gp.get(2), post.alpha, 1e-8, 'alpha')


@pytest.mark.parametrize('n,d,schedule', [
    (4096, 10, 0), (4096, 10, 1), (4096, 10, 2),      # cfg3 metric shape: nb = 32
    (5120, 10, 0), (5120, 10, 1), (5120, 10, 2),      # nb = 40: stream schedule switches to groups of 2 + fine pass
    (6144, 10, 1), (6144, 10, 2),                     # nb = 48: groups of 4 + fine pass
    (8192, 20, 0), (8192, 20, 1), (8192, 20, 2),      # cfg5 shape: nb = 64
    (10240, 10, 0)])                                  # nb = 80: the fused schedule's largest sizes (default up to 96)
def test_large_n_full_matrix_parity(hip_ctx, n, d, schedule):
    """Every entry of L, L^-T, alpha and the log marginal at the sizes of BASELINE.json configs[2] / configs[4], plus
    mean / variance / gradients / LCB at 64 points, against the CPU posterior (LAPACK)."""
    X, y, bounds, h, post = _oracle_for(n, d)
    gp, logz = _fit_with_schedule(X, y, h, schedule)
    assert abs(logz - post.log_marginal) <= 1e-9 * abs(post.log_marginal)
    _close(gp.get(0), post.L, 1e-10, 'L')
    _close(gp.get(1), post.Linv.T, 1e-9, 'L^-T')
    _close(gp.get(2), post.alpha, 1e-8, 'alpha')
    xs = np.random.RandomState(n).uniform(-2, 2, (64, d))
    xs[0] = X[n // 2]
    mu, var, dmu, dvar = gp.predict_grad(xs)
    rmu, rvar = post.predict(xs, noiseless=True)
    gmu, gvar = post.predictive_gradients(xs)
    _close(mu, rmu, 1e-8, 'mu')
    assert np.max(np.abs(var - rvar)) <= 1e-8 * (post.var + post.bias), 'var'
    _close(dmu, gmu, 1e-8, 'grad mu')
    _close(dvar, gvar, 1e-7, 'grad var')
    for t in (0, 300):
        val, grad = gp.lcb(xs, G.lcb_beta(t, d))
        _close(val, G.lcb_evaluate(post, xs, t), 1e-8, 'lcb')
        _close(grad, G.lcb_evaluate_gradient(post, xs, t), 1e-7, 'lcb grad')
    _, g = gp.nlml_grad()
    assert np.max(np.abs(g - post.log_marginal_grad())) <= 1e-7 * np.max(np.abs(g))
    if schedule == 0 and n in (4096, 8192):
        # a 256-point block (configs[4]'s parallel starts): the dense form of the two products
        xs = np.random.RandomState(n + 1).uniform(-2, 2, (256, d))
        mu, var, dmu, dvar = gp.predict_grad(xs)
        rmu, rvar = post.predict(xs, noiseless=True)
        gmu, gvar = post.predictive_gradients(xs)
        _close(mu, rmu, 1e-8, 'mu (256 points)')
        assert np.max(np.abs(var - rvar)) <= 1e-8 * (post.var + post.bias), 'var (256 points)'
        _close(dmu, gmu, 1e-8, 'grad mu (256 points)')
        _close(dvar, gvar, 1e-7, 'grad var (256 points)')


def test_prior_kernel_matrix_is_gpys_kern_K(hip_ctx):
    """`model._gp.kern.K(X, X2)` (what the reference's ExpIntVar evaluates through GPy, acquisition.py:754,770) on the
    device: rbf + bias with [GPy-upstream] Stationary's squared distances, exact diagonal for X2 = None."""
    from elfi_amd import HipGPRegression
    rs = np.random.RandomState(4)
    names = ['a', 'b', 'c']
    m = HipGPRegression(names, bounds={k: (-2, 2) for k in names})
    X, y = rs.uniform(-2, 2, (40, 3)), rs.randn(40, 1)
    m.update(X, y)
    m._hyper = dict(var=1.7, ls=0.6, bias=0.3, noise=0.05)
    m._refit()
    A, B = rs.uniform(-2, 2, (17, 3)), rs.uniform(-2, 2, (5, 3))

    def ref(P, Q=None):
        same = Q is None
        Q = P if same else Q
        r2 = (np.sum(P * P, 1)[:, None] + np.sum(Q * Q, 1)[None, :]) - 2.0 * P @ Q.T
        r2 = np.clip(r2, 0, np.inf)
        if same:
            np.fill_diagonal(r2, 0.0)
        return 1.7 * np.exp(-0.5 * r2 / 0.6 ** 2) + 0.3

    np.testing.assert_allclose(m._gp.kern.K(A, B), ref(A, B), rtol=1e-13, atol=1e-15)
    K = m._gp.kern.K(A)
    np.testing.assert_allclose(K, ref(A), rtol=1e-13, atol=1e-15)
    assert np.all(np.diag(K) == 1.7 + 0.3) and K.shape == (17, 17)
    np.testing.assert_allclose(m._gp.kern.K(X)[:5, :5], ref(X)[:5, :5], rtol=1e-13)


@pytest.mark.parametrize('n,d,S,tm', [(300, 2, 100, 0), (300, 2, 100, 64), (1000, 10, 256, 32), (1000, 10, 256, 16),
                                      (2048, 10, 200, 0), (4096, 10, 256, 64), (4096, 10, 256, 0), (4100, 3, 97, 16),
                                      (8192, 20, 256, 0), (8192, 20, 70, 0)])
def test_dense_form_of_the_products_vs_streaming_form_and_oracle(hip_ctx, n, d, S, tm):
    """Calls with many points run both triangular products as dense 64 x 64 MFMA tiles (csrc/gp_dense.hip).  Same
    quantities as the streaming form: compared with it on the same GP (1e-11: two summation orders of one formula) and
    with the CPU posterior at the usual tolerances (gpy_regression.py:127-140,206-218)."""
    X, y, bounds = _problem(n, d, seed=n + S)
    gp, _, ref = _fit(X, y, bounds)
    xs = np.random.RandomState(5).uniform(-2, 2, (S, d))
    xs[0] = X[n // 3]
    beta = G.lcb_beta(7, d)
    gp.set_dense_threshold(1 << 40)                   # streaming form for every call
    m0, v0, dm0, dv0 = gp.predict_grad(xs)
    val0, g0 = gp.lcb(xs, beta)
    mm0, vv0 = gp.predict(xs, noiseless=False)
    gp.set_dense_threshold(64, tm)                    # dense form, row tiles of tm (0: by size)
    m1, v1, dm1, dv1 = gp.predict_grad(xs)
    val1, g1 = gp.lcb(xs, beta)
    mm1, vv1 = gp.predict(xs, noiseless=False)
    _close(m1, m0, 1e-12, 'mu dense/stream')
    assert np.max(np.abs(v1 - v0)) <= 1e-11 * (ref.var + ref.bias)
    assert np.max(np.abs(vv1 - vv0)) <= 1e-11 * (ref.var + ref.bias) and np.array_equal(mm1, m1)
    _close(dm1, dm0, 1e-11, 'grad mu dense/stream')
    _close(dv1, dv0, 1e-10, 'grad var dense/stream')
    _close(val1, val0, 1e-11, 'lcb dense/stream')
    _close(g1, g0, 1e-10, 'lcb grad dense/stream')
    if n <= 4100:
        rmu, rvar = ref.predict(xs, noiseless=True)
        gmu, gvar = ref.predictive_gradients(xs)
        _close(m1, rmu, 1e-8, 'mu')
        assert np.max(np.abs(v1 - rvar)) <= 1e-8 * (ref.var + ref.bias), 'var'
        _close(dm1, gmu, 1e-8, 'grad mu')
        _close(dv1, gvar, 1e-7, 'grad var')
    gp.set_dense_threshold(0)


def test_dense_form_many_points_in_rounds(hip_ctx):
    """S far above one round of the dense predictor (rounds of at most 4096 points reuse one workspace, csrc/gp_dense.hip):
    a posterior evaluated on a grid -- every point equals its own small call, ragged last round included."""
    n, d, S = 1500, 3, 9001
    X, y, bounds = _problem(n, d, seed=77)
    gp, _, ref = _fit(X, y, bounds)
    xs = np.random.RandomState(3).uniform(-2, 2, (S, d))
    m, v, dm, dv = gp.predict_grad(xs)
    assert m.shape[0] == S and np.all(np.isfinite(m)) and np.all(np.isfinite(dv))
    for lo in (0, 4000, 4096 - 3, 8192 - 1, S - 70):
        sl = slice(lo, lo + 70)
        ms, vs, dms, dvs = gp.predict_grad(xs[sl])
        _close(m[sl], ms, 1e-12, 'mu rounds')
        assert np.max(np.abs(v[sl] - vs)) <= 1e-11 * (ref.var + ref.bias)
        _close(dm[sl], dms, 1e-11, 'grad mu rounds')
        _close(dv[sl], dvs, 1e-10, 'grad var rounds')
    rmu, rvar = ref.predict(xs[-50:], noiseless=True)
    _close(m[-50:], rmu, 1e-8, 'mu')


@pytest.mark.parametrize('n,d,S', [(700, 5, 10), (2100, 2, 16), (4096, 10, 10), (1000, 20, 40)])
def test_fused_lockstep_form_equals_the_six_launch_form(hip_ctx, n, d, S):
    """elfihip_gp_set_lockstep_form: the reduction of the first product's partials and the gradient sums of the second as
    epilogues of the last workgroup to arrive at a row block (write-through partials, relaxed arrival, one acquire) against
    the same work as kernels of their own.  Mean / variance / LCB value: bit for bit (same summation order); gradients to
    rounding (32- against 64-row chunks).  Many calls in a row: a stale read of another workgroup's partials would show."""
    X, y, bounds = _problem(n, d, seed=n + S)
    gp, _, ref = _fit(X, y, bounds)
    rs = np.random.RandomState(1)
    for rep in range(25):
        xs = rs.uniform(-2, 2, (S, d))
        gp.set_lockstep_form(1)
        m0, v0, dm0, dv0 = gp.predict_grad(xs)
        val0, g0 = gp.lcb(xs, 3.0)
        gp.set_lockstep_form(0)
        m1, v1, dm1, dv1 = gp.predict_grad(xs)
        val1, g1 = gp.lcb(xs, 3.0)
        assert np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(val0, val1), rep
        _close(dm1, dm0, 1e-12, 'grad mu')
        _close(dv1, dv0, 1e-11, 'grad var')
        _close(g1, g0, 1e-11, 'lcb grad')
    rmu, rvar = ref.predict(xs, noiseless=True)
    _close(m1, rmu, 1e-8, 'mu')


@pytest.mark.parametrize('n', [12, 126, 200])
def test_extend_on_a_jittered_factor_restarts_at_the_known_rung(hip_ctx, n):
    """elfihip_gp_extend on a factor that carries jitchol jitter rebuilds (GPy rebuilds on every update) -- from round 6 on
    starting at the rung the current factor needed instead of repeating the plain attempt (a full sweep that must fail at
    the same pivot, plus a memset of the whole L^-T matrix, per evidence point).  The outcome is the full ladder's: the same
    (jitter, tries), log Z and factor, bit for bit, as a fresh factorisation of all the evidence; across a 128 boundary too."""
    from elfi_amd.gp import GPHandle
    X, y, h = _jitter_problem(n + 5)
    a = GPHandle(2, n + 5)
    a.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    a.set_data(X[:n], y[:n])
    a.factorize()
    assert a.jitchol()[1] == 1
    for i in range(n, n + 5):
        lz = a.extend(X[i:i + 1], y[i:i + 1])
        b = GPHandle(2, n + 5)
        b.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
        b.set_data(X[:i + 1], y[:i + 1])
        lzb = b.factorize()
        assert a.jitchol() == b.jitchol() and a.jitchol()[1] == 1
        assert lz == lzb, (i, lz, lzb)
        assert np.array_equal(a.get(0), b.get(0)) and np.array_equal(a.get(2), b.get(2))
        b.close()
    # hyper-parameters that need no jitter: the next factorisation is a plain one again
    a.set_hyper(1.0, 1.0, 0.0, 0.5)
    a.factorize()
    assert a.jitchol() == (0.0, 0)
