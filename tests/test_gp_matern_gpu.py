"""GPU: the Matern 3/2 and 5/2 covariance functions of the device GP (elfihip_gp_set_kernel, HipGPRegression(kernel=...))
against the NumPy restatement tests/matern_ref.py (no reference fixture exists for these kernels: GPy is not installed where
fixtures are made; tests/test_gp_matern.py holds the restatement to a 40-digit evaluation).

Tolerances are those the same quantities have under the RBF kernel: tests/test_gp_ard_gpu.py (mean and its gradient 1e-8,
gradient of the variance 1e-7, lcb 1e-8 and its gradient 1e-7, MaxVar 1e-7 and its gradient 1e-5 of the largest entry,
variance 1e-8 (var + bias), kernel matrix rtol 1e-12, log Z 1e-9, hyper-gradients 1e-7 of the largest component),
tests/test_gp_gpu.py for the dense against the streaming form (1e-12 .. 1e-10) and tests/test_lockstep_kinv_gpu.py for the
K^-1 lock-step against the triangular one (1e-9, gradient 1e-8), tests/test_maxvar_surfaces_gpu.py for the posterior
covariance (1e-10) and the ExpIntVar loss (1e-7).  The kernel matrix of nearly coincident rows alone gets more: the squared
distance (|a|^2 + |b|^2) - 2 a.b cancels there, and the bound adds 16 x the largest error the restatement's own GPy-form
kernel matrix (matern_ref.kern_gpy) has against mpmath on the same inputs -- the restatement's error, never the device's.
"""
import os
import sys

import numpy as np
import pytest

import acquisition_oracle as AO
import matern_ref as M

pytestmark = pytest.mark.gpu

KINDS = ['matern32', 'matern52']


def _problem(n, d, seed):
    """Evidence with a kink: y = |x_0 - 0.3| + a smooth part."""
    rs = np.random.RandomState(seed)
    X = rs.uniform(-2, 2, (n, d))
    y = np.abs(X[:, 0] - 0.3) + 0.2 * np.sum(np.sin(X), axis=1) / np.sqrt(d) + 1.0 + 0.05 * rs.randn(n)
    return X, y[:, None]


def _hyper(d):
    """Lengthscale times sqrt(d / 2) for d > 2 (tests/test_gp_hyper_gpu.py: without it K is the identity to rounding)."""
    return dict(var=1.2, ls=1.7 * (np.sqrt(d / 2.0) if d > 2 else 1.0), bias=0.5, noise=0.02)


_CACHE = {}


def _case(kind, n, d):
    """(X, y, hyper, restatement) of one shape, computed once and never modified."""
    if (kind, n, d) not in _CACHE:
        X, y = _problem(n, d, seed=n + d)
        h = _hyper(d)
        _CACHE[(kind, n, d)] = (X, y, h, M.MaternPosterior(X, y, kind, h['var'], h['ls'], h['bias'], h['noise']))
    return _CACHE[(kind, n, d)]


def _handle(X, y, h, kind, cap=None, form=0):
    from elfi_amd.gp import GPHandle
    gp = GPHandle(X.shape[1], cap or X.shape[0], kernel=kind)
    assert gp.get_kernel() == kind
    gp.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    gp.set_data(X, y)
    logz = gp.factorize()
    gp.set_lockstep_form(form)
    return gp, logz


def _err(a, b):
    return np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300)


def _close(a, b, tol, what):
    assert a.shape == b.shape, what
    e = _err(a, b)
    assert np.all(np.isfinite(a)) and e <= tol, '%s: %g of the largest > %g' % (what, e, tol)


def _queries(X, S, seed):
    xs = np.random.RandomState(seed).uniform(-2, 2, (S, X.shape[1]))
    xs[0] = X[len(X) // 3]            # r = 0 exactly against one evidence row
    if S > 2:
        xs[1] = X[0] + 1e-9
    return xs


def _gauss_prior(xs):
    pdf = np.prod(np.exp(-0.5 * ((xs - 0.3) / 3.0) ** 2) / (3.0 * np.sqrt(2 * np.pi)), axis=1)
    return pdf, -(xs - 0.3) / 9.0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_set_kernel_entry_point(hip_ctx):
    from elfi_amd.gp import GPHandle
    X, y = _problem(20, 2, 1)
    gp = GPHandle(2, 20)
    assert gp.get_kernel() == 'rbf'
    for bad in (-1, 3, 17):
        with pytest.raises(Exception):
            gp.set_kernel(bad)
        assert gp.get_kernel() == 'rbf'
    gp.set_hyper(1.2, 1.7, 0.5, 0.02)
    gp.set_data(X, y)
    gp.factorize()
    mu0, _ = gp.predict(X[:3])
    gp.set_kernel('matern32')                         # like set_hyper: the factorisation belongs to the old kernel
    assert gp.get_kernel() == 'matern32'
    with pytest.raises(Exception):
        gp.predict(X[:3])
    gp.factorize()
    mu1, _ = gp.predict(X[:3])
    ref = M.MaternPosterior(X, y, 'matern32', 1.2, 1.7, 0.5, 0.02)
    _close(mu1, ref.predict(X[:3])[0], 1e-8, 'mean after the change of kernel')
    assert not np.array_equal(mu0, mu1)
    gp.set_kernel(0)
    gp.factorize()
    assert np.array_equal(gp.predict(X[:3])[0], mu0)
    gp.close()


# ---- 1. prior covariance: kernel_matrix and cross_cov --------------------------------------------------------------------
def _edge_rows(d, ls):
    """Rows at |x| ~ 10: eight pairs 1e-9 apart (the cancellation in r2), two rows 60 lengthscales apart (underflow of the
    exponential's tail), well separated ones; B repeats rows of A (r = 0 exactly)."""
    rs = np.random.RandomState(100 + d)
    base = rs.randn(8, d)
    base *= 10.0 / np.linalg.norm(base, axis=1)[:, None]
    near = base + 1e-9 * rs.choice([-1.0, 1.0], (8, d))
    far = np.zeros((2, d))
    far[0, 0], far[1, 0] = -30.0 * ls, 30.0 * ls
    A = np.concatenate([base, near, far, rs.uniform(-2, 2, (4, d)) * ls])
    B = np.concatenate([A[[0, 9, 16]], A[:8] + 1e-9, rs.uniform(-2, 2, (3, d)) * ls, far[:1]])
    return A, B


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d', [1, 2, 3, 7, 16, 256])
def test_kernel_matrix_with_coincident_near_and_far_rows(hip_ctx, kind, d):
    from elfi_amd.gp import GPHandle
    ls = 0.3
    A, B = _edge_rows(d, ls)
    gp = GPHandle(d, 8, kernel=kind)
    gp.set_hyper(1.2, ls, 0.5, 0.02)
    K, Ks = gp.kernel_matrix(A, B), gp.kernel_matrix(A)
    gp.close()
    exact, exact_s = M.kern_mp(kind, A, B, 1.2, ls, 0.5), M.kern_mp(kind, A, A, 1.2, ls, 0.5)
    ref, ref_s = M.kern_gpy(kind, A, B, 1.2, ls, 0.5), M.kern_gpy(kind, A, None, 1.2, ls, 0.5)
    own = max(np.max(np.abs(ref - exact)), np.max(np.abs(ref_s - exact_s)))       # the restatement's own error
    dev = max(np.max(np.abs(K - exact)), np.max(np.abs(Ks - exact_s)))
    print('kernel matrix %s d %d: restatement against mpmath %.3g, device against mpmath %.3g' % (kind, d, own, dev))
    assert np.all(np.isfinite(K)) and np.all(np.isfinite(Ks))
    assert np.all(np.abs(K - ref) <= 1e-12 * np.abs(ref) + 16 * own), np.max(np.abs(K - ref))
    assert np.all(np.abs(Ks - ref_s) <= 1e-12 * np.abs(ref_s) + 16 * own), np.max(np.abs(Ks - ref_s))
    assert np.all(np.diag(Ks) == 1.2 + 0.5) and np.array_equal(Ks, Ks.T)
    # 60 lengthscales apart: the stationary part is gone (finite, no NaN from the tail), the bias stays
    assert abs(Ks[16, 17] - 0.5) <= 1e-15 and K[16, -1] == 1.2 + 0.5


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,d,Mi,S', [(5, 1, 3, 1), (63, 2, 17, 10), (65, 7, 33, 65), (257, 3, 40, 17)])
def test_cross_cov_and_expintvar(hip_ctx, kind, n, d, Mi, S):
    X, y, h, ref = _case(kind, n, d)
    gp, _ = _handle(X, y, h, kind)
    P = np.random.RandomState(Mi).uniform(-2, 2, (Mi, d))
    Q = _queries(X, S, seed=S + 1)
    Q[-1] = P[Mi // 2]                                  # a query equal to an integration point: r = 0 in cross_finish_kernel
    gp.set_integration_points(P)
    cov, var = gp.cross_cov(Q)
    rcov = ref.cross_cov(P, Q)
    rmu, rvar = ref.predict(Q, noiseless=True)
    assert cov.shape == (Mi, S) and np.all(np.isfinite(cov))
    assert np.max(np.abs(cov - rcov)) / max(1.0, np.max(np.abs(rcov))) <= 1e-10
    assert np.max(np.abs(var - rvar[:, 0])) <= 1e-8 * (h['var'] + h['bias'])
    w = np.random.RandomState(Mi + 1).uniform(0.05, 1.0, Mi)
    mean_int, var_int = (a[:, 0] for a in ref.predict(P, noiseless=True))
    eps = float(np.percentile(y, 20))
    loss = gp.expintvar(Q, eps, w, mean_int, var_int)
    rloss = AO.expintvar_loss(rcov.T, rvar[:, 0], h['noise'], eps, w, mean_int, var_int)
    _close(loss, np.asarray(rloss).reshape(loss.shape), 1e-7, 'ExpIntVar loss')
    gp.close()


# ---- 2. predictions: VALU and dense form, lock-steps with and without K^-1 ---------------------------------------------
PREDICT_CASES = [(1, 1, 1), (5, 2, 10), (63, 3, 65), (64, 7, 10), (65, 16, 65), (257, 3, 10), (257, 2, 65), (65, 256, 10)]


def _reference_outputs(ref, xs, beta, eps, pdf, glog):
    mu, var = ref.predict(xs, noiseless=True)
    dmu, dvar = ref.predictive_gradients(xs)
    val, grad = ref.lcb(xs, beta)
    return dict(mu=mu, var=var, dmu=dmu, dvar=dvar, lcb=val, lcb_grad=grad,
                maxvar=AO.maxvar_value(mu, var, ref.noise, eps, pdf),
                maxvar_grad=AO.maxvar_gradient(mu, var, dmu, dvar, ref.noise, eps, pdf, glog))


TOL = dict(mu=1e-8, dmu=1e-8, dvar=1e-7, lcb=1e-8, lcb_grad=1e-7, maxvar=1e-7, maxvar_grad=1e-5)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,d,S', PREDICT_CASES)
def test_predictions_and_surfaces_vs_restatement(hip_ctx, kind, n, d, S):
    X, y, h, ref = _case(kind, n, d)
    xs = _queries(X, S, seed=S + d)
    pdf, glog = _gauss_prior(xs)
    eps, beta = float(np.percentile(y, 20)), 4.0
    want = _reference_outputs(ref, xs, beta, eps, pdf, glog)
    top = h['var'] + h['bias']
    gp, logz = _handle(X, y, h, kind)
    assert abs(logz - ref.log_marginal) <= 1e-9 * abs(ref.log_marginal)
    gp.set_dense_threshold(1 << 40)                    # the streaming (VALU) form for every call
    mu, var, dmu, dvar = gp.predict_grad(xs)
    sv, sg = gp.maxvar(xs, eps, pdf, glog)
    got = dict(mu=mu, var=var, dmu=dmu, dvar=dvar, maxvar=sv, maxvar_grad=sg)
    # the lock-step's three forms: fused triangular products (2), six launches (1), ONE product with K^-1 (3)
    lock = {}
    for form in (2, 1, 3):
        gp.set_lockstep_form(form)
        lock[form] = gp.lcb(xs, beta)
        if form == 3:
            assert gp.lockstep_info()[0], 'K^-1 in use'
        _close(lock[form][0], want['lcb'], TOL['lcb'], 'lcb, form %d' % form)
        _close(lock[form][1], want['lcb_grad'], TOL['lcb_grad'], 'lcb gradient, form %d' % form)
    _close(lock[3][0], lock[2][0], 1e-9, 'lcb: K^-1 product against the triangular products')
    _close(lock[3][1], lock[2][1], 1e-8, 'lcb gradient: K^-1 product against the triangular products')
    gp.set_lockstep_form(0)
    for k in got:
        if k == 'var':
            assert np.max(np.abs(got[k] - want[k])) <= 1e-8 * top, 'var'
        else:
            _close(got[k], want[k], TOL[k], k)
    # the gradient at the query that IS an evidence row: finite and the restatement's (2 g (x - X) = 0 for that row)
    assert np.all(np.isfinite(dmu[0])) and np.all(np.isfinite(dvar[0]))
    assert np.max(np.abs(dmu[0] - want['dmu'][0])) <= 1e-8 * np.max(np.abs(want['dmu']))
    if S >= 64 and d <= 24:
        # the dense (MFMA) form of the two products, forced at this small n; row tiles by size and of 16
        for tm in (0, 16):
            gp.set_dense_threshold(64, tm)
            m1, v1, dm1, dv1 = gp.predict_grad(xs)
            val1, g1 = gp.lcb(xs, beta)
            _close(m1, mu, 1e-12, 'mu dense/stream')
            assert np.max(np.abs(v1 - var)) <= 1e-11 * top
            _close(dm1, dmu, 1e-11, 'grad mu dense/stream')
            _close(dv1, dvar, 1e-10, 'grad var dense/stream')
            _close(val1, lock[2][0], 1e-11, 'lcb dense/stream')
            _close(g1, lock[2][1], 1e-10, 'lcb grad dense/stream')
            _close(dm1, want['dmu'], TOL['dmu'], 'grad mu, dense')
            _close(dv1, want['dvar'], TOL['dvar'], 'grad var, dense')
            _close(g1, want['lcb_grad'], TOL['lcb_grad'], 'lcb gradient, dense')
        gp.set_dense_threshold(0)
    # the mean alone (csrc/gp_min.hip)
    _close(gp.predict_mean(xs), want['mu'], 1e-8, 'predict_mean')
    gp.close()


# ---- 3. gradients of the log marginal likelihood -----------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n,d', [(1, 1), (5, 2), (65, 3), (257, 7), (260, 48), (64, 256)])
def test_marginal_likelihood_gradients_vs_restatement(hip_ctx, kind, n, d):
    from elfi_amd.gp import GPHandle, ScaledGPHandle
    X, y, h, ref = _case(kind, n, d)
    gp, logz = _handle(X, y, h, kind)
    lz, g = gp.nlml_grad()
    rg = ref.log_marginal_grad(isotropic=True)
    print('%s n %d d %d: log Z %.3g gradient %.3g of the largest' %
          (kind, n, d, abs(lz - ref.log_marginal) / abs(ref.log_marginal), _err(g, rg)))
    assert lz == logz and abs(lz - ref.log_marginal) <= 1e-9 * abs(ref.log_marginal)
    assert np.max(np.abs(g - rg)) <= 1e-7 * np.max(np.abs(rg)), (g, rg)
    # the per-dimension sums on the same (isotropic) object add up to the lengthscale's
    lz1, g4, gd = gp.nlml_grad_ard()
    assert lz1 == lz and gd.shape == (d,) and np.max(np.abs(g4 - g)) <= 1e-12 * np.max(np.abs(g))
    assert abs(gd.sum() - g[1]) <= 1e-7 * np.max(np.abs(g))
    gp.close()
    # one lengthscale per dimension
    ell = h['ls'] * np.exp(np.random.RandomState(d).uniform(-0.5, 0.5, d))
    ard = M.MaternPosterior(X, y, kind, h['var'], ell, h['bias'], h['noise'])
    sg = ScaledGPHandle(d, n, kernel=kind)
    sg.set_hyper(h['var'], ell, h['bias'], h['noise'])
    sg.set_data(X, y)
    lza = sg.factorize()
    lzb, ga = sg.nlml_grad()
    ra = ard.log_marginal_grad()
    assert lzb == lza and abs(lza - ard.log_marginal) <= 1e-9 * abs(ard.log_marginal)
    assert ga.shape == (3 + d,) and np.max(np.abs(ga - ra)) <= 1e-7 * np.max(np.abs(ra)), (ga, ra)
    # fixed summation order: the same bits again
    assert np.array_equal(GPHandle.nlml_grad_ard(sg)[2], GPHandle.nlml_grad_ard(sg)[2])
    sg.close()


@pytest.mark.parametrize('kind', KINDS)
def test_gradients_are_the_derivatives_of_the_devices_log_marginal(hip_ctx, kind):
    from elfi_amd.gp import ScaledGPHandle
    X, y, h, _ = _case(kind, 65, 3)
    gp, _ = _handle(X, y, h, kind)
    _, g = gp.nlml_grad()
    eps = 1e-5
    for i, name in enumerate(('var', 'ls', 'bias', 'noise')):
        f = []
        for s in (eps, -eps):
            hh = dict(h)
            hh[name] += s
            gp.set_hyper(hh['var'], hh['ls'], hh['bias'], hh['noise'])
            f.append(gp.factorize())
        fd = (f[0] - f[1]) / (2 * eps)
        assert abs(fd - g[i]) <= 1e-5 * (1 + abs(g[i])), (name, fd, g[i])
    gp.close()
    ell = np.array([0.8, 2.1, 1.3])
    sg = ScaledGPHandle(3, 65, kernel=kind)
    sg.set_hyper(h['var'], ell, h['bias'], h['noise'])
    sg.set_data(X, y)
    sg.factorize()
    _, ga = sg.nlml_grad()
    for c in range(3):
        f = []
        for s in (eps, -eps):
            e2 = ell.copy()
            e2[c] += s
            sg.set_hyper(h['var'], e2, h['bias'], h['noise'])
            f.append(sg.factorize())
        fd = (f[0] - f[1]) / (2 * eps)
        assert abs(fd - ga[1 + c]) <= 1e-5 * (1 + abs(ga[1 + c])), (c, fd, ga[1 + c])
    sg.close()


# ---- 4. bordering extend -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n0,k,d,form', [(1, 4, 1, 0), (50, 13, 3, 0), (100, 20, 7, 3), (60, 5, 256, 0)])
def test_extend_equals_a_rebuild(hip_ctx, kind, n0, k, d, form):
    X, y = _problem(n0 + k, d, seed=7 + d)
    h = _hyper(d)
    gp, _ = _handle(X[:n0], y[:n0], h, kind, cap=128, form=form)
    xs = _queries(X, 10, seed=3)
    if form == 3:
        gp.lcb(xs, 3.0)
        assert gp.lockstep_info()[0]
    lz = None
    for i in range(n0, n0 + k - 2):
        lz = gp.extend(X[i:i + 1], y[i:i + 1])                          # one row at a time ...
    lz = gp.extend(X[n0 + k - 2:], y[n0 + k - 2:])                      # ... and two together
    full, lzf = _handle(X, y, h, kind, cap=128, form=2)
    assert abs(lz - lzf) <= 1e-10 * abs(lzf)
    a, b = gp.predict_grad(xs), full.predict_grad(xs)
    _close(a[0], b[0], 1e-8, 'mean after extends')
    assert np.max(np.abs(a[1] - b[1])) <= 1e-8 * (h['var'] + h['bias'])
    _close(a[2], b[2], 1e-8, 'gradient of the mean after extends')
    _close(a[3], b[3], 1e-7, 'gradient of the variance after extends')
    va, ga = gp.lcb(xs, 3.0)
    vb, gb = full.lcb(xs, 3.0)
    if form == 3:
        assert gp.lockstep_info()[0], 'extends inside the padded size keep K^-1'
    _close(va, vb, 1e-9, 'lcb after extends')
    _close(ga, gb, 1e-8, 'lcb gradient after extends')
    # append + factorize is the rebuild itself
    app, _ = _handle(X[:n0], y[:n0], h, kind, cap=128)
    app.append(X[n0:], y[n0:])
    assert app.factorize() == lzf
    for g_ in (gp, full, app):
        g_.close()


# ---- 5. per-dimension lengthscales at model level ---------------------------------------------------------------------
NAMES = ['a', 'b', 'c']
BOUNDS = [(-2.0, 2.0), (-1.5, 2.0), (-2.0, 1.0)]


def _evidence():
    rs = np.random.RandomState(12)
    X = rs.uniform([b[0] for b in BOUNDS], [b[1] for b in BOUNDS], (60, 3))
    y = np.abs(X[:, 0] - 0.3) + 0.3 * X[:, 1] ** 2 + 0.2 * X[:, 2] + 1.0 + 0.1 * rs.randn(60)
    return X, y[:, None]


def _model(kind, ard, ls, X=None, y=None):
    from elfi_amd import HipGPRegression
    if X is None:
        X, y = _evidence()
    m = HipGPRegression(NAMES, bounds=dict(zip(NAMES, BOUNDS)), ard=ard, kernel=kind)
    m.update(X, y)
    m.fix_hyperparameters(var=1.2, ls=ls, bias=0.5, noise=0.02)
    return m


def _model_queries():
    X, _ = _evidence()
    xs = np.random.RandomState(13).uniform([b[0] for b in BOUNDS], [b[1] for b in BOUNDS], (9, 3))
    xs[0] = X[4]
    return (xs,) + _gauss_prior(xs)


def _model_outputs(m):
    xs, pdf, glog = _model_queries()
    eps = float(np.percentile(_evidence()[1], 20))
    mu, var = m.predict(xs, noiseless=True)
    dmu, dvar = m.predictive_gradients(xs)
    val, grad = m.lcb(xs, 4.0)
    sv, sg = m.maxvar_surface(xs, eps, pdf, glog)
    return dict(mu=mu, var=var, dmu=dmu, dvar=dvar, lcb=val, lcb_grad=grad, maxvar=sv, maxvar_grad=sg)


def _check_model(m, want):
    got = _model_outputs(m)
    for k, t in TOL.items():
        _close(got[k], want[k], t, k)
    assert np.max(np.abs(got['var'] - want['var'])) <= 1e-8 * 1.7, 'var'


@pytest.mark.parametrize('kind', KINDS)
def test_ard_model_equal_and_unequal_lengthscales(hip_ctx, kind):
    from elfi_amd.gp import ScaledGPHandle
    X, y = _evidence()
    iso, ard = _model(kind, False, 1.7), _model(kind, True, 1.7)
    assert isinstance(ard._handle, ScaledGPHandle) and ard._handle.get_kernel() == kind == iso._handle.get_kernel()
    _check_model(ard, _model_outputs(iso))
    assert abs(ard._log_marginal - iso._log_marginal) <= 1e-9 * abs(iso._log_marginal)
    ell = np.array([0.8, 2.1, 1.3])
    m = _model(kind, True, ell)
    ref = M.MaternPosterior(X, y, kind, 1.2, ell, 0.5, 0.02)
    assert abs(m._log_marginal - ref.log_marginal) <= 1e-9 * abs(ref.log_marginal)
    xs, pdf, glog = _model_queries()
    _check_model(m, _reference_outputs(ref, xs, 4.0, float(np.percentile(y, 20)), pdf, glog))
    # the stand-in for GPy's kern object tells the kind and evaluates it
    kern = m._gp.kern
    assert kern.name == kind and kern.rbf.name == kind and np.array_equal(kern.rbf.lengthscale.values, ell)
    np.testing.assert_allclose(kern.K(X[:5], X[5:9]), ref.kern(X[:5], X[5:9]), rtol=1e-12)
    assert kind in str(m)
    # copies and pickles keep kind and numbers
    import pickle
    mu = m.predict(xs)[0]
    for k in (m.copy(), pickle.loads(pickle.dumps(m))):
        assert k.kernel == kind and k._handle.get_kernel() == kind
        assert np.max(np.abs(k.predict(xs)[0] - mu)) <= 1e-12 * np.max(np.abs(mu))
    # update() extends the scaled factorisation by bordering
    part = _model(kind, True, ell, X[:50], y[:50])
    part.update(X[50:], y[50:])
    assert abs(part._log_marginal - m._log_marginal) <= 1e-10 * abs(m._log_marginal)
    _close(part.predict(xs)[0], mu, 1e-8, 'mean after update')


# ---- 6. behaviour ------------------------------------------------------------------------------------------------------
def test_a_kink_prefers_matern32_and_minimize_mean_finds_it(hip_ctx):
    """Evidence drawn from |x - x0|: the MAP search with the Matern 3/2 kernel ends at a higher log marginal likelihood than
    with the RBF kernel, and the mean's minimiser is the kink."""
    from elfi_amd import HipGPRegression
    rs = np.random.RandomState(0)
    x0 = 0.3
    X = np.sort(rs.uniform(-2, 2, (40, 1)), axis=0)
    y = np.abs(X - x0) + 0.01 * rs.randn(40, 1)
    lz = {}
    for kind in ('rbf', 'matern32'):
        m = HipGPRegression(['x'], bounds={'x': (-2.0, 2.0)}, kernel=kind)
        m.update(X, y)
        m.optimize()
        lz[kind] = m._log_marginal
        xm, fm = m.minimize_mean(seed=3)
        print('%s: log marginal %.4f, hyper %r, minimiser %.4f (%.4f)' % (kind, lz[kind], m._hyper, xm[0], fm))
        if kind == 'matern32':
            assert abs(xm[0] - x0) <= 0.1 and abs(fm) <= 0.1, (xm, fm)
            ref = M.MaternPosterior(X, y, kind, m._hyper['var'], m._hyper['ls'], m._hyper['bias'], m._hyper['noise'])
            assert abs(m._log_marginal - ref.log_marginal) <= 1e-8 * abs(ref.log_marginal)
            assert abs(fm - ref.predict(xm[None])[0][0, 0]) <= 1e-7 * max(1.0, abs(fm))
            assert fm <= ref.predict(np.linspace(-2, 2, 2001)[:, None])[0].min() + 1e-7
    assert lz['matern32'] > lz['rbf'], lz


def test_minimize_mean_vs_restatement(hip_ctx):
    X, y, h, ref = _case('matern52', 65, 3)
    gp, _ = _handle(X, y, h, 'matern52')
    x, f, info, pop, en = gp.minimize_mean([(-2.0, 2.0)] * 3, seed=5)
    assert abs(f - ref.predict(x[None])[0][0, 0]) <= 1e-8 * abs(f)
    probe = np.random.RandomState(15).uniform(-2, 2, (2000, 3))
    assert f <= ref.predict(probe)[0].min() + 1e-8
    again = gp.minimize_mean([(-2.0, 2.0)] * 3, seed=5)
    assert np.array_equal(again[0], x) and again[1] == f
    gp.close()


ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle')


def test_hip_bolfi_fit_and_sample_with_matern52(hip_ctx):
    """One short HipBOLFI run on MA2 with the Matern 5/2 surrogate: fit, posterior, NUTS sample."""
    sys.path.insert(0, ORACLE)
    import ref_shim
    if not ref_shim.available():
        pytest.skip('no reference package (run oracle/make_ref.sh)')
    elfi = ref_shim.install()
    import elfi.clients.native as native
    native.set_as_default()
    import elfi_amd
    from elfi.examples import ma2
    m = ma2.get_model(seed_obs=1)
    log_d = elfi.Operation(np.log, m['d'], name='log_d')
    bounds = {'t1': (-2, 2), 't2': (-1, 1)}
    gp = elfi_amd.HipGPRegression(['t1', 't2'], bounds=bounds, kernel='matern52')
    bolfi = elfi_amd.HipBOLFI(log_d, batch_size=1, initial_evidence=20, update_interval=10, bounds=bounds,
                              target_model=gp, acq_noise_var=0.1, seed=1)
    post = bolfi.fit(n_evidence=40, bar=False)
    assert isinstance(post, elfi_amd.HipBolfiPosterior)
    assert bolfi.target_model is gp and gp.n_evidence == 40 and gp._handle.get_kernel() == 'matern52'
    res = bolfi.sample(100, n_chains=2)
    assert res.chains.shape == (2, 100, 2) and np.all(np.isfinite(res.chains))
    t1, t2 = res.samples['t1'], res.samples['t2']
    assert np.all((t1 >= -2) & (t1 <= 2) & (t2 >= -1) & (t2 <= 1))
    assert np.all(np.isfinite(post.logpdf(np.array([[0.6, 0.2], [0.0, 0.0]]))))


# ---- 7. the RBF kernel is untouched ---------------------------------------------------------------------------------
def test_rbf_by_name_is_the_default_model_bit_for_bit(hip_ctx):
    from elfi_amd import HipGPRegression
    X, y = _evidence()
    xs, pdf, glog = _model_queries()
    out = []
    for kw in (dict(), dict(kernel='rbf'), dict(kernel='RBF')):
        m = HipGPRegression(NAMES, bounds=dict(zip(NAMES, BOUNDS)), **kw)
        m.update(X, y)
        m.fix_hyperparameters(var=1.2, ls=1.7, bias=0.5, noise=0.02)
        assert m._handle.get_kernel() == 'rbf'
        big = np.random.RandomState(2).uniform(-2, 1, (130, 3))             # the dense form too
        out.append(m.predict(xs) + m.predictive_gradients(xs) + m.lcb(xs, 4.0) + m.predict(big)
                   + (np.asarray(m._handle.nlml_grad()[1]), np.asarray([m._log_marginal])))
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)
