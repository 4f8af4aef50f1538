"""GPU: per-dimension (ARD) lengthscales -- elfihip_gp_nlml_grad_ard and HipGPRegression(ard=True) against the NumPy
restatement tests/ard_ref.py (no reference fixture exists for this kernel: GPy is not installed where fixtures are made).

Gradient tolerances are those of tests/test_gp_hyper_gpu.py: the largest deviation at most 1e-7 of the largest component,
log Z within 1e-9 relative.
"""
import numpy as np
import pytest

import acquisition_oracle as AO
import ard_ref as A
import gp_oracle as G

pytestmark = pytest.mark.gpu

# one tile; the tile edge; three block rows with k chunks; dp padding; both sides of the X-in-LDS limit (dp 44 | 48); d = 256
GRAD_CASES = [(7, 1), (127, 3), (129, 4), (300, 5), (300, 10), (260, 44), (260, 48), (200, 256)]
_CACHE = {}


def _case(n, d):
    """(X, y, hyper with ell, restatement) of one gradient case, computed once: the default hyper-parameters, the
    lengthscale times sqrt(d / 2) when d > 2 (tests/test_gp_hyper_gpu.py: _scaled_hyper -- without it K is the identity to
    rounding and X does not matter), each dimension's times exp(U(-0.5, 0.5)) drawn from RandomState(d)."""
    if (n, d) not in _CACHE:
        X, y, bounds = G.synthetic_gp_problem(n, d, seed=n + d)
        h = dict(G.default_hyper(bounds, y))
        ls = h.pop('ls') * (np.sqrt(d / 2.0) if d > 2 else 1.0)
        h['ell'] = ls * np.exp(np.random.RandomState(d).uniform(-0.5, 0.5, d))
        _CACHE[(n, d)] = (X, y, h, A.ArdPosterior(X, y, h['var'], h['ell'], h['bias'], h['noise']))
    return _CACHE[(n, d)]


def _scaled_handle(X, y, h):
    from elfi_amd.gp import ScaledGPHandle
    gp = ScaledGPHandle(X.shape[1], X.shape[0])
    gp.set_hyper(h['var'], h['ell'], h['bias'], h['noise'])
    gp.set_data(X, y)
    return gp, gp.factorize()


@pytest.mark.parametrize('n,d', GRAD_CASES)
def test_ard_gradient_vs_restatement(hip_ctx, n, d):
    from elfi_amd.gp import GPHandle
    X, y, h, ref = _case(n, d)
    gp, logz = _scaled_handle(X, y, h)
    rg = ref.log_marginal_grad()
    # the test is not vacuous: every lengthscale's derivative is a visible share of the largest
    assert np.min(np.abs(rg[1:-2])) >= 1e-2 * np.max(np.abs(rg[1:-2])), rg
    lz, g = gp.nlml_grad()
    print('n %d d %d: log Z %.3g  gradient %.3g of the largest' %
          (n, d, abs(lz - ref.log_marginal) / abs(ref.log_marginal), np.max(np.abs(g - rg)) / np.max(np.abs(rg))))
    assert lz == logz and abs(lz - ref.log_marginal) <= 1e-9 * abs(ref.log_marginal)
    assert g.shape == (3 + d,)
    assert np.max(np.abs(g - rg)) <= 1e-7 * np.max(np.abs(rg)), (g, rg)
    # the raw entry point next to the isotropic one on the same handle: the four sums, and the d sums add up to the
    # lengthscale's (the device object holds x / l under lengthscale 1)
    lz0, g0 = GPHandle.nlml_grad(gp)
    lz1, g4, gd = GPHandle.nlml_grad_ard(gp)
    assert lz0 == lz1 == lz and gd.shape == (d,)
    both = np.concatenate([g4, [gd.sum()]]), np.concatenate([g0, [g0[1]]])
    assert np.max(np.abs(both[0] - both[1])) <= 1e-7 * np.max(np.abs(g0)), (g4, gd.sum(), g0)
    # fixed summation order: the same bits again
    lz2, g4b, gdb = GPHandle.nlml_grad_ard(gp)
    assert lz2 == lz1 and np.array_equal(g4b, g4) and np.array_equal(gdb, gd)
    gp.close()


def test_ard_gradient_is_the_derivative_of_the_log_marginal(hip_ctx):
    X, y, h, ref = _case(300, 5)
    gp, _ = _scaled_handle(X, y, h)
    _, g = gp.nlml_grad()
    eps = 1e-5
    for c in (1, 3):
        f = []
        for s in (eps, -eps):
            ell = h['ell'].copy()
            ell[c] += s
            gp.set_hyper(h['var'], ell, h['bias'], h['noise'])
            f.append(gp.factorize())
        fd = (f[0] - f[1]) / (2 * eps)
        assert abs(fd - g[1 + c]) <= 1e-5 * (1 + abs(g[1 + c])), (c, fd, g[1 + c])
    gp.close()


# ---- model level: d = 3, n = 60 --------------------------------------------------------------------------------------
def relevance_problem():
    """60 points in [-2, 2]^3 whose y depends on x_0 alone."""
    rs = np.random.RandomState(0)
    X = rs.uniform(-2, 2, (60, 3))
    y = (np.sin(2.0 * X[:, 0]) + 1.5 + 0.05 * rs.randn(60))[:, None]
    return X, y, [(-2., 2.)] * 3


NAMES = ['a', 'b', 'c']
BOUNDS = [(-2.0, 2.0), (-1.5, 2.0), (-2.0, 1.0)]


def _evidence():
    rs = np.random.RandomState(12)
    X = rs.uniform([b[0] for b in BOUNDS], [b[1] for b in BOUNDS], (60, 3))
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] ** 2 + 0.2 * X[:, 2] + 1.0 + 0.1 * rs.randn(60)
    return X, y[:, None]


def _model(ard, ls, X=None, y=None):
    from elfi_amd import HipGPRegression
    if X is None:
        X, y = _evidence()
    m = HipGPRegression(NAMES, bounds=dict(zip(NAMES, BOUNDS)), ard=ard)
    m.update(X, y)
    m.fix_hyperparameters(var=1.2, ls=ls, bias=0.5, noise=0.02)
    return m


def _queries():
    X, _ = _evidence()
    xs = np.random.RandomState(13).uniform([b[0] for b in BOUNDS], [b[1] for b in BOUNDS], (9, 3))
    xs[0] = X[4]
    pdf = np.prod(np.exp(-0.5 * ((xs - 0.3) / 3.0) ** 2) / (3.0 * np.sqrt(2 * np.pi)), axis=1)
    return xs, pdf, -(xs - 0.3) / 9.0


def _check_outputs(m, want, scale_var):
    """predict / predictive_gradients / lcb / maxvar_surface of the model against `want` (the same outputs of a reference),
    with the tolerances tests/test_gp_gpu.py (mean and its gradient 1e-8 and lcb 1e-8 of the largest entry, variance 1e-8
    (var + bias), gradient of the variance and of lcb 1e-7) and tests/test_maxvar_gpu.py / test_maxvar_surfaces_gpu.py (value
    1e-7, gradient 1e-5 of the largest) apply to those quantities."""
    xs, pdf, glog = _queries()
    eps = float(np.percentile(_evidence()[1], 20))
    mu, var = m.predict(xs, noiseless=True)
    dmu, dvar = m.predictive_gradients(xs)
    val, grad = m.lcb(xs, 4.0)
    sv, sg = m.maxvar_surface(xs, eps, pdf, glog)
    got = dict(mu=mu, var=var, dmu=dmu, dvar=dvar, lcb=val, lcb_grad=grad, maxvar=sv, maxvar_grad=sg)
    tol = dict(mu=1e-8, dmu=1e-8, dvar=1e-7, lcb=1e-8, lcb_grad=1e-7, maxvar=1e-7, maxvar_grad=1e-5)
    for k, t in tol.items():
        err = np.max(np.abs(got[k] - want[k])) / np.max(np.abs(want[k]))
        assert got[k].shape == want[k].shape and err <= t, '%s: %g of the largest > %g' % (k, err, t)
    assert np.max(np.abs(got['var'] - want['var'])) <= 1e-8 * scale_var, 'var'
    return got


def _restatement_outputs(ref):
    xs, pdf, glog = _queries()
    eps = float(np.percentile(_evidence()[1], 20))
    mu, var = ref.predict(xs, noiseless=True)
    dmu, dvar = ref.predictive_gradients(xs)
    val, grad = ref.lcb(xs, 4.0)
    return dict(mu=mu, var=var, dmu=dmu, dvar=dvar, lcb=val, lcb_grad=grad,
                maxvar=AO.maxvar_value(mu, var, ref.noise, eps, pdf),
                maxvar_grad=AO.maxvar_gradient(mu, var, dmu, dvar, ref.noise, eps, pdf, glog))


def test_equal_lengthscales_reproduce_the_isotropic_model(hip_ctx):
    """An ard=True model with all lengthscales fixed equal against the isotropic model at that lengthscale; tolerances of
    tests/test_gp_gpu.py and tests/test_maxvar_gpu.py as named in _check_outputs."""
    from elfi_amd.gp import ScaledGPHandle
    iso, ard = _model(False, 1.7), _model(True, 1.7)
    assert isinstance(ard._handle, ScaledGPHandle) and not isinstance(iso._handle, ScaledGPHandle)
    assert np.array_equal(ard.hyperparameters['ls'], np.full(3, 1.7)) and iso.hyperparameters['ls'] == 1.7
    xs, pdf, glog = _queries()
    eps = float(np.percentile(_evidence()[1], 20))
    mu, var = iso.predict(xs, noiseless=True)
    dmu, dvar = iso.predictive_gradients(xs)
    val, grad = iso.lcb(xs, 4.0)
    sv, sg = iso.maxvar_surface(xs, eps, pdf, glog)
    _check_outputs(ard, dict(mu=mu, var=var, dmu=dmu, dvar=dvar, lcb=val, lcb_grad=grad, maxvar=sv, maxvar_grad=sg), 1.7)
    assert abs(ard._log_marginal - iso._log_marginal) <= 1e-9 * abs(iso._log_marginal)


def test_unequal_lengthscales_equal_the_restatement(hip_ctx):
    ell = np.array([0.8, 2.1, 1.3])
    X, y = _evidence()
    m = _model(True, ell)
    ref = A.ArdPosterior(X, y, 1.2, ell, 0.5, 0.02)
    assert abs(m._log_marginal - ref.log_marginal) <= 1e-9 * abs(ref.log_marginal)
    _check_outputs(m, _restatement_outputs(ref), 1.7)
    np.testing.assert_allclose(m._gp.kern.K(X[:5], X[5:9]), ref.kern(X[:5], X[5:9]), rtol=1e-12)
    assert np.array_equal(m._gp.param_array, np.concatenate([[1.2], ell, [0.5, 0.02]]))
    assert np.max(np.abs(m._handle.get(3) - X)) <= 1e-15           # (x / l) l: the last bit at most
    # both searches: points inside the ORIGINAL box whose values are the restatement's at those points
    lo, hi = np.array(BOUNDS).T
    starts = np.random.RandomState(14).uniform(lo, hi, (6, 3))
    locs, vals, iters, _ = m._handle.lcb_minimize(starts, BOUNDS, 4.0)
    assert np.all(locs >= lo) and np.all(locs <= hi) and np.all(iters >= 1)
    rv = ref.lcb(locs, 4.0)[0][:, 0]
    assert np.max(np.abs(vals - rv)) <= 1e-8 * np.max(np.abs(rv))
    assert np.all(vals <= ref.lcb(starts, 4.0)[0][:, 0] + 1e-8)           # ... and no worse than where they started
    xm, fm = m.minimize_mean(seed=3)
    assert np.all(xm >= lo) and np.all(xm <= hi)
    assert abs(fm - ref.predict(xm[None])[0][0, 0]) <= 1e-8 * abs(fm)
    probe = np.random.RandomState(15).uniform(lo, hi, (2000, 3))
    assert fm <= ref.predict(probe)[0].min() + 1e-8


def test_update_extends_the_scaled_factorisation(hip_ctx):
    ell = np.array([0.8, 2.1, 1.3])
    X, y = _evidence()
    m = _model(True, ell, X[:50], y[:50])
    m.update(X[50:], y[50:])                       # hyper-parameters unchanged: extended by bordering
    assert m.n_evidence == 60 and np.array_equal(m.hyperparameters['ls'], ell)
    full = _model(True, ell)
    assert abs(m._log_marginal - full._log_marginal) <= 1e-10 * abs(full._log_marginal)
    xs = _queries()[0]
    (mu, var), (rmu, rvar) = m.predict(xs, noiseless=True), full.predict(xs, noiseless=True)
    assert np.max(np.abs(mu - rmu)) <= 1e-8 * np.max(np.abs(rmu)) and np.max(np.abs(var - rvar)) <= 1e-8 * 1.7
    k = m.copy()
    assert k.ard and np.max(np.abs(k.predict(xs)[0] - rmu)) <= 1e-8 * np.max(np.abs(rmu))


def test_optimize_finds_the_relevant_dimension(hip_ctx):
    """Evidence whose y depends on x_0 alone (relevance_problem): optimize() lowers the MAP objective and ends with l_0
    below l_1 and l_2.  On the CPU the restatement's own SCG search from the same start ends at l = (0.82, 7.66, 7.57):
    a factor 9.3 (tests/test_gp_ard.py asserts at least 2 there)."""
    from elfi_amd import HipGPRegression
    from elfi_amd import hyperopt as H
    X, y, bounds = relevance_problem()
    m = HipGPRegression(NAMES, bounds=dict(zip(NAMES, bounds)), ard=True)
    m.update(X, y)
    assert m._hyper['ls'] == (1.0, 1.0, 1.0)
    obj = H.MarginalObjective(m)
    ref_obj = A.MapObjective(X, y, G.default_priors(bounds, y))
    phi0 = H.logexp_inv(H.pack_hyper(m._hyper))
    f0, g0 = obj.f(phi0), obj.grad(phi0)
    assert abs(f0 - ref_obj.value(phi0)) <= 1e-9 * abs(f0)
    assert np.max(np.abs(g0 - ref_obj.gradient(phi0))) <= 1e-7 * np.max(np.abs(g0))
    m.optimize()
    ell = m.hyperparameters['ls']
    assert m._opt_info['objective'][-1] < f0 - 1.0
    assert ell.shape == (3,) and ell[0] < ell[1] and ell[0] < ell[2], ell
    ref = A.ArdPosterior(X, y, m._hyper['var'], ell, m._hyper['bias'], m._hyper['noise'])   # refitted at the optimum
    xs = np.random.RandomState(0).uniform(-2, 2, (5, 3))
    np.testing.assert_allclose(m.predict(xs)[0], ref.predict(xs)[0], rtol=1e-7)
