"""Per-dimension (ARD) lengthscales without a device: the NumPy restatement (tests/ard_ref.py), the diagonal transform of
elfi_amd.gp.DiagonalScaling over a stand-in handle, and the argument handling of HipGPRegression(ard=True).

The stand-in (`NumpyHandle`) answers every method of GPHandle that the transform wraps, in the coordinates it is GIVEN and
with a single lengthscale, from oracle/gp_oracle.py's isotropic posterior -- what the device object does.  The transform in
front of it must then present original coordinates that equal the restatement, which builds K from the per-dimension
lengthscales directly.  Tolerance 1e-9 relative to the largest entry: both sides are float64 LAPACK on a matrix of
condition ~1e4; the two differ in how r^2 is formed (|u|^2 + |u'|^2 - 2 u.u' against differences), 1e-13 or so.
"""
import pickle

import numpy as np
import pytest

import acquisition_oracle as AO
import ard_ref as A
import gp_oracle as G
from elfi_amd import hyperopt as H
from elfi_amd.gp import DiagonalScaling, HipGPRegression

D, N = 3, 40
ELL = np.array([0.7, 1.9, 3.1])
HYP = dict(var=1.3, bias=0.4, noise=0.05)
BOUNDS = [(-2.0, 2.0), (-1.0, 3.0), (0.5, 2.5)]


def _problem():
    rs = np.random.RandomState(5)
    X = rs.uniform([b[0] for b in BOUNDS], [b[1] for b in BOUNDS], (N, D))
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] + 0.1 * rs.randn(N)
    return X, y[:, None]


def _close(a, b, tol=1e-9):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.max(np.abs(a - b)) <= tol * max(np.max(np.abs(b)), 1e-300), np.max(np.abs(a - b))


# ---- the restatement itself ------------------------------------------------------------------------------------------
def test_restatement_gradient_is_the_derivative_of_its_log_marginal():
    X, y = _problem()
    theta = np.concatenate([[HYP['var']], ELL, [HYP['bias'], HYP['noise']]])
    g = A.ArdPosterior(X, y, theta[0], theta[1:-2], theta[-2], theta[-1]).log_marginal_grad()
    eps = 1e-5
    for i in range(len(theta)):
        tp, tm = theta.copy(), theta.copy()
        tp[i] += eps
        tm[i] -= eps
        fd = (A.log_marginal(X, y, tp[0], tp[1:-2], tp[-2], tp[-1]) - A.log_marginal(X, y, tm[0], tm[1:-2], tm[-2], tm[-1])) / (2 * eps)
        assert abs(fd - g[i]) <= 1e-5 * (1 + abs(g[i])), (i, fd, g[i])


def test_restatement_with_equal_lengthscales_is_the_isotropic_oracle():
    X, y = _problem()
    iso = G.Posterior(X, y, HYP['var'], 1.7, HYP['bias'], HYP['noise'])
    ard = A.ArdPosterior(X, y, HYP['var'], np.full(D, 1.7), HYP['bias'], HYP['noise'])
    xs = np.random.RandomState(1).uniform(-2, 3, (9, D))
    assert abs(ard.log_marginal - iso.log_marginal) <= 1e-11 * abs(iso.log_marginal)
    gi, ga = iso.log_marginal_grad(), ard.log_marginal_grad()
    _close(np.array([ga[0], ga[1:-2].sum(), ga[-2], ga[-1]]), gi)
    for nl in (False, True):
        for a, b in zip(ard.predict(xs, noiseless=nl), iso.predict(xs, noiseless=nl)):
            _close(a, b)
    for a, b in zip(ard.predictive_gradients(xs), iso.predictive_gradients(xs)):
        _close(a, b)


# ---- the transform over a stand-in handle ----------------------------------------------------------------------------
class NumpyHandle:
    """GPHandle's wrapped methods in whatever coordinates the caller uses, one lengthscale, by gp_oracle.Posterior.  Like the
    device handle, no method goes through another one that a subclass overrides."""

    def __init__(self, d):
        self.d, self.n = d, 0
        self.calls = []

    def set_hyper(self, var, ls, bias, noise):
        self.h = (float(var), float(ls), float(bias), float(noise))
        self.post = None

    def set_data(self, X, y):
        self.U, self.y, self.n, self.post = np.array(X, float).reshape(-1, self.d), np.array(y, float).reshape(-1, 1), len(X), None
        self.calls.append('set_data')

    def append(self, X, y):
        self.U, self.y, self.post = np.vstack([self.U, X]), np.vstack([self.y, np.reshape(y, (-1, 1))]), None
        self.n = len(self.U)

    def factorize(self):
        self.post = G.Posterior(self.U, self.y, *self.h)
        return self.post.log_marginal

    def extend(self, X, y):
        NumpyHandle.append(self, X, y)
        return self.factorize()

    def get(self, which):
        return {2: self.post.alpha, 3: self.U, 4: self.y}[which].copy()

    def predict(self, x, noiseless=False):
        return self.post.predict(x, noiseless=noiseless)

    def predict_mean(self, x):
        return self.post.predict(x)[0]

    def predict_grad(self, x):
        return self.post.predict(x, noiseless=False) + self.post.predictive_gradients(x)

    def set_integration_points(self, points):
        self.P = np.array(points, float)

    def _k(self, a, b):
        return G.kern_K(a, b, *self.h[:3])

    def cross_cov(self, x):
        cov = self._k(self.P, x) - self._k(self.P, self.U) @ self.post.Kinv @ self._k(self.U, x)
        return cov, self.post.predict(x, noiseless=True)[1][:, 0]

    def maxvar(self, x, eps, prior_pdf, prior_grad_logpdf):
        mean, var = self.post.predict(x, noiseless=True)
        gm, gv = self.post.predictive_gradients(x)
        pdf = np.asarray(prior_pdf, float).reshape(-1)
        return (AO.maxvar_value(mean, var, self.h[3], eps, pdf),
                AO.maxvar_gradient(mean, var, gm, gv, self.h[3], eps, pdf, prior_grad_logpdf))

    def expintvar(self, x, eps, w_int, mean_int, var_int):
        cov, var_new = NumpyHandle.cross_cov(self, x)
        return AO.expintvar_loss(cov.T, var_new, self.h[3], eps, w_int, mean_int, var_int)

    def lcb(self, x, beta, with_grad=True):
        mu, v = self.post.predict(x, noiseless=True)
        gm, gv = self.post.predictive_gradients(x)
        return mu - np.sqrt(beta * v), (gm - 0.5 * gv * np.sqrt(beta / v)) if with_grad else None

    def nlml_grad_ard(self):
        p = self.post
        g = p.log_marginal_grad()
        E = p.dL_dK() * (p.K - p.bias)
        gd = np.array([np.sum(E * (self.U[:, c, None] - self.U[None, :, c]) ** 2) for c in range(self.d)]) / p.ls ** 3
        return p.log_marginal, g, gd

    def kernel_matrix(self, A_, B=None):
        return self._k(A_, A_ if B is None else B)

    # the two searches: a stand-in that records the box it was given and answers with points of that box
    def lcb_minimize(self, starts, bounds, beta, maxiter=1000):
        self.box = np.array(bounds, float)
        x = 0.5 * (np.asarray(starts) + self.box[:, 0])          # between each start and the lower corner
        x[0] = self.box[:, 1]                                    # ... and the upper corner itself
        return x, NumpyHandle.lcb(self, x, beta, with_grad=False)[0][:, 0], np.ones(len(x), dtype=np.int32), len(x)

    def minimize_mean(self, bounds, seed=0, **kw):
        self.box = np.array(bounds, float)
        x = self.box[:, 0] + np.random.RandomState(seed).uniform(size=self.d) * (self.box[:, 1] - self.box[:, 0])
        return x, float(NumpyHandle.predict_mean(self, x[None])[0, 0]), dict(generations=1), np.zeros((5, self.d)), np.zeros(5)


class ScaledNumpyHandle(DiagonalScaling, NumpyHandle):
    pass


@pytest.fixture(scope='module')
def pair():
    X, y = _problem()
    h = ScaledNumpyHandle(D)
    h.set_data(X[:30], y[:30])                      # uploaded at scale 1 ...
    h.set_hyper(HYP['var'], ELL, HYP['bias'], HYP['noise'])      # ... and again when the scale changes
    assert h.calls == ['set_data', 'set_data']
    h.append(X[30:35], y[30:35])
    h.factorize()
    lz = h.extend(X[35:], y[35:])
    ref = A.ArdPosterior(X, y, HYP['var'], ELL, HYP['bias'], HYP['noise'])
    assert h.n == N and abs(lz - ref.log_marginal) <= 1e-11 * abs(ref.log_marginal)
    return h, ref, X, y


def test_handle_holds_scaled_evidence_and_shows_the_original(pair):
    h, ref, X, y = pair
    _close(h.U, X / ELL, 1e-15)
    _close(h.get(3), X, 1e-15)
    _close(h.get(2), ref.alpha)
    assert h.h[1] == 1.0


def test_predictions_and_gradients_in_original_coordinates(pair):
    h, ref, X, y = pair
    xs = np.random.RandomState(2).uniform(-2, 3, (11, D))
    for nl in (False, True):
        for a, b in zip(h.predict(xs, noiseless=nl), ref.predict(xs, noiseless=nl)):
            _close(a, b)
    _close(h.predict_mean(xs), ref.predict(xs)[0])
    mu, var, dmu, dvar = h.predict_grad(xs)
    gm, gv = ref.predictive_gradients(xs)
    _close(mu, ref.predict(xs)[0])
    _close(var, ref.predict(xs)[1])
    _close(dmu, gm)
    _close(dvar, gv)
    val, grad = h.lcb(xs, 4.0)
    rv, rg = ref.lcb(xs, 4.0)
    _close(val, rv)
    _close(grad, rg)
    assert h.lcb(xs, 4.0, with_grad=False)[1] is None
    _close(h.kernel_matrix(xs), ref.kern(xs, xs))
    _close(h.kernel_matrix(xs, X[:7]), ref.kern(xs, X[:7]))


def test_maxvar_takes_the_prior_gradient_in_original_coordinates(pair):
    h, ref, X, y = pair
    xs = np.random.RandomState(3).uniform(-2, 3, (8, D))
    pdf = np.prod(np.exp(-0.5 * ((xs - 0.3) / 3.0) ** 2) / (3.0 * np.sqrt(2 * np.pi)), axis=1)
    glog = -(xs - 0.3) / 9.0
    eps = float(np.percentile(y, 20))
    val, grad = h.maxvar(xs, eps, pdf, glog)
    mean, var = ref.predict(xs, noiseless=True)
    gm, gv = ref.predictive_gradients(xs)
    _close(val, AO.maxvar_value(mean, var, ref.noise, eps, pdf))
    want = AO.maxvar_gradient(mean, var, gm, gv, ref.noise, eps, pdf, glog)
    _close(grad, want)
    # the prior's gradient matters: without it the answer is another one
    assert np.max(np.abs(h.maxvar(xs, eps, pdf, 0 * glog)[1] - want)) > 1e-3 * np.max(np.abs(want))


def test_integration_points_cross_covariance_and_expintvar(pair):
    h, ref, X, y = pair
    rs = np.random.RandomState(4)
    P, xs = rs.uniform(-2, 3, (6, D)), rs.uniform(-2, 3, (5, D))
    h.set_integration_points(P)
    cov, var = h.cross_cov(xs)
    _close(cov, ref.cross_cov(P, xs))
    _close(var, ref.predict(xs, noiseless=True)[1][:, 0])
    w, eps = rs.uniform(0.5, 1, 6), float(np.percentile(y, 20))
    mi, vi = ref.predict(P, noiseless=True)
    _close(h.expintvar(xs, eps, w, mi[:, 0], vi[:, 0]),
           AO.expintvar_loss(ref.cross_cov(P, xs).T, var, ref.noise, eps, w, mi[:, 0], vi[:, 0]))


def test_log_marginal_gradient_has_one_entry_per_lengthscale(pair):
    h, ref, X, y = pair
    lz, g = h.nlml_grad()
    assert g.shape == (3 + D,) and abs(lz - ref.log_marginal) <= 1e-11 * abs(ref.log_marginal)
    _close(g, ref.log_marginal_grad())


def test_both_minimisers_search_the_scaled_box_and_answer_in_the_original(pair):
    h, ref, X, y = pair
    lo, hi = np.array(BOUNDS).T
    starts = np.random.RandomState(6).uniform(lo, hi, (4, D))
    x, f, it, ne = h.lcb_minimize(starts, BOUNDS, 4.0)
    _close(h.box, np.array(BOUNDS) / ELL[:, None], 1e-15)
    assert np.all(x >= lo) and np.all(x <= hi) and np.array_equal(x[0], hi)
    _close(x[1:], 0.5 * (starts[1:] + lo), 1e-15)
    _close(f, ref.lcb(x, 4.0)[0][:, 0])
    xm, fm = h.minimize_mean(BOUNDS, seed=3)[:2]
    _close(h.box, np.array(BOUNDS) / ELL[:, None], 1e-15)
    assert np.all(xm >= lo) and np.all(xm <= hi)
    _close(xm, lo + np.random.RandomState(3).uniform(size=D) * (hi - lo), 1e-14)
    assert abs(fm - ref.predict(xm[None])[0][0, 0]) <= 1e-9 * abs(fm)
    with pytest.raises(ValueError):
        h.lcb_minimize(starts, BOUNDS[:2], 4.0)


def test_set_hyper_rejects_a_wrong_number_of_lengthscales(pair):
    h = ScaledNumpyHandle(D)
    with pytest.raises(ValueError):
        h.set_hyper(1.0, [1.0, 2.0], 1.0, 0.1)
    with pytest.raises(ValueError):
        h.set_hyper(1.0, [1.0, -2.0, 1.0], 1.0, 0.1)
    h.set_hyper(1.0, 2.5, 1.0, 0.1)
    assert np.array_equal(h.ell, np.full(D, 2.5))


# ---- argument handling of the model, before any device call ----------------------------------------------------------
def _model(ard, **kw):
    names = ['a', 'b', 'c']
    return HipGPRegression(names, bounds=dict(zip(names, BOUNDS)), ard=ard, **kw)


def test_ard_model_arguments_without_a_device():
    X, y = _problem()
    m = _model(True)
    assert m.ard and 'ard' not in m.gp_params
    h = m._default_hyper(y)
    assert h['ls'] == (1.0, 1.0, 1.0) and h['var'] == 1.0 and h['bias'] == 1.0       # all lengthscales start at 1
    assert _model(False)._default_hyper(y)['ls'] == 1.0 and not _model(False).ard
    with pytest.raises(ValueError):
        m.fix_hyperparameters(ls=[1.0, 2.0])
    with pytest.raises(ValueError):
        _model(False).fix_hyperparameters(ls=[1.0, 2.0, 3.0])
    with pytest.raises(RuntimeError):
        m.fix_hyperparameters(ls=[1.0, 2.0, 3.0])       # well-formed, but there is no GP yet
    assert m._ls_value(2.0) == (2.0, 2.0, 2.0) and m._ls_value([1, 2, 3]) == (1.0, 2.0, 3.0)
    for bad in (dict(kernel=object()), dict(mean_function=object())):
        with pytest.raises(NotImplementedError):
            _model(True, **bad)
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.ard and m.copy().ard


def test_search_vector_lengths_and_gpy_order():
    X, y = _problem()
    for ard, nls in ((False, 1), (True, D)):
        m = _model(ard)
        m._hyper = dict(m._default_hyper(y), ls=m._ls_value(ELL if ard else 1.7))
        m._priors = {k: (E, 1.0) for k, E in m._prior_expectations(y).items()}
        obj = H.MarginalObjective(m)
        assert len(obj.names) == 3 + nls and obj._last_grad.shape == (3 + nls,)
        theta = H.pack_hyper(m._hyper)
        assert theta.shape == (3 + nls,) and theta[0] == 1.0 and theta[-1] == m._hyper['noise']
        assert H.unpack_hyper(theta, ard) == m._hyper
        lp, dlp = obj._prior_terms(theta)
        assert dlp[-1] == 0.0 and np.all(dlp[:-1] != 0.0)           # every lengthscale carries the prior, the noise none
        from elfi_amd.gp import _GPShim
        m._X, m._Y, m._log_marginal = X, y, -1.0
        shim = _GPShim(m)
        assert np.array_equal(shim.param_array, theta)
        assert shim.kern.rbf.lengthscale.values.shape == (nls,) and 'rbf.lengthscale' in str(shim)
    assert H.pack_hyper(dict(var=2.0, ls=0.5, bias=3.0, noise=4.0)).tolist() == [2.0, 0.5, 3.0, 4.0]


def test_relevance_problem_of_the_device_test_on_the_restatement():
    """The problem tests/test_gp_ard_gpu.py gives the device search (y depends on x_0 alone): the restatement's own SCG
    search from the model's start ends with l_0 below l_1 and l_2 by a factor of at least 2 (measured: 9.3)."""
    from test_gp_ard_gpu import relevance_problem
    X, y, bounds = relevance_problem()
    pri = G.default_priors(bounds, y)
    h0 = G.initial_hyper(y)
    obj = A.MapObjective(X, y, pri)
    phi0 = H.logexp_inv(np.array([h0['var']] + [1.0] * X.shape[1] + [h0['bias'], h0['noise']]))
    phi, flog, _, _ = H.scg(obj.value, obj.gradient, phi0, maxiters=50)
    ell = H.logexp(phi)[1:-2]
    assert flog[-1] < flog[0] - 1.0 and min(ell[1], ell[2]) >= 2.0 * ell[0], ell
