"""No device: the NumPy restatement of the Matern kernels (tests/matern_ref.py) against a 40-digit evaluation and against
central differences of its own values, and the argument handling of HipGPRegression(kernel=...).

Bounds.  k and g are a handful of rounded operations on top of one exp whose argument t = sqrt(nu) r / l is itself rounded:
a relative error eps in t is an error t eps in exp(-t).  With eps = 2^-52 the values are held to (16 + 2 t) eps of their size
-- 16 eps for the operations, 2 t eps for the argument (for the RBF kernel t stands for r2 / 2l^2).  Central differences with
step h carry h^2 f''' / 6 truncation and eps |f| / h rounding: with h = 1e-5 on values of order 1-100 both stay below 1e-8, so
analytic derivatives are compared to 1e-6 of the largest component.
"""
import pickle

import numpy as np
import pytest

import gp_oracle as G
import matern_ref as M

EPS = 2.0 ** -52
R2 = np.concatenate([[0.0, 1e-300, 1e-18, 1e-9, 1e-3], np.logspace(-2, 3.6, 23)])      # up to 63 lengthscales at l = 1


@pytest.mark.parametrize('kind', M.KINDS)
@pytest.mark.parametrize('var,ls', [(1.0, 1.0), (2.7, 0.3), (0.4, 5.5)])
def test_k_and_g_against_mpmath(kind, var, ls):
    r2 = R2 * ls ** 2
    k, g = M.kg(kind, r2, var, ls)
    assert np.all(np.isfinite(k)) and np.all(np.isfinite(g)) and np.all(g <= 0)
    nu = {'rbf': None, 'matern32': 3.0, 'matern52': 5.0}[kind]
    for i, x in enumerate(r2):
        km, gm = M.kg_mp(kind, x, var, ls)
        t = 0.5 * x / ls ** 2 if nu is None else np.sqrt(nu * x) / ls
        bound = (16 + 2 * t) * EPS
        assert abs(float(km - k[i])) <= bound * abs(float(km)) + 1e-320, (kind, x, float(km), k[i])
        assert abs(float(gm - g[i])) <= bound * abs(float(gm)) + 1e-320, (kind, x, float(gm), g[i])
    # r = 0: k = s_f, g = -(1, 3, 5/3) / 2l^2 x s_f -- finite, no division by r anywhere
    k0, g0 = M.kg(kind, 0.0, var, ls)
    c = {'rbf': 1.0, 'matern32': 3.0, 'matern52': 5.0 / 3.0}[kind]
    assert k0 == var and abs(g0 + c * var / (2 * ls ** 2)) <= 4 * EPS * abs(g0)


@pytest.mark.parametrize('kind', M.KINDS)
def test_g_is_the_derivative_of_k(kind):
    r2 = np.logspace(-2, 2, 30)
    h = 1e-6 * r2
    fd = (M.kg(kind, r2 + h, 1.3, 0.8)[0] - M.kg(kind, r2 - h, 1.3, 0.8)[0]) / (2 * h)
    g = M.kg(kind, r2, 1.3, 0.8)[1]
    assert np.max(np.abs(fd - g)) <= 1e-6 * np.max(np.abs(g))


def _problem(n=40, d=3, seed=5):
    rs = np.random.RandomState(seed)
    X = rs.uniform(-2, 2, (n, d))
    y = (np.abs(X[:, 0] - 0.3) + 0.3 * X[:, 1] ** 2 + 1.0 + 0.05 * rs.randn(n))[:, None]
    return X, y


HYPER = dict(var=1.2, bias=0.5, noise=0.02)
ELL = np.array([0.8, 2.1, 1.3])


def test_rbf_kind_is_the_pinned_oracle():
    X, y = _problem()
    ref = G.Posterior(X, y, 1.2, 1.7, 0.5, 0.02)
    m = M.MaternPosterior(X, y, 'rbf', 1.2, 1.7, 0.5, 0.02)
    xs = np.random.RandomState(1).uniform(-2, 2, (6, 3))
    assert abs(m.log_marginal - ref.log_marginal) <= 1e-12 * abs(ref.log_marginal)
    for a, b in zip(m.predict(xs, True) + m.predictive_gradients(xs), ref.predict(xs, True) + ref.predictive_gradients(xs)):
        assert np.max(np.abs(a - b)) <= 1e-10 * np.max(np.abs(b))
    rg = ref.log_marginal_grad()
    assert np.max(np.abs(m.log_marginal_grad(isotropic=True) - rg)) <= 1e-9 * np.max(np.abs(rg))


@pytest.mark.parametrize('kind', ['matern32', 'matern52'])
def test_hyper_gradients_are_central_differences_of_the_log_marginal(kind):
    X, y = _problem()
    # per-dimension lengthscales: theta = (var, l_1, l_2, l_3, bias, noise)
    theta = np.concatenate([[HYPER['var']], ELL, [HYPER['bias'], HYPER['noise']]])

    def lz(t):
        return M.log_marginal(X, y, kind, t[0], t[1:-2], t[-2], t[-1])

    g = M.MaternPosterior(X, y, kind, theta[0], theta[1:-2], theta[-2], theta[-1]).log_marginal_grad()
    fd = np.empty_like(g)
    for i in range(len(theta)):
        h = 1e-5 * theta[i]
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h
        tm[i] -= h
        fd[i] = (lz(tp) - lz(tm)) / (2 * h)
    assert np.max(np.abs(fd - g)) <= 1e-6 * np.max(np.abs(g)), (fd, g)
    # one lengthscale: theta = (var, l, bias, noise)
    gi = M.MaternPosterior(X, y, kind, 1.2, 1.7, 0.5, 0.02).log_marginal_grad(isotropic=True)
    h = 1.7e-5
    fdl = (M.log_marginal(X, y, kind, 1.2, 1.7 + h, 0.5, 0.02) - M.log_marginal(X, y, kind, 1.2, 1.7 - h, 0.5, 0.02)) / (2 * h)
    assert gi.shape == (4,) and abs(fdl - gi[1]) <= 1e-6 * np.max(np.abs(gi))


@pytest.mark.parametrize('kind', ['matern32', 'matern52'])
def test_gradients_in_x_are_central_differences_also_at_an_evidence_row(kind):
    X, y = _problem()
    ref = M.MaternPosterior(X, y, kind, HYPER['var'], ELL, HYPER['bias'], HYPER['noise'])
    xs = np.random.RandomState(2).uniform(-2, 2, (5, 3))
    xs[0] = X[7]                                  # r = 0 exactly: 2 g (x - X) = 0 there, finite
    dmu, dvar = ref.predictive_gradients(xs)
    dl = ref.lcb(xs, 4.0)[1]
    assert np.all(np.isfinite(dmu)) and np.all(np.isfinite(dvar)) and np.all(ref.dk_dx(xs)[0, 7] == 0.0)
    h = 1e-5
    fm, fv, fl = np.empty_like(dmu), np.empty_like(dvar), np.empty_like(dl)
    for c in range(3):
        e = np.zeros(3)
        e[c] = h
        (mp_, vp), (mm, vm) = ref.predict(xs + e, True), ref.predict(xs - e, True)
        fm[:, c], fv[:, c] = ((mp_ - mm) / (2 * h))[:, 0], ((vp - vm) / (2 * h))[:, 0]
        fl[:, c] = ((ref.lcb(xs + e, 4.0)[0] - ref.lcb(xs - e, 4.0)[0]) / (2 * h))[:, 0]
    # matern32's second derivative jumps at r = 0: the symmetric difference is still second order, its constant larger
    for a, b in ((fm, dmu), (fv, dvar), (fl, dl)):
        assert np.max(np.abs(a - b)) <= 1e-6 * np.max(np.abs(b)), (a, b)


def test_gpy_form_of_r2_against_the_exact_one():
    """kern_gpy (GPy's (|a|^2 + |b|^2) - 2 a.b) against kern_mp on well-separated rows: the same kernel to rounding."""
    rs = np.random.RandomState(3)
    A, B = rs.uniform(-2, 2, (6, 3)), rs.uniform(-2, 2, (5, 3))
    for kind in M.KINDS:
        got, want = M.kern_gpy(kind, A, B, 1.2, 0.7, 0.5), M.kern_mp(kind, A, B, 1.2, 0.7, 0.5)
        assert np.max(np.abs(got - want)) <= 1e-13
        ref = M.MaternPosterior(A, np.zeros(6), kind, 1.2, 0.7, 0.5, 0.02, need_inv=False)
        assert np.max(np.abs(ref.kern(A, B) - want)) <= 64 * EPS * 1.7


# ---- argument handling of the model, with no device ------------------------------------------------------------------
NAMES = ['a', 'b']
BOUNDS = dict(a=(0.0, 1.0), b=(-1.0, 2.0))


def test_kernel_argument():
    from elfi_amd import HipGPRegression
    from elfi_amd.gp import KERNEL_KINDS, kernel_kind
    assert KERNEL_KINDS == dict(rbf=0, matern32=1, matern52=2)
    default = HipGPRegression(NAMES, bounds=BOUNDS)
    assert default.kernel == 'rbf' and kernel_kind(None) == 'rbf'
    for spelled, name in (('RBF', 'rbf'), ('rbf', 'rbf'), ('Matern32', 'matern32'), ('MATERN52', 'matern52')):
        m = HipGPRegression(NAMES, bounds=BOUNDS, kernel=spelled)
        assert m.kernel == name and 'kernel' not in m.gp_params
    rbf = HipGPRegression(NAMES, bounds=BOUNDS, kernel='RBF')
    assert rbf.kernel == default.kernel and rbf.gp_params == default.gp_params and rbf.ard == default.ard
    for bad in ('matern12', 'exponential', ''):
        with pytest.raises(ValueError):
            HipGPRegression(NAMES, bounds=BOUNDS, kernel=bad)
    for bad in (object(), 32, ['matern32'], lambda a, b: 0.0):
        with pytest.raises(NotImplementedError):
            HipGPRegression(NAMES, bounds=BOUNDS, kernel=bad)
    with pytest.raises(NotImplementedError):
        HipGPRegression(NAMES, bounds=BOUNDS, kernel='matern32', mean_function=object())


def test_kind_survives_pickle_and_copy_and_combines_with_ard():
    from elfi_amd import HipGPRegression
    m = HipGPRegression(NAMES, bounds=BOUNDS, kernel='matern52', ard=True, noise_var=0.1)
    assert m.kernel == 'matern52' and m.ard and m.gp_params == dict(noise_var=0.1)
    for k in (pickle.loads(pickle.dumps(m)), m.copy()):
        assert k.kernel == 'matern52' and k.ard and k.gp_params == dict(noise_var=0.1)
    # a state saved before the keyword existed has the RBF kernel
    st = m.__getstate__()
    del st['kernel']
    old = HipGPRegression.__new__(HipGPRegression)
    old.__setstate__(st)
    assert old.kernel == 'rbf'
    # the heuristics of the priors and the start values do not depend on the kind
    y = np.linspace(0.5, 3.0, 7)[:, None]
    a, b = HipGPRegression(NAMES, bounds=BOUNDS), HipGPRegression(NAMES, bounds=BOUNDS, kernel='matern32')
    assert a._prior_expectations(y) == b._prior_expectations(y) and a._default_hyper(y) == b._default_hyper(y)
