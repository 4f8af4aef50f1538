"""GPU: `elfi_amd.HipBOLFIRE` and `elfi_amd.HipBOLFIREPosterior` -- the reference's `elfi.BOLFIRE`
(elfi/methods/inference/bolfire.py) with classifier, surrogate, acquisition and posterior chains on the device -- next to
the reference's own classes (oracle/ref_shim.py) on the reference's MA2 model.

  * the posterior object against the reference's `BOLFIREPosterior` on the same fitted `HipGPRegression`: rel 1e-8, the
    project's stated GP tolerance;
  * ten rounds of `HipBOLFIRE` against the reference's `elfi.BOLFIRE` with the same arguments, the reference's loop driving
    a `HipGPRegression`, a `HipLCBSC` built as bolfire.py:333-343 builds its `LCBSC`, and the reference's own
    `LogisticRegression` with the tight liblinear config of tests/golden/logratio.npz: the prior-phase evidence (same
    parameter points, same simulations, so only the classifiers differ) within the classifier bound of
    tests/test_logratio_gpu.py for m = 2 summaries (prior draws far from the observed data give nearly separable classes,
    log ratios near -7, where the reference's own error against 40-digit arithmetic was measured at 5e-12 to 4e-11 over
    eight states of NumPy's generator: the fixture holds such a case with m = 2, tests/logratio_ref.py), all ten evidence points and values to 1e-6, the project's stated
    end-to-end tolerance for first acquisitions at identical seeds;
  * `sample`: the reference's `BOLFIRESample`, chain ii equal to the reference's `mcmc.metropolis` / `mcmc.nuts` run with
    the point-wise methods of the same posterior and `get_sub_seed(seed, ii)`; the reference's error texts.
"""
import os
import sys

import numpy as np
import pytest

from test_logratio import bound_for

ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle')
sys.path.insert(0, ORACLE)
import ref_shim  # noqa: E402
from conftest import GOLDEN  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref_shim.available(), reason='no reference package (run oracle/make_ref.sh)')]

BOUNDS = {'t1': (-2, 2), 't2': (-1, 1)}
NAMES = ['t1', 't2']
FEATS = ['S1', 'S2']
TIGHT = {'penalty': 'l1', 'solver': 'liblinear', 'tol': 1e-12, 'max_iter': 100000}
ARGS = dict(n_training_data=50, feature_names=FEATS, bounds=BOUNDS, n_initial_evidence=6, update_interval=100, seed=1,
            seed_marginal=2)


@pytest.fixture(scope='module')
def elfi():
    e = ref_shim.install()
    import elfi.clients.native as native
    native.set_as_default()
    return e


def _model(elfi):
    from elfi.examples import ma2
    return ma2.get_model(seed_obs=4)


@pytest.fixture(scope='module')
def fitted(hip_ctx, elfi):
    """HipBOLFIRE after fit(10), with the evidence it gathered."""
    import elfi_amd
    hip = elfi_amd.HipBOLFIRE(_model(elfi), **ARGS)
    post = hip.fit(10, bar=False)
    return hip, post


# 5 ---------------------------------------------------------------------------------------------------------------
def test_posterior_next_to_the_reference_posterior(hip_ctx, elfi):
    import elfi_amd
    from elfi.methods.posteriors import BOLFIREPosterior
    from elfi.model.extensions import ModelPrior
    rs = np.random.RandomState(5)
    X = rs.uniform([-1.8, -0.9], [1.8, 0.9], (30, 2))
    Y = ((X[:, 0] - 0.6) ** 2 + 2 * (X[:, 1] - 0.2) ** 2 + 0.05 * rs.randn(30)).reshape(-1, 1)
    gp = elfi_amd.HipGPRegression(NAMES, bounds=BOUNDS)
    gp.update(X, Y, optimize=True)
    prior = ModelPrior(_model(elfi), parameter_names=NAMES)
    attrs = [{'parameters': {'coef_': [[0.0, 1.0]], 'intercept_': [0.5], 'n_iter': [3]}}]
    ref, hip = BOLFIREPosterior(NAMES, gp, prior, attrs), elfi_amd.HipBOLFIREPosterior(NAMES, gp, prior, attrs)
    assert hip.classifier_attributes is attrs and hip.surrogate_model_attributes == ref.surrogate_model_attributes
    pts = np.vstack([rs.uniform([-0.9, -0.4], [0.9, 0.9], (11, 2)),
                     [[2.5, 0.3], [0.2, 1.4], [-2.2, 1.2], [-0.3, -1.6]],      # outside the bounds
                     [[1.8, -0.9]]])                                           # inside the bounds, outside the prior's support
    assert len(pts) == 16 and np.isneginf(prior.logpdf(pts[-1:]))[0] and np.isfinite(prior.logpdf(pts[:11])).all()
    logp, grad = hip.logpdf_and_gradient(pts)
    assert logp.shape == (16,) and grad.shape == (16, 2)
    for i, x in enumerate(pts):
        a, b = ref.logpdf(x), hip.logpdf(x)
        assert a.shape == b.shape == (1, 1)
        ga, gb = ref.gradient_logpdf(x), hip.gradient_logpdf(x)
        assert ga.shape == gb.shape == (1, 2)
        assert ref.pdf(x).shape == hip.pdf(x).shape and ref.gradient_pdf(x).shape == hip.gradient_pdf(x).shape
        if np.isneginf(a[0, 0]):
            assert np.isneginf(b[0, 0]) and np.isneginf(logp[i]) and hip.pdf(x)[0, 0] == 0.0
        else:
            np.testing.assert_allclose(b, a, rtol=1e-8)
            np.testing.assert_allclose(hip.pdf(x), ref.pdf(x), rtol=1e-8)
            np.testing.assert_allclose(logp[i], a[0, 0], rtol=1e-8)
            np.testing.assert_allclose(hip.gradient_pdf(x), ref.gradient_pdf(x), rtol=1e-8, atol=1e-300)
        np.testing.assert_allclose(gb, ga, rtol=1e-8, atol=1e-12)
        np.testing.assert_allclose(grad[i], ga[0], rtol=1e-8, atol=1e-12)
    assert np.isneginf(logp[-1]) and np.isfinite(logp[:11]).all()
    # the MAP estimate: the reference's type and keys, inside the bounds, no worse than any of the points above
    np.random.seed(3)
    est = hip.compute_map_estimates(n_opt_inits=6)
    assert list(est) == NAMES
    at = np.array([est[k] for k in NAMES])
    assert np.all(at >= [-2, -1]) and np.all(at <= [2, 1])
    assert hip.logpdf(at)[0, 0] >= logp[:11].max() - 1e-9


# 6 ---------------------------------------------------------------------------------------------------------------
def test_ten_rounds_next_to_the_reference_bolfire(hip_ctx, elfi, fitted):
    import elfi_amd
    from elfi.methods.bo.utils import CostFunction
    from elfi.methods.classifier import LogisticRegression
    from elfi.model.extensions import ModelPrior
    gold = np.load(os.path.join(GOLDEN, 'logratio.npz'))
    hip, post = fitted
    assert isinstance(hip, elfi.BOLFIRE) and isinstance(post, elfi_amd.HipBOLFIREPosterior)
    assert hip.n_evidence == 10 and len(hip.classifier_attributes) == 10
    assert set(hip.classifier_attributes[0]['parameters']) == {'coef_', 'intercept_', 'n_iter'}

    model = _model(elfi)
    gp = elfi_amd.HipGPRegression(model.parameter_names, bounds=BOUNDS)
    ref = elfi.BOLFIRE(model, classifier=LogisticRegression(config=dict(TIGHT)), target_model=gp, **ARGS)
    prior = ModelPrior(model, parameter_names=ref.parameter_names)
    cost = CostFunction(prior.logpdf, prior.gradient_logpdf, scale=-1)
    # (the reference's resolver takes its own acquisition classes only: the device one is put in place after it)
    ref.acquisition_method = elfi_amd.HipLCBSC(gp, prior=prior, noise_var=0, exploration_rate=10, seed=1,
                                               additive_cost=cost)
    np.random.seed(0)       # liblinear draws its coordinate order from NumPy's global generator: the same run every time
    ref.fit(10, bar=False)
    assert np.array_equal(ref.marginal, hip.marginal)
    Xh, Yh, Xr, Yr = hip.target_model.X, hip.target_model.Y, gp.X, gp.Y
    assert Xh.shape == Xr.shape == (10, 2) and Yh.shape == Yr.shape == (10, 1)
    b = bound_for(gold, 2, truth=Yr[:6])
    print('prior phase: |device - reference| %s, bound %.2e' % (np.abs(Yh[:6] - Yr[:6]).ravel(), b))
    print('all rounds: points %.2e, values %.2e' % (np.abs(Xh - Xr).max(), np.abs(Yh - Yr).max()))
    assert np.array_equal(Xh[:6], Xr[:6])
    assert np.all(np.abs(Yh[:6] - Yr[:6]) <= b)
    np.testing.assert_allclose(Xh, Xr, rtol=0, atol=1e-6)
    np.testing.assert_allclose(Yh, Yr, rtol=0, atol=1e-6)


# 7 ---------------------------------------------------------------------------------------------------------------
def test_sample_next_to_the_reference_chains(hip_ctx, elfi, fitted):
    import elfi.methods.mcmc as mcmc
    from elfi.loader import get_sub_seed
    from elfi.methods.results import BOLFIRESample
    hip, post = fitted
    res = hip.sample(40, n_chains=2, algorithm='metropolis')
    assert isinstance(res, BOLFIRESample) and res.chains.shape == (2, 40, 2)
    assert res.method_name == 'BOLFIRE' and res.n_chains == 2 and res.parameter_names == NAMES
    assert res.n_samples == 2 * 20 and res.n_sim == hip.state['n_sim'] and res.seed == 1
    post = hip.extract_result()
    pool = np.asarray(hip.target_model.X[np.argsort(hip.target_model.Y[:, 0])])
    usable = [x for x in pool if not np.isinf(post.logpdf(x))]
    sig = np.array([0.4, 0.2])                          # resolve_sigmas: a tenth of the bounds' lengths
    for ii in range(2):
        want = mcmc.metropolis(40, usable[ii], post.logpdf, sig, 20, seed=get_sub_seed(1, ii))
        np.testing.assert_allclose(res.chains[ii], want, rtol=1e-6, atol=1e-9)
    nuts = hip.sample(12, warmup=6, n_chains=2)
    assert nuts.chains.shape == (2, 12, 2)
    for ii in range(2):
        want = mcmc.nuts(12, usable[ii], post.logpdf, post.gradient_logpdf, n_adapt=6, seed=get_sub_seed(1, ii))
        np.testing.assert_allclose(nuts.chains[ii, :4], want[:4], rtol=1e-6, atol=1e-7)
    given = hip.sample(10, n_chains=2, initials=np.array([[0.5, 0.1], [0.4, 0.3]]), algorithm='metropolis')
    assert given.chains.shape == (2, 10, 2)
    with pytest.raises(ValueError, match=r'The shape of initials must be \(n_chains, n_params\)\.'):
        hip.sample(10, n_chains=2, initials=np.zeros((3, 2)))
    with pytest.raises(ValueError, match='The given algorithm is not supported.'):
        hip.sample(10, algorithm='gibbs')
