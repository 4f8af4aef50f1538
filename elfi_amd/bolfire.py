"""elfi.BOLFIRE with the classifier, the surrogate, the acquisition and the posterior chains on the GPU: a drop-in for the
reference's class.

    bolfire = elfi_amd.HipBOLFIRE(model, n_training_data=500, feature_names=['S1', 'S2'], n_initial_evidence=20,
                                  bounds={'t1': (-2, 2), 't2': (-1, 1)}, seed=1)            # instead of elfi.BOLFIRE
    post = bolfire.fit(n_evidence=100)          # HipBOLFIREPosterior
    result = bolfire.sample(1000)               # the reference's BOLFIRESample

`HipBOLFIRE` IS the reference's `elfi.BOLFIRE` (elfi/methods/inference/bolfire.py:24-407) -- a subclass made from the
class of the ELFI the running program has imported (as `HipBOLFI` is), so the rounds, the marginal, the training data,
`predict_log_ratio`, the update rule of the surrogate and the result objects stay the reference's.  What changes:

  * `__init__` (bolfire.py:27-107): `target_model` defaults to `HipGPRegression`, `classifier` to
    `HipLogisticRegression` (elfi_amd/logratio.py: scaler, L1 logistic regression and log-odds of a round in one device
    call) and the acquisition to `HipLCBSC` with the arguments of bolfire.py:333-343 (prior, noise_var,
    exploration_rate, seed and the prior's log density as additive cost).  Objects the caller passes are used as they are.
  * `extract_result` (bolfire.py:119-124): a `HipBOLFIREPosterior` when the surrogate is a device model.
  * `sample` (bolfire.py:171-291): the reference farms one `mcmc.nuts` / `mcmc.metropolis` call per chain to the client,
    each of which calls `posterior.logpdf` / `gradient_logpdf` point by point.  Here the chains advance in lock-step
    (elfi_amd/chains.py) over `posterior.logpdf_and_gradient`: every round is ONE batched device prediction.  Arguments,
    checks, error texts, the choice and skipping of initial points (:224-244), the per-chain seeds
    `get_sub_seed(self.seed, ii)` and the returned `BOLFIRESample` are the reference's: chain ii equals what
    `mcmc.nuts(..., seed=get_sub_seed(self.seed, ii))` returns with the same posterior.

`HipBOLFIREPosterior` mirrors `BOLFIREPosterior` (elfi/methods/posteriors.py:259-390): logpdf = prior.logpdf - GP mean.
"""
import logging
import sys
from collections import OrderedDict

import numpy as np

from . import chains as _chains
from .gp import HipGPRegression
from .lcb_acquisition import HipLCBSC, draw_start_points
from .logratio import HipLogisticRegression
from .multistart import minimize_lockstep
from .posterior import prior_logpdf_and_gradient, sub_seed

logger = logging.getLogger(__name__)
_CLASSES = {}


class HipBOLFIREPosterior:
    """BOLFIREPosterior (posteriors.py:259-390) on a HipGPRegression: same constructor, properties and point-wise methods
    (logpdf, pdf, gradient_logpdf, gradient_pdf, compute_map_estimates; same output shapes), plus `logpdf_and_gradient`
    for a batch in one device call."""

    def __init__(self, parameter_names, model, prior, classifier_attributes, *args, **kwargs):
        if getattr(model, '_handle', None) is None:
            raise TypeError('HipBOLFIREPosterior needs a fitted elfi_amd.HipGPRegression (the device GP); got %r'
                            % (type(model).__name__,))
        self._parameter_names = parameter_names
        self._model = model
        self._prior = prior
        self._classifier_attributes = classifier_attributes

    @property
    def classifier_attributes(self):
        return self._classifier_attributes

    @property
    def surrogate_model_attributes(self):
        return {'parameters': self._model._gp.param_array.tolist(), 'X': self._model.X.tolist(),
                'Y': self._model.Y.tolist()}

    # ---- batched core ---------------------------------------------------------------------------------------------
    def logpdf_and_gradient(self, x):
        """Unnormalised log posterior (S,) and its gradient (S, d) at x (S, d): one device prediction for all rows
        (mean and its gradient), the prior's terms from one pass of the prior net."""
        d = self._model.input_dim
        x = np.ascontiguousarray(np.asanyarray(x, dtype=float).reshape((-1, d)))
        mean, _, grad_mean, _ = self._model._handle.predict_grad(x)
        plog, pgrad = prior_logpdf_and_gradient(self._prior, x)
        return plog - np.asarray(mean).reshape(-1), pgrad - np.asarray(grad_mean).reshape(x.shape)

    # ---- the reference's point-wise interface ---------------------------------------------------------------------
    def logpdf(self, x):
        return self._prior.logpdf(x).reshape(-1, 1) - self._model.predict_mean(x)

    def pdf(self, x):
        return np.exp(self.logpdf(x))

    def gradient_logpdf(self, x):
        return self._prior.gradient_logpdf(x).reshape(1, -1) - self._model.predictive_gradient_mean(x)

    def gradient_pdf(self, x):
        return np.exp(self.logpdf(x)) * self.gradient_logpdf(x)

    def _negative_logpdf(self, x):
        return -1 * self.logpdf(x)

    def _negative_gradient_logpdf(self, x):
        return -1 * self.gradient_logpdf(x)

    def compute_map_estimates(self, n_opt_inits=10, max_opt_iters=1000):
        """The maximum a posteriori estimate of each parameter (posteriors.py:366-390): start points drawn as the
        reference's minimize() draws them (prior.rvs clipped to the bounds), L-BFGS-B from every start in lock-step, each
        round one batched device prediction plus the prior's terms."""
        bounds = self._model.bounds
        starts = draw_start_points(bounds, n_opt_inits, self._prior, None)

        def negative(X):
            logp, grad = self.logpdf_and_gradient(X)
            return -logp, -grad

        res = minimize_lockstep(negative, starts, bounds, maxiter=max_opt_iters)
        loc = np.array(res['locs'][int(np.argmin(res['vals']))], dtype=float)
        for i in range(len(bounds)):
            loc[i] = np.clip(loc[i], *bounds[i])
        return OrderedDict([(param, loc[i]) for i, param in enumerate(self._model.parameter_names)])


def _reference_bolfire():
    mod = sys.modules.get('elfi.methods.inference.bolfire')
    if mod is None:
        raise ImportError("HipBOLFIRE subclasses the running program's elfi.BOLFIRE: `import elfi` first")
    return mod.BOLFIRE, mod


def hip_bolfire_class():
    """The subclass of the imported ELFI's BOLFIRE (made once per reference class)."""
    BOLFIRE, mod = _reference_bolfire()
    cls = _CLASSES.get(BOLFIRE)
    if cls is not None:
        return cls
    CostFunction, BOLFIRESample, mcmc, resolve_sigmas = mod.CostFunction, mod.BOLFIRESample, mod.mcmc, mod.resolve_sigmas

    class HipBOLFIRE(BOLFIRE):
        __doc__ = __doc__

        def __init__(self, model, n_training_data, feature_names=None, marginal=None, seed_marginal=None,
                     classifier=None, bounds=None, n_initial_evidence=0, acq_noise_var=0, exploration_rate=10,
                     update_interval=1, target_model=None, acquisition_method=None, **kwargs):
            if target_model is None:
                target_model = HipGPRegression(model.parameter_names, bounds=bounds)      # bolfire.py:327-328
            if classifier is None:
                classifier = HipLogisticRegression()
            super(HipBOLFIRE, self).__init__(model, n_training_data, feature_names=feature_names, marginal=marginal,
                                             seed_marginal=seed_marginal, classifier=classifier, bounds=bounds,
                                             n_initial_evidence=n_initial_evidence, acq_noise_var=acq_noise_var,
                                             exploration_rate=exploration_rate, update_interval=update_interval,
                                             target_model=target_model, acquisition_method=acquisition_method, **kwargs)

        # -- bolfire.py:333-346 -----------------------------------------------------------------------------------
        def _resolve_acquisition_method(self, acquisition_method):
            if acquisition_method is None and isinstance(self.target_model, HipGPRegression):
                cost = CostFunction(self.prior.logpdf, self.prior.gradient_logpdf, scale=-1)
                return HipLCBSC(self.target_model, prior=self.prior, noise_var=self.acq_noise_var,
                                exploration_rate=self.exploration_rate, seed=self.seed, additive_cost=cost)
            if isinstance(acquisition_method, HipLCBSC):
                return acquisition_method
            return super(HipBOLFIRE, self)._resolve_acquisition_method(acquisition_method)

        # -- bolfire.py:119-124 -----------------------------------------------------------------------------------
        def extract_result(self):
            if getattr(self.target_model, '_handle', None) is None:
                return super(HipBOLFIRE, self).extract_result()
            return HipBOLFIREPosterior(self.parameter_names, self.target_model, self.prior, self.classifier_attributes)

        # -- bolfire.py:171-291 -----------------------------------------------------------------------------------
        def sample(self, n_samples, warmup=None, n_chains=4, initials=None, algorithm='nuts', sigma_proposals=None,
                   n_evidence=None, *args, **kwargs):
            if not isinstance(self.target_model, HipGPRegression):
                return super(HipBOLFIRE, self).sample(n_samples, warmup, n_chains, initials, algorithm, sigma_proposals,
                                                      n_evidence, *args, **kwargs)
            if self.state['n_batches'] == 0:
                self.fit(n_evidence)
            if algorithm not in ['nuts', 'metropolis']:
                raise ValueError('The given algorithm is not supported.')
            if algorithm == 'metropolis':
                sigma_proposals = resolve_sigmas(self.parameter_names, sigma_proposals, self.target_model.bounds)
            posterior = self.extract_result()
            warmup = warmup or n_samples // 2
            if initials is not None:
                if np.asarray(initials).shape != (n_chains, self.target_model.input_dim):
                    raise ValueError('The shape of initials must be (n_chains, n_params).')
                pool = np.asarray(initials, dtype=float)
            else:
                pool = np.asarray(self.target_model.X[np.argsort(self.target_model.Y[:, 0])], dtype=float)
            # discard bad initialization points (:239-244): the candidates in one batched evaluation, not one call each
            usable = ~np.isinf(posterior.logpdf_and_gradient(pool)[0])
            picks, k = [], 0
            for _ in range(n_chains):
                while k < len(pool) and not usable[k]:
                    k += 1
                if k >= len(pool):
                    raise ValueError('BOLFIRE.sample: Cannot find enough acceptable initialization points!')
                picks.append(k)
                k += 1
            starts = pool[picks]
            seeds = [sub_seed(self.seed, ii) for ii in range(n_chains)]
            self.target_model.is_sampling = True
            try:
                if algorithm == 'nuts':
                    chains = _chains.nuts(n_samples, starts, posterior.logpdf_and_gradient, seeds=seeds, n_adapt=warmup,
                                          **kwargs)
                else:
                    chains = _chains.metropolis(n_samples, starts, posterior.logpdf_and_gradient, sigma_proposals,
                                                warmup=warmup, seeds=seeds, **kwargs)
            finally:
                self.target_model.is_sampling = False
            chains = np.asarray(chains)
            logger.info('%d chains of %d iterations acquired. Effective sample size and Rhat for each parameter:'
                        % (n_chains, n_samples))
            for ii, node in enumerate(self.parameter_names):
                logger.info('%s %s %s' % (node, mcmc.eff_sample_size(chains[:, :, ii]),
                                          mcmc.gelman_rubin_statistic(chains[:, :, ii])))
            nuts_only = ('target_prob', 'max_depth', 'info_freq', 'max_retry_inits', 'stepsize')
            rest = {k: v for k, v in kwargs.items() if k not in nuts_only}
            return BOLFIRESample(method_name='BOLFIRE', chains=chains, parameter_names=self.parameter_names,
                                 warmup=warmup, n_sim=self.state['n_sim'], seed=self.seed, *args, **rest)

    HipBOLFIRE.__name__ = 'HipBOLFIRE'
    HipBOLFIRE.__qualname__ = 'HipBOLFIRE'
    _CLASSES[BOLFIRE] = HipBOLFIRE
    return HipBOLFIRE


def HipBOLFIRE(*args, **kwargs):
    """elfi.BOLFIRE(model, n_training_data, feature_names=None, ...) with classifier, surrogate, acquisition and
    posterior chains on the GPU."""
    return hip_bolfire_class()(*args, **kwargs)
