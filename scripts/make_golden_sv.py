"""Records tests/golden/sv.npz: ELFI's own alpha-stable stochastic-volatility example
(elfi.examples.stochastic_volatility_model, imported through oracle/ref_shim.py) run with fixed seeds -- per set the seed, the
parameters (alpha, beta, kappa, eta, mu, phi, sigma, x_0; x_0 NaN where the example's stationary start is used), the returns y
(batch, n_obs) and the reference's kurt and skew, (batch, 2).  The draws are not stored: tests/sv_ref.py's draws_from_state
makes them again from the seed, in the simulator's order; that the replay is what the simulator consumed is asserted here --
the replayed returns must be the simulator's bit for bit.

  true        n_obs = 50 at the example's true parameters (1.2, 0.5)
  prior       eight simulations with alpha, beta drawn from the model's priors
  alpha_one   alpha = 1 with beta = 0.5 (alpha1func and both location shifts), alpha_two: alpha = 2
  beta_zero   beta = 0 (the symmetric expression), beta_plus, beta_minus: beta = +-1
  kappa_zero  kappa = 0: every return is zero and both summaries are 0 / 0
  x0          the initial log-volatility x_0 given
  n_1, n_2, n_65   n_obs in {1, 2, 65}

and SciPy's levy_stable.cdf in the S0 parameterisation at three points for (alpha, beta) in {(0.8, 0.5), (1.5, -0.7)}
(cdf_params, cdf_x, cdf_p), for the distribution test of the device's sampler.

    python scripts/make_golden_sv.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

PARAM_SEED = 30391
FIXED = dict(kappa=1., eta=0., mu=0., phi=0.95, sigma=0.2)
#        name          seed   n_obs batch (alpha, beta) (None: from the priors)   other parameters
SETS = [('true',       30301, 50, 1, (1.2, 0.5), {}),
        ('prior',      30302, 50, 8, None, {}),
        ('alpha_one',  30303, 50, 1, (1.0, 0.5), {}),
        ('alpha_two',  30304, 50, 1, (2.0, 0.5), {}),
        ('beta_zero',  30305, 50, 1, (1.2, 0.0), {}),
        ('beta_plus',  30306, 50, 1, (1.2, 1.0), {}),
        ('beta_minus', 30307, 50, 1, (1.2, -1.0), {}),
        ('kappa_zero', 30308, 50, 1, (1.2, 0.5), dict(kappa=0.)),
        ('x0',         30309, 50, 3, None, dict(x_0=0.7, eta=0.1, mu=-0.3)),
        ('n_1',        30310, 1, 3, None, {}),
        ('n_2',        30311, 2, 3, None, {}),
        ('n_65',       30312, 65, 3, None, {})]
ORDER = ('alpha', 'beta', 'kappa', 'eta', 'mu', 'phi', 'sigma', 'x_0')


def main():
    import scipy.stats as ss
    import ref_shim
    ref_shim.install()
    from elfi.examples import stochastic_volatility_model as svm
    import sv_ref as R
    prs = np.random.RandomState(PARAM_SEED)
    out = {'sets': np.array([s[0] for s in SETS]), 'order': np.array(ORDER)}
    for name, seed, n_obs, batch, ab, other in SETS:
        if ab is None:
            alpha = ss.uniform.rvs(0.5, 1.5, size=batch, random_state=prs)
            beta = ss.uniform.rvs(-1, 2, size=batch, random_state=prs)
        else:
            alpha, beta = np.full(batch, ab[0]), np.full(batch, ab[1])
        kw = dict(FIXED, **other)
        x_0 = kw.pop('x_0', None)
        args = (alpha, beta) if batch > 1 else (alpha[0], beta[0])
        y = svm.alpha_stochastic_volatility_model(*args, **kw, n_obs=n_obs, x_0=x_0, batch_size=batch,
                                                  random_state=np.random.RandomState(seed))
        with np.errstate(all='ignore'):
            S = np.column_stack([np.reshape(svm.kurt(y), -1), np.reshape(svm.skew(y), -1)])
        Z, TH, W = R.draws_from_state(np.random.RandomState(seed), n_obs, batch)
        params = np.column_stack([alpha, beta] + [np.full(batch, kw[k]) for k in ORDER[2:7]] +
                                 [np.full(batch, np.nan if x_0 is None else x_0)])
        yr = R.simulate(*params[:, :7].T, Z, TH, W, x_0=None if x_0 is None else params[:, 7])[3]
        assert y.shape == (batch, n_obs) and np.array_equal(yr, y, equal_nan=True), \
            'the replayed draws are not what the simulator consumed: ' + name
        assert np.array_equal(R.summaries(y), S, equal_nan=True), 'the statement of the summaries differs: ' + name
        out.update({name + '_seed': seed, name + '_params': params, name + '_y': y, name + '_S': S})
        print(name, y.shape, 'NaN summaries:', int(np.isnan(S).sum()))
    pairs, xs = np.array([[0.8, 0.5], [1.5, -0.7]]), np.array([-1.0, 0.5, 3.0])
    ss.levy_stable.parameterization = 'S0'
    try:
        cdf = np.array([[ss.levy_stable.cdf(x, a, b) for x in xs] for a, b in pairs])
    finally:
        ss.levy_stable.parameterization = 'S1'
    out.update(cdf_params=pairs, cdf_x=xs, cdf_p=cdf)
    path = os.path.join(ROOT, 'tests', 'golden', 'sv.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
