"""Records tests/golden/toad.npz: ELFI's own toad example (elfi.examples.toad, imported through oracle/ref_shim.py) run with
fixed seeds -- per set the seed, the parameters, the shape, the positions X (simulation first: (batch, n_days, n_toads)) and the
summaries of lags 1, 2, 4, 8 side by side, (batch, 48).  The draws are not stored: tests/toad_ref.py's draws_from_state makes
them again from the seed, in the simulator's order; that the replay is what the simulator consumed is asserted here -- the
replayed positions must be the simulator's bit for bit.

  true        63 x 66 at the example's true parameters (1.7, 35, 0.6)
  prior       63 x 66, eight simulations with parameters drawn from the model's priors
  p0_one      p0 = 1: every toad returns every day, every column but the counts is inf
  p0_zero     p0 = 0: no toad ever returns (4 092 displacements to sort at lag 1, those at or above thd)
  gamma_zero  gamma = 0: no toad moves
  alpha_one   alpha = 1 (the Cauchy branch), alpha_two: alpha = 2 (Gaussian steps)
  small_585   10 x 65 -- 585 displacements at lag 1, below the 600 at which np.nanmedian changes path
  small_603   10 x 67 -- 603 at lag 1 (above), 536 at lag 2 (below)
  small_2     9 x 2 -- lag 8 leaves a single row of displacements

and SciPy's levy_stable.cdf at three points for alpha in {0.8, 1.5} (cdf_alpha, cdf_x, cdf_p), for the distribution test of
the device's sampler.

    python scripts/make_golden_toad.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

LAGS = (1, 2, 4, 8)
PARAM_SEED = 30291
#        name          seed   (n_toads, n_days)  batch  parameters (None: from the priors)
SETS = [('true',       30201, (66, 63), 1, (1.7, 35., 0.6)),
        ('prior',      30202, (66, 63), 8, None),
        ('p0_one',     30203, (66, 63), 1, (1.7, 35., 1.0)),
        ('p0_zero',    30204, (66, 63), 1, (1.7, 35., 0.0)),
        ('gamma_zero', 30205, (66, 63), 1, (1.7, 0., 0.6)),
        ('alpha_one',  30206, (66, 63), 1, (1.0, 35., 0.6)),
        ('alpha_two',  30207, (66, 63), 1, (2.0, 35., 0.6)),
        ('small_585',  30208, (65, 10), 3, None),
        ('small_603',  30209, (67, 10), 3, None),
        ('small_2',    30210, (2, 9), 3, None)]


def main():
    import scipy.stats as ss
    import ref_shim
    ref_shim.install()
    from elfi.examples import toad
    import toad_ref as R
    prs = np.random.RandomState(PARAM_SEED)
    out = {'sets': np.array([s[0] for s in SETS]), 'lags': np.array(LAGS)}
    for name, seed, (n_toads, n_days), batch, params in SETS:
        if params is None:
            params = [ss.uniform.rvs(lo, width, size=batch, random_state=prs) for lo, width in ((1, 1), (0, 100), (0, 0.9))]
        else:
            params = [np.full(batch, v) for v in params]
        args = params if batch > 1 else [v[0] for v in params]
        y = toad.toad(*args, n_toads=n_toads, n_days=n_days, batch_size=batch, random_state=np.random.RandomState(seed))
        S = np.hstack([toad.compute_summaries(y, lag) for lag in LAGS])
        X = np.ascontiguousarray(y.transpose(2, 0, 1))
        U, TH, W, Rr = R.draws_from_state(np.random.RandomState(seed), n_toads, n_days, batch)
        dx, _ = R.stable_step(params[0][:, None, None], params[1][:, None, None], TH, W)
        assert np.array_equal(R.simulate(*params, U, dx, Rr), X), 'the replayed draws are not what the simulator consumed: ' + name
        assert np.array_equal(R.all_summaries(X, LAGS), S), 'the statement of the summaries differs: ' + name
        out.update({name + '_seed': seed, name + '_shape': np.array([n_toads, n_days]), name + '_params': np.column_stack(params),
                    name + '_X': X, name + '_S': S})
        print(name, X.shape, 'inf summaries:', int(np.isinf(S).sum()))
    alphas, xs = np.array([0.8, 1.5]), np.array([-1.0, 0.5, 3.0])
    out.update(cdf_alpha=alphas, cdf_x=xs, cdf_p=np.array([[ss.levy_stable.cdf(x, a, 0.0) for x in xs] for a in alphas]))
    path = os.path.join(ROOT, 'tests', 'golden', 'toad.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
