"""Records tests/golden/lorenz.npz: ELFI's own stochastic Lorenz-96 example (elfi.examples.lorenz, imported through
oracle/ref_shim.py) run with fixed seeds -- parameters, seeds, series and the six summaries.

  default  2 simulations x 160 rows x 40 variables from the example's own initial state
  small    16 simulations x 20 rows x 8 variables from an explicit (16, 8) initial state
  y0       the example's default initial state, read as row 0 of forecast_lorenz(0, 0, n_timestep=1, batch_size=1)
  e2e      elfi.examples.lorenz.get_model(seed_obs=4) under elfi.Rejection(batch_size=5000, seed=2).sample(200, n_sim=20000):
           the observed summaries, the posterior means of theta1 and theta2 and, as the margin a different random
           realisation of the same run is held to, four standard errors of a 200-sample mean (4 sd / sqrt(200))

Seeds are stored, not draws: the simulator consumes one normal(0, 1, (B, K)) per step, which the tests replay with
tests/lorenz_ref.py:lorenz_noise_from_state.  That the replay is what the simulator consumed is asserted here -- the NumPy
statement tests/lorenz_ref.py on the replayed draws must give the recorded series bit for bit.

    python scripts/make_golden_lorenz.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

DEFAULT_SEED, SMALL_SEED, PARAM_SEED = 20271, 20272, 20273
SMALL_B, SMALL_T, SMALL_K = 16, 20, 8
E2E = dict(seed_obs=4, batch_size=5000, seed=2, n_samples=200, n_sim=20000)


class _Given(np.ndarray):
    """forecast_lorenz tests `if not initial_state`, which a plain array of several elements refuses to answer."""

    def __bool__(self):
        return True


def _summaries(lorenz, X):
    return np.column_stack([lorenz.mean(X), lorenz.var(X), lorenz.autocov(X), lorenz.cov(X), lorenz.xcov(X, True),
                            lorenz.xcov(X, False)])


def main():
    import ref_shim
    elfi = ref_shim.install()
    from elfi.examples import lorenz
    import lorenz_ref as R
    rs = np.random.RandomState(PARAM_SEED)
    out = {}

    y0 = np.array(lorenz.forecast_lorenz(0, 0, n_timestep=1, batch_size=1)[0, 0])
    assert y0.shape == (40,)
    out['y0_default'] = y0

    t1, t2 = rs.uniform(0.5, 3.5, 2), rs.uniform(0, 0.3, 2)
    X = lorenz.forecast_lorenz(t1, t2, batch_size=2, random_state=np.random.RandomState(DEFAULT_SEED))
    E = R.lorenz_noise_from_state(np.random.RandomState(DEFAULT_SEED), 2, 160, 40)
    c, h = R.lorenz_constants(0.984, 160, 4)
    assert np.array_equal(R.lorenz_series(t1, t2, E, y0, 10., c, 0.984, h), X), 'the replayed draws are not what the simulator consumed'
    S = _summaries(lorenz, X)
    assert np.array_equal(R.lorenz_summaries(X), S) and np.array_equal(R.lorenz_summaries_explicit(X), S)
    out.update(default_seed=DEFAULT_SEED, default_t1=t1, default_t2=t2, default_X=X, default_S=S)

    s1, s2 = rs.uniform(0.5, 3.5, SMALL_B), rs.uniform(0, 0.3, SMALL_B)
    sy0 = 3.0 * rs.randn(SMALL_B, SMALL_K)
    Xs = np.asarray(lorenz.forecast_lorenz(s1, s2, n_obs=SMALL_K, n_timestep=SMALL_T, batch_size=SMALL_B,
                                           initial_state=sy0.view(_Given), random_state=np.random.RandomState(SMALL_SEED)))
    Es = R.lorenz_noise_from_state(np.random.RandomState(SMALL_SEED), SMALL_B, SMALL_T, SMALL_K)
    cs, hs = R.lorenz_constants(0.984, SMALL_T, 4)
    assert np.array_equal(R.lorenz_series(s1, s2, Es, sy0, 10., cs, 0.984, hs), Xs), 'the replayed draws are not what the simulator consumed'
    Ss = _summaries(lorenz, Xs)
    assert np.array_equal(R.lorenz_summaries(Xs), Ss) and np.array_equal(R.lorenz_summaries_explicit(Xs), Ss)
    out.update(small_seed=SMALL_SEED, small_t1=s1, small_t2=s2, small_y0=sy0, small_X=Xs, small_S=Ss)

    m = lorenz.get_model(seed_obs=E2E['seed_obs'])
    res = elfi.Rejection(m['d'], batch_size=E2E['batch_size'], seed=E2E['seed']).sample(E2E['n_samples'], n_sim=E2E['n_sim'])
    th = np.column_stack([res.samples['theta1'], res.samples['theta2']])
    out.update(e2e_settings=np.array([E2E[k] for k in ('seed_obs', 'batch_size', 'seed', 'n_samples', 'n_sim')]),
               e2e_obs=_summaries(lorenz, np.asarray(m['Lorenz'].observed))[0],
               e2e_centre=th.mean(axis=0), e2e_margin=4 * th.std(axis=0, ddof=1) / np.sqrt(len(th)),
               e2e_threshold=float(res.threshold))
    print('e2e centre', out['e2e_centre'], 'margin', out['e2e_margin'], 'threshold', out['e2e_threshold'])

    path = os.path.join(ROOT, 'tests', 'golden', 'lorenz.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
