"""Records tests/golden/ricker.npz: ELFI's own Ricker example (elfi.examples.ricker, imported through oracle/ref_shim.py)
run with fixed seeds -- parameters drawn from the model's priors, the MT19937 normals the simulator consumed, the latent
stock, the Poisson counts, the three summaries and the chi_squared discrepancies.

  stochastic     64 simulations x 50 observations
  deterministic  16 simulations x 50 observations (series, Mean and the euclidean distance on it)

The normals and the stock are recorded by replaying the seed in the simulator's order (per step: randn(B), then
poisson(scale stock, B)); that the replay is what the simulator consumed is asserted here -- the replayed counts must be
the simulator's bit for bit.

    python scripts/make_golden_ricker.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

SIM_SEED, PARAM_SEED, OBS_SEED = 20271, 20272, 20273
B, BD, N_OBS = 64, 16, 50


def main():
    import scipy.stats as ss
    import ref_shim
    ref_shim.install()
    from elfi.examples import ricker
    import ricker_ref as R
    rs = np.random.RandomState(PARAM_SEED)
    out = {}

    t1 = ss.expon.rvs(np.e, 2, size=B, random_state=rs)
    t2 = ss.truncnorm.rvs(0, 5, size=B, random_state=rs)
    t3 = ss.uniform.rvs(0, 100, size=B, random_state=rs)
    Y = ricker.stochastic_ricker(t1, t2, t3, n_obs=N_OBS, batch_size=B, random_state=np.random.RandomState(SIM_SEED))
    Z, St, Yr = R.stochastic_ricker_from_state(np.random.RandomState(SIM_SEED), t1, t2, t3, n_obs=N_OBS, batch=B)
    assert np.array_equal(Yr, Y), 'the replayed draws are not what the simulator consumed'
    S = np.column_stack([np.mean(Y, axis=1), np.var(Y, axis=1), ricker.num_zeros(Y)]).astype(np.float64)
    y_obs = ricker.stochastic_ricker(3.8, 0.3, 10., n_obs=N_OBS, random_state=np.random.RandomState(OBS_SEED))
    obs = np.array([np.mean(y_obs, axis=1)[0], np.var(y_obs, axis=1)[0], ricker.num_zeros(y_obs)[0]], dtype=np.float64)
    D = ricker.chi_squared(*S.T, observed=tuple(np.array([o]) for o in obs))
    out.update(t1=t1, t2=t2, t3=t3, Z=Z, St=St, Y=Y, S=S, obs=obs, D=D)

    d1 = ss.expon.rvs(np.e, size=BD, random_state=rs)
    Yd = ricker.ricker(d1, n_obs=N_OBS, batch_size=BD)
    yd_obs = ricker.ricker(3.8, n_obs=N_OBS)
    from scipy.spatial.distance import cdist
    out.update(det_t1=d1, det_Y=Yd, det_mean=np.mean(Yd, axis=1), det_obs=np.mean(yd_obs, axis=1),
               det_D=cdist(np.mean(Yd, axis=1)[:, None], np.mean(yd_obs, axis=1)[:, None])[:, 0])

    path = os.path.join(ROOT, 'tests', 'golden', 'ricker.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
