"""Records tests/golden/series_models.npz: ELFI's own ARCH(1) and M/G/1 examples (elfi.examples.arch / mg1, imported
through oracle/ref_shim.py) run with fixed seeds -- parameters, the MT19937 draws the simulators consumed, the series
and the summaries.

  ARCH   64 simulations x 100 observations, n_lags = 5 (17 summaries)
  M/G/1  64 simulations x 50 observations, 10 equidistant quantiles and the log inter-departure times

The draws are recorded by replaying the seed in the simulators' order (ARCH: normal((B, n_obs + 1)) then normal(B);
M/G/1: standard_exponential((n_obs, B)) then random_sample((n_obs, B))); that the replay is what the simulators consumed
is asserted here -- tests/series_ref.py applied to the recorded draws must give the recorded series bit for bit.

    python scripts/make_golden_series.py
"""
import os
import sys
from itertools import combinations

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

ARCH_SEED, MG1_SEED, PARAM_SEED = 20261, 20262, 20263
B, ARCH_N_OBS, ARCH_LAGS, MG1_N_OBS, MG1_NQ = 64, 100, 5, 50, 10


def main():
    import ref_shim
    ref_shim.install()
    from elfi.examples import arch, mg1
    import series_ref as R
    rs = np.random.RandomState(PARAM_SEED)
    out = {}

    t1, t2 = rs.uniform(-1, 1, B), rs.uniform(0, 1, B)
    Y = arch.arch(t1, t2, n_obs=ARCH_N_OBS, batch_size=B, random_state=np.random.RandomState(ARCH_SEED))
    W = R.arch_noise_from_state(np.random.RandomState(ARCH_SEED), B, ARCH_N_OBS)
    assert np.array_equal(R.arch_series(t1, t2, W), Y), 'the replayed draws are not what the simulator consumed'
    lags = range(1, ARCH_LAGS + 1)
    S = np.column_stack([arch.sample_mean(Y), arch.sample_variance(Y)] + [arch.autocorr(Y, i) for i in lags] +
                        [arch.pairwise_autocorr(Y, i, j) for i, j in combinations(lags, 2)])
    out.update(arch_t1=t1, arch_t2=t2, arch_W=W, arch_Y=Y, arch_S=S, arch_n_lags=ARCH_LAGS)

    m1 = rs.uniform(0, 10, B)
    m2 = m1 + rs.uniform(0, 10, B)
    m3 = rs.uniform(0.01, 0.5, B)
    Yq = mg1.MG1(m1, m2, m3, n_obs=MG1_N_OBS, batch_size=B, random_state=np.random.RandomState(MG1_SEED))
    E, V = R.mg1_draws_from_state(np.random.RandomState(MG1_SEED), B, MG1_N_OBS)
    assert np.array_equal(R.mg1_series(m1, m2, m3, E, V), Yq), 'the replayed draws are not what the simulator consumed'
    q = np.linspace(0, 1, MG1_NQ)
    out.update(mg1_t1=m1, mg1_t2=m2, mg1_t3=m3, mg1_E=E, mg1_V=V, mg1_Y=Yq, mg1_logY=mg1.log_identity(Yq),
               mg1_q=q, mg1_Q=mg1.quantiles(Yq, q))

    path = os.path.join(ROOT, 'tests', 'golden', 'series_models.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
