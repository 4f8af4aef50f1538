"""Records tests/golden/lotka_volterra.npz: ELFI's own Lotka-Volterra example (elfi.examples.lotka_volterra, imported
through oracle/ref_shim.py) run on replayed draws -- its simulator takes any object with exponential / uniform / normal as
random_state, so it is handed tests/lv_ref.py: Replay over matrices E, U, Z drawn from RandomState(seed).

  true    16 simulations at the example's true parameters, time_end 5, observation noise sigma 10
  prior   16 simulations with parameters from the model's priors, time_end 30, no noise

Both with n_obs 16.  Stored: seeds, parameters, the observations (stock_out), the number of events each simulation needed to
pass time_end, the nine summaries by the example's own functions and the euclidean distances to the first row of 'true'.  The
draws are NOT stored: the test regenerates them from the seed with tests/lv_ref.py: golden_draws.

    python scripts/make_golden_lv.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

B, N_OBS = 16, 16
SETS = {'true': dict(seed=20281, time_end=5., n_events=4096, noisy=True),
        'prior': dict(seed=20282, time_end=30., n_events=4096, noisy=False)}


def prior_parameters(seed, batch=B):
    rs = np.random.RandomState(seed + 1000)
    r = np.exp(rs.uniform(-6., 2., (3, batch)))
    prey, pred = rs.normal(50, np.sqrt(50), batch), rs.normal(100, np.sqrt(100), batch)
    prey[0], pred[0] = 0.3, 0.7          # nothing alive: a constant series, NaN correlations
    return r[0], r[1], r[2], prey, pred


def reference_summaries(lv, Y):
    from functools import partial
    fns = [partial(lv.stock_mean, species=0), partial(lv.stock_mean, species=1), partial(lv.stock_log_variance, species=0),
           partial(lv.stock_log_variance, species=1), partial(lv.stock_autocorr, species=0, lag=1),
           partial(lv.stock_autocorr, species=1, lag=1), partial(lv.stock_autocorr, species=0, lag=2),
           partial(lv.stock_autocorr, species=1, lag=2), lv.stock_crosscorr]
    with np.errstate(all='ignore'):
        return np.column_stack([f(Y) for f in fns])


def event_counts(times, time_end):
    """The first event of each row at or past time_end."""
    return np.argmax(times >= time_end, axis=1).astype(np.int64)


def main():
    import ref_shim
    ref_shim.install()
    from elfi.examples import lotka_volterra as lv
    from scipy.spatial.distance import cdist
    import lv_ref as L
    out = {}
    for name, cfg in SETS.items():
        E, U, Z = L.golden_draws(cfg['seed'], B, cfg['n_events'], N_OBS)
        if name == 'true':
            params = [np.full(B, v) for v in (1.0, 0.005, 0.6, 50., 100.)]
        else:
            params = list(prior_parameters(cfg['seed']))
        sigma = np.full(B, 10.) if cfg['noisy'] else 0.
        replay = L.Replay(E, U, Z if cfg['noisy'] else None)
        Y, _, _, times = lv.lotka_volterra(*params, sigma=sigma, n_obs=N_OBS, time_end=cfg['time_end'], batch_size=B,
                                           random_state=replay, return_full=True)
        assert replay.ke <= cfg['n_events'], 'the reference needed more events than were drawn'
        S = reference_summaries(lv, Y)
        obs = out.setdefault('obs', S[0].copy())
        with np.errstate(all='ignore'):
            D = cdist(S, obs[None, :])[:, 0]
        out.update({name + '_seed': cfg['seed'], name + '_time_end': cfg['time_end'], name + '_n_events': cfg['n_events'],
                    name + '_params': np.array(params), name + '_Y': Y, name + '_events': event_counts(times, cfg['time_end']),
                    name + '_S': S, name + '_D': D})
        print(name, 'events', out[name + '_events'])
    path = os.path.join(ROOT, 'tests', 'golden', 'lotka_volterra.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
