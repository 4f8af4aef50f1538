"""Records tests/golden/daycare.npz: ELFI's own day-care example (elfi.examples.daycare, imported through
oracle/ref_shim.py) run on replayed draws -- its simulator takes any object with exponential / uniform as random_state, so it
is handed tests/daycare_ref.py: Replay over matrices E, U drawn from RandomState(seed).

The reference keeps every centre of a batch jumping until the slowest has passed time_end, so every centre is recorded as a
call of its own with batch_size = 1, n_dcc = 1: the only setting in which its result is not batch-dependent.

  true    16 centres at the example's true parameters (3.6, 0.6, 0.1), 53 x 33, 36 observed, time_end 2
  prior   16 centres with parameters from the model's priors, same shape, time_end 1
  small_* 4 centres each at n_ind 2 and 5, n_strains 1 and 3, parameters from the priors, time_end 8
  zero    2 centres at (0, 0, 0): one event of hazard 1e-9 per pair passes any time_end

Stored per set: seed, parameters, shape, time_end, n_events, the final observed states, the number of events each centre
needed, the four summaries by the example's own functions over the set's centres as ONE simulation, an observed array made
from them and the example's distance to it.  The draws are NOT stored: tests regenerate them with daycare_ref.golden_draws.

The recorder asserts two margins for every event of every run, read from the reference's own frame: no uniform within 1e-9
of an entry of its cumprobs, no event time within 1e-9 of time_end.  The device (and daycare_ref.simulate) sums factored
rows where the reference sums all n_ind n_strains hazards, so the two choices agree except within rounding (1e-13) of a
boundary; a seed that comes closer than the margin is refused here and another one picked.

    python scripts/make_golden_daycare.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

MARGIN = 1e-9
DEFAULT = (53, 33, 36)
SETS = {'true': dict(seed=30411, shape=DEFAULT, n_dcc=16, time_end=2., n_events=1024),
        'prior': dict(seed=30412, shape=DEFAULT, n_dcc=16, time_end=1., n_events=2048),
        'small_2_1': dict(seed=30413, shape=(2, 1, 1), n_dcc=4, time_end=8., n_events=1024),
        'small_5_3': dict(seed=30414, shape=(5, 3, 4), n_dcc=4, time_end=8., n_events=1024),
        'small_2_3': dict(seed=30415, shape=(2, 3, 2), n_dcc=4, time_end=8., n_events=1024),
        'small_5_1': dict(seed=30416, shape=(5, 1, 5), n_dcc=4, time_end=8., n_events=1024),
        'zero': dict(seed=30417, shape=DEFAULT, n_dcc=2, time_end=2., n_events=8)}


def parameters(name, cfg):
    n = cfg['n_dcc']
    if name == 'true':
        return np.tile([3.6, 0.6, 0.1], (n, 1))
    if name == 'zero':
        return np.zeros((n, 3))
    rs = np.random.RandomState(cfg['seed'] + 1000)
    return np.column_stack([rs.uniform(0, 11, n), rs.uniform(0, 2, n), rs.uniform(0, 1, n)])


def checked_replay(base):
    """Replay that reads the reference's cumprobs / time out of the calling frame and keeps the smallest margins seen."""
    class Checked(base):
        u_margin = t_margin = np.inf

        def exponential(self, scale):
            out = super().exponential(scale)
            loc = sys._getframe(1).f_locals
            self.t_margin = min(self.t_margin, float(np.min(np.abs(loc['time'] + out - loc['time_end']))))
            return out

        def uniform(self, size):
            out = super().uniform(size)
            cum = sys._getframe(1).f_locals['cumprobs']
            if cum.size:
                self.u_margin = min(self.u_margin, float(np.min(np.abs(out - cum))))
            return out
    return Checked


def main():
    import ref_shim
    ref_shim.install()
    from elfi.examples import daycare as dc
    import daycare_ref as R
    Replay = checked_replay(R.Replay)
    out = {}
    for name, cfg in SETS.items():
        n_ind, n_strains, n_obs = cfg['shape']
        n_dcc = cfg['n_dcc']
        E, U = R.golden_draws(cfg['seed'], n_dcc, cfg['n_events'])
        params = parameters(name, cfg)
        states, events = [], []
        for c in range(n_dcc):
            replay = Replay(E[None, c:c + 1], U[None, c:c + 1])
            y = dc.daycare(*params[c], n_dcc=1, n_ind=n_ind, n_strains=n_strains, n_obs=n_obs, time_end=cfg['time_end'],
                           batch_size=1, random_state=replay)
            assert replay.ke == replay.ku <= cfg['n_events'], 'the reference needed more events than were drawn'
            assert replay.u_margin > MARGIN and replay.t_margin > MARGIN, \
                '%s centre %d: margins %.3g (uniform), %.3g (time): pick another seed' % (name, c, replay.u_margin, replay.t_margin)
            states.append(y[0, 0])
            events.append(replay.ke)
        state = np.array(states)[None]                                # (1, n_dcc, n_obs, n_strains)
        S = np.stack([f(state)[0] for f in (dc.ss_shannon, dc.ss_strains, dc.ss_prevalence, dc.ss_prevalence_multi)]).astype(np.float64)
        obs = np.roll(S, 1, axis=1) * 0.5 + 0.125
        D = dc.distance(*[S[j][None, :] for j in range(4)], observed=[obs[j][None, :] for j in range(4)])
        out.update({name + '_seed': cfg['seed'], name + '_shape': np.array(cfg['shape']), name + '_time_end': cfg['time_end'],
                    name + '_n_events': cfg['n_events'], name + '_params': params, name + '_state': state[0],
                    name + '_events': np.array(events, dtype=np.int64), name + '_S': S, name + '_obs': obs, name + '_D': D})
        print(name, 'events', events, 'D', D)
    out['sets'] = np.array(list(SETS))
    path = os.path.join(ROOT, 'tests', 'golden', 'daycare.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
