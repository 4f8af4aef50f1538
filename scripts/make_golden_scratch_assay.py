"""Records tests/golden/scratch_assay.npz: ELFI's own scratch-assay example (elfi.examples.scratch_assay, imported through
oracle/ref_shim.py) run with fixed seeds -- per set the seeds (one RandomState per simulation), the parameters (pm, pp), the
initial grid, (obs_period, obs_interval, tau), the reference's cell_summaries (batch, n_obs + 1) and the bit-packed last frame
(batch, 32) uint32.  The draws are not stored: tests/assay_ref.py's from_random_state makes them again from the seed, in the
simulator's order; that the replay is what the simulator consumed is asserted here -- every frame must be the simulator's.

  true        the example's truth (0.25, 0.002) on its 27 x 36 grid with 100 cells in 10 rows, 288 iterations
  prior       four simulations with pm, pp drawn from the model's priors
  pm_one      pm = 1, pp = 0;   pp_one: pm = 0, pp = 1 (the grid fills, the skip branch runs)
  pm_nan      pm = NaN (selects nothing);   pm_big: pm = 1.5
  g3x5        a 3 x 5 grid with 4 cells in 2 rows;   g1x1: a full 1 x 1 grid;   g1x7: 1 x 7 with 3 cells
  g32x32      32 x 32 that starts with 1023 cells
  ragged      obs_period = 1, obs_interval = 1 / 5: obs_every = 4 does not divide n_iter = 24
  one_iter    n_iter = 1

`empty` records what the reference does on an all-empty 3 x 5 grid (empty_raises, and its summaries when it does not raise).

For the distribution test: the mean and standard deviation (ddof = 1) of assay_ref.moments over MOMENT_RUNS reference runs at
each of MOMENT_POINTS on the `true` set's grid (moment_points, moment_mean, moment_sd: about 70 s of CPU per point).

    python scripts/make_golden_scratch_assay.py
    python scripts/make_golden_scratch_assay.py --check-statement     # the distribution test on the NumPy statement alone
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

PARAM_SEED = 40491
DEFAULT_TIME = (12, 1 / 12, 1 / 24)
BIG = ('random', 27, 36, 100, 10)
#        name        seed   batch (pm, pp) (None: the priors)  grid                       (obs_period, obs_interval, tau)
SETS = [('true',     40401, 1, (0.25, 0.002), BIG, DEFAULT_TIME),
        ('prior',    40402, 4, None, BIG, DEFAULT_TIME),
        ('pm_one',   40403, 1, (1.0, 0.0), BIG, DEFAULT_TIME),
        ('pp_one',   40404, 1, (0.0, 1.0), BIG, DEFAULT_TIME),
        ('pm_nan',   40405, 1, (np.nan, 0.01), BIG, DEFAULT_TIME),
        ('pm_big',   40406, 1, (1.5, 0.002), BIG, DEFAULT_TIME),
        ('g3x5',     40407, 3, (0.5, 0.05), ('random', 3, 5, 4, 2), (1, 1 / 12, 1 / 24)),
        ('g1x1',     40408, 1, (0.5, 0.5), ('ones', 1, 1, 0), (1, 1 / 12, 1 / 24)),
        ('g1x7',     40409, 3, (0.7, 0.05), ('random', 1, 7, 3, 1), (1, 1 / 12, 1 / 24)),
        ('g32x32',   40410, 2, (0.8, 0.02), ('ones', 32, 32, 1), (1, 1 / 12, 1 / 24)),
        ('ragged',   40411, 2, (0.6, 0.05), ('random', 5, 9, 12, 3), (1, 1 / 5, 1 / 24)),
        ('one_iter', 40412, 2, (1.0, 0.5), ('random', 5, 9, 12, 3), (1 / 24, 1 / 24, 1 / 24))]
MOMENT_POINTS = [(0.25, 0.002), (0.6, 0.01)]
MOMENT_RUNS = 64
MOMENT_SEED = 40500


def reference():
    import ref_shim
    ref_shim.install()
    from elfi.examples import scratch_assay
    return scratch_assay


def grid_of(spec, seed):
    if spec[0] == 'random':
        return reference()._random_init(*spec[1:], random_state=np.random.RandomState(seed)).astype(np.uint8)
    g = np.ones(spec[1] * spec[2], dtype=np.uint8)
    g[len(g) - spec[3]:] = 0                            # ('ones', nrows, ncols, holes): the last cells are empty
    return g.reshape(spec[1], spec[2])


def moment_run(args):
    pm, pp, init, seed = args
    sa = reference()
    x = sa.cell_sim(pm, pp, init.astype(np.float64), random_state=np.random.RandomState(seed))
    return sa.cell_summaries(x[None])[0]


def main():
    sa = reference()
    import assay_ref as R
    prs = np.random.RandomState(PARAM_SEED)
    out = {'sets': np.array([s[0] for s in SETS])}
    for name, seed, batch, par, spec, time in SETS:
        init = grid_of(spec, seed + 5000)
        params = np.column_stack([prs.uniform(0, 1, batch), prs.uniform(0, 1, batch)]) if par is None else np.tile(par, (batch, 1))
        n_iter, obs_every, n_obs = R.shape(*time)
        seeds = seed * 10 + np.arange(batch)
        S, last = [], []
        for (pm, pp), sd in zip(params, seeds):
            x = sa.cell_sim(pm, pp, init.astype(np.float64), None, *time, random_state=np.random.RandomState(sd))
            s = sa.cell_summaries(x[None])
            Sr, fr, ev, _ = R.from_random_state(pm, pp, init, np.random.RandomState(sd), n_iter, obs_every)
            assert x.shape == init.shape + (n_obs + 1,) and np.array_equal(fr, x), \
                'the replayed draws are not what the simulator consumed: ' + name
            assert np.array_equal(Sr, s[0]) and np.array_equal(R.summaries(x[None]), s), 'the statement of the summaries differs: ' + name
            S.append(s[0])
            last.append(R.pack_frames(x[None, :, :, -1:])[0, 0])
            print(name, init.shape, 'cells %d -> %d' % (init.sum(), s[0, -1]), 'events', ev)
        out.update({name + '_seed': seeds, name + '_params': params, name + '_init': init, name + '_time': np.array(time),
                    name + '_S': np.array(S), name + '_last': np.array(last)})
    try:
        x = sa.cell_sim(0.5, 0.5, np.zeros((3, 5)), None, 1, 1 / 12, 1 / 24, random_state=np.random.RandomState(40413))
        out.update(empty_raises=False, empty_S=sa.cell_summaries(x[None]))
    except Exception as e:          # noqa: BLE001 -- whatever it raises is what is recorded
        print('all-empty grid:', repr(e))
        out.update(empty_raises=True, empty_S=np.zeros((1, 13)))
    init = out['true_init']
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        jobs = [(pm, pp, init, MOMENT_SEED + 1000 * j + i) for j, (pm, pp) in enumerate(MOMENT_POINTS) for i in range(MOMENT_RUNS)]
        rows = np.array(list(pool.map(moment_run, jobs))).reshape(len(MOMENT_POINTS), MOMENT_RUNS, -1)
    mom = np.array([R.moments(r) for r in rows])
    out.update(moment_points=np.array(MOMENT_POINTS), moment_runs=MOMENT_RUNS, moment_mean=mom.mean(axis=1),
               moment_sd=mom.std(axis=1, ddof=1))
    print('moments: mean', out['moment_mean'], 'sd', out['moment_sd'])
    path = os.path.join(ROOT, 'tests', 'golden', 'scratch_assay.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


def statement_run(args):
    import assay_ref as R
    pm, pp, init, stream, i = args
    return R.simulate_philox(pm, pp, init, *R.shape()[:2], 1, stream, i, 1)[0][0]


def check_statement():
    """The distribution test of tests/test_scratch_assay_gpu.py on the NumPy statement alone: 256 simulations per point of the
    drawn form at seed 1 against the recorded moments.  Prints the z values; they must stay under 4."""
    import assay_ref as R
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'scratch_assay.npz'))
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for j, (pm, pp) in enumerate(g['moment_points']):
            S = np.array(list(pool.map(statement_run, [(pm, pp, g['true_init'], j, i) for i in range(256)])))
            z = (R.moments(S).mean(axis=0) - g['moment_mean'][j]) / (g['moment_sd'][j] * np.sqrt(1 / 256 + 1 / 64))
            print('pm = %g, pp = %g: z = %s, largest |z| %.2f' % (pm, pp, np.round(z, 2), np.abs(z).max()))


if __name__ == '__main__':
    check_statement() if '--check-statement' in sys.argv else main()
