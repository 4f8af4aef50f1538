"""Records tests/golden/bdm.npz: the reference's birth-death-mutation simulator (elfi/examples/cpp/bdm.cpp) and its AR(1)
example (elfi.examples.ar1, imported through oracle/ref_shim.py) run with fixed seeds.

The simulator is compiled with the host C++ compiler into a temporary directory outside the tree and run on input files, as
elfi/examples/bdm.py runs it; nothing compiled or copied from the reference is kept.  Per set of 16 rows: the parameters as the
binary parsed them (4 decimals), N, mode, seed, the clusters the binary printed, and the number of events each row made
according to tests/bdm_ref.py's replay of the binary's generator -- whose clusters must be the binary's, asserted here.  The
uniforms are not stored: bdm_ref.replay makes them again from the seed.

  truth      the example's truth (0.2, 0, 0.198), N = 20, mode 1
  prior      alpha over the prior's range [0.005, 2.005], the example's other values
  slow       alpha from 0.005 to 0.012: hundreds of events per row, most of them mutations of singletons
  deaths     delta > alpha: several rows go extinct, and mutations open slots that deaths freed
  mode0      mode 0 (stop on reaching N)
  N1, N2, N64, N65, N473    other population sizes, with deaths

For the distribution test: DIST_RUNS binary runs at the truth (one file, one generator) reduced to the number of clusters and
the largest cluster of each run (dist_count, dist_largest).  --check compares two independent reference samples of that size
with the test's own statistic; it must stay under 4.

AR(1): a few elfi.examples.ar1.AR1 runs -- seed, phi, series.

    python scripts/make_golden_bdm.py [--check]
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

ROWS = 16
N_EVENTS = 1 << 14                                       # the replay's bound per row
#        name     seed        mode N   alpha                              delta                          tau
SETS = [('truth', 1,          1, 20,  np.full(ROWS, 0.2),                np.zeros(ROWS),                0.198),
        ('prior', 12345,      1, 20,  np.linspace(0.005, 2.005, ROWS),   np.zeros(ROWS),                0.198),
        ('slow',  777,        1, 20,  np.linspace(0.005, 0.012, ROWS),   np.zeros(ROWS),                0.198),
        ('deaths', 4000000000, 1, 20, np.full(ROWS, 0.5),                np.linspace(0.3, 1.5, ROWS),   0.198),
        ('mode0', 31,         0, 20,  np.linspace(0.05, 1.0, ROWS),      np.linspace(0.0, 0.3, ROWS),   0.198),
        ('N1',    41,         1, 1,   np.linspace(0.1, 1.0, ROWS),       np.linspace(0.0, 1.0, ROWS),   0.5),
        ('N2',    42,         0, 2,   np.linspace(0.1, 1.0, ROWS),       np.linspace(0.0, 1.0, ROWS),   0.5),
        ('N64',   43,         1, 64,  np.linspace(0.3, 1.0, ROWS),       np.linspace(0.0, 0.4, ROWS),   0.4),
        ('N65',   44,         1, 65,  np.linspace(0.3, 1.0, ROWS),       np.linspace(0.0, 0.4, ROWS),   0.4),
        ('N473',  45,         1, 473, np.linspace(0.5, 1.0, ROWS),       np.linspace(0.0, 0.3, ROWS),   0.6)]
DIST_RUNS, DIST_SEED, CHECK_SEED = 4096, 2017, 2018
AR1_RUNS = [(301, 0.9, 200, 3), (302, -0.5, 200, 2), (303, 1.0, 7, 4), (304, 0.0, 1, 2)]     # seed, phi, n_obs, batch


def build_binary(tmp):
    import ref_shim
    src = os.path.join(ref_shim.REFERENCE_ROOT, 'elfi', 'examples', 'cpp', 'bdm.cpp')
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    exe = os.path.join(tmp, 'bdm')
    subprocess.run([cxx, '-O2', '-std=c++11', '-o', exe, src], check=True)
    return exe


def run_binary(exe, tmp, params, N, mode, seed):
    """The rows as the binary parsed them, and the clusters it printed."""
    path = os.path.join(tmp, 'input.txt')
    rows = np.column_stack([params, np.full(len(params), N)])
    np.savetxt(path, rows, fmt='%.4f %.4f %.4f %d')
    out = subprocess.run([exe, path, '--seed', str(seed), '--mode', str(mode)], check=True, capture_output=True, text=True).stdout
    parsed = np.array([[float('%.4f' % v) for v in r[:3]] for r in rows])
    return parsed, np.loadtxt(out.splitlines(), dtype=np.int64, ndmin=2)


def moments_z(a, b):
    """z of the difference of the means and of the variances of two samples (tests/test_bdm_gpu.py uses the same)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ma, mb, va, vb = a.mean(), b.mean(), a.var(ddof=1), b.var(ddof=1)
    z_mean = (ma - mb) / np.sqrt(va / len(a) + vb / len(b))
    sa = (np.mean((a - ma) ** 4) - va ** 2) / len(a)     # the variance of a sample variance, to first order
    sb = (np.mean((b - mb) ** 4) - vb ** 2) / len(b)
    return z_mean, (va - vb) / np.sqrt(sa + sb)


def dist_sample(exe, tmp, seed):
    _, cl = run_binary(exe, tmp, np.tile([0.2, 0.0, 0.198], (DIST_RUNS, 1)), 20, 1, seed)
    return (cl > 0).sum(axis=1).astype(np.uint8), cl.max(axis=1).astype(np.uint8)


def main():
    import bdm_ref as R
    import ar1_ref as A
    import ref_shim
    ref_shim.install()
    from elfi.examples import ar1
    out = {'sets': np.array([s[0] for s in SETS])}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_binary(tmp)
        for name, seed, mode, N, alpha, delta, tau in SETS:
            params, cl = run_binary(exe, tmp, np.column_stack([alpha, delta, np.full(ROWS, tau)]), N, mode, seed)
            Cr, st, ev, reopened, _ = R.replay(params, N, mode, seed, N_EVENTS)
            assert cl.shape == (ROWS, N) and np.array_equal(Cr, cl), 'the statement does not reproduce the binary: ' + name
            print(name, 'events', ev.min(), '..', ev.max(), 'extinct', int((st == R.EXTINCT).sum()), 'reopened', int(reopened.sum()))
            out.update({name + '_params': params, name + '_N': N, name + '_mode': mode, name + '_seed': np.uint32(seed),
                        name + '_clusters': cl.astype(np.int16), name + '_events': ev, name + '_status': st,
                        name + '_reopened': reopened})
        count, largest = dist_sample(exe, tmp, DIST_SEED)
        out.update(dist_count=count, dist_largest=largest, dist_seed=DIST_SEED)
        if '--check' in sys.argv:
            c2, l2 = dist_sample(exe, tmp, CHECK_SEED)
            print('two reference samples of %d: clusters z = %.2f, %.2f; largest z = %.2f, %.2f (bound 4)' %
                  ((DIST_RUNS,) + moments_z(count, c2) + moments_z(largest, l2)))
    for k, (seed, phi, n_obs, batch) in enumerate(AR1_RUNS):
        X = ar1.AR1(phi, n_obs=n_obs, batch_size=batch, random_state=np.random.RandomState(seed))
        W = A.noise_from_state(np.random.RandomState(seed), batch, n_obs)
        assert np.array_equal(A.series(phi, W), X), 'the replayed draws are not what the simulator consumed'
        out.update({'ar1_%d_seed' % k: seed, 'ar1_%d_phi' % k: phi, 'ar1_%d_X' % k: X})
    out['ar1_runs'] = len(AR1_RUNS)
    path = os.path.join(ROOT, 'tests', 'golden', 'bdm.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
