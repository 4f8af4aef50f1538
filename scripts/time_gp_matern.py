"""Developer tool: what the covariance function costs on one MI355X (the Matern kernels).  For each kernel
(rbf, matern32, matern52) at n = 2048 and 4096, d = 10: the rebuild (Gram matrix + factorisation), one acquisition
lock-step of 10 points (value and gradient of the LCB; triangular form and K^-1 form), nlml_grad and nlml_grad_ard.
Every call returns after the host has the result.  Ten warm-up calls, then R timed ones: median with the 10 % / 90 % range,
three rounds per row with the kernels alternating, so that drift of the clocks shows as a spread between rounds.
usage: python scripts/time_gp_matern.py [--lib PATH] [n:d ...]
--lib: another build of libelfihip.so; one without elfihip_gp_set_kernel (an older commit) times the rbf rows alone."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from elfi_amd import _lib

args = sys.argv[1:]
kinds = ['rbf', 'matern32', 'matern52']
if args[:1] == ['--lib']:
    _lib.LIB_PATH = os.path.abspath(args[1])
    args = args[2:]
    import ctypes
    if not hasattr(ctypes.CDLL(_lib.LIB_PATH), 'elfihip_gp_set_kernel'):
        _lib.PROTOTYPES.pop('elfihip_gp_set_kernel')
        _lib.PROTOTYPES.pop('elfihip_gp_get_kernel')
        kinds = ['rbf']
from benchlib.bolfi_bench import problem, heuristic_hyper
from elfi_amd.gp import GPHandle

shapes = [(int(a.split(':')[0]), int(a.split(':')[1])) for a in args] or [(2048, 10), (4096, 10)]
R = 100


def median_ms(call, reps=R):
    for _ in range(10):
        call()
    t = np.empty(reps)
    for i in range(reps):
        t0 = time.perf_counter()
        call()
        t[i] = time.perf_counter() - t0
    return 1e3 * np.median(t), 1e3 * np.percentile(t, 10), 1e3 * np.percentile(t, 90)


print('library', _lib.LIB_PATH)
for n, d in shapes:
    X, y, bounds = problem(n, d)
    h = heuristic_hyper(bounds, y)
    xs = np.random.RandomState(1).uniform([b[0] for b in bounds], [b[1] for b in bounds], (10, d))
    gps = {}
    for kind in kinds:
        gp = GPHandle(d, n, kernel=None if kind == 'rbf' else kind)
        gp.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
        gp.set_data(X, y)
        gp.factorize()
        gps[kind] = gp
    rows = [('rebuild', lambda g: g.factorize(), 30, 2),
            ('lockstep10', lambda g: g.lcb(xs, 3.0), R, 2),
            ('lockstep10_kinv', lambda g: g.lcb(xs, 3.0), R, 3),
            ('nlml_grad', lambda g: g.nlml_grad(), R, 2),
            ('nlml_grad_ard', lambda g: g.nlml_grad_ard(), R, 2)]
    for name, fn, reps, form in rows:
        for rnd in range(3):
            for kind in kinds:
                gp = gps[kind]
                gp.set_lockstep_form(form)
                print('n=%5d d=%2d %-16s %-9s round %d  median %.4f ms (10%% %.4f, 90%% %.4f)' %
                      ((n, d, name, kind, rnd) + median_ms(lambda: fn(gp), reps)), flush=True)
        for gp in gps.values():
            gp.set_lockstep_form(0)
    for gp in gps.values():
        gp.close()
