"""Developer tool: the ARD hyper-gradient next to the isotropic one on the same handle, and the evidence upload's share
of one evaluation of an ARD hyper-parameter search (per-dimension lengthscales).
usage: python scripts/time_grad_ard.py [--lib PATH] [n:d ...]
--lib: another build of libelfihip.so (one without the ARD entry point times the isotropic gradient alone)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from elfi_amd import _lib

args = sys.argv[1:]
if args[:1] == ['--lib']:
    _lib.LIB_PATH = os.path.abspath(args[1])
    args = args[2:]
    import ctypes
    if not hasattr(ctypes.CDLL(_lib.LIB_PATH), 'elfihip_gp_nlml_grad_ard'):
        _lib.PROTOTYPES.pop('elfihip_gp_nlml_grad_ard')
from benchlib.bolfi_bench import problem, heuristic_hyper
from elfi_amd.gp import GPHandle, ScaledGPHandle

has_ard = 'elfihip_gp_nlml_grad_ard' in _lib.PROTOTYPES
shapes = [(int(a.split(':')[0]), int(a.split(':')[1])) for a in args] or [(2048, 10), (2048, 20), (4096, 10), (4096, 20)]
R = 200


def median_ms(call):
    for _ in range(10):
        call()
    t = np.empty(R)
    for i in range(R):
        t0 = time.perf_counter()
        call()          # returns after the host has read the result behind the kernel's ticket
        t[i] = time.perf_counter() - t0
    return 1e3 * np.median(t), 1e3 * np.percentile(t, 10), 1e3 * np.percentile(t, 90)


print('library', _lib.LIB_PATH)
for n, d in shapes:
    X, y, bounds = problem(n, d)
    h = heuristic_hyper(bounds, y)
    gp = GPHandle(d, n)
    gp.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    gp.set_data(X, y)
    gp.factorize()
    # alternate the two forms, three rounds each
    for rnd in range(3):
        print('n=%5d d=%2d round %d  nlml_grad     median %.4f ms (10%% %.4f, 90%% %.4f)' % ((n, d, rnd) + median_ms(gp.nlml_grad)))
        if has_ard:
            print('n=%5d d=%2d round %d  nlml_grad_ard median %.4f ms (10%% %.4f, 90%% %.4f)' % ((n, d, rnd) + median_ms(gp.nlml_grad_ard)))
    gp.close()
    if not has_ard:
        continue
    # one evaluation of an ARD search: set_hyper with new lengthscales (uploads X / l again) + rebuild + gradient
    sg = ScaledGPHandle(d, n)
    sg.set_data(X, y)
    ell = np.full(d, h['ls'])
    t_up, t_all = np.empty(40), np.empty(40)
    for i in range(45):
        ell = ell * (1.0 + 1e-3)
        t0 = time.perf_counter()
        sg.set_hyper(h['var'], ell, h['bias'], h['noise'])
        t1 = time.perf_counter()
        sg.factorize()
        sg.nlml_grad()
        t2 = time.perf_counter()
        if i >= 5:
            t_up[i - 5], t_all[i - 5] = t1 - t0, t2 - t0
    sg.profile(1)
    for _ in range(5):
        sg.factorize()
        sg.nlml_grad()
    ph = {k: v[0] / max(v[1], 1) for k, v in sg.profile(0).items() if v[1]}
    print('n=%5d d=%2d  ARD search evaluation: wall %.3f ms, of which set_hyper + upload %.3f ms (%.1f %%) | device: gram %.3f '
          'sweep %.3f alpha %.3f kinv_grad %.3f' % (n, d, 1e3 * np.median(t_all), 1e3 * np.median(t_up),
                                                    100 * np.median(t_up) / np.median(t_all), ph.get('gram', 0),
                                                    ph.get('sweep', 0), ph.get('alpha', 0), ph.get('kinv_grad', 0)))
    sg.close()
