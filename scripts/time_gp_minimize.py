"""Times BOLFI's extract_result() on one MI355X, the reference's way next to the device search, on a synthetic bowl at
(n, d) = (1024, 2), (4096, 10), (8192, 20).  Needs the reference package (oracle/ref_shim.py).

  reference path   elfi.BOLFI(..., target_model=HipGPRegression).extract_result(): the reference class holding the device
                   model (bolfi.py:180-199 -> stochastic_optimization, elfi/methods/bo/utils.py:9-37 -> SciPy's
                   differential_evolution over HipGPRegression.predict_mean, one elfihip_gp_predict of one point per
                   evaluation).  Generations and evaluations are read off a direct call of differential_evolution with the
                   very arguments stochastic_optimization passes (same seed, so the same run); that call is also the
                   path's warm-up.  Then extract_result() is timed 3 times.
  device path      elfi_amd.HipBOLFI(...).extract_result() on the same evidence and hyper-parameters: 1 warm-up, 5 timed calls;
                   generations and evaluations from minimize_mean(seed=bolfi.seed, return_info=True), the call it makes.

Median, minimum and maximum of the wall time are printed; the ratio is median over median.  Both x_min are compared on the
device's mean.

    python scripts/time_gp_minimize.py [--json out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle')):
    sys.path.insert(0, p)

SHAPES = [(1024, 2), (4096, 10), (8192, 20)]


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), reps=reps)


def bowl(n, d, seed):
    rs = np.random.RandomState(seed)
    lo, hi = -2.0 * np.ones(d), 2.0 * np.ones(d)
    X = rs.uniform(lo, hi, (n, d))
    centre, w = rs.uniform(0.6 * lo, 0.6 * hi), rs.uniform(0.5, 1.5, d)
    y = ((X - centre) ** 2 * w).sum(axis=1) / d + 0.02 * rs.randn(n)
    hyper = dict(var=float(4 * np.var(y) + 1), ls=float(4.0 / 3.0 * np.sqrt(d)), bias=float(np.mean(y) ** 2 + 1),
                 noise=0.02 ** 2 + 1e-4)
    return X, y, hyper


def bolfi_pair(elfi, X, y, hyper):
    """(the reference's BOLFI holding a device model, HipBOLFI) on the same evidence and hyper-parameters."""
    import scipy.stats as ss
    import elfi_amd
    d = X.shape[1]
    names = ['p%02d' % i for i in range(d)]
    bounds = {nm: (-2.0, 2.0) for nm in names}
    out = []
    for hip in (False, True):
        mdl = elfi.new_model()
        pri = [elfi.Prior(ss.uniform, -2, 4, model=mdl, name=nm) for nm in names]
        sim = elfi.Simulator(lambda *th, batch_size=1, random_state=None: np.column_stack([np.ravel(t) for t in th]), *pri,
                             observed=np.zeros((1, d)), name='sim')
        dist = elfi.Distance('euclidean', sim, name='d')
        pre = {nm: X[:, i].copy() for i, nm in enumerate(names)}
        pre['d'] = y.copy()
        if hip:
            b = elfi_amd.HipBOLFI(dist, batch_size=1, initial_evidence=pre, bounds=bounds, seed=1)
        else:
            b = elfi.BOLFI(dist, batch_size=1, initial_evidence=pre, bounds=bounds, seed=1,
                           target_model=elfi_amd.HipGPRegression(names, bounds=bounds))
        b.target_model.fix_hyperparameters(**hyper)
        out.append(b)
    return out


def main():
    import ref_shim
    elfi = ref_shim.install()
    import elfi.clients.native as native
    native.set_as_default()
    from scipy.optimize import differential_evolution
    out = {}
    for n, d in SHAPES:
        X, y, hyper = bowl(n, d, seed=n + d)
        ref_b, hip_b = bolfi_pair(elfi, X, y, hyper)
        gp = ref_b.target_model
        de = differential_evolution(func=lambda x: gp.predict_mean(x).ravel(), bounds=gp.bounds, maxiter=1000, polish=True,
                                    init='latinhypercube', seed=ref_b.seed)
        res_r, t_ref = timed(ref_b.extract_result, 3)
        hip_b.extract_result()
        res_h, t_dev = timed(hip_b.extract_result, 5)
        info = hip_b.target_model.minimize_mean(seed=hip_b.seed, return_info=True)[2]
        names = gp.parameter_names
        xr = np.array([np.ravel(res_r.x_min[nm])[0] for nm in names])
        xh = np.array([np.ravel(res_h.x_min[nm])[0] for nm in names])
        mu = hip_b.target_model.device_handle.predict_mean(np.vstack([xr, xh]))[:, 0]
        rec = dict(n=n, d=d,
                   reference=dict(t_ref, generations=int(de.nit), evaluations=int(de.nfev), mean_at_x=float(mu[0])),
                   device=dict(t_dev, generations=info['generations'], evaluations=info['evaluations'],
                               polish_accepted=info['polish_accepted'], mean_at_x=float(mu[1])),
                   distance=float(np.max(np.abs(xr - xh))), counted_run_is_timed_run=bool(np.array_equal(xr, de.x)),
                   ratio=t_ref['median_ms'] / t_dev['median_ms'])
        out['n%d_d%d' % (n, d)] = rec
        print(json.dumps(rec), flush=True)
    if '--json' in sys.argv:
        with open(sys.argv[sys.argv.index('--json') + 1], 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
