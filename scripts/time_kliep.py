"""Times the device KLIEP fit on one MI355X next to the reference's host class on the same inputs.

  one fit             Nx = Ny = 1000, d = 2, n = 100 basis functions, AdaptiveThresholdSMC's settings (epsilon 0.001,
                      max_iter 200, abs_tol 0.01, a convergence check every 20 steps), one scale
  cross-validation    the same inputs, 7 scales (10^-1 ... 10^5, the list the sampler passes with optimize=True) x 5 folds:
                      7 full fits and 35 fold fits in one call

Every device figure: 3 warm-up calls, then 20 timed calls (host wall clock around the synchronising call, so the copies
count); median, minimum and maximum are printed.  The reference (oracle/ref_shim.py; skipped when it is not installed)
runs its own loop on the same box: DensityRatioEstimation.fit for the one fit (1 warm-up, 3 timed repeats) and one
_KLIEP_lcv scale for the cross-validation (1 repeat; a scale is 5 fold fits, the device figure covers 7 scales).

    python scripts/time_kliep.py [--json out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle')):
    sys.path.insert(0, p)

SMC = dict(n=100, epsilon=0.001, max_iter=200, abs_tol=0.01, conv_check_interval=20)


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), reps=reps)


def main():
    import elfi_amd
    import ref_shim
    DRE = None
    if ref_shim.available():
        ref_shim.install()
        from elfi.methods.density_ratio_estimation import DensityRatioEstimation as DRE
    rs = np.random.RandomState(0)
    N, d = 1000, 2
    x, y = rs.randn(N, d), rs.randn(N, d) * 1.5 + 0.3
    wx, wy = rs.uniform(0.5, 1.5, N), rs.uniform(0.5, 1.5, N)
    sigma = 1.0 * 1.5 / np.sqrt(1.5 ** 2 - 1.0)
    scales = list(10.0 ** np.arange(-1, 6))
    out = {}

    one = elfi_amd.kliep_fit(x, y, wx, wy, sigma=sigma, **SMC)
    assert np.all(np.isfinite(one['w']))
    rec = dict(Nx=N, Ny=N, d=d, iters=int(one['iters'][0]),
               device=timed(lambda: elfi_amd.kliep_fit(x, y, wx, wy, sigma=sigma, **SMC), 3, 20))
    if DRE is not None:
        def host():
            est = DRE(fold=5, **SMC)
            est.fit(x, y, weights_x=wx, weights_y=wy, sigma=float(sigma))
            return est.max_ratio()
        rec['reference'] = timed(host, 1, 3)
    out['one_fit'] = rec
    print('one_fit', json.dumps(rec), flush=True)

    cv = elfi_amd.kliep_fit(x, y, wx, wy, sigma=scales, fold=5, **SMC)
    rec = dict(scales=len(scales), folds=5, lcv=[float(v) for v in cv['lcv']], iters=[int(v) for v in cv['iters']],
               device=timed(lambda: elfi_amd.kliep_fit(x, y, wx, wy, sigma=scales, fold=5, **SMC), 3, 20))
    if DRE is not None:
        est = DRE(fold=5, **SMC)
        est.fit(x[:100], y[:100], sigma=float(sigma))                 # sets the attributes _KLIEP_lcv reads ...
        est.x_len, est.y_len, est.x, est.theta = N, N, x, x[:100]     # ... then the full inputs, as fit would set them
        est.weights_x, est.weights_y = wx / wx.sum(), wy / wy.sum()
        with np.errstate(all='ignore'):
            rec['reference_one_scale'] = timed(lambda: est._KLIEP_lcv(x, y, 1.0), 0, 1)
    out['cross_validation'] = rec
    print('cross_validation', json.dumps(rec), flush=True)
    if '--json' in sys.argv:
        path = sys.argv[sys.argv.index('--json') + 1]
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
