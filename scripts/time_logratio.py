"""Times the batched logistic-regression ratio estimate on one MI355X next to the reference's classifier on the same
inputs.

  single group   n = nm = 1000, m = 32: bound by the launch and the copies as much as by arithmetic
  lock-step      G = 64 groups, n = nm = 500, m = 20, one shared marginal, in one call

Every figure: 3 warm-up calls, then 20 timed calls (host wall clock around the synchronising call, so the copies count);
median, minimum and maximum are printed, with the outer steps the fits took.  The reference (oracle/ref_shim.py; skipped
when it is not installed) runs the same fits as a Python loop over LogisticRegression().fit and
predict_log_likelihood_ratio (elfi/methods/classifier.py:72-121: liblinear at its default tol=1e-4), 1 warm-up and 3 timed
repeats.  The device fits run to the default tol of elfi_amd.log_ratio (optimality violation 1e-13).

    python scripts/time_logratio.py [--json out.json]
"""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle')):
    sys.path.insert(0, p)


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
    LR = None
    if ref_shim.available():
        ref_shim.install()
        from elfi.methods.classifier import LogisticRegression as LR
    rs = np.random.RandomState(0)
    out = {}

    def shape(name, G, n, m):
        X = rs.randn(G, n, m) + rs.uniform(0.0, 0.5, (G, 1, 1))
        M = 1.3 * rs.randn(n, m)
        obs = rs.randn(1, m) + 0.2
        lr, parts = elfi_amd.log_ratio(X, M, obs, return_parts=True)
        assert np.all(np.isfinite(lr)) and np.all(parts['status'] == 0)
        rec = dict(G=G, n=n, nm=n, m=m, n_iter_max=int(parts['n_iter'].max()), n_iter_mean=float(parts['n_iter'].mean()),
                   device=timed(lambda: elfi_amd.log_ratio(X, M, obs), 3, 20))
        if LR is not None:
            y = np.concatenate([np.ones(n), -np.ones(n)])

            def host():
                vals = []
                for g in range(G):
                    clf = LR()
                    with warnings.catch_warnings():
                        warnings.simplefilter('ignore')
                        clf.fit(np.vstack([X[g], M]), y)
                    vals.append(clf.predict_log_likelihood_ratio(obs)[0])
                return np.array(vals)
            rec['reference'] = timed(host, 1, 3)
            rec['max_abs_difference'] = float(np.abs(host() - lr[:, 0]).max())     # the reference stops at tol=1e-4
        out[name] = rec
        print(name, json.dumps(rec), flush=True)

    shape('single_group', 1, 1000, 32)
    shape('lockstep', 64, 500, 20)
    if '--json' in sys.argv:
        path = sys.argv[sys.argv.index('--json') + 1]
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
