"""Times the wide whitened semiparametric synthetic likelihood (csrc/wsemibsl_wide.hip) on one MI355X at the scratch-assay
width, 145 summaries, next to the host statement of the same formulas on the same inputs.

  single group           n = 500, m = 145: seven launches and the copies
  lock-step shape        G = 64 groups, n = 500, m = 145
  select_penalty shape   M = 20 groups, n = 500, m = 145, 1 prefix, the 31 default Warton penalties: 620 evaluations in one call

Every device figure: 3 warm-up calls, then 20 timed calls (host wall clock around the synchronising call, so the copies
count); median, minimum and maximum are printed.  The host statement (tests/wsemibsl_ref.py, NumPy and SciPy in float64)
runs the same evaluations in its Python loop -- wparts once per group, loglik_from_parts per penalty -- 1 warm-up and 3
timed repeats.  The whitening matrix is the reference's formula on the scores of an independent draw of 4 m + 50 rows.  No
per-kernel split is taken here.

    python scripts/time_wsemibsl_wide.py [--json out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
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
    import wsemibsl_ref as R
    rs = np.random.RandomState(0)
    n, m = 500, 145
    scale, loc = np.linspace(1, 10, m), rs.uniform(-20, 20, m)
    Q = R.S.parts(rs.randn(4 * m + 50, m) * scale + loc, loc)[3]
    w, v = np.linalg.eigh(np.cov((Q - Q.mean(0)) / Q.std(0), rowvar=False))
    W = np.round(np.diag(w ** -0.5) @ v.T, 8)
    out = {}

    def host(X, y, pens):
        for Xg in X:
            logpdf, u, rho, d, _, _ = R.wparts(Xg, y, W)
            for pen in pens or [None]:
                R.loglik_from_parts(logpdf, u, rho, d, W, n, pen)

    def shape(name, G, pens):
        X = rs.randn(G, n, m) * scale + loc
        y = X[0, 0] + rs.randn(m)
        kw = dict(shrinkage='warton', penalties=pens) if pens else {}
        rec = dict(G=G, n=n, m=m, penalties=len(pens or []),
                   device=timed(lambda: elfi_amd.wide_wsemi_loglik(X, y, W, **kw), 3, 20),
                   host_statement=timed(lambda: host(X, y, pens), 1, 3))
        out[name] = rec
        print(name, json.dumps(rec), flush=True)

    shape('single_group', 1, None)
    shape('lockstep', 64, None)
    shape('select_penalty', 20, list(np.arange(0.2, 0.8, 0.02)))
    if '--json' in sys.argv:
        path = sys.argv[sys.argv.index('--json') + 1]
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
