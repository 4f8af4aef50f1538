"""Times the batched semiparametric synthetic likelihood on one MI355X next to the reference's host function on the same
inputs.

  select_penalty shape   M = 20 groups, n = 1000, m = 32, 1 prefix, the 31 default Warton penalties in one call
  lock-step shape        G = 64 groups, n = 500, m = 20, no shrinkage
  single group           n = 500, m = 20: bound by the two launches and the copies, not by arithmetic

Every figure: 3 warm-up calls, then 20 timed calls (host wall clock around the synchronising call, so the copies count);
median, minimum and maximum are printed.  The reference (oracle/ref_shim.py; skipped when it is not installed) runs the
same evaluations as a Python loop over pdf_methods.semi_param_kernel_estimate, 1 warm-up and 3 timed repeats.  That
function still uses np.NINF: the script sets the alias for itself.

    python scripts/time_semibsl.py [--json out.json]
"""
import json
import os
import sys
import time

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
    P = None
    if ref_shim.available():
        ref_shim.install()
        np.NINF = -np.inf
        from elfi.methods.bsl import pdf_methods as P
    rs = np.random.RandomState(0)
    out = {}

    def shape(name, G, n, m, pens):
        X = rs.randn(G, n, m) * np.linspace(1, 10, m) + rs.uniform(-20, 20, m)
        y = X[0, :5].mean(axis=0)
        kw = dict(shrinkage='warton', penalties=pens) if pens else {}
        ll = elfi_amd.semi_loglik(X, y, **kw)
        assert np.all(np.isfinite(ll))
        rec = dict(G=G, n=n, m=m, penalties=len(pens or []), device=timed(lambda: elfi_amd.semi_loglik(X, y, **kw), 3, 20))
        if P is not None:
            def host():
                for g in range(G):
                    for pen in (pens or [None]):
                        P.semi_param_kernel_estimate(X[g], y, shrinkage='warton' if pens else None, penalty=pen)
            rec['reference'] = timed(host, 1, 3)
        out[name] = rec
        print(name, json.dumps(rec), flush=True)

    shape('select_penalty', 20, 1000, 32, list(np.arange(0.2, 0.8, 0.02)))
    shape('lockstep', 64, 500, 20, None)
    shape('single_group', 1, 500, 20, None)
    if '--json' in sys.argv:
        path = sys.argv[sys.argv.index('--json') + 1]
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
