"""Times the wide Gaussian synthetic likelihood (csrc/synlik_wide.hip) on one MI355X at the scratch-assay width, 145
summaries, next to the reference's host function on the same inputs.

  single group           n = 500, m = 145, standard likelihood: two launches and the copies
  lock-step shape        G = 64 groups, n = 500, m = 145, standard likelihood
  select_penalty shape   M = 20 groups, n = 500, m = 145, 1 prefix, the 31 default Warton penalties: 620 evaluations in one call

Every figure: 3 warm-up calls, then 20 timed calls (host wall clock around the synchronising call, so the copies count);
median, minimum and maximum are printed.  The reference (oracle/ref_shim.py; skipped when it is not installed) runs the
same evaluations as a Python loop over its gaussian_syn_likelihood, 1 warm-up and 5 timed repeats.

    python scripts/time_synlik_wide.py [--json out.json]
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
        from elfi.methods.bsl import pdf_methods as P
    rs = np.random.RandomState(0)
    out = {}

    def shape(name, G, n, m, pens):
        X = rs.randn(G, n, m) * np.linspace(1, 10, m) + rs.uniform(-20, 20, m)
        y = rs.uniform(-20, 20, m)
        kw = dict(shrinkage='warton', penalties=pens) if pens else {}
        rec = dict(G=G, n=n, m=m, penalties=len(pens or []), device=timed(lambda: elfi_amd.wide_syn_loglik(X, y, **kw), 3, 20))
        if P is not None:
            def host():
                for g in range(G):
                    for pen in (pens or [None]):
                        P.gaussian_syn_likelihood(X[g], y, shrinkage='warton' if pens else None, penalty=pen)
            rec['reference'] = timed(host, 1, 5)
        out[name] = rec
        print(name, json.dumps(rec), flush=True)

    shape('single_group', 1, 500, 145, None)
    shape('lockstep', 64, 500, 145, None)
    shape('select_penalty', 20, 500, 145, list(np.arange(0.2, 0.8, 0.02)))
    if '--json' in sys.argv:
        path = sys.argv[sys.argv.index('--json') + 1]
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
