"""Times the wide semiparametric synthetic likelihood (csrc/semibsl_wide.hip) on one MI355X at the scratch-assay width, 145
summaries, next to the narrow kernel at its widest and to the host statement of the same formulas on the same inputs.

  single group           n = 500, m = 145: three launches and the copies
  lock-step shape        G = 64 groups, n = 500, m = 145
  select_penalty shape   M = 20 groups, n = 500, m = 145, 1 prefix, the 31 default Warton penalties: 620 evaluations in one call
  narrow                 semi_loglik (csrc/semibsl.hip) at n = 500, m = 64, the same three shapes

Every device figure: 3 warm-up calls, then 20 timed calls (host wall clock around the synchronising call, so the copies
count); median, minimum and maximum are printed.  The host statement (tests/semibsl_ref.py: semi_loglik_ref, NumPy and
SciPy in float64) runs the same evaluations in its Python loop, 1 warm-up and 3 timed repeats.

    python scripts/time_semibsl_wide.py [--json out.json]
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
    import semibsl_ref
    rs = np.random.RandomState(0)
    out = {}

    def shape(name, call, G, n, m, pens, host):
        X = rs.randn(G, n, m) * np.linspace(1, 10, m) + rs.uniform(-20, 20, m)
        y = X[0, 0] + rs.randn(m)
        kw = dict(shrinkage='warton', penalties=pens) if pens else {}
        rec = dict(G=G, n=n, m=m, penalties=len(pens or []), device=timed(lambda: call(X, y, **kw), 3, 20))
        if host:
            rec['host_statement'] = timed(lambda: semibsl_ref.semi_loglik_ref(X, y, n_groups=G, **kw), 1, 3)
        out[name] = rec
        print(name, json.dumps(rec), flush=True)

    lmdas = list(np.arange(0.2, 0.8, 0.02))
    for tag, call, m in (('', elfi_amd.wide_semi_loglik, 145), ('narrow_', elfi_amd.semi_loglik, 64)):
        shape(tag + 'single_group', call, 1, 500, m, None, not tag)
        shape(tag + 'lockstep', call, 64, 500, m, None, not tag)
        shape(tag + 'select_penalty', call, 20, 500, m, lmdas, not tag)
    if '--json' in sys.argv:
        path = sys.argv[sys.argv.index('--json') + 1]
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
