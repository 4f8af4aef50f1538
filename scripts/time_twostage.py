"""Times the summary-statistic selection (Nunes & Balding's two-stage procedure) on one MI355X next to the reference's
TwoStageSelection on the same host: MA2 with the four candidate statistics of tests/twostage_ref.py (15 combinations).

  small   run(n_sim=20000, n_acc=500, n_closest=20, batch_size=5000)       the fixture's run
  large   run(n_sim=10**6, n_acc=10**4, n_closest=100, batch_size=50000)

The device class is timed whole (host wall clock around `run`) and in its parts: the one simulation pass (ELFI's own
Rejection and the model's NumPy simulator, on the host) and the three device calls (`subset_best`, `knn_entropy`,
`mrsse`; synchronising, copies included).  1 warm-up run, then the median of 3 (1 for the large run).  The reference's
class (the imported ELFI's, through oracle/ref_shim.py where that copy is present; skipped with --no-reference) runs once
per size: one Rejection per combination, one cKDTree query per accepted parameter, one norm per closest parameter.  Both
must choose the same combination.

    python scripts/time_twostage.py [--large] [--no-reference] [--json out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

SIZES = {'small': dict(n_sim=20000, n_acc=500, n_closest=20, batch_size=5000),
         'large': dict(n_sim=10 ** 6, n_acc=10 ** 4, n_closest=100, batch_size=50000)}


def main():
    import ref_shim
    import twostage_ref as R
    elfi = ref_shim.install() if ref_shim.available() else __import__('elfi')
    import elfi_amd
    from elfi_amd import twostage
    from elfi.methods.diagnostics import TwoStageSelection
    cands = R.ma2_candidates()
    out = {}
    for name in ['small'] + (['large'] if '--large' in sys.argv else []):
        size = SIZES[name]
        parts = {}

        def clocked(key, fn):
            def wrapper(*a, **k):
                t0 = time.perf_counter()
                r = fn(*a, **k)
                parts[key] = parts.get(key, 0.0) + time.perf_counter() - t0
                return r
            return wrapper
        sel = elfi_amd.HipTwoStageSelection(R.ma2_simulator(elfi), 'euclidean', list_ss=cands, seed=1)
        sel._simulate = clocked('simulation_pass_s', sel._simulate)
        saved = {k: getattr(twostage, k) for k in ('subset_best', 'knn_entropy', 'mrsse')}
        for k, fn in saved.items():
            setattr(twostage, k, clocked(k + '_s', fn))
        runs, chosen = [], None
        reps = 3 if name == 'small' else 1
        for rep in range(1 + reps):
            parts.clear()
            t0 = time.perf_counter()
            chosen = sel.run(k=4, **size)
            runs.append(dict(parts, total_s=time.perf_counter() - t0))
        for k, fn in saved.items():
            setattr(twostage, k, fn)
        timed = sorted(runs[1:], key=lambda r: r['total_s'])[len(runs[1:]) // 2]
        rec = dict(size, combinations=len(sel.ss_candidates), device=timed,
                   chosen=[f.__name__ for f in chosen])
        if '--no-reference' not in sys.argv:
            ref = TwoStageSelection(R.ma2_simulator(elfi), 'euclidean', list_ss=cands, seed=1)
            t0 = time.perf_counter()
            ref_chosen = ref.run(k=4, **size)
            rec['reference_total_s'] = time.perf_counter() - t0
            rec['reference_chosen'] = [f.__name__ for f in ref_chosen]
            assert rec['reference_chosen'] == rec['chosen'], (rec['reference_chosen'], rec['chosen'])
        out[name] = rec
        print(name, json.dumps(rec), flush=True)
    if '--json' in sys.argv:
        path = sys.argv[sys.argv.index('--json') + 1]
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
