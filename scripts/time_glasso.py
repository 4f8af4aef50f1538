"""Times the graphical-lasso synthetic likelihood on one MI355X next to the reference's host function on the same inputs.

  select_glasso_penalty shape   M = 20 groups, n = 1000, m = 32, the 20 default penalties exp(-5.5 .. -1.7) in one call
  one problem                   n = 192, m = 64, the smallest default penalty

Every figure: 3 warm-up calls, then 20 timed calls (host wall clock around the synchronising call, so the copies count);
median, minimum and maximum are printed, and the sweeps over all columns the solver took.  The reference
(oracle/ref_shim.py; skipped when it is not installed) runs gaussian_syn_likelihood(..., shrinkage='glasso') in its Python
loop over the same groups and penalties, once (it takes tens of seconds and warns where it does not converge).

    python scripts/time_glasso.py [--json out.json]
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

from time_synlik import timed  # noqa: E402


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
        Z = rs.randn(G, n, m)
        for j in range(1, m):
            Z[:, :, j] = 0.6 * Z[:, :, j - 1] + 0.8 * Z[:, :, j]
        X = Z * np.linspace(1, 2, m) + rs.uniform(-3, 3, m)
        y = X[0, 0] + 0.1
        rec = dict(G=G, n=n, m=m, penalties=len(pens), device=timed(lambda: elfi_amd.glasso_loglik(X, y, penalties=pens), 3, 20))
        S = np.stack([np.cov(X[g], rowvar=False) for g in range(G)])
        n_iter, status = elfi_amd.graphical_lasso(S, pens, return_n_iter=True, return_status=True)[2:]
        rec['sweeps'] = dict(min=int(n_iter.min()), median=float(np.median(n_iter)), max=int(n_iter.max()))
        rec['status'] = np.bincount(status.ravel(), minlength=3).tolist()
        if P is not None:
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                for g in range(G):
                    for pen in pens:
                        P.gaussian_syn_likelihood(X[g], y, shrinkage='glasso', penalty=pen)
            rec['reference_ms'] = (time.perf_counter() - t0) * 1e3
        out[name] = rec
        print(name, json.dumps(rec), flush=True)

    shape('select_glasso_penalty', 20, 1000, 32, list(np.exp(np.arange(-5.5, -1.5, 0.2))))
    shape('one_problem_m64', 1, 192, 64, [float(np.exp(-5.5))])
    if '--json' in sys.argv:
        with open(sys.argv[sys.argv.index('--json') + 1], 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
