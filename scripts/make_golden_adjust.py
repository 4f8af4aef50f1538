"""Records tests/golden/adjust.npz from the reference ELFI's LinearAdjustment (run where the reference is installed;
oracle/ref_shim.py makes it importable).

For every case of tests/adjust_ref.py (inputs are regenerated from the recipe, not stored) it stores
  ref_coef_<i>, ref_adj_<i>       LinearAdjustment (scikit-learn's LinearRegression, then _adjust) on the case's float inputs,
  truth_coef_<i>, truth_adj_<i>   the same in 40-digit arithmetic (mpmath) on the same float inputs: the columns centred
                                  and normalised, the normal equations formed and solved in 40 digits, rounded to double,
  e_coef, e_adj                   |reference - truth| in the metrics of adjust_ref,
  cond, crc                       the condition number of the centred, normalised regressors; the checksum of the inputs.
It refuses to write a case whose e_ref exceeds 1e-10 in either metric or whose condition number exceeds 1e6: the bound of
the tests (16 x e_ref) would say nothing there.

For the gauss run (adjust_ref.GAUSS_RUN: the example of adjust_posterior's docstring with fixed seeds) it stores results
only: the accepted mu, the two summaries, the discrepancies, the observed summaries, the reference's adjusted mu and
the 40-digit truth.

    python scripts/make_golden_adjust.py
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import ref_shim  # noqa: E402
import adjust_ref as R  # noqa: E402

mp.mp.dps = 40
mpf = mp.mpf


def truth(X, Y):
    """(coef (q, m), adjusted (n, q)) in 40 digits, rounded to double."""
    n, m = X.shape
    q = Y.shape[1]
    cols = [[mpf(float(v)) for v in X[:, j]] for j in range(m)]
    ycols = [[mpf(float(v)) for v in Y[:, t]] for t in range(q)]

    def centred(col):
        mean = mp.fsum(col) / n
        return [v - mean for v in col]
    xc = [centred(c) for c in cols]
    norms = [mp.sqrt(mp.fsum(v * v for v in c)) for c in xc]
    xn = [[v / nrm for v in c] for c, nrm in zip(xc, norms)]
    yc = [centred(c) for c in ycols]
    G = mp.matrix(m, m)
    for a in range(m):
        for b in range(a, m):
            G[a, b] = G[b, a] = mp.fsum(u * v for u, v in zip(xn[a], xn[b]))
    coef = []
    for t in range(q):
        sol = mp.lu_solve(G, mp.matrix([mp.fsum(u * v for u, v in zip(xn[a], yc[t])) for a in range(m)]))
        coef.append([sol[a] / norms[a] for a in range(m)])
    adj = np.empty((n, q))
    for t in range(q):
        for i in range(n):
            adj[i, t] = float(ycols[t][i] - mp.fsum(cols[a][i] * coef[t][a] for a in range(m)))
    return np.array([[float(c) for c in row] for row in coef]), adj


def reference(mod, X, Y):
    """LinearAdjustment on regressors X and parameters Y: its own pairing, scikit-learn fit and _adjust."""
    names = ['t%d' % t for t in range(Y.shape[1])]
    adj = mod.LinearAdjustment()
    adj._X = X
    adj._sample = mod.results.Sample(method_name='case', outputs={nm: Y[:, t].copy() for t, nm in enumerate(names)},
                                     parameter_names=names)
    adj._parameter_names = names
    adj._get_finite()
    for pair in adj._pairs():
        adj.regression_models.append(adj._fit1(*pair))
    adj._fitted = True
    out = adj.adjust()
    return (np.array([mdl.coef_ for mdl in adj.regression_models]),
            np.column_stack([out.outputs[nm] for nm in names]))


def main():
    elfi = ref_shim.install()
    from elfi.methods import post_processing as mod
    out = {}
    nc = len(R.CASES)
    e_coef, e_adj, cond, crc = np.zeros(nc), np.zeros(nc), np.zeros(nc), np.zeros(nc, dtype=np.int64)
    for ci, (seed, n, m, q, kind) in enumerate(R.CASES):
        X, Y = R.make_case(ci)
        rc, ra = reference(mod, X, Y)
        tc, ta = truth(X, Y)
        e_coef[ci], e_adj[ci] = R.coef_error(rc, tc), R.adjusted_error(ra, ta)
        cond[ci], crc[ci] = R.condition_number(X), R.checksum(ci)
        sa, sc = R.lstsq_adjust(X, Y)[:2]
        print('case %d n=%d m=%d q=%d %-10s cond %.2e  e_ref coef %.2e (%.1f eps) adjusted %.2e (%.1f eps)  lstsq %.1f / %.1f eps'
              % (ci, n, m, q, kind, cond[ci], e_coef[ci], e_coef[ci] / R.EPS, e_adj[ci], e_adj[ci] / R.EPS,
                 R.coef_error(sc, tc) / R.EPS, R.adjusted_error(sa, ta) / R.EPS), flush=True)
        if not (e_coef[ci] <= R.MAX_E_REF and e_adj[ci] <= R.MAX_E_REF and cond[ci] <= R.MAX_COND):
            raise SystemExit('case %d does not meet the yardstick conditions: its bound would be vacuous' % ci)
        out['ref_coef_%d' % ci], out['ref_adj_%d' % ci] = rc, ra
        out['truth_coef_%d' % ci], out['truth_adj_%d' % ci] = tc, ta
    out.update(cases=np.array([c[:4] for c in R.CASES], dtype=np.int64), kinds=np.array([c[4] for c in R.CASES]),
               e_coef=e_coef, e_adj=e_adj, cond=cond, crc=crc)

    # ---- the gauss run: the example of adjust_posterior's docstring
    from elfi.examples import gauss
    run = R.GAUSS_RUN
    m = gauss.get_model(seed_obs=run['seed_obs'])
    res = elfi.Rejection(m['d'], output_names=list(run['summaries']), batch_size=run['batch_size'],
                         seed=run['seed']).sample(run['n_samples'], bar=False)
    adj = mod.adjust_posterior(res, m, list(run['summaries']), list(run['parameters']), mod.LinearAdjustment())
    observed = np.array([np.asarray(m[s].observed, dtype=float).reshape(-1)[0] for s in run['summaries']])
    S = np.column_stack([res.outputs[s] for s in run['summaries']])
    mu = np.asarray(res.outputs['mu'], dtype=float)
    tc, ta = truth(S - observed, mu.reshape(-1, 1))
    e = R.adjusted_error(adj.outputs['mu'], ta[:, 0])
    print('gauss run: %d accepted, cond %.2e, e_ref adjusted %.2e (%.1f eps)' % (len(mu), R.condition_number(S - observed),
                                                                                  e, e / R.EPS))
    out.update(gauss_mu=mu, gauss_summaries=S, gauss_discrepancies=np.asarray(res.discrepancies, dtype=float),
               gauss_observed=observed, gauss_ref_adjusted=np.asarray(adj.outputs['mu'], dtype=float),
               gauss_truth_adjusted=ta[:, 0], gauss_e_adj=np.array(e))
    path = os.path.join(ROOT, 'tests', 'golden', 'adjust.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
