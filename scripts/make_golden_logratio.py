"""Records tests/golden/logratio.npz from the reference ELFI's ratio-estimation classifier (run where the reference is
installed; oracle/ref_shim.py makes it importable).

For every case of tests/logratio_ref.py (inputs are regenerated from the recipe, not stored) it stores
  ref_default  the reference's LogisticRegression() as shipped (scikit-learn's liblinear at tol=1e-4): coefficients,
               intercept and the log ratio at the case's observed row,
  ref_tight    the same with config={'penalty': 'l1', 'solver': 'liblinear', 'tol': 1e-12, 'max_iter': 100000},
  truth        ref_tight polished on its support: Newton steps on  g_S(v) + sign(v_S) = 0  with the gradient in 40-digit
               arithmetic (mpmath; the scaler's sums too) and a float64 Hessian, until the violation stops falling;
               coefficients, intercept, support and log ratio, rounded to double,
  e_default, e_tight   the largest |ref - truth| over log ratio, coefficients and intercept,
  kkt_tight    the optimality violation of ref_tight (tests/logratio_ref.py's statement, the reference's own scaler),
  kkt_truth    the violation of truth in 40 digits, and slack = the largest |g_j| over truth's zero coordinates.
The script refuses to write when a zero coordinate of a truth has |g_j| > 1 - 1e-3 or truth and ref_tight differ in
support: the support of such a case is ambiguous; change its seed.

    python scripts/make_golden_logratio.py
"""
import os
import sys
import warnings

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import ref_shim  # noqa: E402
import logratio_ref as R  # noqa: E402

mp.mp.dps = 40
mpf = mp.mpf
TIGHT = {'penalty': 'l1', 'solver': 'liblinear', 'tol': 1e-12, 'max_iter': 100000}


def mp_design(X, M):
    """Standardised stacked rows (lists of mpf per column), labels; the scaler in 40 digits."""
    Z = np.vstack([X, M])
    N, m = Z.shape
    cols, means, scales = [], [], []
    for j in range(m):
        col = [mpf(float(x)) for x in Z[:, j]]
        mu = mp.fsum(col) / N
        var = mp.fsum((x - mu) ** 2 for x in col) / N
        const = var <= N * mpf(R.EPS) * var + (N * mu * mpf(R.EPS)) ** 2
        s = mpf(1) if const else mp.sqrt(var)
        cols.append([(x - mu) / s for x in col])
        means.append(mu)
        scales.append(s)
    y = [1] * len(X) + [-1] * len(M)
    return cols, y, means, scales


def mp_gradient(cols, y, v, C):
    """Gradient of the smooth part at v (list of mpf, intercept last): sums over the columns with v_j != 0 only."""
    N, m = len(y), len(cols)
    act = [j for j in range(m) if v[j] != 0]
    coef = []
    for i in range(N):
        t = v[m] + mp.fsum(v[j] * cols[j][i] for j in act)
        coef.append(-y[i] / (1 + mp.exp(y[i] * t)))
    g = [C * mp.fdot(cols[j], coef) for j in range(m)]
    g.append(C * mp.fsum(coef))
    return g


def mp_violation(g, v):
    return max(abs(gj + mp.sign(vj)) if vj != 0 else max(abs(gj) - 1, mpf(0)) for gj, vj in zip(g, v))


def polish(X, M, C, v0):
    """truth (list of mpf), its violation and the slack of the zero coordinates, from the float start v0."""
    cols, y, means, scales = mp_design(X, M)
    Zf, yf = R.design(X, M)
    v = [mpf(float(x)) for x in v0]
    S = [j for j in range(len(v)) if v[j] != 0]
    sg = [mp.sign(v[j]) for j in S]
    best = None
    for _ in range(12):
        g = mp_gradient(cols, y, v, mpf(C))
        viol = mp_violation(g, v)
        if best is not None and viol >= best[1]:
            break
        best = ([+x for x in v], viol, g)
        if not S:
            break
        vf = np.array([float(x) for x in v])
        p = 1.0 / (1.0 + np.exp(yf * (Zf @ vf)))
        H = C * (Zf[:, S].T * (p * (1 - p))) @ Zf[:, S]
        r = [g[j] + s for j, s in zip(S, sg)]
        # the step in double-double: solve with the float Hessian for the residual's head, then for what is left of it
        rh = np.array([float(x) for x in r])
        rl = np.array([float(x - mpf(float(x))) for x in r])
        step_h, step_l = np.linalg.solve(H, rh), np.linalg.solve(H, rl)
        for k, j in enumerate(S):
            v[j] = v[j] - mpf(float(step_h[k])) - mpf(float(step_l[k]))
    v, viol, g = best
    slack = max([abs(g[j]) for j in range(len(v)) if v[j] == 0] or [mpf(0)])
    return v, viol, slack, means, scales


def main():
    ref_shim.install()
    np.random.seed(0)       # liblinear draws its coordinate order from NumPy's global generator: the same fixture every run
    from sklearn.exceptions import ConvergenceWarning
    from elfi.methods.classifier import LogisticRegression
    out = {}
    nc = len(R.CASES)
    coef = {k: np.zeros((nc, 64)) for k in ('truth', 'ref_default', 'ref_tight')}
    icpt = {k: np.zeros(nc) for k in coef}
    lr = {k: np.zeros(nc) for k in coef}
    support = np.zeros((nc, 65), dtype=bool)
    e_default, e_tight, kkt_tight, kkt_truth, slack_all = (np.zeros(nc) for _ in range(5))
    n_iter_tight = np.zeros(nc, dtype=np.int64)
    for ci, case in enumerate(R.CASES):
        X, M, obs, C = R.make_case(ci)
        m = X.shape[1]
        Xy = np.vstack([X, M])
        y = np.concatenate([np.ones(len(X)), -np.ones(len(M))])
        fits = {}
        for name, cfg in (('ref_default', None), ('ref_tight', dict(TIGHT))):
            if C != 1.0:
                cfg = dict(cfg or {'penalty': 'l1', 'solver': 'liblinear'}, C=C)
            clf = LogisticRegression(config=cfg)
            with warnings.catch_warnings():
                # the shipped default may stop at its 100 iterations; the tight fit must converge
                warnings.simplefilter('error' if name == 'ref_tight' else 'ignore', ConvergenceWarning)
                clf.fit(Xy, y)
            with np.errstate(all='ignore'):
                value = clf.predict_log_likelihood_ratio(obs)[0]
            fits[name] = clf
            coef[name][ci, :m] = clf.model.coef_[0]
            icpt[name][ci] = clf.model.intercept_[0]
            lr[name][ci] = value
        tight = fits['ref_tight']
        n_iter_tight[ci] = tight.model.n_iter_[0]
        v0 = np.concatenate([tight.model.coef_[0], tight.model.intercept_])
        Zt, yt = R.design(X, M, tight.scaler.mean_, tight.scaler.scale_)
        kkt_tight[ci] = R.violation(v0, Zt, yt, C)
        v, viol, slack, means, scales = polish(X, M, C, v0)
        kkt_truth[ci], slack_all[ci] = float(viol), float(slack)
        t = v[m] + mp.fsum(v[j] * (mpf(float(obs[0, j])) - means[j]) / scales[j] for j in range(m))
        coef['truth'][ci, :m] = [float(x) for x in v[:m]]
        icpt['truth'][ci] = float(v[m])
        lr['truth'][ci] = float(t)
        support[ci, :m] = [x != 0 for x in v[:m]]
        support[ci, 64] = v[m] != 0
        if slack > 1 - mpf('1e-3'):
            raise SystemExit('case %d: a zero coordinate has |g| = %s; change the seed' % (ci, mp.nstr(slack, 8)))
        if not np.array_equal(v0 != 0, np.array([x != 0 for x in v])):
            raise SystemExit('case %d: truth and ref_tight differ in support; change the seed' % ci)
        for name, e in (('ref_default', e_default), ('ref_tight', e_tight)):
            err = [abs(mpf(float(lr[name][ci])) - t), abs(mpf(float(icpt[name][ci])) - v[m])]
            err += [abs(mpf(float(coef[name][ci, j])) - v[j]) for j in range(m)]
            e[ci] = float(max(err))
        rm, rs = R.scaler(X, M)
        print('case %2d n=%d nm=%d m=%d C=%g  support %d of %d  log ratio % .15g  e_default %.2e  e_tight %.2e  kkt_tight '
              '%.2e  kkt_truth %.1e  slack %.4f  n_iter %d  scaler-vs-sklearn %.1e'
              % (ci, len(X), len(M), m, C, support[ci].sum(), m + 1, lr['truth'][ci], e_default[ci], e_tight[ci],
                 kkt_tight[ci], kkt_truth[ci], slack_all[ci], n_iter_tight[ci],
                 max(np.abs(rm - tight.scaler.mean_).max(), np.abs(rs - tight.scaler.scale_).max())), flush=True)
    out.update(cases=np.array(R.CASES, dtype=float), support=support, e_default=e_default, e_tight=e_tight,
               kkt_tight=kkt_tight, kkt_truth=kkt_truth, slack=slack_all, n_iter_tight=n_iter_tight)
    for k in coef:
        out[k + '_coef'], out[k + '_intercept'], out[k + '_logratio'] = coef[k], icpt[k], lr[k]
    path = os.path.join(ROOT, 'tests', 'golden', 'logratio.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
