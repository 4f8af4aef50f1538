"""Writes tests/golden/glasso.npz: the cases of tests/glasso_ref.py, the converged NumPy statement's W and
log-likelihoods, and the bound per case -- 16 x the disagreement between that statement and scikit-learn's
graphical_lasso at the tightest tol = enet_tol at which it converges without a warning, floored at the standard
synthetic likelihood's bound (16 x e_ref of tests/golden/synlik.npz) for the nearest m.  Also recorded, for DESIGN.md:
the disagreement itself and how far the reference at its own settings (tol 1e-4, max_iter 200) is from the converged answer.

    python scripts/make_golden_glasso.py        (CPU only; minutes: the statement is plain Python loops)
"""
import os
import sys
import warnings
from multiprocessing import Pool

import numpy as np
from scipy.stats import multivariate_normal
from sklearn.covariance import graphical_lasso

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import glasso_ref as R  # noqa: E402
import synlik_ref as SR  # noqa: E402

N_RECORDED = 5      # the rank-deficient case R.CASES[5] is not recorded


def sym_cov(X):
    S = np.atleast_2d(np.cov(X, rowvar=False))
    return np.tril(S) + np.tril(S, -1).T


def matrix_of(ci, form):
    """(S the solve runs on, mean, y) of case ci in one of the three forms."""
    X, y, Wh = R.make_case(*R.CASES[ci])
    if form == 'whitening':
        X, y = X @ Wh.T, Wh @ y
    S = sym_cov(X)
    if form == 'standardise':
        sd = np.sqrt(np.diag(S))
        S = S / np.outer(sd, sd)
    return S, X.mean(0), y


def sklearn_tight(S, alpha):
    for tol in 10.0 ** np.arange(-13, -3):
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            try:
                return graphical_lasso(S, alpha=alpha, tol=tol, enet_tol=tol, max_iter=100000)[0]
            except (Warning, FloatingPointError):
                continue
    raise RuntimeError('scikit-learn did not converge')


def solve(task):
    ci, form, alpha = task
    S, mean, y = matrix_of(ci, form)
    W, _, sweeps, res = R.graphical_lasso_ref(S, alpha)
    assert res <= 1e-13, (task, res)
    if alpha == 0 or len(S) == 1:
        Wsk = Wown = S
    else:
        Wsk = sklearn_tight(S, alpha)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            Wown = graphical_lasso(S, alpha=alpha, max_iter=200)[0]
    ll = [multivariate_normal.logpdf(y, mean=mean, cov=M, allow_singular=False) for M in (W, Wsk, Wown)]
    logdet = [np.linalg.slogdet(M)[1] for M in (W, Wown)]
    top = np.diag(S).max()
    return dict(task=task, W=W, sweeps=sweeps, ll=ll[0], dis_W=np.abs(W - Wsk).max() / top, dis_ll=abs(ll[0] - ll[1]),
                own_W=np.abs(W - Wown).max() / top, own_ll=abs(ll[0] - ll[2]), own_logdet=abs(logdet[0] - logdet[1]))


def floor_for(m, gold):
    ms = np.array([c[2] for c in SR.CASES])
    near = ms[np.abs(ms - m).argmin()]
    return 16.0 * max(gold['e_ref'][i, 0] for i, c in enumerate(SR.CASES) if c[2] == near)


def main():
    syn = np.load(os.path.join(ROOT, 'tests', 'golden', 'synlik.npz'))
    tasks, alphas = [], []
    for ci in range(N_RECORDED):
        a = R.alphas_of(matrix_of(ci, 'plain')[0])
        alphas.append(a)
        tasks += [(ci, 'plain', x) for x in a]
        tasks += [(ci, 'standardise', x) for x in R.LOGLIK_ALPHAS]
    tasks += [(2, 'whitening', x) for x in R.LOGLIK_ALPHAS]
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        done = {r['task']: r for r in pool.imap_unordered(solve, tasks)}
    out = dict(cases=np.array(R.CASES[:N_RECORDED]), alphas=np.array(alphas))
    nP, nL = len(alphas[0]), len(R.LOGLIK_ALPHAS)
    for key in ('bound_W', 'dis_W', 'own_W', 'own_logdet', 'sweeps'):
        out[key] = np.zeros((N_RECORDED, nP))
    for form in ('plain', 'standardise', 'whitening'):
        for key in ('ll_', 'bound_ll_', 'dis_ll_', 'own_ll_'):
            out[key + form] = np.full((N_RECORDED, nL), np.nan)
    for ci in range(N_RECORDED):
        m = R.CASES[ci][2]
        fl = floor_for(m, syn)
        out['S_%d' % ci] = matrix_of(ci, 'plain')[0]
        out['W_%d' % ci] = np.stack([done[(ci, 'plain', x)]['W'] for x in alphas[ci]])
        for p, x in enumerate(alphas[ci]):
            r = done[(ci, 'plain', x)]
            out['bound_W'][ci, p] = max(16.0 * r['dis_W'], fl)
            for key in ('dis_W', 'own_W', 'own_logdet', 'sweeps'):
                out[key][ci, p] = r[key]
        for form in ('plain', 'standardise', 'whitening'):
            for p, x in enumerate(R.LOGLIK_ALPHAS):
                r = done.get((ci, form, x))
                if r is None:
                    continue
                out['ll_' + form][ci, p] = r['ll']
                out['bound_ll_' + form][ci, p] = max(16.0 * r['dis_ll'], fl)
                out['dis_ll_' + form][ci, p] = r['dis_ll']
                out['own_ll_' + form][ci, p] = r['own_ll']
    np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', 'glasso.npz'), **out)
    np.set_printoptions(precision=2, linewidth=160)
    for key in ('sweeps', 'dis_W', 'bound_W', 'own_W', 'own_logdet', 'dis_ll_plain', 'bound_ll_plain', 'own_ll_plain',
                'bound_ll_standardise', 'bound_ll_whitening'):
        print(key, out[key], sep='\n')


if __name__ == '__main__':
    main()
