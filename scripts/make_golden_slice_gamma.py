"""Records tests/golden/slice_gamma.npz from the reference ELFI's own gamma slice samplers (run where the reference is
installed; oracle/ref_shim.py makes it importable).  CPU only.

For every case of CASES it stores, under the prefix c<k>_:
  y, mean, cov, gamma, loglik, adj, tau, w, max_iter   the inputs,
  draws        the buffer of doubles in [0, 1) the samplers consume (what was used and a few more),
  ref_gamma, ref_loglik, used, evals   what slice_gamma_mean / slice_gamma_variance of the reference return when their
               RandomState hands out that buffer (tests/slice_gamma_ref.py: BufferedRandomState), and their counts,
  truth_hi, truth_lo   the returned log-likelihood of the statement (tests/slice_gamma_ref.py) run in 50-digit mpmath on
               the same inputs and draws, as a double-double,
  margin       the smallest relative margin |a - b| / (1 + |b|) over the comparisons of that run.
Only cases with settled decisions are recorded: the reference, the float64 statement and the truth consume the same
number of draws and make the same number of evaluations, and the truth's margin is at least 1e-6; the seed of a case goes
up until that holds.  bound_m / bound: per m, 16 x the largest |reference - truth| over the recorded cases with that m
(the convention of the synthetic likelihoods).

Two 30-sample R-BSL chains of the reference on its MA2 model (variance and mean adjustment, the reference's likelihood
and samplers) are stored as chain_<adjustment>_params / _logpost / _gamma.

    python scripts/make_golden_slice_gamma.py
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import ref_shim  # noqa: E402
import slice_gamma_ref as S  # noqa: E402

mp.mp.dps = 50
mpf = mp.mpf

SHAPES = (1, 2, 15, 16, 17, 33, 64)
# (kind, adjustment, m, w, max_iter, first seed)
CASES = []
for _m in SHAPES:
    for _adj in (S.MEAN, S.VARIANCE):
        CASES.append(('base', _adj, _m, 1.0, 1000, 100 * _m + _adj))
        if _m <= 17:
            CASES.append(('base', _adj, _m, 1.0, 1000, 100 * _m + 50 + _adj))
for _adj in (S.MEAN, S.VARIANCE):
    CASES.append(('corr95', _adj, 16, 1.0, 1000, 7000 + _adj))
    CASES.append(('far8', _adj, 15, 1.0, 1000, 7100 + _adj))
    CASES.append(('base', _adj, 2, 0.05, 1000, 7200 + _adj))
    for _it in (0, 1, 2):
        CASES.append(('base', _adj, 15, 1.0, _it, 7300 + 10 * _it + _adj))
CASES.append(('gamma0', S.VARIANCE, 16, 1.0, 1000, 7400))
TAU = 0.5
SPARE_DRAWS = 8
CHAIN = dict(n=30, round=100, seed=3)


def make_inputs(kind, adj, m, seed):
    """A chain's state as BSL keeps it: the moments of n simulated summary rows, an observation, gamma and its
    log-likelihood."""
    rs = np.random.RandomState(seed)
    n = 4 * m + 20
    if kind == 'corr95':
        C = np.full((m, m), 0.95) + 0.05 * np.eye(m)
        X = rs.randn(n, m) @ np.linalg.cholesky(C).T
    else:
        X = rs.randn(n, m) @ (np.eye(m) + 0.3 * rs.randn(m, m) / np.sqrt(m)) * (0.5 + rs.rand(m))
    mean = X.mean(0) + rs.randn(m)
    cov = np.atleast_2d(np.cov(X, rowvar=False))
    std = np.sqrt(np.diag(cov))
    y = mean + std * rs.randn(m)
    if kind == 'far8':
        y[min(3, m - 1)] = mean[min(3, m - 1)] + 8.0 * std[min(3, m - 1)]
    if adj == S.MEAN:
        gamma = rs.laplace(0.0, 0.3, m)
        loglik = S.F64.logpdf(list(y - (mean + std * gamma)), cov.tolist())
    else:
        gamma = np.zeros(m) if kind == 'gamma0' else rs.exponential(TAU, m)
        loglik = S.F64.logpdf(list(y - mean), (cov + np.diag((std * gamma) ** 2)).tolist())
    return y, mean, cov, gamma, float(loglik)


class MP:
    """mpmath scalars; the log-density from a Cholesky factorisation, kept between calls while the matrix is the same
    object (the mean adjustment's covariance never changes)."""
    LOG_2PI = mp.log(2 * mp.pi)
    num = staticmethod(mpf)
    log = staticmethod(mp.log)
    sqrt = staticmethod(mp.sqrt)
    isfinite = staticmethod(mp.isfinite)
    _kept = (None, None)

    @staticmethod
    def _factor(cov):
        m = len(cov)
        L = [[mpf(0)] * m for _ in range(m)]
        for j in range(m):
            s = cov[j][j] - mp.fsum(L[j][k] * L[j][k] for k in range(j))
            if not s > 0:
                raise FloatingPointError('no Cholesky factor')
            L[j][j] = mp.sqrt(s)
            for i in range(j + 1, m):
                L[i][j] = (cov[i][j] - mp.fsum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
        return L

    @classmethod
    def logpdf(cls, resid, cov):
        if cls._kept[0] is not cov:
            cls._kept = (cov, cls._factor(cov))
        L = cls._kept[1]
        m = len(resid)
        z = []
        for i in range(m):
            z.append((resid[i] - mp.fsum(L[i][k] * z[k] for k in range(i))) / L[i][i])
        logdet = 2 * mp.fsum(mp.log(L[j][j]) for j in range(m))
        return -((m * cls.LOG_2PI + logdet) + mp.fsum(v * v for v in z)) / 2


def split(t):
    hi = float(t)
    return hi, float(t - mpf(hi))


def record_case(kind, adj, m, w, max_iter, seed, reference):
    while True:
        y, mean, cov, gamma, loglik = make_inputs(kind, adj, m, seed)
        draws = np.random.RandomState(seed + 1000003).random_sample(m * 64 + 4096)
        rs = S.BufferedRandomState(draws)
        counts = []
        orig = reference[adj].__globals__['ss'].multivariate_normal.logpdf

        def counted(*a, **k):
            counts.append(1)
            return orig(*a, **k)
        reference[adj].__globals__['ss'].multivariate_normal.logpdf = counted
        try:
            ref_gamma, ref_ll = reference[adj](y, loglik, gamma, mean, cov, tau=TAU, w=w, max_iter=max_iter, random_state=rs)
        finally:
            del reference[adj].__globals__['ss'].multivariate_normal.logpdf
        g64, ll64, used64, evals64, margin64 = S.slice_gamma(adj, y, mean, cov, gamma, loglik, TAU, w, max_iter, draws)
        ok = used64 == rs.used and evals64 == len(counts) and margin64 >= 1e-6 and np.array_equal(g64, ref_gamma)
        if ok:
            gt, llt, usedt, evalst, margint = S.slice_gamma(adj, y, mean, cov, gamma, loglik, TAU, w, max_iter, draws, ops=MP)
            ok = usedt == rs.used and evalst == len(counts) and margint >= 1e-6
        if ok:
            break
        print('   seed %d not settled, next' % seed, flush=True)
        seed += 1
    hi, lo = split(llt)
    e_ref = float(abs(mpf(float(ref_ll)) - llt))
    e_64 = float(abs(mpf(float(ll64)) - llt))
    e_gamma = max(float(abs(mpf(float(a)) - b)) for a, b in zip(ref_gamma, gt))
    print('%-7s adj %d m %2d w %.2f max_iter %4d seed %5d: used %4d evals %4d margin %.2e  |ref-truth| %.2e  '
          '|statement-truth| %.2e  |gamma-truth| %.1e' % (kind, adj, m, w, max_iter, seed, rs.used, len(counts), margint,
                                                           e_ref, e_64, e_gamma), flush=True)
    return dict(y=y, mean=mean, cov=cov, gamma=gamma, loglik=loglik, adj=adj, tau=TAU, w=w, max_iter=max_iter, seed=seed,
                draws=draws[:rs.used + SPARE_DRAWS].copy(), ref_gamma=np.asarray(ref_gamma, dtype=np.float64),
                ref_loglik=float(ref_ll), used=rs.used, evals=len(counts), truth_hi=hi, truth_lo=lo, margin=margint,
                e_ref=e_ref)


def main():
    elfi = ref_shim.install()
    import elfi.clients.native as native
    native.set_as_default()
    from elfi.examples import ma2
    from elfi.methods.bsl import pdf_methods as P
    from elfi.methods.bsl.slice_gamma_mean import slice_gamma_mean
    from elfi.methods.bsl.slice_gamma_variance import slice_gamma_variance
    reference = {S.MEAN: slice_gamma_mean, S.VARIANCE: slice_gamma_variance}
    out = {'n_cases': len(CASES), 'kinds': np.array([c[0] for c in CASES])}
    worst = {}
    for k, case in enumerate(CASES):
        rec = record_case(*case, reference=reference)
        for key, val in rec.items():
            out['c%d_%s' % (k, key)] = val
        worst[case[2]] = max(worst.get(case[2], 0.0), rec['e_ref'])
    ms = sorted(worst)
    out.update(bound_m=np.array(ms), bound=np.array([16.0 * worst[m] for m in ms]))
    for m in ms:
        print('m=%2d  max |reference - truth| %.3e  bound %.3e' % (m, worst[m], 16.0 * worst[m]))

    theta, feats = [0.6, 0.2], ['S1', 'S2']
    for adjustment in ('variance', 'mean'):
        bsl = elfi.BSL(ma2.get_model(seed_obs=4), CHAIN['round'], feature_names=feats,
                       likelihood=P.robust_likelihood(adjustment), seed=CHAIN['seed'])
        bsl.sample(CHAIN['n'], sigma_proposals=0.02 * np.eye(2), params0=theta, bar=False)
        out['chain_%s_params' % adjustment] = bsl.state['params'].copy()
        out['chain_%s_logpost' % adjustment] = bsl.state['logposterior'].copy()
        out['chain_%s_gamma' % adjustment] = bsl.state['gamma'].copy()
        moved = np.any(np.diff(bsl.state['params'], axis=0) != 0, axis=1)
        print('R-BSL chain (%s): %d of %d proposals accepted' % (adjustment, moved.sum(), CHAIN['n'] - 1))
    out.update(chain_n=CHAIN['n'], chain_round=CHAIN['round'], chain_seed=CHAIN['seed'])

    path = os.path.join(ROOT, 'tests', 'golden', 'slice_gamma.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
