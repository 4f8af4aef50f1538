"""The statement of the gamma slice samplers (include/elfihip.h: elfihip_slice_gamma) with the direct formulas: every
trial point is a full multivariate-normal log-density from a Cholesky factorisation of that trial's covariance.  The
control flow is the reference's (elfi/methods/bsl/slice_gamma_mean.py, slice_gamma_variance.py) line by line; the draws
come from a buffer of doubles in [0, 1).

The arithmetic is behind `ops`, so the same statement runs in float64 (F64, the default) and, for the golden file's truth,
in mpmath (scripts/make_golden_slice_gamma.py).  `slice_gamma` also reports the smallest relative margin
|a - b| / (1 + |b|) over all comparisons a < b / a > b it decided: a case whose margin is far above the rounding error of a
log-likelihood has the same decisions in every correct implementation."""
import math

import numpy as np

MEAN, VARIANCE = 0, 1
OK, OUT_OF_DRAWS, NONFINITE = 0, 1, 2


class OutOfDraws(Exception):
    """The draw buffer ended; args[0] is its length."""


class F64:
    """float64 scalars, sums in index order, the log-density from np.linalg.cholesky."""
    LOG_2PI = np.float64(math.log(2.0 * math.pi))

    @staticmethod
    def num(x):
        return np.float64(x)

    @staticmethod
    def log(x):
        return np.float64(math.log(x))

    @staticmethod
    def sqrt(x):
        return np.float64(math.sqrt(x))

    @staticmethod
    def isfinite(x):
        return bool(np.isfinite(x))

    @staticmethod
    def logpdf(resid, cov):
        """-1/2 (m log 2 pi + log det cov + resid' cov^-1 resid); cov a list of rows, lower triangle read."""
        C = np.tril(np.array(cov, dtype=np.float64))
        C = C + np.tril(C, -1).T
        L = np.linalg.cholesky(C)
        z = np.linalg.solve(L, np.array(resid, dtype=np.float64))
        logdet = np.float64(0.0)
        for j in range(len(resid)):
            logdet = logdet + np.float64(math.log(L[j, j]))
        quad = np.float64(0.0)
        for v in z:
            quad = quad + v * v
        return np.float64(-0.5) * ((len(resid) * F64.LOG_2PI + 2.0 * logdet) + quad)


def slice_gamma(adjustment, y, mean, cov, gamma, loglik, tau, w, max_iter, draws, ops=F64):
    """One sweep.  -> (gamma (list), ll_curr, used, evals, smallest margin).  OutOfDraws when `draws` ends."""
    m = len(gamma)
    num = ops.num
    y, mean = [num(v) for v in y], [num(v) for v in mean]
    cov = [[num(cov[i][j]) for j in range(m)] for i in range(m)]
    gam = [num(v) for v in gamma]
    tau, w = num(tau), num(w)
    std = [ops.sqrt(cov[i][i]) for i in range(m)]
    loglik = num(loglik)
    ll_curr = loglik
    state = {'used': 0, 'evals': 0, 'margin': float('inf')}
    rate = num(1) / tau
    log_tau = ops.log(tau)

    def draw():
        if state['used'] >= len(draws):
            raise OutOfDraws(len(draws))
        d = num(draws[state['used']])
        state['used'] += 1
        return d

    def total(terms):
        s = num(0)
        for t in terms:
            s = s + t
        return s

    def prior(g):
        if adjustment == MEAN:
            return m * ops.log(rate / 2) - rate * total(abs(v) for v in g)
        if any(v < 0 for v in g):
            return num('-inf')
        return total(-(v / tau) - log_tau for v in g)

    def lik(g):
        state['evals'] += 1
        if adjustment == MEAN:
            return ops.logpdf([y[i] - (mean[i] + std[i] * g[i]) for i in range(m)], cov)
        c = [row[:] for row in cov]
        for i in range(m):
            c[i][i] = c[i][i] + (std[i] * g[i]) * (std[i] * g[i])
        return ops.logpdf([y[i] - mean[i] for i in range(m)], c)

    def decide(a, b):
        rel = abs(a - b) / (1 + abs(b))
        state['margin'] = min(state['margin'], float(rel))

    def finite(v):
        if not ops.isfinite(v):
            raise FloatingPointError('a target that is not finite')
        return v

    for ii in range(m):
        e = -ops.log(num(1) - draw())
        g0 = gam[ii]
        target = finite((loglik + prior(gam)) - e)
        lower = g0 - w if adjustment == MEAN else num(0)
        upper = g0 + w
        trial = gam[:]
        if adjustment == MEAN:
            i = 0
            while i <= max_iter:
                trial[ii] = lower
                loglik = lik(trial)
                tx = finite(loglik + prior(trial))
                decide(tx, target)
                if tx < target:
                    break
                lower = lower - w
                i += 1
        i = 0
        while i <= max_iter:
            trial[ii] = upper
            loglik = lik(trial)
            tx = finite(loglik + prior(trial))
            decide(tx, target)
            if tx < target:
                break
            upper = upper + w
            i += 1
        i = 0
        while i < max_iter:
            prop = lower + (upper - lower) * draw()
            trial[ii] = prop
            loglik = lik(trial)
            tx = finite(loglik + prior(trial))
            decide(tx, target)
            if tx > target:
                gam = trial[:]
                ll_curr = loglik
                break
            decide(prop, g0)
            if prop < g0:
                lower = prop
            else:
                upper = prop
            i += 1
    return gam, ll_curr, state['used'], state['evals'], state['margin']


def slice_gamma_status(adjustment, y, mean, cov, gamma, loglik, tau, w, max_iter, draws):
    """The float64 statement with the device's outputs: (gamma (m), loglik, used, evals, status); NaN outputs with
    OUT_OF_DRAWS (used = len(draws)) and NONFINITE (the counts are not modelled: -1, or 0 where the factorisation fails
    before the first draw)."""
    m = len(gamma)
    try:
        g, ll, used, evals, _ = slice_gamma(adjustment, y, mean, cov, gamma, loglik, tau, w, max_iter, draws)
        return np.array(g, dtype=np.float64), float(ll), used, evals, OK
    except OutOfDraws:
        return np.full(m, np.nan), float('nan'), len(draws), -1, OUT_OF_DRAWS
    except np.linalg.LinAlgError:
        first = adjustment == MEAN or not np.any(np.asarray(gamma, dtype=np.float64)[1:])
        return np.full(m, np.nan), float('nan'), 0 if first else -1, 0 if first else -1, NONFINITE
    except FloatingPointError:
        return np.full(m, np.nan), float('nan'), -1, -1, NONFINITE


class BufferedRandomState(np.random.RandomState):
    """A RandomState whose exponential(1) and uniform(lower, upper) come from a buffer of doubles, by the formulas NumPy's
    legacy generator applies to the double random_sample() would return."""

    def __init__(self, draws):
        super().__init__(0)
        self.draws = np.asarray(draws, dtype=np.float64)
        self.used = 0

    def _next(self):
        if self.used >= self.draws.size:
            raise OutOfDraws(self.draws.size)
        d = self.draws[self.used]
        self.used += 1
        return d

    def exponential(self, scale=1.0, size=None):
        assert scale == 1 and size is None
        return -math.log(1.0 - self._next())

    def uniform(self, low=0.0, high=1.0, size=None):
        assert size is None
        return low + (high - low) * self._next()
