"""NumPy/SciPy statement of the Gaussian synthetic likelihoods the device kernel computes (csrc/synlik.hip), written
from the formulas, and the recipe of the synthetic test cases.

  standard   log N(y; mean, S), mean and S = the sample mean and the unbiased sample covariance of the n rows
             (Price et al. 2018); optionally S -> Warton's ridge estimator with the reference's eps inside both diagonal
             scalings: d = sqrt(diag(S) + 1e-5), R = S / (d d^T), S' = (g R + (1 - g) I) * (d d^T), g = 1 - penalty
  unbiased   Ghurye & Olkin (1969) as Price et al. use it:
             -d/2 log(2 pi) + log c(d, n-2) - log c(d, n-1) - d/2 log(1 - 1/n) - (n-d-2)/2 (log(n-1) + log|S|)
             + (n-d-3)/2 log|psi|,  psi = (n-1) S - (y - mean)(y - mean)^T / (1 - 1/n),
             log c(k, v) = -k v/2 log 2 - k (k-1)/4 log pi - sum_{x<k} lgamma((v - x)/2)
  mean       log N(y; mean + std * gamma, S)                     (Frazier & Drovandi 2021), std = sqrt(diag S)
  variance   log N(y; mean, S + diag((std * gamma)^2))
  whitening  rows -> rows W^T, y -> W y in front of everything.
A matrix that is not positive definite gives -inf.
"""
import math

import numpy as np
from scipy.linalg import cholesky, solve_triangular
from scipy.special import gammaln

# (seed, n, m, correlation of neighbouring columns, largest column scale): the fixture cases of tests/golden/synlik.npz
CASES = [(11, 100, 2, 0.5, 1.0), (12, 500, 8, 0.9, 20.0), (13, 2000, 20, 0.7, 10.0), (14, 5000, 32, 0.9, 20.0),
         (15, 300, 64, 0.8, 5.0), (16, 200, 40, 0.6, 8.0)]
PENALTIES = [0.1, 0.4, 0.8]
# configurations recorded for every case: name -> keywords of syn_loglik_ref / elfi_amd.syn_loglik
CONFIGS = ['standard', 'unbiased', 'mean', 'variance', 'whitening', 'warton0', 'warton1', 'warton2']


def make_case(seed, n, m, rho, smax):
    """Rows with AR(1)-correlated columns of scales 1 .. smax and offsets of several scales; y near the centre; a
    whitening matrix and an adjustment vector.  Plain RandomState draws, so a test regenerates the inputs."""
    rs = np.random.RandomState(seed)
    Z = rs.randn(n, m)
    X = np.empty((n, m))
    X[:, 0] = Z[:, 0]
    for j in range(1, m):
        X[:, j] = rho * X[:, j - 1] + math.sqrt(1 - rho * rho) * Z[:, j]
    scales = np.linspace(1.0, smax, m)
    loc = rs.uniform(-5, 5, m) * scales
    X = X * scales + loc
    y = loc + 0.5 * scales * rs.randn(m)
    W = np.eye(m) + rs.randn(m, m) / (2 * math.sqrt(m))
    gamma = 0.3 * np.abs(rs.randn(m))
    return X, y, W, gamma


def config_kwargs(name, W, gamma):
    if name == 'standard':
        return {}
    if name == 'unbiased':
        return dict(variant='unbiased')
    if name in ('mean', 'variance'):
        return dict(adjustment=name, gamma=gamma)
    if name == 'whitening':
        return dict(whitening=W)
    return dict(shrinkage='warton', penalty=PENALTIES[int(name[-1])])


def warton(S, penalty):
    g = 1.0 - penalty
    d = np.sqrt(np.diag(S) + 1e-5)
    dd = np.outer(d, d)
    return (g * (S / dd) + (1.0 - g) * np.eye(len(S))) * dd


def _chol_logdet_quad(S, v):
    """(log|S|, v^T S^-1 v), or None when S has no Cholesky factor."""
    if not np.all(np.isfinite(S)):
        return None
    try:
        L = cholesky(S, lower=True)
    except np.linalg.LinAlgError:
        return None
    z = solve_triangular(L, v, lower=True)
    return 2.0 * np.sum(np.log(np.diag(L))), float(z @ z)


def mvn_logpdf(y, mean, S):
    lq = _chol_logdet_quad(S, y - mean)
    if lq is None:
        return -math.inf
    return -0.5 * (len(y) * math.log(2 * math.pi) + lq[0] + lq[1])


def _logc(k, v):
    return -k * v / 2 * math.log(2) - k * (k - 1) / 4 * math.log(math.pi) - np.sum(gammaln([(v - x) / 2 for x in range(k)]))


def unbiased_loglik(y, mean, S, n):
    d = len(y)
    v = y - mean
    psi = (n - 1) * S - np.outer(v, v) / (1 - 1 / n)
    a, b = _chol_logdet_quad(S, v), _chol_logdet_quad(psi, v)
    if a is None or b is None or n <= d + 1:
        return -math.inf
    return (-0.5 * d * math.log(2 * math.pi) + _logc(d, n - 2) - _logc(d, n - 1) - 0.5 * d * math.log(1 - 1 / n)
            - 0.5 * (n - d - 2) * (math.log(n - 1) + a[0]) + 0.5 * (n - d - 3) * b[0])


def syn_loglik_ref(ssx, ssy, n_groups=1, variant='standard', shrinkage=None, penalty=None, whitening=None, gamma=None,
                   adjustment=None, prefixes=None, penalties=None, return_moments=False):
    """(n_groups, K, P) log-likelihoods (K = len(prefixes) or 1, P = len(penalties) or 1) [, mean, cov of full groups]."""
    X = np.asarray(ssx, dtype=float)
    X = X.reshape(-1, X.shape[-1])
    y = np.asarray(ssy, dtype=float).reshape(-1)
    if whitening is not None:
        X, y = X @ np.asarray(whitening).T, np.asarray(whitening) @ y
    n = len(X) // n_groups
    pre = [n] if prefixes is None else list(prefixes)
    pens = [penalty] if penalties is None else list(penalties)
    out = np.empty((n_groups, len(pre), len(pens)))
    means, covs = [], []
    for g in range(n_groups):
        Xg = X[g * n:(g + 1) * n]
        for k, p in enumerate(pre):
            mean = Xg[:p].mean(0)
            D = Xg[:p] - mean
            S = D.T @ D / (p - 1)
            if p == n:
                means.append(mean)
                covs.append(S)
            std = np.sqrt(np.diag(S))
            for j, pen in enumerate(pens):
                Sj = warton(S, pen) if shrinkage == 'warton' else S
                if variant == 'unbiased':
                    out[g, k, j] = unbiased_loglik(y, mean, Sj, p)
                elif adjustment == 'mean':
                    out[g, k, j] = mvn_logpdf(y, mean + std * gamma, Sj)
                elif adjustment == 'variance':
                    out[g, k, j] = mvn_logpdf(y, mean, Sj + np.diag((std * gamma) ** 2))
                else:
                    out[g, k, j] = mvn_logpdf(y, mean, Sj)
    if return_moments:
        return out, np.array(means), np.array(covs)
    return out
