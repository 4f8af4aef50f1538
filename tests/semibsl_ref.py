"""NumPy/SciPy statement of the semiparametric synthetic likelihood the device kernels compute (csrc/semibsl.hip), written
from the formulas (An, Nott & Drovandi 2020), and the recipe of the test cases.

For n rows x m columns X, observed y and an optional Warton penalty l:
  KDE        h_j = (3 n / 4)^(-1/5) std_j (ddof 1), z_ij = (y_j - x_ij) / h_j,
             logpdf_j = logsumexp_i(-z_ij^2 / 2) - log n - log h_j - log(2 pi) / 2,  u_j = min(1, mean_i Phi(z_ij))
  score      eta_j = Phi^-1(u_j); an infinite one gives -inf
  rank corr  r_ij the 1-based rank of x_ij within its column (ties: the average rank), q_ij = Phi^-1(r_ij / (n + 1)),
             rho_ab = sum_i q_ia q_ib / sum_{i=1..n} Phi^-1(i / (n + 1))^2, rho_aa = 1
  shrinkage  rho <- (1 - l) rho + l I
  loglik     -(log|rho| + eta^T rho^-1 eta - eta^T eta) / 2 + sum_j logpdf_j
A column without spread, a matrix without a Cholesky factor, two rows with more than one column: -inf (the device's rules).
"""
import math

import numpy as np
from scipy.linalg import cholesky, solve_triangular
from scipy.special import logsumexp, ndtr, ndtri

import synlik_ref

# (seed, n, m, correlation of neighbouring columns, largest column scale): the fixture cases of tests/golden/semibsl.npz
CASES = [(31, 5, 1, 0.0, 1.0), (32, 100, 2, 0.5, 1.0), (33, 33, 15, 0.6, 4.0), (34, 40, 16, 0.95, 3.0),
         (35, 257, 17, 0.7, 8.0), (36, 500, 8, 0.9, 20.0), (37, 255, 33, 0.8, 5.0), (38, 300, 64, 0.8, 5.0),
         (39, 1000, 32, 0.9, 20.0)]
PENALTIES = [0.1, 0.4, 0.8]
CONFIGS = ['none', 'warton0', 'warton1', 'warton2']
TWO_VALUED = (4, 3)     # the tied twin of CASES[4] has column 3 quantised to two values
SCORE_TABLES = (5, 257, 1000)


def make_case(ci, tied=False):
    """(X, y) of CASES[ci] by synlik_ref's recipe; the tied twin has rows and y rounded to integers."""
    X, y, _, _ = synlik_ref.make_case(*CASES[ci])
    if tied:
        X, y = np.round(X), np.round(y)
        if ci == TWO_VALUED[0]:
            c = TWO_VALUED[1]
            X[:, c] = y[c] + np.where(X[:, c] > np.median(X[:, c]), 1.0, -1.0)
    return X, y


def config_kwargs(name):
    return {} if name == 'none' else dict(shrinkage='warton', penalty=PENALTIES[int(name[-1])])


def ranks(c):
    """1-based ranks, ties at the average rank (scipy.stats.rankdata's default), by counting."""
    c = np.asarray(c)
    lt = (c[None, :] < c[:, None]).sum(1)
    eq = (c[None, :] == c[:, None]).sum(1)
    return lt + (eq + 1) / 2.0


def parts(X, y):
    """(logpdf (m), u (m), rho (m, m) unshrunk, scores (n, m)) of one group."""
    n, m = X.shape
    with np.errstate(all='ignore'):
        h = (0.75 * n) ** (-0.2) * X.std(0, ddof=1)
        Z = (y[None, :] - X) / h
        logpdf = logsumexp(-0.5 * Z * Z, axis=0) - math.log(n) - np.log(h) - 0.5 * math.log(2 * math.pi)
        logpdf = np.where(h > 0, logpdf, -np.inf)
        u = np.minimum(1.0, ndtr(Z).mean(0))
    Q = ndtri(np.column_stack([ranks(X[:, j]) for j in range(m)]) / (n + 1))
    den = np.sum(ndtri(np.arange(1, n + 1) / (n + 1)) ** 2)
    rho = Q.T @ Q / den
    np.fill_diagonal(rho, 1.0)
    return logpdf, u, rho, Q


def loglik_from_parts(logpdf, u, rho, n, penalty=None):
    m = len(u)
    with np.errstate(all='ignore'):
        eta = ndtri(u)
    if not np.all(np.isfinite(eta)) or not np.all(np.isfinite(logpdf)) or not np.all(np.isfinite(rho)) or (n == 2 and m > 1):
        return -math.inf
    if penalty is not None:
        rho = (1.0 - penalty) * rho + penalty * np.eye(m)
    try:
        L = cholesky(rho, lower=True)
    except np.linalg.LinAlgError:
        return -math.inf
    z = solve_triangular(L, eta, lower=True)
    return -0.5 * (2.0 * np.log(np.diag(L)).sum() + (z @ z - eta @ eta)) + logpdf.sum()


def semi_loglik_ref(ssx, ssy, n_groups=1, shrinkage=None, penalty=None, prefixes=None, penalties=None):
    """(n_groups, K, P) log-likelihoods (K = len(prefixes) or 1, P = len(penalties) or 1)."""
    X = np.asarray(ssx, dtype=float)
    X = X.reshape(-1, X.shape[-1])
    y = np.asarray(ssy, dtype=float).reshape(-1)
    n = len(X) // n_groups
    pre = [n] if prefixes is None else list(prefixes)
    pens = [penalty if shrinkage == 'warton' else None] if penalties is None else list(penalties)
    out = np.empty((n_groups, len(pre), len(pens)))
    for g in range(n_groups):
        Xg = X[g * n:(g + 1) * n]
        for k, p in enumerate(pre):
            logpdf, u, rho, _ = parts(Xg[:p], y)
            for j, pen in enumerate(pens):
                out[g, k, j] = loglik_from_parts(logpdf, u, rho, p, pen)
    return out
