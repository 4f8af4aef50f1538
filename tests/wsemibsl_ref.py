"""NumPy/SciPy statement of the whitened semiparametric synthetic likelihood the device kernels compute
(csrc/wsemibsl.hip) and the recipe of the test cases.  For n rows x m columns X, observed y, a whitening matrix W (m, m)
and an optional Warton penalty l, with logpdf, u and the normal scores Q of semibsl_ref.parts:
  transform  T = Q W^T
  re-rank    q'_ij = Phi^-1(rank'_ij / (n + 1)), rank' the rank within T's column (ties: the average rank),
             rho_ab = sum_i q'_ia q'_ib / sum_{i=1..n} Phi^-1(i / (n + 1))^2, rho_aa = 1
  scale      C = cov(Q) (ddof 1), d_a = sqrt((W C W^T)_aa)
  shrinkage  rho <- (1 - l) rho + l I          (before the scaling)
  loglik     M = diag(d) rho diag(d), eta_w = W Phi^-1(u):  -(log|M| + eta_w^T M^-1 eta_w - eta_w^T eta_w) / 2 + sum_j logpdf_j
-inf: an infinite Phi^-1(u_j), a column without spread, a d_a that is not positive and finite, a matrix without a Cholesky
factor, a non-finite value, two rows with more than one column (the device's rules).
"""
import math

import numpy as np
from scipy.linalg import cholesky, solve_triangular
from scipy.special import ndtri

import semibsl_ref as S

CASES = [0, 1, 2, 3, 4, 6, 7]           # indices into semibsl_ref.CASES: 5x1, 100x2, 33x15, 40x16, 257x17, 255x33, 300x64
TIED = [2, 4]                           # the cases recorded with their tied twins too
CONFIGS = [None, 0.4]                   # no shrinkage, Warton 0.4
SEEDS = {1: 155}                        # a case whose seed differs from semibsl_ref's (see below)
MIN_GAP = 1e-9                          # the fixture's condition on the gaps within T's columns: rounding changes no rank


def variants():
    return [(ci, False) for ci in CASES] + [(ci, True) for ci in TIED]          # the fixture's order


def whitening_matrix(ci):
    """The reference's formula (estimate_whitening_matrix: standardise, covariance, eigendecomposition, diag(w^-1/2) v^T,
    8 decimals) on the normal scores of an independent draw of 4 m + 50 rows from the case's recipe with seed + 1000."""
    seed, _, m, corr, scale = S.CASES[ci]
    X, _, _, _ = S.synlik_ref.make_case(seed + 1000, 4 * m + 50, m, corr, scale)
    Q = np.atleast_2d(S.parts(X, X[0])[3])
    Q = (Q - Q.mean(0)) / Q.std(0)
    cov = np.atleast_2d(np.cov(Q, rowvar=False))
    w, v = np.linalg.eigh(cov)
    return np.round(np.diag(w ** -0.5) @ v.T, 8)


def make_case(ci, tied=False):
    """(X, y, W).  X and y are semibsl_ref.make_case's, except for the seeds of SEEDS: with two columns W's rows are
    c (1, 1) and c' (1, -1) whatever the draw, so rows whose scores are (a, b) and (b, a), or two rows with the same rank in
    both columns, are exact ties of T that rounding splits; 100 x 2 takes a seed without such rows."""
    if ci in SEEDS:
        assert not tied
        X, y = S.synlik_ref.make_case(SEEDS[ci], *S.CASES[ci][1:])[:2]
    else:
        X, y = S.make_case(ci, tied=tied)
    return X, y, whitening_matrix(ci)


def wparts(X, y, W):
    """(logpdf (m), u (m), rho (m, m) unshrunk, of the transformed scores, d (m), scores q' (n, m), T (n, m))."""
    n, m = X.shape
    logpdf, u, _, Q = S.parts(X, y)
    T = Q @ W.T
    Q2 = ndtri(np.column_stack([S.ranks(T[:, j]) for j in range(m)]) / (n + 1))
    den = np.sum(ndtri(np.arange(1, n + 1) / (n + 1)) ** 2)
    rho = Q2.T @ Q2 / den
    np.fill_diagonal(rho, 1.0)
    C = np.atleast_2d(np.cov(Q, rowvar=False))
    with np.errstate(all='ignore'):
        d = np.sqrt(np.diag(W @ C @ W.T))
    return logpdf, u, rho, d, Q2, T


def loglik_from_parts(logpdf, u, rho, d, W, n, penalty=None):
    m = len(u)
    with np.errstate(all='ignore'):
        eta = ndtri(u)
    finite = np.all(np.isfinite(eta)) and np.all(np.isfinite(logpdf)) and np.all(np.isfinite(rho))
    if not finite or (n == 2 and m > 1) or not np.all((d > 0) & np.isfinite(d)):
        return -math.inf
    if penalty is not None:
        rho = (1.0 - penalty) * rho + penalty * np.eye(m)
    ew = W @ eta
    try:
        L = cholesky(d[:, None] * rho * d[None, :], lower=True)
    except (np.linalg.LinAlgError, ValueError):
        return -math.inf
    z = solve_triangular(L, ew, lower=True)
    ll = -0.5 * (2.0 * np.log(np.diag(L)).sum() + (z @ z - ew @ ew)) + logpdf.sum()
    return ll if np.isfinite(ll) else -math.inf


def wsemi_loglik_ref(X, y, W, shrinkage=None, penalty=None):
    """The log-likelihood of one group."""
    logpdf, u, rho, d, _, _ = wparts(X, y, W)
    return loglik_from_parts(logpdf, u, rho, d, W, len(X), penalty if shrinkage == 'warton' else None)
