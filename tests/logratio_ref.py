"""NumPy statement of the logistic-regression ratio estimate the device kernel computes (csrc/logratio.hip), written from
the formulas, and the recipe of the test cases.

For n likelihood rows X (label +1) stacked on nm marginal rows M (label -1), N = n + nm:
  scaler      mean_j and the population variance var_j (ddof 0) of the N stacked rows; scale_j = sqrt(var_j), and 1 for a
              column scikit-learn's StandardScaler treats as constant: var <= N eps var + (N mean eps)^2
              (scikit-learn 1.7.2, sklearn/preprocessing/_data.py:76-89 `_is_constant_feature`, applied at :1046-1051);
              x~ = (x - mean) / scale.  The sums here are exact (math.fsum) and rounded once.
  objective   f(v) = ||v||_1 + C sum_i log(1 + exp(-y_i v.z_i)),  z_i = (x~_i, 1),  v = (w, b): liblinear's L1R_LR with
              fit_intercept=True, intercept_scaling=1 -- the intercept is a penalised coordinate
  gradient    g = C Z^T (-y o sigma(-y o Z v))   (of the smooth part)
  violation   max_j of |g_j + sign(v_j)| where v_j != 0 and max(|g_j| - 1, 0) where v_j == 0
  log ratio   t = w.x~_obs + b where expit(t) >= class_min, else log(class_min / (1 - class_min))
`fit` is a plain proximal-Newton solver of the same problem in NumPy (for smoke checks; the fixture's truth does not come
from it).
"""
import math

import numpy as np
from scipy.special import expit, log_expit

EPS = np.finfo(np.float64).eps

# (seed, n, nm, m, sep, C): likelihood rows randn(n, m) + sep against marginal rows 1.3 randn(nm, m); the fixture cases of
# tests/golden/logratio.npz.  The last one is the regime of BOLFIRE's first rounds on a two-summary model (parameters drawn
# from the prior, far from the observed data: nearly separable classes of 50 rows).  CONSTANT_COLUMN: that case has one
# column set to a constant in both blocks.
CASES = [(41, 5, 5, 8, 0.3, 1.0), (42, 10, 10, 2, 0.5, 1.0), (43, 33, 33, 7, 0.2, 1.0), (44, 100, 100, 16, 0.05, 0.05),
         (45, 257, 257, 63, 0.2, 1.0), (46, 64, 64, 3, 3.0, 1.0), (47, 20, 20, 4, 6.0, 1.0), (48, 1000, 1000, 32, 0.1, 1.0),
         (49, 300, 300, 64, 0.2, 1.0), (50, 70, 45, 5, 0.4, 1.0), (51, 40, 40, 1, 0.8, 1.0), (52, 50, 50, 2, 3.0, 1.0)]
CONSTANT_COLUMN = (2, 4, 2.5)     # (case index, column, value)


def make_case(ci):
    """(X (n, m), M (nm, m), observed (1, m), C) of CASES[ci]."""
    seed, n, nm, m, sep, C = CASES[ci]
    rs = np.random.RandomState(seed)
    X = rs.randn(n, m) + sep
    M = 1.3 * rs.randn(nm, m)
    obs = rs.randn(1, m) + sep
    if ci == CONSTANT_COLUMN[0]:
        X[:, CONSTANT_COLUMN[1]] = CONSTANT_COLUMN[2]
        M[:, CONSTANT_COLUMN[1]] = CONSTANT_COLUMN[2]
    return X, M, obs, C


def scaler(X, M):
    """(mean (m), scale (m)) of the stacked rows."""
    Z = np.vstack([X, M])
    N, m = Z.shape
    mean = np.array([math.fsum(Z[:, j]) / N for j in range(m)])
    var = np.array([math.fsum((Z[:, j] - mean[j]) ** 2) / N for j in range(m)])
    constant = var <= N * EPS * var + (N * mean * EPS) ** 2
    scale = np.sqrt(var)
    scale[constant] = 1.0
    return mean, scale


def design(X, M, mean=None, scale=None):
    """(Z (N, m + 1) standardised rows with the column of ones, y (N))."""
    if mean is None:
        mean, scale = scaler(X, M)
    S = (np.vstack([X, M]) - mean) / scale
    Z = np.column_stack([S, np.ones(len(S))])
    y = np.concatenate([np.ones(len(X)), -np.ones(len(M))])
    return Z, y


def objective(v, Z, y, C):
    return np.abs(v).sum() - C * log_expit(y * (Z @ v)).sum()


def gradient(v, Z, y, C):
    return C * (Z.T @ (-y * expit(-y * (Z @ v))))


def violation(v, Z, y, C):
    g = gradient(v, Z, y, C)
    return float(np.max(np.where(v != 0, np.abs(g + np.sign(v)), np.maximum(np.abs(g) - 1.0, 0.0))))


def log_ratio_at(v, obs, mean, scale, class_min=0.0):
    t = ((np.atleast_2d(obs) - mean) / scale) @ v[:-1] + v[-1]
    if class_min > 0:
        t = np.where(expit(t) >= class_min, t, math.log(class_min / (1.0 - class_min)))
    return t


def _cd(H, g, v, tol, max_sweeps=2000):
    """Coordinate descent with soft-thresholding on  g.d + d.H d / 2 + ||v + d||_1; returns v + d."""
    u = v.copy()
    Hd = np.zeros_like(v)
    for _ in range(max_sweeps):
        worst = 0.0
        for j in range(len(v)):
            a, b, c = H[j, j], g[j] + Hd[j], u[j]
            worst = max(worst, abs(b + math.copysign(1.0, c)) if c != 0 else max(abs(b) - 1.0, 0.0))
            if b + 1.0 <= a * c:
                new = c - (b + 1.0) / a
            elif b - 1.0 >= a * c:
                new = c - (b - 1.0) / a
            else:
                new = 0.0
            if new != c:
                Hd += (new - c) * H[:, j]
                u[j] = new
        if worst <= tol:
            break
    return u


def fit(X, M, C=1.0, tol=1e-10, max_iter=100):
    """(v (m + 1), n_iter, converged) by proximal Newton: quadratic model, coordinate descent, backtracking."""
    Z, y = design(X, M)
    v = np.zeros(Z.shape[1])
    for it in range(max_iter + 1):
        p = expit(-y * (Z @ v))
        g = C * (Z.T @ (-y * p))
        viol = float(np.max(np.where(v != 0, np.abs(g + np.sign(v)), np.maximum(np.abs(g) - 1.0, 0.0))))
        if viol <= tol:
            return v, it, True
        if it == max_iter:
            break
        H = C * (Z.T * (p * (1.0 - p))) @ Z
        H[np.diag_indices_from(H)] += 1e-12
        u = _cd(H, g, v, min(0.1, viol) * viol * 0.1)
        d = u - v
        delta = g @ d + np.abs(u).sum() - np.abs(v).sum()
        f0 = objective(v, Z, y, C)
        lam = 1.0
        for _ in range(40):
            cand = u if lam == 1.0 else v + lam * d
            if objective(cand, Z, y, C) - f0 <= 0.01 * lam * delta + 64 * EPS * abs(f0):
                break
            lam *= 0.5
        else:
            break
        v = cand
    return v, max_iter, False
