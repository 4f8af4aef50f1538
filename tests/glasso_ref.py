"""NumPy statement of the graphical lasso the device kernel solves (csrc/glasso.hip), and the recipe of the test cases.

    minimise over Theta   -log det Theta + tr(S Theta) + alpha sum_{i != j} |Theta_ij|,      W = Theta^-1

by column-wise coordinate descent in the most obvious loops, run until the KKT residual is <= kkt_tol max diag S:
    |W_ij - S_ij - alpha sign Theta_ij|   where Theta_ij != 0,
    max(|W_ij - S_ij| - alpha, 0)         where Theta_ij == 0,
    |W_ii - S_ii|.
The optimum is unique, so this converged answer is the yardstick (tests/golden/glasso.npz, scripts/make_golden_glasso.py).
"""
import math

import numpy as np

# (seed, n, m): n rows of AR(1)-correlated normals.  The last one has a rank-deficient covariance (n = m / 2) and is not
# recorded in the fixture ("Graphical-lasso shrinkage")
CASES = [(31, 3, 1), (32, 6, 2), (33, 51, 17), (34, 120, 40), (35, 192, 64), (36, 20, 40)]
FIXED_ALPHAS = [0.0, math.exp(-5.5), math.exp(-3.5), math.exp(-1.7)]
LOGLIK_ALPHAS = FIXED_ALPHAS[1:]


def make_case(seed, n, m):
    """(X (n, m), y (m), whitening (m, m)): plain RandomState draws, so a test regenerates the inputs."""
    rs = np.random.RandomState(seed)
    Z = rs.randn(n, m)
    X = np.empty((n, m))
    X[:, 0] = Z[:, 0]
    for j in range(1, m):
        X[:, j] = 0.6 * X[:, j - 1] + 0.8 * Z[:, j]
    scales = np.linspace(1.0, 2.0, m)
    loc = rs.uniform(-3, 3, m)
    X = X * scales + loc
    y = loc + 0.5 * scales * rs.randn(m)
    Wh = np.eye(m) + rs.randn(m, m) / (2 * math.sqrt(m))
    return X, y, Wh


def alphas_of(S):
    """The fixed penalties and 1.01 x the largest off-diagonal |S_ij| (the solution is diagonal from there on)."""
    off = np.abs(S - np.diag(np.diag(S)))
    return np.array(FIXED_ALPHAS + [1.01 * off.max() if len(S) > 1 else 1.0])


def kkt_residual(S, W, alpha):
    """The largest KKT violation with Theta = W^-1 by LAPACK (the Theta assembled from the columns satisfies the
    conditions by construction); an entry below 1e-9 sqrt(Theta_ii Theta_jj) counts as zero, which at a solution costs
    nothing: there |W_ij - S_ij| = alpha either way."""
    R = W - S
    Theta = np.linalg.inv(W)
    d = np.sqrt(np.abs(np.diag(Theta)))
    Theta = np.where(np.abs(Theta) > 1e-9 * np.outer(d, d), Theta, 0.0)
    off = ~np.eye(len(S), dtype=bool)
    res = np.where(Theta != 0, np.abs(R - alpha * np.sign(Theta)), np.maximum(np.abs(R) - alpha, 0.0))
    return max(np.abs(np.diag(R)).max(), res[off].max() if len(S) > 1 else 0.0)


def graphical_lasso_ref(S, alpha, kkt_tol=1e-13, max_sweeps=20000):
    """(W, Theta, sweeps, kkt residual / max diag S); sweeps is max_sweeps when the residual was not reached."""
    S = np.asarray(S, dtype=np.float64)
    m = len(S)
    top = np.diag(S).max()
    if alpha == 0 or m == 1:
        return S.copy(), np.linalg.inv(S), 0, 0.0
    W = 0.95 * S
    W[np.diag_indices(m)] = np.diag(S)
    Bc = np.zeros((m, m))
    Theta = np.zeros((m, m))
    inner = 1e-15 * top
    for sweep in range(1, max_sweeps + 1):
        for j in range(m):
            beta = Bc[j].copy()
            beta[j] = 0.0
            for _ in range(2000):
                step = 0.0
                for k in range(m):
                    if k == j:
                        continue
                    r = S[k, j] - (W[k] @ beta - W[k, k] * beta[k])
                    new = math.copysign(max(abs(r) - alpha, 0.0), r) / W[k, k]
                    step = max(step, abs(new - beta[k]) * W[k, k])
                    beta[k] = new
                if step <= inner:
                    break
            w12 = W @ beta
            keep = np.arange(m) != j
            W[keep, j] = w12[keep]
            W[j, keep] = w12[keep]
            Bc[j] = beta
            t22 = 1.0 / (W[j, j] - w12[keep] @ beta[keep])
            Theta[j, j] = t22
            Theta[:j, j] = Theta[j, :j] = -beta[:j] * t22
        res = kkt_residual(S, W, alpha) / top
        if res <= kkt_tol:
            return W, Theta, sweep, res
    return W, Theta, max_sweeps, res
