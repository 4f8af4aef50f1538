"""NumPy statement of the KLIEP density-ratio fit the device kernels compute (csrc/kliep.hip), written from the formulas
(Sugiyama et al. 2008, as elfi/methods/density_ratio_estimation.py applies them), and the recipe of the test cases.

For numerator rows x (Nx, d), denominator rows y (Ny, d), a scale sigma and n basis functions centred at theta = x[:n]:
  basis      A_ij = exp(-0.5 |x_i - theta_j|^2 / sigma / sigma),  b_j = sum_t exp(-0.5 |theta_j - y_t|^2 / sigma / sigma) wy_t
             (wy normalised), b_normalized = b / (b . b)
  rows       row i is non-null when some A_ij > 1e-64; its filtered index is the number of non-null rows in front of it;
             fold f holds the filtered indices np.array_split(arange(L), F)[f]
  iteration  alpha = 1 / n; prev = A alpha over ALL rows; step i = 0 .. max_iter - 1:
               alpha += epsilon A_tr^T (w_tr / (A_tr alpha))           (training rows: non-null, not held out)
               alpha = max(0, alpha + (1 - b . alpha) b_normalized);  alpha /= b . alpha
               if i % interval == 0: t = A alpha over all rows; stop when |t - prev|_2 < abs_tol, else prev = t
  outputs    alpha, w = A alpha, the index i at which the loop ended; per held-out fold the weighted mean of log w over
             its rows, lcv = the mean over the folds (+inf when no row is non-null)
The full fit takes the caller's weights as they are, the fold fits and the scores the normalised ones.
"""
import math

import numpy as np

NULL_LEVEL = 1e-64
DEFAULTS = dict(n=100, epsilon=0.1, max_iter=500, abs_tol=0.01, interval=20)
SMC = dict(n=100, epsilon=0.001, max_iter=200, abs_tol=0.01, interval=20)      # AdaptiveThresholdSMC's estimator

# the fixture cases of tests/golden/kliep.npz: shapes, the scale, the iteration's settings, and how the weights are made
# ('none': no weights given, 'random': uniform(0.5, 1.5), 'zeros': random with every 5th entry 0)
CASES = [
    dict(seed=41, Nx=5, Ny=5, d=1, sigma=1.0, weights='none', **dict(DEFAULTS, n=5, interval=1)),
    dict(seed=3042, Nx=157, Ny=211, d=3, sigma=1.7, weights='random', far_row=120,
         **dict(DEFAULTS, n=37, interval=7, max_iter=120)),
    dict(seed=43, Nx=300, Ny=300, d=2, sigma=None, weights='random', **SMC),
    dict(seed=44, Nx=500, Ny=500, d=3, sigma=None, weights='random', **SMC),
    dict(seed=45, Nx=257, Ny=64, d=5, sigma=2.0, weights='zeros', **dict(DEFAULTS, n=64)),
    dict(seed=46, Nx=1000, Ny=500, d=8, sigma=3.0, weights='random', **dict(DEFAULTS, n=256)),
    dict(seed=47, Nx=64, Ny=50, d=2, sigma=1.2, weights='random', **dict(DEFAULTS, n=16, abs_tol=1e3)),
]
SEED_STEP = 1000            # the recording script moves a case's seed on by this much until its conditions hold
CV_CASE = 1
CV_SIGMAS = [10.0, 1.0, 0.1]
CV_FOLD = 5
SPREAD_X, SPREAD_Y, SHIFT_Y = 1.0, 1.5, 0.3


def smc_sigma(s1=SPREAD_X, s2=SPREAD_Y):
    """The scale AdaptiveThresholdSMC hands to the estimator for populations of these spreads."""
    return s1 * s2 / math.sqrt(abs(s1 ** 2 - s2 ** 2))


def make_case(ci, seed=None):
    """dict(x, y, weights_x, weights_y (None or arrays), sigma, and the keywords n, epsilon, max_iter, abs_tol,
    interval) of CASES[ci]; `seed` replaces the recipe's (the fixture records the one that was used)."""
    c = CASES[ci]
    rs = np.random.RandomState(c['seed'] if seed is None else int(seed))
    x = rs.randn(c['Nx'], c['d']) * SPREAD_X
    y = rs.randn(c['Ny'], c['d']) * SPREAD_Y + SHIFT_Y
    wx = wy = None
    if c['weights'] != 'none':
        wx, wy = rs.uniform(0.5, 1.5, c['Nx']), rs.uniform(0.5, 1.5, c['Ny'])
    if c['weights'] == 'zeros':
        wx[3::5] = 0.0
        wy[1::5] = 0.0
    if 'far_row' in c:
        x[c['far_row']] = 80.0
    out = dict(x=x, y=y, weights_x=wx, weights_y=wy, sigma=c['sigma'] if c['sigma'] is not None else smc_sigma())
    out.update({k: c[k] for k in ('n', 'epsilon', 'max_iter', 'abs_tol', 'interval')})
    return out


def fit_kwargs(case):
    return dict(n=case['n'], epsilon=case['epsilon'], max_iter=case['max_iter'], abs_tol=case['abs_tol'],
                conv_check_interval=case['interval'])


def basis(points, centres, sigma):
    """(len(points), len(centres)) Gaussian basis values; the exponent is divided by sigma twice."""
    diff = points[:, None, :] - centres[None, :, :]
    with np.errstate(all='ignore'):
        return np.exp(-0.5 * np.sum(diff * diff, axis=2) / sigma / sigma)


def fold_of_rows(non_null, F):
    """(Nx) the fold of every row (-1: a null row) and L, the number of non-null rows."""
    L = int(np.count_nonzero(non_null))
    fold = np.full(len(non_null), -1)
    parts = np.array_split(np.arange(L), F) if F > 0 else []
    of_filtered = np.empty(L, dtype=int)
    for f, idx in enumerate(parts):
        of_filtered[idx] = f
    if F > 0:
        fold[non_null] = of_filtered
    return fold, L


def iterate(A_all, A_tr, w_tr, b, bn, n, epsilon, max_iter, abs_tol, interval, trace=None):
    """(alpha, index at which the loop ended); `trace` collects the norm of every convergence check."""
    with np.errstate(all='ignore'):
        alpha = np.full(n, 1.0 / n)
        prev = A_all @ alpha
        i = 0
        for i in range(max_iter):
            alpha = alpha + epsilon * (A_tr.T @ (w_tr / (A_tr @ alpha)))
            alpha = np.maximum(0, alpha + (1 - b @ alpha) * bn)
            alpha = alpha / (b @ alpha)
            if i % interval == 0:
                t = A_all @ alpha
                diff = np.sqrt(np.sum((t - prev) ** 2))
                if trace is not None:
                    trace.append(float(diff))
                if diff < abs_tol:
                    break
                prev = t
    return alpha, i


def kliep_fit_ref(x, y, weights_x=None, weights_y=None, sigma=1.0, n=100, epsilon=0.1, max_iter=500, abs_tol=0.01,
                  conv_check_interval=20, fold=0, traces=None):
    """dict(alpha (S, n), w (S, Nx), iters (S)[, scores (S, F), lcv (S)]) for the scales `sigma` (a float or a list)."""
    x = np.asarray(x, dtype=float).reshape(len(x), -1)
    y = np.asarray(y, dtype=float).reshape(len(y), -1)
    sigmas = np.atleast_1d(np.asarray(sigma, dtype=float))
    Nx = len(x)
    wx = np.ones(Nx) if weights_x is None else np.asarray(weights_x, dtype=float)
    wy = np.ones(len(y)) if weights_y is None else np.asarray(weights_y, dtype=float)
    with np.errstate(all='ignore'):
        wxn, wyn = wx / np.sum(wx), wy / np.sum(wy)
    theta = x[:n]
    S, F = len(sigmas), int(fold)
    out = dict(alpha=np.empty((S, n)), w=np.empty((S, Nx)), iters=np.empty(S, dtype=np.int64))
    if F > 0:
        out.update(scores=np.full((S, F), np.nan), lcv=np.empty(S))
    for s, sg in enumerate(sigmas):
        A = basis(x, theta, sg)
        with np.errstate(all='ignore'):
            b = basis(theta, y, sg) @ wyn
            bn = b / (b @ b)
        non_null = np.any(A > NULL_LEVEL, axis=1)
        tr = [] if traces is not None else None
        alpha, it = iterate(A, A[non_null], wx[non_null], b, bn, n, epsilon, max_iter, abs_tol, conv_check_interval, tr)
        if traces is not None:
            traces.append(tr)
        out['alpha'][s], out['w'][s], out['iters'][s] = alpha, A @ alpha, it
        if F > 0:
            fold_of, L = fold_of_rows(non_null, F)
            for f in range(F):
                train, held = non_null & (fold_of != f), fold_of == f
                a_f, _ = iterate(A, A[train], wxn[train], b, bn, n, epsilon, max_iter, abs_tol, conv_check_interval)
                with np.errstate(all='ignore'):
                    out['scores'][s, f] = np.sum(np.log(A[held] @ a_f) * wxn[held]) / np.sum(wxn[held])
            out['lcv'][s] = np.mean(out['scores'][s]) if L > 0 else np.inf
    return out


def kliep_ratio_ref(points, centres, alpha, sigma):
    points = np.atleast_2d(np.asarray(points, dtype=float))
    return basis(points, np.asarray(centres, dtype=float), float(sigma)) @ np.asarray(alpha, dtype=float)


def rel_err(got, hi, lo):
    """max |got - truth| as a fraction of max |truth|, truth = hi + lo."""
    return float(np.max(np.abs((np.asarray(got) - hi) - lo)) / np.max(np.abs(hi)))
