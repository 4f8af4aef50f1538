"""NumPy statement of the two time-series example models the device runs (csrc/series.hip): ARCH(1) with its 2 + L +
L (L - 1) / 2 summaries and the M/G/1 queue with its log inter-departure times and quantiles.

Written from the models' definitions, draws handed in, in the operation order the device keeps: every function here is
pinned bit for bit to recorded runs of ELFI's own examples (tests/golden/series_models.npz, tests/test_series_models.py)
and the device kernels are pinned bit for bit to these functions (tests/test_series_models_gpu.py).  Sums along a row
are np.sum over a C-contiguous axis, i.e. NumPy's pairwise sum.
"""
from itertools import combinations

import numpy as np


# ---- ARCH(1) ------------------------------------------------------------------------------------------------------
def arch_noise_from_state(random_state, batch, n_obs):
    """The (batch, n_obs + 2) noise matrix from the draws ELFI's example makes, in its order: normal((batch, n_obs + 1))
    fills columns 0 .. n_obs (column 0 is drawn and never used), normal(batch) is the last column (the start e_0)."""
    xi = random_state.normal(size=(batch, n_obs + 1))
    e0 = random_state.normal(size=batch)
    return np.column_stack((xi, e0))


def arch_series(t1, t2, W):
    """y (batch, n_obs): e_0 = W[:, n_obs + 1]; e_i = W[:, i] sqrt(0.2 + t2 e_{i-1}^2); y_0 = 0, y_i = t1 y_{i-1} + e_i."""
    W = np.asarray(W, dtype=np.float64)
    batch, n_obs = W.shape[0], W.shape[1] - 2
    t1 = np.broadcast_to(np.asarray(t1, dtype=np.float64).reshape(-1), (batch,))
    t2 = np.broadcast_to(np.asarray(t2, dtype=np.float64).reshape(-1), (batch,))
    e = W[:, n_obs + 1].copy()
    y = np.zeros(batch)
    Y = np.empty((batch, n_obs))
    with np.errstate(all='ignore'):
        for i in range(1, n_obs + 1):
            e = W[:, i] * np.sqrt(0.2 + t2 * (e * e))
            y = t1 * y + e
            Y[:, i - 1] = y
    return Y


def arch_names(n_lags=5):
    lags = range(1, n_lags + 1)
    return ['MU', 'VAR'] + ['AC_%d' % i for i in lags] + ['PW_%d_%d' % ij for ij in combinations(lags, 2)]


def arch_summaries(Y, n_lags=5):
    """(batch, 2 + L + L (L - 1) / 2): mean, variance (ddof 1), the autocorrelations of the standardised series at lags
    1 .. L, and their pairwise products in itertools.combinations order."""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    n = Y.shape[1]
    with np.errstate(all='ignore'):
        mu = np.sum(Y, axis=1) / n
        d = Y - mu[:, None]
        var = np.sum(d * d, axis=1) / (n - 1)
        sc = d / np.sqrt(var)[:, None]
        ac = [np.sum(np.ascontiguousarray(sc[:, l:] * sc[:, :-l]), axis=1) / (n - l) for l in range(1, n_lags + 1)]
        pw = [ac[i] * ac[j] for i, j in combinations(range(n_lags), 2)]
    return np.column_stack([mu, var] + ac + pw)


# ---- M/G/1 --------------------------------------------------------------------------------------------------------
def mg1_draws_from_state(random_state, batch, n_obs):
    """(E, V), each (batch, n_obs): the standard exponentials and uniforms ELFI's example consumes (it draws them
    (n_obs, batch): exponential(1 / t3) = (1 / t3) standard_exponential, uniform(t1, t2) = t1 + (t2 - t1) random_sample)."""
    E = random_state.standard_exponential((n_obs, batch))
    V = random_state.random_sample((n_obs, batch))
    return np.ascontiguousarray(E.T), np.ascontiguousarray(V.T)


def mg1_series(t1, t2, t3, E, V):
    """Inter-departure times y (batch, n_obs): arrivals every W = (1 / t3) E, service times U = t1 + (t2 - t1) V,
    y_i = U_i + max(0, arrival_i - departure_{i-1})."""
    E, V = np.asarray(E, dtype=np.float64), np.asarray(V, dtype=np.float64)
    batch, n_obs = E.shape
    t1, t2, t3 = [np.broadcast_to(np.asarray(t, dtype=np.float64).reshape(-1), (batch,)) for t in (t1, t2, t3)]
    with np.errstate(all='ignore'):
        W = (1 / t3)[:, None] * E
        U = t1[:, None] + (t2 - t1)[:, None] * V
        sum_w, sum_x = np.zeros(batch), np.zeros(batch)
        Y = np.empty((batch, n_obs))
        for i in range(n_obs):
            sum_w = sum_w + W[:, i]
            y = U[:, i] + np.maximum(0, sum_w - sum_x)
            sum_x = sum_x + y
            Y[:, i] = y
    return Y


def quantile_positions(q, n):
    """(lo, hi, t) of np.quantile(method='linear') on n sorted values: the two neighbours of the virtual index (n - 1) q
    and the interpolation weight.  At the upper end NumPy names the last element -1 and measures the weight from there
    (t = n); the interpolation between two equal neighbours does not depend on it."""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    virt = (n - 1) * q
    prev = np.floor(virt)
    nxt = prev + 1
    above = virt >= n - 1
    prev[above], nxt[above] = -1, -1
    below = virt < 0
    prev[below], nxt[below] = 0, 0
    t = virt - prev
    return (prev.astype(np.int64) % n).astype(np.int32), (nxt.astype(np.int64) % n).astype(np.int32), t


def quantiles_at(Y, lo, hi, t):
    """(batch, nq): a + (b - a) t below one half, b - (b - a) (1 - t) from there on, a and b the sorted neighbours."""
    s = np.sort(np.asarray(Y, dtype=np.float64), axis=1)
    a, b = s[:, lo], s[:, hi]
    with np.errstate(all='ignore'):
        diff = b - a
        out = np.where(t >= 0.5, b - diff * (1 - t), a + diff * t)
    out[np.isnan(s[:, -1])] = np.nan
    return out


def mg1_quantiles(Y, q):
    return quantiles_at(Y, *quantile_positions(q, np.asarray(Y).shape[1]))


def log_identity(Y):
    with np.errstate(all='ignore'):
        return np.log(Y)


def weighted_euclidean(S, obs, w=None):
    """cdist's order: one accumulator, left to right, s += w_j (d_j d_j), then the root."""
    S = np.atleast_2d(np.asarray(S, dtype=np.float64))
    obs = np.asarray(obs, dtype=np.float64).reshape(-1)
    s = np.zeros(S.shape[0])
    with np.errstate(all='ignore'):
        for j in range(S.shape[1]):
            d = S[:, j] - obs[j]
            s = s + (d * d if w is None else w[j] * (d * d))
        return np.sqrt(s)
