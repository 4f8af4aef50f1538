"""NumPy statement of the g-and-k example models the device runs (csrc/gnk.hip): the univariate and the bivariate series,
the reference's three summaries, the true order statistics, the distance, the replay of the draws the reference's
simulators consume, and the error unit the device's series is held to.

Written from the models' definitions, draws handed in, in the operation order the device keeps: every function here is
pinned bit for bit to recorded runs of ELFI's own examples (tests/golden/gnk.npz, tests/test_gnk.py); the device's
summaries are pinned bit for bit to these functions and its series -- which goes through the device's exp and pow -- to
the bound stated in tests/test_gnk_gpu.py.
"""
import numpy as np

EPS = np.finfo(float).eps
OCTILES = np.linspace(12.5, 87.5, 7)


# ---- the draws -------------------------------------------------------------------------------------------------------
def gnk_draws_from_state(random_state, batch, n_obs):
    """(batch, n_obs): the standard normals GNK consumes (gnk.py:61)."""
    import scipy.stats as ss
    return ss.norm.rvs(size=(batch, n_obs), random_state=random_state)


def bignk_draws_from_state(random_state, rho, n_obs):
    """(batch, n_obs, 2): the correlated normals BiGNK consumes, one multivariate_normal.rvs call per simulation
    (bignk.py:84-90)."""
    import scipy.stats as ss
    rho = np.asarray(rho, dtype=np.float64).reshape(-1)
    z = [ss.multivariate_normal.rvs(cov=np.array([[1, float(r)], [float(r), 1]]), size=n_obs, random_state=random_state)
         for r in rho]
    return np.array(z).reshape(rho.shape[0], n_obs, 2)


def correlate(e, rho):
    """The device's pairs: (batch, n_obs, 2) independent normals e -> z0 = e0, z1 = (rho e0) + (sqrt(1 - rho rho) e1)."""
    e = np.asarray(e, dtype=np.float64)
    rho = np.asarray(rho, dtype=np.float64).reshape(-1, 1)
    z = e.copy()
    z[:, :, 1] = (rho * e[:, :, 0]) + (np.sqrt(1.0 - rho * rho) * e[:, :, 1])
    return z


# ---- the series ------------------------------------------------------------------------------------------------------
def split_params(P):
    """P (batch, 4) = A, B, g, k or (batch, 9) = A1, A2, B1, B2, g1, g2, k1, k2, rho -> A, B, g, k each (batch, 1, dim)."""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    dim = 1 if P.shape[1] == 4 else 2
    return [P[:, q * dim:(q + 1) * dim][:, None, :] for q in range(4)]


def series(P, z, c=0.8):
    """y (batch, n_obs, dim) = A + ((B (1 + c ((1 - exp(-g z)) / (1 + exp(-g z))))) (1 + z z)^k) z, per dimension."""
    A, B, g, k = split_params(P)
    z = np.asarray(z, dtype=np.float64)
    if z.ndim == 2:
        z = z[:, :, None]
    with np.errstate(all='ignore'):
        ex = np.exp(-(g * z))
        br = 1 + c * ((1 - ex) / (1 + ex))
        return A + ((B * br) * np.power(1 + z * z, k)) * z


# ---- the summaries ---------------------------------------------------------------------------------------------------
def ss_order(y):
    """The reference's ss_order: np.sort along the LAST axis (the dimensions of one observation), (batch, n_obs, dim)."""
    return np.sort(y)


def order_from_swaps(y, swaps):
    """The recorded output of the reference's ss_order: y with the two values of the marked observations exchanged."""
    return np.where(np.asarray(swaps, dtype=bool)[:, :, None], y[:, :, ::-1], y)


def sorted_rows(y):
    """True order statistics: every (simulation, dimension) column sorted, NaNs last."""
    return np.sort(y, axis=1)


def octile_positions(n_obs):
    """(lo, hi, t) of np.percentile(method='linear') at the seven octiles of n_obs sorted values."""
    virt = (n_obs - 1) * np.true_divide(OCTILES, 100)
    lo = np.floor(virt)
    return lo.astype(np.int32), np.minimum(lo + 1, n_obs - 1).astype(np.int32), virt - lo


def octiles(y):
    """(7, batch, dim): a + (b - a) t below one half, b - (b - a) (1 - t) from there on; a column with a NaN is NaN."""
    s = np.sort(np.asarray(y, dtype=np.float64), axis=1)
    lo, hi, t = octile_positions(s.shape[1])
    out = np.empty((7,) + s[:, 0].shape)
    with np.errstate(all='ignore'):
        for j in range(7):
            a, b = s[:, lo[j]], s[:, hi[j]]
            diff = b - a
            out[j] = b - diff * (1 - t[j]) if t[j] >= 0.5 else a + diff * t[j]
    out[:, np.isnan(s[:, -1])] = np.nan
    return out


def ss_octile(y):
    """(batch, 7 dim, 1) = [E1_d0, E1_d1, E2_d0, ...]."""
    return np.hstack(list(octiles(y)))[:, :, None]


def ss_robust(y):
    """(batch, 4 dim, 1) = [A_d0, A_d1, B_d0, ...]: E4; E6 - E2 (exact zeros become eps); ((E6 + E2) - 2 E4) / ss_B;
    (((E7 - E5) + E3) - E1) / ss_B."""
    E1, E2, E3, E4, E5, E6, E7 = octiles(y)
    with np.errstate(all='ignore'):
        sB = E6 - E2
        sB[sB == 0] += EPS
        sg = ((E6 + E2) - 2 * E4) / sB
        sk = (((E7 - E5) + E3) - E1) / sB
    return np.hstack((E4, sB, sg, sk))[:, :, None]


def euclidean_multiss(s, obs):
    """gnk.py:115-142 for one summary (batch, m, 1) against the observed (1, m, 1)."""
    with np.errstate(all='ignore'):
        return np.sqrt(np.sum(np.sum((s - obs) ** 2., axis=1), axis=1))


def flat(s):
    """A summary or a series (batch, m, dim) as the (batch, m dim) rows the device returns."""
    s = np.asarray(s)
    return s.reshape(s.shape[0], -1)


# ---- the error unit of the series ------------------------------------------------------------------------------------
def error_in_units(y, y_hi, y_lo, P):
    """|y - y*| / (eps (|A| + |y* - A|)) per element, y* = y_hi + y_lo the 40-digit value as a double-double pair."""
    A = split_params(P)[0]
    return np.abs((y - y_hi) - y_lo) / (EPS * (np.abs(A) + np.abs((y_hi - A) + y_lo)))


def e_ref(g):
    """The largest error of the reference's own series over the golden block (both models), in that unit."""
    return max(float(np.max(error_in_units(g[p + '_y'], g[p + '_y_hi'], g[p + '_y_lo'], g[p + '_P']))) for p in ('gnk', 'bignk'))
