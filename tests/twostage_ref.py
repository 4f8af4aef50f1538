"""NumPy/SciPy statement of the three quantities of the device summary-statistic selection (csrc/twostage.hip), written
from the formulas of Nunes & Balding (2010) as elfi/methods/diagnostics.py states them, and the recipe of the synthetic
cases (inputs are regenerated from it, never stored).

    kth_distances_ref   R_ik: the k-th smallest of the n distances from point i (itself included, at 0), by sorting ALL
                        squared distances -- no tree.  A squared distance is summed left to right over the dimensions.
    knn_entropy_ref     E = log(pi^(q/2) / Gamma(q/2 + 1)) - psi(k) + log n + (q / n) sum_i log R_ik
    mrsse_ref           (1 / J) sum_j sqrt(sum_{i,d} (theta_id - closest_jd)^2)
    subset_best_ref     the k rows of smallest euclidean distance over the columns a 0/1 mask selects, stable order, NaN last

A plain module: tests, the fixture script and smoke() import it; it defines no fixture and needs no GPU.
"""
import math

import numpy as np
from scipy.special import digamma, gammaln

EPS = np.finfo(np.float64).eps

# (seed, n, q, k, J, scale, offset): n points in q dimensions = offset + scale * standard normal draws; J closest
CASES = [
    (11, 200, 1, 4, 5, 1.0, 0.0),
    (12, 500, 2, 4, 20, 0.3, 0.5),
    (13, 513, 2, 5, 7, 2.0, -1.0),
    (14, 300, 3, 4, 3, 1.0, 10.0),
    (15, 255, 3, 16, 2, 0.05, 0.0),
    (16, 257, 8, 8, 4, 1.0, 0.0),
    (17, 400, 32, 16, 6, 1.5, 2.0),
    (18, 1200, 2, 2, 12, 1.0, 0.0),
]

# the MA2 run of the fixture (scripts/make_golden_twostage.py) and of the end-to-end test
MA2_RUN = dict(seed_obs=4, seed=1, n_sim=20000, n_acc=500, n_closest=20, batch_size=5000, k=4)
MA2_RECORDED = (('ac1', 'ac2'), ('ac1', 'ac2', 'var'))      # combinations whose accepted parameters the fixture keeps


def make_case(ci):
    """(thetas (n, q), closest (J, q), k) of case ci."""
    seed, n, q, k, J, scale, offset = CASES[ci]
    rs = np.random.RandomState(seed)
    thetas = offset + scale * rs.randn(n, q)
    closest = offset + scale * rs.randn(J, q)
    return thetas, closest, k


def _groups(thetas, n_groups):
    T = np.asarray(thetas, dtype=np.float64)
    if T.ndim == 3:
        return T
    return T.reshape(n_groups, -1, T.shape[-1])


def squared_distances(T):
    """(n, n) squared euclidean distances, each summed left to right over the dimensions."""
    n, q = T.shape
    d2 = np.zeros((n, n))
    for d in range(q):
        diff = T[:, d][:, None] - T[:, d][None, :]
        d2 = d2 + diff * diff
    return d2


def kth_distances_ref(thetas, k, n_groups=1):
    """(G, n): the distance from every point to its k-th nearest neighbour, the point itself being the first; inf for k > n."""
    G = _groups(thetas, n_groups)
    out = np.full(G.shape[:2], np.inf)
    if k <= G.shape[1]:
        for g, T in enumerate(G):
            out[g] = np.sqrt(np.sort(squared_distances(T), axis=1)[:, k - 1])
    return out


def knn_entropy_ref(thetas, k=4, n_groups=1):
    G = _groups(thetas, n_groups)
    n, q = G.shape[1:]
    R = kth_distances_ref(G, k)
    const = 0.5 * q * math.log(math.pi) - gammaln(0.5 * q + 1.0) - digamma(k) + math.log(n)
    with np.errstate(divide='ignore'):
        logs = np.log(R)
    out = np.empty(len(G))
    for g in range(len(G)):
        s = math.fsum(logs[g]) if np.all(np.isfinite(logs[g])) else float(np.sum(logs[g]))
        out[g] = const + (q / n) * s
    return out


def mrsse_ref(thetas, closest, n_groups=1):
    G = _groups(thetas, n_groups)
    Cl = np.asarray(closest, dtype=np.float64).reshape(-1, G.shape[2])
    out = np.empty(len(G))
    for g, T in enumerate(G):
        out[g] = math.fsum(math.sqrt(math.fsum(((T - c) ** 2).ravel())) for c in Cl) / len(Cl)
    return out


def subset_distances(X, y, masks):
    """(n, C) euclidean distances over the columns every mask selects, summed left to right over the selected columns."""
    X, y, M = np.asarray(X, float), np.asarray(y, float).reshape(-1), np.atleast_2d(np.asarray(masks, float))
    out = np.empty((len(X), len(M)))
    for c, mask in enumerate(M):
        s = np.zeros(len(X))
        for j in np.flatnonzero(mask):
            diff = X[:, j] - y[j]
            s = s + diff * diff
        out[:, c] = np.sqrt(s)
    return out


def best_of_columns(D, k):
    """(vals (C, k'), rows (C, k')) of a distance matrix D (n, C): stable order, NaN last, k' = min(k, n)."""
    k = min(k, len(D))
    rows = np.stack([np.argsort(D[:, c], kind='stable')[:k] for c in range(D.shape[1])])
    return np.take_along_axis(D.T, rows, axis=1), rows


def subset_best_ref(X, y, masks, k):
    return best_of_columns(subset_distances(X, y, masks), k)


def bound(e_ref_same_q, truth):
    """The yardstick of the tests: 16 x the reference's largest own error over the cases with the same number of
    parameters, and never below 16 eps (1 + |truth|)."""
    return max(16.0 * float(np.max(e_ref_same_q)), 16.0 * EPS * (1.0 + abs(float(truth))))


def same_q(ci):
    return [i for i, c in enumerate(CASES) if c[2] == CASES[ci][2]]


def ulps(a, b):
    """|a - b| in units of the spacing of doubles at b."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b) / np.spacing(np.abs(b))


# ---- the MA2 setup of the end-to-end check -----------------------------------------------------------------------------

def ma2_candidates():
    """The four candidate statistics of the MA2 run, in the order the combinations are built from."""
    def ac1(x):
        return np.mean(x[:, 1:] * x[:, :-1], axis=1)

    def ac2(x):
        return np.mean(x[:, 2:] * x[:, :-2], axis=1)

    def mean(x):
        return np.mean(x, axis=1)

    def var(x):
        return np.var(x, axis=1)
    return [ac1, ac2, mean, var]


def ma2_simulator(elfi):
    """The MA2 example's simulator node in a model without the example's own summaries and distance."""
    from elfi.examples import ma2
    m = ma2.get_model(seed_obs=MA2_RUN['seed_obs'])
    for name in ('d', 'S2', 'S1'):
        m.remove_node(name)
    return m['MA2']


def combination_names(n_candidates=4, max_cardinality=4):
    from itertools import combinations
    names = [f.__name__ for f in ma2_candidates()][:n_candidates]
    return [c for i in range(max_cardinality) for c in combinations(names, i + 1)]
