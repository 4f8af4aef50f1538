"""The yardstick of the device regression adjustment (csrc/adjust.hip): the recorded cases, the recipe that regenerates
their inputs from a seed (inputs are never stored), the error metric and the bound.

    coefficients      |c - truth| / max_a |truth_a|   per parameter (the largest coefficient of that parameter)
    adjusted values   |a - truth| / (1 + |truth|)

`truth` is the least-squares solution in 40-digit arithmetic on the same float inputs (scripts/make_golden_adjust.py).
The bound of a case is 16 x the largest error of the reference (elfi's LinearAdjustment, scikit-learn's SVD) over the
recorded cases with the same m, and never below 16 eps: the margin the project grants a differently ordered summation.
So that the bound is not vacuous a recorded case has e_ref <= 1e-10 in both metrics and a condition number of the centred,
column-normalised regressors of at most 1e6.

A plain module: tests, the fixture script and smoke() import it; it defines no fixture and needs no GPU.
"""
import zlib

import numpy as np

EPS = np.finfo(np.float64).eps
MAX_E_REF = 1e-10
MAX_COND = 1e6

# (seed, n, m, q, kind).  Rows against the tile of 256: one tile minus one, exactly one, one plus one, two plus one,
# several (and several tiles of 128: m + q > 40 at 66 x 64); m = 1, across a 16-column boundary (33) and 64; q = 1 and 16.
CASES = [
    (21, 3, 1, 1, 'plain'),
    (22, 66, 64, 2, 'plain'),
    (23, 255, 3, 1, 'correlated'),
    (24, 256, 2, 2, 'scales'),
    (25, 257, 8, 3, 'offset'),
    (26, 513, 2, 2, 'plain'),
    (27, 1000, 33, 5, 'plain'),
    (28, 700, 16, 16, 'plain'),
]

# the gauss run of the fixture and of the end-to-end tests: adjust_posterior's docstring example with a fixed seed
GAUSS_RUN = dict(seed_obs=7, seed=3, n_samples=500, batch_size=10, summaries=('ss_mean', 'ss_var'), parameters=('mu',))


def make_case(ci):
    """(X (n, m), Y (n, q)) of case ci.  Z are standard normal regressors, Y = Z B + 0.3 noise.
    'correlated': every column shares a common factor (pairwise correlation 0.9);
    'scales': the columns are scaled by 10^-3 ... 10^3; 'offset': the columns sit 10^4 standard deviations from zero."""
    seed, n, m, q, kind = CASES[ci]
    rs = np.random.RandomState(seed)
    Z = rs.randn(n, m)
    if kind == 'correlated':
        Z = np.sqrt(0.9) * rs.randn(n, 1) + np.sqrt(0.1) * Z
    B = rs.randn(m, q)
    Y = Z @ B + 0.3 * rs.randn(n, q)
    X = Z
    if kind == 'scales':
        X = Z * np.logspace(-3, 3, m)
    elif kind == 'offset':
        X = Z + 1e4 * np.sign(rs.randn(m))
    return np.ascontiguousarray(X), np.ascontiguousarray(Y)


def checksum(ci):
    """CRC-32 of the case's inputs as bytes: the fixture records it, so a recipe that drifts is seen."""
    X, Y = make_case(ci)
    return zlib.crc32(Y.tobytes(), zlib.crc32(X.tobytes()))


def coef_error(coef, truth):
    """coef, truth (q, m) -> the largest |c - truth| / max_a |truth_a| over the parameters."""
    coef, truth = np.atleast_2d(coef), np.atleast_2d(truth)
    return float(np.max(np.abs(coef - truth) / np.max(np.abs(truth), axis=1, keepdims=True)))


def adjusted_error(adj, truth):
    adj, truth = np.asarray(adj, float), np.asarray(truth, float)
    return float(np.max(np.abs(adj - truth) / (1.0 + np.abs(truth))))


def same_m(m):
    return [i for i, c in enumerate(CASES) if c[2] == m]


def bound(e_ref_same_m):
    """16 x the reference's largest own error over the recorded cases with the same m, never below 16 eps."""
    return max(16.0 * float(np.max(e_ref_same_m)), 16.0 * EPS)


def condition_number(X):
    """Of the centred, column-normalised regressors."""
    Xc = X - X.mean(axis=0)
    return float(np.linalg.cond(Xc / np.linalg.norm(Xc, axis=0)))


def reference_adjust(mod, X, Y):
    """(coef (q, m), adjusted (n, q)) by the reference's LinearAdjustment (mod: its post_processing module) on regressors
    X and parameters Y: its own pairing, its scikit-learn fit and its _adjust."""
    names = ['t%d' % t for t in range(Y.shape[1])]
    adj = mod.LinearAdjustment()
    adj._X = X
    adj._sample = mod.results.Sample(method_name='case', outputs={nm: Y[:, t].copy() for t, nm in enumerate(names)},
                                     parameter_names=names)
    adj._parameter_names = names
    adj._get_finite()
    for pair in adj._pairs():
        adj.regression_models.append(adj._fit1(*pair))
    adj._fitted = True
    out = adj.adjust()
    return (np.array([mdl.coef_ for mdl in adj.regression_models]),
            np.column_stack([out.outputs[nm] for nm in names]))


def gauss_sample(mod, gold, rows=None):
    """(Sample, model stand-in) of the recorded gauss run (its first `rows` rows in the order given by `rows`, an index
    array, or all): what adjust_posterior needs of an ElfiModel is `model[name].observed`."""
    import types
    run = GAUSS_RUN
    idx = np.arange(len(gold['gauss_mu'])) if rows is None else np.asarray(rows)
    outputs = {'mu': gold['gauss_mu'][idx], 'd': gold['gauss_discrepancies'][idx]}
    for j, s in enumerate(run['summaries']):
        outputs[s] = gold['gauss_summaries'][idx, j]
    sample = mod.results.Sample(method_name='Rejection', outputs=outputs, parameter_names=list(run['parameters']),
                                discrepancy_name='d')
    model = {s: types.SimpleNamespace(observed=np.array([gold['gauss_observed'][j]]))
             for j, s in enumerate(run['summaries'])}
    return sample, model


def lstsq_adjust(X, Y):
    """The NumPy statement: (adjusted (n, q), coef (q, m), intercept (q), rss (q)) by LAPACK's least squares on the centred
    columns; the adjustment uses the uncentred X."""
    X, Y = np.asarray(X, float), np.asarray(Y, float).reshape(len(X), -1)
    xb, yb = X.mean(axis=0), Y.mean(axis=0)
    B = np.linalg.lstsq(X - xb, Y - yb, rcond=None)[0]
    res = (Y - yb) - (X - xb) @ B
    return Y - X @ B, B.T.copy(), yb - xb @ B, np.sum(res * res, axis=0)
