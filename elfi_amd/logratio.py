"""Logistic-regression ratio estimation on the GPU: the batched call and a drop-in for the reference's classifier.

    lr = elfi_amd.log_ratio(likelihood, marginal, observed, n_groups=64)      # 64 fits in ONE device call
    clf = elfi_amd.HipLogisticRegression()                                    # instead of elfi's LogisticRegression
    bolfire = elfi.BOLFIRE(model, 500, classifier=clf, ...)                   # nothing in ELFI edited

`log_ratio` is the thin mirror of `elfihip_log_ratio` (csrc/logratio.hip): G groups of n likelihood rows, each stacked
on the same marginal rows, standardised, fitted by L1-penalised logistic regression (the objective of scikit-learn's
liblinear with its defaults, the intercept penalised) and read at the observed rows -- what
elfi/methods/classifier.py:72-121 does for one group per call on the host.  `HipLogisticRegression` carries the
reference's interface (fit, predict_log_likelihood_ratio, predict_likelihood_ratio, attributes) and is a subclass of the
imported ELFI's `Classifier`, so `BOLFIRE._resolve_classifier` (bolfire.py:311-317) accepts it.

Not on the device: other penalties and solvers, class weights, a fit without intercept, the GP classifier.
They raise; nothing falls back quietly.
"""
import math
import sys
import warnings

import numpy as np

from . import _lib

MAX_FEATURES = 64
DEFAULT_TOL = 1e-13         # of the optimality violation (why)
DEFAULT_MAX_ITER = 100      # outer (Newton) steps; the cases of the fixture take 4 to 9
STATUS_MAX_ITER, STATUS_NOT_FINITE, STATUS_STALLED = 1, 2, 4
_CLASSES = {}


class LogRatioConvergenceWarning(UserWarning):
    """A group stopped before its optimality violation reached tol."""


def _rows(a, name, m=None):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a.reshape(-1, 1) if m in (None, 1) else a.reshape(1, -1)
    if a.ndim != 2:
        raise ValueError('%s must be 2d (rows of summaries)' % name)
    if m is not None and a.shape[1] != m:
        raise ValueError('%s has %d columns, the likelihood rows have %d' % (name, a.shape[1], m))
    return np.ascontiguousarray(a)


def warn_unconverged(status, tol):
    """One warning for the groups of a call that stopped before tol (as scikit-learn's ConvergenceWarning does)."""
    status = np.atleast_1d(status)
    stopped = np.flatnonzero(status & (STATUS_MAX_ITER | STATUS_STALLED))
    if stopped.size:
        warnings.warn('log_ratio: %d of %d fits stopped before the optimality violation reached tol=%g (first: group %d, '
                      '%s); increase max_iter or tol' % (stopped.size, status.size, tol, stopped[0],
                                                         'max_iter reached' if status[stopped[0]] & STATUS_MAX_ITER
                                                         else 'the objective cannot be lowered further'),
                      LogRatioConvergenceWarning, stacklevel=3)


def log_ratio(likelihood, marginal, observed, n_groups=1, C=1.0, class_min=0, tol=None, max_iter=DEFAULT_MAX_ITER,
              return_parts=False, ctx=None):
    """Log likelihood ratios log p(observed | theta_g) / p(observed) of `n_groups` parameter points in one device call.

    likelihood: (n_groups * n, m), group g = rows g n ... g n + n - 1, or (n_groups, n, m): rows simulated at theta_g
    (label +1).  marginal: (nm, m), rows from the marginal (label -1), shared by every group.  observed: (k, m) or (m,).
    C: inverse strength of the L1 penalty (liblinear's default 1); class_min: lower limit of the class probability;
    tol: limit of the optimality violation (default DEFAULT_TOL); max_iter: limit of the outer steps.
    Returns (n_groups, k); (k,) for one group given as a 2-d array.  With return_parts: (logratio, parts) with
    parts = dict(coef (G, m), intercept (G), mean (G, m), scale (G, m), n_iter (G), status (G)), status 0: converged,
    1: max_iter reached, 2: a non-finite value (NaN outputs), 4: stalled at the rounding level of the objective.
    A group that stops before tol warns (LogRatioConvergenceWarning).
    """
    X = np.asarray(likelihood, dtype=np.float64)
    keep_group_axis = X.ndim == 3 or n_groups != 1
    if X.ndim == 3:
        if n_groups not in (1, X.shape[0]):
            raise ValueError('n_groups=%d but likelihood has %d groups' % (n_groups, X.shape[0]))
        n_groups = X.shape[0]
        X = X.reshape(-1, X.shape[2])
    X = _rows(X, 'likelihood')
    n_groups = int(n_groups)
    rows, m = X.shape
    if n_groups < 1 or rows % n_groups or rows == 0:
        raise ValueError('%d rows do not divide into %d groups' % (rows, n_groups))
    if m < 1 or m > MAX_FEATURES:
        raise ValueError('%d summaries: the device kernel takes 1 to %d' % (m, MAX_FEATURES))
    M = _rows(marginal, 'marginal', m)
    Y = _rows(observed, 'observed', m)
    if len(M) < 1 or len(Y) < 1:
        raise ValueError('marginal and observed need at least one row')
    C, class_min = float(C), float(class_min)
    if not (C > 0 and math.isfinite(C)):
        raise ValueError('C must be positive and finite')
    if not 0 <= class_min < 1:
        raise ValueError('class_min must lie in [0, 1)')
    tol = DEFAULT_TOL if tol is None else float(tol)
    if not tol >= 0:
        raise ValueError('tol must not be negative')
    max_iter = int(max_iter)
    if max_iter < 0:
        raise ValueError('max_iter must not be negative')
    n, k = rows // n_groups, len(Y)
    out = np.empty((n_groups, k), dtype=np.float64)
    parts = dict(coef=np.empty((n_groups, m)), intercept=np.empty(n_groups), mean=np.empty((n_groups, m)),
                 scale=np.empty((n_groups, m)), n_iter=np.empty(n_groups, dtype=np.int32),
                 status=np.empty(n_groups, dtype=np.int32))
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_log_ratio", _lib.ptr(X), n_groups, n, m, m, _lib.ptr(M), len(M), m, _lib.ptr(Y), k, C, class_min, tol,
             max_iter, _lib.ptr(out), _lib.ptr(parts['coef']), _lib.ptr(parts['intercept']), _lib.ptr(parts['mean']),
             _lib.ptr(parts['scale']), _lib.ptr(parts['n_iter']), _lib.ptr(parts['status']))
    warn_unconverged(parts['status'], tol)
    if not keep_group_axis:
        out = out[0]
    return (out, parts) if return_parts else out


# ---- the reference's classifier interface (classifier.py:12-121) --------------------------------------------------------

_HONOURED = ('penalty', 'solver', 'C', 'tol', 'max_iter')
_FIXED = {'penalty': 'l1', 'solver': 'liblinear', 'fit_intercept': True, 'intercept_scaling': 1, 'class_weight': None}


def resolve_config(config):
    """dict(C, tol, max_iter) of the reference's config dict (the keywords of scikit-learn's LogisticRegression);
    ValueError naming the first key or value the device fit does not compute."""
    if not isinstance(config, dict):                    # classifier.py:111-115: anything else means the default
        config = {'penalty': 'l1', 'solver': 'liblinear'}
    for key, value in config.items():
        if key in ('C', 'tol', 'max_iter'):
            continue
        if key not in _FIXED:
            raise ValueError('HipLogisticRegression: config key %r is not supported (honoured: %s)'
                             % (key, ', '.join(_HONOURED)))
        if value != _FIXED[key] or (value is True) != (_FIXED[key] is True):
            raise ValueError('HipLogisticRegression: config %s=%r is not supported: the device fit computes %s=%r '
                             'only, and the package has no CPU fallback' % (key, value, key, _FIXED[key]))
    for key in ('penalty', 'solver'):
        if key not in config:                           # scikit-learn's own defaults are l2 / lbfgs
            raise ValueError("HipLogisticRegression: config must say %s=%r (scikit-learn's default differs)"
                             % (key, _FIXED[key]))
    return dict(C=float(config.get('C', 1.0)), tol=config.get('tol'), max_iter=int(config.get('max_iter', DEFAULT_MAX_ITER)))


def _reference_classifier():
    mod = sys.modules.get('elfi.methods.classifier')
    if mod is None:
        raise ImportError("HipLogisticRegression subclasses the running program's elfi.methods.classifier.Classifier: "
                          "`import elfi` first")
    return mod.Classifier


def hip_logistic_regression_class():
    """The subclass of the imported ELFI's Classifier (made once per reference class): the interface of the reference's
    LogisticRegression (classifier.py:72-121) with scaler, fit and log-odds in one device call per fit."""
    Classifier = _reference_classifier()
    cls = _CLASSES.get(Classifier)
    if cls is not None:
        return cls

    class HipLogisticRegression(Classifier):
        __doc__ = hip_logistic_regression_class.__doc__

        def __init__(self, config=None, class_min=0, ctx=None):
            self.config = config if isinstance(config, dict) else {'penalty': 'l1', 'solver': 'liblinear'}
            self._settings = resolve_config(config)
            if not (isinstance(class_min, int) or isinstance(class_min, float)):
                raise TypeError('class_min has to be either non-negative int or float')      # classifier.py:117-121
            self.class_min = class_min
            self._ctx = ctx
            self._rows = None
            self._fit = None

        def fit(self, X, y):
            """X (n_samples, n_features), y in {+1, -1}, any row order: rows are split by label, each label's rows in
            the order given.  The device call happens with the first prediction (it needs the points) and once more
            for every other set of points."""
            X = np.asarray(X, dtype=np.float64)
            y = np.asarray(y).reshape(-1)
            if X.ndim != 2 or len(y) != len(X):
                raise ValueError('X must be (n_samples, n_features) and y (n_samples,)')
            pos, neg = y == 1, y == -1
            if not np.all(pos | neg) or not pos.any() or not neg.any():
                raise ValueError('y must hold the labels +1 and -1, both present')
            self._rows = (np.ascontiguousarray(X[pos]), np.ascontiguousarray(X[neg]))
            self._fit = None

        def _run(self, points):
            if self._rows is None:
                raise RuntimeError('fit first')
            s = self._settings
            with warnings.catch_warnings():
                if self._fit is not None:       # the same fit, read at other points: it has warned already
                    warnings.simplefilter('ignore', LogRatioConvergenceWarning)
                value, parts = log_ratio(self._rows[0], self._rows[1], points, C=s['C'], class_min=self.class_min,
                                         tol=s['tol'], max_iter=s['max_iter'], return_parts=True, ctx=self._ctx)
            self._fit = parts
            return value

        def predict_log_likelihood_ratio(self, X):
            return self._run(np.asarray(X, dtype=np.float64).reshape(-1, self._rows[0].shape[1])
                             if self._rows is not None else X)

        @property
        def attributes(self):
            if self._fit is None:
                if self._rows is None:
                    raise RuntimeError('fit first')
                self._run(self._rows[0][:1])
            f = self._fit
            return {'parameters': {'coef_': f['coef'].tolist(), 'intercept_': f['intercept'].tolist(),
                                   'n_iter': f['n_iter'].tolist()}}

    HipLogisticRegression.__name__ = 'HipLogisticRegression'
    HipLogisticRegression.__qualname__ = 'HipLogisticRegression'
    _CLASSES[Classifier] = HipLogisticRegression
    return HipLogisticRegression


def HipLogisticRegression(config=None, class_min=0, **kwargs):
    """elfi.methods.classifier.LogisticRegression(config=None, class_min=0) with the fit on the GPU."""
    return hip_logistic_regression_class()(config=config, class_min=class_min, **kwargs)
