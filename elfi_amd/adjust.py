"""Regression adjustment of an ABC sample on the GPU: elfi.adjust_posterior / elfi.LinearAdjustment with the fit and the
adjustment on the device, and their batched form.

    res = elfi.Rejection(m['d'], output_names=['ss_mean', 'ss_var'], batch_size=1000).sample(500)
    adj = elfi_amd.adjust_posterior(res, m, ['ss_mean', 'ss_var'], ['mu'])                 # instead of elfi.adjust_posterior
    adjs = elfi_amd.adjust_posterior(res, m, ['ss_mean', 'ss_var'], n_closest=[100, 250, 500])   # three thresholds, one call
    A = elfi_amd.linear_adjust(X, Y, n_groups=64)                                          # 64 samples in ONE device call

`linear_adjust` is the thin mirror of `elfihip_linear_adjust` (csrc/adjust.hip): per group (and per nested prefix of a
group) a least-squares fit of every parameter column on the centred regressors by a Householder QR, and the adjusted
values theta_i - x_i.b.  `HipLinearAdjustment` IS the reference's `LinearAdjustment`
(elfi/methods/post_processing.py:195-209) -- a subclass made from the class of the ELFI the running program has imported
-- with `fit` as one device call for all parameters and `adjust` returning the device's columns.

Not on the device: weighted regression, other regression models, keyword arguments for scikit-learn's
LinearRegression other than fit_intercept=True, the minimum-norm solution for linearly dependent summaries, more than 64
summaries or 16 parameters.  They raise; nothing falls back quietly.
"""
import sys

import numpy as np

from . import _lib

MAX_FEATURES = 64
MAX_RESPONSES = 16
STATUS_RANK = 3             # (2: a non-finite value; the class never sends one)
_CLASSES = {}


def _grouped(a, n_groups, name, vector_is_column):
    """(rows (G n, c) contiguous, G or None when `a` carried no group axis)."""
    a = np.asarray(a, dtype=np.float64)
    groups = None
    if a.ndim == 3:
        groups = a.shape[0]
        a = a.reshape(-1, a.shape[2])
    elif a.ndim == 1 and vector_is_column:
        a = a.reshape(-1, 1)
    if a.ndim != 2:
        raise ValueError('%s must be 2d (rows) or 3d (groups of rows)' % name)
    if groups is not None and n_groups not in (1, groups):
        raise ValueError('n_groups=%d but %s has %d groups' % (n_groups, name, groups))
    return np.ascontiguousarray(a), groups


def check_prefixes(prefixes, n, what='prefixes'):
    """The list as an int64 array: ascending whole numbers, at least 2, the last == n."""
    p = np.asarray(prefixes)
    if p.ndim != 1 or p.size < 1 or not np.all(np.equal(np.mod(p, 1), 0)):
        raise ValueError('%s must be a non-empty list of whole numbers' % what)
    p = p.astype(np.int64)
    if p[0] < 2 or np.any(np.diff(p) <= 0):
        raise ValueError('%s must be ascending and at least 2' % what)
    if n is not None and p[-1] != n:
        raise ValueError('the last of %s must be the number of rows (%d), not %d' % (what, n, p[-1]))
    return np.ascontiguousarray(p)


def linear_adjust(X, Y, n_groups=1, prefixes=None, return_parts=False, ctx=None):
    """The linear regression adjustment of `n_groups` samples of equal size, and of nested prefixes of each, in one
    device call.

    X: (n_groups * n, m), group g = rows g n ... g n + n - 1, or (n_groups, n, m): the summaries minus the observed ones.
    Y: the parameters in the same layout with q columns; a 1-d Y is one parameter.  1 <= m <= 64, 1 <= q <= 16, n >= 2.
    prefixes: ascending row counts >= 2, the last == n: job (g, k) fits and adjusts the first prefixes[k] rows of group g
    (a Rejection sample is ordered by discrepancy, so a prefix is a tighter threshold).
    Returns adjusted (n_groups, K, n, q) = Y - X @ coef.T per job, NaN in the rows at or beyond the prefix; the group
    axis is dropped for one group given as 2-d arrays, the prefix axis without prefixes: (n, q) for the plain call.
    With return_parts: (adjusted, parts), parts = dict(coef (.., q, m), intercept (.., q), rss (.., q), status (..)) with
    the same axes dropped; status 0: ok, 2: a non-finite value in the job's rows, 3: rank-deficient (linearly dependent
    or constant columns, or fewer than m + 1 rows); a job with status 2 or 3 is NaN.
    """
    X, gx = _grouped(X, n_groups, 'X', False)
    Y, gy = _grouped(Y, n_groups, 'Y', True)
    if gx is not None and gy is not None and gx != gy:
        raise ValueError('X has %d groups, Y has %d' % (gx, gy))
    groups = gx if gx is not None else gy
    keep_group_axis = groups is not None or n_groups != 1
    n_groups = int(groups if groups is not None else n_groups)
    rows, m = X.shape
    q = Y.shape[1]
    if Y.shape[0] != rows:
        raise ValueError('X has %d rows, Y has %d' % (rows, Y.shape[0]))
    if n_groups < 1 or rows == 0 or rows % n_groups:
        raise ValueError('%d rows do not divide into %d groups' % (rows, n_groups))
    if m < 1 or m > MAX_FEATURES:
        raise ValueError('%d summaries: the device kernel takes 1 to %d' % (m, MAX_FEATURES))
    if q < 1 or q > MAX_RESPONSES:
        raise ValueError('%d parameters: the device kernel takes 1 to %d' % (q, MAX_RESPONSES))
    n = rows // n_groups
    if n < 2:
        raise ValueError('a group needs at least two rows')
    K = 0
    if prefixes is not None:
        prefixes = check_prefixes(prefixes, n)
        K = len(prefixes)
    Ke = max(K, 1)
    adjusted = np.empty((n_groups, Ke, n, q), dtype=np.float64)
    parts = dict(coef=np.empty((n_groups, Ke, q, m)), intercept=np.empty((n_groups, Ke, q)),
                 rss=np.empty((n_groups, Ke, q)), status=np.empty((n_groups, Ke), dtype=np.int32))
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_linear_adjust", _lib.ptr(X), n_groups, n, m, m, _lib.ptr(Y), q, q,
             _lib.ptr(prefixes) if K else None, K, _lib.ptr(adjusted), _lib.ptr(parts['coef']),
             _lib.ptr(parts['intercept']), _lib.ptr(parts['rss']), _lib.ptr(parts['status']))

    def squeezed(a):
        if K == 0:
            a = a[:, 0]
        return a if keep_group_axis else a[0]
    adjusted = squeezed(adjusted)
    return (adjusted, {k: squeezed(v) for k, v in parts.items()}) if return_parts else adjusted


# ---- the reference's interface (post_processing.py:21-266) -------------------------------------------------------------

def check_model_kwargs(kwargs):
    """The keyword arguments the reference hands to scikit-learn's LinearRegression: the device fit is the default model
    with an intercept."""
    for key, value in kwargs.items():
        if key != 'fit_intercept':
            raise ValueError('HipLinearAdjustment: keyword %r is not supported: the device fits the plain linear model '
                             'with an intercept, and the package has no CPU fallback' % (key,))
        if value is not True:
            raise ValueError('HipLinearAdjustment: fit_intercept=%r is not supported: the device fit has an intercept, '
                             'and the package has no CPU fallback' % (value,))


class FittedLinearModel:
    """What `regression_models[i]` carries of scikit-learn's fitted LinearRegression."""

    def __init__(self, coef, intercept, rss):
        self.coef_, self.intercept_, self.rss_ = coef, intercept, rss


def _reference_module():
    mod = sys.modules.get('elfi.methods.post_processing')
    if mod is None:
        raise ImportError("HipLinearAdjustment subclasses the running program's elfi.LinearAdjustment: `import elfi` first")
    return mod


def _raise_for_status(status, names):
    for name, st in zip(names, status):
        if st == STATUS_RANK:
            raise ValueError('LinearAdjustment of %r: the summaries are linearly dependent (or one is constant), or the '
                             'finite rows are too few for them.  The reference returns the minimum-norm solution there; '
                             'that is not on the device, and the package has no CPU fallback' % (name,))
        if st != 0:
            raise ValueError('LinearAdjustment of %r: the device reports status %d' % (name, st))


def hip_linear_adjustment_class():
    """The subclass of the imported ELFI's LinearAdjustment (made once per reference class): `_input_variables`,
    `_get_finite` with its warning, the properties and `_check_fitted` are the reference's; `fit` is one device call for
    all parameters (one per distinct mask of finite rows), `adjust` returns the device's adjusted columns."""
    mod = _reference_module()
    Ref = mod.LinearAdjustment
    cls = _CLASSES.get(Ref)
    if cls is not None:
        return cls

    class HipLinearAdjustment(Ref):
        __doc__ = hip_linear_adjustment_class.__doc__
        _elfi_amd_device = True

        def __init__(self, ctx=None, **kwargs):
            check_model_kwargs(kwargs)
            super(HipLinearAdjustment, self).__init__(**kwargs)
            self._ctx = ctx
            self._adjusted = []

        def _device_fit(self, X, names, columns):
            """Fit and adjust the parameters `names` (their columns over the rows of X) in one call:
            (models, adjusted columns)."""
            if len(X) < 2:
                _raise_for_status([STATUS_RANK] * len(names), names)
            adj, parts = linear_adjust(X, np.column_stack(columns), return_parts=True, ctx=self._ctx)
            _raise_for_status([parts['status']] * len(names), names)
            models = [FittedLinearModel(parts['coef'][t].copy(), float(parts['intercept'][t]), float(parts['rss'][t]))
                      for t in range(len(names))]
            return models, [np.ascontiguousarray(adj[:, t]) for t in range(len(names))]

        # -- post_processing.py:84-110 ---------------------------------------------------------------------------------
        def fit(self, sample, model, summary_names, parameter_names=None):
            self._X = self._input_variables(model, sample, summary_names)
            self._sample = sample
            self._parameter_names = parameter_names or sample.parameter_names
            self._get_finite()
            names = list(self._parameter_names)
            self.regression_models = [None] * len(names)
            self._adjusted = [None] * len(names)
            by_mask = {}
            for i, mask in enumerate(self._finite):
                by_mask.setdefault(np.asarray(mask, dtype=bool).tobytes(), []).append(i)
            for members in by_mask.values():
                mask = np.asarray(self._finite[members[0]], dtype=bool)
                X = self._X if mask.all() else self._X[mask]
                columns = [np.asarray(sample.outputs[names[i]], dtype=np.float64)[mask] for i in members]
                models, adjusted = self._device_fit(X, [names[i] for i in members], columns)
                for i, mdl, adj in zip(members, models, adjusted):
                    self.regression_models[i], self._adjusted[i] = mdl, adj
            self._fitted = True

        # -- post_processing.py:122-141 --------------------------------------------------------------------------------
        def adjust(self):
            outputs = {name: self._adjusted[i] for i, name in enumerate(self.parameter_names)}
            return mod.results.Sample(method_name=self._name, outputs=outputs, parameter_names=self._parameter_names)

        def adjust_nested(self, sample, model, summary_names, parameter_names, n_closest):
            """One Sample per count of `n_closest`: the adjustment of the rows of that many smallest discrepancies, all
            from one device call (the counts are nested prefixes of the sample ordered by discrepancy)."""
            counts = check_prefixes(n_closest, None, 'n_closest')
            names = list(parameter_names or sample.parameter_names)
            if sample.discrepancies is None:
                raise ValueError('n_closest orders the rows by discrepancy: the sample has none')
            X = self._input_variables(model, sample, summary_names)
            Y = np.column_stack([np.asarray(sample.outputs[name], dtype=np.float64) for name in names])
            if counts[-1] > len(X):
                raise ValueError('n_closest asks for %d rows, the sample has %d' % (counts[-1], len(X)))
            if not (np.isfinite(X).all() and np.isfinite(Y).all()):
                raise ValueError('n_closest needs an all-finite sample: drop the non-finite rows first')
            order = np.argsort(np.asarray(sample.discrepancies).reshape(-1), kind='stable')[:counts[-1]]
            adj, parts = linear_adjust(X[order], Y[order], prefixes=counts, return_parts=True, ctx=self._ctx)
            out = []
            for k, p in enumerate(counts):
                _raise_for_status([parts['status'][k]] * len(names), names)
                outputs = {name: np.ascontiguousarray(adj[k, :p, t]) for t, name in enumerate(names)}
                out.append(mod.results.Sample(method_name=self._name, outputs=outputs, parameter_names=names))
            return out

    HipLinearAdjustment.__name__ = 'HipLinearAdjustment'
    HipLinearAdjustment.__qualname__ = 'HipLinearAdjustment'
    _CLASSES[Ref] = HipLinearAdjustment
    return HipLinearAdjustment


def HipLinearAdjustment(**kwargs):
    """elfi.LinearAdjustment(**kwargs) with the fit and the adjustment on the GPU.  Keyword arguments other than
    fit_intercept=True raise ValueError."""
    check_model_kwargs({k: v for k, v in kwargs.items() if k != 'ctx'})
    return hip_linear_adjustment_class()(**kwargs)


def adjust_posterior(sample, model, summary_names, parameter_names=None, adjustment='linear', n_closest=None):
    """elfi.adjust_posterior (post_processing.py:212-253) on the GPU: the same arguments, the same Sample.

    adjustment: 'linear' or a HipLinearAdjustment; any other adjustment object raises TypeError (it would run on the
    host).  n_closest: ascending row counts; the rows are ordered by `sample.discrepancies` (stable) and the adjustment
    of the `c` closest rows is returned for every count c, as a list of Samples, from ONE device call.  The sample must
    be all-finite then.
    """
    if n_closest is not None:
        check_prefixes(n_closest, None, 'n_closest')
    if isinstance(adjustment, str):
        if adjustment != 'linear':
            raise ValueError("Could not find adjustment method:{}".format(adjustment))
        adjustment = HipLinearAdjustment()
    elif not getattr(adjustment, '_elfi_amd_device', False):
        raise TypeError('adjust_posterior takes adjustment=\'linear\' or an elfi_amd.HipLinearAdjustment; %s would run on '
                        'the host (use elfi.adjust_posterior for it)' % (type(adjustment).__name__,))
    if n_closest is not None:
        return adjustment.adjust_nested(sample, model, summary_names, parameter_names, n_closest)
    adjustment.fit(model=model, sample=sample, parameter_names=parameter_names, summary_names=summary_names)
    return adjustment.adjust()
