"""KLIEP density-ratio estimation on the GPU: the batched fit and a drop-in for the reference's estimator.

    fit = elfi_amd.kliep_fit(x, y, weights_x, weights_y, sigma=[10., 1., .1], fold=5)    # ONE device call: 3 scales x (1 + 5) fits
    est = elfi_amd.HipDensityRatioEstimation(n=100, epsilon=0.001, max_iter=200, fold=5)
    smc = elfi_amd.HipAdaptiveThresholdSMC(d, densratio_estimation=est)                   # nothing in ELFI edited

`kliep_fit` and `kliep_ratio` are the thin mirrors of `elfihip_kliep_fit` / `elfihip_kliep_ratio` (csrc/kliep.hip).
`HipDensityRatioEstimation` is a subclass of the imported ELFI's DensityRatioEstimation
(elfi/methods/density_ratio_estimation.py:31-207): constructor, attributes, argument checks and their messages are the
reference's; `fit` is one device call, `w` a callable on one point or an array of points, `max_ratio()` the maximum of
the `w` the fit itself returned.

Decided divergence: with optimize=True the reference takes np.argmax of a zip object, which is always index
0, so it keeps the FIRST scale of the list whatever the scores are; the device class evaluates every scale and fold in the
same call and keeps sigma[argmax(lcv)].
"""
import sys
from functools import partial

import numpy as np

from . import _lib

MAX_DIM = 64
MAX_BASIS = 256
MAX_ROWS = 65536
MAX_SCALES = 16
MAX_FOLDS = 16
_CLASSES = {}


def _rows(a, name):
    a = np.asarray(a, dtype=np.float64)
    a = np.ascontiguousarray(a.reshape(a.shape[0], -1) if a.ndim else a.reshape(1, 1))
    if not 1 <= a.shape[1] <= MAX_DIM:
        raise ValueError('%s has %d columns: the device kernel takes 1 to %d' % (name, a.shape[1], MAX_DIM))
    return a


def _weights(w, count, name):
    """(the weights as given, the normalised weights), both float64 (count); None: ones."""
    if w is None:
        raw = np.ones(count)
    else:
        raw = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1))
        if raw.shape != (count,):
            raise ValueError('%s has %d entries for %d rows' % (name, raw.size, count))
    with np.errstate(all='ignore'):
        return raw, np.ascontiguousarray(raw / np.sum(raw))


def _sigmas(sigma):
    if sigma is None:
        raise ValueError('RBF width (sigma) has to provided in first call.')
    s = np.ascontiguousarray(np.atleast_1d(np.asarray(sigma, dtype=np.float64)))
    if s.ndim != 1 or not 1 <= s.size <= MAX_SCALES:
        raise ValueError('sigma must be a float or a list of 1 to %d scales' % MAX_SCALES)
    if not np.all((s > 0) & np.isfinite(s)):
        raise ValueError('every sigma must be positive and finite')
    return s


def kliep_fit(x, y, weights_x=None, weights_y=None, sigma=None, n=100, epsilon=0.1, max_iter=500, abs_tol=0.01,
              conv_check_interval=20, fold=0, ctx=None):
    """KLIEP fits of the ratio p_x / p_y for every scale of `sigma` (a float or a list) in one device call.

    x (Nx, d), y (Ny, d): samples of the numerator and the denominator; the n basis functions are centred at x[:n].
    weights_x, weights_y: non-negative sample weights or None.  As in the reference, the full fit of a scale takes
    weights_x as given and the cross-validation fits take it normalised.
    fold > 0: also the leave-fold-out fits of every scale and their scores.
    Returns a dict: alpha (S, n), w (S, Nx) = the fitted ratio at x, iters (S) = the index at which the loop ended, and
    with fold > 0 scores (S, fold) and lcv (S) (+inf for a scale at which no row of x has a basis value above 1e-64).
    A float sigma gives the same arrays with S = 1.
    """
    x, y = _rows(x, 'x'), _rows(y, 'y')
    if x.shape[1] != y.shape[1]:
        raise ValueError('x has %d columns, y has %d' % (x.shape[1], y.shape[1]))
    Nx, d = x.shape
    Ny = y.shape[0]
    n, max_iter, interval, fold = int(n), int(max_iter), int(conv_check_interval), int(fold)
    if Nx < n:
        raise ValueError("Number of RBFs ({}) can't be larger than number of samples ({}).".format(n, Nx))
    if not 1 <= n <= MAX_BASIS:
        raise ValueError('%d basis functions: the device kernel takes 1 to %d' % (n, MAX_BASIS))
    if Nx > MAX_ROWS or not 1 <= Ny <= MAX_ROWS:
        raise ValueError('%d and %d rows: the device kernel takes up to %d' % (Nx, Ny, MAX_ROWS))
    if not 0 <= fold <= MAX_FOLDS:
        raise ValueError('fold=%d: the device kernel takes 0 to %d' % (fold, MAX_FOLDS))
    if max_iter < 1 or interval < 1:
        raise ValueError('max_iter and conv_check_interval must be at least 1')
    s = _sigmas(sigma)
    wx, wxn = _weights(weights_x, Nx, 'weights_x')
    _, wyn = _weights(weights_y, Ny, 'weights_y')
    S = s.size
    out = dict(alpha=np.empty((S, n)), w=np.empty((S, Nx)), iters=np.empty(S, dtype=np.int64))
    if fold > 0:
        out.update(scores=np.empty((S, fold)), lcv=np.empty(S))
    ctx = ctx or _lib.default_context()
    ctx.call('elfihip_kliep_fit', _lib.ptr(x), Nx, d, d, _lib.ptr(y), Ny, d, _lib.ptr(wx), _lib.ptr(wxn), _lib.ptr(wyn),
             _lib.ptr(s), S, n, float(epsilon), max_iter, float(abs_tol), interval, fold, _lib.ptr(out['alpha']),
             _lib.ptr(out['w']), _lib.ptr(out['iters']), _lib.ptr(out.get('scores')), _lib.ptr(out.get('lcv')))
    return out


def kliep_ratio(points, centres, alpha, sigma, ctx=None):
    """The fitted ratio sum_j exp(-0.5 |p - c_j|^2 / sigma / sigma) alpha_j at one point or an array of points."""
    centres = _rows(centres, 'centres')
    n, d = centres.shape
    p = np.atleast_2d(np.asarray(points, dtype=np.float64))
    p = np.ascontiguousarray(p.reshape(p.shape[0], -1) if p.size else p.reshape(0, d))
    if p.shape[1] != d:
        raise ValueError('points have %d columns, the centres %d' % (p.shape[1], d))
    alpha = np.ascontiguousarray(np.asarray(alpha, dtype=np.float64).reshape(-1))
    if alpha.shape != (n,) or not 1 <= n <= MAX_BASIS:
        raise ValueError('alpha has %d entries for %d centres (1 to %d)' % (alpha.size, n, MAX_BASIS))
    sigma = float(sigma)
    if not (sigma > 0 and np.isfinite(sigma)):
        raise ValueError('sigma must be positive and finite')
    out = np.empty(p.shape[0])
    ctx = ctx or _lib.default_context()
    ctx.call('elfihip_kliep_ratio', _lib.ptr(p), p.shape[0], d, d, _lib.ptr(centres), n, d, _lib.ptr(alpha), sigma,
             _lib.ptr(out))
    return out


def _reference_class():
    mod = sys.modules.get('elfi.methods.density_ratio_estimation')
    if mod is None:
        raise ImportError("HipDensityRatioEstimation subclasses the running program's ELFI class: `import elfi` first")
    return mod.DensityRatioEstimation


def hip_density_ratio_class():
    """The subclass of the imported ELFI's DensityRatioEstimation (made once per reference class) whose fit runs on the
    device; with optimize=True it keeps the scale with the largest cross-validation score."""
    Base = _reference_class()
    cls = _CLASSES.get(Base)
    if cls is not None:
        return cls

    class HipDensityRatioEstimation(Base):
        __doc__ = hip_density_ratio_class.__doc__

        def fit(self, x, y, weights_x=None, weights_y=None, sigma=None):
            """DensityRatioEstimation.fit (density_ratio_estimation.py:71-134) as one device call."""
            self.x_len = x.shape[0]
            self.y_len = y.shape[0]
            x = x.reshape(self.x_len, -1)
            y = y.reshape(self.y_len, -1)
            self.x = x
            if self.x_len < self.n:
                raise ValueError("Number of RBFs ({}) can't be larger "
                                 "than number of samples ({}).".format(self.n, self.x_len))
            self.theta = x[:self.n, :]
            if weights_x is None:
                weights_x = np.ones(self.x_len)
            if weights_y is None:
                weights_y = np.ones(self.y_len)
            self.weights_x = weights_x / np.sum(weights_x)
            self.weights_y = weights_y / np.sum(weights_y)
            self.x0 = np.average(x, axis=0, weights=weights_x)
            if isinstance(sigma, float):
                self.sigma = sigma
                self.optimize = False
            if self.optimize and not isinstance(sigma, list):
                raise ValueError("To optimize RBF scale, "
                                 "you need to provide a list of candidate scales.")
            if not self.optimize and self.sigma is None:
                raise ValueError("RBF width (sigma) has to provided in first call.")
            kw = dict(n=self.n, epsilon=self.epsilon, max_iter=self.max_iter, abs_tol=self.abs_tol,
                      conv_check_interval=self.conv_check_interval)
            if self.optimize:
                res = kliep_fit(x, y, weights_x, weights_y, sigma=sigma, fold=self.fold, **kw)
                self.lcv_scores = res['lcv']
                pick = int(np.argmax(res['lcv']))
                self.sigma = sigma[pick]
            else:
                res = kliep_fit(x, y, weights_x, weights_y, sigma=float(self.sigma), **kw)
                pick = 0
            self.alpha = res['alpha'][pick]
            self.iterations = int(res['iters'][pick])
            self._w_x = res['w'][pick]
            self.w = partial(kliep_ratio, centres=self.theta, alpha=self.alpha, sigma=float(self.sigma))

        def max_ratio(self):
            """The maximum of the ratio at the numerator sample: of the w the fit returned, without a second pass."""
            return np.max(self._w_x)

    HipDensityRatioEstimation.__name__ = 'HipDensityRatioEstimation'
    HipDensityRatioEstimation.__qualname__ = 'HipDensityRatioEstimation'
    _CLASSES[Base] = HipDensityRatioEstimation
    return HipDensityRatioEstimation


def HipDensityRatioEstimation(*args, **kwargs):
    """elfi's DensityRatioEstimation(n=100, epsilon=0.1, max_iter=500, abs_tol=0.01, conv_check_interval=20, fold=5,
    optimize=False) with the fit on the GPU."""
    return hip_density_ratio_class()(*args, **kwargs)
