"""Bayesian synthetic likelihood (BSL) on the GPU: the batched evaluation and drop-ins for the reference's tools.

    lik = elfi_amd.standard_likelihood(shrinkage='warton', penalty=0.3)       # instead of elfi's pdf_methods factory
    bsl = elfi.BSL(model, n_sim_round=500, likelihood=lik)                    # nothing in ELFI edited
    bsl = elfi_amd.HipBSL(model, n_sim_round=500)                             # the same with the device default
    elfi_amd.log_SL_stdev(model, theta, [100, 200, 500], ['S1', 'S2'], M=20)  # ONE device call for M x 3 evaluations
    elfi_amd.select_penalty(model, 500, theta, ['S1', 'S2'], shrinkage='warton')   # ONE call for M x 31 (the default penalties)
    semi = elfi_amd.semiparametric_likelihood()                               # semiBSL: KDE marginals + Gaussian copula
    elfi_amd.select_penalty(model, 500, theta, ['S1', 'S2'], likelihood=semi) # the same ONE call for the semiparametric form
    bsl = elfi_amd.HipBSL(model, 500, likelihood=elfi_amd.robust_likelihood('variance'), gamma_sampler='device')   # R-BSL-V

`syn_loglik` is the thin mirror of `elfihip_syn_loglik` (csrc/synlik.hip): G groups of n summary rows, K prefixes of
every group and P Warton penalties in one launch.  The factories carry the reference's names and call signatures
(elfi/methods/bsl/pdf_methods.py:19-74) and return callables with the reference's return types (`np.array([ll])`; a
scalar for the robust one, a `functools.partial` with an `adjustment` keyword, which is how `BSL.__init__` detects
misspecification, bsl.py:54).  `semi_loglik` mirrors `elfihip_semi_loglik` (csrc/semibsl.hip) in the same way: the
semiparametric likelihood of An, Nott & Drovandi (pdf_methods.py:46-59, 179-264) with the same (G, K, P) call shape.
`log_SL_stdev` / `select_penalty` (pre_sample_methods.py:102-143, 215-318) draw the same
child seeds through `model.generate` as the reference and stack the M matrices as M groups.

`slice_gamma` mirrors `elfihip_slice_gamma` (csrc/slice_gamma.hip): one slice-sampler sweep over the adjustment
parameters gamma of G robust chains' states in one launch; `slice_gamma_mean` / `slice_gamma_variance` carry the
reference's signatures (slice_gamma_mean.py:35, slice_gamma_variance.py:31) and leave the caller's RandomState where the
reference's functions would; `HipBSL(..., gamma_sampler='device')` puts them into the chain.

Not on the device: graphical-lasso shrinkage, the whitened semiparametric likelihood (wsemiBSL),
estimate_whitening_matrix.  They raise or stay the reference's; nothing falls back quietly.
"""
import ctypes as C
import sys
from functools import partial

import numpy as np

from . import _lib
from .priors import SLICE_GAMMA_STREAM_BASE

MAX_FEATURES = 64
MAX_SEMI_ROWS = 16384       # rows per group of the semiparametric likelihood: one column is held in LDS
_VARIANTS = {'standard': 0, 'unbiased': 1, 'mean': 2, 'variance': 3}
_CLASSES = {}


def _variant_code(variant, adjustment):
    if adjustment is not None:
        if adjustment not in ('mean', 'variance'):
            raise ValueError("adjustment must be 'mean' or 'variance', not %r" % (adjustment,))
        if variant not in ('standard', 'robust', adjustment):
            raise ValueError("adjustment=%r does not go with variant=%r" % (adjustment, variant))
        return _VARIANTS[adjustment]
    if variant == 'robust':
        raise ValueError("variant='robust' needs adjustment='mean' or 'variance'")
    if variant not in _VARIANTS:
        raise ValueError("unknown variant %r (standard, unbiased, robust)" % (variant,))
    return _VARIANTS[variant]


def _groups(ssx, ssy, n_groups):
    """(X (n_groups n, m), y (m), n_groups, n, m, keep_group_axis) of the two layouts ssx may have."""
    X = np.asarray(ssx, dtype=np.float64)
    keep_group_axis = X.ndim == 3 or n_groups != 1
    if X.ndim == 3:
        if n_groups not in (1, X.shape[0]):
            raise ValueError('n_groups=%d but ssx has %d groups' % (n_groups, X.shape[0]))
        n_groups = X.shape[0]
        X = X.reshape(-1, X.shape[2])
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    if X.ndim != 2:
        raise ValueError('ssx must be 2d (rows of summaries) or 3d (groups of rows)')
    n_groups = int(n_groups)
    rows, m = X.shape
    if n_groups < 1 or rows % n_groups:
        raise ValueError('%d rows do not divide into %d groups' % (rows, n_groups))
    n = rows // n_groups
    if n < 2:
        raise ValueError('a group needs at least 2 rows (n=%d)' % n)
    if m < 1 or m > MAX_FEATURES:
        raise ValueError('%d summaries: the device kernel takes 1 to %d' % (m, MAX_FEATURES))
    y = np.ascontiguousarray(np.asarray(ssy, dtype=np.float64).reshape(-1))
    if y.shape != (m,):
        raise ValueError('ssy has %d entries, ssx has %d columns' % (y.size, m))
    return X, y, n_groups, n, m, keep_group_axis


def _penalty_list(shrinkage, penalty, penalties):
    """The Warton penalties as an array, or None without shrinkage."""
    if shrinkage == 'glasso':
        raise NotImplementedError("graphical-lasso shrinkage is not on the device; shrinkage='warton' is")
    if shrinkage not in (None, 'warton'):
        raise ValueError('unknown shrinkage %r' % (shrinkage,))
    if shrinkage is None:
        if penalties is not None:
            raise ValueError("penalties need shrinkage='warton'")
        return None
    if penalties is None and penalty is None:
        raise ValueError("shrinkage='warton' needs penalty or penalties")
    pen = np.ascontiguousarray(np.atleast_1d(np.asarray(penalty if penalties is None else penalties, dtype=np.float64)))
    if pen.ndim != 1 or pen.size < 1:
        raise ValueError('penalties must be a non-empty list')
    if not np.all((pen >= 0) & (pen <= 1)):
        raise ValueError('Gamma must be between 0 and 1')           # cov_warton.py:21-22
    return pen


def _prefix_list(prefixes, n):
    if prefixes is None:
        return None
    pre = np.ascontiguousarray(np.atleast_1d(np.asarray(prefixes)).astype(np.int64))
    if pre.ndim != 1 or pre.size < 1 or np.any(np.diff(pre) <= 0) or pre[0] < 2 or pre[-1] != n:
        raise ValueError('prefixes must be ascending row counts >= 2 whose last entry is n=%d' % n)
    return pre


def _squeeze(ll, keep_group_axis, prefixes, penalties):
    """(G, K, max(P, 1)) -> the axes the caller asked for; a float for one group given as a 2-d array and neither list."""
    if penalties is None:
        ll = ll[:, :, 0]
    if prefixes is None:
        ll = ll[:, 0]
    if not keep_group_axis:
        ll = ll[0]
        if ll.ndim == 0:
            ll = float(ll)
    return ll


def syn_loglik(ssx, ssy, n_groups=1, variant='standard', shrinkage=None, penalty=None, whitening=None, gamma=None,
               adjustment=None, prefixes=None, penalties=None, return_moments=False, ctx=None):
    """Gaussian synthetic log-likelihoods of `n_groups` groups of simulated summaries in one device call.

    ssx: (n_groups * n, m), group g = rows g n ... g n + n - 1, or (n_groups, n, m); ssy: the m observed summaries.
    variant: 'standard' | 'unbiased' | 'robust' (with adjustment 'mean' | 'variance' and gamma (m)).
    shrinkage: None | 'warton' with `penalty` (one) or `penalties` (several, an axis of the result).
    prefixes: row counts, ascending, the last == n: the likelihood of the first prefixes[k] rows of every group (an axis).
    Returns an array (n_groups[, len(prefixes)][, len(penalties)]); a float for one group given as a 2-d array and
    neither list.  With return_moments: (loglik, mean (G, m), cov (G, m, m)) of the full groups after whitening.
    """
    X, y, n_groups, n, m, keep_group_axis = _groups(ssx, ssy, n_groups)
    code = _variant_code(variant, adjustment)
    g = None
    if code >= 2:
        if gamma is None:
            raise ValueError('the robust likelihood needs gamma')
        g = np.ascontiguousarray(np.broadcast_to(np.asarray(gamma, dtype=np.float64).reshape(-1), (m,)))
    pen = _penalty_list(shrinkage, penalty, penalties)
    if shrinkage is not None and code != 0:
        raise ValueError('shrinkage goes with the standard likelihood only (the unbiased and robust ones have none)')
    pre = _prefix_list(prefixes, n)
    W = None
    if whitening is not None:
        W = np.ascontiguousarray(whitening, dtype=np.float64)
        if W.shape != (m, m):
            raise ValueError('whitening must be (%d, %d)' % (m, m))
    X = np.ascontiguousarray(X)
    K = 1 if pre is None else pre.size
    P = 0 if pen is None else pen.size
    ll = np.empty((n_groups, K, max(P, 1)), dtype=np.float64)
    mean = np.empty((n_groups, m), dtype=np.float64) if return_moments else None
    cov = np.empty((n_groups, m, m), dtype=np.float64) if return_moments else None
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_syn_loglik", _lib.ptr(X), n_groups, n, m, m, _lib.ptr(y), _lib.ptr(W), code, _lib.ptr(g),
             _lib.ptr(pre), 0 if pre is None else K, _lib.ptr(pen), P, _lib.ptr(ll), _lib.ptr(mean), _lib.ptr(cov))
    ll = _squeeze(ll, keep_group_axis, prefixes, penalties)
    return (ll, mean, cov) if return_moments else ll


def semi_loglik(ssx, ssy, n_groups=1, shrinkage=None, penalty=None, prefixes=None, penalties=None, return_parts=False,
                ctx=None):
    """Semiparametric synthetic log-likelihoods (semiBSL: a kernel density estimate per summary, a Gaussian copula with
    the Gaussian rank correlation) of `n_groups` groups of simulated summaries in one device call.

    ssx, ssy, n_groups, shrinkage ('warton': rho -> (1 - penalty) rho + penalty I), penalty / penalties, prefixes and the
    shape of the result: as syn_loglik.  A group has 2 to MAX_SEMI_ROWS rows.  -inf where ssy lies outside the reach of a
    column's density estimate (its integral is 0 or 1), where a column has no spread or the correlation matrix no
    Cholesky factor.  With return_parts: (loglik, u (G, m), rho (G, m, m), scores (G, n, m)) of the full groups -- the
    integrals of the density estimates up to ssy, the rank correlation before shrinkage, the normal scores of the rows.
    """
    X, y, n_groups, n, m, keep_group_axis = _groups(ssx, ssy, n_groups)
    if n > MAX_SEMI_ROWS:
        raise ValueError('%d rows per group: the semiparametric kernel takes 2 to %d' % (n, MAX_SEMI_ROWS))
    pen = _penalty_list(shrinkage, penalty, penalties)
    pre = _prefix_list(prefixes, n)
    X = np.ascontiguousarray(X)
    K = 1 if pre is None else pre.size
    P = 0 if pen is None else pen.size
    ll = np.empty((n_groups, K, max(P, 1)), dtype=np.float64)
    u = np.empty((n_groups, m), dtype=np.float64) if return_parts else None
    rho = np.empty((n_groups, m, m), dtype=np.float64) if return_parts else None
    scores = np.empty((n_groups, n, m), dtype=np.float64) if return_parts else None
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_semi_loglik", _lib.ptr(X), n_groups, n, m, m, _lib.ptr(y), _lib.ptr(pre), 0 if pre is None else K,
             _lib.ptr(pen), P, _lib.ptr(ll), _lib.ptr(u), _lib.ptr(rho), _lib.ptr(scores))
    ll = _squeeze(ll, keep_group_axis, prefixes, penalties)
    return (ll, u, rho, scores) if return_parts else ll


# ---- the reference's likelihood callables (pdf_methods.py:77-135, 138-176, 267-316) ----------------------------------

def gaussian_syn_likelihood(ssx, ssy, shrinkage=None, penalty=None, whitening=None):
    """Standard synthetic log-likelihood of one (n, m) summary matrix; np.array([ll]) as the reference returns."""
    return np.array([syn_loglik(np.asarray(ssx, dtype=np.float64).reshape(len(ssx), -1), ssy, shrinkage=shrinkage,
                                penalty=penalty, whitening=whitening)])


def gaussian_syn_likelihood_ghurye_olkin(ssx, ssy):
    """The unbiased estimator of the synthetic likelihood (Ghurye & Olkin); np.array([ll])."""
    return np.array([syn_loglik(np.asarray(ssx, dtype=np.float64).reshape(len(ssx), -1), ssy, variant='unbiased')])


def syn_likelihood_misspec(ssx, ssy, gamma, adjustment):
    """Mean- or variance-adjusted synthetic log-likelihood (Frazier & Drovandi); a scalar."""
    return syn_loglik(np.asarray(ssx, dtype=np.float64).reshape(len(ssx), -1), ssy, gamma=gamma, adjustment=adjustment)


def semi_param_kernel_estimate(ssx, ssy, shrinkage=None, penalty=None, whitening=None):
    """Semiparametric synthetic log-likelihood of one (n, m) summary matrix; np.array([ll]), the shape of the other
    device callables (the reference's own return is a (1, 1, 1) array that BSL only adds to a scalar)."""
    if whitening is not None:
        raise NotImplementedError('the whitened semiparametric likelihood (wsemiBSL) is not on the device')
    return np.array([semi_loglik(np.asarray(ssx, dtype=np.float64).reshape(len(ssx), -1), ssy, shrinkage=shrinkage,
                                 penalty=penalty)])


def standard_likelihood(shrinkage=None, penalty=None, whitening=None):
    """pdf_methods.standard_likelihood on the device (Warton shrinkage or none)."""
    if shrinkage == 'glasso':
        raise NotImplementedError("graphical-lasso shrinkage is not on the device; shrinkage='warton' is")
    if shrinkage not in (None, 'warton'):
        raise ValueError('unknown shrinkage %r' % (shrinkage,))
    return partial(gaussian_syn_likelihood, shrinkage=shrinkage, penalty=penalty, whitening=whitening)


def semiparametric_likelihood(shrinkage=None, penalty=None, whitening=None):
    """pdf_methods.semiparametric_likelihood on the device (Warton shrinkage of the correlation matrix or none)."""
    if shrinkage == 'glasso':
        raise NotImplementedError("graphical-lasso shrinkage is not on the device; shrinkage='warton' is")
    if shrinkage not in (None, 'warton'):
        raise ValueError('unknown shrinkage %r' % (shrinkage,))
    if whitening is not None:
        raise NotImplementedError('the whitened semiparametric likelihood (wsemiBSL) is not on the device')
    return partial(semi_param_kernel_estimate, shrinkage=shrinkage, penalty=penalty, whitening=whitening)


def unbiased_likelihood():
    """pdf_methods.unbiased_likelihood on the device."""
    return gaussian_syn_likelihood_ghurye_olkin


def robust_likelihood(adjustment):
    """pdf_methods.robust_likelihood on the device: a partial with the `adjustment` keyword BSL looks for."""
    if adjustment not in ('mean', 'variance'):
        raise ValueError("adjustment must be 'mean' or 'variance', not %r" % (adjustment,))
    return partial(syn_likelihood_misspec, adjustment=adjustment)


def _likelihood_setup(likelihood, **override):
    """syn_loglik keywords of one of the callables above (None: the standard one); with semi=True: semi_loglik's."""
    kw = {}
    fn = likelihood
    if isinstance(likelihood, partial):
        fn, kw = likelihood.func, dict(likelihood.keywords)
    if fn is None or fn is gaussian_syn_likelihood:
        kw.update({k: v for k, v in override.items()})
        return dict(shrinkage=kw.get('shrinkage'), penalty=kw.get('penalty'), whitening=kw.get('whitening'))
    if fn is semi_param_kernel_estimate:
        kw.update({k: v for k, v in override.items()})
        if kw.get('whitening') is not None:
            raise NotImplementedError('the whitened semiparametric likelihood (wsemiBSL) is not on the device')
        return dict(semi=True, shrinkage=kw.get('shrinkage'), penalty=kw.get('penalty'))
    if fn is gaussian_syn_likelihood_ghurye_olkin and not override:
        return dict(variant='unbiased')
    raise TypeError('the batched evaluation takes the device likelihoods of elfi_amd (standard_likelihood(...), '
                    'semiparametric_likelihood(...), unbiased_likelihood()); got %r' % (likelihood,))


def _generate_groups(model, theta, max_sim, feature_names, M, seed):
    """(M, max_sim, m) summaries and the (m,) observed ones: repeat i is one `model.generate` call of max_sim simulations
    at theta under child seed i of SeedSequence(seed) -- the draws the reference's tools make, so the matrices are theirs."""
    names = [feature_names] if isinstance(feature_names, str) else list(feature_names)
    if isinstance(theta, dict):
        fixed = dict(theta)
    else:
        fixed = {name: value for name, value in zip(model.parameter_names, theta)}
    y = np.concatenate([np.ravel(model[name].observed) for name in names])
    groups = np.empty((M, max_sim, y.size))
    for i, child in enumerate(np.random.SeedSequence(seed).generate_state(M)):
        sims = model.generate(max_sim, outputs=names, with_values=fixed, seed=child)
        col = 0
        for name in names:
            block = np.reshape(sims[name], (max_sim, -1))
            groups[i, :, col:col + block.shape[1]] = block
            col += block.shape[1]
    return groups, y


def _prefix_axis(n_sim):
    counts = np.atleast_1d(np.asarray(n_sim)).astype(np.int64).reshape(-1)
    uniq = np.unique(counts)
    return counts, uniq, np.searchsorted(uniq, counts)


def log_SL_stdev(model, theta, n_sim, feature_names, likelihood=None, M=20, seed=None):
    """pre_sample_methods.log_SL_stdev: the standard deviation of the log synthetic likelihood for every simulation
    count of n_sim, from M repeats -- the M x len(n_sim) likelihoods in one device call."""
    setup = _likelihood_setup(likelihood)
    counts, uniq, where = _prefix_axis(n_sim)
    groups, observed = _generate_groups(model, theta, int(uniq[-1]), feature_names, M, seed)
    batched = semi_loglik if setup.pop('semi', False) else syn_loglik
    ll = batched(groups, observed, prefixes=uniq, **setup)          # (M, len(uniq))
    return np.std(np.ascontiguousarray(ll[:, where].T), axis=1)     # (len(n_sim), M), the reference's layout


def select_penalty(model, n_sim, theta, feature_names, likelihood=None, lmdas=None, M=20, sigma=1.5,
                   shrinkage='warton', whitening=None, seed=None, verbose=False):
    """pre_sample_methods.select_penalty with Warton shrinkage: for every simulation count the penalty whose log-likelihood
    standard deviation over M repeats is closest to sigma -- the M x len(n_sim) x len(lmdas) likelihoods in one call."""
    if shrinkage == 'glasso':
        raise NotImplementedError("graphical-lasso shrinkage is not on the device; shrinkage='warton' is")
    if shrinkage != 'warton':
        raise ValueError('unknown shrinkage %r' % (shrinkage,))
    setup = _likelihood_setup(likelihood, shrinkage=shrinkage, whitening=whitening)
    if lmdas is None:
        lmdas = list(np.arange(0.2, 0.8, 0.02))
    counts, uniq, where = _prefix_axis(n_sim)
    groups, observed = _generate_groups(model, theta, int(uniq[-1]), feature_names, M, seed)
    setup.pop('penalty', None)
    batched = semi_loglik if setup.pop('semi', False) else syn_loglik
    logliks = batched(groups, observed, prefixes=uniq, penalties=lmdas, **setup)        # (M, len(uniq), len(lmdas))
    spread = logliks.std(axis=0)[where]                    # over the repeats: (len(n_sim), len(lmdas))
    pick = np.abs(spread - sigma).argmin(axis=1)           # ties go to the smaller penalty index, as argmin does
    if verbose:
        print('log-likelihoods (repeat, simulation count, penalty):', logliks[:, where], sep='\n')
        print('standard deviations (simulation count, penalty):', spread, sep='\n')
    return np.asarray(lmdas, dtype=float)[pick], spread[np.arange(len(pick)), pick]


# ---- the slice samplers for gamma (slice_gamma_mean.py:35-138, slice_gamma_variance.py:31-115) ------------------------

_ADJUSTMENTS = {'mean': 0, 'variance': 1}
SLICE_OK, SLICE_OUT_OF_DRAWS, SLICE_NONFINITE = 0, 1, 2
MAX_SLICE_ITER = 1 << 20


def slice_gamma(ssy, loglik, gamma, sample_mean, sample_cov, adjustment, tau=0.5, w=1.0, max_iter=1000, draws=None,
                seed=None, n_groups=None, return_info=False, ctx=None):
    """One slice-sampler sweep over the m adjustment parameters of every one of G chains' states in one device call
    (`elfihip_slice_gamma`, csrc/slice_gamma.hip: one wavefront per chain).

    gamma (G, m), loglik (G), sample_mean (G, m), sample_cov (G, m, m); ssy (G, m) or (m) for all; without the leading
    axis (and n_groups None): one problem.  adjustment: 'mean' | 'variance'.
    draws: (G, n_u) (or (n_u) for one problem) doubles in [0, 1), consumed in the reference's order -- one per exponential,
    one per uniform; or seed: the device generator's (Philox stream SLICE_GAMMA_STREAM_BASE + the chain's position).
    Returns (gamma, loglik) -- a problem that ran out of draws or met a non-finite value has NaN -- and with return_info
    also (used, evals, status): the draws consumed, the likelihood evaluations and SLICE_OK / SLICE_OUT_OF_DRAWS /
    SLICE_NONFINITE per problem.
    """
    if adjustment not in _ADJUSTMENTS:
        raise ValueError("adjustment must be 'mean' or 'variance', not %r" % (adjustment,))
    g_in = np.asarray(gamma, dtype=np.float64)
    single = g_in.ndim <= 1 and n_groups is None
    g_in = np.ascontiguousarray(np.atleast_2d(g_in))
    if g_in.ndim != 2:
        raise ValueError('gamma must be (m) or (G, m)')
    G, m = g_in.shape
    if n_groups is not None and int(n_groups) != G:
        raise ValueError('n_groups=%d but gamma has %d rows' % (n_groups, G))
    if m < 1 or m > MAX_FEATURES:
        raise ValueError('%d adjustment parameters: the device kernel takes 1 to %d' % (m, MAX_FEATURES))
    try:
        y = np.ascontiguousarray(np.broadcast_to(np.asarray(ssy, dtype=np.float64).reshape((-1, m)), (G, m)))
        mean = np.ascontiguousarray(np.asarray(sample_mean, dtype=np.float64).reshape((G, m)))
        cov = np.ascontiguousarray(np.asarray(sample_cov, dtype=np.float64).reshape((G, m, m)))
        ll = np.ascontiguousarray(np.asarray(loglik, dtype=np.float64).reshape((G,)))
    except ValueError:
        raise ValueError('ssy, loglik, sample_mean and sample_cov do not have the shapes of %d problems of %d '
                         'parameters' % (G, m)) from None
    tau, w, max_iter = float(tau), float(w), int(max_iter)
    if not (tau > 0 and np.isfinite(tau)):
        raise ValueError('tau must be positive')
    if not (w > 0 and np.isfinite(w)):
        raise ValueError('w must be positive')
    if max_iter < 0 or max_iter > MAX_SLICE_ITER:
        raise ValueError('max_iter=%d: 0 to %d' % (max_iter, MAX_SLICE_ITER))
    if (draws is None) == (seed is None):
        raise ValueError('give either draws or seed')
    U, n_u = None, 0
    if draws is not None:
        U = np.asarray(draws, dtype=np.float64)
        if U.ndim == 1 and G == 1:
            U = U.reshape(1, -1)
        if U.ndim != 2 or U.shape[0] != G:
            raise ValueError('draws must be (G, n_u)')
        U = np.ascontiguousarray(U)
        n_u = U.shape[1]
    g_out = np.empty((G, m), dtype=np.float64)
    ll_out = np.empty(G, dtype=np.float64)
    used, evals = np.empty(G, dtype=np.int64), np.empty(G, dtype=np.int64)
    status = np.empty(G, dtype=np.int32)
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_slice_gamma", _ADJUSTMENTS[adjustment], G, m, _lib.ptr(y), _lib.ptr(mean), _lib.ptr(cov), m,
             _lib.ptr(g_in), _lib.ptr(ll), tau, w, max_iter, _lib.ptr(U), n_u, C.c_uint64(0 if seed is None else int(seed)),
             C.c_uint64(SLICE_GAMMA_STREAM_BASE), _lib.ptr(g_out), _lib.ptr(ll_out), _lib.ptr(used), _lib.ptr(evals),
             _lib.ptr(status))
    if single:
        g_out, ll_out, used, evals, status = g_out[0], ll_out[0], int(used[0]), int(evals[0]), int(status[0])
    return (g_out, ll_out, used, evals, status) if return_info else (g_out, ll_out)


def _first_draws(m):
    """Length of the first draw buffer of the drop-ins: a coordinate takes one exponential and, typically, a few uniforms."""
    return 8 * m + 16


def _slice_gamma_drop_in(adjustment, ssy, loglik, gamma, sample_mean, sample_cov, tau, w, max_iter, random_state):
    """The reference's call on the device, with the caller's generator kept on the reference's sequence: the draws are a
    buffer of its random_sample doubles, and afterwards the generator has consumed exactly the doubles the sweep used."""
    rs = np.random if random_state is None else random_state
    g_in = np.asarray(gamma, dtype=np.float64).reshape(-1)
    ll_in = np.asarray(loglik, dtype=np.float64).reshape(-1)
    if ll_in.size != 1:
        raise ValueError('loglik must be one number')
    saved = rs.get_state()
    n_u, most = _first_draws(g_in.size), g_in.size * (1 + max(int(max_iter), 0))
    while True:
        rs.set_state(saved)
        n_u = max(1, min(n_u, most))
        try:
            g_out, ll_out, used, _, status = slice_gamma(ssy, ll_in, g_in, sample_mean, sample_cov, adjustment, tau=tau, w=w,
                                                         max_iter=max_iter, draws=rs.random_sample(n_u), return_info=True)
        finally:
            rs.set_state(saved)
        if status != SLICE_OUT_OF_DRAWS or n_u >= most:
            break
        n_u *= 4         # the longer buffer starts with the same doubles, so the sweep repeats its steps and goes on
    rs.random_sample(used)
    if status != SLICE_OK:
        raise FloatingPointError('the %s-adjustment slice sampler met a covariance without a Cholesky factor or a target '
                                 'that is not finite' % adjustment)
    return g_out, np.float64(ll_out)


def slice_gamma_mean(ssy, loglik, gamma, sample_mean, sample_cov, tau=0.5, w=1.0, max_iter=1000, random_state=None):
    """slice_gamma_mean.slice_gamma_mean on the device: (gamma, loglik) after one sweep; random_state (None: NumPy's
    global one) ends where the reference's would."""
    return _slice_gamma_drop_in('mean', ssy, loglik, gamma, sample_mean, sample_cov, tau, w, max_iter, random_state)


def slice_gamma_variance(ssy, loglik, gamma, sample_mean, sample_cov, tau=0.5, w=1.0, max_iter=1000, random_state=None):
    """slice_gamma_variance.slice_gamma_variance on the device; as slice_gamma_mean."""
    return _slice_gamma_drop_in('variance', ssy, loglik, gamma, sample_mean, sample_cov, tau, w, max_iter, random_state)


# ---- elfi.BSL with the device likelihood as its default ----------------------------------------------------------------

def _reference_bsl():
    mod = sys.modules.get('elfi.methods.inference.bsl')
    if mod is None:
        raise ImportError("HipBSL subclasses the running program's elfi.BSL: `import elfi` first")
    return mod.BSL


def hip_bsl_class():
    """The subclass of the imported ELFI's BSL (made once per reference class): the loop, the proposals and the BslSample
    are the reference's; the default likelihood is the device one, and with gamma_sampler='device' a robust chain's
    gamma sweeps are too (the default, None, keeps the reference's slice samplers)."""
    BSL = _reference_bsl()
    cls = _CLASSES.get(BSL)
    if cls is not None:
        return cls

    class HipBSL(BSL):
        __doc__ = hip_bsl_class.__doc__

        def __init__(self, model, n_sim_round, feature_names=None, likelihood=None, gamma_sampler=None, **kwargs):
            if gamma_sampler not in (None, 'device'):
                raise ValueError("gamma_sampler must be None (the reference's slice samplers) or 'device', not %r"
                                 % (gamma_sampler,))
            if gamma_sampler == 'device' and not (isinstance(likelihood, partial) and 'adjustment' in likelihood.keywords):
                raise ValueError("gamma_sampler='device' goes with a robust likelihood (robust_likelihood('mean' | "
                                 "'variance')): no other has adjustment parameters to sample")
            super(HipBSL, self).__init__(model, n_sim_round, feature_names=feature_names,
                                         likelihood=likelihood or standard_likelihood(), **kwargs)
            self.gamma_sampler_choice = gamma_sampler

        def _resolve_gamma_sampler(self, tau, w, max_iter):
            sampler, gamma0 = super(HipBSL, self)._resolve_gamma_sampler(tau, w, max_iter)
            if self.gamma_sampler_choice == 'device':
                sampler = {'mean': slice_gamma_mean, 'variance': slice_gamma_variance}[self.likelihood.keywords['adjustment']]
                sampler = partial(sampler, tau=tau, w=w, max_iter=max_iter, random_state=self.random_state)
            return sampler, gamma0

    HipBSL.__name__ = 'HipBSL'
    HipBSL.__qualname__ = 'HipBSL'
    _CLASSES[BSL] = HipBSL
    return HipBSL


def HipBSL(model, n_sim_round, **kwargs):
    """elfi.BSL(model, n_sim_round, feature_names=None, likelihood=None, ...) with the synthetic likelihood on the GPU."""
    return hip_bsl_class()(model, n_sim_round, **kwargs)
