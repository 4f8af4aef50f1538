"""Summary-statistic selection (Nunes & Balding 2010) on the GPU: elfi.methods.diagnostics.TwoStageSelection with its
data-parallel steps on the device.

    sel = elfi_amd.HipTwoStageSelection(model['MA2'], 'euclidean', list_ss=[ac1, ac2, mean, var])     # nothing in ELFI edited
    best = sel.run(n_sim=20000, n_acc=500, n_closest=20, batch_size=5000)                            # the reference's tuple

`knn_entropy`, `mrsse` and `subset_best` are the thin mirrors of `elfihip_knn_entropy`, `elfihip_mrsse` and
`elfihip_subset_best` (csrc/twostage.hip): the k-th-nearest-neighbour entropy (diagnostics.py:214-253) and the mean root
sum of squared errors (:255-289) of G groups of accepted parameters in one launch each, and the best rows of every
candidate combination of summary columns from ONE pool of simulations.

`HipTwoStageSelection.run` simulates once: the reference runs one `elfi.Rejection` per combination over a shared pool
(:172-212), so every run reads the same simulations and differs only in the columns its distance sums.  Here one
`elfi.Rejection` with every distinct candidate as a Summary fills a pool of parameters and summaries; the per-combination
selection, the entropies and the MRSSEs are one device call each.  No random generator is modelled: the draws are ELFI's.

Not on the device: metrics other than 'euclidean', callable discrepancies, k > 16, more than 32 parameters.
They raise; nothing falls back quietly.
"""
import logging
import sys

import numpy as np

from . import _lib

MAX_DIM = 32            # parameters (q) of knn_entropy / mrsse
MAX_NEIGHBOUR = 16      # k of knn_entropy
_CLASSES = {}

logger = logging.getLogger(__name__)


def _point_groups(thetas, n_groups, what='thetas'):
    """(T (n_groups n, q) contiguous, n_groups, n, q, keep_group_axis) of the two layouts the points may have."""
    T = np.asarray(thetas, dtype=np.float64)
    keep_group_axis = T.ndim == 3 or n_groups != 1
    if T.ndim == 3:
        if n_groups not in (1, T.shape[0]):
            raise ValueError('n_groups=%d but %s has %d groups' % (n_groups, what, T.shape[0]))
        n_groups = T.shape[0]
        T = T.reshape(-1, T.shape[2])
    if T.ndim != 2:
        raise ValueError('%s must be 2d (rows of parameters) or 3d (groups of rows)' % what)
    n_groups = int(n_groups)
    rows, q = T.shape
    if n_groups < 1 or rows % n_groups:
        raise ValueError('%d rows do not divide into %d groups' % (rows, n_groups))
    n = rows // n_groups
    if n < 1:
        raise ValueError('a group needs at least one row')
    if q < 1 or q > MAX_DIM:
        raise ValueError('%d parameters: the device kernels take 1 to %d' % (q, MAX_DIM))
    return np.ascontiguousarray(T), n_groups, n, q, keep_group_axis


def knn_entropy(thetas, k=4, n_groups=1, return_kth=False, ctx=None):
    """The k-th-nearest-neighbour entropy estimate of `n_groups` groups of parameters in one device call
    (TwoStageSelection._calc_entropy, diagnostics.py:214-253):

        E = log(pi^(q/2) / Gamma(q/2 + 1)) - psi(k) + log n + (q / n) sum_i log R_ik

    thetas: (n_groups * n, q), group g = rows g n ... g n + n - 1, or (n_groups, n, q).  R_ik is the reference's
    cKDTree.query(theta_i, k)[0][-1]: the point itself is its first neighbour, so k = 1 (or k coincident points) gives
    -inf and k > n gives +inf.  1 <= k <= 16, q <= 32.
    Returns an array (n_groups); a float for one group given as a 2-d array.  With return_kth: (E, R (n_groups, n) --
    (n,) for that single group).
    """
    T, n_groups, n, q, keep_group_axis = _point_groups(thetas, n_groups)
    if int(k) != k or k < 1 or k > MAX_NEIGHBOUR:
        raise ValueError('k=%r: the device kernel takes 1 to %d' % (k, MAX_NEIGHBOUR))
    E = np.empty(n_groups, dtype=np.float64)
    kth = np.empty((n_groups, n), dtype=np.float64) if return_kth else None
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_knn_entropy", _lib.ptr(T), n_groups, n, q, q, int(k), _lib.ptr(E), _lib.ptr(kth))
    if not keep_group_axis:
        E = float(E[0])
        kth = kth[0] if return_kth else None
    return (E, kth) if return_kth else E


def mrsse(thetas, closest, n_groups=1, ctx=None):
    """The mean root sum of squared errors of `n_groups` groups of accepted parameters against the J `closest` parameters
    (TwoStageSelection._calc_MRSSE, diagnostics.py:255-289): (1 / J) sum_j sqrt(sum_{i,d} (thetas[g, i, d] - closest[j, d])^2).

    thetas as for knn_entropy; closest (J, q).  Returns an array (n_groups); a float for one group given as a 2-d array.
    """
    T, n_groups, n, q, keep_group_axis = _point_groups(thetas, n_groups)
    Cl = np.asarray(closest, dtype=np.float64)
    if Cl.ndim == 1:
        Cl = Cl.reshape(1, -1)
    if Cl.ndim != 2 or Cl.shape[1] != q or Cl.shape[0] < 1:
        raise ValueError('closest must be (J, %d) with J >= 1, not %r' % (q, Cl.shape))
    if Cl.shape[0] > 65535:
        raise ValueError('%d closest parameters: the device kernel takes at most 65535' % Cl.shape[0])
    Cl = np.ascontiguousarray(Cl)
    out = np.empty(n_groups, dtype=np.float64)
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_mrsse", _lib.ptr(T), n_groups, n, q, q, _lib.ptr(Cl), Cl.shape[0], q, _lib.ptr(out))
    return out if keep_group_axis else float(out[0])


def subset_best(X, y, masks, k, ctx=None):
    """The k rows of X (n, m) nearest to y (m) under every 0/1 column mask of `masks` (C, m), euclidean over the selected
    columns: what one Rejection per combination accepts from the same pool of simulations.

    Returns (vals (C, min(k, n)), rows (C, min(k, n)) int64), ascending by (distance, row), NaN last.  The distances are
    `nested_weighted_euclidean(X, y, masks)` bit for bit, so a non-finite value in an unselected column gives the row
    0 * inf = NaN: it ranks last.  A mask entry other than 0 or 1 and an all-zero mask are errors.
    """
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError('X must be a non-empty 2d array (rows of summaries)')
    n, m = X.shape
    y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
    if y.shape != (m,):
        raise ValueError('y has %d entries, X has %d columns' % (y.size, m))
    M = np.asarray(masks, dtype=np.float64)
    if M.ndim == 1:
        M = M.reshape(1, -1)
    if M.ndim != 2 or M.shape[1] != m or M.shape[0] < 1:
        raise ValueError('masks must be (C, %d) with C >= 1, not %r' % (m, M.shape))
    if not np.all((M == 0.0) | (M == 1.0)):
        raise ValueError('a mask holds 0 and 1 only')
    if not np.all(M.any(axis=1)):
        raise ValueError('mask %d selects no column' % int(np.flatnonzero(~M.any(axis=1))[0]))
    if int(k) != k or k < 1:
        raise ValueError('k=%r must be a positive integer' % (k,))
    X, M = np.ascontiguousarray(X), np.ascontiguousarray(M)
    ke = min(int(k), n)
    vals = np.empty((M.shape[0], ke), dtype=np.float64)
    rows = np.empty((M.shape[0], ke), dtype=np.int64)
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_subset_best", _lib.ptr(X), n, m, m, _lib.ptr(y), _lib.ptr(M), M.shape[0], int(k), _lib.ptr(vals),
             _lib.ptr(rows))
    return vals, rows


# ---- elfi.methods.diagnostics.TwoStageSelection with one simulation pass ------------------------------------------------

def _reference_two_stage():
    mod = sys.modules.get('elfi.methods.diagnostics')
    if mod is None:
        raise ImportError("HipTwoStageSelection subclasses the running program's TwoStageSelection: "
                          "`import elfi.methods.diagnostics` first")
    return mod.TwoStageSelection


def _check_distance(fn_distance):
    if not isinstance(fn_distance, str):
        raise NotImplementedError("a callable discrepancy is not on the device; fn_distance='euclidean' is")
    if fn_distance != 'euclidean':
        raise NotImplementedError("fn_distance=%r is not on the device; 'euclidean' is" % (fn_distance,))


def _candidate_layout(ss_candidates):
    """(distinct statistics in order of first appearance, per combination the indices into that list).  A combination
    must list its statistics once each and in that common order: the subset distance sums its columns left to right, and
    only then are its bits those of the reference's distance over the combination's own columns."""
    distinct, index = [], []
    for set_ss in ss_candidates:
        where = []
        for ss in set_ss:
            pos = next((i for i, s in enumerate(distinct) if s is ss), None)
            if pos is None:
                pos = len(distinct)
                distinct.append(ss)
            where.append(pos)
        if len(where) < 1:
            raise ValueError('an empty summary-statistics combination')
        if any(b <= a for a, b in zip(where, where[1:])):
            raise NotImplementedError('the device selection takes combinations that list their statistics once each and '
                                      'in one common order; %s does not' % ([ss.__name__ for ss in set_ss],))
        index.append(where)
    return distinct, index


def hip_two_stage_selection_class():
    """The subclass of the imported ELFI's TwoStageSelection (made once per reference class): the constructor, the
    combinations, the defaults, the log lines and the tie rules are the reference's; the simulations run once and the
    selection, the entropies and the MRSSEs are device calls."""
    Ref = _reference_two_stage()
    cls = _CLASSES.get(Ref)
    if cls is not None:
        return cls
    import elfi

    class HipTwoStageSelection(Ref):
        __doc__ = hip_two_stage_selection_class.__doc__

        def _simulate(self, n_sim, n_acc, batch_size):
            """One pass of the reference's Rejection with every distinct candidate as a Summary: (theta (N, q), X (N, m),
            observed (m), masks (C, m)), the pool's batches stacked in batch order."""
            distinct, index = _candidate_layout(self.ss_candidates)
            m = self.simulator.model.copy()
            nodes = [elfi.Summary(ss, m[self.simulator.name], model=m) for ss in distinct]
            d = elfi.Distance('euclidean', *nodes, model=m)
            params, names = list(m.parameter_names), [node.name for node in nodes]
            pool = elfi.OutputPool(params + names)
            sampler = elfi.Rejection(d, batch_size=batch_size, seed=self.seed, pool=pool, output_names=params + names)
            sampler.sample(n_acc, n_sim=n_sim)
            batches = [pool.get_batch(b, params + names) for b in range(len(pool))]

            def stacked(name):
                return np.concatenate([np.reshape(batch[name], (len(batch[name]), -1)) for batch in batches])
            theta = np.column_stack([stacked(name) for name in params])
            blocks = [stacked(name) for name in names]
            observed = [np.reshape(m[name].observed, -1) for name in names]
            widths = [blk.shape[1] for blk in blocks]
            starts = np.concatenate([[0], np.cumsum(widths)])
            masks = np.zeros((len(index), int(starts[-1])))
            for c, where in enumerate(index):
                for pos in where:
                    masks[c, starts[pos]:starts[pos + 1]] = 1.0
            return theta, np.column_stack(blocks), np.concatenate(observed), masks

        def run(self, n_sim, n_acc=None, n_closest=None, batch_size=1, k=4):
            """TwoStageSelection.run (diagnostics.py:103-170) with the reference's defaults, errors, log lines and tie rules.
            After it, `entropies_`, `mrsses_` (one value per combination) and `accepted_` (C, n_acc, q) hold what the two
            stages compared."""
            _check_distance(self.fn_distance)
            if n_acc is None:
                n_acc = int(n_sim / 100)
            if n_closest is None:
                n_closest = int(n_acc / 100)
            if n_sim < n_acc or n_acc < n_closest or n_closest == 0:
                raise ValueError("The number of simulations is too small.")
            if int(k) != k or k < 1 or k > MAX_NEIGHBOUR:
                raise ValueError('k=%r: the device kernel takes 1 to %d' % (k, MAX_NEIGHBOUR))

            theta, X, observed, masks = self._simulate(n_sim, n_acc, batch_size)
            _, rows = subset_best(X, observed, masks, n_acc)
            accepted = theta[rows]                                   # (C, n_acc, q), each in the sampler's order
            entropies = knn_entropy(accepted, k=k)
            self.entropies_, self.accepted_ = entropies, accepted

            E_me = np.inf
            names_ss_me = []
            thetas_closest = None
            for c, set_ss in enumerate(self.ss_candidates):
                names_ss = [ss.__name__ for ss in set_ss]
                E_ss = entropies[c]
                # If equal, dismiss the combination which contains uninformative summary statistics.
                if (E_ss == E_me and (len(names_ss_me) > len(names_ss))) or E_ss < E_me:
                    E_me = E_ss
                    names_ss_me = names_ss
                    thetas_closest = accepted[c, :n_closest]
                logger.info('Combination %s shows the entropy of %f' % (names_ss, E_ss))
            logger.info('\nThe minimum entropy of %f was found in %s.\n' % (E_me, names_ss_me))
            self.names_min_entropy_ = names_ss_me
            if thetas_closest is None:     # (the reference fails here with an unbound name: every entropy is +inf or NaN)
                raise ValueError('no combination has a finite entropy (n_acc=%d, k=%d)' % (n_acc, k))

            errors = mrsse(accepted, thetas_closest)
            self.mrsses_ = errors
            MRSSE_min = np.inf
            names_ss_MRSSE = []
            set_ss_2stage = None
            for c, set_ss in enumerate(self.ss_candidates):
                names_ss = [ss.__name__ for ss in set_ss]
                MRSSE_ss = errors[c]
                # If equal, dismiss the combination which contains uninformative summary statistics.
                if (MRSSE_ss == MRSSE_min and (len(names_ss_MRSSE) > len(names_ss))) or MRSSE_ss < MRSSE_min:
                    MRSSE_min = MRSSE_ss
                    names_ss_MRSSE = names_ss
                    set_ss_2stage = set_ss
                logger.info('Combination %s shows the MRSSE of %f' % (names_ss, MRSSE_ss))
            logger.info('\nThe minimum MRSSE of %f was found in %s.' % (MRSSE_min, names_ss_MRSSE))
            self.names_min_mrsse_ = names_ss_MRSSE
            return set_ss_2stage

    HipTwoStageSelection.__name__ = 'HipTwoStageSelection'
    HipTwoStageSelection.__qualname__ = 'HipTwoStageSelection'
    _CLASSES[Ref] = HipTwoStageSelection
    return HipTwoStageSelection


def HipTwoStageSelection(simulator, fn_distance, list_ss=None, prepared_ss=None, max_cardinality=4, seed=0):
    """elfi.methods.diagnostics.TwoStageSelection(simulator, fn_distance, ...) with one simulation pass and the selection,
    the entropies and the MRSSEs on the GPU.  fn_distance must be 'euclidean'."""
    _check_distance(fn_distance)
    return hip_two_stage_selection_class()(simulator, fn_distance, list_ss=list_ss, prepared_ss=prepared_ss,
                                           max_cardinality=max_cardinality, seed=seed)
