"""ROMC (Robust Optimisation Monte Carlo, Ikonomov & Gutmann 2019) on the GPU for the device MA2 model.

    romc = elfi_amd.HipROMC(elfi_amd.ma2_model(seed_obs=4), bounds=[(-2, 2), (-1.25, 1.25)], discrepancy_name='d')
    romc.solve_problems(n1=500, seed=21)              # ONE launch: 500 Nelder-Mead runs and their Hessians
    romc.estimate_regions(eps_filter=romc.compute_eps(.75), fit_models=False)     # ONE launch: 2000 line searches
    romc.sample(n2=100)                               # ONE launch: the points and their distances
    romc.eval_posterior(grid)                         # ONE launch per call: BS x n1 indicator evaluations

ROMC freezes the simulator's noise into n1 deterministic objectives f_i(theta) = d_i(theta)^2.  The reference
(elfi/methods/inference/romc.py, RomcPosterior in elfi/methods/posteriors.py) makes every evaluation with a
model.generate(batch_size=1, seed=nuisance_i) call; here problem i's noise is one (seed, stream) pair of the device
generator and lives in a matrix the handle keeps on the device (csrc/romc.hip, the statements in include/elfihip.h and
tests/romc_ref.py).

`RomcProblems` owns that handle; `romc_objective`, `romc_solve`, `romc_regions`, `romc_sample` and `romc_count` are the
batched calls on it, for users with their own loop.

`HipROMC` is a subclass of the imported ELFI's ROMC that overrides _solve_gradients, _build_boxes and _define_posterior.
Problem i's (seed, stream) pair is the one the model's own simulator would use under model.generate(batch_size=1,
with_values=..., seed=int(nuisance_i)): seed = one randint of RandomState(get_sub_seed(nuisance_i, 0)), stream =
SIMULATOR_STREAM_BASE.  So f_i is the reference's _det_generator on this model, up to one ulp: the rule here is d d,
the reference's float(d) ** 2 goes through libm's pow.  self.optim_problems holds the reference's own OptimisationProblem,
RomcOptimisationResult and NDimBoundingBox objects (state flags, result, regions, initial_point; objective stays the
reference's _freeze_seed partial), so compute_eps, _filter_solutions, extract_result, visualize_region, distance_hist,
compute_ess, compute_divergence and result run as the reference's code.

Differences, all decided:
  * the start points are prior.rvs(size=n1, random_state=seed) drawn ONCE; the reference redraws all n1 for every problem
    and takes row `ind` -- the same values;
  * the Hessian is a central second difference (the reference: numdifftools), the rotation a Jacobi rotation (the
    reference: numpy.linalg.eig) -- the same box up to the order and sign of the eigenvectors;
  * `HipRomcPosterior.sample` weighs w = 1[f < eps] prior / q with q = 1 / volume: a drawn point is inside its box by
    construction, the reference re-tests containment through rotation_inv (a difference of measure zero);
  * the sample uniforms are the device generator's (one Philox stream per region above ROMC_STREAM_BASE).

What stays the reference's: use_bo=True (GP surrogates) and fit_models=True (local quadratic surrogates) exist to avoid
simulator calls that now cost nothing; they run the reference's own methods on these objects, and `HipRomcPosterior` takes
the reference's path whenever a surrogate is in use.  A model other than ma2_model, custom_optim_class, or optimiser
arguments other than seed / x0 raise NotImplementedError.
"""
import ctypes as C
import sys
from functools import partial

import numpy as np

from . import _lib
from .priors import ROMC_STREAM_BASE, SIMULATOR_STREAM_BASE

DIM = 2
MAX_OBS = 126
MAX_PROBLEMS = 1 << 20
MAX_POINTS = 1 << 24
MODEL_MA2 = 0
SOLVED, MAXFEV, MAXITER, NONFINITE = range(4)
_NO_LIMIT = 2 ** 31 - 1
_CLASSES = {}


def _call(ctx, name, *args):
    rc = getattr(ctx.lib, name)(*args)
    if rc != _lib.OK:
        _lib._raise(ctx.lib, ctx.handle, rc)


def _points(a, name, cols=DIM):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1 and a.size == cols:
        a = a.reshape(1, cols)
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError('%s must have shape (n, %d), got %r' % (name, cols, a.shape))
    return np.ascontiguousarray(a)


def _index(prob, n1, count=None, name='prob'):
    p = np.asarray(prob)
    if p.size and not np.issubdtype(p.dtype, np.integer):
        raise ValueError('%s must hold integer problem indices' % name)
    p = np.ascontiguousarray(p.reshape(-1).astype(np.int64))
    if count is not None and p.shape[0] != count:
        raise ValueError('%s has %d entries for %d rows' % (name, p.shape[0], count))
    if p.size and (p.min() < 0 or p.max() >= n1):
        raise ValueError('%s holds an index outside [0, %d)' % (name, n1))
    return p


class RomcProblems:
    """n1 frozen-noise MA2 objectives on the device: f_i(theta) = d_i(theta)^2 for the noise row w_i.

    observed: the two observed summaries; n_obs: 3 to 126.  Either W (n1, n_obs + 2), the noise itself, or seeds and
    streams (n1 each; a scalar stream is broadcast): row i = normals 0 .. n_obs + 1 of stream (seeds[i], streams[i]) of
    the device generator, what ma2_draw_distance(seed=seeds[i], stream=streams[i]) simulates a single row from."""

    handle = None

    def __init__(self, n_obs, observed, W=None, seeds=None, streams=None, ctx=None):
        n_obs = int(n_obs)
        if not 3 <= n_obs <= MAX_OBS:
            raise ValueError('n_obs=%d: the device objective takes 3 to %d observations' % (n_obs, MAX_OBS))
        o = np.asarray(observed, dtype=np.float64).reshape(-1)
        if o.shape[0] != 2 or not np.all(np.isfinite(o)):
            raise ValueError('observed must hold the two finite observed summaries')
        if (W is None) == (seeds is None):
            raise ValueError('give either the noise matrix W or the (seeds, streams) pairs')
        if W is not None:
            if streams is not None:
                raise ValueError('give either the noise matrix W or the (seeds, streams) pairs')
            W = np.ascontiguousarray(np.asarray(W, dtype=np.float64))
            if W.ndim != 2 or W.shape[1] != n_obs + 2:
                raise ValueError('W must have shape (n1, n_obs + 2) = (n1, %d), got %r' % (n_obs + 2, W.shape))
            n1 = W.shape[0]
        else:
            seeds = np.ascontiguousarray(np.asarray(seeds).reshape(-1).astype(np.uint64))
            n1 = seeds.shape[0]
            streams = np.ascontiguousarray(np.broadcast_to(np.asarray(0 if streams is None else streams).astype(np.uint64), (n1,)))
        if not 1 <= n1 <= MAX_PROBLEMS:
            raise ValueError('%d problems: the device takes 1 to %d' % (n1, MAX_PROBLEMS))
        self.ctx = ctx or _lib.default_context()
        self.n1, self.n_obs, self.observed = n1, n_obs, (float(o[0]), float(o[1]))
        self.handle = None
        h = C.c_void_p()
        _call(self.ctx, 'elfihip_romc_create', self.ctx.handle, MODEL_MA2, n1, n_obs, C.c_double(o[0]), C.c_double(o[1]),
              _lib.ptr(W), _lib.ptr(seeds), _lib.ptr(streams), C.byref(h))
        self.handle = h

    def free(self):
        if self.handle is not None:
            h, self.handle = self.handle, None
            try:
                self.ctx.lib.elfihip_romc_free(h)
            except Exception:
                pass

    def __del__(self):
        self.free()

    def _h(self):
        if self.handle is None:
            raise ValueError('the problems have been freed')
        return self.handle


def romc_objective(problems, theta, prob):
    """f[p] = f_{prob[p]}(theta[p]) for P pairs in one launch; theta (P, 2), prob (P) problem indices."""
    theta = _points(theta, 'theta')
    prob = _index(prob, problems.n1, theta.shape[0])
    f = np.empty(theta.shape[0])
    _call(problems.ctx, 'elfihip_romc_objective', problems._h(), theta.shape[0], _lib.ptr(theta), _lib.ptr(prob), _lib.ptr(f))
    return f


def _limits(maxiter, maxfev):
    """SciPy's rule for the two limits of Nelder-Mead: both None -> 200 D each; one given -> the other unlimited."""
    if maxiter is None and maxfev is None:
        return 200 * DIM, 200 * DIM
    out = []
    for v, name in ((maxiter, 'maxiter'), (maxfev, 'maxfev')):
        if v is None or v == np.inf:
            out.append(_NO_LIMIT)
        elif int(v) != v or int(v) < 1:
            raise ValueError('%s must be a positive integer' % name)
        else:
            out.append(min(int(v), _NO_LIMIT))
    if min(out) > 1 << 20:
        raise ValueError('the smaller of maxiter and maxfev bounds the search: at most 2^20')
    return tuple(out)


def romc_solve(problems, x0, maxiter=None, maxfev=None):
    """Every problem's Nelder-Mead minimum from its start x0 (n1, 2), as scipy.optimize.minimize(method='Nelder-Mead') finds it,
    and the difference Hessian there; one launch.  Returns a dict: x_min (n1, 2), f_min (n1), hess (n1, 2, 2), nfev, nit,
    status (n1: SOLVED, MAXFEV, MAXITER, NONFINITE); hess is NaN where the status is not SOLVED."""
    x0 = _points(x0, 'x0')
    n1 = problems.n1
    if x0.shape[0] != n1:
        raise ValueError('x0 has %d rows for %d problems' % (x0.shape[0], n1))
    maxiter, maxfev = _limits(maxiter, maxfev)
    out = dict(x_min=np.empty((n1, DIM)), f_min=np.empty(n1), hess=np.empty((n1, DIM, DIM)), nfev=np.empty(n1, dtype=np.int32),
               nit=np.empty(n1, dtype=np.int32), status=np.empty(n1, dtype=np.int32))
    _call(problems.ctx, 'elfihip_romc_solve', problems._h(), _lib.ptr(x0), maxiter, maxfev, _lib.ptr(out['x_min']),
          _lib.ptr(out['f_min']), _lib.ptr(out['hess']), _lib.ptr(out['nfev']), _lib.ptr(out['nit']), _lib.ptr(out['status']))
    return out


def _search_args(eps_region, K, eta, rep_lim):
    eps_region, eta = float(eps_region), float(eta)
    if int(K) != K or not 1 <= int(K) <= 64:
        raise ValueError('K=%r refinements: 1 to 64' % (K,))
    if int(rep_lim) != rep_lim or not 0 <= int(rep_lim) <= 1 << 20:
        raise ValueError('rep_lim=%r: 0 to 2^20' % (rep_lim,))
    if not (eta > 0 and np.isfinite(eta)):
        raise ValueError('the step eta must be positive and finite')
    if np.isnan(eps_region):
        raise ValueError('eps_region is NaN')
    return eps_region, int(K), eta, int(rep_lim)


def romc_regions(problems, prob, centre, hess, eps_region, K=10, eta=1., rep_lim=300):
    """The bounding boxes of R problems in one launch: prob (R), centre (R, 2), hess (R, 2, 2).  Returns a dict: rotation
    (R, 2, 2) (columns: the search directions), limits (R, 2, 2) = [direction][left <= 0, right >= 0], nfev (R, 2, 2)."""
    centre = _points(centre, 'centre')
    R = centre.shape[0]
    prob = _index(prob, problems.n1, R)
    hess = np.ascontiguousarray(np.asarray(hess, dtype=np.float64))
    if hess.shape != (R, DIM, DIM):
        raise ValueError('hess must have shape (%d, 2, 2), got %r' % (R, hess.shape))
    eps_region, K, eta, rep_lim = _search_args(eps_region, K, eta, rep_lim)
    out = dict(rotation=np.empty((R, DIM, DIM)), limits=np.empty((R, DIM, 2)), nfev=np.empty((R, DIM, 2), dtype=np.int32))
    _call(problems.ctx, 'elfihip_romc_regions', problems._h(), R, _lib.ptr(prob), _lib.ptr(centre), _lib.ptr(hess),
          C.c_double(eps_region), K, C.c_double(eta), rep_lim, _lib.ptr(out['rotation']), _lib.ptr(out['limits']),
          _lib.ptr(out['nfev']))
    return out


def _boxes(R, centre, rotation, limits, rot_name='rotation'):
    centre = _points(centre, 'centre')
    if centre.shape[0] != R:
        raise ValueError('centre has %d rows for %d regions' % (centre.shape[0], R))
    rotation = np.ascontiguousarray(np.asarray(rotation, dtype=np.float64))
    limits = np.ascontiguousarray(np.asarray(limits, dtype=np.float64))
    if rotation.shape != (R, DIM, DIM) or limits.shape != (R, DIM, 2):
        raise ValueError('%s and limits must have shape (%d, 2, 2), got %r and %r' % (rot_name, R, rotation.shape, limits.shape))
    return centre, rotation, limits


def romc_sample(problems, prob, centre, rotation, limits, n2, seed=0, stream=ROMC_STREAM_BASE):
    """n2 points per region, uniform in its box, and the region's objective there; one launch.  Region r draws from Philox
    stream (seed, stream + r).  Returns (theta (R, n2, 2), f (R, n2))."""
    prob = _index(prob, problems.n1)
    R, n2 = prob.shape[0], int(n2)
    centre, rotation, limits = _boxes(R, centre, rotation, limits)
    if not 0 <= n2 <= MAX_POINTS:
        raise ValueError('n2=%d points per region: 0 to %d' % (n2, MAX_POINTS))
    theta, f = np.empty((R, n2, DIM)), np.empty((R, n2))
    _call(problems.ctx, 'elfihip_romc_sample', problems._h(), R, _lib.ptr(prob), _lib.ptr(centre), _lib.ptr(rotation),
          _lib.ptr(limits), n2, C.c_uint64(int(seed)), C.c_uint64(int(stream)), _lib.ptr(theta), _lib.ptr(f))
    return theta, f


def romc_count(problems, theta, prob, eps, boxes=None):
    """count[b] = the number of regions r with f_{prob[r]}(theta[b]) <= eps; with boxes = (centre, rotation_inv, limits) the
    point must also lie in box r (NDimBoundingBox.contains).  One launch; int32 (BS)."""
    theta = _points(theta, 'theta')
    prob = _index(prob, problems.n1)
    R = prob.shape[0]
    if theta.shape[0] > MAX_POINTS:
        raise ValueError('%d points: up to %d' % (theta.shape[0], MAX_POINTS))
    centre = rotation_inv = limits = None
    if boxes is not None:
        centre, rotation_inv, limits = _boxes(R, *boxes, rot_name='rotation_inv')
    count = np.empty(theta.shape[0], dtype=np.int32)
    _call(problems.ctx, 'elfihip_romc_count', problems._h(), theta.shape[0], _lib.ptr(theta), R, _lib.ptr(prob), C.c_double(float(eps)),
          int(boxes is not None), _lib.ptr(centre), _lib.ptr(rotation_inv), _lib.ptr(limits), _lib.ptr(count))
    return count


# ---- the reference's classes on these calls ----------------------------------------------------------------------------------
def _module(name, what):
    mod = sys.modules.get(name)
    if mod is None:
        raise ImportError("%s subclasses the running program's ELFI class: `import elfi` first" % what)
    return mod


def problem_streams(nuisance):
    """The (seed, stream) pairs the device simulator of a fused model uses under model.generate(batch_size=1,
    with_values=<all parameters>, seed=int(nuisance_i)): ELFI seeds batch 0 with RandomState(get_sub_seed(seed, 0)), and the
    simulator -- the only stochastic node left to run -- takes one randint of it as its Philox seed on
    SIMULATOR_STREAM_BASE."""
    from .fused_models import _seed_of
    get_sub_seed = _module('elfi.utils', 'HipROMC').get_sub_seed
    seeds = np.array([_seed_of(np.random.RandomState(get_sub_seed(int(v), 0))) for v in nuisance], dtype=np.uint64)
    return seeds, np.full(seeds.shape, SIMULATOR_STREAM_BASE, dtype=np.uint64)


def ma2_model_parts(model, discrepancy_name):
    """(n_obs, observed summaries) of a model made by elfi_amd.ma2_model; NotImplementedError for any other."""
    from . import fused_models
    what = 'HipROMC runs on the model elfi_amd.ma2_model() returns (D = 2, n_obs <= %d)' % MAX_OBS
    try:
        op = model.get_state('MA2')['attr_dict']['_operation']
        parents = sorted(model.get_parents(discrepancy_name))
    except Exception:
        raise NotImplementedError(what)
    if not isinstance(op, partial) or op.func is not fused_models.ma2_summaries or parents != ['S1', 'S2'] \
            or list(model.parameter_names) != ['t1', 't2']:
        raise NotImplementedError(what)
    n_obs = int(op.keywords.get('n_obs', 100))
    if not 3 <= n_obs <= MAX_OBS:
        raise NotImplementedError(what + '; this model has n_obs = %d' % n_obs)
    return n_obs, tuple(float(v) for v in op.keywords['observed_summaries'])


def hip_romc_posterior_class():
    """The subclass of the imported ELFI's RomcPosterior whose sample and pdf_unnorm_batched are one device call each; with
    a surrogate in use both take the reference's path."""
    Base = _module('elfi.methods.posteriors', 'HipRomcPosterior').RomcPosterior
    cls = _CLASSES.get(Base)
    if cls is not None:
        return cls

    class HipRomcPosterior(Base):
        __doc__ = hip_romc_posterior_class.__doc__

        def __init__(self, *args, problems=None, prob_index=None, **kwargs):
            super().__init__(*args, **kwargs)
            self.problems = problems
            self.prob_index = np.asarray(prob_index, dtype=np.int64)

        def _box_arrays(self):
            regs = self.regions
            return (np.array([r.center for r in regs], dtype=np.float64).reshape(-1, DIM),
                    np.array([r.rotation for r in regs], dtype=np.float64).reshape(-1, DIM, DIM),
                    np.array([r.limits for r in regs], dtype=np.float64).reshape(-1, DIM, 2))

        def sample(self, n2, seed=None):
            """RomcPosterior.sample (posteriors.py:694-772): one device call for the points and their distances, ONE vectorised
            prior.pdf on the (R n2, D) points; w = 1[f < eps] prior / q with q = 1 / volume (a drawn point is inside its box
            by construction).  seed None draws one from numpy's global state."""
            if self.surrogate_used:
                return super().sample(n2, seed=seed)
            R = len(self.regions)
            if R == 0:
                return np.empty((0, n2, DIM)), np.empty((0, n2)), np.empty(0)
            if seed is None:
                seed = int(np.random.randint(0, 2 ** 31 - 1))
            centre, rotation, limits = self._box_arrays()
            theta, f = romc_sample(self.problems, self.prob_index, centre, rotation, limits, n2, seed=seed)
            pr = np.asarray(self.prior.pdf(theta.reshape(-1, DIM)), dtype=np.float64).reshape(R, n2)
            q = 1.0 / np.array([r.volume for r in self.regions], dtype=np.float64)
            w = (f < self.eps_cutoff) * pr / q[:, None]
            return theta, w, f.reshape(-1)

        def pdf_unnorm_batched(self, theta):
            """RomcPosterior.pdf_unnorm_batched (posteriors.py:587-617): one device call for the BS x R indicators, one
            prior.pdf."""
            if self.surrogate_used:
                return super().pdf_unnorm_batched(theta)
            assert isinstance(theta, np.ndarray)
            assert theta.ndim == 2
            pr = np.asarray(self.prior.pdf(theta), dtype=np.float64).reshape(-1)
            if len(self.regions) == 0:
                return pr * 0
            return pr * romc_count(self.problems, theta, self.prob_index, self.eps_cutoff)

    HipRomcPosterior.__name__ = HipRomcPosterior.__qualname__ = 'HipRomcPosterior'
    _CLASSES[Base] = HipRomcPosterior
    return HipRomcPosterior


def hip_romc_class():
    """The subclass of the imported ELFI's ROMC (made once per reference class) whose optimisation, region construction,
    sampling and density evaluation run on the device for the model of elfi_amd.ma2_model (module docstring)."""
    romc_mod = _module('elfi.methods.inference.romc', 'HipROMC')
    Base = romc_mod.ROMC
    cls = _CLASSES.get(Base)
    if cls is not None:
        return cls

    class HipROMC(Base):
        __doc__ = hip_romc_class.__doc__

        def __init__(self, model, bounds=None, discrepancy_name=None, output_names=None, custom_optim_class=None,
                     parallelize=False, **kwargs):
            if custom_optim_class is not None:
                raise NotImplementedError('HipROMC builds the reference\'s own OptimisationProblem objects: custom_optim_class '
                                          'is not supported (use elfi.ROMC)')
            super().__init__(model, bounds=bounds, discrepancy_name=discrepancy_name, output_names=output_names,
                             custom_optim_class=None, parallelize=parallelize, **kwargs)
            self._n_obs, self._observed = ma2_model_parts(self.model, self.discrepancy_name)
            self.problems = None

        def _solve_gradients(self, **kwargs):
            """ROMC._solve_gradients (romc.py:614-664) as one device call; optimiser arguments: seed, x0."""
            extra = sorted(set(kwargs) - {'seed', 'x0'})
            if extra:
                raise NotImplementedError('HipROMC runs SciPy\'s default Nelder-Mead on the device: the optimiser arguments '
                                          'seed and x0 are supported, not %s' % ', '.join(extra))
            assert self.inference_state['_has_defined_problems']
            n1 = self.inference_args['N1']
            probs = self.optim_problems
            seeds, streams = problem_streams([p.nuisance for p in probs])
            if self.problems is not None:
                self.problems.free()
            self.problems = RomcProblems(self._n_obs, self._observed, seeds=seeds, streams=streams)
            if kwargs.get('x0') is not None:
                x0 = np.broadcast_to(np.asarray(kwargs['x0'], dtype=np.float64).reshape(-1), (n1, DIM))
            else:
                x0 = np.asarray(self.model_prior.rvs(size=n1, random_state=kwargs.get('seed')), dtype=np.float64)
            x0 = np.ascontiguousarray(x0.reshape(n1, DIM))
            res = romc_solve(self.problems, x0)
            solved = [bool(s == SOLVED) for s in res['status']]
            for i, p in enumerate(probs):
                p.state['attempted'] = True
                p.state['solved'] = solved[i]
                if solved[i]:
                    p.result = romc_mod.RomcOptimisationResult(res['x_min'][i].copy(), float(res['f_min'][i]), res['hess'][i].copy())
                    p.initial_point = x0[i].copy()
            self.solve_info = res
            self.inference_state['solved'] = solved
            self.inference_state['attempted'] = [True] * n1
            self.inference_state['_has_solved_problems'] = True

        def _build_boxes(self, **kwargs):
            """ROMC._build_boxes (romc.py:758-806) as one device call; with use_surrogate=True the reference's own."""
            if kwargs.get('use_surrogate') or self.problems is None:
                return super()._build_boxes(**kwargs)
            extra = sorted(set(kwargs) - {'use_surrogate', 'eps_region', 'eta', 'K', 'rep_lim'})
            if extra:
                raise NotImplementedError('region arguments: eps_region, eta, K, rep_lim, use_surrogate; not %s' % ', '.join(extra))
            assert 'eps_region' in kwargs, 'In the current build region implementation, kwargs must contain eps_region'
            probs = self.optim_problems
            accepted = self.inference_state['accepted']
            n1 = self.inference_args['N1']
            idx = [i for i in range(n1) if accepted[i]]
            computed = [False] * n1
            if idx:
                centre = np.array([np.array(probs[i].result.x_min, dtype=float) for i in idx])
                hess = np.array([probs[i].result.hess_appr for i in idx])
                res = romc_regions(self.problems, idx, centre, hess, kwargs['eps_region'], K=kwargs.get('K', 10),
                                   eta=kwargs.get('eta', 1.), rep_lim=kwargs.get('rep_lim', 300))
                for k, i in enumerate(idx):
                    p = probs[i]
                    p.state['has_built_region_with_surrogate'] = False
                    p.eps_region = kwargs['eps_region']
                    p.regions = [romc_mod.NDimBoundingBox(res['rotation'][k].copy(), centre[k].copy(), res['limits'][k].copy())]
                    p.state['region'] = True
                    computed[i] = True
            self.inference_state['computed_BB'] = computed
            self.inference_state['_has_estimated_regions'] = True

        def _define_posterior(self, eps_cutoff):
            """ROMC._define_posterior (romc.py:838-895) with a HipRomcPosterior over the same regions and objectives."""
            if self.problems is None:
                return super()._define_posterior(eps_cutoff)
            use_surrogate = self.inference_state['_has_fitted_surrogate_model']
            use_local = self.inference_state['_has_fitted_local_models']
            regions, objectives, actual, nuisance, index = [], [], [], [], []
            surrogate = [] if use_surrogate else None
            local = [] if use_local else None
            for i, p in enumerate(self.optim_problems):
                if not p.state['region']:
                    continue
                for jj, region in enumerate(p.regions):
                    nuisance.append(p.nuisance)
                    index.append(i)
                    regions.append(region)
                    actual.append(p.objective)
                    if use_surrogate:
                        surrogate.append(p.surrogate)
                    if use_local:
                        local.append(p.local_surrogates[jj])
                    objectives.append(p.local_surrogates[jj] if use_local else (p.surrogate if use_surrogate else p.objective))
            self.posterior = hip_romc_posterior_class()(
                regions, objectives, actual, surrogate, local, nuisance, use_local or use_surrogate, self.model_prior,
                self.left_lim, self.right_lim, self.inference_args['eps_filter'], self.inference_args['eps_region'], eps_cutoff,
                self.inference_args['parallelize'], problems=self.problems, prob_index=index)
            self.inference_state['_has_defined_posterior'] = True

    HipROMC.__name__ = HipROMC.__qualname__ = 'HipROMC'
    _CLASSES[Base] = HipROMC
    return HipROMC


def HipROMC(*args, **kwargs):
    """elfi.ROMC(model, bounds=None, discrepancy_name=None, output_names=None, parallelize=False) for elfi_amd.ma2_model with
    the optimisation, the regions, the sampling and the density on the GPU."""
    return hip_romc_class()(*args, **kwargs)
