"""GPU: a call's result is a function of its arguments and of the handle it is given, not of what its context ran before.

Nearly every entry point borrows buffers the context owns (csrc/common.hpp, struct elfihip_ctx): the staging buffers `in`,
`out`, `par`; `scratch` (selection, Welford, weighted statistics, mixtures, the likelihoods, KLIEP); `stat` and the fold's
arrival counter; `sel`; the kept distances and rows with their epochs; the mailbox and its ticket; the GP's side streams and
events; the lazily raised LDS limits and the form switches.  DevBuf::reserve frees and reallocates when a larger call arrives,
so every cached address moves.  What each family computes is pinned by its own test file; this one holds the sharing, the way
tests/test_sim_shared_state_gpu.py holds it for the four event simulators:

  alone        every entry of the table on a fresh context of its own -- twice, and the two runs must agree byte for byte
               (a family that fails here is not deterministic, which is another finding than a dependence on shared state);
  interleaved  on ONE fresh context the whole table in five orders, each followed by its own reverse: forward (the large
               instance L of a family follows its small instance S), backward (small ones follow into buffers that are already
               large), small-first (all S before all L: every shared buffer grows mid-run) and two fixed shuffles.  Every
               output must equal the entry's output alone in dtype, shape and bytes;
  adopted      the forward order once more on a context adopted onto the busy non-null stream of tests/stream_order.py, some
               milliseconds of other work enqueued in front of every call.  All calls are host forms, so only the bytes are
               asserted.  The GP's side streams fork from the adopted stream here;
  control      a pure-Python entry whose output depends on how many calls its context has seen must be flagged, so that the
               comparison is known to see such a dependence.  It stays out of the real runs.

An entry is a sequence of steps `step(elfi_amd, ctx, st) -> arrays`; most have one.  The handles that outlive a call -- the
sampler state, kept distances and kept rows, two GP objects on one context, a ROMC handle -- have several, and the interleaved
runs deal those out one at a time between the other entries, each sequence in its own order.

Shapes are the smallest that reach the branch named next to them.  The very wide rows (m = 300) take n = 515 and 8209 instead
of 4099 and 70001: the wide kernel is chosen by m alone (distance.hip: launch_rows), 8209 rows are one more than its largest
grid covers in one trip (four rows per workgroup, eight workgroups per CU, 256 CUs), and 70001 x 300 doubles are 168 MB.
"""
import faulthandler
import functools
import random
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---- inputs: made on first use (collecting this module costs nothing), shared, never written ------------------------------
@functools.lru_cache(maxsize=None)
def _normal(seed, *shape):
    return np.random.RandomState(seed).standard_normal(shape)


@functools.lru_cache(maxsize=None)
def _unif(seed, lo, hi, *shape):
    return np.random.RandomState(seed).uniform(lo, hi, shape)


@functools.lru_cache(maxsize=None)
def _spd(seed, m):
    a = np.random.RandomState(seed).standard_normal((m, m))
    return a @ a.T / m + np.eye(m)


def _rows(big):
    return 70001 if big else 4099


# ---- the one-call families: f(elfi_amd, ctx, big) -------------------------------------------------------------------------
def rows_euclidean_w(ea, ctx, big):                      # m = 32: the LDS-DMA row stream
    return ea.cdist_rows(_normal(1, _rows(big), 32), _normal(2, 1, 32), 'euclidean', w=_unif(3, 0.1, 2.0, 32), ctx=ctx)


def rows_mahalanobis(ea, ctx, big):
    return ea.cdist_rows(_normal(4, _rows(big), 12), _normal(5, 1, 12), 'mahalanobis', VI=_spd(6, 12), ctx=ctx)


def rows_wide(ea, ctx, big):                             # m = 300: one wavefront per row
    return ea.cdist_rows(_normal(7, 8209 if big else 515, 300), _normal(8, 1, 300), 'euclidean', ctx=ctx)


def cols(ea, ctx, big):
    return ea.cdist_cols([_normal(10 + j, _rows(big)) for j in range(5)], _normal(9, 5), 'cityblock', ctx=ctx)


def nested(m, K, ea, ctx, big):                          # (32, 3) DMA, (4, 8) narrow, (10, 9) plain tile
    return ea.nested_weighted_euclidean(_normal(20 + m, _rows(big), m), _normal(21 + m, m), _unif(22 + m, 0.1, 2.0, K, m), ctx=ctx)


def welford(m, ea, ctx, big):
    n = (8209 if big else 2053) if m == 300 else _rows(big)
    return ea.welford_update(_normal(60 + m, n, m), 7, _normal(61 + m, m), _unif(62 + m, 0.5, 2.0, m), ctx=ctx)


def weighted_var(ea, ctx, big):
    return ea.weighted_var(_normal(70, _rows(big), 6), _unif(71, 0.0, 1.0, _rows(big)), ctx=ctx)


def topk(form, ea, ctx, big):                            # 16385: two LDS slices; 70001: keys in registers
    ctx.call('elfihip_topk_set_form', form)
    try:
        return ea.smallest_k(_normal(80, 70001 if big else 16385), 300, ctx=ctx)
    finally:
        ctx.call('elfihip_topk_set_form', 0)


def provisional(m, ea, ctx, big):
    """An adaptive batch into an EMPTY sampler state: m = 32 the fused pass (stat, fold_cnt, mailbox); m = 33 a resident
    selection in scratch, its flag through the mailbox, then the two-pass Welford update in scratch again."""
    n = 45001 if big else 20000
    state = ea.RunningBest(100, ctx=ctx)
    try:
        d, store = ea.adaptive_batch(_normal(90 + m, n, m), _normal(91 + m, m), _unif(92 + m, 0.1, 2.0, 3, m), store=(0, 0., 0.),
                                     state=state, ctx=ctx)
        return d, store, state.result(), state.meta()
    finally:
        state.close()


def gm_pdf(ea, ctx, big):
    return ea.GMDistribution.pdf(_normal(100, 1200 if big else 300, 8), _normal(101, 2000, 8), cov=_spd(102, 8),
                                 weights=_unif(103, 0.1, 1.0, 2000), ctx=ctx)


def gm_rvs(ea, ctx, big):
    return ea.GMDistribution.rvs(_normal(104, 1000, 5), cov=_spd(105, 5), weights=_unif(106, 0.1, 1.0, 1000),
                                 size=20001 if big else 1000, random_state=np.random.RandomState(107), ctx=ctx)


def prior_uniform(ea, ctx, big):
    return ea.priors.prior_draw(ea.priors.UNIFORM, (0.5, 2.0), size=_rows(big), seed=110, stream=3, ctx=ctx)


def prior_ma2_t2(ea, ctx, big):
    return ea.priors.prior_draw(ea.priors.MA2_T2, (1.0,), cond=_unif(111, -2.0, 2.0, _rows(big)), size=_rows(big), seed=112, stream=5,
                                ctx=ctx)


def poisson(ea, ctx, big):                               # inversion below 10, transformed rejection above
    return ea.poisson(_unif(113, 0.5, 30.0, _rows(big)), seed=114, stream=7, ctx=ctx)


def stable(ea, ctx, big):
    return ea.levy_stable(_unif(115, 0.5, 2.0, _rows(big)), scale=_unif(116, 0.5, 2.0, _rows(big)), seed=117, stream=9, ctx=ctx)


def syn_loglik(ea, ctx, big):
    G = 12 if big else 3
    return ea.syn_loglik(_normal(120, G, 600, 8), 0.1 * _normal(121, 8), shrinkage='warton', prefixes=[300, 600], penalties=[0.1, 0.5],
                         return_moments=True, ctx=ctx)


def semi_loglik(ea, ctx, big):
    G = 9 if big else 3
    return ea.semi_loglik(_normal(122, G, 400, 8), 0.1 * _normal(123, 8), shrinkage='warton', prefixes=[200, 400], penalties=[0.2],
                          return_parts=True, ctx=ctx)


def slice_gamma(adjustment, ea, ctx, big):
    G, m = 64 if big else 4, 16
    mean, y = 0.3 * _normal(124, G, m), 0.3 * _normal(125, m)
    cov = np.stack([_spd(126 + g % 4, m) for g in range(G)])
    gamma = np.abs(0.2 * _normal(127, G, m)) if adjustment == 'variance' else 0.2 * _normal(127, G, m)
    r = y - mean                                         # the standard synthetic log-likelihood at gamma = 0: a plausible level
    ll = np.array([-0.5 * np.linalg.slogdet(cov[g])[1] - 0.5 * r[g] @ np.linalg.solve(cov[g], r[g]) for g in range(G)])
    return ea.slice_gamma(y, ll, gamma, mean, cov, adjustment, max_iter=200, seed=128, n_groups=G, return_info=True, ctx=ctx)


def kliep(ea, ctx, big):
    Nx, Ny = (1500, 1200) if big else (500, 400)
    x, y, sig = 0.8 * _normal(130, Nx, 3) + 0.3, _normal(131, Ny, 3), (0.7, 1.5)
    fit = ea.kliep_fit(x, y, weights_x=_unif(132, 0.5, 1.5, Nx), sigma=sig, n=100, fold=3, ctx=ctx)
    return fit, [ea.kliep_ratio(x[:100], x[:100], fit['alpha'][s], sig[s], ctx=ctx) for s in range(2)]


def log_ratio(ea, ctx, big):
    G = 16 if big else 4
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                  # (a fit that stops at max_iter warns: not what is compared here)
        return ea.log_ratio(_normal(133, G, 60, 5) + 0.5, _normal(134, 45, 5), 0.3 * _normal(135, 2, 5), return_parts=True, ctx=ctx)


def linear_adjust(ea, ctx, big):
    G = 9 if big else 3
    X = _normal(136, G, 700, 5)
    Y = X[:, :, :2] * 0.5 + 0.1 * _normal(137, G, 700, 2)
    return ea.linear_adjust(X, Y, prefixes=[100, 350, 700], return_parts=True, ctx=ctx)


def knn_entropy(ea, ctx, big):
    return ea.knn_entropy(_normal(138, 21 if big else 7, 300, 2), k=4, return_kth=True, ctx=ctx)


def mrsse(ea, ctx, big):
    return ea.mrsse(_normal(139, 21 if big else 7, 300, 2), 0.1 * _normal(140, 20, 2), ctx=ctx)


def subset_best(ea, ctx, big):                           # 65 masks: two blocks, each with a resident selection and its flag
    masks = np.array([[(c % 31 + 1) >> j & 1 for j in range(5)] for c in range(65)], dtype=np.float64)
    return ea.subset_best(_normal(141, 9000 if big else 3000, 5), _normal(142, 5), masks, 200, ctx=ctx)


def _sims(big):
    return 800 if big else 200


def ma2(ea, ctx, big):
    n = _sims(big)
    return ea.ma2_draw_distance(_unif(150, -1.0, 1.0, n), _unif(151, 0.0, 1.0, n), (0.4, 0.1), n_obs=100, seed=152, stream=11, ctx=ctx)


def gauss(ea, ctx, big):
    n = _sims(big)
    return ea.gauss_distance(_unif(153, -1.0, 3.0, n), _unif(154, 0.5, 2.0, n), (1.0, 1.2), n_obs=50, seed=155, stream=13, ctx=ctx)


def arch(ea, ctx, big):
    n = _sims(big)
    return ea.arch_summaries(_unif(156, -0.9, 0.9, n), _unif(157, 0.0, 0.9, n), n_obs=100, seed=158, stream=15,
                             observed=0.1 * _normal(159, 17), ctx=ctx)


def mg1(ea, ctx, big):                                   # the quantile positions travel in `par`
    n = _sims(big)
    t1 = _unif(160, 0.5, 5.0, n)
    return ea.mg1_summaries(t1, t1 + _unif(161, 0.5, 5.0, n), _unif(162, 0.05, 0.3, n), n_obs=50, seed=163, stream=17,
                            observed=np.linspace(1.0, 12.0, 10), w=_unif(164, 0.5, 1.5, 10), ctx=ctx)


def gnk(ea, ctx, big):                                   # ... and here
    n = _sims(big)
    return ea.gnk_summaries(_unif(165, 2.0, 4.0, n), _unif(166, 0.5, 2.0, n), _unif(167, 1.0, 3.0, n), _unif(168, 0.2, 0.8, n), n_obs=50,
                            seed=169, stream=19, summary=('octile', 'robust'), observed=np.linspace(1.0, 8.0, 7), ctx=ctx)


def _named(fn, *args):
    f = functools.partial(fn, *args)
    f.__name__ = '-'.join([fn.__name__] + [str(a) for a in args])
    return f


FAMILIES = (rows_euclidean_w, rows_mahalanobis, rows_wide, cols, _named(nested, 32, 3), _named(nested, 4, 8), _named(nested, 10, 9),
            _named(welford, 33), _named(welford, 300), weighted_var, _named(topk, 0), _named(topk, 1), _named(topk, 2),
            _named(provisional, 32), _named(provisional, 33), gm_pdf, gm_rvs, prior_uniform, prior_ma2_t2, poisson, stable, syn_loglik,
            semi_loglik, _named(slice_gamma, 'mean'), _named(slice_gamma, 'variance'), kliep, log_ratio, linear_adjust, knn_entropy,
            mrsse, subset_best, ma2, gauss, arch, mg1, gnk)


# ---- handles that outlive a call: sequences of steps s(elfi_amd, ctx, st); st is the sequence's own dict ----------------------
def _keep(st, handle, close):
    st['closers'].append(close)
    return handle


def sampler_steps(k):
    """Four batches of 5000 rows into one RunningBest, then its result: k = 300 merges on the device (two candidate lists, sealed
    merges inside the next distance pass), k = 4096 on the host."""
    def push(b, ea, ctx, st):
        if b == 0:
            st['state'] = ea.RunningBest(k, w=_unif(201, 0.1, 2.0, 32), ctx=ctx)
            _keep(st, None, st['state'].close)
        return st['state'].push(_normal(200, 20000, 32)[5000 * b:5000 * (b + 1)], _normal(202, 1, 32))

    def result(ea, ctx, st):
        return st['state'].result(), st['state'].meta()
    return tuple(functools.partial(push, b) for b in range(4)) + (result,)


def _kept_distance(ea, ctx, st):
    st['d'] = ea.cdist_rows(_normal(210, 4099, 32), _normal(211, 1, 32), ctx=ctx)
    return st['d']


def _kept_between(ea, ctx, st):                          # unrelated: leaves the epoch alone, reuses `in` and `scratch`
    return ea.weighted_var(_normal(212, 9001, 6), ctx=ctx)


def _kept_push(ea, ctx, st):
    """The state takes the device copy the distance call left if the context still keeps it (elfihip_reject_push_kept), and
    uploads the host array if another distance call has moved the epoch on since: the same rows either way."""
    state = ea.RunningBest(50, ctx=ctx)
    try:
        state.push_distances(st['d'])
        return state.result(), state.meta()
    finally:
        state.close()


def _rows_draw(ea, ctx, st):
    st['X'] = ea.randn_rows(_unif(213, -1.0, 1.0, 3001), _unif(214, 0.5, 2.0, 6), seed=215, stream=21, ctx=ctx)
    return st['X']


def _rows_between(ea, ctx, st):
    return ea.welford_update(_normal(216, 5003, 7), 0, 0.0, 0.0, ctx=ctx)


def _rows_distance(ea, ctx, st):
    return ea.cdist_rows(st['X'], _normal(217, 1, 6), ctx=ctx)


def _gp_data(seed, n, d):
    X = _unif(seed, 0.0, 1.0, n, d)
    # (minima inside the unit box: the searches below take more than one step)
    return X, 4.0 * (X[:, 0] - 0.4) ** 2 + np.sin(5.0 * X[:, 1]) + 0.5 * np.cos(X.sum(axis=1)) + 0.05 * _normal(seed + 1, n)


def _gp_a(st):
    return st['A']


def _gp_b(st):
    return st['B']


def _gp_make(which, ea, ctx, st):
    from elfi_amd.gp import GPHandle
    if which == 'A':                                     # the stream schedule: the context's side streams and events
        X, y = _gp_data(220, 300, 2)
        gp = GPHandle(2, 512, ctx=ctx)
        gp.set_hyper(1.0, 0.3, 1.0, 0.05)
        gp.set_schedule(1, 0)
    else:                                                # dp > 24: queries are uploaded; the fused schedule
        X, y = _gp_data(222, 700, 30)
        gp = GPHandle(30, 768, ctx=ctx)
        gp.set_hyper(1.5, 2.0, 0.5, 0.1)
        gp.set_schedule(2, 0)
    st[which] = _keep(st, gp, gp.close)
    gp.set_data(X, y)
    return gp.factorize()


_BOUNDS_A = ((0.0, 1.0), (0.0, 1.0))

GP_STEPS = (
    functools.partial(_gp_make, 'A'),
    functools.partial(_gp_make, 'B'),
    lambda ea, ctx, st: _gp_a(st).predict_grad(_unif(224, 0.0, 1.0, 7, 2)),
    lambda ea, ctx, st: _gp_b(st).lcb(_unif(225, 0.0, 1.0, 17, 30), 2.0),
    lambda ea, ctx, st: _gp_a(st).extend(*(a[:3] for a in _gp_data(226, 8, 2))),
    lambda ea, ctx, st: _gp_b(st).nlml_grad(),
    lambda ea, ctx, st: _gp_a(st).lcb_minimize(_unif(227, 0.0, 1.0, 10, 2), _BOUNDS_A, 2.0, maxiter=30),
    lambda ea, ctx, st: _gp_b(st).predict(_unif(228, 0.0, 1.0, 130, 30)),
    lambda ea, ctx, st: _gp_a(st).minimize_mean(_BOUNDS_A, seed=229, stream=23, maxiter=20),      # (the mailbox)
    lambda ea, ctx, st: _gp_b(st).kernel_matrix(_unif(230, 0.0, 1.0, 40, 30), _unif(231, 0.0, 1.0, 25, 30)),   # (ctx->out)
    lambda ea, ctx, st: _gp_a(st).maxvar(_unif(232, 0.0, 1.0, 16, 2), 0.3, _unif(233, 0.5, 1.5, 16), _normal(234, 16, 2)),
    lambda ea, ctx, st: _gp_b(st).set_integration_points(_unif(235, 0.0, 1.0, 50, 30)),
    lambda ea, ctx, st: _gp_b(st).cross_cov(_unif(236, 0.0, 1.0, 20, 30)),
    lambda ea, ctx, st: _gp_b(st).expintvar(_unif(236, 0.0, 1.0, 20, 30), 0.3, _unif(237, 0.0, 1.0, 50), _normal(238, 50),
                                            _unif(239, 0.1, 1.0, 50)),
    lambda ea, ctx, st: _gp_a(st).factorize(),
)

_ROMC_OBS = (0.4, 0.1)


def _romc_objective(ea, ctx, st):
    st['p'] = ea.RomcProblems(50, _ROMC_OBS, seeds=np.arange(64) + 1000, streams=25, ctx=ctx)      # drawn noise
    _keep(st, None, st['p'].free)
    return ea.romc_objective(st['p'], _unif(240, -0.8, 0.8, 100, 2), np.arange(100) % 64)


def _romc_solve(ea, ctx, st):
    st['sol'] = ea.romc_solve(st['p'], _unif(241, -0.5, 0.5, 64, 2))
    return st['sol']


def _romc_regions(ea, ctx, st):
    sol = st['sol']
    solved = np.flatnonzero(sol['status'] == 0)
    idx = (solved if solved.size >= 8 else np.arange(64))[:8]
    st['idx'], st['centre'], st['eps'] = idx, sol['x_min'][idx], 2.0 * float(np.max(sol['f_min'][idx])) + 0.05
    st['reg'] = ea.romc_regions(st['p'], idx, st['centre'], sol['hess'][idx], st['eps'])
    return st['reg']


def _romc_sample(ea, ctx, st):
    st['theta'], f = ea.romc_sample(st['p'], st['idx'], st['centre'], st['reg']['rotation'], st['reg']['limits'], 40, seed=242)
    return st['theta'], f


def _romc_count(ea, ctx, st):
    boxes = (st['centre'], np.ascontiguousarray(np.transpose(st['reg']['rotation'], (0, 2, 1))), st['reg']['limits'])
    return ea.romc_count(st['p'], st['theta'].reshape(-1, 2), st['idx'], st['eps'], boxes=boxes)


class Entry:
    def __init__(self, name, steps, size=None):
        self.name, self.steps, self.size = name, tuple(steps), size


def _one_call(fn, big):
    return Entry('%s/%s' % (fn.__name__, 'L' if big else 'S'), [lambda ea, ctx, st: fn(ea, ctx, big)], 'L' if big else 'S')


TABLE = tuple(_one_call(fn, big) for fn in FAMILIES for big in (False, True)) + (
    Entry('sampler-300', sampler_steps(300)),
    Entry('sampler-4096', sampler_steps(4096)),
    Entry('kept-distances', (_kept_distance, _kept_between, _kept_push)),
    Entry('kept-rows', (_rows_draw, _rows_between, _rows_distance)),
    Entry('two-gps', GP_STEPS),
    Entry('romc', (_romc_objective, _romc_solve, _romc_regions, _romc_sample, _romc_count)),
)


def control(ea, ctx, st):
    """NOT a library call: what a dependence on the context's history looks like to the comparison below."""
    return np.array([getattr(ctx, 'calls_seen', 0)])


# ---- running a schedule ---------------------------------------------------------------------------------------------------
def flat(x):
    """Whatever a wrapper returns -> a list of arrays of its own (copies: a pinned result buffer is recycled)."""
    if x is None:
        return []
    if isinstance(x, dict):
        return [a for key in sorted(x) for a in flat(x[key])]
    if isinstance(x, (tuple, list)):
        return [a for v in x for a in flat(v)]
    return [np.array(x)]


def one_pass(entries, instance):
    """The one-call entries in the order given, a step of the sequences dealt out behind each of them in turn; what is left of
    the sequences afterwards, still in turn -> [(entry, instance, step)]."""
    single = [e for e in entries if len(e.steps) == 1]
    left = [[e, 0] for e in entries if len(e.steps) > 1]
    out, turn = [], 0

    def deal():
        nonlocal turn
        turn %= len(left)
        e, s = left[turn]
        out.append((e, instance, s))
        left[turn][1] += 1
        if left[turn][1] == len(e.steps):
            del left[turn]
        else:
            turn += 1
    for e in single:
        out.append((e, instance, 0))
        if left:
            deal()
    while left:
        deal()
    return out


def there_and_back(entries):
    return one_pass(entries, 0) + one_pass(entries[::-1], 1)


def run(ea, ctx, schedule, check, before=None):
    """Every (entry, instance, step) of the schedule on ctx; check(position, entry, step, outputs) after each.  The handles a
    sequence made are closed at the end, also on failure (a context is destroyed after its handles)."""
    states = {}
    try:
        for pos, (entry, instance, step) in enumerate(schedule):
            st = states.setdefault((entry.name, instance), {'closers': []})
            if before is not None:
                before()
            out = flat(entry.steps[step](ea, ctx, st))
            ctx.calls_seen = getattr(ctx, 'calls_seen', 0) + 1
            check(pos, entry, step, out)
    finally:
        for st in states.values():
            for close in reversed(st['closers']):
                close()


def run_alone(ea, table):
    """entry name -> [outputs of step 0, of step 1, ...], every entry on a context of its own, its steps back to back."""
    want = {}
    for entry in table:
        ctx = ea.Context()
        try:
            got = want.setdefault(entry.name, [])
            run(ea, ctx, [(entry, 0, s) for s in range(len(entry.steps))], lambda pos, e, s, out: got.append(out))
        finally:
            ctx.close()
    return want


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def differences(first, second):
    return ['%s, step %d, output %d' % (name, s, i) for name in first for s, (x, y) in enumerate(zip(first[name], second[name]))
            for i in range(max(len(x), len(y))) if i >= min(len(x), len(y)) or not same(x[i], y[i])]


def run_interleaved(ea, table, want, order, entries, before=None, ctx=None):
    def check(pos, entry, step, got):
        ref = want[entry.name][step]
        assert len(got) == len(ref), '%s, position %d (%s, step %d): %d outputs, %d alone' % (order, pos, entry.name, step, len(got),
                                                                                              len(ref))
        for part, (a, b) in enumerate(zip(got, ref)):
            assert same(a, b), '%s, position %d (%s, step %d): output %d differs from the call alone' % (order, pos, entry.name, step,
                                                                                                        part)
    own = ctx is None
    ctx = ea.Context() if own else ctx
    try:
        run(ea, ctx, there_and_back(entries), check, before)
    finally:
        if own:
            ctx.close()


def ordered(table, order):
    table = list(table)
    if order == 'forward':
        return table
    if order == 'backward':
        return table[::-1]
    if order == 'small-first':
        return [e for e in table if e.size == 'S'] + [e for e in table if e.size is None] + [e for e in table if e.size == 'L']
    random.Random({'shuffle-1': 1, 'shuffle-2': 2}[order]).shuffle(table)
    return table


ORDERS = ('forward', 'backward', 'small-first', 'shuffle-1', 'shuffle-2')


@pytest.fixture(autouse=True)
def time_limit():
    """A hung kernel ends the run instead of holding the device: the process exits after 120 s in one test."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope='module')
def alone_twice(hip_ctx):
    import elfi_amd
    return run_alone(elfi_amd, TABLE), run_alone(elfi_amd, TABLE)


@pytest.fixture(scope='module')
def alone(alone_twice):
    return alone_twice[0]


def test_every_entry_alone_is_deterministic(alone_twice):
    first, second = alone_twice
    assert all(len(first[e.name]) == len(e.steps) and any(len(out) for out in first[e.name]) for e in TABLE)
    assert differences(first, second) == [], 'two runs alone, each on a fresh context, differ'


def test_the_orders_make_the_shared_buffers_grow_and_deal_the_sequences_out():
    """Of the schedule itself (no device work): every entry runs twice per order, sequences keep their own order and are spread
    between the other entries, and L follows S of its family forward and precedes it backward."""
    for order in ORDERS:
        sched = there_and_back(ordered(TABLE, order))
        for e in TABLE:
            for instance in (0, 1):
                assert [s for x, i, s in sched if x is e and i == instance] == list(range(len(e.steps))), (order, e.name)
        gp = [p for p, (x, i, s) in enumerate(sched) if x.name == 'two-gps' and i == 0]
        assert all(b - a > 1 for a, b in zip(gp, gp[1:])), order
    where = {(x.name, i): p for p, (x, i, s) in enumerate(there_and_back(ordered(TABLE, 'forward')))}
    assert where['rows_wide/S', 0] < where['rows_wide/L', 0] and where['rows_wide/L', 1] < where['rows_wide/S', 1]
    small_first = [x.size for x, i, s in one_pass(ordered(TABLE, 'small-first'), 0) if x.size]
    assert small_first == sorted(small_first, reverse=True)


@pytest.mark.parametrize('order', ORDERS)
def test_interleaved_calls_on_one_context_equal_calls_alone(alone, order):
    import elfi_amd
    run_interleaved(elfi_amd, TABLE, alone, order, ordered(TABLE, order))


def test_forward_order_on_a_busy_adopted_stream_equals_calls_alone(alone):
    """Host forms all: each waits for its own results, so nothing is asserted about the stream still being busy, only the
    bytes.  The first run of the GP, ROMC, likelihood and post-processing families on an adopted stream."""
    import elfi_amd
    import stream_order as SO
    ctx = elfi_amd.Context()
    try:
        with SO.adopted_stream(ctx) as s:
            run_interleaved(elfi_amd, TABLE, alone, 'forward on the adopted stream', ordered(TABLE, 'forward'),
                            before=lambda: SO.busy(s, 5.0), ctx=ctx)
    finally:
        ctx.close()


def test_a_dependence_on_earlier_calls_is_flagged(hip_ctx):
    """The control: with an entry whose output counts the calls its context has seen, the two runs alone still agree (each
    on a fresh context) and the interleaved comparison fails, naming that entry."""
    import elfi_amd
    table = [e for e in TABLE if e.name in ('weighted_var/S', 'kept-rows')] + [Entry('control', [control])]
    first, second = run_alone(elfi_amd, table), run_alone(elfi_amd, table)
    assert differences(first, second) == []
    with pytest.raises(AssertionError, match=r'\(control, step 0\): output 0 differs from the call alone'):
        run_interleaved(elfi_amd, table, first, 'forward', table)
    run_interleaved(elfi_amd, table[:-1], first, 'forward', table[:-1])      # ... and without it the same runs pass
