"""Records tests/golden/demin.npz: the inputs and the reference's result for the search for the GP mean's minimiser (run where
the reference is installed; oracle/ref_shim.py makes it importable).  CPU only; data only.

Cases (n, d): (3, 1), (255, 2) and (257, 2) either side of the 256-row block, (300, 5) with the dimension padded to 8,
(600, 25) in the form for padded dimensions above 24 -- each a bowl-shaped target with its minimum inside the box -- and one
d = 2 case whose bowl is centred outside the box, so the minimiser lies on an edge.  Per case (key suffix _<index>):
  X, y, hyper (var, ls, bias, noise), bounds        the inputs
  x_ref, f_ref                                      stochastic_optimization of the imported reference (elfi/methods/bo/utils.py)
                                                    over predict_mean of the CPU posterior (oracle/oracle_gp_model.py), seed 1
  x_star                                            the refined minimiser: L-BFGS-B, then projected Newton steps on the
                                                    analytic CPU mean (tests/de_ref.py: GPMean on the CPU posterior's alpha)
                                                    until the projected gradient is below 1e-12
  e_ref = |x_ref - x_star|_inf,  excess_ref = mu(x_ref) - mu(x_star)
  pin_gap                                           the closest accept comparison |E_trial - E_member| of the first three
                                                    generations of tests/de_ref.py with seed PIN_SEED
  mean_scale = sum_i |alpha_i| (s_f + s_b)          what one unit of rounding in a kernel value is multiplied by in the mean
and pin_case: the case the pinned-statement test uses -- the first with d > 1 whose pin_gap exceeds 1e-9 and whose mean_scale
is at most 2000, so that two evaluations of the mean whose kernel values differ by two units in the last place (one from exp,
one from the dot product under it: 2 x 2^-52 mean_scale <= 8.9e-13) agree to the 1e-12 that test asks for -- asserted to
exist.  The noise variance 0.0504 (the targets carry noise of standard deviation 0.02) keeps alpha, and with it mean_scale,
that small.
Condition on a case, asserted here (a case that fails it moves its seed on by SEED_STEP and is done again): of 64 d L-BFGS-B
starts on the CPU mean, every end point away from x_star lies at least 1e-3 above it -- both searches must land in one basin.

    python scripts/make_golden_demin.py
"""
import os
import sys

import numpy as np
from scipy.optimize import minimize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import ref_shim  # noqa: E402
import de_ref as D  # noqa: E402

#        n    d  bowl centred outside the box   seed
CASES = [(3, 1, False, 11), (255, 2, False, 12), (257, 2, False, 13), (300, 5, False, 14), (600, 25, False, 15),
         (200, 2, True, 16)]
SEED_STEP = 100
REF_SEED = 1
PIN_SEED = 7
MIN_GAP = 1e-3


def make_inputs(n, d, edge, seed):
    rs = np.random.RandomState(seed)
    lo = np.where(np.arange(d) % 2 == 1, -1.0, -2.0)
    hi = -lo
    X = rs.uniform(lo, hi, (n, d))
    centre = rs.uniform(0.6 * lo, 0.6 * hi)
    if edge:
        centre[0] = 1.3 * hi[0]
    w = rs.uniform(0.5, 1.5, d)
    y = ((X - centre) ** 2 * w).sum(axis=1) / d + 0.02 * rs.randn(n)
    hyper = dict(var=float(4.0 * np.var(y) + 1.0), ls=float((hi - lo).max() / 3.0 * np.sqrt(d)),
                 bias=float(np.mean(y) ** 2 + 1.0), noise=float(0.02 ** 2 + 0.05))
    return X, y.reshape(-1, 1), hyper, np.column_stack([lo, hi])


def hessian(mean, x):
    k = mean.kernel(x)[0] * mean.alpha
    diff = x[None, :] - mean.X
    return (diff * k[:, None]).T @ diff / mean.ls ** 4 - np.eye(x.shape[0]) * k.sum() / mean.ls ** 2


def projected_gradient(g, x, lo, hi):
    pg = g.copy()
    pg[(x <= lo) & (g > 0)] = 0.0
    pg[(x >= hi) & (g < 0)] = 0.0
    return pg


def refine(mean, x0, lo, hi):
    fun = lambda v: (float(mean(v)[0]), mean.gradient(v)[0])   # noqa: E731
    x = minimize(fun, x0, jac=True, method='L-BFGS-B', bounds=list(zip(lo, hi)),
                 options=dict(ftol=1e-16, gtol=1e-13, maxiter=2000, maxcor=30)).x
    for _ in range(50):
        g = mean.gradient(x)[0]
        pg = projected_gradient(g, x, lo, hi)
        if np.max(np.abs(pg)) < 1e-12:
            return x, float(np.max(np.abs(pg)))
        free = pg != 0.0
        step = np.zeros_like(x)
        step[free] = -np.linalg.solve(hessian(mean, x)[np.ix_(free, free)], g[free])
        x = np.clip(x + step, lo, hi)
    raise AssertionError('the projected gradient stays at %.3e' % np.max(np.abs(pg)))


def other_minima_gap(mean, x_star, lo, hi, seed):
    rs = np.random.RandomState(seed + 1)
    d = lo.shape[0]
    fun = lambda v: (float(mean(v)[0]), mean.gradient(v)[0])   # noqa: E731
    f_star, gap = float(mean(x_star)[0]), np.inf
    for s in rs.uniform(lo, hi, (64 * d, d)):
        r = minimize(fun, s, jac=True, method='L-BFGS-B', bounds=list(zip(lo, hi)), options=dict(ftol=1e-15, gtol=1e-10))
        if np.max(np.abs(r.x - x_star)) > 1e-4:
            gap = min(gap, float(mean(r.x)[0]) - f_star)
    return gap


def do_case(elfi, n, d, edge, seed):
    from elfi.methods.bo.utils import stochastic_optimization
    from oracle_gp_model import OracleGPRegression
    X, y, hyper, bounds = make_inputs(n, d, edge, seed)
    lo, hi = bounds[:, 0].copy(), bounds[:, 1].copy()
    names = ['p%d' % j for j in range(d)]
    model = OracleGPRegression(names, bounds={nm: tuple(b) for nm, b in zip(names, bounds)})
    model._X, model._Y, model.hyper = X, y, hyper
    model._refit()
    x_ref, f_ref = stochastic_optimization(model.predict_mean, model.bounds, seed=REF_SEED)
    mean = D.GPMean(X, model._post.alpha, hyper['var'], hyper['ls'], hyper['bias'])
    x_star, pg = refine(mean, x_ref, lo, hi)
    gap = other_minima_gap(mean, x_star, lo, hi, seed)
    if gap < MIN_GAP:
        return None, 'another local minimum lies only %.3e above the global one' % gap
    if edge and not x_star[0] == hi[0]:
        return None, 'the minimiser is not on the edge'
    if not edge and not np.all((x_star > lo) & (x_star < hi)):
        return None, 'the minimiser is not inside the box'
    trace = []
    D.minimize(mean, lo, hi, seed=PIN_SEED, maxiter=3, polish=False, trace=trace)
    mine = D.minimize(mean, lo, hi, seed=REF_SEED)
    rec = dict(X=X, y=y, hyper=np.array([hyper[k] for k in ('var', 'ls', 'bias', 'noise')]), bounds=bounds,
               x_ref=np.asarray(x_ref), f_ref=float(f_ref), x_star=x_star,
               e_ref=float(np.max(np.abs(x_ref - x_star))), excess_ref=float(mean(x_ref)[0] - mean(x_star)[0]),
               pin_gap=float(min(trace)),
               mean_scale=float(np.abs(mean.alpha).sum() * (hyper['var'] + hyper['bias'])))
    print('case n=%d d=%d edge=%d seed %d: mean scale %.3g, projected gradient %.1e, other minima >= %.3g above, e_ref %.3e, excess_ref %.3e, '
          'pin gap %.3e; the statement: %d generations, |x - x*| %.3e, excess %.3e'
          % (n, d, edge, seed, rec['mean_scale'], pg, gap, rec['e_ref'], rec['excess_ref'], rec['pin_gap'], mine['generations'],
             np.max(np.abs(mine['x'] - x_star)), float(mean(mine['x'])[0] - mean(x_star)[0])), flush=True)
    return rec, None


def main():
    elfi = ref_shim.install()
    out, seeds = {}, []
    for ci, (n, d, edge, seed) in enumerate(CASES):
        while True:
            rec, why = do_case(elfi, n, d, edge, seed)
            if rec is not None:
                break
            print('case %d seed %d: %s -> next seed' % (ci, seed, why), flush=True)
            seed += SEED_STEP
        seeds.append(seed)
        for k, v in rec.items():
            out['%s_%d' % (k, ci)] = v
    gaps = [out['pin_gap_%d' % ci] for ci in range(len(CASES))]
    pin = [ci for ci, g in enumerate(gaps) if g > 1e-9 and CASES[ci][1] > 1 and out['mean_scale_%d' % ci] <= 2000.0]
    assert pin, 'no case keeps its accept comparisons 1e-9 apart with a mean scale of at most 2000: %s' % gaps
    out.update(cases=np.array([(n, d, int(e)) for n, d, e, _ in CASES]), seeds=np.array(seeds), pin_case=pin[0],
               pin_seed=PIN_SEED, ref_seed=REF_SEED)
    path = os.path.join(ROOT, 'tests', 'golden', 'demin.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes; pinned case', pin[0])


if __name__ == '__main__':
    main()
