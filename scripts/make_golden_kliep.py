"""Records tests/golden/kliep.npz from the reference ELFI's DensityRatioEstimation (run where the reference is installed;
oracle/ref_shim.py makes it importable).

For every case of tests/kliep_ref.py it stores
  ref      what the reference class gives: alpha, w(self.x), max_ratio() and the index at which its loop ended -- read off
           a subclass that records what _weighted_basis_sum returns during fit (one call for the start, one per
           convergence check; the loop ended at the last check when the last two differ by less than abs_tol, else at
           max_iter - 1),
  truth    the same quantities of the same float inputs in 60-digit arithmetic, as double-doubles (hi, lo),
  e_ref    |ref - truth| as a fraction of max |alpha| / max |w|,
  trace    the norm the truth computes at every convergence check.
Cross-validation (the CV_CASE with CV_SIGMAS and CV_FOLD folds): the reference's _KLIEP_lcv after a fit, the truth's score
of every fold and their mean, the scale the reference's optimize=True keeps (always the first of the list) and the
reference's value at the scale 1e-3.
Conditions on a recorded case, asserted here (a case that fails one moves its seed on by SEED_STEP and is done again):
every norm of the truth's trace differs from abs_tol by more than 1 %, the reference's loop ends where the truth's does,
no row's largest basis value lies in [1e-65, 1e-63], no training row has A_tr . alpha = 0, and a score is finite in the
reference's arithmetic exactly when it is in the truth.  Synthetic inputs are not stored: the seed that was used is.

    python scripts/make_golden_kliep.py
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import ref_shim  # noqa: E402
import kliep_ref as R  # noqa: E402

mp.mp.dps = 60
mpf = mp.mpf
WORKERS = 8


class Retry(Exception):
    pass


def split(v):
    hi = np.array([float(t) for t in v])
    lo = np.array([float(t - mpf(h)) for t, h in zip(v, hi)])
    return hi, lo


def mp_basis(points, centres, sigma):
    sg = mpf(float(sigma))
    rows = []
    for p in points:
        pm = [mpf(float(v)) for v in p]
        rows.append([mp.exp(-mp.fsum((a - mpf(float(c))) ** 2 for a, c in zip(pm, cj)) / 2 / sg / sg) for cj in centres])
    return rows


def mp_problem(case):
    """The basis of a case in mpmath: A (Nx rows), b, b_normalized, the non-null mask, the weights raw and normalised."""
    x, y, n = case['x'], case['y'], case['n']
    wx = [mpf(1)] * len(x) if case['weights_x'] is None else [mpf(float(v)) for v in case['weights_x']]
    wy = [mpf(1)] * len(y) if case['weights_y'] is None else [mpf(float(v)) for v in case['weights_y']]
    wxn = [v / mp.fsum(wx) for v in wx]
    wyn = [v / mp.fsum(wy) for v in wy]
    A = mp_basis(x, x[:n], case['sigma'])
    b = [mp.fdot(row, wyn) for row in mp_basis(x[:n], y, case['sigma'])]
    bb = mp.fdot(b, b)
    bn = [v / bb for v in b]
    top = [max(row) for row in A]
    if any(mpf(1e-65) <= t <= mpf(1e-63) for t in top):
        raise Retry('a row\'s largest basis value is next to the null level')
    non_null = [t > mpf(R.NULL_LEVEL) for t in top]
    return A, b, bn, non_null, wx, wxn


def mp_iterate(case, A, b, bn, train, w):
    """(alpha, A alpha over all rows, exit index, trace) with the training rows `train` (indices) and their weights."""
    n, eps, tol = case['n'], mpf(float(case['epsilon'])), mpf(float(case['abs_tol']))
    A_tr = [A[i] for i in train]
    cols = [[row[j] for row in A_tr] for j in range(n)]
    w_tr = [w[i] for i in train]
    alpha = [mpf(1) / n] * n
    prev = [mp.fdot(row, alpha) for row in A]
    trace, i = [], 0
    for i in range(case['max_iter']):
        den = [mp.fdot(row, alpha) for row in A_tr]
        if any(v == 0 for v in den):
            raise Retry('A_tr . alpha is zero on a training row')
        r = [wi / v for wi, v in zip(w_tr, den)]
        alpha = [a + eps * mp.fdot(c, r) for a, c in zip(alpha, cols)]
        ba = 1 - mp.fdot(b, alpha)
        alpha = [max(mpf(0), a + ba * v) for a, v in zip(alpha, bn)]
        ba = mp.fdot(b, alpha)
        alpha = [a / ba for a in alpha]
        if i % case['interval'] == 0:
            t = [mp.fdot(row, alpha) for row in A]
            diff = mp.sqrt(mp.fsum((u - v) ** 2 for u, v in zip(t, prev)))
            trace.append(float(diff))
            if abs(diff - tol) <= tol / 100:
                raise Retry('a convergence check lies within 1 %% of abs_tol (%.6g)' % float(diff))
            if diff < tol:
                break
            prev = t
    return alpha, [mp.fdot(row, alpha) for row in A], i, trace


def reference_class():
    ref_shim.install()
    from elfi.methods.density_ratio_estimation import DensityRatioEstimation

    class Recording(DensityRatioEstimation):
        """Keeps what _weighted_basis_sum returns, in the order of the calls."""
        calls = None

        def _weighted_basis_sum(self, x, sigma, alpha):
            r = super()._weighted_basis_sum(x, sigma, alpha)
            if self.calls is not None:
                self.calls.append(np.array(r, copy=True))
            return r
    return Recording


def reference_fit(case, **extra):
    sigma = extra.pop('sigma_arg', case['sigma'])
    est = reference_class()(fold=R.CV_FOLD, **dict(R.fit_kwargs(case), **extra))
    est.calls = []
    est.fit(case['x'], case['y'], weights_x=case['weights_x'], weights_y=case['weights_y'], sigma=sigma)
    calls, est.calls = est.calls, None
    return est, calls


def job_case(args):
    """One fixture case: reference and truth of the full fit."""
    ci, seed = args
    case = R.make_case(ci, seed)
    try:
        A, b, bn, non_null, wx, _ = mp_problem(case)
        train = [i for i, ok in enumerate(non_null) if ok]
        alpha, w, it, trace = mp_iterate(case, A, b, bn, train, wx)
    except Retry as e:
        return ci, seed, str(e), None
    est, calls = reference_fit(case)
    checks = len(calls) - 1
    ended = np.sqrt(np.sum((calls[-1] - calls[-2]) ** 2)) < case['abs_tol']
    it_ref = (checks - 1) * case['interval'] if ended else case['max_iter'] - 1
    if it_ref != it:
        return ci, seed, 'the reference ended at %d, the truth at %d' % (it_ref, it), None
    w_ref = est.w(est.x)
    alpha_ref = est.w.keywords['alpha']
    a_hi, a_lo = split(alpha)
    w_hi, w_lo = split(w)
    mine = R.kliep_fit_ref(case['x'], case['y'], case['weights_x'], case['weights_y'], case['sigma'], **R.fit_kwargs(case))
    rec = dict(alpha_ref=alpha_ref, w_ref=w_ref, max_ratio_ref=float(est.max_ratio()), iters=it, trace=trace,
               alpha_hi=a_hi, alpha_lo=a_lo, w_hi=w_hi, w_lo=w_lo, null_rows=int(len(non_null) - len(train)),
               clamped=int(np.count_nonzero(alpha_ref == 0)),
               e_alpha=R.rel_err(alpha_ref, a_hi, a_lo), e_w=R.rel_err(w_ref, w_hi, w_lo),
               mine_alpha=R.rel_err(mine['alpha'][0], a_hi, a_lo), mine_w=R.rel_err(mine['w'][0], w_hi, w_lo),
               mine_iters=int(mine['iters'][0]))
    return ci, seed, None, rec


def job_cv_truth(args):
    """The truth's score of one (scale, held-out fold) of the cross-validation case."""
    seed, si, f = args
    case = dict(R.make_case(R.CV_CASE, seed), sigma=R.CV_SIGMAS[si])
    try:
        A, b, bn, non_null, _, wxn = mp_problem(case)
        fold_of, L = R.fold_of_rows(np.array(non_null), R.CV_FOLD)
        train = [i for i in range(len(A)) if non_null[i] and fold_of[i] != f]
        held = [i for i in range(len(A)) if fold_of[i] == f]
        alpha, w, _, _ = mp_iterate(case, A, b, bn, train, wxn)
    except Retry as e:
        return si, f, str(e), None, None
    if any(w[i] == 0 for i in held):
        return si, f, None, -mp.inf, L
    return si, f, None, mp.fsum(mp.log(w[i]) * wxn[i] for i in held) / mp.fsum(wxn[i] for i in held), L


def job_cv_ref(args):
    """The reference's _KLIEP_lcv at one scale (after a fit, which sets the attributes it reads); si = -1: the scale the
    reference's optimize=True keeps; si = -2: its value at the scale 1e-3."""
    seed, si = args
    case = R.make_case(R.CV_CASE, seed)
    if si == -1:
        est, _ = reference_fit(case, optimize=True, sigma_arg=list(R.CV_SIGMAS))
        return si, float(est.sigma)
    est, _ = reference_fit(case)
    with np.errstate(all='ignore'):
        got = est._KLIEP_lcv(est.x, case['y'], 1e-3 if si == -2 else R.CV_SIGMAS[si])
    return si, float(np.ravel(got)[0])


def prefilter(ci, seed):
    """The conditions in double precision, with twice the margin: spares a 60-digit run that would be thrown away."""
    case = R.make_case(ci, seed)
    sigmas = [case['sigma']] + (list(R.CV_SIGMAS) if ci == R.CV_CASE else [])
    traces = []
    R.kliep_fit_ref(case['x'], case['y'], case['weights_x'], case['weights_y'], sigmas, traces=traces, **R.fit_kwargs(case))
    tol = case['abs_tol']
    if any(abs(t - tol) <= tol / 50 for t in traces[0]):
        return False
    top = np.concatenate([R.basis(case['x'], case['x'][:case['n']], s).max(axis=1) for s in sigmas])
    return not np.any((top >= 1e-66) & (top <= 1e-62))


def main():
    ncase = len(R.CASES)
    seeds = [c['seed'] for c in R.CASES]
    for ci in range(ncase):
        while not prefilter(ci, seeds[ci]):
            seeds[ci] += R.SEED_STEP
    print('seeds after the double-precision look:', seeds, flush=True)
    recs = [None] * ncase
    cv = None
    with ProcessPoolExecutor(WORKERS) as pool:
        pending = list(range(ncase))
        while pending or cv is None:
            futures = [pool.submit(job_case, (ci, seeds[ci])) for ci in pending]
            cv_jobs = None
            if cv is None:
                s = seeds[R.CV_CASE]
                cv_jobs = ([pool.submit(job_cv_truth, (s, si, f)) for si in range(len(R.CV_SIGMAS)) for f in range(R.CV_FOLD)],
                           [pool.submit(job_cv_ref, (s, si)) for si in [-2, -1] + list(range(len(R.CV_SIGMAS)))])
            pending = []
            for fu in futures:
                ci, seed, why, rec = fu.result()
                if why:
                    print('case %d seed %d: %s -> next seed' % (ci, seed, why), flush=True)
                    seeds[ci] += R.SEED_STEP
                    pending.append(ci)
                    if ci == R.CV_CASE:
                        cv = None
                else:
                    recs[ci] = rec
                    print('case %d seed %d: ended at %d, %d null rows, %d components clamped, max_ratio %.6g, e_ref alpha '
                          '%.2e w %.2e; restatement - truth alpha %.2e w %.2e; trace %s'
                          % (ci, seed, rec['iters'], rec['null_rows'], rec['clamped'], rec['max_ratio_ref'], rec['e_alpha'],
                             rec['e_w'], rec['mine_alpha'], rec['mine_w'], ' '.join('%.4g' % t for t in rec['trace'])),
                          flush=True)
                    assert rec['mine_iters'] == rec['iters']
            if cv_jobs is not None:
                S, F = len(R.CV_SIGMAS), R.CV_FOLD
                scores = [[None] * F for _ in range(S)]
                L = [None] * S
                why_cv = None
                for fu in cv_jobs[0]:
                    si, f, why, sc, Ls = fu.result()
                    why_cv = why_cv or why
                    scores[si][f], L[si] = sc, Ls
                ref = dict(fu.result() for fu in cv_jobs[1])
                if why_cv is None:
                    lcv = [mp.fsum(row) / F for row in scores]
                    for si in range(S):
                        if np.isfinite(ref[si]) != bool(mp.isfinite(lcv[si])):
                            why_cv = 'scale %g: the reference gives %r, the truth %s' % (R.CV_SIGMAS[si], ref[si], lcv[si])
                if why_cv is not None:
                    print('cross-validation, seed %d: %s -> next seed' % (seeds[R.CV_CASE], why_cv), flush=True)
                    if R.CV_CASE not in pending:
                        seeds[R.CV_CASE] += R.SEED_STEP
                        pending.append(R.CV_CASE)
                    cv = None
                elif R.CV_CASE not in pending:
                    cv = dict(scores=scores, lcv=lcv, ref=ref, L=L)

    out = dict(seeds=np.array(seeds), iters=np.array([r['iters'] for r in recs]),
               max_ratio_ref=np.array([r['max_ratio_ref'] for r in recs]),
               e_ref_alpha=np.array([r['e_alpha'] for r in recs]), e_ref_w=np.array([r['e_w'] for r in recs]),
               null_rows=np.array([r['null_rows'] for r in recs]), clamped=np.array([r['clamped'] for r in recs]))
    nmax, Nmax = max(c['n'] for c in R.CASES), max(c['Nx'] for c in R.CASES)
    tmax = max(len(r['trace']) for r in recs)
    for key, width in (('alpha_ref', nmax), ('alpha_hi', nmax), ('alpha_lo', nmax), ('w_ref', Nmax), ('w_hi', Nmax),
                       ('w_lo', Nmax), ('trace', tmax)):
        a = np.full((ncase, width), np.nan)
        for ci, r in enumerate(recs):
            a[ci, :len(r[key])] = r[key]
        out[key] = a
    S, F = len(R.CV_SIGMAS), R.CV_FOLD
    finite = [v for row in cv['scores'] for v in row if mp.isfinite(v)]
    scale = max(abs(float(v)) for v in finite)
    sc_hi, sc_lo = np.empty((S, F)), np.empty((S, F))
    for si in range(S):
        for f in range(F):
            v = cv['scores'][si][f]
            sc_hi[si, f], sc_lo[si, f] = (float(v), float(v - mpf(float(v)))) if mp.isfinite(v) else (float(v), 0.0)
    lcv_hi = np.array([float(v) for v in cv['lcv']])
    lcv_lo = np.array([float(v - mpf(h)) if np.isfinite(h) else 0.0 for v, h in zip(cv['lcv'], lcv_hi)])
    lcv_ref = np.array([cv['ref'][si] for si in range(S)])
    ok = np.isfinite(lcv_ref)
    e_cv = float(np.max(np.abs((lcv_ref[ok] - lcv_hi[ok]) - lcv_lo[ok])) / scale)
    out.update(cv_sigmas=np.array(R.CV_SIGMAS), cv_fold=F, cv_scores_hi=sc_hi, cv_scores_lo=sc_lo, cv_lcv_hi=lcv_hi,
               cv_lcv_lo=lcv_lo, cv_lcv_ref=lcv_ref, cv_L=np.array(cv['L']), cv_scale=scale, e_ref_cv=e_cv,
               cv_ref_choice=cv['ref'][-1], cv_small_sigma=1e-3, cv_small_ref=cv['ref'][-2])
    print('cross-validation: L %s, reference lcv %s, truth %s, e_ref %.2e of the largest finite score %.4g; the '
          'reference\'s optimize=True keeps sigma %g; its lcv at 1e-3: %r'
          % (cv['L'], lcv_ref, lcv_hi, e_cv, scale, cv['ref'][-1], cv['ref'][-2]))
    e_max = max(out['e_ref_alpha'].max(), out['e_ref_w'].max(), e_cv)
    out['e_ref_max'] = e_max
    print('largest relative e_ref %.3e -> bound 16 x = %.3e' % (e_max, 16 * e_max))
    path = os.path.join(ROOT, 'tests', 'golden', 'kliep.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
