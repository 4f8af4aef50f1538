"""Records tests/golden/twostage.npz from the reference ELFI's TwoStageSelection (run where the reference is installed;
oracle/ref_shim.py makes it importable).

For every synthetic case of tests/twostage_ref.py (inputs are regenerated from the recipe, not stored) it stores
  ref_entropy, ref_mrsse       TwoStageSelection._calc_entropy (cKDTree) and ._calc_MRSSE on the case's float inputs,
  truth_entropy, truth_mrsse   the same quantities in 40-digit arithmetic (mpmath) on the same float inputs, rounded to double,
  e_entropy, e_mrsse           |reference - truth|.
The k-th neighbour of the truth is taken among the k + 4 nearest points by float distance; the script checks in 40 digits
that the first point left out is farther than the k-th by more than any float error could hide.

For the MA2 run (tests/twostage_ref.py: MA2_RUN, the candidates ac1, ac2, mean, var) it stores results only: the entropy
and the MRSSE of every combination, the names of the minimum-entropy and of the chosen combination and the accepted
parameters of the combinations MA2_RECORDED.  It refuses to write when the two smallest entropies, or the two smallest
MRSSEs, are closer than 1000 x the test's bound: the choice must not hang on rounding.

    python scripts/make_golden_twostage.py
"""
import logging
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import ref_shim  # noqa: E402
import twostage_ref as R  # noqa: E402

mp.mp.dps = 40
mpf = mp.mpf


def mp_d2(a, b):
    return mp.fsum((mpf(float(x)) - mpf(float(y))) ** 2 for x, y in zip(a, b))


def truth_entropy(T, k):
    n, q = T.shape
    d2 = R.squared_distances(T)
    near = np.argsort(d2, axis=1, kind='stable')[:, :min(n, k + 4)]
    logs = []
    for i in range(n):
        cand = sorted(mp_d2(T[i], T[j]) for j in near[i])
        kth = cand[k - 1]
        if len(cand) < n:
            # every point left out has a float d2 >= that of the last candidate; float d2 carries <= (q + 2) eps relative
            assert cand[-1] * (1 - 4 * (q + 2) * mpf(R.EPS)) > kth, 'case needs more candidates'
        logs.append(mp.log(mp.sqrt(kth)))
    E = (mpf(q) / 2 * mp.log(mp.pi) - mp.loggamma(mpf(q) / 2 + 1) - mp.digamma(k) + mp.log(n)
         + mpf(q) / n * mp.fsum(logs))
    return E


def truth_mrsse(T, Cl):
    roots = []
    for c in Cl:
        roots.append(mp.sqrt(mp.fsum((mpf(float(x)) - mpf(float(cd))) ** 2 for row in T for x, cd in zip(row, c))))
    return mp.fsum(roots) / len(Cl)


def main():
    elfi = ref_shim.install()
    from elfi.methods.diagnostics import TwoStageSelection
    bare = TwoStageSelection.__new__(TwoStageSelection)      # the two formulas use no state of the object
    nc = len(R.CASES)
    out = {k: np.zeros(nc) for k in ('ref_entropy', 'ref_mrsse', 'truth_entropy', 'truth_mrsse', 'e_entropy', 'e_mrsse')}
    for ci, case in enumerate(R.CASES):
        T, Cl, k = R.make_case(ci)
        ref_e = float(bare._calc_entropy(T, len(T), k))
        ref_m = float(bare._calc_MRSSE(None, Cl, T))
        te, tm = truth_entropy(T, k), truth_mrsse(T, Cl)
        out['ref_entropy'][ci], out['ref_mrsse'][ci] = ref_e, ref_m
        out['truth_entropy'][ci], out['truth_mrsse'][ci] = float(te), float(tm)
        out['e_entropy'][ci], out['e_mrsse'][ci] = float(abs(mpf(ref_e) - te)), float(abs(mpf(ref_m) - tm))
        print('case %d n=%d q=%d k=%d J=%d  entropy % .15g e_ref %.2e  restatement %.2e | mrsse %.15g e_ref %.2e  restatement %.2e'
              % (ci, len(T), T.shape[1], k, len(Cl), float(te), out['e_entropy'][ci],
                 float(abs(mpf(float(R.knn_entropy_ref(T, k)[0])) - te)), float(tm), out['e_mrsse'][ci],
                 float(abs(mpf(float(R.mrsse_ref(T, Cl)[0])) - tm))), flush=True)
    out['cases'] = np.array(R.CASES, dtype=float)

    # ---- the MA2 run: the reference's own class, one Rejection per combination
    run = R.MA2_RUN
    cands = R.ma2_candidates()
    sel = TwoStageSelection(R.ma2_simulator(elfi), 'euclidean', list_ss=cands, seed=run['seed'])
    combos = [tuple(f.__name__ for f in c) for c in sel.ss_candidates]
    assert combos == R.combination_names()
    lines = []
    handler = logging.Handler()
    handler.emit = lambda record: lines.append(record.getMessage())
    log = logging.getLogger('elfi.methods.diagnostics')
    log.addHandler(handler)
    log.setLevel(logging.INFO)
    kept = {}
    inner = sel._obtain_accepted_thetas

    def recording(set_ss, *a):
        thetas = inner(set_ss, *a)
        kept[tuple(f.__name__ for f in set_ss)] = np.array(thetas)
        return thetas
    sel._obtain_accepted_thetas = recording
    chosen = sel.run(run['n_sim'], run['n_acc'], run['n_closest'], batch_size=run['batch_size'], k=run['k'])
    log.removeHandler(handler)
    E = np.array([bare._calc_entropy(kept[c], run['n_acc'], run['k']) for c in combos])
    i_me = min(range(len(combos)), key=lambda i: (E[i], len(combos[i])))
    closest = kept[combos[i_me]][:run['n_closest']]
    M = np.array([bare._calc_MRSSE(None, closest, kept[c]) for c in combos])
    i_ms = min(range(len(combos)), key=lambda i: (M[i], len(combos[i])))
    assert combos[i_ms] == tuple(f.__name__ for f in chosen), (combos[i_ms], chosen)
    assert any('minimum entropy' in ln and str(list(combos[i_me])) in ln for ln in lines), lines[-3:]
    for name, v, e_ref in (('entropy', E, out['e_entropy']), ('MRSSE', M, out['e_mrsse'])):
        two = np.sort(v)[:2]
        same = [i for i, c in enumerate(R.CASES) if c[2] == 2]
        need = 1000.0 * R.bound(e_ref[same], two[0])
        print('%s: smallest %.6f, next %.6f (gap %.3e, needed %.3e)' % (name, two[0], two[1], two[1] - two[0], need))
        if not two[1] - two[0] > need:
            raise SystemExit('the two smallest %s values are too close: the choice would hang on rounding' % name)
    for c, e, r in zip(combos, E, M):
        print('  %-28s entropy % .6f  MRSSE %.6f' % (', '.join(c), e, r))
    print('minimum entropy:', combos[i_me], ' chosen:', combos[i_ms])
    out.update(ma2_entropy=E, ma2_mrsse=M, ma2_min_entropy=np.array(combos[i_me]), ma2_chosen=np.array(combos[i_ms]),
               ma2_combinations=np.array([','.join(c) for c in combos]))
    for c in R.MA2_RECORDED:
        out['ma2_accepted_' + '_'.join(c)] = kept[c]
    path = os.path.join(ROOT, 'tests', 'golden', 'twostage.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
