"""Records tests/golden/synlik.npz from the reference ELFI's own BSL functions (run where the reference is installed;
oracle/ref_shim.py makes it importable).

For every synthetic case of tests/synlik_ref.py (CASES x CONFIGS) it stores
  ref      what the reference's pdf_methods function returns,
  truth    the same quantity of the same float inputs in exact / 60-digit arithmetic, as a double-double (hi, lo): the
           sums of the moments are exact integer sums of the scaled inputs, the rest runs in mpmath,
  e_ref    |ref - truth|.
On the reference's MA2 model: log_SL_stdev and select_penalty (outputs, and ref / truth of every likelihood they
evaluate) and one short elfi.BSL chain.  Synthetic inputs are not stored: the tests regenerate them from the recipe.

    python scripts/make_golden_synlik.py
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import ref_shim  # noqa: E402
import synlik_ref as R  # noqa: E402

mp.mp.dps = 60
mpf = mp.mpf


# ---- exact moments -----------------------------------------------------------------------------------------------
def _bits(*arrays):
    """Smallest s with x 2^s an integer for every entry."""
    s = 0
    for a in arrays:
        for x in np.asarray(a, dtype=float).ravel():
            s = max(s, float(x).as_integer_ratio()[1].bit_length() - 1)
    return s


def _ints(a, s):
    a = np.asarray(a, dtype=float)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        num, den = float(a[idx]).as_integer_ratio()
        out[idx] = num << (s - (den.bit_length() - 1))
    return out


def exact_moments(X, y, W=None):
    """(mean, cov, y) as lists of mpf, of the rows (after whitening) -- no rounding before the final divisions."""
    s = _bits(X, y) if W is None else _bits(X, y, W)
    Xi, yi = _ints(X, s), _ints(y, s)
    t = s
    if W is not None:
        Wi = _ints(W, s)
        Xi, yi, t = Xi @ Wi.T, Wi @ yi, 2 * s
    n, m = Xi.shape
    S1 = Xi.sum(axis=0)
    S2 = Xi.T @ Xi
    one, two = mpf(2) ** t, mpf(2) ** (2 * t)
    mean = [mpf(int(S1[j])) / n / one for j in range(m)]
    cov = [[mpf(int(n * S2[i, j] - S1[i] * S1[j])) / (n * (n - 1)) / two for j in range(m)] for i in range(m)]
    return mean, cov, [mpf(int(v)) / one for v in yi]


def chol_logdet_quad(S, v):
    m = len(v)
    L = [[mpf(0)] * m for _ in range(m)]
    for j in range(m):
        d = S[j][j] - mp.fsum(L[j][k] * L[j][k] for k in range(j))
        if d <= 0:
            return None
        L[j][j] = mp.sqrt(d)
        for i in range(j + 1, m):
            L[i][j] = (S[i][j] - mp.fsum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
    z = []
    for i in range(m):
        z.append((v[i] - mp.fsum(L[i][k] * z[k] for k in range(i))) / L[i][i])
    return 2 * mp.fsum(mp.log(L[j][j]) for j in range(m)), mp.fsum(x * x for x in z)


def mvn(y, mean, S):
    lq = chol_logdet_quad(S, [a - b for a, b in zip(y, mean)])
    if lq is None:
        return -mp.inf
    return -(len(y) * mp.log(2 * mp.pi) + lq[0] + lq[1]) / 2


def warton(S, penalty):
    g, m = 1 - mpf(float(penalty)), len(S)
    d = [mp.sqrt(S[i][i] + mpf(1e-5)) for i in range(m)]
    return [[(g * S[i][j] / (d[i] * d[j]) + ((1 - g) if i == j else 0)) * d[i] * d[j] for j in range(m)] for i in range(m)]


def logc(k, v):
    return -mpf(k) * v / 2 * mp.log(2) - mpf(k) * (k - 1) / 4 * mp.log(mp.pi) - mp.fsum(mp.loggamma(mpf(v - x) / 2) for x in range(k))


def truth_loglik(X, y, variant=None, shrinkage=None, penalty=None, whitening=None, gamma=None, adjustment=None, mom=None):
    mean, S, yv = mom if mom is not None else exact_moments(X, y, whitening)
    n, d = len(X), len(yv)
    if shrinkage == 'warton':
        S = warton(S, penalty)
    std = [mp.sqrt(S[i][i]) for i in range(d)]
    if adjustment == 'mean':
        mean = [mean[i] + std[i] * mpf(float(gamma[i])) for i in range(d)]
    if adjustment == 'variance':
        S = [[S[i][j] + ((std[i] * mpf(float(gamma[i]))) ** 2 if i == j else 0) for j in range(d)] for i in range(d)]
    if variant != 'unbiased':
        return mvn(yv, mean, S)
    v = [a - b for a, b in zip(yv, mean)]
    psi = [[(n - 1) * S[i][j] - v[i] * v[j] / (1 - mpf(1) / n) for j in range(d)] for i in range(d)]
    a, b = chol_logdet_quad(S, v), chol_logdet_quad(psi, v)
    return (-mpf(d) / 2 * mp.log(2 * mp.pi) + logc(d, n - 2) - logc(d, n - 1) - mpf(d) / 2 * mp.log(1 - mpf(1) / n)
            - mpf(n - d - 2) / 2 * (mp.log(n - 1) + a[0]) + mpf(n - d - 3) / 2 * b[0])


def split(t):
    hi = float(t)
    return hi, float(t - mpf(hi))


def main():
    elfi = ref_shim.install()
    import elfi.clients.native as native
    native.set_as_default()
    from elfi.examples import ma2
    from elfi.methods.bsl import pdf_methods as P
    from elfi.methods.bsl import pre_sample_methods as PS
    out = {}

    # ---- synthetic cases ---------------------------------------------------------------------------------------
    ref = np.empty((len(R.CASES), len(R.CONFIGS)))
    hi, lo, e_ref = np.empty_like(ref), np.empty_like(ref), np.empty_like(ref)
    for ci, case in enumerate(R.CASES):
        X, y, W, gamma = R.make_case(*case)
        plain, white = exact_moments(X, y), exact_moments(X, y, W)
        for ki, name in enumerate(R.CONFIGS):
            kw = R.config_kwargs(name, W, gamma)
            if name == 'unbiased':
                r = P.gaussian_syn_likelihood_ghurye_olkin(X, y)[0]
            elif name in ('mean', 'variance'):
                r = P.syn_likelihood_misspec(X, y, gamma, name)
            else:
                r = P.gaussian_syn_likelihood(X, y[None, :], **kw)[0]
            t = truth_loglik(X, y, mom=white if name == 'whitening' else plain, **kw)
            ref[ci, ki] = r
            hi[ci, ki], lo[ci, ki] = split(t)
            e_ref[ci, ki] = float(abs(mpf(float(r)) - t))
            mine = R.syn_loglik_ref(X, y, **kw)[0, 0, 0]
            print('case n=%d m=%d %-9s ref % .17g  e_ref %.2e  restatement-truth %.2e'
                  % (case[1], case[2], name, r, e_ref[ci, ki], float(abs(mpf(float(mine)) - t))), flush=True)
    out.update(cases=np.array(R.CASES, dtype=float), ref=ref, truth_hi=hi, truth_lo=lo, e_ref=e_ref)
    # the moments of the full group (what BSL keeps for the gamma sampler): case 1, NumPy's own
    X, y, W, gamma = R.make_case(*R.CASES[1])
    out.update(mom_mean=X.mean(0), mom_cov=np.cov(X, rowvar=False))

    # ---- the reference's MA2 model -----------------------------------------------------------------------------
    theta, feats = [0.6, 0.2], ['S1', 'S2']

    def matrices(model, max_sim, M, seed):
        at = {name: value for name, value in zip(model.parameter_names, theta)}
        obs = np.array([[np.ravel(model[f].observed)[0] for f in feats]])
        mats = []
        for child in np.random.SeedSequence(seed).generate_state(M):
            sims = model.generate(max_sim, outputs=feats, with_values=at, seed=child)
            mats.append(np.stack([np.ravel(sims[f]) for f in feats], axis=1))
        return mats, obs

    sl_n, sl_M, sl_seed = [50, 100, 200], 20, 1
    model = ma2.get_model(seed_obs=4)
    out.update(sl_n_sim=np.array(sl_n), sl_M=sl_M, sl_seed=sl_seed,
               sl_std=PS.log_SL_stdev(model, theta, sl_n, feats, M=sl_M, seed=sl_seed))
    mats, obs = matrices(model, max(sl_n), sl_M, sl_seed)
    sref = np.empty((sl_M, len(sl_n)))
    shi, slo = np.empty_like(sref), np.empty_like(sref)
    for i, Xm in enumerate(mats):
        for k, n in enumerate(sl_n):
            sref[i, k] = P.gaussian_syn_likelihood(Xm[:n], obs)[0]
            shi[i, k], slo[i, k] = split(truth_loglik(Xm[:n], obs.ravel()))
    assert np.array_equal(np.std(np.ascontiguousarray(sref.T), axis=1), out['sl_std'])
    out.update(sl_ref=sref, sl_truth_hi=shi, sl_truth_lo=slo)

    pen_n, pen_M, pen_seed = [100, 200], 20, 2
    lmdas = list(np.arange(0.2, 0.8, 0.02))
    pl, ps = PS.select_penalty(model, pen_n, theta, feats, M=pen_M, shrinkage='warton', seed=pen_seed)
    out.update(pen_n_sim=np.array(pen_n), pen_M=pen_M, pen_seed=pen_seed, pen_lmdas=pl, pen_stds=ps)
    mats, obs = matrices(model, max(pen_n), pen_M, pen_seed)
    pref = np.empty((pen_M, len(pen_n), len(lmdas)))
    phi, plo = np.empty_like(pref), np.empty_like(pref)
    for i, Xm in enumerate(mats):
        for k, n in enumerate(pen_n):
            mom = exact_moments(Xm[:n], obs.ravel())
            for j, lm in enumerate(lmdas):
                pref[i, k, j] = P.gaussian_syn_likelihood(Xm[:n], obs, shrinkage='warton', penalty=lm)[0]
                phi[i, k, j], plo[i, k, j] = split(truth_loglik(Xm[:n], obs.ravel(), shrinkage='warton', penalty=lm, mom=mom))
    out.update(pen_ref=pref, pen_truth_hi=phi, pen_truth_lo=plo)

    # ---- one short BSL chain -----------------------------------------------------------------------------------
    bsl_n, bsl_round, bsl_seed = 300, 100, 3
    model = ma2.get_model(seed_obs=4)
    bsl = elfi.BSL(model, bsl_round, feature_names=feats, seed=bsl_seed)
    bsl.sample(bsl_n, sigma_proposals=0.02 * np.eye(2), params0=theta, bar=False)
    out.update(bsl_n=bsl_n, bsl_round=bsl_round, bsl_seed=bsl_seed, bsl_params=bsl.state['params'].copy(),
               bsl_logpost=bsl.state['logposterior'].copy())
    moved = np.any(np.diff(bsl.state['params'], axis=0) != 0, axis=1)
    print('BSL chain: %d of %d proposals accepted' % (moved.sum(), bsl_n - 1))

    path = os.path.join(ROOT, 'tests', 'golden', 'synlik.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    for m in sorted(set(c[2] for c in R.CASES)):
        rows = [i for i, c in enumerate(R.CASES) if c[2] == m]
        print('m=%d  max e_ref %.3e' % (m, e_ref[rows].max()))
    print('MA2 (m=2) max e_ref: log_SL_stdev %.3e  select_penalty %.3e'
          % (np.abs((sref - shi) - slo).max(), np.abs((pref - phi) - plo).max()))


if __name__ == '__main__':
    main()
