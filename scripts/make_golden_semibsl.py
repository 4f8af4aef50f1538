"""Records tests/golden/semibsl.npz from the reference ELFI's semiparametric synthetic likelihood (run where the reference
is installed; oracle/ref_shim.py makes it importable).  The reference's function uses np.NINF, which this NumPy no longer
has: the script sets the alias in its own process, so everything that needs the reference's semiparametric values lives
here and no test calls that function.

For every case of tests/semibsl_ref.py (CASES x CONFIGS, each with its tied twin) it stores
  ref      what pdf_methods.semi_param_kernel_estimate returns,
  truth    the same quantity of the same float inputs in 60-digit arithmetic, as a double-double (hi, lo): the inputs are
           taken as exact, the ranks are exact, Phi^-1(p) = sqrt 2 erfinv(2 p - 1) at the exact rational p = r / (n + 1),
  e_ref    |ref - truth|,
  u        the integrals of the density estimates, rounded to double.
Tables: Phi^-1(i / (n + 1)), i = 1..n, for n in SCORE_TABLES (the exact rational; hi, lo) with the relative error of
SciPy's ndtri at the double i / (n + 1), and Phi^-1(u) for u = 1e-1 ... 1e-298 with ndtri's error (the yardstick of
the tail figures in csrc/special.hpp; eta is no output, so no test reads that table).
On the reference's MA2 model with the reference's semiparametric likelihood: log_SL_stdev and select_penalty (outputs, and
ref / truth of every likelihood they evaluate) and one short elfi.BSL chain.  Synthetic inputs are not stored: the tests
regenerate them from the recipe.

    python scripts/make_golden_semibsl.py
"""
import os
import sys

import mpmath as mp
import numpy as np
from scipy.special import ndtri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import ref_shim  # noqa: E402
import semibsl_ref as R  # noqa: E402

mp.mp.dps = 60
mpf = mp.mpf


def mp_ppf(p):
    return mp.sqrt(2) * mp.erfinv(2 * p - 1)


def mp_ppf_tail(u):
    """Phi^-1 of a tiny u: 2 u - 1 needs as many digits as u has zeros."""
    with mp.workdps(400):
        return +(mp.sqrt(2) * mp.erfinv(2 * mpf(float(u)) - 1))


def truth_parts(X, y):
    """(sum of logpdf, eta, u, rho unshrunk) in mpmath."""
    n, m = X.shape
    lp, eta, us, Q = mpf(0), [], [], []
    table = {}
    for j in range(m):
        col = [mpf(float(v)) for v in X[:, j]]
        mu = mp.fsum(col) / n
        var = mp.fsum((v - mu) ** 2 for v in col) / (n - 1)
        h = (mpf(3) * n / 4) ** (mpf(-1) / 5) * mp.sqrt(var)
        zs = [(mpf(float(y[j])) - v) / h for v in col]
        lp += mp.log(mp.fsum(mp.exp(-z * z / 2) for z in zs) / n / h / mp.sqrt(2 * mp.pi))
        u = mp.fsum(mp.ncdf(z) for z in zs) / n
        us.append(u)
        eta.append(mp_ppf(u))
        q = []
        for r in R.ranks(X[:, j]):
            r = float(r)
            if r not in table:
                table[r] = mp_ppf(mpf(r) / (n + 1))
            q.append(table[r])
        Q.append(q)
    den = mp.fsum(mp_ppf(mpf(i) / (n + 1)) ** 2 for i in range(1, n + 1))
    rho = [[mpf(1) if a == b else None for b in range(m)] for a in range(m)]
    for a in range(m):
        for b in range(a):
            rho[a][b] = rho[b][a] = mp.fdot(Q[a], Q[b]) / den
    return lp, eta, us, rho


def truth_loglik(parts, penalty=None):
    lp, eta, us, rho = parts
    m = len(eta)
    g = mpf(1) if penalty is None else 1 - mpf(float(penalty))
    S = [[mpf(1) if a == b else g * rho[a][b] for b in range(m)] for a in range(m)]
    L = [[mpf(0)] * m for _ in range(m)]
    for j in range(m):
        d = S[j][j] - mp.fsum(L[j][k] * L[j][k] for k in range(j))
        assert d > 0
        L[j][j] = mp.sqrt(d)
        for i in range(j + 1, m):
            L[i][j] = (S[i][j] - mp.fdot(L[i][:j], L[j][:j])) / L[j][j]
    z = []
    for i in range(m):
        z.append((eta[i] - mp.fdot(L[i][:i], z)) / L[i][i])
    logdet = 2 * mp.fsum(mp.log(L[j][j]) for j in range(m))
    return -(logdet + mp.fsum(v * v for v in z) - mp.fsum(v * v for v in eta)) / 2 + lp


def split(t):
    hi = float(t)
    return hi, float(t - mpf(hi))


def main():
    elfi = ref_shim.install()
    np.NINF = -np.inf           # pdf_methods.py:229 and pre_sample_methods.py:303 still use the name
    import elfi.clients.native as native
    native.set_as_default()
    from elfi.examples import ma2
    from elfi.methods.bsl import pdf_methods as P
    from elfi.methods.bsl import pre_sample_methods as PS
    out = {}

    def ref_value(X, y, **kw):
        if X.shape[1] == 1:
            # one summary: the reference's function squeezes ssy to 0-d and fails at ssy[j]; its value is what its column
            # loop computes (pdf_methods.py:226-227) -- the copula term of a single column is zero, with any penalty
            import scipy.stats as ss
            return float(ss.gaussian_kde(X[:, 0], bw_method='silverman').logpdf(y[0])[0])
        return float(np.ravel(P.semi_param_kernel_estimate(X, y, **kw))[0])

    # ---- synthetic cases: axis 1 = (plain, tied twin) ------------------------------------------------------------
    shape = (len(R.CASES), 2, len(R.CONFIGS))
    ref, hi, lo, e_ref = (np.empty(shape) for _ in range(4))
    u_hi = np.full((len(R.CASES), 2, 64), np.nan)
    for ci, case in enumerate(R.CASES):
        for ti in (0, 1):
            X, y = R.make_case(ci, tied=bool(ti))
            parts = truth_parts(X, y)
            u_hi[ci, ti, :case[2]] = [float(u) for u in parts[2]]
            for ki, name in enumerate(R.CONFIGS):
                kw = R.config_kwargs(name)
                r = ref_value(X, y, **kw)
                t = truth_loglik(parts, kw.get('penalty'))
                ref[ci, ti, ki] = r
                hi[ci, ti, ki], lo[ci, ti, ki] = split(t)
                e_ref[ci, ti, ki] = float(abs(mpf(r) - t))
                mine = R.semi_loglik_ref(X, y, **kw)[0, 0, 0]
                print('case n=%d m=%d %s %-8s ref % .17g  e_ref %.2e  restatement-truth %.2e'
                      % (case[1], case[2], 'tied ' if ti else 'plain', name, r, e_ref[ci, ti, ki],
                         float(abs(mpf(float(mine)) - t))), flush=True)
    out.update(cases=np.array(R.CASES, dtype=float), ref=ref, truth_hi=hi, truth_lo=lo, e_ref=e_ref, u=u_hi)

    # ---- tables of the inverse normal cdf ------------------------------------------------------------------------
    for n in R.SCORE_TABLES:
        t = [mp_ppf(mpf(i) / (n + 1)) for i in range(1, n + 1)]
        got = ndtri(np.arange(1, n + 1) / (n + 1))
        rel = np.array([float(abs((mpf(float(g)) - v) / v)) if v != 0 else abs(float(g)) for g, v in zip(got, t)])
        out['ppf_%d_hi' % n] = np.array([split(v)[0] for v in t])
        out['ppf_%d_lo' % n] = np.array([split(v)[1] for v in t])
        out['ppf_%d_ndtri_rel' % n] = rel
        print('Phi^-1(i / %d): ndtri max relative error %.3e' % (n + 1, rel.max()))
    us = 10.0 ** -np.arange(1.0, 300.0, 3.0)
    t = [mp_ppf_tail(u) for u in us]
    out.update(tail_u=us, tail_hi=np.array([split(v)[0] for v in t]), tail_lo=np.array([split(v)[1] for v in t]),
               tail_ndtri_rel=np.array([float(abs((mpf(float(g)) - v) / v)) for g, v in zip(ndtri(us), t)]))
    print('Phi^-1(u), u = 1e-1 ... 1e-298: ndtri max relative error %.3e' % out['tail_ndtri_rel'].max())

    # ---- the reference's MA2 model -------------------------------------------------------------------------------
    theta, feats = [0.6, 0.2], ['S1', 'S2']

    def matrices(model, max_sim, M, seed):
        at = {name: value for name, value in zip(model.parameter_names, theta)}
        obs = np.array([[np.ravel(model[f].observed)[0] for f in feats]])
        mats = []
        for child in np.random.SeedSequence(seed).generate_state(M):
            sims = model.generate(max_sim, outputs=feats, with_values=at, seed=child)
            mats.append(np.stack([np.ravel(sims[f]) for f in feats], axis=1))
        return mats, obs

    sl_n, sl_M, sl_seed = [50, 100], 5, 1
    model = ma2.get_model(seed_obs=4)
    out.update(sl_n_sim=np.array(sl_n), sl_M=sl_M, sl_seed=sl_seed,
               sl_std=PS.log_SL_stdev(model, theta, sl_n, feats, likelihood=P.semiparametric_likelihood(), M=sl_M,
                                      seed=sl_seed))
    mats, obs = matrices(model, max(sl_n), sl_M, sl_seed)
    sref = np.empty((sl_M, len(sl_n)))
    shi, slo = np.empty_like(sref), np.empty_like(sref)
    for i, Xm in enumerate(mats):
        for k, n in enumerate(sl_n):
            sref[i, k] = ref_value(Xm[:n], obs)
            shi[i, k], slo[i, k] = split(truth_loglik(truth_parts(Xm[:n], obs.ravel())))
    assert np.array_equal(np.std(np.ascontiguousarray(sref.T), axis=1), out['sl_std'])
    out.update(sl_ref=sref, sl_truth_hi=shi, sl_truth_lo=slo)

    pen_n, pen_M, pen_seed, lmdas = [50, 100], 5, 2, [0.2, 0.4, 0.6, 0.8]
    pl, ps = PS.select_penalty(model, pen_n, theta, feats, likelihood=P.semiparametric_likelihood(), lmdas=lmdas, M=pen_M,
                               shrinkage='warton', seed=pen_seed)
    out.update(pen_n_sim=np.array(pen_n), pen_M=pen_M, pen_seed=pen_seed, pen_grid=np.array(lmdas), pen_lmdas=pl,
               pen_stds=ps)
    mats, obs = matrices(model, max(pen_n), pen_M, pen_seed)
    pref = np.empty((pen_M, len(pen_n), len(lmdas)))
    phi, plo = np.empty_like(pref), np.empty_like(pref)
    for i, Xm in enumerate(mats):
        for k, n in enumerate(pen_n):
            parts = truth_parts(Xm[:n], obs.ravel())
            for j, lm in enumerate(lmdas):
                pref[i, k, j] = ref_value(Xm[:n], obs, shrinkage='warton', penalty=lm)
                phi[i, k, j], plo[i, k, j] = split(truth_loglik(parts, lm))
    out.update(pen_ref=pref, pen_truth_hi=phi, pen_truth_lo=plo)

    # ---- one short BSL chain -------------------------------------------------------------------------------------
    bsl_n, bsl_round, bsl_seed = 100, 100, 3
    model = ma2.get_model(seed_obs=4)
    bsl = elfi.BSL(model, bsl_round, feature_names=feats, likelihood=P.semiparametric_likelihood(), seed=bsl_seed)
    bsl.sample(bsl_n, sigma_proposals=0.02 * np.eye(2), params0=theta, bar=False)
    out.update(bsl_n=bsl_n, bsl_round=bsl_round, bsl_seed=bsl_seed, bsl_params=bsl.state['params'].copy(),
               bsl_logpost=bsl.state['logposterior'].copy())
    moved = np.any(np.diff(bsl.state['params'], axis=0) != 0, axis=1)
    print('BSL chain: %d of %d proposals accepted' % (moved.sum(), bsl_n - 1))

    path = os.path.join(ROOT, 'tests', 'golden', 'semibsl.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    for m in sorted(set(c[2] for c in R.CASES)):
        rows = [i for i, c in enumerate(R.CASES) if c[2] == m]
        print('m=%d  max e_ref %.3e' % (m, e_ref[rows].max()))
    print('MA2 (m=2) max e_ref: log_SL_stdev %.3e  select_penalty %.3e'
          % (np.abs((sref - shi) - slo).max(), np.abs((pref - phi) - plo).max()))


if __name__ == '__main__':
    main()
