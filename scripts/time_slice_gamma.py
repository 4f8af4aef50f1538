"""Times the gamma slice samplers (csrc/slice_gamma.hip) against the reference's functions on the same box.

Host wall clock around the synchronising call, copies included; 3 warm-up + 20 timed calls, median (min - max).
  * one problem at m = 32 and 64, both adjustments: elfi_amd.slice_gamma_mean / slice_gamma_variance (the drop-ins a chain
    calls, RandomState bookkeeping included) against the reference's functions with the same generator;
  * the same problems with max_iter = 0 -- every coordinate steps out once and nothing else: for the variance form that
    is m factorisations, 2 m triangular solves and m trials, for the mean form one factorisation;
  * G = 64 problems at m = 32 in one call of elfi_amd.slice_gamma;
  * 100 iterations of an R-BSL-V chain on elfi_amd.toad_model (48 summaries) with the reference's sampler and with
    gamma_sampler='device'.
The reference is the copy oracle/make_ref.sh makes (oracle/ref_shim.py).

    python scripts/time_slice_gamma.py [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle')):
    sys.path.insert(0, p)

WARM, REPS = 3, 20
TAU, W = 0.5, 1.0


def state(adjustment, m, seed):
    """A chain's state: the moments of 4 m + 20 simulated summary rows, an observation, gamma and its log-likelihood."""
    rs = np.random.RandomState(seed)
    X = rs.randn(4 * m + 20, m) @ (np.eye(m) + 0.3 * rs.randn(m, m) / np.sqrt(m)) * (0.5 + rs.rand(m))
    mean, cov = X.mean(0) + rs.randn(m), np.cov(X, rowvar=False)
    std = np.sqrt(np.diag(cov))
    y = mean + std * rs.randn(m)
    gamma = rs.laplace(0.0, 0.3, m) if adjustment == 'mean' else rs.exponential(TAU, m)
    C = cov if adjustment == 'mean' else cov + np.diag((std * gamma) ** 2)
    r = y - mean - (std * gamma if adjustment == 'mean' else 0.0)
    L = np.linalg.cholesky(C)
    z = np.linalg.solve(L, r)
    loglik = -0.5 * (m * np.log(2 * np.pi) + 2 * np.log(np.diag(L)).sum() + z @ z)
    return y, loglik, gamma, mean, cov


def timed(fn):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=float(min(t)), max_ms=float(max(t)))


def show(label, r):
    print('%-58s %9.3f ms (%.3f - %.3f)' % (label, r['median_ms'], r['min_ms'], r['max_ms']), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--chain-iterations', type=int, default=100)
    args = ap.parse_args()
    import ref_shim
    elfi = ref_shim.install()
    import elfi.clients.native as native
    native.set_as_default()
    from elfi.methods.bsl.slice_gamma_mean import slice_gamma_mean as ref_mean
    from elfi.methods.bsl.slice_gamma_variance import slice_gamma_variance as ref_variance
    import elfi_amd
    ctx = elfi_amd.default_context()
    print(ctx.device_info()['name'])
    res = {}
    device = {'mean': elfi_amd.slice_gamma_mean, 'variance': elfi_amd.slice_gamma_variance}
    reference = {'mean': ref_mean, 'variance': ref_variance}
    for m in (32, 64):
        for adjustment in ('mean', 'variance'):
            st = state(adjustment, m, 10 * m)
            for max_iter in (1000, 0):
                for who, fns in (('device', device), ('reference', reference)):
                    if who == 'reference' and max_iter == 0:
                        continue
                    rs = np.random.RandomState(1)
                    key = '%s m=%d %s max_iter=%d' % (who, m, adjustment, max_iter)
                    res[key] = timed(lambda: fns[adjustment](*st, tau=TAU, w=W, max_iter=max_iter, random_state=rs))
                    show(key, res[key])
    G, m = 64, 32
    for adjustment in ('mean', 'variance'):
        sts = [state(adjustment, m, 500 + g) for g in range(G)]
        y, ll, gam, mean, cov = (np.array([s[i] for s in sts]) for i in range(5))
        draws = np.random.RandomState(2).random_sample((G, 64 * m))
        out = elfi_amd.slice_gamma(y, ll, gam, mean, cov, adjustment, tau=TAU, w=W, draws=draws, return_info=True)
        assert not out[4].any(), out[4]
        key = 'device G=%d m=%d %s one call' % (G, m, adjustment)
        res[key] = timed(lambda: elfi_amd.slice_gamma(y, ll, gam, mean, cov, adjustment, tau=TAU, w=W, draws=draws))
        res[key]['draws'], res[key]['evals'] = int(out[2].sum()), int(out[3].sum())
        show(key + ' (%d draws, %d trials)' % (res[key]['draws'], res[key]['evals']), res[key])

    n = args.chain_iterations
    feats = ['S1', 'S2', 'S4', 'S8']
    for sampler in (None, 'device'):
        bsl = elfi_amd.HipBSL(elfi_amd.toad_model(seed_obs=4), n_sim_round=500, feature_names=feats,
                              likelihood=elfi_amd.robust_likelihood('variance'), gamma_sampler=sampler, seed=1)
        t0 = time.perf_counter()
        bsl.sample(n, sigma_proposals=np.diag([1e-4, 1e-2, 1e-5]), params0=[1.7, 35.0, 0.6], bar=False)
        dt = time.perf_counter() - t0
        key = 'R-BSL-V toad chain, %d iterations, %s sampler' % (n, sampler or 'reference')
        res[key] = dict(seconds=dt, ms_per_iteration=1e3 * dt / n)
        print('%-58s %9.3f s  (%.2f ms per iteration)' % (key, dt, 1e3 * dt / n), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
