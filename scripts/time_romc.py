"""Times ROMC on one MI355X next to the reference's host loop on the same box.

  device      elfi_amd.HipROMC on elfi_amd.ma2_model(n_obs=100, seed_obs=4), n1 = 500: solve_problems, estimate_regions
              (eps_filter = the 0.75 quantile of the minima, eps_region 0.02, eps_cutoff 0.1, fit_models=False), sample(n2 = 100)
              and eval_posterior on the 30 x 30 grid over the bounds (its first call also integrates the partition on a
              30 x 30 grid of its own: two density calls).  One warm-up run at n1 = 16, then REPS timed runs; the medians are
              printed per step and as a total, and per problem.
  reference   elfi.ROMC on elfi.examples.ma2.get_model(n_obs=100, seed_obs=4) (oracle/ref_shim.py; skipped when it is not
              installed), at n1 = N1_REF problems, per problem: scipy.optimize.minimize(method='Nelder-Mead') on the
              reference's frozen-seed objective, RegionConstructor.build with the same thresholds, n2 = 100 weighted samples of
              the box and the problem's share of a 30 x 30 density grid (900 evaluations of its indicator).  The reference's
              Hessian step needs numdifftools, which is not installed here: the device's Hessian is handed to the region
              constructor and the step is left out of the reference's time.

    python scripts/time_romc.py [--json out.json] [--n1 500] [--n1-ref 3]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle')):
    sys.path.insert(0, p)

BOUNDS = [(-2, 2), (-1.25, 1.25)]
REPS = 5


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def grid(n=30):
    return np.array([[a, b] for a in np.linspace(*BOUNDS[0], n) for b in np.linspace(*BOUNDS[1], n)])


def device_run(elfi_amd, n1, seed=21):
    steps = {}
    m = elfi_amd.ma2_model(n_obs=100, seed_obs=4)
    romc = elfi_amd.HipROMC(m, bounds=BOUNDS, discrepancy_name='d')
    t = time.perf_counter()
    romc.solve_problems(n1=n1, seed=seed)
    steps['solve_problems'] = time.perf_counter() - t
    t = time.perf_counter()
    romc.estimate_regions(eps_filter=romc.compute_eps(0.75), fit_models=False, eps_region=0.02, eps_cutoff=0.1)
    steps['estimate_regions'] = time.perf_counter() - t
    t = time.perf_counter()
    romc.sample(n2=100)
    steps['sample'] = time.perf_counter() - t
    t = time.perf_counter()
    dens = romc.eval_posterior(grid())
    steps['eval_posterior'] = time.perf_counter() - t
    info = dict(solved=int(np.sum(romc.inference_state['solved'])), accepted=int(np.sum(romc.inference_state['accepted'])),
                nfev=int(romc.solve_info['nfev'].sum()), density_sum=float(np.sum(dens)))
    romc.problems.free()
    return steps, info


def reference_run(elfi, elfi_amd, n1, device_hess):
    import scipy.optimize as optim
    from elfi.examples import ma2
    from elfi.methods.inference import romc as ref
    m = ma2.get_model(n_obs=100, seed_obs=4)
    romc = elfi.ROMC(m, bounds=BOUNDS, discrepancy_name='d')
    romc._define_objectives(n1=n1, seed=21)
    x0 = romc.model_prior.rvs(size=n1, random_state=21)
    pts = grid()
    steps = dict(solve_problems=0.0, estimate_regions=0.0, sample=0.0, eval_posterior=0.0)
    for i, p in enumerate(romc.optim_problems):
        t = time.perf_counter()
        res = optim.minimize(p.objective, x0[i], method='Nelder-Mead')
        steps['solve_problems'] += time.perf_counter() - t
        result = ref.RomcOptimisationResult(res.x, res.fun, device_hess)
        t = time.perf_counter()
        box = ref.RegionConstructor(result, p.objective, 2, eps_region=0.02, K=10, eta=1., rep_lim=300).build()[0]
        steps['estimate_regions'] += time.perf_counter() - t
        t = time.perf_counter()
        th = box.sample(100)
        for row in th:
            romc.model_prior.pdf(row[None, :]), p.objective(row), box.pdf(row)
        steps['sample'] += time.perf_counter() - t
        t = time.perf_counter()
        for row in pts:
            p.objective(row)
        steps['eval_posterior'] += time.perf_counter() - t
    return steps


def main():
    import elfi_amd
    import ref_shim
    elfi = ref_shim.install() if ref_shim.available() else None
    if elfi is None:
        raise SystemExit('HipROMC subclasses the imported ELFI: no ELFI package found (oracle/make_ref.sh)')
    import elfi.clients.native as native
    native.set_as_default()
    n1, n1_ref = _arg('--n1', 500), _arg('--n1-ref', 3)
    device_run(elfi_amd, 16)
    runs = [device_run(elfi_amd, n1) for _ in range(REPS)]
    med = {k: float(np.median([r[0][k] for r in runs])) for k in runs[0][0]}
    totals = [sum(r[0].values()) for r in runs]
    total = float(np.median(totals))
    out = dict(device=dict(n1=n1, reps=REPS, seconds=med, total_seconds=total, total_min=float(min(totals)), total_max=float(max(totals)),
                           ms_per_problem=1e3 * total / n1, **runs[0][1]))
    print('device', json.dumps(out['device']), flush=True)
    steps = reference_run(elfi, elfi_amd, n1_ref, np.array([[2.0, 0.5], [0.5, 1.0]]))
    tot = sum(steps.values())
    out['reference'] = dict(n1=n1_ref, seconds=steps, total_seconds=tot, ms_per_problem=1e3 * tot / n1_ref)
    out['ratio_per_problem'] = out['reference']['ms_per_problem'] / out['device']['ms_per_problem']
    print('reference', json.dumps(out['reference']), flush=True)
    print('per problem: reference / device = %.0f' % out['ratio_per_problem'], flush=True)
    if '--json' in sys.argv:
        with open(sys.argv[sys.argv.index('--json') + 1], 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
