"""Times the day-care-centre transmission example on one MI355X next to the reference's simulator on the same host.

  kernels     device pointers in and out, draws made in the kernel (device timer; 1 warm-up, median of 5), the example's
              shape (29 centres x 53 individuals x 33 strains, 36 observed, time_end 10), max_events 2^16 per centre.  The
              example's true parameters (3.6, 0.6, 0.1) and parameters from the model's priors, each at batch 1 (BOLFI's
              case: 29 wavefronts, nothing to hide an event's latency behind) and at batch 256 (7424 wavefronts).  At batch 1
              the priors' row is the median over 8 draws, one call each.  "simulation": the call without summaries and
              distance (dc_sim_kernel alone); "all": simulation + summaries + distance.  Events per second from the event
              counts the simulation returns.  A digest of every output, to compare builds bit for bit.
  host form   elfi_amd.daycare_summaries with the distance: parameters up, summaries down, synchronised (host wall clock,
              median of 3)
  reference   elfi.examples.daycare.daycare at the true parameters and at the first of the priors' draws, batch 1, once each
              (its lock-step loop recomputes all 1749 hazards of all 29 centres per event of the slowest one)

    python scripts/time_daycare.py [--no-reference] [--json out.json]
"""
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

U64 = C.c_uint64
N_DCC, N_IND, N_STRAINS, N_OBS, TIME_END, MAX_EVENTS = 29, 53, 33, 36, 10., 1 << 16
TRUE = (3.6, 0.6, 0.1)


def median_ms(ctx, launch, reps=5):
    launch()
    ctx.synchronize()
    times = []
    for _ in range(reps):
        ctx.timer_start()
        launch()
        times.append(ctx.timer_stop())
    return float(np.median(times))


def prior_draws(n, rs):
    return [rs.uniform(0, 11, n), rs.uniform(0, 2, n), rs.uniform(0, 1, n)]


def true_parameters(n):
    return [np.full(n, v) for v in TRUE]


def observed():
    rs = np.random.RandomState(2)
    return np.stack([rs.uniform(0, 2, N_DCC), rs.randint(0, 11, N_DCC).astype(float), rs.uniform(0, 1, N_DCC), rs.uniform(0, 1, N_DCC)])


def kernel_case(ctx, params):
    import torch
    lib, h = ctx.lib, ctx.handle
    n = params[0].shape[0]
    pairs = n * N_DCC
    dp = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in params]
    S = torch.empty((n, 4 * N_DCC), dtype=torch.float64, device='cuda')
    M = torch.empty((pairs, N_OBS), dtype=torch.int64, device='cuda')
    D = torch.empty(n, dtype=torch.float64, device='cuda')
    T = torch.empty(pairs, dtype=torch.float64, device='cuda')
    st = torch.empty(pairs, dtype=torch.int32, device='cuda')
    ev = torch.empty(pairs, dtype=torch.int64, device='cuda')
    obs = observed()
    torch.cuda.synchronize()

    def call(summaries):
        def launch():
            assert lib.elfihip_daycare_summaries_dev(
                h, None, 0, None, 0, U64(1), U64(0), 0, n, N_DCC, N_IND, N_STRAINS, N_OBS, C.c_double(TIME_END), MAX_EVENTS,
                *[a.data_ptr() for a in dp], None, obs.ctypes.data, M.data_ptr(), N_OBS, T.data_ptr(), st.data_ptr(),
                ev.data_ptr(), S.data_ptr() if summaries else None, 4 * N_DCC, D.data_ptr() if summaries else None) == 0
        return launch
    sim_ms, all_ms = median_ms(ctx, call(False)), median_ms(ctx, call(True))
    ctx.synchronize()
    events, status = ev.cpu().numpy(), st.cpu().numpy()
    digest = hashlib.sha256()
    for a in (S, M, D, T, st, ev):
        digest.update(a.cpu().numpy().tobytes())
    return dict(batch=n, simulation_ms=sim_ms, all_ms=all_ms, events=int(events.sum()), events_per_s=float(events.sum() / (sim_ms * 1e-3)),
                sims_per_s=n / (all_ms * 1e-3), events_per_centre_median=float(np.median(events)), events_per_centre_max=int(events.max()),
                status_counts=np.bincount(status, minlength=3).tolist(), digest=digest.hexdigest())


def kernels(ctx, out):
    out['true_1'] = kernel_case(ctx, true_parameters(1))
    out['true_256'] = kernel_case(ctx, true_parameters(256))
    prior = prior_draws(256, np.random.RandomState(1))
    singles = [kernel_case(ctx, [a[i:i + 1] for a in prior]) for i in range(8)]
    out['prior_1'] = dict(batch=1, draws=8, simulation_ms=float(np.median([s['simulation_ms'] for s in singles])),
                          all_ms=float(np.median([s['all_ms'] for s in singles])),
                          all_ms_max=float(np.max([s['all_ms'] for s in singles])),
                          events_per_s=float(np.median([s['events_per_s'] for s in singles])),
                          sims_per_s=float(np.median([s['sims_per_s'] for s in singles])),
                          events_per_centre_max=int(np.max([s['events_per_centre_max'] for s in singles])))
    out['prior_256'] = kernel_case(ctx, prior)


def host_form(out):
    import elfi_amd
    obs = observed()
    for key, params in (('true_1', true_parameters(1)), ('true_256', true_parameters(256))):
        fn = lambda: elfi_amd.daycare_summaries(*params, seed=1, observed=obs)
        fn()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        out[key]['host_form_s'] = float(np.median(times))


def reference(out):
    from elfi.examples import daycare as dc
    first = [float(a[0]) for a in prior_draws(256, np.random.RandomState(1))]
    for key, params in (('reference_true', TRUE), ('reference_prior_first', first)):
        t0 = time.perf_counter()
        dc.daycare(*params, batch_size=1, random_state=np.random.RandomState(1))
        out[key] = dict(batch=1, parameters=list(params), s=time.perf_counter() - t0)
    out['batch_1_true_beats_the_reference'] = bool(out['true_1']['host_form_s'] < out['reference_true']['s'])


def main():
    import warnings
    import ref_shim
    with_reference = '--no-reference' not in sys.argv
    if with_reference:
        if ref_shim.available():
            ref_shim.install()
        else:
            import elfi  # noqa: F401  (an installed ELFI)
    import elfi_amd
    ctx = elfi_amd.default_context()
    rec = {'device': ctx.device_info()['name']}
    kernels(ctx, rec)
    host_form(rec)
    if with_reference:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            reference(rec)
    print(json.dumps(rec, indent=1), flush=True)
    if '--json' in sys.argv:
        path = sys.argv[sys.argv.index('--json') + 1]
        with open(path, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
