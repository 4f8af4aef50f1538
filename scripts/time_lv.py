"""Times the stochastic Lotka-Volterra example on one MI355X next to the reference's simulator on the same host, with the
ARCH(1) kernel from the same run as the control (a kernel this work does not touch: two runs whose ARCH times differ were
not taken under the same conditions).

  kernels     device pointers in and out, draws made in the kernel (device timer; 1 warm-up, median of 5), n_obs 50, time_end
              30.  Parameters from the model's priors: batch 10^5 at max_events 2^20 (the default) and at 2^15 (under the
              priors the slowest simulations are the ones cut off, so the bound sets the tail); batch 10^6 at 2^15 (more
              simulations than the device holds lanes); batch 10^5 cut after ONE event (the launches, the refill and
              the summary kernel with next to no simulation).  The example's true parameters: batch 10^4.
              "simulation": the call without summaries and distance (lv_sim_kernel alone); "all": simulation +
              lv_summary_kernel; the summary kernel is the difference (read it off the one-event run: elsewhere it is
              below the spread of the simulation).  Events per second from the event counts the simulation returns.  A
              digest of every output, to compare builds bit for bit.
  host form   elfi_amd.lotka_volterra_summaries: parameters up, summaries down, synchronised (host wall clock, median of 3)
  reference   elfi.examples.lotka_volterra.lotka_volterra at the true parameters, batch 8, once (its lock-step loop runs
              until the slowest simulation of the batch is done and cannot finish a batch from the priors)

    python scripts/time_lv.py [--no-reference] [--json out.json]
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
N_OBS, TIME_END = 50, 30.
OBS = np.array([170., 180., 8.9, 9.8, 0.8, 0.85, 0.55, 0.6, 0.1])


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
    return [np.exp(rs.uniform(-6, 2, n)) for _ in range(3)] + [rs.normal(50, np.sqrt(50), n), rs.normal(100, 10, n)]


def true_parameters(n):
    return [np.full(n, v) for v in (1.0, 0.005, 0.6, 50., 100.)]


def kernels(ctx, out):
    import torch
    lib, h = ctx.lib, ctx.handle
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for key, params, max_events in (('prior_1e5', prior_draws(10 ** 5, np.random.RandomState(1)), 1 << 20),
                                    ('prior_1e5_max_2_15', prior_draws(10 ** 5, np.random.RandomState(1)), 1 << 15),
                                    ('prior_1e6_max_2_15', prior_draws(10 ** 6, np.random.RandomState(1)), 1 << 15),
                                    ('prior_1e5_one_event', prior_draws(10 ** 5, np.random.RandomState(1)), 1),
                                    ('true_1e4', true_parameters(10 ** 4), 1 << 20)):
        n = params[0].shape[0]
        dp = [dev(a) for a in params]
        S = torch.empty((n, 9), dtype=torch.float64, device='cuda')
        Y = torch.empty((n, N_OBS, 2), dtype=torch.float64, device='cuda')
        D, T = [torch.empty(n, dtype=torch.float64, device='cuda') for _ in range(2)]
        st = torch.empty(n, dtype=torch.int32, device='cuda')
        ev = torch.empty(n, dtype=torch.int64, device='cuda')
        torch.cuda.synchronize()

        def call(summaries):
            def launch():
                assert lib.elfihip_lv_summaries_dev(
                    h, None, 0, None, 0, None, 0, U64(1), U64(0), 0, n, N_OBS, C.c_double(TIME_END), max_events,
                    *[a.data_ptr() for a in dp], None, OBS.ctypes.data, Y.data_ptr(), 2 * N_OBS, T.data_ptr(), st.data_ptr(),
                    ev.data_ptr(), S.data_ptr() if summaries else None, 9, D.data_ptr() if summaries else None) == 0
            return launch
        sim_ms, all_ms = median_ms(ctx, call(False)), median_ms(ctx, call(True))
        ctx.synchronize()
        events = ev.cpu().numpy()
        status = st.cpu().numpy()
        digest = hashlib.sha256()
        for a in (S, Y, D, T, st, ev):
            digest.update(a.cpu().numpy().tobytes())
        out[key] = dict(batch=n, max_events=max_events, simulation_ms=sim_ms, all_ms=all_ms, summary_ms=all_ms - sim_ms,
                        events=int(events.sum()), events_per_s=float(events.sum() / (sim_ms * 1e-3)),
                        sims_per_s=n / (all_ms * 1e-3), events_median=float(np.median(events)), events_max=int(events.max()),
                        status_counts=np.bincount(status, minlength=4).tolist(), digest=digest.hexdigest())
    n = 10 ** 6
    rs = np.random.RandomState(1)
    a1, a2 = dev(rs.uniform(-1, 1, n)), dev(rs.uniform(0, 1, n))
    Sa, Da, aobs = torch.empty((n, 17), dtype=torch.float64, device='cuda'), torch.empty(n, dtype=torch.float64, device='cuda'), np.ones(17)

    def arch():
        assert lib.elfihip_arch_summaries_dev(h, None, 52, U64(1), U64(0), n, 50, 5, a1.data_ptr(), a2.data_ptr(),
                                              aobs.ctypes.data, Sa.data_ptr(), 17, None, 50, Da.data_ptr()) == 0
    out['arch_control_ms'] = median_ms(ctx, arch)


def host_form(out):
    import elfi_amd
    for key, params in (('prior_1e5', prior_draws(10 ** 5, np.random.RandomState(1))), ('true_1e4', true_parameters(10 ** 4))):
        fn = lambda: elfi_amd.lotka_volterra_summaries(*params, n_obs=N_OBS, time_end=TIME_END, seed=1, observed=OBS)
        fn()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        out[key]['host_form_s'] = float(np.median(times))


def reference(out):
    from elfi.examples import lotka_volterra as lv
    n = 8
    t0 = time.perf_counter()
    _, _, _, times = lv.lotka_volterra(1.0, 0.005, 0.6, 50, 100, n_obs=N_OBS, time_end=TIME_END, batch_size=n,
                                       random_state=np.random.RandomState(1), return_full=True)
    s = time.perf_counter() - t0
    events = int(np.argmax(times >= TIME_END, axis=1).sum())
    out['reference_true'] = dict(batch=n, s=s, lock_step_iterations=times.shape[1] - 1, events=events, events_per_s=events / s,
                                 sims_per_s=n / s)


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
