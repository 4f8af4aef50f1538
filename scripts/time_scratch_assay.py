"""Times the scratch-assay example on one MI355X, and the reference's simulator on a host.

  kernel      elfihip_assay_summaries_dev, device pointers in and out, draws made in the kernel (device timer; 1 warm-up, median
              of 5), the example's 27 x 36 grid with 100 cells in 10 rows and 288 iterations, batches of 500 (a BSL round) and
              10^4, at the example's truth (0.25, 0.002) and with pm, pp from the model's priors.  "no events": the same call
              with pm = pp = 0, which runs every list build and every draw pass and no event, so 1 - no_events / all is the
              share of the serial walk (over the priors a lower bound: with no proliferation the draw passes stay at 100 slots).
              The events executed, per second.  A digest of the summaries, to compare builds bit for bit.
  slowest     the simulation of the prior batch of 500 with the most events, alone in a batch of 1: the latency the walk sets
  host form   elfi_amd.scratch_assay_summaries: parameters up, summaries down, synchronised (host wall clock, median of 3)
  reference   elfi.examples.scratch_assay's cell_sim + cell_summaries, one simulation at a time as elfi.tools.vectorize runs
              it: at the truth (median of 5) and the mean over the first 8 parameters of the prior batch (host wall clock);
              --reference-only times it alone, on a host without a GPU

    python scripts/time_scratch_assay.py [--no-reference | --reference-only] [--json out.json]
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
N_ITER, OBS_EVERY = 288, 2
TRUTH = (0.25, 0.002)


def grid():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'scratch_assay.npz'))['true_init']


def params(n, prior):
    rs = np.random.RandomState(1)
    return (rs.uniform(0, 1, n), rs.uniform(0, 1, n)) if prior else (np.full(n, TRUTH[0]), np.full(n, TRUTH[1]))


def median_ms(ctx, launch, reps=5):
    launch()
    ctx.synchronize()
    times = []
    for _ in range(reps):
        ctx.timer_start()
        launch()
        times.append(ctx.timer_stop())
    return float(np.median(times)), float(min(times)), float(max(times))


def kernel_case(ctx, pm, pp, with_no_events=True, first=0):
    import torch
    lib, h, init, n = ctx.lib, ctx.handle, grid(), len(pm)
    S = torch.empty((n, N_ITER // OBS_EVERY + 1), dtype=torch.float64, device='cuda')
    ev = torch.empty((n, 2), dtype=torch.int64, device='cuda')

    def call(a, b):
        da, db = torch.from_numpy(np.ascontiguousarray(a)).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda()
        torch.cuda.synchronize()

        def launch():
            assert lib.elfihip_assay_summaries_dev(h, None, None, None, U64(1), U64(0), first, n, *init.shape, N_ITER, OBS_EVERY,
                                                   init.ctypes.data, da.data_ptr(), db.data_ptr(), S.data_ptr(), S.shape[1], None,
                                                   ev.data_ptr(), None) == 0
        return launch, (da, db)
    out = dict(batch=n)
    if with_no_events:
        out['no_events_ms'] = median_ms(ctx, call(np.zeros(n), np.zeros(n))[0])[0]
    launch, keep = call(pm, pp)
    out['all_ms'], out['all_ms_min'], out['all_ms_max'] = median_ms(ctx, launch)
    ctx.synchronize()
    events = ev.cpu().numpy()
    out.update(events=int(events.sum()), most_events=int(events.sum(axis=1).max()), most_events_at=int(events.sum(axis=1).argmax()),
               events_per_s=float(events.sum() / (out['all_ms'] * 1e-3)), sims_per_s=n / (out['all_ms'] * 1e-3),
               digest=hashlib.sha256(S.cpu().numpy().tobytes()).hexdigest())
    if with_no_events:
        out['walk_share'] = 1 - out['no_events_ms'] / out['all_ms']
    return out


def host_form(rec):
    import elfi_amd
    init = grid()
    for prior in (False, True):
        for n in (500, 10000):
            pm, pp = params(n, prior)
            fn = lambda: elfi_amd.scratch_assay_summaries(pm, pp, init, seed=1)      # noqa: E731
            fn()
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                fn()
                times.append(time.perf_counter() - t0)
            rec['%s_batch_%d' % ('prior' if prior else 'truth', n)]['host_form_s'] = float(np.median(times))


def reference(rec):
    from elfi.examples import scratch_assay as sa
    init = grid().astype(np.float64)

    def one(pm, pp, seed):
        t0 = time.perf_counter()
        sa.cell_summaries(sa.cell_sim(pm, pp, init, random_state=np.random.RandomState(seed))[None])
        return time.perf_counter() - t0
    rec['reference_truth'] = dict(s=float(np.median([one(*TRUTH, rep) for rep in range(5)])))
    pm, pp = params(500, True)
    times = [one(pm[i], pp[i], i) for i in range(8)]
    rec['reference_prior'] = dict(simulations=8, mean_s=float(np.mean(times)), max_s=float(np.max(times)))


def main():
    import warnings
    import ref_shim
    with_reference, only_reference = '--no-reference' not in sys.argv, '--reference-only' in sys.argv
    if with_reference:
        if ref_shim.available():
            ref_shim.install()
        else:
            import elfi  # noqa: F401  (an installed ELFI)
    rec = {}
    if not only_reference:
        import elfi_amd
        ctx = elfi_amd.default_context()
        rec['device'] = ctx.device_info()['name']
        for prior in (False, True):
            for n in (500, 10000):
                rec['%s_batch_%d' % ('prior' if prior else 'truth', n)] = kernel_case(ctx, *params(n, prior))
        pm, pp = params(500, True)
        at = rec['prior_batch_500']['most_events_at']
        rec['slowest_of_prior_batch_500'] = kernel_case(ctx, pm[at:at + 1], pp[at:at + 1], False, first=at)
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
