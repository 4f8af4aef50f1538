"""Times the toad movement example and the stable-law sampler on one MI355X next to the reference on the same host.

  kernel      elfihip_toad_summaries_dev, device pointers in and out, draws made in the kernel (device timer; 1 warm-up,
              median of 5), the example's shape (66 toads x 63 days, lags 1, 2, 4, 8, 48 summaries), parameters from the
              model's priors, batches of 500 (a BSL round) and 10^5.  "no sort": the same call with thd = inf, which
              counts every displacement as a return and leaves nothing to sort -- the draws, the steps, the chain and the
              compaction pass are all still made, so 1 - no_sort / all is the share of the sort and the quantile reads.
              A digest of the summaries, to compare builds bit for bit.
  host form   elfi_amd.toad_summaries: parameters up, summaries down, synchronised (host wall clock, median of 3)
  sampler     elfihip_stable_dev alone on 10^7 elements, alpha from the prior, in draws per second
  reference   elfi.examples.toad.toad plus its four compute_summaries calls at batch 500, once

    python scripts/time_toad.py [--no-reference] [--json out.json]
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
N_TOADS, N_DAYS = 66, 63
LAGS = np.array([1, 2, 4, 8], dtype=np.int32)
P = np.linspace(0, 1, 11)


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
    return [rs.uniform(1, 2, n), rs.uniform(0, 100, n), rs.uniform(0, 0.9, n)]


def kernel_case(ctx, n):
    import torch
    lib, h = ctx.lib, ctx.handle
    dp = [torch.from_numpy(a).cuda() for a in prior_draws(n, np.random.RandomState(1))]
    S = torch.empty((n, 48), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()

    def call(thd):
        def launch():
            assert lib.elfihip_toad_summaries_dev(h, None, None, None, None, 0, U64(1), U64(0), 0, n, N_TOADS, N_DAYS, len(LAGS),
                                                  LAGS.ctypes.data, len(P), P.ctypes.data, C.c_double(thd),
                                                  *[a.data_ptr() for a in dp], S.data_ptr(), 48, None, 0, None, 0, None, None,
                                                  None, None, 0) == 0
        return launch
    no_sort_ms = median_ms(ctx, call(np.inf))
    all_ms = median_ms(ctx, call(10.))
    ctx.synchronize()
    return dict(batch=n, all_ms=all_ms, no_sort_ms=no_sort_ms, sort_share=1 - no_sort_ms / all_ms, sims_per_s=n / (all_ms * 1e-3),
                steps_per_s=n * (N_DAYS - 1) * N_TOADS / (all_ms * 1e-3), digest=hashlib.sha256(S.cpu().numpy().tobytes()).hexdigest())


def host_form(out):
    import elfi_amd
    for key, n in (('batch_500', 500), ('batch_100000', 100000)):
        params = prior_draws(n, np.random.RandomState(1))
        fn = lambda: elfi_amd.toad_summaries(*params, seed=1)
        fn()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        out[key]['host_form_s'] = float(np.median(times))


def sampler(ctx, out, n=10 ** 7):
    import torch
    lib, h = ctx.lib, ctx.handle
    rs = np.random.RandomState(2)
    alpha, scale = torch.from_numpy(rs.uniform(1, 2, n)).cuda(), torch.from_numpy(rs.uniform(0, 100, n)).cuda()
    x = torch.empty(n, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    ms = median_ms(ctx, lambda: lib.elfihip_stable_dev(h, U64(1), U64(0), n, alpha.data_ptr(), scale.data_ptr(), None, None, x.data_ptr()))
    out['sampler'] = dict(n=n, ms=ms, draws_per_s=n / (ms * 1e-3))


def reference(out):
    from elfi.examples import toad
    params = prior_draws(500, np.random.RandomState(1))
    t0 = time.perf_counter()
    y = toad.toad(*params, batch_size=500, random_state=np.random.RandomState(1))
    t1 = time.perf_counter()
    for lag in LAGS:
        toad.compute_summaries(y, int(lag))
    t2 = time.perf_counter()
    out['reference_500'] = dict(batch=500, toad_s=t1 - t0, summaries_s=t2 - t1, s=t2 - t0)
    out['speedup_500_host_form'] = out['reference_500']['s'] / out['batch_500']['host_form_s']


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
    rec['batch_500'] = kernel_case(ctx, 500)
    rec['batch_100000'] = kernel_case(ctx, 100000)
    host_form(rec)
    sampler(ctx, rec)
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
