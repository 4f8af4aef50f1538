"""Times the alpha-stable stochastic-volatility example and the general stable-law sampler on one MI355X, and the reference's
simulator on a host.

  kernel      elfihip_sv_summaries_dev, device pointers in and out, draws made in the kernel (device timer; 1 warm-up, median
              of 5), alpha and beta from the model's priors and the example's constants, n_obs 50 and 1000, batches of 500 (a
              BSL round) and 10^5.  "no sort": the same call with mu = +inf, which makes the log-volatilities and so the
              returns NaN from the second observation on -- the draws, the shocks, the chain and the exponentials are all
              still made, but a NaN row is not sorted, so 1 - no_sort / all is the share of the sort and the quantile reads.
              A digest of the summaries, to compare builds bit for bit.
  host form   elfi_amd.sv_summaries: parameters up, summaries and series down, synchronised (host wall clock, median of 3)
  sampler     elfihip_stable_general_dev alone on 10^7 elements in S0, alpha and beta from the priors, in draws per second
  reference   elfi.examples.stochastic_volatility_model's simulator plus kurt and skew at batch 500, n_obs 50 and 1000
              (host wall clock, median of 5); --reference-only times it alone, on a host without a GPU

    python scripts/time_sv.py [--no-reference | --reference-only] [--json out.json]
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
Q = np.array([.05, .25, .75, .95, .05, .5, .95])
FIXED = dict(kappa=1., eta=0., mu=0., phi=0.95, sigma=0.2)
SIZES = (50, 1000)


def median_ms(ctx, launch, reps=5):
    launch()
    ctx.synchronize()
    times = []
    for _ in range(reps):
        ctx.timer_start()
        launch()
        times.append(ctx.timer_stop())
    return float(np.median(times)), float(min(times)), float(max(times))


def params(n, rs, mu=0.):
    fixed = dict(FIXED, mu=mu)
    return [rs.uniform(0.5, 2, n), rs.uniform(-1, 1, n)] + [np.full(n, fixed[k]) for k in ('kappa', 'eta', 'mu', 'phi', 'sigma')]


def kernel_case(ctx, n, n_obs):
    import torch
    lib, h = ctx.lib, ctx.handle
    S = torch.empty((n, 2), dtype=torch.float64, device='cuda')

    def call(mu):
        dp = [torch.from_numpy(a).cuda() for a in params(n, np.random.RandomState(1), mu)]
        torch.cuda.synchronize()

        def launch():
            assert lib.elfihip_sv_summaries_dev(h, None, None, None, 0, U64(1), U64(0), 0, n, n_obs, Q.ctypes.data,
                                                *[a.data_ptr() for a in dp], None, S.data_ptr(), 2, None, 0, None, 0, None, 0,
                                                None, None, None, 0) == 0
        return launch
    no_sort_ms = median_ms(ctx, call(np.inf))[0]
    all_ms, lo, hi = median_ms(ctx, call(0.))
    ctx.synchronize()
    return dict(batch=n, n_obs=n_obs, all_ms=all_ms, all_ms_min=lo, all_ms_max=hi, no_sort_ms=no_sort_ms, sort_share=1 - no_sort_ms / all_ms,
                sims_per_s=n / (all_ms * 1e-3), cells_per_s=n * n_obs / (all_ms * 1e-3),
                digest=hashlib.sha256(S.cpu().numpy().tobytes()).hexdigest())


def host_form(rec):
    import elfi_amd
    for n_obs in SIZES:
        for n in (500, 100000):
            p = params(n, np.random.RandomState(1))
            fn = lambda: elfi_amd.sv_summaries(*p, n_obs=n_obs, seed=1)      # noqa: E731
            fn()
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                fn()
                times.append(time.perf_counter() - t0)
            rec['n_obs_%d_batch_%d' % (n_obs, n)]['host_form_s'] = float(np.median(times))


def sampler(ctx, rec, n=10 ** 7):
    import torch
    lib, h = ctx.lib, ctx.handle
    rs = np.random.RandomState(2)
    d = [torch.from_numpy(a).cuda() for a in (rs.uniform(0.5, 2, n), rs.uniform(-1, 1, n), np.zeros(n), np.ones(n))]
    x = torch.empty(n, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    ms, lo, hi = median_ms(ctx, lambda: lib.elfihip_stable_general_dev(h, U64(1), U64(0), n, 1, *[a.data_ptr() for a in d], None, None,
                                                               x.data_ptr()))
    rec['sampler'] = dict(n=n, ms=ms, ms_min=lo, ms_max=hi, draws_per_s=n / (ms * 1e-3))


def reference(rec):
    from elfi.examples import stochastic_volatility_model as svm
    for n_obs in SIZES:
        p = params(500, np.random.RandomState(1))
        times = []
        for rep in range(5):
            t0 = time.perf_counter()
            y = svm.alpha_stochastic_volatility_model(*p, n_obs=n_obs, batch_size=500, random_state=np.random.RandomState(rep))
            t1 = time.perf_counter()
            svm.kurt(y), svm.skew(y)
            times.append((t1 - t0, time.perf_counter() - t1))
        sim, summ = np.median(np.array(times), axis=0)
        rec['reference_n_obs_%d_batch_500' % n_obs] = dict(batch=500, n_obs=n_obs, simulator_s=float(sim), summaries_s=float(summ),
                                                           s=float(sim + summ))


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
        for n_obs in SIZES:
            for n in (500, 100000):
                rec['n_obs_%d_batch_%d' % (n_obs, n)] = kernel_case(ctx, n, n_obs)
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
