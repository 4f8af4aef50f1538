"""Times the g-and-k example models on one MI355X next to the reference's simulator and summary functions on the same
host, with the M/G/1 kernel (same structure: draws, a per-row sort, quantiles) from the same run for scale.

  kernel      the fused kernel alone, draws made in the kernel, device pointers in and out (device timer; 1 warm-up, median
              of 5): univariate, n_obs 50, octiles + robust statistics at batch 10^6; bivariate, n_obs 150, robust statistics
              at batch 10^5; M/G/1, n_obs 50, 10 quantiles at batch 10^6
  host form   elfi_amd.gnk_summaries / bignk_summaries: parameters up, summaries down, synchronised (host wall clock, median
              of 3)
  reference   elfi.examples.gnk: GNK + ss_octile + ss_robust at batch 10^5; elfi.examples.bignk: BiGNK + ss_robust at batch
              2000 (its simulator is a Python loop over the batch), once each

The reference is the imported ELFI's (through oracle/ref_shim.py where that copy is present); --no-reference skips it.

    python scripts/time_gnk.py [--no-reference] [--json out.json]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

U64 = C.c_uint64


def median_ms(ctx, launch, reps=5):
    launch()
    ctx.synchronize()
    times = []
    for _ in range(reps):
        ctx.timer_start()
        launch()
        times.append(ctx.timer_stop())
    return float(np.median(times))


def wall_s(fn, reps=3):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


def bignk_params(rs, n):
    return np.column_stack([rs.uniform(0, 5, (n, 4)), rs.uniform(-5, 5, (n, 2)), rs.uniform(-.5, 5, (n, 2)),
                            rs.uniform(-1, 1, n)])


def kernels(ctx, out):
    import torch
    from elfi_amd.summaries import GNK_OCTILES, quantile_positions
    lib, h = ctx.lib, ctx.handle
    rs = np.random.RandomState(1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device='cuda')
    obs = np.ones(14)

    def gnk(dim, n, n_obs, P, O, R, D, which):
        lo, hi, t = [np.ascontiguousarray(v) for v in quantile_positions(np.true_divide(GNK_OCTILES, 100), n_obs)]

        def launch():
            assert lib.elfihip_gnk_summaries_dev(h, None, n_obs * dim, U64(1), U64(0), n, n_obs, dim, P.data_ptr(), P.shape[1],
                                                 C.c_double(0.8), lo.ctypes.data, hi.ctypes.data, t.ctypes.data, obs.ctypes.data,
                                                 which, None, 0, None, 0, None, 0, O.data_ptr() if O is not None else None,
                                                 7 * dim, R.data_ptr(), 4 * dim, D.data_ptr()) == 0
        return median_ms(ctx, launch)
    n = 10 ** 6
    ms = gnk(1, n, 50, dev(rs.uniform(0, 10, (n, 4))), empty(n, 7), empty(n, 4), empty(n), 3)
    out['gnk_batch'], out['gnk_kernel_ms'], out['gnk_sims_per_s'] = n, ms, n / (ms * 1e-3)
    out['gnk_elements_per_s'] = n * 50 / (ms * 1e-3)
    n = 10 ** 5
    ms = gnk(2, n, 150, dev(bignk_params(rs, n)), None, empty(n, 8), empty(n), 3)
    out['bignk_batch'], out['bignk_kernel_ms'], out['bignk_sims_per_s'] = n, ms, n / (ms * 1e-3)
    out['bignk_elements_per_s'] = n * 300 / (ms * 1e-3)
    # M/G/1, 50 observations, 10 quantiles, batch 10^6: the same structure (draws, a per-row sort, quantiles)
    n = 10 ** 6
    m1 = rs.uniform(0, 10, n)
    a, b, c = dev(m1), dev(m1 + rs.uniform(0, 10, n)), dev(rs.uniform(0.01, 0.5, n))
    q = np.linspace(0, 1, 10)
    lo, hi, t = [np.ascontiguousarray(v) for v in quantile_positions(q, 50)]
    logy, Q, d, qobs = empty(n, 50), empty(n, 10), empty(n), np.ones(10)

    def mg1():
        assert lib.elfihip_mg1_summaries_dev(h, None, 50, None, 50, U64(1), U64(0), n, 50, a.data_ptr(), b.data_ptr(),
                                             c.data_ptr(), 10, lo.ctypes.data, hi.ctypes.data, t.ctypes.data, qobs.ctypes.data,
                                             None, logy.data_ptr(), 50, Q.data_ptr(), 10, None, 50, None, 50, None, 50,
                                             d.data_ptr()) == 0
    ms = median_ms(ctx, mg1)
    out['mg1_batch'], out['mg1_kernel_ms'], out['mg1_sims_per_s'] = n, ms, n / (ms * 1e-3)


def host_forms(out):
    import elfi_amd
    rs = np.random.RandomState(2)
    n = 10 ** 6
    P = rs.uniform(0, 10, (n, 4))
    s = wall_s(lambda: elfi_amd.gnk_summaries(*P.T, seed=1, summary=('octile', 'robust')))
    out['gnk_host_form_s'], out['gnk_host_form_sims_per_s'] = s, n / s
    n = 10 ** 5
    P = bignk_params(rs, n)
    s = wall_s(lambda: elfi_amd.bignk_summaries(*P.T, seed=1, summary='robust'))
    out['bignk_host_form_s'], out['bignk_host_form_sims_per_s'] = s, n / s


def reference(out):
    from elfi.examples import bignk, gnk
    rs = np.random.RandomState(3)
    n = 10 ** 5
    P = rs.uniform(0, 10, (n, 4))
    t0 = time.perf_counter()
    y = gnk.GNK(*P.T, n_obs=50, batch_size=n, random_state=rs)
    out['gnk_reference_simulator_s'] = time.perf_counter() - t0
    gnk.ss_octile(y)
    gnk.ss_robust(y)
    s = time.perf_counter() - t0
    out['gnk_reference_batch'], out['gnk_reference_s'], out['gnk_reference_sims_per_s'] = n, s, n / s
    n = 2000
    P = bignk_params(rs, n)
    t0 = time.perf_counter()
    y = bignk.BiGNK(*P.T, n_obs=150, batch_size=n, random_state=rs)
    out['bignk_reference_simulator_s'] = time.perf_counter() - t0
    gnk.ss_robust(y)
    s = time.perf_counter() - t0
    out['bignk_reference_batch'], out['bignk_reference_s'], out['bignk_reference_sims_per_s'] = n, s, n / s


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
    host_forms(rec)
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
