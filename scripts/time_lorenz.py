"""Times the stochastic Lorenz-96 example model (160 rows x 40 variables) on one MI355X next to the reference's simulator
and summary functions on the same host.

  kernel      the fused kernel alone at batch 10^4 and 10^5, draws made in the kernel, device pointers in and out, no series
              output (device timer; 1 warm-up, median of 5): simulations and normals per second
  host form   elfi_amd.lorenz_summaries: parameters up, summaries down, synchronised (host wall clock, median of 3)
  reference   elfi.examples.lorenz: forecast_lorenz + the six summary functions at batch 10^3 (once), scaled to the batch

The reference is the imported ELFI's (through oracle/ref_shim.py where that copy is present); --no-reference skips it.
The condition checked is that the device host form at batch 10^4 beats the reference chain scaled to that batch.

    python scripts/time_lorenz.py [--no-reference] [--json out.json]
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

U64, DBL = C.c_uint64, C.c_double
T, K, REF_BATCH = 160, 40, 1000


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


def initial_state():
    return 3.0 * np.random.RandomState(0).randn(K)


def kernel(ctx, n, out):
    import torch
    lib, h = ctx.lib, ctx.handle
    rs = np.random.RandomState(1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t1, t2, y0 = dev(rs.uniform(0.5, 3.5, n)), dev(rs.uniform(0, 0.3, n)), dev(initial_state())
    S = torch.empty((n, 6), dtype=torch.float64, device='cuda')
    d = torch.empty(n, dtype=torch.float64, device='cuda')
    obs = np.zeros(6)
    c, step = float(np.sqrt(1 - pow(0.984, 2))), 4 / T
    torch.cuda.synchronize()

    def launch():
        assert lib.elfihip_lorenz_summaries_dev(h, None, (T - 1) * K, U64(1), U64(0), n, K, T, t1.data_ptr(), t2.data_ptr(),
                                                DBL(10.0), DBL(c), DBL(0.984), DBL(step), y0.data_ptr(), 0, obs.ctypes.data,
                                                S.data_ptr(), 6, None, T * K, d.data_ptr()) == 0
    ms = median_ms(ctx, launch)
    out['kernel_ms'], out['sims_per_s'], out['normals_per_s'] = ms, n / (ms * 1e-3), n * (T - 1) * K / (ms * 1e-3)


def host_form(n, out):
    import elfi_amd
    rs = np.random.RandomState(2)
    t1, t2, y0 = rs.uniform(0.5, 3.5, n), rs.uniform(0, 0.3, n), initial_state()
    out['host_form_s'] = wall_s(lambda: elfi_amd.lorenz_summaries(t1, t2, y0, seed=1))
    out['host_form_sims_per_s'] = n / out['host_form_s']


def reference(out):
    from elfi.examples import lorenz
    rs = np.random.RandomState(3)
    t1, t2 = rs.uniform(0.5, 3.5, REF_BATCH), rs.uniform(0, 0.3, REF_BATCH)
    t0 = time.perf_counter()
    y = lorenz.forecast_lorenz(t1, t2, batch_size=REF_BATCH, random_state=rs)
    out['reference_simulator_s'] = time.perf_counter() - t0
    [lorenz.mean(y), lorenz.var(y), lorenz.autocov(y), lorenz.cov(y), lorenz.xcov(y, True), lorenz.xcov(y, False)]
    out['reference_s'] = time.perf_counter() - t0
    out['reference_batch'], out['reference_sims_per_s'] = REF_BATCH, REF_BATCH / out['reference_s']


def main():
    import ref_shim
    with_reference = '--no-reference' not in sys.argv
    if with_reference:
        if ref_shim.available():
            ref_shim.install()
        else:
            import elfi  # noqa: F401  (an installed ELFI)
    import elfi_amd
    ctx = elfi_amd.default_context()
    result = {'device': ctx.device_info()['name']}
    if with_reference:
        rec = {}
        reference(rec)
        result['reference'] = rec
        print('reference', json.dumps(rec), flush=True)
    for n in (10 ** 4, 10 ** 5):
        rec = {}
        kernel(ctx, n, rec)
        host_form(n, rec)
        if with_reference:
            rec['reference_scaled_s'] = result['reference']['reference_s'] * n / REF_BATCH
            rec['host_form_speedup'] = rec['reference_scaled_s'] / rec['host_form_s']
            assert n != 10 ** 4 or rec['host_form_s'] < rec['reference_scaled_s'], 'Lorenz: the device form is not faster'
        result['batch_%d' % n] = rec
        print('batch', n, json.dumps(rec), flush=True)
    if '--json' in sys.argv:
        path = sys.argv[sys.argv.index('--json') + 1]
        with open(path, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
