"""Times the two time-series example models (ARCH(1), M/G/1) on one MI355X next to the reference's simulator and summary
functions on the same host, at batch 10^5 and 10^6.

  kernel      the fused kernel alone, draws made in the kernel, device pointers in and out (device timer; 1 warm-up, median
              of 5); for ARCH also the normals per second, next to the MA2 draw form's from the same run
  host form   elfi_amd.arch_summaries / mg1_summaries: parameters up, summaries down, synchronised (host wall clock, median of 3)
  reference   elfi.examples.arch: arch + the 17 summary functions; elfi.examples.mg1: MG1 + log_identity + quantiles (once)
  rejection   HipRejection(model['d'], batch_size=10**6).sample(1000, n_sim=10**7) on the fused models (once)

The reference is the imported ELFI's (through oracle/ref_shim.py where that copy is present); --no-reference skips it
and the rejection runs, which need its graph.

    python scripts/time_series_models.py [--no-reference] [--json out.json]
"""
import ctypes as C
import json
import os
import sys
import time
from itertools import combinations

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


def kernels(ctx, n, out):
    import torch
    from elfi_amd.summaries import quantile_positions
    lib, h = ctx.lib, ctx.handle
    rs = np.random.RandomState(1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device='cuda')
    # MA2, 100 observations: 102 normals per simulation
    t1, t2 = dev(rs.uniform(-1, 1, n)), dev(rs.uniform(0, 1, n))
    s1, s2, d = empty(n), empty(n), empty(n)
    torch.cuda.synchronize()

    def ma2():
        assert lib.elfihip_ma2_draw_distance_dev(h, U64(1), U64(0), n, 100, t1.data_ptr(), t2.data_ptr(), C.c_double(0.3),
                                                 C.c_double(0.1), s1.data_ptr(), s2.data_ptr(), d.data_ptr()) == 0
    ms = median_ms(ctx, ma2)
    out['ma2_kernel_ms'], out['ma2_normals_per_s'] = ms, n * 102 / (ms * 1e-3)
    # ARCH, 100 observations, 5 lags: 102 normals per simulation, 17 summaries and the distance
    S, obs = empty(n, 17), np.zeros(17)

    def arch():
        assert lib.elfihip_arch_summaries_dev(h, None, 102, U64(1), U64(0), n, 100, 5, t1.data_ptr(), t2.data_ptr(),
                                              obs.ctypes.data, S.data_ptr(), 17, None, 100, d.data_ptr()) == 0
    ms = median_ms(ctx, arch)
    out['arch_kernel_ms'], out['arch_normals_per_s'], out['arch_sims_per_s'] = ms, n * 102 / (ms * 1e-3), n / (ms * 1e-3)
    # M/G/1, 50 observations, 10 quantiles
    m1 = rs.uniform(0, 10, n)
    a, b, c = dev(m1), dev(m1 + rs.uniform(0, 10, n)), dev(rs.uniform(0.01, 0.5, n))
    q = np.linspace(0, 1, 10)
    lo, hi, t = [np.ascontiguousarray(v) for v in quantile_positions(q, 50)]
    w = (1 / 100) ** q
    logy, Q, qobs = empty(n, 50), empty(n, 10), np.ones(10)

    def mg1():
        assert lib.elfihip_mg1_summaries_dev(h, None, 50, None, 50, U64(1), U64(0), n, 50, a.data_ptr(), b.data_ptr(),
                                             c.data_ptr(), 10, lo.ctypes.data, hi.ctypes.data, t.ctypes.data, qobs.ctypes.data,
                                             w.ctypes.data, logy.data_ptr(), 50, Q.data_ptr(), 10, None, 50, None, 50, None, 50,
                                             d.data_ptr()) == 0
    ms = median_ms(ctx, mg1)
    out['mg1_kernel_ms'], out['mg1_sims_per_s'] = ms, n / (ms * 1e-3)


def host_forms(n, out):
    import elfi_amd
    rs = np.random.RandomState(2)
    t1, t2 = rs.uniform(-1, 1, n), rs.uniform(0, 1, n)
    out['arch_host_form_s'] = wall_s(lambda: elfi_amd.arch_summaries(t1, t2, seed=1))
    m1 = rs.uniform(0, 10, n)
    m2, m3 = m1 + rs.uniform(0, 10, n), rs.uniform(0.01, 0.5, n)
    out['mg1_host_form_s'] = wall_s(lambda: elfi_amd.mg1_summaries(m1, m2, m3, seed=1))


def reference(n, out):
    from elfi.examples import arch, mg1
    rs = np.random.RandomState(3)
    t1, t2 = rs.uniform(-1, 1, n), rs.uniform(0, 1, n)
    lags = range(1, 6)
    t0 = time.perf_counter()
    y = arch.arch(t1, t2, n_obs=100, batch_size=n, random_state=rs)
    out['arch_reference_simulator_s'] = time.perf_counter() - t0
    [arch.sample_mean(y), arch.sample_variance(y)] + [arch.autocorr(y, i) for i in lags] + \
        [arch.pairwise_autocorr(y, i, j) for i, j in combinations(lags, 2)]
    out['arch_reference_s'] = time.perf_counter() - t0
    m1 = rs.uniform(0, 10, n)
    m2, m3 = m1 + rs.uniform(0, 10, n), rs.uniform(0.01, 0.5, n)
    t0 = time.perf_counter()
    y = mg1.MG1(m1, m2, m3, n_obs=50, batch_size=n, random_state=rs)
    out['mg1_reference_simulator_s'] = time.perf_counter() - t0
    mg1.log_identity(y)
    mg1.quantiles(y, np.linspace(0, 1, 10))
    out['mg1_reference_s'] = time.perf_counter() - t0


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
    for n in (10 ** 5, 10 ** 6):
        rec = {}
        kernels(ctx, n, rec)
        host_forms(n, rec)
        if with_reference:
            reference(n, rec)
            assert n != 10 ** 5 or rec['arch_host_form_s'] < rec['arch_reference_s'], 'ARCH: the device form is not faster'
            assert n != 10 ** 5 or rec['mg1_host_form_s'] < rec['mg1_reference_s'], 'M/G/1: the device form is not faster'
        result['batch_%d' % n] = rec
        print('batch', n, json.dumps(rec), flush=True)
    if with_reference:
        for name, make in (('arch', elfi_amd.arch_model), ('mg1', elfi_amd.mg1_model)):
            m = make(seed_obs=4)
            t0 = time.perf_counter()
            res = elfi_amd.HipRejection(m['d'], batch_size=10 ** 6, seed=1).sample(1000, n_sim=10 ** 7)
            rec = {'seconds': time.perf_counter() - t0, 'threshold': float(res.threshold),
                   'means': {k: float(np.mean(v)) for k, v in res.samples.items()}}
            result['rejection_' + name] = rec
            print('rejection', name, json.dumps(rec), flush=True)
    if '--json' in sys.argv:
        path = sys.argv[sys.argv.index('--json') + 1]
        with open(path, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
