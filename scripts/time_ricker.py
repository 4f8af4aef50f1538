"""Times the Ricker example model on one MI355X next to the reference's simulator, summaries and chi_squared on the same
host, with the ARCH(1) kernel from the same run for scale (the same tile shape and one normal per step, no Poisson pass: the
difference bounds what the Poisson pass costs).

  kernel      the fused kernel alone, device pointers in and out (device timer; 1 warm-up, median of 5), batch 10^6, n_obs 50,
              parameters drawn from the model's priors: with the normals drawn in the kernel and every optional output
              (counts, stock, normals, distance); with the normals drawn and summaries + distance only; the deterministic
              form; the stochastic form at scale = 0 (every intensity 0: everything but the sampler); elfihip_poisson_dev
              alone on the model's 5 x 10^7 intensities in row-major and in column-major order; ARCH(1), n_obs 50, 5 lags,
              summaries + distance
  host form   elfi_amd.ricker_summaries: parameters up, summaries down, synchronised (host wall clock, median of 3)
  branches    the share of the Poisson intensities scale * stock (batch 10^5, from the device's own stock) in each branch of
              the sampler: invalid (NaN), exactly 0, inversion (0 < lam < 10), PTRS (lam >= 10), and the mean number of
              uniform pairs an element reads (tests/ricker_ref.py)
  reference   elfi.examples.ricker: stochastic_ricker + np.mean + np.var + num_zeros + chi_squared at batch 10^4, once

The reference is the imported ELFI's (through oracle/ref_shim.py where that copy is present); --no-reference skips it.

    python scripts/time_ricker.py [--no-reference] [--json out.json]
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
N_OBS = 50


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


def prior_draws(n, rs):
    import scipy.stats as ss
    return (ss.expon.rvs(np.e, 2, size=n, random_state=rs), ss.truncnorm.rvs(0, 5, size=n, random_state=rs),
            ss.uniform.rvs(0, 100, size=n, random_state=rs))


def kernels(ctx, out):
    import torch
    lib, h = ctx.lib, ctx.handle
    rs = np.random.RandomState(1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device='cuda')
    n = 10 ** 6
    t1, t2, t3 = [dev(a) for a in prior_draws(n, rs)]
    S, D, obs = empty(n, 3), empty(n), np.array([40.28, 3602.3616, 18.0])
    Y, St, Zo = empty(n, N_OBS), empty(n, N_OBS), empty(n, N_OBS)

    def ricker(full, stochastic=True):
        opt = lambda a: a.data_ptr() if full else None

        def launch():
            assert lib.elfihip_ricker_summaries_dev(h, None, N_OBS, U64(1), U64(0), n, N_OBS, t1.data_ptr(),
                                                    t2.data_ptr() if stochastic else None,
                                                    t3.data_ptr() if stochastic else None, C.c_double(1.0), obs.ctypes.data,
                                                    0 if stochastic else 1, S.data_ptr(), 3, opt(Y), N_OBS, opt(St), N_OBS,
                                                    opt(Zo) if stochastic else None, N_OBS, D.data_ptr()) == 0
        return median_ms(ctx, launch)
    out['batch'], out['n_obs'] = n, N_OBS
    for key, ms in (('ricker_all_outputs', ricker(True)), ('ricker_summaries_only', ricker(False)),
                    ('ricker_deterministic', ricker(False, stochastic=False))):
        out[key + '_kernel_ms'], out[key + '_sims_per_s'] = ms, n / (ms * 1e-3)
    # everything but the sampler: scale = 0 makes every intensity 0, which draws nothing
    t3_saved, t3 = t3, torch.zeros_like(t3)
    ms = ricker(False)
    t3 = t3_saved
    out['ricker_scale_zero_kernel_ms'] = ms
    # the sampler alone on the model's intensities (the stock of the run with every output), in the two orders a kernel
    # could present them to a wavefront: row-major (neighbouring lanes = neighbouring steps of one simulation, the order of
    # the kernel's element pass) and column-major (neighbouring lanes = unrelated simulations at the same step, what a
    # lane-per-simulation form would present)
    ricker(True)
    lam = t3[:, None] * St
    lam_t = lam.t().contiguous()
    torch.cuda.synchronize()
    for key, L in (('poisson_row_major', lam), ('poisson_column_major', lam_t)):
        def draw():
            assert lib.elfihip_poisson_dev(h, U64(1), U64(1), n * N_OBS, L.data_ptr(), Y.data_ptr()) == 0
        ms = median_ms(ctx, draw)
        out[key + '_ms'], out[key + '_elements_per_s'] = ms, n * N_OBS / (ms * 1e-3)
    del lam, lam_t
    a1, a2 = dev(rs.uniform(-1, 1, n)), dev(rs.uniform(0, 1, n))
    Sa, aobs = empty(n, 17), np.ones(17)

    def arch():
        assert lib.elfihip_arch_summaries_dev(h, None, N_OBS + 2, U64(1), U64(0), n, N_OBS, 5, a1.data_ptr(), a2.data_ptr(),
                                              aobs.ctypes.data, Sa.data_ptr(), 17, None, N_OBS, D.data_ptr()) == 0
    ms = median_ms(ctx, arch)
    out['arch_kernel_ms'], out['arch_sims_per_s'] = ms, n / (ms * 1e-3)


def host_form_and_branches(out):
    import elfi_amd
    import ricker_ref as R
    rs = np.random.RandomState(2)
    n = 10 ** 6
    t1, t2, t3 = prior_draws(n, rs)
    obs = np.array([40.28, 3602.3616, 18.0])
    s = wall_s(lambda: elfi_amd.ricker_summaries(t1, t2, t3, n_obs=N_OBS, seed=1, observed=obs))
    out['ricker_host_form_s'], out['ricker_host_form_sims_per_s'] = s, n / s
    n = 10 ** 5
    _, Y, St = elfi_amd.ricker_summaries(t1[:n], t2[:n], t3[:n], n_obs=N_OBS, seed=1, return_series=True, return_stock=True)
    lam = t3[:n, None] * St
    valid = (lam >= 0) & (lam <= 2.0 ** 53)
    out['branch_share'] = dict(invalid=float(np.mean(~valid)), zero=float(np.mean(lam == 0)),
                               inversion=float(np.mean(valid & (lam > 0) & (lam < 10))),
                               ptrs=float(np.mean(valid & (lam >= 10))))
    want, sens, attempts = R.poisson_ref(lam, 1, 1, return_attempts=True)
    ok = ~sens & ~(lam > 1e6)
    out['uniform_pairs_per_element'] = float(attempts.mean())
    out['masked_share'] = float(sens.mean())
    out['counts_equal_statement'] = bool(np.array_equal(Y[ok], want[ok], equal_nan=True))


def reference(out):
    from elfi.examples import ricker
    n = 10 ** 4
    obs = tuple(np.array([v]) for v in (40.28, 3602.3616, 18.0))
    for seed in range(3, 8):        # the reference refuses a whole batch that holds one overflowed stock: draw again
        rs = np.random.RandomState(seed)
        t1, t2, t3 = prior_draws(n, rs)
        try:
            t0 = time.perf_counter()
            y = ricker.stochastic_ricker(t1, t2, t3, n_obs=N_OBS, batch_size=n, random_state=rs)
            out['reference_simulator_s'] = time.perf_counter() - t0
            ricker.chi_squared(np.mean(y, axis=1), np.var(y, axis=1), ricker.num_zeros(y), observed=obs)
            s = time.perf_counter() - t0
        except ValueError as e:
            out['reference_refused_seed_%d' % seed] = str(e)
            continue
        out['reference_batch'], out['reference_s'], out['reference_sims_per_s'] = n, s, n / s
        break


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
    host_form_and_branches(rec)
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
