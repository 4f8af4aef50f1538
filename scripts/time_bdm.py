"""Times the birth-death-mutation example on one MI355X, and the reference's external simulator on the same box's host.

  kernel      elfihip_bdm_clusters_dev, device pointers in and out, draws made in the kernel (device timer; 1 warm-up, median of
              5), mode 1: N = 20 in batches of 1, 500, 10^4 and 10^5 at the example's truth (0.2, 0, 0.198) and with alpha from
              the prior U(0.005, 2.005); N = 473 in a batch of 500.  The events made, the most events of one simulation, ns per
              event (device time over all events: the throughput figure), and a digest of the clusters to compare builds.
  slowest     the simulation of the prior batch with the most events, alone in a batch of 1: the tail, and with it the ns per
              event of a lone wavefront (the latency figure)
  host form   elfi_amd.bdm_clusters: parameters up, clusters down, synchronised (host wall clock, median of 5)
  reference   elfi.examples.bdm.BDM, the reference's elfi.tools.external_operation: np.savetxt, the `bdm` executable (compiled
              here from the reference's source into a temporary directory, -O2) as a subprocess, np.loadtxt and two deletions,
              per batch, the same parameters (host wall clock, median of 5; 10^5: of 3); --reference-only times it alone

    python scripts/time_bdm.py [--no-reference | --reference-only] [--json out.json]
"""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

U64 = C.c_uint64
TRUTH = (0.2, 0.0, 0.198)
MAX_EVENTS = 1 << 16
#         name           N    batch   prior
CASES = [('truth_1',     20,  1,      False), ('truth_500', 20, 500, False), ('truth_10000', 20, 10 ** 4, False),
         ('truth_100000', 20, 10 ** 5, False), ('prior_1', 20, 1, True), ('prior_500', 20, 500, True),
         ('prior_10000', 20, 10 ** 4, True), ('prior_100000', 20, 10 ** 5, True), ('N473_truth_500', 473, 500, False),
         ('N473_prior_500', 473, 500, True)]


def params(n, prior):
    rs = np.random.RandomState(1)
    return rs.uniform(0.005, 2.005, n) if prior else np.full(n, TRUTH[0])


def median_ms(ctx, launch, reps=5):
    launch()
    ctx.synchronize()
    times = []
    for _ in range(reps):
        ctx.timer_start()
        launch()
        times.append(ctx.timer_stop())
    return float(np.median(times)), float(min(times)), float(max(times))


def kernel_case(ctx, alpha, N, first=0):
    import torch
    lib, h, n = ctx.lib, ctx.handle, len(alpha)
    da = torch.from_numpy(np.ascontiguousarray(alpha)).cuda()
    dd, dt = torch.full((n,), TRUTH[1], dtype=torch.float64, device='cuda'), torch.full((n,), TRUTH[2], dtype=torch.float64, device='cuda')
    Cl = torch.empty((n, N), dtype=torch.int32, device='cuda')
    st, ev = torch.empty(n, dtype=torch.int32, device='cuda'), torch.empty(n, dtype=torch.int64, device='cuda')
    T, D = torch.empty((n, 2), dtype=torch.float64, device='cuda'), torch.empty(n, dtype=torch.float64, device='cuda')
    obs = np.array([0.55])
    torch.cuda.synchronize()

    def launch():
        assert lib.elfihip_bdm_clusters_dev(h, None, 0, U64(1), U64(0), first, n, N, 1, MAX_EVENTS, da.data_ptr(), dd.data_ptr(),
                                            dt.data_ptr(), C.c_double(N), obs.ctypes.data, Cl.data_ptr(), N, st.data_ptr(),
                                            ev.data_ptr(), T.data_ptr(), 2, D.data_ptr()) == 0
    out = dict(batch=n, N=N)
    out['ms'], out['ms_min'], out['ms_max'] = median_ms(ctx, launch)
    ctx.synchronize()
    events, status = ev.cpu().numpy(), st.cpu().numpy()
    out.update(events=int(events.sum()), median_events=float(np.median(events)), most_events=int(events.max()),
               most_events_at=int(events.argmax()), ns_per_event=float(out['ms'] * 1e6 / max(1, events.sum())),
               sims_per_s=n / (out['ms'] * 1e-3), not_reached=int((status != 0).sum()),
               digest=hashlib.sha256(Cl.cpu().numpy().tobytes()).hexdigest())
    return out


def host_form(rec):
    import elfi_amd
    for name, N, n, prior in CASES:
        alpha = params(n, prior)
        fn = lambda: elfi_amd.bdm_clusters(alpha, TRUTH[1], TRUTH[2], N=N, seed=1)      # noqa: E731
        fn()
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        rec[name]['host_form_ms'] = float(np.median(times)) * 1e3


def reference(rec):
    """The reference's own node operation in a temporary working directory that holds its compiled executable."""
    import ref_shim
    from elfi.examples import bdm
    src = os.path.join(ref_shim.REFERENCE_ROOT, 'elfi', 'examples', 'cpp', 'bdm.cpp') if ref_shim.available() else \
        os.path.join(bdm.get_sources_path(), 'bdm.cpp')
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([shutil.which('g++') or shutil.which('c++'), '-O2', '-std=c++11', '-o', os.path.join(tmp, 'bdm'), src], check=True)
        os.chdir(tmp)
        try:
            for k, (name, N, n, prior) in enumerate(CASES):
                alpha = params(n, prior)
                times = []
                for rep in range(3 if n >= 10 ** 5 else 5):
                    t0 = time.perf_counter()
                    y = bdm.BDM(alpha, TRUTH[1], TRUTH[2], N, batch_size=n, random_state=np.random.RandomState(rep),
                                meta=dict(model_name='bdm', batch_index=k, submission_index=rep))
                    times.append(time.perf_counter() - t0)
                assert np.atleast_2d(y).shape == (n, N)
                rec.setdefault(name, dict(batch=n, N=N))['reference_ms'] = float(np.median(times)) * 1e3
        finally:
            os.chdir(cwd)


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
        for name, N, n, prior in CASES:
            rec[name] = kernel_case(ctx, params(n, prior), N)
        for name, N in (('prior_100000', 20), ('N473_prior_500', 473)):
            at = rec[name]['most_events_at']
            alpha = params(rec[name]['batch'], True)
            rec['slowest_of_' + name] = kernel_case(ctx, alpha[at:at + 1], N, first=at)
        host_form(rec)
    if with_reference:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            reference(rec)
    for name, r in rec.items():
        if isinstance(r, dict) and 'reference_ms' in r and 'host_form_ms' in r:
            r['reference_over_host_form'] = r['reference_ms'] / r['host_form_ms']
    print(json.dumps(rec, indent=1), flush=True)
    if '--json' in sys.argv:
        path = sys.argv[sys.argv.index('--json') + 1]
        with open(path, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
