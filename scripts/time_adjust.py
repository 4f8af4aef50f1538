"""Times the device regression adjustment on one MI355X next to the reference's adjust_posterior on the same host.

  one      one adjustment of 10^4 accepted rows, 32 summaries, 4 parameters      adjust_posterior against adjust_posterior
  nested   one sample of 10^5 rows, 32 summaries, 4 parameters, 16 thresholds    ONE call with n_closest against 16 refits
  groups   64 samples of 1000 rows, 20 summaries, 4 parameters                   ONE linear_adjust against 64 calls

Host wall clock, copies and synchronisation included: 1 warm-up, then the median of 3.  The reference is the imported
ELFI's (through oracle/ref_shim.py where that copy is present).  The largest difference between the two results is
printed with each shape, in the metric of tests/adjust_ref.py.

    python scripts/time_adjust.py [--json out.json]
"""
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def median_time(fn):
    fn()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return sorted(times)[1], out


def synthetic(mod, rs, n, m, q):
    """(Sample ordered by discrepancy, model stand-in, summary names, parameter names)."""
    S = rs.randn(n, m) * np.linspace(0.5, 3.0, m)
    T = S[:, :q] * 0.5 + 0.3 * rs.randn(n, q)
    snames, pnames = ['s%d' % j for j in range(m)], ['t%d' % t for t in range(q)]
    order = np.argsort(np.sqrt((S * S).sum(axis=1)), kind='stable')
    outputs = {nm: np.ascontiguousarray(S[order, j]) for j, nm in enumerate(snames)}
    outputs.update({nm: np.ascontiguousarray(T[order, t]) for t, nm in enumerate(pnames)})
    outputs['d'] = np.sqrt((S * S).sum(axis=1))[order]
    sample = mod.results.Sample(method_name='Rejection', outputs=outputs, parameter_names=pnames, discrepancy_name='d')
    model = {nm: types.SimpleNamespace(observed=np.zeros(1)) for nm in snames}
    return sample, model, snames, pnames


def head(mod, sample, pnames, count):
    outputs = {k: v[:count] for k, v in sample.outputs.items()}
    return mod.results.Sample(method_name='Rejection', outputs=outputs, parameter_names=pnames, discrepancy_name='d')


def worst(got, want, pnames):
    import adjust_ref as R
    return max(R.adjusted_error(got.outputs[nm], want.outputs[nm]) for nm in pnames)


def main():
    import ref_shim
    if ref_shim.available():
        ref_shim.install()
    import elfi  # noqa: F401
    from elfi.methods import post_processing as mod
    import elfi_amd
    rs = np.random.RandomState(0)
    out = {}

    sample, model, snames, pnames = synthetic(mod, rs, 10 ** 4, 32, 4)
    dev_s, got = median_time(lambda: elfi_amd.adjust_posterior(sample, model, snames, pnames))
    ref_s, want = median_time(lambda: mod.adjust_posterior(sample, model, snames, pnames, mod.LinearAdjustment()))
    out['one'] = dict(n=10 ** 4, m=32, q=4, device_s=dev_s, reference_s=ref_s, difference=worst(got, want, pnames))
    print('one', json.dumps(out['one']), flush=True)

    sample, model, snames, pnames = synthetic(mod, rs, 10 ** 5, 32, 4)
    counts = [int(c) for c in np.linspace(10 ** 5 / 16, 10 ** 5, 16)]
    dev_s, got = median_time(lambda: elfi_amd.adjust_posterior(sample, model, snames, pnames, n_closest=counts))
    ref_s, want = median_time(lambda: [mod.adjust_posterior(head(mod, sample, pnames, c), model, snames, pnames,
                                                            mod.LinearAdjustment()) for c in counts])
    out['nested'] = dict(n=10 ** 5, m=32, q=4, K=16, device_s=dev_s, reference_s=ref_s,
                         difference=max(worst(g, w, pnames) for g, w in zip(got, want)))
    print('nested', json.dumps(out['nested']), flush=True)

    G, n, m, q = 64, 1000, 20, 4
    groups = [synthetic(mod, rs, n, m, q) for _ in range(G)]
    snames, pnames = groups[0][2], groups[0][3]
    Xg = np.stack([np.column_stack([s.outputs[nm] for nm in snames]) for s, _, _, _ in groups])
    Yg = np.stack([np.column_stack([s.outputs[nm] for nm in pnames]) for s, _, _, _ in groups])
    dev_s, got = median_time(lambda: elfi_amd.linear_adjust(Xg, Yg))
    ref_s, want = median_time(lambda: [mod.adjust_posterior(s, mdl, snames, pnames, mod.LinearAdjustment())
                                       for s, mdl, _, _ in groups])
    import adjust_ref as R
    diff = max(R.adjusted_error(got[g][:, t], want[g].outputs[nm]) for g in range(G) for t, nm in enumerate(pnames))
    out['groups'] = dict(G=G, n=n, m=m, q=q, device_s=dev_s, reference_s=ref_s, difference=diff)
    print('groups', json.dumps(out['groups']), flush=True)
    if '--json' in sys.argv:
        path = sys.argv[sys.argv.index('--json') + 1]
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
