"""Developer tool: time the distance pass of canberra / braycurtis / cosine / correlation against cityblock.

usage: python scripts/time_metrics.py [--reps R] [--json PATH]

For each shape (10^6 x 32, 1.25 10^6 x 64, 4 10^6 x 2; and 2 10^6 x 16, the third DMA width), each metric, unweighted
and weighted, it times with the context's event timer (include/elfihip.h: elfihip_timer_start / _stop; R calls between
the events, after a warm-up):
  * dist     elfihip_dist_rows_dev, the row-major pass (form 0: LDS-DMA at 16 / 32 / 64 summaries, narrow rows at 2);
  * form1    the same call with elfihip_dist_set_form(1) (the register-staged pipeline), where form 0 is the DMA form;
  * push     elfihip_reject_push_rows_dev, the device form of RunningBest.push (k = 1000): the pass with the candidate
             offer and the sealed-list merge beside it;
  * cols     elfihip_dist_cols_dev on the same matrix stored column-major (correlation reads its columns twice).
Every call reads the next matrix of a rotation of copies that holds more than 640 MB (2.5 x the 256 MiB Infinity Cache),
as scripts/bench_kernels.py does.  The share of HBM peak counts (8 m + 8) bytes per row against 8 TB/s.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import elfi_amd
from elfi_amd import _lib

PEAK = 8e12
SHAPES = [(10 ** 6, 32), (1250000, 64), (4 * 10 ** 6, 2), (2 * 10 ** 6, 16)]
ROTATE = 640e6   # bytes a rotation of copies of the matrix spans at least
METRICS = ['cityblock', 'canberra', 'braycurtis', 'cosine', 'correlation']


def timed(ctx, f, reps):
    for _ in range(3):
        f()
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(reps):
        f()
    return ctx.timer_stop() / reps * 1e3   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    ctx = elfi_amd.Context(0)
    lib = ctx.lib
    dev = torch.device('cuda', 0)
    rows = []
    for n, m in SHAPES:
        g = torch.Generator(device=dev).manual_seed(n + m)
        copies = int(ROTATE // (8 * n * m)) + 2
        Xs = [torch.randn(n, m, dtype=torch.float64, device=dev, generator=g) for _ in range(copies)]
        Xcs = [X.t().contiguous() for X in Xs]  # column-major copies: column j at Xc[j]
        it = [0]

        def nxt(bufs):
            it[0] += 1
            return bufs[it[0] % copies].data_ptr()

        y = torch.randn(m, dtype=torch.float64, device=dev, generator=g)
        w = torch.rand(m, dtype=torch.float64, device=dev, generator=g) + 0.5
        out = torch.empty(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        nbytes = n * (8 * m + 8)
        for metric in METRICS:
            mid = _lib.METRICS[metric]
            for wt in (None, w):
                aux = None if wt is None else wt.data_ptr()

                def dist():
                    ctx.call('elfihip_dist_rows_dev', mid, nxt(Xs), n, m, m, y.data_ptr(), aux, C.c_double(2.0),
                             out.data_ptr())

                def cols():
                    ctx.call('elfihip_dist_cols_dev', mid, nxt(Xcs), n, m, n, y.data_ptr(), aux, C.c_double(2.0),
                             out.data_ptr())

                r = {'n': n, 'm': m, 'metric': metric, 'weighted': wt is not None}
                r['dist_us'] = timed(ctx, dist, a.reps)
                if m in (16, 32, 64):
                    ctx.call('elfihip_dist_set_form', 1)
                    r['form1_us'] = timed(ctx, dist, a.reps)
                    ctx.call('elfihip_dist_set_form', 0)
                r['cols_us'] = timed(ctx, cols, a.reps)
                h = C.c_void_p()
                ctx.call('elfihip_reject_create', 1000, C.byref(h))
                base = [0]

                def push():
                    rc = lib.elfihip_reject_push_rows_dev(h, mid, C.c_void_p(nxt(Xs)), n, m, m,
                                                          C.c_void_p(y.data_ptr()), None if aux is None else C.c_void_p(aux),
                                                          C.c_double(2.0), C.c_void_p(out.data_ptr()), base[0])
                    assert rc == 0, lib.elfihip_last_error(ctx.handle)
                    base[0] += n

                r['push_us'] = timed(ctx, push, a.reps)
                ctx.synchronize()
                lib.elfihip_reject_free(h)
                for key in ('dist', 'form1', 'push', 'cols'):
                    if key + '_us' in r:
                        r[key + '_hbm'] = nbytes / PEAK / (r[key + '_us'] * 1e-6)
                rows.append(r)
                print('%8d x %-3d %-12s %-3s dist %7.1f us (%.2f)  form1 %7s  push %7.1f us (%.2f)  cols %7.1f us (%.2f)' % (
                    n, m, metric, 'w' if r['weighted'] else '', r['dist_us'], r['dist_hbm'],
                    '%.1f' % r['form1_us'] if 'form1_us' in r else '-', r['push_us'], r['push_hbm'], r['cols_us'],
                    r['cols_hbm']), flush=True)
        del Xs, Xcs
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
