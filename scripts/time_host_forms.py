#!/usr/bin/env python3
"""Latency of three host-form calls of the example simulators (elfihip_arch_summaries, elfihip_lv_summaries,
elfihip_sv_summaries: draws made in the kernel, every optional output asked for) at the shapes of
tests/test_host_forms_subsets_gpu.py and a batch of 10^5, in THIS process:

    scripts/time_host_forms.py LIBRARY TAG

LIBRARY is the libelfihip.so to load (so that a parent build and the tree's can alternate in fresh processes), TAG goes into
the record.  Prints one JSON line: per entry point the median over the timed calls, in ms, and a digest of what it returned.
A host form ends in a stream synchronisation, so the host clock around the call is the call's time."""
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import elfi_amd._lib as L   # noqa: E402

L.LIB_PATH = os.path.abspath(sys.argv[1])
import elfi_amd   # noqa: E402

N, WARM, TIMED = 100000, 5, 30
U64, DBL = C.c_uint64, C.c_double
rs = np.random.RandomState(5)
p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
ctx = elfi_amd.Context()


def arch():
    t1, t2, obs = rs.uniform(-0.9, 0.9, N), rs.uniform(0.1, 0.9, N), rs.randn(5)
    out = [np.empty((N, 5)), np.empty((N, 5)), np.empty(N)]
    return out, lambda: ctx.call('elfihip_arch_summaries', None, U64(7), U64(2), N, 5, 2, p(t1), p(t2), p(obs), *[p(a) for a in out])


def lv():
    par = [rs.uniform(0.8, 1.2, N), rs.uniform(0.004, 0.006, N), rs.uniform(0.5, 0.7, N), np.full(N, 5.0), np.full(N, 10.0)]
    obs = np.arange(1.0, 10.0)
    out = [np.empty((N, 6)), np.empty(N), np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int64), np.empty((N, 9)), np.empty(N)]
    return out, lambda: ctx.call('elfihip_lv_summaries', None, None, None, U64(7), U64(2), 0, N, 3, DBL(2.0), 64,
                                 *[p(a) for a in par], None, p(obs), *[p(a) for a in out])


def sv():
    par = [rs.uniform(1.2, 1.9, N), rs.uniform(-0.5, 0.5, N), np.ones(N), np.zeros(N), np.zeros(N), np.full(N, 0.95), np.full(N, 0.2)]
    q = np.array([.05, .25, .75, .95, .05, .5, .95])
    out = [np.empty((N, 2))] + [np.empty((N, 3)) for _ in range(6)]
    return out, lambda: ctx.call('elfihip_sv_summaries', None, None, None, U64(7), U64(2), 0, N, 3, p(q), *[p(a) for a in par], None,
                                 *[p(a) for a in out])


res = {'tag': sys.argv[2], 'lib': sys.argv[1], 'n': N, 'timed': TIMED}
for name, make in (('arch', arch), ('lv', lv), ('sv', sv)):
    out, call = make()
    for _ in range(WARM):
        call()
    ts = []
    for _ in range(TIMED):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    res[name + '_ms'] = 1e3 * float(np.median(ts))
    res[name + '_digest'] = hashlib.sha256(b''.join(a.tobytes() for a in out)).hexdigest()[:16]
print(json.dumps(res))
