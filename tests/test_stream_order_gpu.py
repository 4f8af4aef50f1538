"""Every `_dev` entry point on a busy adopted stream, in stream order (include/elfihip.h: "enqueue on the context's stream
and return without synchronising; results are ordered with later work on the same stream").

A case issues its call twice, back to back, with different host-side arguments and into different outputs.  It runs twice
(tests/stream_order.py: Driver): the established way -- inputs filled and synchronised, the context's own stream, a
synchronisation behind every call -- and then on ONE non-null stream shared with torch that is busy for some 20 ms, where
the device inputs are poison (NaN, 0) until their contents arrive behind that delay, every host array argument is
overwritten the moment its call returns, nothing synchronises between the calls, and the stream must still be busy when
the last call has returned.  The two runs must agree bit for bit, sentinels around the outputs included: the synchronous
form is what the rest of the suite holds to the references, so no tolerance appears here.

What each outcome means: a mismatch = a launch, memset or copy outside the stream's order, a host argument read after the
call returned, or context-owned state reused by two calls in flight; "stream idle" = the call waited for the stream on the
host (a hidden synchronisation), or the delay was too short to tell.

Measured on an MI355X (ROCm 7.0): the delay is 20 ms (82 float64 matmuls of 2048^2 at 0.245 ms), the two or three calls of
a case are issued in 0.01 - 0.12 ms and the stream is still busy behind every case that must not synchronise; the pushes on a
host-merge state wait for the stream (19.7 ms) and elfihip_subset_best_dev does (24 ms), as the header says;
elfihip_reject_flush and elfihip_reject_state_dev on a device state do not.

The reference run fills its inputs only after the uploads have been synchronised and read back (stream_order.Driver.go).
What was observed while this module was written: with the reference run's device copy (poisoned buffer <- uploaded tensor,
torch's default stream) issued directly behind torch's blocking upload of the 208 000-byte draw matrices of `lv given`,
the REFERENCE of its first call differed from the host form elfi_amd.lotka_volterra_summaries on the same draws in 129 of
130 simulations, on every repetition in some processes and never in others, while the busy run equalled the host form bit
for bit each time; a read-back of the uploaded tensors showed the right data; with the copy issued behind a device
synchronisation both runs equal the host form (both orders were run in one process: the first differed, the second did
not).  The cause is NOT established.  A copy that overtakes the upload in front of it on one stream is only a supposition
-- it would be a fault of the runtime, and nothing here shows it.  The synchronisation in go() would hide another cause
just as well, which is why go() also reads every upload back and fails loudly when one is wrong.
"""
import ctypes as C

import numpy as np
import pytest

import stream_order as SO

pytestmark = pytest.mark.gpu

U64 = C.c_uint64
DBL = C.c_double
N = 4099                  # ragged over many tiles of every row kernel (tests/test_device_layouts_gpu.py: NS)


def _rows(n, m, seed):
    rs = np.random.RandomState(seed)
    return rs.randn(n, m) * rs.uniform(0.5, 3, m) + rs.uniform(-1, 1, m), rs.randn(m), rs.uniform(0.1, 2, m)


# ---------------------------------------------------------------------------------------------------------- distances
def _dist_rows(m, metric, weighted):
    def case(d):
        calls = []
        for which in (0, 1):
            X, y, w = _rows(N, m, 10 * m + which)
            calls.append((d.input(X), d.input(y), d.input(w) if weighted else None, d.out(N)))
        d.go()
        for x, y, w, o in calls:
            d.call('elfihip_dist_rows_dev', d.cx, metric, x.ptr, N, m, m, y.ptr, w.ptr if w else None, DBL(2.0), o.ptr)
        d.done()
    return case


def case_dist_cols(d):
    m, calls = 5, []
    for which in (0, 1):
        X, y, w = _rows(N, m, 50 + which)
        calls.append((d.input(X.T), d.input(y), d.input(w), d.out(N)))
    d.go()
    for x, y, w, o in calls:
        d.call('elfihip_dist_cols_dev', d.cx, 2, x.ptr, N, m, N, y.ptr, w.ptr, DBL(2.0), o.ptr)
    d.done()


def case_dist_multiw(d):
    m, K, calls = 32, 3, []
    for which in (0, 1):
        X, y, _ = _rows(N, m, 60 + which)
        W = np.vstack([np.ones(m), np.random.RandomState(which).uniform(0.2, 2, (K - 1, m))])
        calls.append((d.input(X), d.input(y), d.input(W), d.out(N, K)))
    d.go()
    for x, y, w, o in calls:
        d.call('elfihip_dist_multiw_dev', d.cx, x.ptr, N, m, m, y.ptr, w.ptr, K, o.ptr)
    d.done()


def case_daycare_distance(d):
    n, k, m, calls = 1000, 4, 5, []
    for which in (0, 1):
        rs = np.random.RandomState(70 + which)
        calls.append((d.input(rs.uniform(0, 1, (n, k * m))), d.host(rs.uniform(0.1, 1, (k, m))), d.out(n)))
    d.go()
    for x, obs, o in calls:
        d.call('elfihip_daycare_distance_dev', d.cx, x.ptr, k * m, n, k, m, obs.ctypes.data, o.ptr, host=(obs,))
    d.done()


# ------------------------------------------------------------------------------------------- statistics and selection
def case_welford_update(d):
    m, calls = 33, []
    for which in (0, 1):
        X, _, _ = _rows(N, m, 80 + which)
        rs = np.random.RandomState(which)
        calls.append((d.input(X), d.inout(np.concatenate([[100.0], rs.randn(m), rs.uniform(1, 2, m) * 100]))))
    d.go()
    for x, st in calls:
        d.call('elfihip_welford_update_dev', d.cx, x.ptr, N, m, m, st.ptr)
    d.done()


def case_welford_update_one_store(d):
    """Two updates in flight on ONE store: the second reads what the first leaves."""
    m = 64
    xs = [d.input(_rows(N, m, 90 + which)[0]) for which in (0, 1)]
    st = d.inout(np.zeros(1 + 2 * m))
    d.go()
    for x in xs:
        d.call('elfihip_welford_update_dev', d.cx, x.ptr, N, m, m, st.ptr)
    d.done()


def case_welford_merge(d):
    m, calls = 33, []
    for which in (0, 1):
        world = 3 + which
        rs = np.random.RandomState(95 + which)
        st = np.column_stack([rs.randint(50, 500, world).astype(np.float64), rs.randn(world, m), rs.uniform(1, 9, (world, m))])
        calls.append((world, d.input(st), d.out(1 + 2 * m), d.out(m)))
    d.go()
    for world, st, mg, w2 in calls:
        d.call('elfihip_welford_merge_dev', d.cx, st.ptr, world, m, mg.ptr, w2.ptr)
    d.done()


def case_weighted_var(d):
    m, calls = 33, []
    for which in (0, 1):
        X, _, _ = _rows(N, m, 100 + which)
        calls.append((d.input(X), d.input(np.random.RandomState(which).gamma(0.5, 1.0, N) + 1e-3), d.out(m)))
    d.go()
    for x, w, o in calls:
        d.call('elfihip_weighted_var_dev', d.cx, x.ptr, N, m, m, w.ptr, o.ptr)
    d.done()


def _topk(form, n, k):
    def case(d):
        import torch
        calls = []
        for which in (0, 1):
            D = np.random.RandomState(110 + which).rand(n)
            calls.append((d.input(D), k + 7 * which, d.out(k + 7 * which), d.out_raw(k + 7 * which, torch.int64)))
        d.cleanup.append(lambda: d.lib.elfihip_topk_set_form(d.cx, 0))
        assert d.lib.elfihip_topk_set_form(d.cx, form) == 0
        d.go()
        for x, kk, v, i in calls:
            d.call('elfihip_topk_smallest_dev', d.cx, x.ptr, n, 1, kk, v.ptr, i.ptr)
        d.done()
    return case


# ------------------------------------------------------------------------------------------------------ sampler state
class _State:
    def __init__(self, d, k):
        self.h = C.c_void_p()
        assert d.lib.elfihip_reject_create(d.cx, k, C.byref(self.h)) == 0
        d.cleanup.append(lambda: d.lib.elfihip_reject_free(self.h))
        self.k = k

    def result(self, d, name):
        vals, rows, cnt = np.full(self.k, -1.0), np.full(self.k, -1, dtype=np.int64), C.c_int64()
        assert d.lib.elfihip_reject_result(self.h, vals.ctypes.data, rows.ctypes.data, C.byref(cnt)) == 0
        d.keep(name + ' count', np.array([cnt.value]))
        d.keep(name + ' vals', vals[:cnt.value])
        d.keep(name + ' rows', rows[:cnt.value])


def _reject(k, m=32):
    """Three pushes in flight on one state -- fused with the row distances, with the K-weight distances, of distances that
    exist -- with the export buffer armed, then elfihip_reject_state_dev: work queued behind it sees every batch merged, so
    the k values and rows are read through the pointers it returns by device copies on the same stream.  Then
    elfihip_reject_result (which synchronises: behind done())."""
    def case(d):
        import torch
        K, ns = 3, (4099, 3000, 5000)
        st = _State(d, k)
        X0, y, w = _rows(ns[0], m, 120)
        X1 = _rows(ns[1], m, 121)[0]
        W = np.vstack([np.ones(m), np.random.RandomState(5).uniform(0.2, 2, (K - 2, m)), w])
        D2 = np.random.RandomState(122).rand(ns[2], 2) * 20
        x0, x1, d2, dy, dw, dW = d.input(X0), d.input(X1), d.input(D2), d.input(y), d.input(w), d.input(W)
        o0, o1 = d.out(ns[0]), d.out(ns[1], K)
        ex = d.out_raw(2 * k, torch.int64)
        sv, sr = d.out(k), d.out_raw(k, torch.int64)      # the state as elfihip_reject_state_dev shows it
        assert d.lib.elfihip_reject_export_dev(st.h, ex.ptr) == 0
        d.go()
        d.call('elfihip_reject_push_rows_dev', st.h, 0, x0.ptr, ns[0], m, m, dy.ptr, dw.ptr, DBL(2.0), o0.ptr, 0)
        d.call('elfihip_reject_push_multiw_dev', st.h, x1.ptr, ns[1], m, m, dy.ptr, dW.ptr, K, o1.ptr, ns[0])
        d.call('elfihip_reject_push_dev', st.h, d2.ptr + 8, ns[2], 2, ns[0] + ns[1])
        pv, pr = C.c_void_p(), C.c_void_p()
        d.call('elfihip_reject_state_dev', st.h, C.byref(pv), C.byref(pr))
        d.fetch(sv, pv.value, k)
        d.fetch(sr, pr.value, k)
        d.done()
        st.result(d, 'state')
    return case


def case_reject_flush(d):
    """elfihip_reject_flush between pushes on a device state (k <= 2048): the merge is queued, nothing waits."""
    import torch
    m, k, n = 32, 300, 3000
    st = _State(d, k)
    y, w = _rows(n, m, 125)[1:]
    xs = [d.input(_rows(n, m, 126 + b)[0]) for b in range(3)]
    dy, dw = d.input(y), d.input(w)
    outs = [d.out(n) for _ in xs]
    ex = d.out_raw(2 * k, torch.int64)
    assert d.lib.elfihip_reject_export_dev(st.h, ex.ptr) == 0
    d.go()
    for b, (x, o) in enumerate(zip(xs, outs)):
        d.call('elfihip_reject_push_rows_dev', st.h, 0, x.ptr, n, m, m, dy.ptr, dw.ptr, DBL(2.0), o.ptr, b * n)
        d.call('elfihip_reject_flush', st.h)
    d.done()
    st.result(d, 'state')


def case_adaptive_push(d):
    m, K, k = 32, 3, 50
    st = _State(d, k)
    calls = []
    for which in (0, 1, 2):
        X, y, _ = _rows(N, m, 130 + which)
        W = np.vstack([np.ones(m), np.random.RandomState(which).uniform(0.2, 2, (K - 1, m))])
        calls.append((d.input(X), d.input(y), d.input(W), d.out(N, K)))
    wel = d.inout(np.zeros(1 + 2 * m))
    d.go()
    for b, (x, y, w, o) in enumerate(calls):
        d.call('elfihip_adaptive_push_dev', d.cx, st.h, x.ptr, N, m, m, y.ptr, w.ptr, K, o.ptr, wel.ptr, b * N)
    d.done()
    st.result(d, 'state')


# --------------------------------------------------------------------------------------------------------- generators
def case_random_bits(d):
    import torch
    outs = [d.out_raw(4 * (5000 + which), torch.int32) for which in (0, 1)]
    d.go()
    for which, o in enumerate(outs):
        d.call('elfihip_random_bits_dev', d.cx, U64(3 + which), U64(which), 5000 + which, o.ptr)
    d.done()


def case_randn(d):
    outs = [d.out(70001 + which) for which in (0, 1)]
    d.go()
    for which, o in enumerate(outs):
        d.call('elfihip_randn_dev', d.cx, U64(3 + which), U64(2 * which), 70001 + which, DBL(-1.5 + which), DBL(2.25), o.ptr)
    d.done()


def case_prior_draw(d):
    n = 70001
    calls = [(d.host(np.array([0.5 + which, 2.0])), d.out(n)) for which in (0, 1)]
    d.go()
    for which, (a, o) in enumerate(calls):
        d.call('elfihip_prior_draw_dev', d.cx, 0, U64(9 + which), U64(which), n, a.ctypes.data, None, o.ptr, host=(a,))
    d.done()


def case_poisson(d):
    n, calls = 70001, []
    for which in (0, 1):
        rs = np.random.RandomState(140 + which)
        lam = np.concatenate([rs.uniform(0, 10, n // 2), 10 ** rs.uniform(1, 6, n - n // 2)])
        calls.append((d.input(lam), d.out(n)))
    d.go()
    for which, (lam, o) in enumerate(calls):
        d.call('elfihip_poisson_dev', d.cx, U64(3 + which), U64(2 + which), n, lam.ptr, o.ptr)
    d.done()


def _stable(drawn):
    def case(d):
        n, calls = 70001, []
        for which in (0, 1):
            rs = np.random.RandomState(150 + which)
            ins = [d.input(rs.uniform(0.3, 2, n)), d.input(rs.uniform(0.1, 5, n))]
            ins += [None, None] if drawn else [d.input(rs.uniform(-1.5, 1.5, n)), d.input(rs.exponential(1.0, n))]
            calls.append((ins, d.out(n)))
        d.go()
        for which, (ins, o) in enumerate(calls):
            d.call('elfihip_stable_dev', d.cx, U64(5 + which), U64(2 + which), n, *[b.ptr if b else None for b in ins], o.ptr)
        d.done()
    return case


def _stable_general(drawn):
    def case(d):
        n, calls = 70001, []
        for which in (0, 1):
            rs = np.random.RandomState(160 + which)
            ins = [d.input(rs.uniform(0.3, 2, n)), d.input(rs.uniform(-1, 1, n)), d.input(rs.randn(n)), d.input(rs.uniform(0.1, 5, n))]
            ins += [None, None] if drawn else [d.input(rs.uniform(-1.5, 1.5, n)), d.input(rs.exponential(1.0, n))]
            calls.append((ins, d.out(n)))
        d.go()
        for which, (ins, o) in enumerate(calls):
            d.call('elfihip_stable_general_dev', d.cx, U64(5 + which), U64(2 + which), n, which,
                   *[b.ptr if b else None for b in ins], o.ptr)
        d.done()
    return case


# ------------------------------------------------------------------------------------------------------- fused models
def case_row_summary(d):
    L, calls = 100, []
    for which in (0, 1):
        rs = np.random.RandomState(170 + which)
        calls.append((d.input(rs.randn(N, L) * rs.uniform(0.1, 50, L)), d.out(N)))
    d.go()
    for which, (x, o) in enumerate(calls):
        d.call('elfihip_row_summary_dev', d.cx, 2, x.ptr, N, L, L, 1 + 6 * which, o.ptr)
    d.done()


def _ma2(drawn):
    def case(d):
        n_obs, calls = 100, []
        for which in (0, 1):
            rs = np.random.RandomState(180 + which)
            w = None if drawn else d.input(rs.randn(N, n_obs + 2))
            calls.append((w, d.input(rs.uniform(-2, 2, N)), d.input(rs.uniform(-1, 1, N)), [d.out(N) for _ in range(3)]))
        d.go()
        for which, (w, t1, t2, o) in enumerate(calls):
            tail = (t1.ptr, t2.ptr, DBL(0.3 + which), DBL(0.1 - which), o[0].ptr, o[1].ptr, o[2].ptr)
            if drawn:
                d.call('elfihip_ma2_draw_distance_dev', d.cx, U64(4 + which), U64(which), N, n_obs, *tail)
            else:
                d.call('elfihip_ma2_distance_dev', d.cx, w.ptr, N, n_obs, n_obs + 2, *tail)
        d.done()
    return case


def _gauss(drawn):
    def case(d):
        n, n_obs, calls = 1000, 50, []
        for which in (0, 1):
            rs = np.random.RandomState(190 + which)
            z = None if drawn else d.input(rs.randn(n, n_obs))
            calls.append((z, d.input(rs.randn(n)), d.input(rs.uniform(0.5, 2, n)), d.out(n, n_obs), [d.out(n) for _ in range(3)]))
        d.go()
        for which, (z, mu, sg, y, o) in enumerate(calls):
            d.call('elfihip_gauss_distance_dev', d.cx, z.ptr if z else None, n_obs, U64(1 + which), U64(2 + which), n, n_obs,
                   mu.ptr, sg.ptr, DBL(0.2 + which), DBL(1.1), y.ptr, o[0].ptr, o[1].ptr, o[2].ptr)
        d.done()
    return case


# ------------------------------------------------------------------------------- likelihoods and post-processing
def _synlik_inputs(which, n=600, m=8, G=3):
    rs = np.random.RandomState(200 + which)
    X = rs.randn(G * n, m) * np.linspace(1, 5, m) + 3.0
    y = rs.randn(m) + 3.0
    pre = np.array([n // 2 + 1 + which, n], dtype=np.int64)
    pens = np.array([0.1 + 0.2 * which, 0.6])
    return X, y, pre, pens, G, n, m


def _issue_synlik(d, which):
    X, y, pre, pens, G, n, m = _synlik_inputs(which)
    x, dy, hp, hq = d.input(X), d.input(y), d.host(pre), d.host(pens)
    outs = (d.out(G * 2 * 2), d.out(G * m), d.out(G * m * m))

    def issue():
        d.call('elfihip_syn_loglik_dev', d.cx, x.ptr, G, n, m, m, dy.ptr, None, 0, None, hp.ctypes.data, 2, hq.ctypes.data, 2,
               outs[0].ptr, outs[1].ptr, outs[2].ptr, host=(hp, hq))
    return issue


def _issue_semi(d, which):
    X, y, pre, pens, G, n, m = _synlik_inputs(2 + which, n=400)
    x, dy, hp, hq = d.input(X), d.input(y), d.host(pre), d.host(pens)
    outs = (d.out(G * 2 * 2), d.out(G * m), d.out(G * m * m), d.out(G * n, m))

    def issue():
        d.call('elfihip_semi_loglik_dev', d.cx, x.ptr, G, n, m, m, dy.ptr, hp.ctypes.data, 2, hq.ctypes.data, 2,
               outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, host=(hp, hq))
    return issue


def _two(issue_of):
    def case(d):
        issues = [issue_of(d, which) for which in (0, 1)]
        d.go()
        for issue in issues:
            issue()
        d.done()
    return case


def _issue_adjust(d, which):
    import torch
    G, n, m, q = 3, 700, 5, 2
    rs = np.random.RandomState(210 + which)
    X = rs.randn(G * n, m) * np.linspace(0.5, 4, m)
    Y = rs.randn(G * n, q)
    Y += X[:, :q]
    pre = np.array([300 + which, 512, n], dtype=np.int64)
    K = len(pre)
    x, yy, hp = d.input(X), d.input(Y), d.host(pre)
    outs = (d.out(G * K * n * q), d.out(G * K * q * m), d.out(G * K * q), d.out(G * K * q), d.out_raw(G * K, torch.int32))

    def issue():
        d.call('elfihip_linear_adjust_dev', d.cx, x.ptr, G, n, m, m, yy.ptr, q, q, hp.ctypes.data, K, *[o.ptr for o in outs],
               host=(hp,))
    return issue


def _issue_log_ratio(d, which):
    import torch
    G, n, m, nm, k = 4, 60, 5, 45, 2
    rs = np.random.RandomState(220 + which)
    X = rs.randn(G * n, m) + np.repeat(np.linspace(0.2, 0.8, G), n)[:, None]
    M, obs = 1.3 * rs.randn(nm, m), rs.randn(k, m) + 0.4
    x, dm, dobs = d.input(X), d.input(M), d.input(obs)
    outs = (d.out(G * k), d.out(G * m), d.out(G), d.out(G * m), d.out(G * m), d.out_raw(G, torch.int32), d.out_raw(G, torch.int32))

    def issue():
        d.call('elfihip_log_ratio_dev', d.cx, x.ptr, G, n, m, m, dm.ptr, nm, m, dobs.ptr, k, DBL(1.0 + which), DBL(0.0),
               DBL(1e-8), 200, *[o.ptr for o in outs])
    return issue


def _issue_knn(d, which):
    G, n, q, k = 7, 300, 2, 4 + which
    T = np.random.RandomState(230 + which).randn(G * n, q)
    t, oE, oK = d.input(T), d.out(G), d.out(G * n)
    return lambda: d.call('elfihip_knn_entropy_dev', d.cx, t.ptr, G, n, q, q, k, oE.ptr, oK.ptr)


def _issue_mrsse(d, which):
    G, n, q, J = 7, 300, 2, 9 + which
    rs = np.random.RandomState(240 + which)
    t, c, o = d.input(rs.randn(G * n, q)), d.input(rs.randn(J, q)), d.out(G)
    return lambda: d.call('elfihip_mrsse_dev', d.cx, t.ptr, G, n, q, q, c.ptr, J, q, o.ptr)


def _issue_subset(d, which):
    import torch
    n, m, Cn, k = 3000, 5, 65 + which, 200       # (more than 64 combinations: two blocks)
    rs = np.random.RandomState(250 + which)
    X, y = rs.randn(n, m) * np.linspace(0.5, 2.0, m), rs.randn(m)
    masks = (rs.rand(Cn, m) < 0.5).astype(np.float64)
    masks[np.arange(Cn), rs.randint(0, m, Cn)] = 1.0
    x, dy, hm = d.input(X), d.input(y), d.host(masks)
    oV, oR = d.out(Cn, k), d.out_raw(Cn * k, torch.int64)
    return lambda: d.call('elfihip_subset_best_dev', d.cx, x.ptr, n, m, m, dy.ptr, hm.ctypes.data, Cn, k, oV.ptr, oR.ptr,
                          host=(hm,))


# ------------------------------------------------------------------------ fused models with host arrays, given and drawn
def _qpos(q, n_obs, d):
    from elfi_amd.summaries import quantile_positions
    return [d.host(a) for a in quantile_positions(q, n_obs)]


def _arch(drawn):
    def issue_of(d, which):
        n, n_obs, n_lags, m = 777, 100, 5, 17
        rs = np.random.RandomState(500 + which)
        w = None if drawn else d.input(rs.randn(n, n_obs + 2))
        t1, t2, obs = d.input(rs.uniform(-1, 1, n)), d.input(rs.uniform(0, 1, n)), d.host(rs.randn(m))
        S, Y, D = d.out(n, m), d.out(n, n_obs), d.out(n)
        return lambda: d.call('elfihip_arch_summaries_dev', d.cx, w.ptr if w else None, n_obs + 2, U64(11 + which), U64(which), n,
                              n_obs, n_lags, t1.ptr, t2.ptr, obs.ctypes.data, S.ptr, m, Y.ptr, n_obs, D.ptr, host=(obs,))
    return _two(issue_of)


def _mg1(drawn):
    def issue_of(d, which):
        n, n_obs, nq = 1000, 50, 10
        rs = np.random.RandomState(510 + which)
        t1 = rs.uniform(0, 10, n)
        E = None if drawn else d.input(rs.exponential(size=(n, n_obs)))
        V = None if drawn else d.input(rs.uniform(size=(n, n_obs)))
        dt = [d.input(a) for a in (t1, t1 + rs.uniform(0, 10, n), rs.uniform(0.01, 0.5, n))]
        lo, hi, t = _qpos(np.linspace(0, 1, nq) ** (1 + which), n_obs, d)
        obs, w = d.host(rs.uniform(0, 5, nq)), d.host(rs.uniform(0.5, 2, nq))
        LY, Q, Y, Eo, Vo, D = d.out(n, n_obs), d.out(n, nq), d.out(n, n_obs), d.out(n, n_obs), d.out(n, n_obs), d.out(n)
        return lambda: d.call('elfihip_mg1_summaries_dev', d.cx, E.ptr if E else None, n_obs, V.ptr if V else None, n_obs,
                              U64(12 + which), U64(2 * which), n, n_obs, dt[0].ptr, dt[1].ptr, dt[2].ptr, nq, lo.ctypes.data,
                              hi.ctypes.data, t.ctypes.data, obs.ctypes.data, w.ctypes.data, LY.ptr, n_obs, Q.ptr, nq, Y.ptr, n_obs,
                              Eo.ptr, n_obs, Vo.ptr, n_obs, D.ptr, host=(lo, hi, t, obs, w))
    return _two(issue_of)


def _ricker(drawn):
    def issue_of(d, which):
        n, n_obs = 777, 51
        rs = np.random.RandomState(520 + which)
        Z = None if drawn else d.input(rs.randn(n, n_obs))
        dt = [d.input(a) for a in (3.0 + rs.exponential(1.0, n), rs.uniform(0, 1, n), rs.uniform(0, 20, n))]
        obs = d.host(np.array([3.5 + which, 40.25, 7.0]))
        S, Y, St, Zo, D = d.out(n, 3), d.out(n, n_obs), d.out(n, n_obs), d.out(n, n_obs), d.out(n)
        return lambda: d.call('elfihip_ricker_summaries_dev', d.cx, Z.ptr if Z else None, n_obs, U64(13 + which), U64(which), n,
                              n_obs, dt[0].ptr, dt[1].ptr, dt[2].ptr, DBL(1.0 + which), obs.ctypes.data, 0, S.ptr, 3, Y.ptr, n_obs,
                              St.ptr, n_obs, Zo.ptr, n_obs, D.ptr, host=(obs,))
    return _two(issue_of)


def _gnk(drawn):
    def issue_of(d, which):
        from elfi_amd.summaries import GNK_OCTILES
        n, n_obs, dim = 203, 50, 1
        rs = np.random.RandomState(530 + which)
        L = n_obs * dim
        Z = None if drawn else d.input(rs.standard_normal((n, L)))
        P = d.input(rs.uniform(0, 10, (n, 4)))
        lo, hi, t = _qpos(np.true_divide(GNK_OCTILES, 100), n_obs, d)
        obs = d.host(rs.uniform(0, 10, 7 * dim))
        outs = [d.out(n, w) for w in (L, L, L, 7 * dim, 4 * dim)]
        D = d.out(n)
        args = []
        for o, w in zip(outs, (L, L, L, 7 * dim, 4 * dim)):
            args += [o.ptr, w]
        return lambda: d.call('elfihip_gnk_summaries_dev', d.cx, Z.ptr if Z else None, L, U64(14 + which), U64(which), n, n_obs,
                              dim, P.ptr, 4, DBL(0.8), lo.ctypes.data, hi.ctypes.data, t.ctypes.data, obs.ctypes.data, 2, *args,
                              D.ptr, host=(lo, hi, t, obs))
    return _two(issue_of)


def _lorenz(drawn):
    def issue_of(d, which):
        n, T, K, phi = 300, 20, 8, 0.984
        rs = np.random.RandomState(540 + which)
        E = None if drawn else d.input(rs.randn(n, (T - 1) * K))
        t1, t2, y0 = d.input(rs.uniform(0.5, 3.5, n)), d.input(rs.uniform(0, 0.3, n)), d.input(3.0 * rs.randn(n, K))
        obs = d.host(rs.randn(6))
        S, Y, D = d.out(n, 6), d.out(n, T * K), d.out(n)
        c, h = float(np.sqrt(1 - pow(phi, 2))), 0.5 / T
        return lambda: d.call('elfihip_lorenz_summaries_dev', d.cx, E.ptr if E else None, (T - 1) * K, U64(15 + which), U64(which),
                              n, K, T, t1.ptr, t2.ptr, DBL(10.0), DBL(c), DBL(phi), DBL(h), y0.ptr, K, obs.ctypes.data, S.ptr, 6,
                              Y.ptr, T * K, D.ptr, host=(obs,))
    return _two(issue_of)


def _lv(drawn):
    def issue_of(d, which):
        import torch
        n, n_obs, time_end, n_events = 130, 7, 2.0, 200
        rs = np.random.RandomState(550 + which)
        p = [np.exp(rs.uniform(-6, 2, n)) for _ in range(3)] + [rs.normal(50, np.sqrt(50), n), rs.normal(100, 10, n),
                                                                  np.exp(rs.uniform(np.log(0.5), np.log(50), n))]
        ins = [None] * 3 if drawn else [d.input(rs.exponential(size=(n, n_events))), d.input(rs.uniform(size=(n, n_events))),
                                         d.input(rs.randn(n, 2 * (n_obs - 1)))]
        dp = [d.input(a) for a in p]
        obs = d.host(np.array([170., 180., 8.9, 9.8, 0.8, 0.85, 0.55, 0.6, 0.1]) + which)
        Y, T, st, ev = d.out(n, 2 * n_obs), d.out(n), d.out_raw(n, torch.int32), d.out_raw(n, torch.int64)
        S, D = d.out(n, 9), d.out(n)
        lds = (n_events, n_events, 2 * (n_obs - 1))
        head = []
        for b, ld in zip(ins, lds):
            head += [b.ptr if b else None, ld]
        return lambda: d.call('elfihip_lv_summaries_dev', d.cx, *head, U64(16 + which), U64(which), 1000 * which, n, n_obs,
                              DBL(time_end), n_events, *[a.ptr for a in dp], obs.ctypes.data, Y.ptr, 2 * n_obs, T.ptr, st.ptr,
                              ev.ptr, S.ptr, 9, D.ptr, host=(obs,))
    return _two(issue_of)


def _issue_lv_draws(d, which):
    n, n_events = 130, 200 + which
    E, U = d.out(n, n_events), d.out(n, n_events)
    return lambda: d.call('elfihip_lv_draws_dev', d.cx, U64(5 + which), U64(2), 77 * which, n, n_events, E.ptr, n_events, U.ptr,
                          n_events)


def _daycare(drawn):
    def issue_of(d, which):
        import torch
        n, n_dcc, n_ind, n_strains, n_obs, time_end, n_events = 7, 5, 9, 6, 7, 2.0, 120
        rs = np.random.RandomState(560 + which)
        pairs = n * n_dcc
        E = None if drawn else d.input(rs.exponential(size=(pairs, n_events)))
        U = None if drawn else d.input(rs.uniform(size=(pairs, n_events)))
        dt = [d.input(a) for a in (rs.uniform(0, 11, n), rs.uniform(0, 2, n), rs.uniform(0, 1, n))]
        obs = d.host(np.stack([rs.uniform(0, 2, n_dcc), rs.randint(0, 11, n_dcc).astype(float), rs.uniform(0, 1, n_dcc),
                               rs.uniform(0, 1, n_dcc)]))
        freq = d.host(rs.uniform(0, 0.3, n_strains))
        M, T, st, ev = d.out_raw(pairs * n_obs, torch.int64), d.out(pairs), d.out_raw(pairs, torch.int32), d.out_raw(pairs, torch.int64)
        S, D = d.out(n, 4 * n_dcc), d.out(n)
        return lambda: d.call('elfihip_daycare_summaries_dev', d.cx, E.ptr if E else None, n_events, U.ptr if U else None, n_events,
                              U64(17 + which), U64(which), 50 * which, n, n_dcc, n_ind, n_strains, n_obs, DBL(time_end), n_events,
                              dt[0].ptr, dt[1].ptr, dt[2].ptr, freq.ctypes.data, obs.ctypes.data, M.ptr, n_obs, T.ptr, st.ptr,
                              ev.ptr, S.ptr, 4 * n_dcc, D.ptr, host=(freq, obs))
    return _two(issue_of)


def _issue_daycare_draws(d, which):
    n, n_dcc, n_events = 7, 5, 120 + which
    E, U = d.out(n * n_dcc, n_events), d.out(n * n_dcc, n_events)
    return lambda: d.call('elfihip_daycare_draws_dev', d.cx, U64(5 + which), U64(2), 9 * which, n, n_dcc, n_events, E.ptr,
                          n_events, U.ptr, n_events)


def _toad(drawn):
    def issue_of(d, which):
        import torch
        n, n_toads, n_days, nq = 5, 5, 9, 11
        cells, grid = (n_days - 1) * n_toads, n_days * n_toads
        rs = np.random.RandomState(570 + which)
        ins = [None] * 4
        if not drawn:
            R = np.stack([rs.randint(0, i, (n, n_toads)) for i in range(1, n_days)], axis=1).astype(np.int32)
            ins = [d.input(rs.uniform(size=(n, cells))), d.input(rs.uniform(-1.5, 1.5, (n, cells))),
                   d.input(rs.exponential(size=(n, cells))), d.input(R)]
        dp = [d.input(a) for a in (rs.uniform(1, 2, n), rs.uniform(0, 100, n), rs.uniform(0, 0.9, n))]
        lags = d.host(np.array([[1, 8], [2, 4]][which], dtype=np.int32))
        p = d.host(np.linspace(0, 1, nq) ** (1 + which))
        ns = (nq + 1) * len(lags)
        S, X, Dx = d.out(n, ns), d.out(n, grid), d.out(n, cells)
        echo = [d.out(n, cells) for _ in range(3)] + [d.out_raw(n * cells, torch.int32)]
        return lambda: d.call('elfihip_toad_summaries_dev', d.cx, *[b.ptr if b else None for b in ins], cells, U64(8 + which),
                              U64(which), 40 * which, n, n_toads, n_days, len(lags), lags.ctypes.data, nq, p.ctypes.data,
                              DBL(10.0 + which), dp[0].ptr, dp[1].ptr, dp[2].ptr, S.ptr, ns, X.ptr, grid, Dx.ptr, cells,
                              echo[0].ptr, echo[1].ptr, echo[2].ptr, echo[3].ptr, cells, host=(lags, p))
    return _two(issue_of)


def _sv(drawn):
    def issue_of(d, which):
        n, n_obs = 5, 37
        rs = np.random.RandomState(580 + which)
        ins = [None] * 3 if drawn else [d.input(rs.randn(n, n_obs)), d.input(rs.uniform(-1.5, 1.5, (n, n_obs))),
                                         d.input(rs.exponential(size=(n, n_obs)))]
        par = [rs.uniform(0.5, 2, n), rs.uniform(-1, 1, n), rs.uniform(0.5, 2, n), rs.uniform(-1, 1, n), rs.uniform(-1, 1, n),
               rs.uniform(-0.9, 0.9, n), rs.uniform(0, 0.5, n), rs.uniform(-1, 1, n)]
        dp = [d.input(a) for a in par]
        q = d.host(np.array([0.05, 0.25, 0.75, 0.95, 0.05, 0.5, 0.95]) + 0.01 * which)
        S, Y, X, V = d.out(n, 2), d.out(n, n_obs), d.out(n, n_obs), d.out(n, n_obs)
        echo = [d.out(n, n_obs) for _ in range(3)]
        return lambda: d.call('elfihip_sv_summaries_dev', d.cx, *[b.ptr if b else None for b in ins], n_obs, U64(8 + which),
                              U64(which), 30 * which, n, n_obs, q.ctypes.data, *[a.ptr for a in dp], S.ptr, 2, Y.ptr, n_obs, X.ptr,
                              n_obs, V.ptr, n_obs, echo[0].ptr, echo[1].ptr, echo[2].ptr, n_obs, host=(q,))
    return _two(issue_of)


# -------------------------------------------------------------------------------------------------------- cross-family
def case_dist_topk_push(d):
    """The staging buffers are the context's: a distance pass, a selection in its results and a push of them, in flight."""
    import torch
    m, k = 32, 100
    X, y, w = _rows(N, m, 300)
    st = _State(d, k)
    x, dy, dw = d.input(X), d.input(y), d.input(w)
    dist, vals, idx = d.out(N), d.out(k), d.out_raw(k, torch.int64)
    d.go()
    d.call('elfihip_dist_rows_dev', d.cx, 0, x.ptr, N, m, m, dy.ptr, dw.ptr, DBL(2.0), dist.ptr)
    d.call('elfihip_topk_smallest_dev', d.cx, dist.ptr, N, 1, k, vals.ptr, idx.ptr)
    d.call('elfihip_reject_push_dev', st.h, dist.ptr, N, 1, 0)
    d.done()
    st.result(d, 'state')


def case_synlik_then_semi(d):
    """Both keep their group parameters in the context's `par` buffer."""
    a, b = _issue_synlik(d, 0), _issue_semi(d, 0)
    d.go()
    a()
    b()
    d.done()


def case_drawn_model_then_distance(d):
    """A drawn model's summaries read by a distance pass in the same submission."""
    n_obs = 100
    t1, t2 = d.input(np.random.RandomState(1).uniform(-2, 2, N)), d.input(np.random.RandomState(2).uniform(-1, 1, N))
    S = d.out(N, 2)              # S1 and S2 as two columns of one matrix, column-major: what dist_cols reads
    dd, y, dist = d.out(N), d.input(np.array([0.3, 0.1])), d.out(N)
    d.go()
    d.call('elfihip_ma2_draw_distance_dev', d.cx, U64(4), U64(0), N, n_obs, t1.ptr, t2.ptr, DBL(0.3), DBL(0.1), S.ptr,
           S.ptr + 8 * N, dd.ptr)
    d.call('elfihip_dist_cols_dev', d.cx, 0, S.ptr, N, 2, N, y.ptr, None, DBL(2.0), dist.ptr)
    d.done()


# ----------------------------------------------------------------------------------------------------------- the table
# (name, case, syncs): syncs = the header documents a synchronisation; only the "still busy" assertion is skipped
CASES = [
    ('dist_rows narrow euclidean', _dist_rows(4, 0, True), False),
    ('dist_rows lds-dma euclidean', _dist_rows(32, 0, True), False),
    ('dist_rows wide euclidean', _dist_rows(300, 0, False), False),
    ('dist_rows lds-dma canberra', _dist_rows(32, 7, False), False),
    ('dist_rows pipelined cosine', _dist_rows(48, 9, True), False),
    ('dist_cols', case_dist_cols, False),
    ('dist_multiw', case_dist_multiw, False),
    ('daycare_distance', case_daycare_distance, False),
    ('welford_update', case_welford_update, False),
    ('welford_update one store', case_welford_update_one_store, False),
    ('welford_merge', case_welford_merge, False),
    ('weighted_var', case_weighted_var, False),
    ('topk form 0', _topk(0, 70001, 300), False),
    ('topk form 1', _topk(1, 70001, 300), False),
    ('topk form 2', _topk(2, 70001, 300), False),
    ('reject pushes k=300', _reject(300), False),
    ('reject_flush k=300', case_reject_flush, False),
    ('reject pushes k=4096 (host merge)', _reject(4096), True),
    ('adaptive_push', case_adaptive_push, True),
    ('random_bits', case_random_bits, False),
    ('randn', case_randn, False),
    ('prior_draw', case_prior_draw, False),
    ('poisson', case_poisson, False),
    ('stable given', _stable(False), False),
    ('stable drawn', _stable(True), False),
    ('stable_general given', _stable_general(False), False),
    ('stable_general drawn', _stable_general(True), False),
    ('row_summary', case_row_summary, False),
    ('ma2_distance', _ma2(False), False),
    ('ma2_draw_distance', _ma2(True), False),
    ('gauss_distance given', _gauss(False), False),
    ('gauss_distance drawn', _gauss(True), False),
    ('arch given', _arch(False), False), ('arch drawn', _arch(True), False),
    ('mg1 given', _mg1(False), False), ('mg1 drawn', _mg1(True), False),
    ('ricker given', _ricker(False), False), ('ricker drawn', _ricker(True), False),
    ('gnk given', _gnk(False), False), ('gnk drawn', _gnk(True), False),
    ('lorenz given', _lorenz(False), False), ('lorenz drawn', _lorenz(True), False),
    ('lv given', _lv(False), False), ('lv drawn', _lv(True), False),
    ('lv_draws', _two(_issue_lv_draws), False),
    ('daycare given', _daycare(False), False), ('daycare drawn', _daycare(True), False),
    ('daycare_draws', _two(_issue_daycare_draws), False),
    ('toad given', _toad(False), False), ('toad drawn', _toad(True), False),
    ('sv given', _sv(False), False), ('sv drawn', _sv(True), False),
    ('syn_loglik', _two(_issue_synlik), False),
    ('semi_loglik', _two(_issue_semi), False),
    ('linear_adjust', _two(_issue_adjust), False),
    ('log_ratio', _two(_issue_log_ratio), False),
    ('knn_entropy', _two(_issue_knn), False),
    ('mrsse', _two(_issue_mrsse), False),
    ('subset_best', _two(_issue_subset), True),
    ('dist_rows -> topk -> reject_push', case_dist_topk_push, False),
    ('syn_loglik -> semi_loglik', case_synlik_then_semi, False),
    ('drawn ma2 -> dist_cols', case_drawn_model_then_distance, False),
]


def test_the_control_sees_the_poison():
    """The harness is not vacuous: with the delay pending on the adopted stream, a reader on the null stream observes the
    poison of a buffer whose contents are enqueued behind the delay."""
    SO.select_stream()
    assert 'stream' in SO._state
    print('stream_order control:', SO._state['control'])


@pytest.mark.parametrize('name,case,syncs', CASES, ids=[c[0].replace(' ', '_') for c in CASES])
def test_dev_entry_point_in_stream_order(hip_ctx, name, case, syncs):
    ref, got, d = SO.run_both(hip_ctx, case, name, syncs)
    SO.guards_intact(ref, d.guarded)
    SO.guards_intact(got, d.guarded)
    SO.assert_same(ref, got, name)
    if not syncs:
        assert d.still_busy, ('%s: the stream was idle when the last call had returned (delay %.1f ms, calls issued in '
                              '%.1f ms): a call waited for the stream on the host' % (name, d.delay, d.issue_ms))


def test_host_forms_on_the_adopted_busy_stream(hip_ctx):
    """A host form synchronises, so its inputs may be overwritten as soon as it has returned, whatever else the adopted
    stream is doing: the results are the own-stream results."""
    import elfi_amd
    X, y, w = _rows(N, 32, 400)
    rs = np.random.RandomState(401)
    ta, tg, tp = rs.uniform(1, 2, 6), rs.uniform(0, 100, 6), rs.uniform(0, 0.9, 6)
    want_d = np.array(elfi_amd.cdist_rows(X, y[None, :], 'euclidean', w=w))
    want_s = np.array(elfi_amd.toad_summaries(ta, tg, tp, n_toads=20, n_days=15, seed=3))
    Xb, yb, wb = X.copy(), y[None, :].copy(), w.copy()
    tb = [ta.copy(), tg.copy(), tp.copy()]
    with SO.adopted_stream(hip_ctx) as s:
        SO.busy(s)
        got_d = elfi_amd.cdist_rows(Xb, yb, 'euclidean', w=wb)
        for a in (Xb, yb, wb):
            a[...] = np.nan
        got_d = np.array(got_d)
        SO.busy(s)
        got_s = elfi_amd.toad_summaries(*tb, n_toads=20, n_days=15, seed=3)
        for a in tb:
            a[...] = np.nan
        got_s = np.array(got_s)
    assert np.array_equal(got_d, want_d) and not np.isnan(got_d).any()
    assert np.array_equal(got_s.view(np.int64), want_s.view(np.int64))
