"""The device-pointer (`_dev`) row entry points at the caller's pitch and alignment (include/elfihip.h: the `_dev`
layout contract), against the same oracles and tolerances as the host-form tests.

The host forms stage every matrix into a packed, 16-byte aligned buffer before a kernel sees it, so the tests that hand
them NumPy views exercise the staging copy.  Here the kernels themselves read rows at `ldx > m`, at an odd pitch, from an
8-byte aligned base: the layouts of tests/device_layout.py, each surrounded by NaN, the results surrounded by sentinels.
For every entry point the result in a layout must also equal the packed layout's bit for bit whenever both take the same
kernel: the pitch must not change the arithmetic.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.spatial.distance as ssd

import distance_oracle as O
from device_layout import LAYOUTS, guarded_out, place, place_rows_only, to_device, vec2
from test_adaptive_gpu import _best_ref as best_nested_ref
from test_adaptive_gpu import _check_stats, _nested_ref
from test_distance_gpu import _check as check_classic
from test_distance_gpu import _fold_and_check
from test_distance_metrics_gpu import check as check_new

pytestmark = pytest.mark.gpu

NS = (1, 63, 65, 4099)     # below one tile, across one tile, ragged over many tiles (tiles of 32 / 64 / 128 / 256 / 1024 rows)
IDS = {'euclidean': 0, 'sqeuclidean': 1, 'cityblock': 2, 'chebyshev': 3, 'minkowski': 4, 'seuclidean': 5, 'mahalanobis': 6,
       'canberra': 7, 'braycurtis': 8, 'cosine': 9, 'correlation': 10}
EXACT = ('euclidean', 'sqeuclidean', 'cityblock', 'chebyshev')
CLASSIC = EXACT + ('minkowski', 'seuclidean', 'mahalanobis')


def _sync_in():
    import torch
    torch.cuda.synchronize()     # (torch's stream and the context's own stream are not ordered against each other)


def _data(n, m, seed):
    rs = np.random.RandomState(seed)
    X = rs.randn(n, m) * rs.uniform(0.5, 3, m) + rs.uniform(-1, 1, m)
    y = rs.randn(1, m)
    w = rs.uniform(0.1, 2, m)
    return X, y, w


def _vi(m, rs):
    """A proper inverse covariance with negative off-diagonal entries, symmetrised (test_mahalanobis_shapes_vs_oracle)."""
    Z = rs.randn(4 * m + 5, m) @ rs.randn(m, m)
    VI = np.linalg.inv(np.cov(Z.T).reshape(m, m) + 0.1 * np.eye(m))
    return 0.5 * (VI + VI.T)


def _reference(X, y, metric, kw):
    if metric in CLASSIC:
        return O.cdist_rows(X, y, metric, **kw)
    with np.errstate(all='ignore'):
        return ssd.cdist(X, y, metric, **kw)[:, 0]


def _check(got, ref, metric, m, kw, what):
    """The project's own tolerance per metric and width (test_distance_gpu._check,
    test_distance_metrics_gpu.check, test_wide_rows_fallback)."""
    if metric not in CLASSIC:
        return check_new(got, ref, metric, m, kw.get('w'), what)
    if m > 299 and metric in EXACT:      # one wavefront per row, butterfly sums; a maximum has no order
        assert got.shape == ref.shape, what
        return np.testing.assert_allclose(got, ref, rtol=0 if metric == 'chebyshev' else 1e-14, atol=0, err_msg=what)
    return check_classic(got, ref, metric in EXACT, '%s %s' % (metric, what))


def _aux(kw):
    """The metric's vector or matrix argument (w, V or VI) on the device; None without one."""
    for key in ('w', 'V', 'VI'):
        if key in kw:
            return to_device(kw[key])
    return None


def _dist_rows(ctx, metric, ptr, n, m, ldx, dy, daux, p=2.0, out_off=0):
    out = guarded_out(n, 1, out_off)
    _sync_in()
    ctx.call('elfihip_dist_rows_dev', IDS[metric], ptr, n, m, ldx, dy.data_ptr(), daux.data_ptr() if daux is not None else None,
             C.c_double(p), out.ptr)
    ctx.synchronize()
    return out.check()


def _forms(m, layout):
    """The two values of elfihip_dist_set_form differ where rows arrive by 16-byte loads: the narrow and the LDS-DMA
    forms against the tile kernels, non-temporal against plain loads in the pipelined kernels (m <= 128)."""
    return (0, 1) if vec2(m, layout) and m <= 128 else (0,)


def _kernel_group(m, layout):
    """Layouts with the same value take the same kernel: rows wider than 299 all take the wide kernel, otherwise the
    16-byte-load kernels and the 8-byte-load kernels."""
    return 'wide' if m > 299 else vec2(m, layout)


M_ALL = [2, 4, 6, 16, 32, 64, 48, 100, 130, 298, 300, 5, 33]      # narrow, pipelined, DMA x 3, pipelined, vec2 tile, wide, odd
M_MORE = (4, 32, 33, 64, 100)


@pytest.mark.parametrize('m', M_ALL)
def test_dist_rows_dev_every_layout(hip_ctx, m):
    try:
        for n in NS:
            X, y, w = _data(n, m, 100 * m + n)
            rs = np.random.RandomState(m + n)
            cases = [('euclidean', {}), ('euclidean', dict(w=w)), ('cityblock', dict(w=w)), ('chebyshev', {}),
                     ('sqeuclidean', {}), ('canberra', {})]
            if m in M_MORE:
                cases += [('minkowski', dict(p=3.0)), ('seuclidean', dict(V=w)), ('cosine', dict(w=w)), ('correlation', {}),
                          ('braycurtis', {}), ('mahalanobis', dict(VI=_vi(m, rs)))]
            refs = [_reference(X, y, metric, kw) for metric, kw in cases]
            dy = to_device(y)
            auxs = [_aux(kw) for _, kw in cases]
            first = {}
            for layout in LAYOUTS:
                pad, off = layout
                buf, ptr = place(X, m + pad, off)
                for form in _forms(m, layout):
                    hip_ctx.call('elfihip_dist_set_form', form)
                    for ci, (metric, kw) in enumerate(cases):
                        what = '%s n=%d m=%d layout=%s form=%d' % (sorted(kw), n, m, layout, form)
                        got = _dist_rows(hip_ctx, metric, ptr, n, m, m + pad, dy, auxs[ci], kw.get('p', 2.0))
                        _check(got, refs[ci], metric, m, kw, what)
                        base = first.setdefault((ci, form, _kernel_group(m, layout)), got)
                        assert np.array_equal(base, got, equal_nan=True), 'the pitch changed the arithmetic: ' + metric + what
                hip_ctx.call('elfihip_dist_set_form', 0)
                del buf
    finally:
        hip_ctx.call('elfihip_dist_set_form', 0)


@pytest.mark.parametrize('m', [2, 4, 32, 33, 130])
def test_dist_multiw_dev_every_layout(hip_ctx, m):
    """K weighted euclidean distances per row, out (n, K): the narrow form (K <= 8) writes whole 16-byte pieces when
    `dout` is 16-byte aligned and single results otherwise -- both are run, the sentinels around `dout` stay."""
    try:
        for n in NS:
            X, y, _ = _data(n, m, 7 * m + n)
            rs = np.random.RandomState(n)
            Wall = np.vstack([np.ones(m), rs.uniform(0.2, 2, (8, m))])
            dy = to_device(y)
            for K in (1, 3, 8, 9):
                W = Wall[:K]
                ref = _nested_ref(X, y, W)
                dW = to_device(W)
                for layout in LAYOUTS:
                    pad, off = layout
                    buf, ptr = place(X, m + pad, off)
                    for form in _forms(m, layout):
                        hip_ctx.call('elfihip_dist_set_form', form)
                        for out_off in (0, 1):
                            out = guarded_out(n, K, out_off)
                            _sync_in()
                            hip_ctx.call('elfihip_dist_multiw_dev', ptr, n, m, m + pad, dy.data_ptr(), dW.data_ptr(), K, out.ptr)
                            hip_ctx.synchronize()
                            got = out.check().reshape(n, K)
                            assert np.array_equal(got, ref), (n, m, K, layout, form, out_off)
                    hip_ctx.call('elfihip_dist_set_form', 0)
    finally:
        hip_ctx.call('elfihip_dist_set_form', 0)


class _State:
    """An elfihip_reject through the C ABI."""

    def __init__(self, ctx, k):
        self.ctx, self.k, self.h = ctx, k, C.c_void_p()
        ctx.call('elfihip_reject_create', k, C.byref(self.h))

    def result(self):
        from elfi_amd import _lib
        vals, rows, cnt = np.empty(self.k), np.empty(self.k, dtype=np.int64), C.c_int64()
        assert self.ctx.lib.elfihip_reject_result(self.h, _lib.ptr(vals), _lib.ptr(rows), C.byref(cnt)) == 0
        return vals[:cnt.value], rows[:cnt.value]

    def close(self):
        self.ctx.lib.elfihip_reject_free(self.h)


@pytest.mark.parametrize('multiw', [False, True])
@pytest.mark.parametrize('m', [4, 32, 33])
def test_reject_push_dev_reads_pitched_rows(hip_ctx, m, multiw):
    """The fused filter and the in-pass merge of the sealed list (m = 32: the LDS-DMA row form) on pitched rows: after
    every push the distances are the oracle's and the state is the k best of everything pushed, ties to the earlier row."""
    k, K = 300, 3
    lib = hip_ctx.lib
    rs = np.random.RandomState(31 * m + multiw)
    y, w = rs.randn(1, m), rs.uniform(0.1, 3, m)
    W = np.vstack([np.ones(m), rs.uniform(0.2, 2, (K - 2, m)), w])
    dy, dw, dW = to_device(y), to_device(w), to_device(W)
    batches = [rs.randn(n, m) for n in (100, 150, 4000, 70001)]
    refs = [O.cdist_rows(X, y, 'euclidean', w=w) for X in batches]
    for layout in [(0, 0), (6, 2), (1, 0)]:
        pad, off = layout
        st = _State(hip_ctx, k)
        try:
            base = 0
            for b, X in enumerate(batches):
                n = len(X)
                buf, ptr = place(X, m + pad, off)
                out = guarded_out(n, K if multiw else 1)
                _sync_in()
                if multiw:
                    assert lib.elfihip_reject_push_multiw_dev(st.h, ptr, n, m, m + pad, dy.data_ptr(), dW.data_ptr(), K,
                                                              out.ptr, base) == 0
                else:
                    assert lib.elfihip_reject_push_rows_dev(st.h, 0, ptr, n, m, m + pad, dy.data_ptr(), dw.data_ptr(),
                                                            C.c_double(2.0), out.ptr, base) == 0
                hip_ctx.synchronize()
                got = out.check()
                assert np.array_equal(got[:, K - 1] if multiw else got, refs[b]), (layout, b)
                if multiw:
                    assert np.array_equal(got[:, 0], O.cdist_rows(X, y, 'euclidean')), (layout, b)
                base += n
                allv = np.concatenate(refs[:b + 1])
                order = np.lexsort((np.arange(len(allv)), allv))[:k]
                vals, rows = st.result()
                assert np.array_equal(vals, allv[order]) and np.array_equal(rows, order), (layout, b)
        finally:
            st.close()


def _adaptive_push(ctx, X, layout, y, W, k, row_base):
    """One batch through elfihip_adaptive_push_dev in a layout, into an empty state of k rows and a zero store ->
    (nested distances, (vals, rows) of the state, the store's 1 + 2m doubles)."""
    n, m = X.shape
    K = len(W)
    pad, off = layout
    dy, dW = to_device(y), to_device(W)
    buf, ptr = place(X, m + pad, off)
    out = guarded_out(n, K)
    wel = to_device(np.zeros(1 + 2 * m))
    st = _State(ctx, k)
    try:
        _sync_in()
        ctx.call('elfihip_adaptive_push_dev', st.h, ptr, n, m, m + pad, dy.data_ptr(), dW.data_ptr(), K, out.ptr,
                 wel.data_ptr(), row_base)
        best = st.result()
        ctx.synchronize()
    finally:
        st.close()
    return out.check().reshape(n, K), best, wel.cpu().numpy()


def _welford_dev(ctx, X, layout):
    """elfihip_welford_update_dev on the same rows in the same layout, from a zero store."""
    n, m = X.shape
    buf, ptr = place(X, m + layout[0], layout[1])
    st = to_device(np.zeros(1 + 2 * m))
    _sync_in()
    ctx.call('elfihip_welford_update_dev', ptr, n, m, m + layout[0], st.data_ptr())
    ctx.synchronize()
    return st.cpu().numpy()


@pytest.mark.parametrize('m', [2, 4, 6, 32, 64, 128])
def test_adaptive_push_dev_fused_and_fallback_layouts(hip_ctx, m):
    """Layouts (0, 0) and (6, 2) take the fused pass (adaptive_pass_supported: m and ldx even, 16-byte aligned rows),
    (1, 0) and (0, 1) the separate passes.  Nested distances bit-identical to cdist and the running best exact either way.

    Column statistics, fused layouts: test_adaptive_gpu's a-priori bounds on its own hard data (|mean| up to 10^4 spreads),
    and the same bits at both pitches.  Fallback layouts: the store must be, bit for bit, what elfihip_welford_update_dev
    leaves for the same rows in the same layout -- that IS the separate pass, and test_welford_update_dev_every_layout holds
    it to test_welford_vs_oracle's bounds.  test_adaptive_gpu's bound for the fallback shapes (2e-13 of sum |x (x - mean)|
    against the exact M2) is checked on columns where it can hold: the two-pass form follows the reference's formula,
    whose first batch gives M2 - delta N mean for a mean off by delta, and a mean rounded to binary64 is off by up to half
    an ulp however it is summed, so no implementation of that formula meets the bound once the spread is below about
    1e-3 |mean|; the bound on the mean itself (64 ulp) implies the bound on M2 only from a spread of 0.036 |mean| on.  The
    fallback layouts therefore also run columns with |mean| <= 10 standard deviations, where both bounds are consistent.
    (On the hard columns the two-pass store misses it as the arithmetic says: n = 4099, m = 64, mean 946, spread 0.08:
    6.9e-7 off against a bound of 1.0e-7, i.e. 1.5 ulp of the mean.)"""
    K, k = 3, 50
    for n in NS:
        rs = np.random.RandomState(1000 * m + n)
        scale = rs.uniform(0.1, 100, m)
        X = rs.randn(n, m) * scale + rs.uniform(-1000, 1000, m)
        Xc = rs.randn(n, m) * scale + rs.uniform(-10, 10, m) * scale      # |mean| <= 10 standard deviations
        y = rs.randn(1, m)
        W = np.vstack([np.ones(m)] + [rs.uniform(0.01, 4, m) for _ in range(K - 1)])
        ref = _nested_ref(X, y, W)
        rv, rr, _ = best_nested_ref(ref, k, base=5 * n)
        fused_first = None
        for layout in [(0, 0), (6, 2), (1, 0), (0, 1)]:
            fused = vec2(m, layout)
            got, (vals, rows), s = _adaptive_push(hip_ctx, X, layout, y, W, k, 5 * n)
            assert np.array_equal(got, ref), (n, m, layout)
            assert np.array_equal(vals, rv) and np.array_equal(rows, rr), (n, m, layout)
            if fused:
                if n > 1:
                    _check_stats((int(s[0]), s[1:1 + m], s[1 + m:]), X, fused=True)
                else:
                    assert s[0] == 1 and np.array_equal(s[1:1 + m], X[0]) and np.all(s[1 + m:] == 0)
                fused_first = s if fused_first is None else fused_first
                assert np.array_equal(s, fused_first), ('fused statistics depend on the pitch', n, m, layout)
            else:
                assert np.array_equal(s, _welford_dev(hip_ctx, X, layout)), ('not the separate pass', n, m, layout)
                gc, _, sc = _adaptive_push(hip_ctx, Xc, layout, y, W, k, 0)
                assert np.array_equal(gc, _nested_ref(Xc, y, W)), (n, m, layout)
                assert np.array_equal(sc, _welford_dev(hip_ctx, Xc, layout)), (n, m, layout)
                if n > 1:
                    _check_stats((int(sc[0]), sc[1:1 + m], sc[1 + m:]), Xc, fused=False)


@pytest.mark.parametrize('L', [7, 100, 128, 130])
def test_row_summary_dev_every_layout(hip_ctx, L):
    for n in NS:
        rs = np.random.RandomState(n + L)
        x = rs.randn(n, L) * rs.uniform(0.1, 50, L) + rs.uniform(-3, 3, L)
        lag7 = min(7, L - 1)
        refs = [(0, 0, O.ss_mean(x)), (1, 0, O.ss_var(x)), (2, 1, O.autocov(x, 1)), (2, lag7, O.autocov(x, lag7))]
        for layout in LAYOUTS:
            pad, off = layout
            buf, ptr = place(x, L + pad, off)
            for kind, lag, ref in refs:
                for out_off in (0, 1):
                    out = guarded_out(n, 1, out_off)
                    _sync_in()
                    hip_ctx.call('elfihip_row_summary_dev', kind, ptr, n, L, L + pad, lag, out.ptr)
                    hip_ctx.synchronize()
                    assert np.array_equal(out.check(), ref), (n, L, kind, lag, layout)


# 129 observations are the first the eight-lanes-per-row form of the fused MA2 kernel does not take (its in-place x covers
# 128): one more width than the four of the summaries
@pytest.mark.parametrize('n_obs', [37, 100, 126, 129, 200])
def test_ma2_distance_dev_every_layout(hip_ctx, n_obs):
    L = n_obs + 2
    for n in NS:
        rs = np.random.RandomState(n_obs + n)
        t1, t2 = rs.uniform(-2, 2, n), rs.uniform(-1, 1, n)
        w = rs.randn(n, L)
        x = w[:, 2:] + t1[:, None] * w[:, 1:-1] + t2[:, None] * w[:, :-2]      # elfi/examples/ma2.py:35
        S1, S2 = O.autocov(x), O.autocov(x, 2)
        obs = (np.array([0.3]), np.array([0.1]))
        d = O.make_distance('euclidean')(S1, S2, observed=obs)
        dt1, dt2 = to_device(t1), to_device(t2)
        for layout in LAYOUTS:
            pad, off = layout
            buf, ptr = place(w, L + pad, off)
            outs = [guarded_out(n) for _ in range(3)]
            _sync_in()
            hip_ctx.call('elfihip_ma2_distance_dev', ptr, n, n_obs, L + pad, dt1.data_ptr(), dt2.data_ptr(), C.c_double(0.3),
                         C.c_double(0.1), outs[0].ptr, outs[1].ptr, outs[2].ptr)
            hip_ctx.synchronize()
            for o, ref, name in zip(outs, (S1, S2, d), ('S1', 'S2', 'distance')):
                assert np.array_equal(o.check(), ref), (name, n, n_obs, layout)


@pytest.mark.parametrize('m', [1, 33, 64, 300])
def test_welford_update_dev_every_layout(hip_ctx, m, monkeypatch):
    """test_welford_vs_oracle's fold -- its reference, its a-priori tolerances -- with every batch read by the device form
    in the given layout; the summation order is fixed by the launch shape, so every layout gives the packed layout's bits."""
    import elfi_amd
    states = {}
    for n in NS:
        for layout in LAYOUTS:
            pad, off = layout

            def update(X, cnt, mean, M2):
                buf, ptr = place(X, m + pad, off)
                st = to_device(np.concatenate([[float(cnt)], mean, M2]))
                _sync_in()
                hip_ctx.call('elfihip_welford_update_dev', ptr, len(X), m, m + pad, st.data_ptr())
                hip_ctx.synchronize()
                s = st.cpu().numpy()
                return int(s[0]), s[1:1 + m].copy(), s[1 + m:].copy()

            monkeypatch.setattr(elfi_amd, 'welford_update', update)
            rs = np.random.RandomState(n + m)
            batches = [rs.randn(n, m) * rs.uniform(0.1, 100, m) + rs.uniform(-1000, 1000, m) for _ in range(3)]
            cnt, mean, M2 = _fold_and_check(batches, m)
            base = states.setdefault(n, (mean, M2))
            assert cnt == 3 * n and np.array_equal(mean, base[0]) and np.array_equal(M2, base[1]), (n, m, layout)


@pytest.mark.parametrize('m', [1, 33, 64, 300])
def test_weighted_var_dev_every_layout(hip_ctx, m):
    """elfi/methods/utils.py:108-139 against the oracle at test_weighted.py's tolerance (1e-12: the summation order
    only), with and without weights; the order is fixed, so every layout gives the packed layout's bits."""
    import weighted_oracle as WO
    for n in (2, 63, 65, 4099):
        rs = np.random.RandomState(3 * n + m)
        x = rs.randn(n, m) * rs.uniform(0.1, 50, m) + rs.uniform(-3, 3, m)
        wts = rs.gamma(0.5, 1.0, n) + 1e-3
        for w in (None, wts):
            ref = np.atleast_1d(np.asarray(WO.weighted_var(x, w)))
            dw = to_device(w) if w is not None else None
            first = None
            for layout in LAYOUTS:
                pad, off = layout
                buf, ptr = place(x, m + pad, off)
                out = guarded_out(m)
                _sync_in()
                hip_ctx.call('elfihip_weighted_var_dev', ptr, n, m, m + pad, dw.data_ptr() if w is not None else None, out.ptr)
                hip_ctx.synchronize()
                got = out.check()
                np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0, err_msg=str((n, m, layout, w is not None)))
                first = got if first is None else first
                assert np.array_equal(got, first), (n, m, layout)


@pytest.mark.parametrize('m', [2, 5, 32])
def test_dist_cols_dev_pitch_and_alignment(hip_ctx, m):
    """Column-major device matrix: the two-rows-per-lane path needs ldc even and 16-byte aligned columns AND results
    (make_col_args); every combination of the three gives the row-major oracle's bits for the exact metrics."""
    for n in NS:
        X, y, w = _data(n, m, 9 * m + n)
        cases = [('euclidean', None), ('euclidean', w), ('sqeuclidean', w), ('cityblock', w), ('chebyshev', None),
                 ('canberra', None), ('braycurtis', w)]
        refs = [_reference(X, y, metric, {} if ww is None else {'w': ww}) for metric, ww in cases]
        dy, dw = to_device(y), to_device(w)
        for ldc in (n, n + 1, n + 6):
            for off in (0, 1):
                buf, ptr = place(X.T, ldc, off)
                for out_off in (0, 1):
                    for (metric, ww), ref in zip(cases, refs):
                        out = guarded_out(n, 1, out_off)
                        _sync_in()
                        hip_ctx.call('elfihip_dist_cols_dev', IDS[metric], ptr, n, m, ldc, dy.data_ptr(),
                                     dw.data_ptr() if ww is not None else None, C.c_double(2.0), out.ptr)
                        hip_ctx.synchronize()
                        np.testing.assert_array_equal(out.check(), ref, err_msg=str((metric, n, m, ldc, off, out_off)))


def test_misaligned_results_of_the_row_entry_points(hip_ctx):
    """include/elfihip.h: `dout` needs 8-byte alignment only.  The kernels that write results in 16-byte pieces (the
    narrow K-weight forms, through wave_store_rows) test `dout` themselves and store single results otherwise; the
    fused adaptive pass on narrow rows is the second of them (the K-weight entry point is covered above)."""
    n, m, K = 4099, 4, 3
    X, y, _ = _data(n, m, 5)
    W = np.vstack([np.ones(m), np.random.RandomState(1).uniform(0.2, 2, (K - 1, m))])
    ref = _nested_ref(X, y, W)
    dy, dW = to_device(y), to_device(W)
    buf, ptr = place(X, m, 0)
    for out_off in (0, 1):
        out = guarded_out(n, K, out_off)
        _sync_in()
        hip_ctx.call('elfihip_adaptive_push_dev', None, ptr, n, m, m, dy.data_ptr(), dW.data_ptr(), K, out.ptr, None, 0)
        hip_ctx.synchronize()
        assert np.array_equal(out.check().reshape(n, K), ref), out_off


def _limit_case(hip_ctx, ldx):
    """65 rows of 32 summaries at pitch ldx (only the rows are written): euclidean and mahalanobis against the oracle."""
    import torch
    n, m = 65, 32
    X, y, _ = _data(n, m, 77)
    VI = _vi(m, np.random.RandomState(78))
    dy, dvi = to_device(y), to_device(VI)
    buf, ptr = place_rows_only(X, ldx, 0)
    try:
        e = _dist_rows(hip_ctx, 'euclidean', ptr, n, m, ldx, dy, None)
        mah = _dist_rows(hip_ctx, 'mahalanobis', ptr, n, m, ldx, dy, dvi)
    finally:
        del buf
        torch.cuda.empty_cache()
    assert np.array_equal(e, O.cdist_rows(X, y, 'euclidean')), ldx
    np.testing.assert_allclose(mah, O.cdist_rows(X, y, 'mahalanobis', VI=VI), rtol=1e-13, atol=0, err_msg=str(ldx))
    return e, mah


def test_lds_dma_pitch_limit_both_sides(hip_ctx):
    """The LDS-DMA row form addresses a slot's rows with 32-bit byte offsets and is taken up to ldx = 2^21 (launch_rows);
    one pitch further the register-staged pipeline runs: the same bits on both sides."""
    e_on, _ = _limit_case(hip_ctx, 1 << 21)
    e_off, _ = _limit_case(hip_ctx, (1 << 21) + 2)
    assert np.array_equal(e_on, e_off)


def test_matrix_core_mahalanobis_pitch_limit_both_sides(hip_ctx):
    """The split Mahalanobis kernel forms row addresses in 32 bits and is taken below ldx = 2^22 (launch_mahalanobis);
    from there on the LDS-operand form with 64-bit addresses runs."""
    _limit_case(hip_ctx, (1 << 22) - 2)
    _limit_case(hip_ctx, 1 << 22)
