"""GPU: the regression adjustment kernels (csrc/adjust.hip) through the C ABI and the Python side (elfi_amd/adjust.py).

Yardstick (tests/adjust_ref.py, tests/test_adjust.py): `truth`, the least-squares solution in 40-digit arithmetic; the
bound is 16 x the reference's largest own error over the recorded cases with the same m, never below 16 eps, in the
metrics |c - truth| / max_a |truth_a| (coefficients) and |a - truth| / (1 + |truth|) (adjusted values).
Measured errors are printed per case (pytest -s).  Recorded on one MI355X, in eps, coefficients / adjusted values:

    (n, m, q)        e_ref          device        bound
    (3, 1, 1)        0.0 / 0.1      0.9 / 0.8     16 / 16
    (66, 64, 2)      24 / 206       12 / 63       383 / 3298
    (255, 3, 1)      2.3 / 11       1.6 / 3.7     37 / 183
    (256, 2, 2)      0.6 / 2.7      0.7 / 3.7     16 / 105
    (257, 8, 3)      6.6 / 16       4.9 / 5.1     105 / 258
    (513, 2, 2)      0.9 / 6.6      3.3 / 12      16 / 105
    (1000, 33, 5)    10 / 180       3.0 / 44      159 / 2874
    (700, 16, 16)    8.0 / 91       3.5 / 27      128 / 1457

The recorded gauss run: 0.8 eps from the reference's adjusted mu (bound 105 eps).
"""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import adjust_ref as R
import device_layout as L
import ref_shim

pytestmark = pytest.mark.gpu
needs_reference = pytest.mark.skipif(not ref_shim.available(), reason='no reference package (run oracle/make_ref.sh)')

ERR_ARG = 1
PARTS = ('coef', 'intercept', 'rss', 'status')


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'adjust.npz'))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def all_same(got, want):
    """(adjusted, parts) pairs, bit for bit (NaN included)."""
    return same_bits(got[0], want[0]) and all(same_bits(got[1][k], want[1][k]) for k in PARTS)


@pytest.mark.parametrize('ci', range(len(R.CASES)))
def test_yardstick_and_identities(gold, ci):
    import elfi_amd
    seed, n, m, q, kind = R.CASES[ci]
    X, Y = R.make_case(ci)
    adj, parts = elfi_amd.linear_adjust(X, Y, return_parts=True)
    coef, icpt, rss = parts['coef'], parts['intercept'], parts['rss']
    assert adj.shape == (n, q) and coef.shape == (q, m) and icpt.shape == rss.shape == (q,) and parts['status'] == 0
    same = R.same_m(m)
    b_coef, b_adj = R.bound(gold['e_coef'][same]), R.bound(gold['e_adj'][same])
    e_coef, e_adj = R.coef_error(coef, gold['truth_coef_%d' % ci]), R.adjusted_error(adj, gold['truth_adj_%d' % ci])
    print('case %d (%d, %d, %d) %-10s in eps: coefficients e_ref %.1f device %.1f bound %.1f | adjusted e_ref %.1f device '
          '%.1f bound %.1f' % (ci, n, m, q, kind, gold['e_coef'][ci] / R.EPS, e_coef / R.EPS, b_coef / R.EPS,
                               gold['e_adj'][ci] / R.EPS, e_adj / R.EPS, b_adj / R.EPS))
    assert e_coef <= b_coef and e_adj <= b_adj
    # the adjusted values are Y - X @ coef.T from the returned coefficients: one dot product's rounding on each side
    again = Y - X @ coef.T
    assert np.all(np.abs(adj - again) <= 4 * (m + 2) * R.EPS * (1 + np.abs(again)))
    # intercept = ybar - xbar.coef: the bound, on the scale of the terms of that sum
    xb, yb = X.mean(axis=0), Y.mean(axis=0)
    assert np.all(np.abs(icpt - (yb - coef @ xb)) <= b_adj * (1 + np.abs(yb) + np.abs(coef) @ np.abs(xb)))
    # rss = the sum of squared residuals (centred form: the residuals do not carry the columns' offsets); a backward error
    # of the factorisation moves it by the bound on the scale of the response's own sum of squares
    res = (Y - yb) - (X - xb) @ coef.T
    tss = np.sum((Y - yb) ** 2, axis=0)
    assert np.all(np.abs(rss - np.sum(res * res, axis=0)) <= b_adj * tss)
    assert np.all(rss >= 0) and np.all(rss <= tss * (1 + b_adj))


def test_a_groups_outputs_do_not_depend_on_the_call(gold):
    import elfi_amd
    X0, Y0 = R.make_case(5)                                   # (513, 2, 2): two tiles plus one row
    rs = np.random.RandomState(31)
    Xg = np.stack([X0, X0 * [3.0, 0.25] + rs.randn(*X0.shape), rs.randn(*X0.shape) - 2.0])
    Yg = np.stack([Y0, Y0 + 0.5 * rs.randn(*Y0.shape), rs.randn(*Y0.shape)])
    adj, parts = elfi_amd.linear_adjust(Xg, Yg, return_parts=True)
    assert adj.shape == (3, 513, 2) and parts['coef'].shape == (3, 2, 2) and parts['status'].shape == (3,)
    flat = elfi_amd.linear_adjust(Xg.reshape(-1, 2), Yg.reshape(-1, 2), n_groups=3, return_parts=True)
    assert all_same(flat, (adj, parts))
    for g in range(3):
        alone = elfi_amd.linear_adjust(Xg[g], Yg[g], return_parts=True)
        assert all_same(alone, (adj[g], {k: parts[k][g] for k in PARTS})), g
        assert alone[1]['status'] == 0


@pytest.mark.parametrize('ci', [5, 6])
def test_a_prefix_has_the_bits_of_a_group_of_that_many_rows(ci):
    import elfi_amd
    seed, n, m, q, kind = R.CASES[ci]
    X, Y = R.make_case(ci)
    prefixes = [m + 2, 256, 300, n]
    adj, parts = elfi_amd.linear_adjust(X, Y, prefixes=prefixes, return_parts=True)
    assert adj.shape == (4, n, q) and parts['coef'].shape == (4, q, m) and parts['status'].shape == (4,)
    assert np.all(parts['status'] == 0)
    for k, p in enumerate(prefixes):
        alone = elfi_amd.linear_adjust(X[:p], Y[:p], return_parts=True)
        assert same_bits(adj[k, :p], alone[0]), p
        assert np.all(np.isnan(adj[k, p:]))
        assert all(same_bits(parts[key][k], alone[1][key]) for key in PARTS), p
    # ... and with groups: job (g, k) is group g's prefix k
    G2 = elfi_amd.linear_adjust(np.stack([X, X[::-1]]), np.stack([Y, Y[::-1]]), prefixes=prefixes, return_parts=True)
    assert G2[0].shape == (2, 4, n, q) and same_bits(G2[0][0], adj) and same_bits(G2[1]['coef'][0], parts['coef'])
    back = elfi_amd.linear_adjust(X[::-1][:300], Y[::-1][:300])
    assert same_bits(G2[0][1, 2, :300], back)


# m + q = 40 is the widest shape with tiles of 256 rows, 41 the first with tiles of 128; (64, 16) is the widest of all: its
# pair of stacked triangles is the largest LDS request.  300 rows are 2 tiles of 256 or 3 of 128.
@pytest.mark.parametrize('m,q', [(30, 10), (31, 10), (64, 16)])
def test_both_tile_heights_and_the_widest_shape(m, q):
    import elfi_amd
    n = 300
    rs = np.random.RandomState(100 * m + q)
    X = rs.randn(n, m) * rs.uniform(0.5, 2.0, m) + rs.randn(m)
    Y = X[:, :q] + 0.5 * rs.randn(n, q)
    prefixes = [130, n]
    adj, parts = elfi_amd.linear_adjust(X, Y, prefixes=prefixes, return_parts=True)
    assert np.all(parts['status'] == 0)
    for k, p in enumerate(prefixes):
        alone = elfi_amd.linear_adjust(X[:p], Y[:p], return_parts=True)
        assert same_bits(adj[k, :p], alone[0]) and all(same_bits(parts[key][k], alone[1][key]) for key in PARTS)
        # the residual of a least-squares fit is orthogonal to every regressor: |x_j . r_t| is rounding on the scale
        # ||x_j|| ||y_t||.  Each of the m + q reflections rounds the columns once (a backward error of eps per column and
        # reflection), and the check itself (NumPy's residual and product) rounds as much again: 4 (m + q) eps with a
        # factor 2 to spare on each side
        Xc, Yc = X[:p] - X[:p].mean(axis=0), Y[:p] - Y[:p].mean(axis=0)
        B = parts['coef'][k]
        r = Yc - Xc @ B.T
        scale = np.linalg.norm(Xc, axis=0)[:, None] * np.linalg.norm(Yc, axis=0)[None, :]
        worst = np.max(np.abs(Xc.T @ r) / scale)
        print('m=%d q=%d p=%d: |x_j . r_t| at most %.1f eps ||x_j|| ||y_t|| (allowed %d)' % (m, q, p, worst / R.EPS, 4 * (m + q)))
        assert worst <= 4 * (m + q) * R.EPS
        again = Y[:p] - X[:p] @ B.T
        assert np.all(np.abs(adj[k, :p] - again) <= 4 * (m + 2) * R.EPS * (1 + np.abs(again)))
        assert np.all(np.abs(parts['rss'][k] - np.sum(r * r, axis=0)) <= 4 * (m + q) * R.EPS * np.sum(Yc * Yc, axis=0))


def int_out(count, fill=-77):
    import torch
    return torch.full((2 + count + 8,), fill, dtype=torch.int32, device='cuda')


@pytest.mark.parametrize('ci', [4, 5])
def test_host_and_dev_forms_agree_at_the_callers_pitch(hip_ctx, ci):
    import elfi_amd
    import torch
    seed, n, m, q, kind = R.CASES[ci]
    X, Y = R.make_case(ci)
    prefixes = np.array([m + 2, 256, n], dtype=np.int64)
    for pf in (None, prefixes):
        K = 0 if pf is None else len(pf)
        Ke = max(K, 1)
        adj, parts = elfi_amd.linear_adjust(X, Y, prefixes=pf, return_parts=True)
        for (padx, off), pady in zip(((0, 0), (3, 1), (2, 0)), (0, 2, 5)):
            dX, pX = L.place(X, m + padx, off)                    # the padding is NaN
            dY, pY = L.place(Y, q + pady, off)
            oA, oC = L.guarded_out(Ke * n * q, 1, off), L.guarded_out(Ke * q * m, 1, off)
            oI, oR = L.guarded_out(Ke * q), L.guarded_out(Ke * q, 1, off)
            dS = int_out(Ke)
            torch.cuda.synchronize()
            hip_ctx.call("elfihip_linear_adjust_dev", pX, 1, n, m, m + padx, pY, q, q + pady,
                         pf.ctypes.data if K else None, K, oA.ptr, oC.ptr, oI.ptr, oR.ptr, dS.data_ptr() + 8)
            hip_ctx.synchronize()
            hA = oA.t.cpu().numpy()[oA.start:oA.start + Ke * n * q]       # (NaN rows beyond a prefix: read past check())
            guard = np.float64(L.SENTINEL).view(np.int64)
            whole = oA.t.cpu().numpy().view(np.int64)
            assert np.all(whole[:oA.start] == guard) and np.all(whole[oA.start + Ke * n * q:] == guard)
            assert same_bits(hA.reshape(np.shape(adj)), adj)
            assert same_bits(oC.check().reshape(np.shape(parts['coef'])), parts['coef'])
            assert same_bits(oI.check().reshape(np.shape(parts['intercept'])), parts['intercept'])
            assert same_bits(oR.check().reshape(np.shape(parts['rss'])), parts['rss'])
            hS = dS.cpu().numpy()
            assert np.all(hS[:2] == -77) and np.all(hS[2 + Ke:] == -77) and np.all(hS[2:2 + Ke] == 0)
    # without the optional outputs
    dX, pX = L.place(X, m, 0)
    dY, pY = L.place(Y, q, 0)
    oA = L.guarded_out(n * q)
    torch.cuda.synchronize()
    hip_ctx.call("elfihip_linear_adjust_dev", pX, 1, n, m, m, pY, q, q, None, 0, oA.ptr, None, None, None, None)
    hip_ctx.synchronize()
    assert same_bits(oA.check().reshape(n, q), elfi_amd.linear_adjust(X, Y))
    # the host form at a pitch: rows cut out of wider arrays
    wide_x, wide_y = np.full((n, m + 3), np.nan), np.full((n, q + 1), np.nan)
    wide_x[:, :m], wide_y[:, :q] = X, Y
    out = np.empty((1, 1, n, q))
    hip_ctx.call("elfihip_linear_adjust", wide_x.ctypes.data, 1, n, m, m + 3, wide_y.ctypes.data, q, q + 1, None, 0,
                 out.ctypes.data, None, None, None, None)
    assert same_bits(out[0, 0], elfi_amd.linear_adjust(X, Y))


def test_rank_deficient_jobs_get_status_3_and_the_others_are_untouched():
    import elfi_amd
    rs = np.random.RandomState(41)
    n, m, q = 300, 4, 2
    Xg, Yg = rs.randn(5, n, m), rs.randn(5, n, q)
    Xg[1, :, 3] = Xg[1, :, 1]                 # a duplicated column
    Xg[2, :, 2] = 0.1                         # a constant column whose mean does not round to it
    Xg[3, :, 0] = 0.0                         # a constant column of zeros
    Xg[4] = Xg[4] * [1e-3, 1.0, 1e3, 1.0]     # scales alone are no dependency
    adj, parts = elfi_amd.linear_adjust(Xg, Yg, return_parts=True)
    assert list(parts['status']) == [0, 3, 3, 3, 0]
    for g in (1, 2, 3):
        assert np.all(np.isnan(adj[g])) and all(np.all(np.isnan(parts[k][g])) for k in ('coef', 'intercept', 'rss'))
    for g in (0, 4):
        alone = elfi_amd.linear_adjust(Xg[g], Yg[g], return_parts=True)
        assert all_same(alone, (adj[g], {k: parts[k][g] for k in PARTS})) and np.all(np.isfinite(adj[g]))
    # the scaled group has the unscaled group's adjustment: the fit does not depend on the columns' scales
    plain = elfi_amd.linear_adjust(Xg[4] / [1e-3, 1.0, 1e3, 1.0], Yg[4])
    assert np.all(np.abs(adj[4] - plain) <= 64 * R.EPS * (1 + np.abs(plain)))
    # p - 1 < m: that job alone
    adj, parts = elfi_amd.linear_adjust(Xg[0], Yg[0], prefixes=[m, m + 1, n], return_parts=True)
    assert list(parts['status']) == [3, 0, 0]
    assert np.all(np.isnan(adj[0])) and np.all(np.isnan(parts['coef'][0])) and np.all(np.isnan(parts['rss'][0]))
    assert np.all(np.isfinite(adj[1, :m + 1])) and np.all(np.isnan(adj[1, m + 1:]))
    assert same_bits(adj[2], elfi_amd.linear_adjust(Xg[0], Yg[0]))
    # m + 1 rows determine the fit: no residual is left
    assert np.all(parts['rss'][1] <= 256 * R.EPS * np.sum((Yg[0, :m + 1] - Yg[0, :m + 1].mean(axis=0)) ** 2, axis=0))


def test_a_non_finite_value_gives_status_2_in_its_group_alone():
    import elfi_amd
    rs = np.random.RandomState(43)
    n, m, q = 600, 3, 2
    Xg, Yg = rs.randn(4, n, m), rs.randn(4, n, q)
    Xg[1, 599, 2] = np.nan                    # in the last, partial tile
    Yg[2, 0, 1] = np.inf
    adj, parts = elfi_amd.linear_adjust(Xg, Yg, return_parts=True)
    assert list(parts['status']) == [0, 2, 2, 0]
    for g in (1, 2):
        assert np.all(np.isnan(adj[g])) and all(np.all(np.isnan(parts[k][g])) for k in ('coef', 'intercept', 'rss'))
    for g in (0, 3):
        assert all_same(elfi_amd.linear_adjust(Xg[g], Yg[g], return_parts=True), (adj[g], {k: parts[k][g] for k in PARTS}))
    # a prefix that ends before the value is not touched by it
    adj, parts = elfi_amd.linear_adjust(Xg[1], Yg[1], prefixes=[256, 599, 600], return_parts=True)
    assert list(parts['status']) == [0, 0, 2] and same_bits(adj[1, :599], elfi_amd.linear_adjust(Xg[1, :599], Yg[1, :599]))


def test_c_entry_points_refuse_bad_arguments_with_outputs_untouched(hip_ctx):
    rs = np.random.RandomState(2)
    X, Y = np.ascontiguousarray(rs.randn(40, 66)), np.ascontiguousarray(rs.randn(40, 18))
    out = np.full(4096, L.SENTINEL)
    st = np.full(16, -77, dtype=np.int32)
    lib, h = hip_ctx.lib, hip_ctx.handle
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)      # noqa: E731
    pre = lambda *v: np.array(v, dtype=np.int64)                        # noqa: E731
    bad = [dict(m=0), dict(m=65, ldx=65), dict(q=0), dict(q=17, ldy=17), dict(n=1), dict(ldx=2), dict(ldy=1), dict(G=0),
           dict(prefixes=pre(5, 9), K=2), dict(prefixes=pre(8, 5, 10), K=3), dict(prefixes=pre(1, 10), K=2),
           dict(prefixes=pre(5, 5, 10), K=3), dict(prefixes=pre(5, 10), K=0), dict(K=2), dict(adjusted=None)]
    for kw in bad:
        a = dict(G=1, n=10, m=3, ldx=3, q=2, ldy=2, prefixes=None, K=0, adjusted=out)
        a.update(kw)
        for name in ("elfihip_linear_adjust", "elfihip_linear_adjust_dev"):
            rc = getattr(lib, name)(h, p(X), a['G'], a['n'], a['m'], a['ldx'], p(Y), a['q'], a['ldy'], p(a['prefixes']),
                                    a['K'], p(a['adjusted']), p(out[1024:]), p(out[2048:]), p(out[3072:]), p(st))
            assert rc == ERR_ARG and lib.elfihip_last_error(h), (name, kw)
    for name in ("elfihip_linear_adjust", "elfihip_linear_adjust_dev"):
        assert getattr(lib, name)(h, None, 1, 10, 3, 3, p(Y), 2, 2, None, 0, p(out), None, None, None, None) == ERR_ARG
    hip_ctx.synchronize()
    assert np.all(out.view(np.int64) == np.float64(L.SENTINEL).view(np.int64)) and np.all(st == -77)


def test_recorded_gauss_run_through_the_batched_call(gold):
    import elfi_amd
    X = gold['gauss_summaries'] - gold['gauss_observed']
    b_adj = R.bound(gold['e_adj'][R.same_m(2)])
    adj = elfi_amd.linear_adjust(X, gold['gauss_mu'])
    assert adj.shape == (R.GAUSS_RUN['n_samples'], 1)
    e = R.adjusted_error(adj[:, 0], gold['gauss_ref_adjusted'])
    print('gauss run: device against the reference %.1f eps, against the truth %.1f eps, bound %.1f eps'
          % (e / R.EPS, R.adjusted_error(adj[:, 0], gold['gauss_truth_adjusted']) / R.EPS, b_adj / R.EPS))
    assert e <= b_adj and R.adjusted_error(adj[:, 0], gold['gauss_truth_adjusted']) <= b_adj


@needs_reference
def test_adjust_posterior_reproduces_the_recorded_gauss_run(gold):
    import elfi_amd
    ref_shim.install()
    from elfi.methods import post_processing as mod
    names = list(R.GAUSS_RUN['summaries'])
    b_adj = R.bound(gold['e_adj'][R.same_m(2)])
    sample, model = R.gauss_sample(mod, gold)
    for adjustment in ('linear', elfi_amd.HipLinearAdjustment()):
        res = elfi_amd.adjust_posterior(sample, model, names, ['mu'], adjustment)
        assert isinstance(res, mod.results.Sample) and res.method_name == 'LinearAdjustment'
        assert res.parameter_names == ['mu'] and list(res.outputs) == ['mu']
        assert R.adjusted_error(res.outputs['mu'], gold['gauss_ref_adjusted']) <= b_adj
    fitted = elfi_amd.HipLinearAdjustment()
    fitted.fit(sample, model, names)                               # parameter_names from the sample
    assert fitted.parameter_names == ['mu'] and fitted.X.shape == (500, 2)
    mdl = fitted.regression_models[0]
    ref = mod.LinearAdjustment()
    ref.fit(sample, model, names)
    want = ref.regression_models[0]
    b_coef = R.bound(gold['e_coef'][R.same_m(2)])
    assert R.coef_error(mdl.coef_, want.coef_) <= b_coef and abs(mdl.intercept_ - want.intercept_) <= b_adj * (1 + abs(want.intercept_))
    assert same_bits(fitted.adjust().outputs['mu'], res.outputs['mu'])


@needs_reference
def test_nested_thresholds_equal_the_single_threshold_calls(gold):
    import elfi_amd
    ref_shim.install()
    from elfi.methods import post_processing as mod
    names = list(R.GAUSS_RUN['summaries'])
    rs = np.random.RandomState(3)
    shuffled = rs.permutation(500)                                  # the rows are ordered by discrepancy, whatever their order
    sample, model = R.gauss_sample(mod, gold, shuffled)
    counts = [100, 250, 500]
    nested = elfi_amd.adjust_posterior(sample, model, names, ['mu'], n_closest=counts)
    assert isinstance(nested, list) and len(nested) == 3
    for res, c in zip(nested, counts):
        closest, _ = R.gauss_sample(mod, gold, np.arange(c))
        single = elfi_amd.adjust_posterior(closest, model, names, ['mu'])
        assert isinstance(res, mod.results.Sample) and res.method_name == 'LinearAdjustment'
        assert res.outputs['mu'].shape == (c,) and same_bits(res.outputs['mu'], single.outputs['mu'])


@needs_reference
def test_adjust_posterior_after_hip_rejection_on_the_gauss_model(gold):
    import elfi_amd
    ref_shim.install()
    from elfi.examples import gauss
    from elfi.methods import post_processing as mod
    run = R.GAUSS_RUN
    names = list(run['summaries'])
    m = gauss.get_model(seed_obs=run['seed_obs'])
    res = elfi_amd.HipRejection(m['d'], output_names=names, batch_size=10000, seed=run['seed']).sample(500, bar=False)
    got = elfi_amd.adjust_posterior(res, m, names, ['mu'])
    want = mod.adjust_posterior(res, m, names, ['mu'], mod.LinearAdjustment())
    assert got.outputs['mu'].shape == (500,)
    assert R.adjusted_error(got.outputs['mu'], want.outputs['mu']) <= R.bound(gold['e_adj'][R.same_m(2)])
    assert np.var(got.outputs['mu']) < np.var(res.outputs['mu'])    # the adjustment tightens the sample


@needs_reference
def test_a_non_finite_summary_row_is_dropped_as_the_reference_drops_it(gold):
    import elfi_amd
    ref_shim.install()
    from elfi.methods import post_processing as mod
    names = list(R.GAUSS_RUN['summaries'])
    sample, model = R.gauss_sample(mod, gold)
    sample.outputs['ss_var'] = sample.outputs['ss_var'].copy()
    sample.outputs['ss_var'][5] = np.nan
    with pytest.warns(UserWarning, match='Non-finite inputs and outputs will be omitted'):
        got = elfi_amd.adjust_posterior(sample, model, names, ['mu'])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        want = mod.adjust_posterior(sample, model, names, ['mu'], mod.LinearAdjustment())
    assert got.outputs['mu'].shape == want.outputs['mu'].shape == (499,)
    assert R.adjusted_error(got.outputs['mu'], want.outputs['mu']) <= R.bound(gold['e_adj'][R.same_m(2)])
    # dependent summaries: refused, with no host fallback
    sample2, _ = R.gauss_sample(mod, gold)
    sample2.outputs['ss_var'] = 2.0 * sample2.outputs['ss_mean']
    model2 = dict(model, ss_var=type(model['ss_mean'])(observed=2.0 * model['ss_mean'].observed))
    with pytest.raises(ValueError, match='linearly dependent.*minimum-norm'):
        elfi_amd.adjust_posterior(sample2, model2, names, ['mu'])
