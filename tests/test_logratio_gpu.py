"""GPU: the batched logistic-regression ratio estimate (csrc/logratio.hip through elfi_amd/logratio.py).

The yardstick of coefficients, intercept and log ratio is `truth` of tests/golden/logratio.npz (the reference's tight fit
polished in 40-digit arithmetic), the bound 16 x max(e_tight over the recorded cases with the same m),
e_tight = |ref_tight - truth|, floor 16 eps (1 + |truth|) (tests/test_logratio.py: bound_for); the optimality violation,
recomputed in NumPy from the returned coefficients, is held to 16 x kkt_tight in the same way.  Quantities that are the
same sums (groups in one call against single calls, the device-pointer form against the host form, at any pitch) must be
equal bit for bit.

Measured on an MI355X (|device - truth| and the violation per case against e_tight, kkt_tight): see DESIGN.md, "Logistic-
regression ratio estimation".
"""
import math
import os
import sys
import warnings

import numpy as np
import pytest

import device_layout as DL
import logratio_ref as R
from test_logratio import bound_for, truth_vector

ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle')
sys.path.insert(0, ORACLE)
import ref_shim  # noqa: E402

pytestmark = pytest.mark.gpu
needs_reference = pytest.mark.skipif(not ref_shim.available(), reason='no reference package (run oracle/make_ref.sh)')


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'logratio.npz'))


def _ulps(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.spacing(np.abs(np.asarray(b))))


def _five_groups(n=37, nm=29, m=6):
    rs = np.random.RandomState(7)
    X = rs.randn(5, n, m) + np.linspace(0.1, 0.9, 5)[:, None, None]
    return X, 1.3 * rs.randn(nm, m), rs.randn(3, m) + 0.5


def _same(a, b):
    """Bit for bit, parts included."""
    (la, pa), (lb, pb) = a, b
    return np.array_equal(la, lb) and all(np.array_equal(pa[k], pb[k]) for k in pa)


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ci', range(len(R.CASES)))
def test_parity_with_truth(hip_ctx, gold, ci):
    import elfi_amd
    X, M, obs, C = R.make_case(ci)
    m = X.shape[1]
    with warnings.catch_warnings():
        warnings.simplefilter('error')              # the default tol is reached: no warning
        lr, p = elfi_amd.log_ratio(X, M, obs, C=C, return_parts=True)
    assert lr.shape == (1,) and p['coef'].shape == (1, m) and p['status'][0] == 0
    t = truth_vector(gold, ci)
    v = np.concatenate([p['coef'][0], p['intercept']])
    Z, y = R.design(X, M, p['mean'][0], p['scale'][0])
    viol = R.violation(v, Z, y, C)
    err_v, err_lr = np.abs(v - t).max(), abs(lr[0] - gold['truth_logratio'][ci])
    b_v, b_lr = bound_for(gold, m, truth=t), bound_for(gold, m, truth=gold['truth_logratio'][ci])
    b_kkt = bound_for(gold, m, 'kkt_tight')
    print('case %2d n=%d nm=%d m=%d: n_iter %d  |device-truth| log ratio %.2e coefficients %.2e (e_tight %.2e, e_default '
          '%.2e, bounds %.2e %.2e)  violation %.2e (kkt_tight %.2e, bound %.2e)'
          % (ci, len(X), len(M), m, p['n_iter'][0], err_lr, err_v, gold['e_tight'][ci], gold['e_default'][ci], b_lr, b_v,
             viol, gold['kkt_tight'][ci], b_kkt))
    assert np.array_equal(v != 0, t != 0), 'support'
    assert err_v <= b_v and err_lr <= b_lr
    assert viol <= b_kkt
    mean, scale = R.scaler(X, M)
    assert _ulps(p['mean'][0], mean) <= 4 and _ulps(p['scale'][0], scale) <= 4
    if ci == R.CONSTANT_COLUMN[0]:
        assert p['scale'][0, R.CONSTANT_COLUMN[1]] == 1.0 and p['coef'][0, R.CONSTANT_COLUMN[1]] == 0.0
    if ci == 3:
        assert lr[0] == 0.0 and not v.any() and p['n_iter'][0] == 0


# 2 ---------------------------------------------------------------------------------------------------------------
def _groups_in_one_call_equal_single_calls(m):
    import elfi_amd
    X, M, obs = _five_groups(m=m)
    lr, p = elfi_amd.log_ratio(X, M, obs, return_parts=True)
    assert lr.shape == (5, 3) and np.all(p['status'] == 0) and len(set(lr[:, 0])) == 5
    for g in range(5):
        one, q = elfi_amd.log_ratio(X[g], M, obs, return_parts=True)
        assert one.shape == (3,) and np.array_equal(one, lr[g]), g
        for k in q:
            assert np.array_equal(q[k][0], p[k][g]), (g, k)
    flat = elfi_amd.log_ratio(X.reshape(-1, X.shape[2]), M, obs, n_groups=5)
    assert np.array_equal(flat, lr)


def test_groups_in_one_call_equal_single_calls(hip_ctx):
    _groups_in_one_call_equal_single_calls(6)


def test_groups_in_one_call_equal_single_calls_at_three_tiles(hip_ctx):
    _groups_in_one_call_equal_single_calls(40)     # 33 <= m <= 48: the three-tile instance of the kernel


def _dev_call(ctx, X, M, obs, layout_x, layout_m, G, C=1.0, class_min=0.0, max_iter=100):
    import torch
    from elfi_amd.logratio import DEFAULT_TOL as tol
    rows, m = X.shape
    tx, px = DL.place(X, m + layout_x[0], layout_x[1])
    tm, pm = DL.place(M, m + layout_m[0], layout_m[1])
    dy = DL.to_device(obs)
    k = len(obs)
    outs = dict(lr=DL.guarded_out(G, k, 1), coef=DL.guarded_out(G, m), icpt=DL.guarded_out(G, 1, 1),
                mean=DL.guarded_out(G, m, 1), scale=DL.guarded_out(G, m))
    ints = torch.full((2 * G + 2,), -77, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()     # (torch's stream and the context's own stream are not ordered against each other)
    ctx.call('elfihip_log_ratio_dev', px, G, rows // G, m, m + layout_x[0], pm, len(M), m + layout_m[0], dy.data_ptr(), k, C,
             class_min, tol, max_iter, outs['lr'].ptr, outs['coef'].ptr, outs['icpt'].ptr, outs['mean'].ptr,
             outs['scale'].ptr, ints.data_ptr(), ints.data_ptr() + 4 * G)
    ctx.synchronize()
    h = ints.cpu().numpy()
    assert np.all(h[2 * G:] == -77)
    parts = dict(coef=outs['coef'].check().reshape(G, m), intercept=outs['icpt'].check().reshape(G),
                 mean=outs['mean'].check().reshape(G, m), scale=outs['scale'].check().reshape(G, m), n_iter=h[:G].copy(),
                 status=h[G:2 * G].copy())
    return outs['lr'].check().reshape(G, k), parts


@pytest.mark.parametrize('m', [6, 7, 40])      # (40: the three-tile instance of the kernel)
def test_dev_form_at_every_layout_equals_host_form(hip_ctx, m):
    import elfi_amd
    X, M, obs = _five_groups(m=m)
    X2 = X.reshape(-1, m)
    host = elfi_amd.log_ratio(X2, M, obs, n_groups=5, return_parts=True)
    assert np.all(host[1]['status'] == 0)
    for lx, lm in zip(DL.LAYOUTS, DL.LAYOUTS[::-1]):
        got = _dev_call(hip_ctx, X2, M, obs, lx, lm, 5)
        assert _same(got, host), (lx, lm)


def test_c_entry_point_refuses_bad_arguments(hip_ctx):
    """ELFIHIP_ERR_ARG before any launch: the output keeps its sentinel."""
    from elfi_amd import _lib
    from elfi_amd.logratio import DEFAULT_TOL
    SENTINEL = -12345.5
    X, M, obs = np.zeros((8, 3)), np.ones((6, 3)), np.zeros((1, 3))
    lr = np.full(2, SENTINEL)
    inf, nan = float('inf'), float('nan')

    def call(G=1, n=8, m=3, ldx=3, nm=6, ldm=3, k=1, C=1.0, class_min=0.0, tol=DEFAULT_TOL, max_iter=100, out=lr):
        hip_ctx.call("elfihip_log_ratio", _lib.ptr(X), G, n, m, ldx, _lib.ptr(M), nm, ldm, _lib.ptr(obs), k, C, class_min, tol,
                     max_iter, _lib.ptr(out), None, None, None, None, None, None)
    for kw in (dict(m=65), dict(n=0), dict(nm=0), dict(ldx=2), dict(ldm=2), dict(k=0), dict(C=0.0), dict(C=inf), dict(C=nan),
               dict(class_min=1.0), dict(class_min=-0.1), dict(tol=-1.0), dict(max_iter=-1), dict(out=None)):
        with pytest.raises(ValueError):
            call(**kw)
        assert np.all(lr == SENTINEL), kw
    call()                                   # the call itself is sound: good arguments go through
    assert lr[0] != SENTINEL and lr[1] == SENTINEL


# 3 ---------------------------------------------------------------------------------------------------------------
def test_class_min(hip_ctx):
    import elfi_amd
    X, M, _, C = R.make_case(5)             # nearly separable: large log ratios of either sign
    obs = np.array([[3.0, 3.0, 3.0], [-2.0, -2.0, -2.0], [0.3, 0.2, 0.1]])
    free = elfi_amd.log_ratio(X, M, obs)
    assert free[0] > 3 and free[1] < -3
    cm = 0.01
    got = elfi_amd.log_ratio(X, M, obs, class_min=cm)
    from scipy.special import expit
    binds = expit(free) < cm
    assert binds[1] and not binds[0]
    assert np.array_equal(got[~binds], free[~binds])
    assert np.all(got[binds] == math.log(cm / (1 - cm)))
    # the value is finite where the reference's expit under- or overflows
    far = elfi_amd.log_ratio(X, M, 1e3 * obs[:2])
    assert np.all(np.isfinite(far)) and far[0] > 700 and far[1] < -700


def test_max_iter_sets_the_flag_and_warns(hip_ctx):
    import elfi_amd
    from elfi_amd.logratio import LogRatioConvergenceWarning
    X, M, obs = _five_groups()
    with pytest.warns(LogRatioConvergenceWarning, match='max_iter'):
        lr, p = elfi_amd.log_ratio(X, M, obs, max_iter=1, return_parts=True)
    assert np.all(p['status'] == 1) and np.all(p['n_iter'] == 1) and np.all(np.isfinite(lr))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        full, q = elfi_amd.log_ratio(X, M, obs, return_parts=True)
    assert np.all(q['n_iter'] > 1) and not np.array_equal(full, lr)


def test_nan_row_spoils_its_group_only(hip_ctx):
    import elfi_amd
    X, M, obs = _five_groups()
    clean, p0 = elfi_amd.log_ratio(X, M, obs, return_parts=True)
    Xn = X.copy()
    Xn[2, 11, 3] = np.nan
    Xn[4, 0, 0] = np.inf
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        lr, p = elfi_amd.log_ratio(Xn, M, obs, return_parts=True)
    for g in range(5):
        if g in (2, 4):
            assert p['status'][g] == 2 and np.all(np.isnan(lr[g])) and np.all(np.isnan(p['coef'][g]))
            assert np.isnan(p['intercept'][g]) and np.all(np.isnan(p['mean'][g])) and np.all(np.isnan(p['scale'][g]))
        else:
            assert p['status'][g] == 0 and np.array_equal(lr[g], clean[g]) and np.array_equal(p['coef'][g], p0['coef'][g])


def test_three_observed_rows(hip_ctx):
    import elfi_amd
    X, M, obs = _five_groups()
    lr, p = elfi_amd.log_ratio(X[0], M, obs, return_parts=True)
    assert lr.shape == (3,)
    v = np.concatenate([p['coef'][0], p['intercept']])
    want = R.log_ratio_at(v, obs, p['mean'][0], p['scale'][0])
    np.testing.assert_allclose(lr, want, rtol=0, atol=16 * R.EPS * (1 + np.abs(want).max()) * X.shape[2])
    for j in range(3):
        assert elfi_amd.log_ratio(X[0], M, obs[j])[0] == lr[j]


@pytest.mark.parametrize('n,nm,m', [(1, 1, 1), (1, 2, 64), (3, 1, 5), (2, 40, 17)])
def test_smallest_groups(hip_ctx, n, nm, m):
    """The limits n >= 1, nm >= 1: the fit is stationary to the default tol plus the rounding of NumPy's own gradient (a
    sum of N terms of size <= max|z|)."""
    import elfi_amd
    from elfi_amd.logratio import DEFAULT_TOL
    rs = np.random.RandomState(100 * n + nm + m)
    X, M, obs = rs.randn(n, m) + 0.7, 1.3 * rs.randn(nm, m), rs.randn(2, m)
    lr, p = elfi_amd.log_ratio(X, M, obs, return_parts=True)
    assert p['status'][0] == 0 and np.all(np.isfinite(lr))
    v = np.concatenate([p['coef'][0], p['intercept']])
    Z, y = R.design(X, M, p['mean'][0], p['scale'][0])
    assert R.violation(v, Z, y, 1.0) <= DEFAULT_TOL + 4 * R.EPS * len(Z) * np.abs(Z).max()
    mean, scale = R.scaler(X, M)
    assert _ulps(p['mean'][0], mean) <= 4 and _ulps(p['scale'][0], scale) <= 4


# 4 ---------------------------------------------------------------------------------------------------------------
@needs_reference
def test_classifier_interface(hip_ctx):
    ref_shim.install()
    import elfi_amd
    from elfi.methods.classifier import LogisticRegression
    X, M, obs = _five_groups()
    X, m = X[1], X.shape[2]
    want, parts = elfi_amd.log_ratio(X, M, obs, return_parts=True)
    rows = np.vstack([X, M])
    y = np.concatenate([np.ones(len(X)), -np.ones(len(M))])
    # any interleaving of the two labels that keeps each label's rows in their order is the same device call
    rs = np.random.RandomState(3)
    slots = np.zeros(len(rows), dtype=bool)
    slots[rs.choice(len(rows), len(X), replace=False)] = True
    mixed, labels = np.empty_like(rows), np.where(slots, 1.0, -1.0)
    mixed[slots], mixed[~slots] = X, M
    assert not np.array_equal(labels, y)
    clf = elfi_amd.HipLogisticRegression()
    clf.fit(mixed, labels)
    got = clf.predict_log_likelihood_ratio(obs)
    assert got.shape == (3,) and np.array_equal(got, want)
    assert np.array_equal(clf.predict_likelihood_ratio(obs), np.exp(want))
    # a full shuffle is the ordered call on the rows split by label
    full = rs.permutation(len(rows))
    clf.fit(rows[full], y[full])
    assert np.array_equal(clf.predict_log_likelihood_ratio(obs),
                          elfi_amd.log_ratio(rows[full][y[full] == 1], rows[full][y[full] == -1], obs))
    clf.fit(rows, y)
    ref = LogisticRegression()
    ref.fit(rows, y)
    a, b = clf.attributes['parameters'], ref.attributes['parameters']
    assert set(a) == set(b) == {'coef_', 'intercept_', 'n_iter'}
    for key in a:
        assert np.shape(a[key]) == np.shape(b[key]), key
    assert np.array_equal(a['coef_'], parts['coef']) and np.array_equal(a['intercept_'], parts['intercept'])
    with pytest.warns(elfi_amd.logratio.LogRatioConvergenceWarning):
        slow = elfi_amd.HipLogisticRegression(config={'penalty': 'l1', 'solver': 'liblinear', 'max_iter': 1})
        slow.fit(rows, y)
        slow.predict_log_likelihood_ratio(obs)
