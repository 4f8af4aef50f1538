"""canberra, braycurtis, cosine and correlation on the HIP distance path, against scipy.spatial.distance.cdist.

Tolerances:
  * unweighted canberra / braycurtis / cosine / correlation, weighted canberra / braycurtis, rows of at most 299
    columns: BIT-EXACT (SciPy's summation order, no FMA).
  * weighted cosine / correlation: absolute 1e-13 (SciPy forms them with np.dot, whose order is its BLAS's).
  * rows wider than 299 columns (one wavefront per row, butterfly sums): canberra / braycurtis relative 1e-14, cosine /
    correlation absolute 1e-14 (weighted: 1e-13).
Every launch form of the row-major pass is reached: narrow (m = 2, 4), LDS-DMA (16 / 32 / 64), pipelined, plain tile
(odd or unaligned rows, m up to 299), wide (m >= 300); and the column-major pass through HipDiscrepancy.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.spatial.distance as ssd

pytestmark = pytest.mark.gpu

NEW = ('canberra', 'braycurtis', 'cosine', 'correlation')
ALL = ('euclidean', 'sqeuclidean', 'cityblock', 'chebyshev', 'minkowski', 'seuclidean', 'mahalanobis') + NEW


def cdist(X, y, metric, w=None):
    with np.errstate(all='ignore'):
        return ssd.cdist(X, y, metric, **({} if w is None else {'w': w}))[:, 0]


def check(got, ref, metric, m, w, what=''):
    what = '%s m=%d w=%s %s' % (metric, m, w is not None, what)
    assert got.shape == ref.shape, what
    cos_like = metric in ('cosine', 'correlation')
    if m > 299:
        if cos_like:
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-13 if w is not None else 1e-14, err_msg=what)
        else:
            np.testing.assert_allclose(got, ref, rtol=1e-14, atol=0, err_msg=what)
    elif cos_like and w is not None:
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-13, err_msg=what)
    else:
        np.testing.assert_array_equal(got, ref, err_msg=what)   # (NaN equals NaN here)


def data(n, m, seed):
    rs = np.random.RandomState(seed)
    X = rs.randn(n, m) * rs.uniform(0.5, 3, m) + rs.uniform(-1, 1, m)
    y = rs.randn(1, m)
    w = rs.uniform(0.1, 2, m)
    w[rs.rand(m) < 0.1] = 0.0
    return X, y, w


@pytest.mark.parametrize('metric', NEW)
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('m', [2, 4, 16, 32, 64, 3, 5, 33, 100, 128, 299, 300, 700])
def test_every_launch_form(hip_ctx, metric, weighted, m):
    import elfi_amd
    n = 4099 if m < 300 else 777                 # a multiple of no tile
    X, y, w = data(n, m, 1000 + m)
    w = w if weighted else None
    check(elfi_amd.cdist_rows(X, y, metric, w=w), cdist(X, y, metric, w), metric, m, w)
    # the register-staged forms (form 1) as well: same results
    hip_ctx.call('elfihip_dist_set_form', 1)
    try:
        check(elfi_amd.cdist_rows(X, y, metric, w=w), cdist(X, y, metric, w), metric, m, w, 'form 1')
    finally:
        hip_ctx.call('elfihip_dist_set_form', 0)


@pytest.mark.parametrize('metric', NEW)
@pytest.mark.parametrize('m', [4, 32, 33, 100, 300])
def test_small_n_and_strided_rows(hip_ctx, metric, m):
    import elfi_amd
    for weighted in (False, True):
        Xb, y, w = data(1001, m + 6, 7 * m)
        y, w = y[:, :m], (w[:m] if weighted else None)
        for n in (0, 1, 2, 65):
            X = np.ascontiguousarray(Xb[:n, :m])
            got = elfi_amd.cdist_rows(X, y, metric, w=w)
            assert got.shape == (n,)
            check(got, cdist(X, y, metric, w), metric, m, w, 'n=%d' % n)
        for off in (1, 2):                          # column slices of a wider array: ldx = m + 6 (odd / even offset)
            X = Xb[:, off:off + m]
            assert X.strides[1] == 8 and X.strides[0] == 8 * (m + 6)
            check(elfi_amd.cdist_rows(X, y, metric, w=w), cdist(X, y, metric, w), metric, m, w, 'slice %d' % off)


@pytest.mark.parametrize('metric', NEW)
@pytest.mark.parametrize('m', [2, 5, 32, 100])
def test_column_major_path(hip_ctx, metric, m):
    import elfi_amd
    for weighted in (False, True):
        X, y, w = data(3001, m, 50 + m)
        w = w if weighted else None
        op = elfi_amd.HipDiscrepancy(metric, w=w)
        got = op(*[np.ascontiguousarray(X[:, j]) for j in range(m)], observed=tuple(y[:, j] for j in range(m)))
        check(got, cdist(X, y, metric, w), metric, m, w, 'columns')


def special_rows(m, rs):
    X = rs.randn(12, m)
    X[0] = 0.0
    X[1, 0] = np.inf
    X[2, m - 1] = -np.inf
    X[3, 0] = np.nan
    X[4, 0], X[4, m - 1] = np.inf, -np.inf
    X[5] = -0.0
    X[6, :] = 2.5                                   # a constant row: correlation 0/0
    X[7, 0] = 0.0
    return X


@pytest.mark.parametrize('metric', NEW)
@pytest.mark.parametrize('m', [4, 5, 32, 64, 300])
def test_special_values(hip_ctx, metric, m):
    import elfi_amd
    rs = np.random.RandomState(m)
    X = special_rows(m, rs)
    w = rs.uniform(0.5, 2, m)
    ys = [rs.randn(1, m), np.zeros((1, m))]
    ys[0][0, m // 2] = 0.0                          # canberra: 0/0 terms where the row is zero too
    X[7, m // 2] = 0.0
    for y in ys:
        X[8] = y[0]                                  # distance 0 (canberra, braycurtis), 0 (cosine: clipped cosine)
        for ww in (None, w):
            got = elfi_amd.cdist_rows(X, y, metric, w=ww)
            ref = cdist(X, y, metric, ww)
            if ww is not None and metric == 'correlation':
                # the constant row: its weighted mean is 2.5 only to within an ulp, so what is left after centering is
                # rounding noise whose cosine depends on the summation order (SciPy's is its BLAS's)
                got, ref = np.delete(got, 6), np.delete(ref, 6)
            np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg='%s NaN pattern' % metric)
            check(got, ref, metric, m, ww, 'special values')


def test_c_abi_ids(hip_ctx):
    import elfi_amd._lib as L
    X, y, w = data(1000, 12, 3)
    out = np.empty(1000)
    for mid, metric in zip((7, 8, 9, 10), NEW):
        assert L.METRICS[metric] == mid
        for ww in (None, w):
            hip_ctx.call('elfihip_dist_rows', mid, L.ptr(X), 1000, 12, 12, L.ptr(y), L.ptr(ww), C.c_double(2.0),
                         L.ptr(out))
            check(out.copy(), cdist(X, y, metric, ww), metric, 12, ww, 'C ABI')
    with pytest.raises(ValueError):
        hip_ctx.call('elfihip_dist_rows', 11, L.ptr(X), 1000, 12, 12, L.ptr(y), None, C.c_double(2.0), L.ptr(out))


def _selection_case(metric, k, m, nbatch, n, weighted, seed):
    import elfi_amd
    rs = np.random.RandomState(seed)
    y = rs.randn(1, m)
    w = rs.uniform(0.2, 2, m) if weighted else None
    rb = elfi_amd.RunningBest(k, metric=metric, w=w)
    try:
        ds = []
        for b in range(nbatch):
            X = rs.randn(n, m) + 0.1 * b
            X[17::1013] = X[16::1013][:len(X[17::1013])]    # duplicated rows: ties
            d = rb.push(X, y)
            s = slice(0, 2048) if w is not None else slice(None)   # (SciPy's weighted cosine is a Python loop)
            check(d[s], cdist(X[s], y, metric, w), metric, m, w, 'push %d' % b)
            ds.append(d)
        d = np.concatenate(ds)
        order = np.argsort(d, kind='stable')[:k]    # ties to the earlier row
        vals, rows = rb.result()
    finally:
        rb.close()
    np.testing.assert_array_equal(vals, d[order])
    np.testing.assert_array_equal(rows, order)


@pytest.mark.parametrize('metric', NEW)
def test_running_best_device_state(hip_ctx, metric):
    # k <= 2048: the device state; m = 32 batches of 2^16 rows, sixteen pushes without result(): sealed lists merged
    # inside the next DMA row pass.  m = 4 (narrow form) and m = 33 (tile form) beside it.
    _selection_case(metric, 500, 32, 16, 1 << 16, False, 1)
    _selection_case(metric, 500, 32, 12, 1 << 16, True, 2)
    _selection_case(metric, 1000, 4, 10, 1 << 15, False, 3)
    _selection_case(metric, 200, 33, 8, 1 << 14, True, 4)


@pytest.mark.parametrize('metric', NEW)
def test_running_best_host_state(hip_ctx, metric):
    _selection_case(metric, 3000, 32, 8, 1 << 15, False, 5)   # k > 2048: host-side state
    _selection_case(metric, 2500, 5, 6, 1 << 14, True, 6)


@pytest.mark.parametrize('metric', NEW)
def test_full_size(hip_ctx, metric):
    """10^6 x 32: a seeded 2^16-row sample checked bit-exactly against cdist, and the SoA path against the AoS path."""
    import elfi_amd
    rs = np.random.RandomState(0)
    n, m = 10 ** 6, 32
    X = rs.randn(n, m) + 0.5
    y = np.random.RandomState(1).randn(1, m)
    d = elfi_amd.cdist_rows(X, y, metric)
    idx = rs.choice(n, 1 << 16, replace=False)
    np.testing.assert_array_equal(d[idx], cdist(X[idx], y, metric))
    if metric in ('canberra', 'braycurtis'):
        w = np.random.RandomState(2).uniform(.5, 2, m)
        np.testing.assert_array_equal(elfi_amd.cdist_rows(X, y, metric, w=w)[idx], cdist(X[idx], y, metric, w))
    perm = rs.permutation(n)[:1 << 18]
    np.testing.assert_array_equal(elfi_amd.cdist_rows(X[perm], y, metric), d[perm])
    cols = [np.ascontiguousarray(X[:, j]) for j in range(m)]
    np.testing.assert_array_equal(elfi_amd.cdist_cols(cols, y, metric), d)


def _aux_kw(metric, m, rs):
    if metric == 'seuclidean':
        return {'V': rs.uniform(0.5, 2, m)}
    if metric == 'mahalanobis':
        A = rs.randn(m, m)
        return {'VI': A @ A.T + m * np.eye(m)}
    if metric == 'minkowski':
        return {'p': 3.0}
    return {}


@pytest.mark.parametrize('metric', ALL)
def test_aliases(hip_ctx, metric):
    import elfi_amd
    rs = np.random.RandomState(len(metric))
    m = 8
    X, y = rs.randn(2000, m), rs.randn(1, m)
    kw = _aux_kw(metric, m, rs)
    ref = elfi_amd.HipDistance(metric, **kw)(X, y)
    names = sorted(ssd._METRICS[metric].aka)
    assert metric in names and len(names) >= 1
    for name in names + [metric.upper(), metric.title()]:
        d = elfi_amd.HipDistance(name, **kw)
        assert d.metric == metric
        np.testing.assert_array_equal(d(X, y), ref, err_msg=name)
        np.testing.assert_array_equal(elfi_amd.cdist_rows(X, y, name, **kw), ref, err_msg=name)
        if metric != 'mahalanobis':
            cols = [np.ascontiguousarray(X[:, j]) for j in range(m)]
            np.testing.assert_array_equal(
                elfi_amd.HipDiscrepancy(name, **kw)(*cols, observed=tuple(y[:, j] for j in range(m))),
                elfi_amd.cdist_cols(cols, y, metric, **kw), err_msg=name)
    if metric == 'mahalanobis':
        # the stored canonical name keeps HipDiscrepancy's 1-d summaries on the row-major path for 'mahal' too
        cols = [np.ascontiguousarray(X[:, j]) for j in range(m)]
        got = elfi_amd.HipDiscrepancy('MAHAL', **kw)(*cols, observed=tuple(y[:, j] for j in range(m)))
        np.testing.assert_array_equal(got, ref)
    with pytest.raises(ValueError):
        elfi_amd.HipDistance('nonsense')
    with pytest.raises(ValueError):
        elfi_amd.cdist_rows(X, y, 'nonsense')


@pytest.mark.parametrize('name', ['cos', 'CO', 'Canberra', 'BRAYCURTIS'])
def test_running_best_alias(hip_ctx, name):
    import elfi_amd
    import elfi_amd._lib as L
    rs = np.random.RandomState(9)
    X, y = rs.randn(5000, 16), rs.randn(1, 16)
    canon = L.resolve_metric(name)[0]
    rb = elfi_amd.RunningBest(50, metric=name)
    try:
        d = rb.push(X, y)
        vals, rows = rb.result()
    finally:
        rb.close()
    np.testing.assert_array_equal(d, cdist(X, y, canon))
    order = np.argsort(d, kind='stable')[:50]
    np.testing.assert_array_equal(rows, order)
    np.testing.assert_array_equal(vals, d[order])
    with pytest.raises(ValueError):
        elfi_amd.RunningBest(50, metric='nonsense')
