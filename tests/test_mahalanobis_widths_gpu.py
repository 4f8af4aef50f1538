"""Mahalanobis distances at every row width that selects a kernel or fills its tiles differently (csrc/mahalanobis.hip:
launch_mahalanobis), through the host form and through elfihip_dist_rows_dev at a packed, an even and an odd pitch.

The reference is SciPy's cdist through the oracle at the project's 1e-13 relative.  Every case is
also computed in np.longdouble on the host; the test prints, per kernel form, the device's and SciPy's own worst error
against it (the figures of DESIGN.md section 5), and if the device ever missed SciPy by more than 1e-13 they say which of
the two is off.
"""
import ctypes as C

import numpy as np
import pytest

import distance_oracle as O
from device_layout import guarded_out, place, to_device, vec2

pytestmark = pytest.mark.gpu

WIDTHS = list(range(1, 67)) + [100, 128, 299]
NS = (1, 65, 1000)
DEV_LAYOUTS = [(0, 0), (2, 0), (1, 0)]


def kernel_form(m, layout):
    """launch_mahalanobis' choice for rows of m doubles in a layout of tests/device_layout.py."""
    v = vec2(m, layout)
    if v and m in (2, 4):
        return 'narrow'
    if 8 <= m <= 64:
        if v:
            return 'register' if (m + 15) // 16 == 3 else 'split'
        return 'lds-mfma'
    return 'lane-per-row'


def make_vi(m, rs):
    """As test_mahalanobis_shapes_vs_oracle: a proper inverse covariance with negative off-diagonals, symmetrised."""
    Z = rs.randn(4 * m + 5, m) @ rs.randn(m, m)
    VI = np.linalg.inv(np.cov(Z.T).reshape(m, m) + 0.1 * np.eye(m))
    return 0.5 * (VI + VI.T)


def longdouble_reference(X, y, VI):
    d = X.astype(np.longdouble) - y.astype(np.longdouble)
    return np.sqrt(np.sum((d @ VI.astype(np.longdouble)) * d, axis=1))


def rel_err(a, exact):
    return float(np.max(np.abs(a.astype(np.longdouble) - exact) / exact))


def dev_call(ctx, ptr, n, m, ldx, dy, dvi):
    import torch
    out = guarded_out(n)
    torch.cuda.synchronize()     # (torch's stream and the context's own stream are not ordered against each other)
    ctx.call('elfihip_dist_rows_dev', 6, ptr, n, m, ldx, dy.data_ptr(), dvi.data_ptr(), C.c_double(2.0), out.ptr)
    ctx.synchronize()
    return out.check()


@pytest.mark.parametrize('m', WIDTHS)
def test_every_width_host_and_device_layouts(hip_ctx, m):
    import elfi_amd
    worst = {}
    for n in NS:
        rs = np.random.RandomState(77 * m + n)
        VI = make_vi(m, rs)
        X, y = rs.randn(n, m) * 2, rs.randn(1, m)
        ref = O.cdist_rows(X, y, 'mahalanobis', VI=VI)
        exact = longdouble_reference(X, y, VI)
        scipy_err = rel_err(ref, exact)
        dy, dvi = to_device(y), to_device(VI)
        results = [('host', kernel_form(m, (0, 0)), elfi_amd.cdist_rows(X, y, 'mahalanobis', VI=VI))]
        for layout in DEV_LAYOUTS:
            buf, ptr = place(X, m + layout[0], layout[1])
            results.append((layout, kernel_form(m, layout), dev_call(hip_ctx, ptr, n, m, m + layout[0], dy, dvi)))
        for where, form, got in results:
            w = worst.setdefault(form, [0.0, 0.0])
            w[0], w[1] = max(w[0], rel_err(got, exact)), max(w[1], scipy_err)
        for form, (dev_err, sp_err) in worst.items():
            print('MAHALANOBIS m=%d n=%d form=%s device_err=%.3g scipy_err=%.3g' % (m, n, form, dev_err, sp_err))
        for where, form, got in results:
            np.testing.assert_allclose(got, ref, rtol=1e-13, atol=0, err_msg='m=%d n=%d %s (%s kernel)' % (m, n, where, form))
        # the pitch does not change the arithmetic: (2, 0) takes the kernel of the packed layout, which the host form takes too
        assert np.array_equal(results[0][2], results[1][2]) and np.array_equal(results[1][2], results[2][2]), (m, n)


@pytest.mark.parametrize('m', [12, 24, 40, 56, 33, 5])
def test_rows_do_not_leak_into_each_other(hip_ctx, m):
    """A NaN row, a +inf row and a row with both beside finite rows (rows 3, 64, 99 of 100: inside a full tile of 64 and in
    the short last tile): the NaN pattern is SciPy's, and every other row has the bits it has when those three rows are
    finite.  The matrix-core kernels read operands beyond a row's m columns (the register form: the neighbouring row's
    values, masked) and a short last tile holds stale rows; neither may reach another row's result."""
    import elfi_amd
    rs = np.random.RandomState(m)
    VI = make_vi(m, rs)
    clean, y = rs.randn(100, m) * 2, rs.randn(1, m)
    X = clean.copy()
    X[3] = np.nan
    X[64] = np.inf
    X[99, ::2] = np.nan
    X[99, 1::3] = np.inf
    bad = np.zeros(100, dtype=bool)
    bad[[3, 64, 99]] = True
    with np.errstate(all='ignore'):
        ref = O.cdist_rows(X, y, 'mahalanobis', VI=VI)
    assert np.array_equal(np.isnan(ref), bad)
    dy, dvi = to_device(y), to_device(VI)
    runs = [('host', lambda A: elfi_amd.cdist_rows(A, y, 'mahalanobis', VI=VI))]
    for layout in DEV_LAYOUTS:
        def run(A, layout=layout):
            buf, ptr = place(A, m + layout[0], layout[1])
            return dev_call(hip_ctx, ptr, 100, m, m + layout[0], dy, dvi)
        runs.append((layout, run))
    for where, run in runs:
        got, base = run(X), run(clean)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (m, where)
        assert np.array_equal(got[~bad], base[~bad]), (m, where, 'a neighbouring row changed a finite row')
        np.testing.assert_allclose(got[~bad], ref[~bad], rtol=1e-13, atol=0)
