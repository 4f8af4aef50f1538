"""GPU: KLIEP density-ratio estimation on the device (csrc/kliep.hip through elfi_amd/kliep.py).

The yardstick of alpha, w and the cross-validation scores is `truth` of tests/golden/kliep.npz (60-digit arithmetic on the
same float inputs); alpha is compared as a fraction of max |alpha|, w of max |w|, a score of the largest finite score, and
each must lie within 16 x the largest recorded relative error of the reference (tests/test_kliep.py: bound_for).  Iteration
counts must be equal.  Quantities that are the same sums (scales in one call against single calls, full fits with and
without folds, the ratio at the fit's own rows, the device-pointer forms against the host forms) must be equal bit for bit.

Measured on an MI355X (|device - truth| per case against e_ref): see DESIGN.md, "KLIEP density-ratio estimation".
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import device_layout as DL
import kliep_ref as R
import stream_order as SO
from test_kliep import bound_for, case_truth, score_dev

ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle')
sys.path.insert(0, ORACLE)
import ref_shim  # noqa: E402

pytestmark = pytest.mark.gpu
needs_reference = pytest.mark.skipif(not ref_shim.available(), reason='no reference package (run oracle/make_ref.sh)')
DBL = C.c_double


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'kliep.npz'))


@pytest.fixture(scope='module')
def elfi():
    e = ref_shim.install()
    import elfi.clients.native as native
    native.set_as_default()
    return e


def _fit(case, **kw):
    import elfi_amd
    return elfi_amd.kliep_fit(case['x'], case['y'], case['weights_x'], case['weights_y'],
                              **dict(dict(R.fit_kwargs(case), sigma=case['sigma']), **kw))


def _same(a, b):
    """Bit for bit, NaNs included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ci', range(len(R.CASES)))
def test_parity_with_truth(hip_ctx, gold, ci):
    case = R.make_case(ci, gold['seeds'][ci])
    tol = bound_for(gold)
    a_hi, a_lo, w_hi, w_lo = case_truth(gold, ci)
    got = _fit(case)
    ea, ew = R.rel_err(got['alpha'][0], a_hi, a_lo), R.rel_err(got['w'][0], w_hi, w_lo)
    em = abs((got['w'][0].max() - w_hi.max()) - w_lo[np.argmax(w_hi)]) / np.max(np.abs(w_hi))
    print('case %d: iters %d (truth %d); |device-truth| alpha %.2e (e_ref %.2e) w %.2e (e_ref %.2e) max_ratio %.2e; bound %.2e'
          % (ci, got['iters'][0], gold['iters'][ci], ea, gold['e_ref_alpha'][ci], ew, gold['e_ref_w'][ci], em, tol))
    assert got['alpha'].shape == (1, case['n']) and got['w'].shape == (1, len(case['x']))
    assert got['iters'][0] == gold['iters'][ci]
    assert ea <= tol and ew <= tol and em <= tol
    if 'far_row' in R.CASES[ci]:
        assert got['w'][0, R.CASES[ci]['far_row']] == 0.0


@needs_reference
@pytest.mark.parametrize('ci', range(len(R.CASES)))
def test_class_fit_max_ratio_and_w(hip_ctx, elfi, gold, ci):
    import elfi_amd
    case = R.make_case(ci, gold['seeds'][ci])
    tol = bound_for(gold)
    a_hi, a_lo, w_hi, w_lo = case_truth(gold, ci)
    est = elfi_amd.HipDensityRatioEstimation(**R.fit_kwargs(case))
    est.fit(case['x'], case['y'], weights_x=case['weights_x'], weights_y=case['weights_y'], sigma=float(case['sigma']))
    assert est.optimize is False and est.sigma == case['sigma'] and est.iterations == gold['iters'][ci]
    assert R.rel_err(est.alpha, a_hi, a_lo) <= tol
    wmax = np.max(np.abs(w_hi))
    assert abs((est.max_ratio() - w_hi.max()) - w_lo[np.argmax(w_hi)]) / wmax <= tol
    assert abs(est.max_ratio() - gold['max_ratio_ref'][ci]) / wmax <= tol + gold['e_ref_w'][ci]
    pts = case['x'][::3]
    w = est.w(pts)
    assert w.shape == (len(pts),) and R.rel_err(w, w_hi[::3], w_lo[::3]) * np.max(np.abs(w_hi[::3])) / wmax <= tol
    one = est.w(case['x'][1])                     # one point: an array of one, as the reference's partial returns
    assert one.shape == (1,) and one[0] == est.w(case['x'])[1]
    est.fit(case['x'], case['y'], weights_x=case['weights_x'], weights_y=case['weights_y'])     # sigma persists
    assert est.sigma == case['sigma'] and _same(est.w(pts), w)


# 2 ---------------------------------------------------------------------------------------------------------------
def test_cross_validation_against_truth(hip_ctx, gold):
    case = R.make_case(R.CV_CASE, gold['seeds'][R.CV_CASE])
    tol, scale = bound_for(gold), float(gold['cv_scale'])
    got = _fit(case, sigma=R.CV_SIGMAS, fold=R.CV_FOLD)
    assert got['scores'].shape == (len(R.CV_SIGMAS), R.CV_FOLD) and got['lcv'].shape == (len(R.CV_SIGMAS),)
    es = score_dev(got['scores'], gold['cv_scores_hi'], gold['cv_scores_lo'], scale)
    el = score_dev(got['lcv'], gold['cv_lcv_hi'], gold['cv_lcv_lo'], scale)
    print('cross-validation: lcv %s; |device-truth| scores %.2e lcv %.2e (e_ref %.2e), bound %.2e'
          % (got['lcv'], es, el, gold['e_ref_cv'], tol))
    assert es <= tol and el <= tol
    # the scale at which the reference's own scores go to NaN (b underflows to 0): not a number here either
    small = _fit(case, sigma=float(gold['cv_small_sigma']), fold=R.CV_FOLD)
    assert np.isnan(gold['cv_small_ref']) and np.isnan(small['lcv'][0])
    # no row with a basis value above 1e-64 (only rows that are not numbers give that: a centre is a row): +inf
    bad = dict(case, x=np.full_like(case['x'], np.nan))
    none = _fit(bad, sigma=[1.0], fold=R.CV_FOLD, max_iter=9)
    assert none['lcv'][0] == np.inf and np.all(np.isnan(none['alpha'])) and none['iters'][0] == 8


@needs_reference
def test_optimize_selects_the_best_scale_where_the_reference_keeps_the_first(hip_ctx, elfi, gold):
    import elfi_amd
    case = R.make_case(R.CV_CASE, gold['seeds'][R.CV_CASE])
    est = elfi_amd.HipDensityRatioEstimation(fold=R.CV_FOLD, optimize=True, **R.fit_kwargs(case))
    est.fit(case['x'], case['y'], weights_x=case['weights_x'], weights_y=case['weights_y'], sigma=list(R.CV_SIGMAS))
    assert est.sigma == 1.0 and est.optimize is True
    assert float(gold['cv_ref_choice']) == 10.0             # what the reference class kept on the same inputs
    assert np.argmax(gold['cv_lcv_ref']) == 1                # ... against its own scores
    one = _fit(case, sigma=1.0)
    assert _same(est.alpha, one['alpha'][0]) and est.max_ratio() == one['w'][0].max()


# 3 ---------------------------------------------------------------------------------------------------------------
def test_scales_folds_and_ratio_bit_for_bit(hip_ctx, gold):
    import elfi_amd
    case = R.make_case(R.CV_CASE, gold['seeds'][R.CV_CASE])
    sig = R.CV_SIGMAS + [case['sigma']]
    allof = _fit(case, sigma=sig, fold=R.CV_FOLD)
    plain = _fit(case, sigma=sig)
    assert sorted(plain) == ['alpha', 'iters', 'w']
    for k in ('alpha', 'w', 'iters'):
        assert _same(allof[k], plain[k]), k                                  # full fits with F = 5 equal F = 0
    for s, sg in enumerate(sig):
        one = _fit(case, sigma=sg, fold=R.CV_FOLD)
        for k in ('alpha', 'w', 'iters', 'scores', 'lcv'):
            assert _same(one[k][0], allof[k][s]), (k, sg)                    # S scales in one call equal S single calls
        n = case['n']
        assert _same(elfi_amd.kliep_ratio(case['x'], case['x'][:n], allof['alpha'][s], sg), allof['w'][s])
    big = R.make_case(5, gold['seeds'][5])                                   # n = 256: every column slot of a lane
    fit = _fit(big)
    assert _same(elfi_amd.kliep_ratio(big['x'][:501], big['x'][:big['n']], fit['alpha'][0], big['sigma']), fit['w'][0, :501])


def _dev_fit_args(case, sig, F):
    x, y = case['x'], case['y']
    wx, wy = case['weights_x'], case['weights_y']
    return x, y, wx, wx / wx.sum(), wy / wy.sum(), np.array(sig, dtype=np.float64), F


def test_device_pointer_forms_at_a_pitch_and_an_offset_equal_the_host_forms(hip_ctx, gold):
    """elfihip_kliep_fit_dev / elfihip_kliep_ratio_dev on torch tensors, rows at the pitch d + 3 from a base that is only
    8-byte aligned, every output between sentinels; the optional outputs left out; and the host forms at that pitch."""
    import torch
    import elfi_amd
    from elfi_amd import _lib
    case = R.make_case(R.CV_CASE, gold['seeds'][R.CV_CASE])
    sig, F = [1.0, case['sigma']], R.CV_FOLD
    want = _fit(case, sigma=sig, fold=F)
    x, y, wx, wxn, wyn, s, _ = _dev_fit_args(case, sig, F)
    (Nx, d), Ny, n, S = x.shape, len(y), case['n'], len(sig)
    ld = d + 3
    tail = (DBL(case['epsilon']), case['max_iter'], DBL(case['abs_tol']), case['interval'])
    # the host form at a pitch
    wide_x, wide_y = np.full((Nx, ld), np.nan), np.full((Ny, ld), np.nan)
    wide_x[:, :d], wide_y[:, :d] = x, y
    got = dict(alpha=np.empty((S, n)), w=np.empty((S, Nx)), iters=np.empty(S, dtype=np.int64), scores=np.empty((S, F)),
               lcv=np.empty(S))
    hip_ctx.call('elfihip_kliep_fit', _lib.ptr(wide_x), Nx, d, ld, _lib.ptr(wide_y), Ny, ld, _lib.ptr(wx), _lib.ptr(wxn),
                 _lib.ptr(wyn), _lib.ptr(s), S, n, *tail, F, *[_lib.ptr(got[k]) for k in ('alpha', 'w', 'iters', 'scores', 'lcv')])
    for k in got:
        assert _same(got[k], want[k]), k
    # the device form
    kx, dx = DL.place(x, ld, 1)
    ky, dy = DL.place(y, ld, 1)
    dwx, dwxn, dwyn = DL.to_device(wx), DL.to_device(wxn), DL.to_device(wyn)
    outs = dict(alpha=DL.guarded_out(S, n, off=1), w=DL.guarded_out(S, Nx), iters=DL.guarded_out(S, 1, off=1),
                scores=DL.guarded_out(S, F), lcv=DL.guarded_out(S, 1, off=1))
    torch.cuda.synchronize()
    hip_ctx.call('elfihip_kliep_fit_dev', dx, Nx, d, ld, dy, Ny, ld, dwx.data_ptr(), dwxn.data_ptr(), dwyn.data_ptr(),
                 _lib.ptr(s), S, n, *tail, F, *[outs[k].ptr for k in ('alpha', 'w', 'iters', 'scores', 'lcv')])
    hip_ctx.synchronize()
    for k in ('alpha', 'w', 'scores', 'lcv'):
        assert _same(outs[k].check().reshape(want[k].shape), want[k]), k
    assert np.array_equal(outs['iters'].check().view(np.int64), want['iters'])
    # optional outputs left NULL: each of the others is the same
    for keep in ('alpha', 'w', 'lcv'):
        o = DL.guarded_out(*want[keep].reshape(S, -1).shape)
        ptrs = [o.ptr if k == keep else None for k in ('alpha', 'w', 'iters', 'scores', 'lcv')]
        hip_ctx.call('elfihip_kliep_fit_dev', dx, Nx, d, ld, dy, Ny, ld, dwx.data_ptr(), dwxn.data_ptr(), dwyn.data_ptr(),
                     _lib.ptr(s), S, n, *tail, F, *ptrs)
        hip_ctx.synchronize()
        assert _same(o.check().reshape(want[keep].shape), want[keep]), keep
    # F = 0 without normalised numerator weights
    o = DL.guarded_out(S, n)
    hip_ctx.call('elfihip_kliep_fit_dev', dx, Nx, d, ld, dy, Ny, ld, dwx.data_ptr(), None, dwyn.data_ptr(), _lib.ptr(s), S, n,
                 *tail, 0, o.ptr, None, None, None, None)
    hip_ctx.synchronize()
    assert _same(o.check(), want['alpha'])
    # the ratio: points and centres at the pitch, M no multiple of the rows of a workgroup
    M = 155
    da = DL.to_device(want['alpha'][1])
    o = DL.guarded_out(M, 1, off=1)
    hip_ctx.call('elfihip_kliep_ratio_dev', dx, M, d, ld, dx, n, ld, da.data_ptr(), DBL(sig[1]), o.ptr)
    hip_ctx.synchronize()
    assert _same(o.check(), want['w'][1, :M])
    host = np.empty(M)
    hip_ctx.call('elfihip_kliep_ratio', _lib.ptr(wide_x), M, d, ld, _lib.ptr(wide_x), n, ld, _lib.ptr(want['alpha'][1]),
                 DBL(sig[1]), _lib.ptr(host))
    assert _same(host, want['w'][1, :M])
    assert elfi_amd.kliep_ratio(np.empty((0, d)), x[:n], want['alpha'][1], sig[1]).shape == (0,)
    del kx, ky


# 4 ---------------------------------------------------------------------------------------------------------------
def _issue_fit(d, which):
    case = R.make_case(R.CV_CASE, R.CASES[R.CV_CASE]['seed'] + which)
    sig, F = [1.0 + which, 1.7], 3
    x, y, wx, wxn, wyn, s, _ = _dev_fit_args(case, sig, F)
    (Nx, dim), Ny, n, S = x.shape, len(y), case['n'], len(sig)
    bx, by, bwx, bwxn, bwyn, hs = d.input(x), d.input(y), d.input(wx), d.input(wxn), d.input(wyn), d.host(s)
    outs = (d.out(S, n), d.out(S, Nx), d.out(S), d.out(S, F), d.out(S))

    def issue():
        d.call('elfihip_kliep_fit_dev', d.cx, bx.ptr, Nx, dim, dim, by.ptr, Ny, dim, bwx.ptr, bwxn.ptr, bwyn.ptr,
               hs.ctypes.data, S, n, DBL(case['epsilon']), 40, DBL(case['abs_tol']), case['interval'], F,
               *[o.ptr for o in outs], host=(hs,))
    return issue


def _issue_ratio(d, which):
    rs = np.random.RandomState(300 + which)
    M, n, dim = 1001, 70, 4
    pts, cen, alpha = rs.randn(M, dim), rs.randn(n, dim), rs.uniform(0, 1, n)
    bp, bc, ba, o = d.input(pts), d.input(cen), d.input(alpha), d.out(M)

    def issue():
        d.call('elfihip_kliep_ratio_dev', d.cx, bp.ptr, M, dim, dim, bc.ptr, n, dim, ba.ptr, DBL(1.5 + which), o.ptr)
    return issue


def _two(issue_of):
    def case(d):
        issues = [issue_of(d, which) for which in (0, 1)]
        d.go()
        for issue in issues:
            issue()
        d.done()
    return case


@pytest.mark.parametrize('name,issue_of', [('kliep fit', _issue_fit), ('kliep ratio', _issue_ratio)],
                         ids=['kliep_fit', 'kliep_ratio'])
def test_dev_entry_point_in_stream_order(hip_ctx, name, issue_of):
    ref, got, d = SO.run_both(hip_ctx, _two(issue_of), name)
    SO.guards_intact(ref, d.guarded)
    SO.guards_intact(got, d.guarded)
    SO.assert_same(ref, got, name)
    assert d.still_busy, ('%s: the stream was idle when the last call had returned (delay %.1f ms, calls issued in %.1f '
                          'ms): a call waited for the stream on the host' % (name, d.delay, d.issue_ms))


# 5 ---------------------------------------------------------------------------------------------------------------
def test_c_entry_points_refuse_every_limit(hip_ctx):
    from elfi_amd import _lib
    x, y, w = np.zeros((8, 2)), np.zeros((6, 2)), np.ones(8)
    out = np.zeros(64)

    def fit(Nx=8, d=2, ldx=2, Ny=6, ldy=2, sig=(1.0,), S=None, n=4, max_iter=5, interval=2, F=0):
        s = np.array(sig, dtype=np.float64)
        hip_ctx.call('elfihip_kliep_fit', _lib.ptr(x), Nx, d, ldx, _lib.ptr(y), Ny, ldy, _lib.ptr(w), _lib.ptr(w), _lib.ptr(w),
                     _lib.ptr(s), len(s) if S is None else S, n, DBL(0.1), max_iter, DBL(0.01), interval, F, _lib.ptr(out),
                     None, None, None, None)
    fit()                                                                       # the arguments the cases below vary are fine
    for kw in (dict(d=0), dict(d=65), dict(n=0), dict(n=257), dict(n=9), dict(Nx=65537), dict(Ny=65537), dict(Ny=0),
               dict(S=0), dict(S=17), dict(F=-1), dict(F=17), dict(max_iter=0), dict(interval=0), dict(sig=(0.0,)),
               dict(sig=(1.0, -2.0)), dict(sig=(np.inf,)), dict(sig=(np.nan,)), dict(ldx=1), dict(ldy=1)):
        with pytest.raises(ValueError):          # ELFIHIP_ERR_ARG, before any launch
            fit(**kw)

    def ratio(M=3, d=2, ldp=2, n=4, ldc=2, sigma=1.0):
        hip_ctx.call('elfihip_kliep_ratio', _lib.ptr(x), M, d, ldp, _lib.ptr(x), n, ldc, _lib.ptr(w), DBL(sigma), _lib.ptr(out))
    ratio()
    for kw in (dict(d=0), dict(d=65), dict(n=0), dict(n=257), dict(M=-1), dict(sigma=0.0), dict(sigma=np.inf),
               dict(sigma=np.nan), dict(ldp=1), dict(ldc=1)):
        with pytest.raises(ValueError):
            ratio(**kw)


# 6 ---------------------------------------------------------------------------------------------------------------
@needs_reference
def test_adaptive_threshold_smc_with_the_device_estimator(hip_ctx, elfi, gold):
    """HipAdaptiveThresholdSMC on the reference's MA2 with the device estimator: every fit's inputs are also fitted by the
    reference class on the host, and the two maximum ratios agree within the bound."""
    import elfi_amd
    from elfi.examples import ma2
    from elfi.methods.density_ratio_estimation import DensityRatioEstimation
    tol = bound_for(gold)
    settings = dict(n=100, epsilon=0.001, max_iter=200, abs_tol=0.01, fold=5)
    pairs = []

    class Checked(elfi_amd.hip_density_ratio_class()):
        def fit(self, x, y, weights_x=None, weights_y=None, sigma=None):
            super().fit(x, y, weights_x=weights_x, weights_y=weights_y, sigma=sigma)
            host = DensityRatioEstimation(**settings)
            host.fit(x, y, weights_x=weights_x, weights_y=weights_y, sigma=sigma)
            pairs.append((float(self.max_ratio()), float(host.max_ratio())))

    smc = elfi_amd.HipAdaptiveThresholdSMC(ma2.get_model(seed_obs=4)['d'], batch_size=2000, seed=7,
                                           densratio_estimation=Checked(**settings))
    assert isinstance(smc.densratio, DensityRatioEstimation)
    res = smc.sample(200, max_iter=3, bar=False)
    assert len(pairs) >= 1
    for dev, host in pairs:
        print('max_ratio device %.15g host %.15g relative difference %.2e bound %.2e'
              % (dev, host, abs(dev - host) / abs(host), tol))
        assert abs(dev - host) <= tol * abs(host)
    assert type(res).__name__ == 'SmcSample' and res.n_samples == 200
    assert np.all(np.isfinite(res.samples_array)) and np.all(res.weights >= 0) and res.weights.sum() > 0
    qs = [q for q in smc._quantiles if q is not None]
    assert len(qs) == len(pairs) + 1 and all(0.05 <= q <= 1 for q in qs)
