"""CPU: the NumPy statement of the KLIEP fit (tests/kliep_ref.py) against the values recorded from the reference's own class
(tests/golden/kliep.npz, scripts/make_golden_kliep.py), and the argument handling of the Python mirrors
(elfi_amd/kliep.py), which happens before any device call.

Tolerance: the yardstick is `truth` (the quantity in 60-digit arithmetic).  alpha is compared as a fraction of max |alpha|,
w of max |w|, a score of the largest finite score; each must lie within 16 x the largest recorded relative error of the
reference, e_ref = |reference - truth| -- the rule of tests/test_semibsl.py.  Iteration counts must be equal.
"""
import os
import sys

import numpy as np
import pytest

import kliep_ref as R


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'kliep.npz'))


def bound_for(gold):
    """16 x the largest recorded relative error of the reference over every case and the cross-validation."""
    return 16.0 * max(gold['e_ref_alpha'].max(), gold['e_ref_w'].max(), float(gold['e_ref_cv']))


def case_truth(gold, ci):
    """(alpha_hi, alpha_lo, w_hi, w_lo) of a case, cut to its sizes."""
    c = R.CASES[ci]
    return (gold['alpha_hi'][ci, :c['n']], gold['alpha_lo'][ci, :c['n']], gold['w_hi'][ci, :c['Nx']],
            gold['w_lo'][ci, :c['Nx']])


def score_dev(got, hi, lo, scale):
    """Largest |score - truth| over the finite scores as a fraction of `scale`; the others must be equal."""
    got, fin = np.asarray(got), np.isfinite(hi)
    assert np.array_equal(got[~fin], hi[~fin])
    return float(np.max(np.abs((got[fin] - hi[fin]) - lo[fin])) / scale)


def test_fixture_matches_the_recipe(gold):
    assert np.array_equal(gold['seeds'], [c['seed'] for c in R.CASES])
    assert [(c['Nx'], c['Ny'], c['d'], c['n']) for c in R.CASES[:6]] == [
        (5, 5, 1, 5), (157, 211, 3, 37), (300, 300, 2, 100), (500, 500, 3, 100), (257, 64, 5, 64), (1000, 500, 8, 256)]
    assert np.array_equal(gold['cv_sigmas'], R.CV_SIGMAS) and int(gold['cv_fold']) == R.CV_FOLD
    assert float(gold['e_ref_max']) * 16 == bound_for(gold) and 0 < bound_for(gold) < 1e-9
    # the paths: a loop that runs out, loops that stop at a later check, one that stops at the first; a null row
    iters = gold['iters']
    assert iters[1] == R.CASES[1]['max_iter'] - 1 and iters[6] == 0 and 0 < iters[2] < R.CASES[2]['max_iter'] - 1
    assert gold['null_rows'][1] == 1 and gold['w_ref'][1, R.CASES[1]['far_row']] == 0.0
    assert np.all(gold['clamped'][1:] > 0)
    for ci, c in enumerate(R.CASES):           # the conditions the script asserts, seen from the stored trace
        tr = gold['trace'][ci]
        tr = tr[~np.isnan(tr)]
        assert np.all(np.abs(tr - c['abs_tol']) > c['abs_tol'] / 100)
        assert iters[ci] == ((len(tr) - 1) * c['interval'] if tr[-1] < c['abs_tol'] else c['max_iter'] - 1)


@pytest.mark.parametrize('ci', range(len(R.CASES)))
def test_restatement_against_truth_and_reference(gold, ci):
    case = R.make_case(ci, gold['seeds'][ci])
    tol = bound_for(gold)
    got = R.kliep_fit_ref(case['x'], case['y'], case['weights_x'], case['weights_y'], case['sigma'], **R.fit_kwargs(case))
    a_hi, a_lo, w_hi, w_lo = case_truth(gold, ci)
    ea, ew = R.rel_err(got['alpha'][0], a_hi, a_lo), R.rel_err(got['w'][0], w_hi, w_lo)
    print('case %d: e_ref alpha %.2e w %.2e, restatement alpha %.2e w %.2e, bound %.2e'
          % (ci, gold['e_ref_alpha'][ci], gold['e_ref_w'][ci], ea, ew, tol))
    assert got['iters'][0] == gold['iters'][ci]
    assert ea <= tol and ew <= tol
    n, Nx = R.CASES[ci]['n'], R.CASES[ci]['Nx']
    assert np.max(np.abs(got['alpha'][0] - gold['alpha_ref'][ci, :n])) <= (tol + gold['e_ref_alpha'][ci]) * np.max(np.abs(a_hi))
    assert np.max(np.abs(got['w'][0] - gold['w_ref'][ci, :Nx])) <= (tol + gold['e_ref_w'][ci]) * np.max(np.abs(w_hi))
    assert abs(got['w'][0].max() - gold['max_ratio_ref'][ci]) <= (tol + gold['e_ref_w'][ci]) * np.max(np.abs(w_hi))
    assert np.array_equal(R.kliep_ratio_ref(case['x'], case['x'][:n], got['alpha'][0], case['sigma']), got['w'][0])


def test_restatement_cross_validation(gold):
    case = R.make_case(R.CV_CASE, gold['seeds'][R.CV_CASE])
    tol = bound_for(gold)
    got = R.kliep_fit_ref(case['x'], case['y'], case['weights_x'], case['weights_y'], R.CV_SIGMAS, fold=R.CV_FOLD,
                          **R.fit_kwargs(case))
    scale = float(gold['cv_scale'])
    es = score_dev(got['scores'], gold['cv_scores_hi'], gold['cv_scores_lo'], scale)
    el = score_dev(got['lcv'], gold['cv_lcv_hi'], gold['cv_lcv_lo'], scale)
    print('cross-validation: e_ref %.2e, restatement scores %.2e lcv %.2e, bound %.2e' % (gold['e_ref_cv'], es, el, tol))
    assert es <= tol and el <= tol
    assert np.max(np.abs(got['lcv'] - gold['cv_lcv_ref'])) <= (tol + gold['e_ref_cv']) * scale
    # the decided divergence: the reference's optimize=True kept the first scale, the scores favour the second
    assert float(gold['cv_ref_choice']) == R.CV_SIGMAS[0] == 10.0
    assert R.CV_SIGMAS[int(np.argmax(gold['cv_lcv_ref']))] == R.CV_SIGMAS[int(np.argmax(got['lcv']))] == 1.0
    # a scale at which some rows are null: the folds split the non-null rows alone
    assert list(gold['cv_L']) == [157, 156, 154]
    # full fits do not depend on the folds, and a scale's results not on the other scales
    one = R.kliep_fit_ref(case['x'], case['y'], case['weights_x'], case['weights_y'], R.CV_SIGMAS[1], **R.fit_kwargs(case))
    assert np.array_equal(one['alpha'][0], got['alpha'][1]) and np.array_equal(one['w'][0], got['w'][1])


def test_restatement_folds_and_degenerate_rows():
    fold, L = R.fold_of_rows(np.array([True, False, True, True, True, False, True, True, True]), 3)
    assert L == 7 and list(fold) == [0, -1, 0, 0, 1, -1, 1, 2, 2]           # array_split: 3 + 2 + 2
    fold, L = R.fold_of_rows(np.array([True, True, False]), 5)              # fewer rows than folds: the last folds are empty
    assert L == 2 and list(fold) == [0, 1, -1]
    case = R.make_case(6)
    bad = np.full_like(case['x'], np.nan)                                   # no basis value is above 1e-64: L = 0
    got = R.kliep_fit_ref(bad, case['y'], None, None, 1.0, fold=3, **R.fit_kwargs(case))
    assert got['lcv'][0] == np.inf and np.all(np.isnan(got['alpha']))
    assert got['iters'][0] == case['max_iter'] - 1                          # a NaN never ends the loop early


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib, kliep

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    rs = np.random.RandomState(0)
    x, y = rs.randn(40, 3), rs.randn(30, 3)
    for kw in (dict(n=41), dict(n=0), dict(sigma=None), dict(sigma=0.0), dict(sigma=[1.0, -1.0]), dict(sigma=np.inf),
               dict(sigma=[1.0] * (kliep.MAX_SCALES + 1)), dict(sigma=[]), dict(fold=-1), dict(fold=kliep.MAX_FOLDS + 1),
               dict(max_iter=0), dict(conv_check_interval=0), dict(weights_x=np.ones(39)), dict(weights_y=np.ones(31))):
        with pytest.raises(ValueError):
            elfi_amd.kliep_fit(x, y, **dict(dict(sigma=1.0, n=10), **kw))
    with pytest.raises(ValueError):
        elfi_amd.kliep_fit(np.zeros((300, 2)), y[:, :2], sigma=1.0, n=kliep.MAX_BASIS + 1)
    with pytest.raises(ValueError):
        elfi_amd.kliep_fit(x, rs.randn(30, 2), sigma=1.0, n=10)
    with pytest.raises(ValueError):
        elfi_amd.kliep_fit(np.zeros((40, kliep.MAX_DIM + 1)), np.zeros((30, kliep.MAX_DIM + 1)), sigma=1.0, n=10)
    with pytest.raises(ValueError):
        elfi_amd.kliep_fit(np.zeros((kliep.MAX_ROWS + 1, 1)), y[:, :1], sigma=1.0, n=10)
    for args in ((x, x[:10], np.ones(9), 1.0), (x[:, :2], x[:10], np.ones(10), 1.0), (x, x[:10], np.ones(10), 0.0),
                 (x, x[:10], np.ones(10), np.nan)):
        with pytest.raises(ValueError):
            elfi_amd.kliep_ratio(*args)


def test_class_factory_requires_elfi(monkeypatch):
    import elfi_amd
    for name in [m for m in sys.modules if m == 'elfi' or m.startswith('elfi.')]:
        monkeypatch.delitem(sys.modules, name)
    with pytest.raises(ImportError):
        elfi_amd.hip_density_ratio_class()
    with pytest.raises(ImportError):
        elfi_amd.HipDensityRatioEstimation(n=10)


def test_class_keeps_the_reference_checks(monkeypatch):
    """The reference's ValueErrors, with its texts, before any device call; a float sigma switches optimize off."""
    ref_shim = pytest.importorskip('ref_shim')
    if not ref_shim.available():
        pytest.skip('no reference package')
    ref_shim.install()
    import elfi  # noqa: F401
    import elfi_amd
    from elfi.methods.density_ratio_estimation import DensityRatioEstimation
    from elfi_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    cls = elfi_amd.hip_density_ratio_class()
    assert issubclass(cls, DensityRatioEstimation) and cls is elfi_amd.hip_density_ratio_class()
    assert cls.__name__ == 'HipDensityRatioEstimation'
    rs = np.random.RandomState(1)
    x, y = rs.randn(20, 2), rs.randn(25, 2)
    for make, kw in ((dict(n=21), dict(sigma=1.0)), (dict(n=10), dict()), (dict(n=10, optimize=True), dict(sigma=1)),
                     (dict(n=10, optimize=True), dict())):
        mine, theirs = elfi_amd.HipDensityRatioEstimation(**make), DensityRatioEstimation(**make)
        with pytest.raises(ValueError) as e_ref:
            theirs.fit(x, y, **kw)
        with pytest.raises(ValueError) as e_mine:
            mine.fit(x, y, **kw)
        assert str(e_mine.value) == str(e_ref.value)
        assert (mine.x_len, mine.y_len) == (20, 25)
    est = elfi_amd.HipDensityRatioEstimation(n=10, optimize=True, fold=3)
    assert (est.n, est.epsilon, est.max_iter, est.abs_tol, est.conv_check_interval, est.fold, est.sigma, est.optimize) == \
        (10, 0.1, 500, 0.01, 20, 3, None, True)
    with pytest.raises(AssertionError, match='device context'):          # everything was accepted: the device is next
        est.fit(x, y, weights_x=np.arange(1.0, 21.0), sigma=2.5)
    assert est.sigma == 2.5 and est.optimize is False
    assert np.array_equal(est.theta, x[:10]) and np.isclose(est.weights_x.sum(), 1.0) and est.weights_y.shape == (25,)
    assert np.allclose(est.x0, np.average(x, axis=0, weights=np.arange(1.0, 21.0)))
