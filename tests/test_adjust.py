"""CPU: the yardstick of the device regression adjustment (tests/adjust_ref.py, tests/golden/adjust.npz recorded by
scripts/make_golden_adjust.py) and the argument handling of the Python side (elfi_amd/adjust.py), which happens before
any device call.

Yardstick: `truth` is the least-squares solution in 40-digit arithmetic on the same float inputs; a value must lie within
16 x max(e_ref over the recorded cases with the same m), e_ref = |reference - truth| in the metrics of adjust_ref, and the
bound is never below 16 eps.  The recorded cases keep e_ref <= 1e-10 and a condition number <= 1e6, so that the bound says
something.
"""
import os

import numpy as np
import pytest

import adjust_ref as R
import ref_shim

needs_reference = pytest.mark.skipif(not ref_shim.available(), reason='no reference package (run oracle/make_ref.sh)')


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'adjust.npz'))


def test_recorded_reference_meets_the_yardstick_conditions(gold):
    assert np.array_equal(gold['cases'], np.array([c[:4] for c in R.CASES]))
    assert list(gold['kinds']) == [c[4] for c in R.CASES]
    assert [tuple(c[1:4]) for c in R.CASES] == [(3, 1, 1), (66, 64, 2), (255, 3, 1), (256, 2, 2), (257, 8, 3), (513, 2, 2),
                                                (1000, 33, 5), (700, 16, 16)]
    for ci, (seed, n, m, q, kind) in enumerate(R.CASES):
        tc, ta = gold['truth_coef_%d' % ci], gold['truth_adj_%d' % ci]
        assert tc.shape == (q, m) and ta.shape == (n, q) and np.all(np.isfinite(tc)) and np.all(np.isfinite(ta))
        e_coef, e_adj = R.coef_error(gold['ref_coef_%d' % ci], tc), R.adjusted_error(gold['ref_adj_%d' % ci], ta)
        assert e_coef == gold['e_coef'][ci] and e_adj == gold['e_adj'][ci]
        assert e_coef <= R.MAX_E_REF and e_adj <= R.MAX_E_REF and gold['cond'][ci] <= R.MAX_COND
        assert R.bound(gold['e_coef'][R.same_m(m)]) <= 16 * R.MAX_E_REF
    n = R.GAUSS_RUN['n_samples']
    assert gold['gauss_mu'].shape == gold['gauss_ref_adjusted'].shape == gold['gauss_discrepancies'].shape == (n,)
    assert gold['gauss_summaries'].shape == (n, 2) and gold['gauss_observed'].shape == (2,)
    assert np.all(np.diff(gold['gauss_discrepancies']) >= 0)            # a Rejection sample is ordered by discrepancy
    assert float(gold['gauss_e_adj']) <= R.MAX_E_REF


@pytest.mark.parametrize('ci', range(len(R.CASES)))
def test_recipe_regenerates_the_recorded_inputs(gold, ci):
    seed, n, m, q, kind = R.CASES[ci]
    X, Y = R.make_case(ci)
    assert X.shape == (n, m) and Y.shape == (n, q)
    assert R.checksum(ci) == gold['crc'][ci]
    assert abs(R.condition_number(X) - gold['cond'][ci]) <= 1e-6 * gold['cond'][ci]
    if kind == 'scales':
        assert np.ptp(np.log10(np.std(X, axis=0))) > 5.9
    if kind == 'offset':
        assert np.all(np.abs(X.mean(axis=0)) > 9e3 * X.std(axis=0))


@pytest.mark.parametrize('ci', range(len(R.CASES)))
def test_statement_lies_within_the_bound(gold, ci):
    """The NumPy statement (LAPACK least squares on the centred columns) against the truth: the metric and the bound at
    work without a GPU."""
    m = R.CASES[ci][2]
    X, Y = R.make_case(ci)
    adj, coef, icpt, rss = R.lstsq_adjust(X, Y)
    same = R.same_m(m)
    e_coef, e_adj = R.coef_error(coef, gold['truth_coef_%d' % ci]), R.adjusted_error(adj, gold['truth_adj_%d' % ci])
    print('case %d coefficients: e_ref %.2e statement %.2e bound %.2e | adjusted: e_ref %.2e statement %.2e bound %.2e'
          % (ci, gold['e_coef'][ci], e_coef, R.bound(gold['e_coef'][same]), gold['e_adj'][ci], e_adj,
             R.bound(gold['e_adj'][same])))
    assert e_coef <= R.bound(gold['e_coef'][same]) and e_adj <= R.bound(gold['e_adj'][same])


@needs_reference
@pytest.mark.parametrize('ci', range(len(R.CASES)))
def test_recorded_reference_values_are_reproduced(gold, ci):
    ref_shim.install()
    from elfi.methods import post_processing as mod
    m = R.CASES[ci][2]
    X, Y = R.make_case(ci)
    coef, adj = R.reference_adjust(mod, X, Y)
    same = R.same_m(m)
    # the same library on another machine may sum in another order: within the yardstick's bound of the record
    assert R.coef_error(coef, gold['ref_coef_%d' % ci]) <= R.bound(gold['e_coef'][same])
    assert R.adjusted_error(adj, gold['ref_adj_%d' % ci]) <= R.bound(gold['e_adj'][same])


@needs_reference
def test_recorded_gauss_run_is_the_references_adjustment(gold):
    ref_shim.install()
    from elfi.methods import post_processing as mod
    sample, model = R.gauss_sample(mod, gold)
    adj = mod.adjust_posterior(sample, model, list(R.GAUSS_RUN['summaries']), ['mu'], mod.LinearAdjustment())
    assert R.adjusted_error(adj.outputs['mu'], gold['gauss_ref_adjusted']) <= 16 * R.EPS


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    rs = np.random.RandomState(0)
    X, Y = rs.randn(40, 3), rs.randn(40, 2)
    for kw in (dict(n_groups=3), dict(n_groups=0), dict(prefixes=[10, 5, 40]), dict(prefixes=[10, 10, 40]),
               dict(prefixes=[1, 40]), dict(prefixes=[10, 30]), dict(prefixes=[10.5, 40]), dict(prefixes=[])):
        with pytest.raises(ValueError):
            elfi_amd.linear_adjust(X, Y, **kw)
    for a, b in ((rs.randn(40, 65), Y), (X, rs.randn(40, 17)), (X, rs.randn(39, 2)), (rs.randn(1, 3), rs.randn(1, 2)),
                 (np.empty((0, 3)), np.empty((0, 2))), (rs.randn(40), Y), (rs.randn(2, 20, 3), rs.randn(4, 10, 2))):
        with pytest.raises(ValueError):
            elfi_amd.linear_adjust(a, b)
    # keyword arguments of the regression model: named in the message, checked before the reference's class is looked for
    with pytest.raises(ValueError, match='positive'):
        elfi_amd.HipLinearAdjustment(positive=True)
    with pytest.raises(ValueError, match='fit_intercept'):
        elfi_amd.HipLinearAdjustment(fit_intercept=False)
    with pytest.raises(ValueError, match='n_jobs'):
        elfi_amd.HipLinearAdjustment(fit_intercept=True, n_jobs=2)
    # n_closest: before the sample is looked at
    for bad in ([250, 100, 500], [100, 100], [1, 100], [], [100.5, 200]):
        with pytest.raises(ValueError, match='n_closest'):
            elfi_amd.adjust_posterior(None, None, ['s'], n_closest=bad)
    # an adjustment object of another kind would run on the host

    class RegressionAdjustment:
        def fit(self, **kw):
            raise AssertionError('a foreign adjustment was fitted')
    with pytest.raises(TypeError, match='RegressionAdjustment'):
        elfi_amd.adjust_posterior(None, None, ['s'], adjustment=RegressionAdjustment())
    with pytest.raises(ValueError, match='quadratic'):
        elfi_amd.adjust_posterior(None, None, ['s'], adjustment='quadratic')


@needs_reference
def test_class_keeps_the_references_parts(gold, monkeypatch):
    import elfi_amd
    from elfi_amd import _lib
    ref_shim.install()
    from elfi.methods import post_processing as mod
    cls = elfi_amd.hip_linear_adjustment_class()
    assert cls is elfi_amd.hip_linear_adjustment_class() and issubclass(cls, mod.LinearAdjustment)
    for name in ('_input_variables', '_get_finite', '_check_fitted'):
        assert getattr(cls, name) is getattr(mod.LinearAdjustment, name)
    adj = elfi_amd.HipLinearAdjustment(fit_intercept=True)
    assert isinstance(adj, mod.RegressionAdjustment) and adj._name == 'LinearAdjustment'
    with pytest.raises(ValueError, match='fitted first'):
        adj.parameter_names
    with pytest.raises(TypeError):
        elfi_amd.adjust_posterior(None, None, ['s'], adjustment=mod.LinearAdjustment())
    # a sample that is not all-finite cannot take nested thresholds; refused before the device is asked for
    monkeypatch.setattr(_lib, 'default_context', lambda *a, **k: (_ for _ in ()).throw(AssertionError('device')))
    sample, model = R.gauss_sample(mod, gold)
    sample.outputs['ss_var'] = sample.outputs['ss_var'].copy()
    sample.outputs['ss_var'][5] = np.nan
    with pytest.raises(ValueError, match='all-finite'):
        elfi_amd.adjust_posterior(sample, model, list(R.GAUSS_RUN['summaries']), ['mu'], n_closest=[100, 500])
    with pytest.raises(ValueError, match='rows'):
        elfi_amd.adjust_posterior(R.gauss_sample(mod, gold)[0], model, list(R.GAUSS_RUN['summaries']), ['mu'],
                                  n_closest=[100, 501])
