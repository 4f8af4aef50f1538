"""CPU: the NumPy statement of the logistic-regression ratio estimate (tests/logratio_ref.py) against the fixture recorded
from the reference's classifier (tests/golden/logratio.npz, scripts/make_golden_logratio.py), and the argument handling
and class plumbing of the Python mirrors (elfi_amd/logratio.py, elfi_amd/bolfire.py), which happen before any device call.

The yardstick of the GPU tests is `truth` (the reference's tight fit polished in 40-digit arithmetic).  A device value must
lie within 16 x max(e_tight over the recorded cases with the same number of summaries m), e_tight = |ref_tight - truth|,
with the floor 16 eps (1 + |truth|): `bound_for`, the rule of tests/test_semibsl.py.
"""
import os
import sys

import numpy as np
import pytest

import logratio_ref as R

ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle')
sys.path.insert(0, ORACLE)
import ref_shim  # noqa: E402

needs_reference = pytest.mark.skipif(not ref_shim.available(), reason='no reference package (run oracle/make_ref.sh)')


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'logratio.npz'))


def bound_for(gold, m, key='e_tight', truth=0.0):
    """16 x the largest recorded value of the reference (its error e_tight, or its violation kkt_tight) over every case
    with m summaries; never below 16 eps (1 + |truth|), what the number format gives."""
    worst = max(gold[key][i] for i, c in enumerate(R.CASES) if c[3] == m)
    return max(16.0 * worst, 16.0 * R.EPS * (1.0 + np.max(np.abs(truth))))


def truth_vector(gold, ci):
    m = R.CASES[ci][3]
    return np.concatenate([gold['truth_coef'][ci, :m], [gold['truth_intercept'][ci]]])


def test_fixture_matches_the_recipe(gold):
    assert np.array_equal(gold['cases'], np.array(R.CASES, dtype=float))
    shapes = [(c[1], c[3], c[4], c[5]) for c in R.CASES]
    for want in [(5, 8, 0.3, 1), (10, 2, 0.5, 1), (33, 7, 0.2, 1), (100, 16, 0.05, 0.05), (257, 63, 0.2, 1), (64, 3, 3.0, 1),
                 (20, 4, 6.0, 1), (1000, 32, 0.1, 1)]:
        assert want in shapes
    ms = [c[3] for c in R.CASES]
    assert 64 in ms and 1 in ms and any(c[1] != c[2] for c in R.CASES)
    for key in ('e_tight', 'kkt_tight', 'e_default'):
        assert np.all(np.isfinite(gold[key])), key
    assert np.all(gold['e_tight'] < 1e-9) and np.all(gold['kkt_tight'] < 1e-8)
    # the generator's two conditions: no zero coordinate at the edge of the threshold, one support
    assert np.all(gold['slack'] <= 1 - 1e-3)
    for ci, c in enumerate(R.CASES):
        m = c[3]
        tight = np.concatenate([gold['ref_tight_coef'][ci, :m], [gold['ref_tight_intercept'][ci]]])
        sup = np.concatenate([gold['support'][ci, :m], [gold['support'][ci, 64]]])
        assert np.array_equal(tight != 0, sup), ci
        assert np.array_equal(truth_vector(gold, ci) != 0, sup), ci
    X, M, _, _ = R.make_case(R.CONSTANT_COLUMN[0])
    mean, scale = R.scaler(X, M)
    assert scale[R.CONSTANT_COLUMN[1]] == 1.0 and mean[R.CONSTANT_COLUMN[1]] == R.CONSTANT_COLUMN[2]
    assert not gold['support'][R.CONSTANT_COLUMN[0], R.CONSTANT_COLUMN[1]]
    assert not gold['support'][3].any() and gold['truth_logratio'][3] == 0.0       # the all-zero solution


@pytest.mark.parametrize('ci', range(len(R.CASES)))
def test_restatement_is_stationary_at_truth(gold, ci):
    """The violation of `truth` by the NumPy statement is at rounding level: truth is rounded to double (eps |v| per
    coordinate, through a Hessian of norm <= C N max|z|^2 / 4) and the gradient is a sum of N terms of size <= C max|z|."""
    X, M, obs, C = R.make_case(ci)
    Z, y = R.design(X, M)
    v = truth_vector(gold, ci)
    N, zmax = len(Z), np.abs(Z).max()
    bound = R.EPS * C * N * zmax * (2.0 + 0.25 * zmax * np.abs(v).sum())
    got = R.violation(v, Z, y, C)
    print('case %d: violation of truth %.2e (bound %.2e), kkt_tight %.2e' % (ci, got, bound, gold['kkt_tight'][ci]))
    assert got <= bound
    mean, scale = R.scaler(X, M)
    lr = R.log_ratio_at(v, obs, mean, scale)[0]
    assert abs(lr - gold['truth_logratio'][ci]) <= 16 * R.EPS * (1 + np.abs(v) @ np.abs(np.append((obs[0] - mean) / scale, 1)))


@pytest.mark.parametrize('ci', [0, 1, 2, 3, 5, 6, 9, 10, 11])
def test_numpy_solver_reaches_truth(gold, ci):
    X, M, obs, C = R.make_case(ci)
    v, n_iter, ok = R.fit(X, M, C, tol=1e-13)
    t = truth_vector(gold, ci)
    assert ok and np.array_equal(v != 0, t != 0)
    assert np.abs(v - t).max() <= bound_for(gold, R.CASES[ci][3], truth=t)


def test_config_errors():
    from elfi_amd.logratio import DEFAULT_MAX_ITER, resolve_config
    assert resolve_config(None) == dict(C=1.0, tol=None, max_iter=DEFAULT_MAX_ITER)
    assert resolve_config({'penalty': 'l1', 'solver': 'liblinear', 'tol': 1e-12, 'max_iter': 100000, 'C': 2}) == \
        dict(C=2.0, tol=1e-12, max_iter=100000)
    assert resolve_config({'penalty': 'l1', 'solver': 'liblinear', 'fit_intercept': True, 'intercept_scaling': 1,
                           'class_weight': None})['C'] == 1.0
    base = {'penalty': 'l1', 'solver': 'liblinear'}
    for extra, word in [({'penalty': 'l2'}, 'penalty'), ({'solver': 'saga'}, 'solver'),
                        ({'class_weight': 'balanced'}, 'class_weight'), ({'fit_intercept': False}, 'fit_intercept'),
                        ({'intercept_scaling': 2.0}, 'intercept_scaling'), ({'dual': True}, 'dual'),
                        ({'random_state': 1}, 'random_state')]:
        with pytest.raises(ValueError, match=word):
            resolve_config(dict(base, **extra))
    with pytest.raises(ValueError, match='penalty'):
        resolve_config({'C': 2.0})


def test_log_ratio_argument_errors():
    import elfi_amd
    X, M, y = np.zeros((6, 3)), np.zeros((4, 3)), np.zeros(3)
    with pytest.raises(ValueError, match='divide'):
        elfi_amd.log_ratio(X, M, y, n_groups=4)
    with pytest.raises(ValueError, match='columns'):
        elfi_amd.log_ratio(X, np.zeros((4, 2)), y)
    with pytest.raises(ValueError, match='columns'):
        elfi_amd.log_ratio(X, M, np.zeros((1, 4)))
    with pytest.raises(ValueError, match='1 to 64'):
        elfi_amd.log_ratio(np.zeros((6, 65)), np.zeros((4, 65)), np.zeros(65))
    with pytest.raises(ValueError, match='class_min'):
        elfi_amd.log_ratio(X, M, y, class_min=1.0)
    with pytest.raises(ValueError, match='C must'):
        elfi_amd.log_ratio(X, M, y, C=0.0)
    with pytest.raises(ValueError, match='tol'):
        elfi_amd.log_ratio(X, M, y, tol=-1.0)


@needs_reference
def test_class_plumbing_without_a_device():
    elfi = ref_shim.install()
    import elfi_amd
    from elfi.methods.classifier import Classifier
    clf = elfi_amd.HipLogisticRegression()
    assert isinstance(clf, Classifier) and type(clf) is elfi_amd.hip_logistic_regression_class()
    assert type(clf).__name__ == 'HipLogisticRegression'
    assert clf.config == {'penalty': 'l1', 'solver': 'liblinear'} and clf.class_min == 0
    with pytest.raises(TypeError, match='class_min'):
        elfi_amd.HipLogisticRegression(class_min='0')
    with pytest.raises(ValueError, match='penalty'):
        elfi_amd.HipLogisticRegression(config={'penalty': 'l2', 'solver': 'liblinear'})
    with pytest.raises(ValueError, match='labels'):
        clf.fit(np.zeros((4, 2)), np.array([1, 1, 0, -1]))
    with pytest.raises(ValueError, match='labels'):
        clf.fit(np.zeros((4, 2)), np.ones(4))
    with pytest.raises(RuntimeError, match='fit first'):
        elfi_amd.HipLogisticRegression().predict_log_likelihood_ratio(np.zeros((1, 2)))
    # rows split by label, each label's rows in the order given
    X = np.arange(12.0).reshape(6, 2)
    clf.fit(X, np.array([1, -1, 1, -1, -1, 1]))
    assert np.array_equal(clf._rows[0], X[[0, 2, 5]]) and np.array_equal(clf._rows[1], X[[1, 3, 4]])
    # the reference's BOLFIRE accepts the classifier, the device GP and the device acquisition; the subclass builds them
    from elfi.examples import ma2
    m = ma2.get_model(seed_obs=4)
    bounds = {'t1': (-2, 2), 't2': (-1, 1)}
    ref = elfi.BOLFIRE(m, 10, feature_names=['S1', 'S2'], classifier=clf, bounds=bounds, seed=1, seed_marginal=3,
                       target_model=elfi_amd.HipGPRegression(m.parameter_names, bounds=bounds))
    assert ref.classifier is clf
    hip = elfi_amd.HipBOLFIRE(m, 10, feature_names=['S1', 'S2'], bounds=bounds, seed=1, seed_marginal=3,
                              acq_noise_var=0.1)
    assert isinstance(hip, elfi.BOLFIRE) and type(hip) is elfi_amd.hip_bolfire_class()
    assert isinstance(hip.target_model, elfi_amd.HipGPRegression)
    assert type(hip.classifier) is elfi_amd.hip_logistic_regression_class()
    acq = hip.acquisition_method
    assert isinstance(acq, elfi_amd.HipLCBSC) and acq.prior is hip.prior and acq.noise_var == 0.1
    assert acq.exploration_rate == 10 and acq.seed == 1 and acq.additive_cost.scale == -1
    x = np.array([[0.5, 0.2]])
    assert np.array_equal(np.ravel(acq.additive_cost.evaluate(x)), -hip.prior.logpdf(x))
    own = elfi_amd.HipLCBSC(hip.target_model, seed=5)
    assert elfi_amd.HipBOLFIRE(m, 10, feature_names=['S1', 'S2'], bounds=bounds, acquisition_method=own,
                               classifier=clf).acquisition_method is own
    assert np.array_equal(hip.marginal, ref.marginal)           # the same seed_marginal, the same marginal rows
    with pytest.raises(TypeError, match='fitted'):
        elfi_amd.HipBOLFIREPosterior(['t1', 't2'], hip.target_model, hip.prior, [])
